#!/usr/bin/env python3
"""What adaptive sampling buys at an equal sample budget: C2 (Cornell box, Optix7Gui rule) at 320x180 on the device.

For each target (the 0.5, 0.75 and 0.9 quantile of the frame's own error map at 16 spp): an ADAPTIVE render — 16 uniform
iterations, then rounds of twk_adaptive_select + 8 samples on the selected pixels, until nothing is selected or 64 spp x pixels
samples are spent — and a UNIFORM render of as many samples, rounded up to whole iterations. Both against a 512 spp reference that
is seeded apart (twk_set_sample_offset 2^20), so that its error is independent of theirs (about sqrt(spp / 512) of theirs):
  relative RMSE            sqrt(mean((L - Lref)^2)) / mean(Lref), L the luminance of the picture
  per-pixel relative RMSE  sqrt(mean(((L - Lref) / (Lref + 0.01))^2)), the error the estimate is an estimate of
  0.95 quantile of e       twk_noise_quantile of the frame's own estimate (the upper edge of its bin)
Nothing is asserted. Prints a markdown table.
usage (GPU box): python tools/adaptive_sweep.py > table.md"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = (320, 180)
FIRST, INTERVAL, BUDGET_SPP, REFERENCE_SPP = 16, 8, 64, 512
DARK_FLOOR = 0.01


def luminance(rgb):
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


def device(twk, adaptive=False, offset=0):
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableMoments(True)
    if adaptive:
        dev.enableAdaptive(True)
    if offset:
        dev.setSampleOffset(offset)
    return dev


def main():
    import tweeker_raytracer_amd as twk
    import noise_restate as nr
    pixels = RES[0] * RES[1]
    ref = device(twk, offset=1 << 20)
    for it in range(REFERENCE_SPP):
        ref.render(it)
    reference = luminance(ref.getOutputBufferHost()[..., :3].astype(np.float64))
    ref.close()

    def errors(dev):
        L = luminance(dev.getOutputBufferHost()[..., :3].astype(np.float64))
        s = dev.estimateNoise()
        return (float(np.sqrt(((L - reference) ** 2).mean()) / reference.mean()), float(np.sqrt((((L - reference) / (reference + DARK_FLOOR)) ** 2).mean())),
                s.quantile(0.95), s.mean)

    probe = device(twk)
    for it in range(FIRST):
        probe.render(it)
    cls, e = nr.classify(probe.readMoments().reshape(-1, 4))
    targets = [float(np.quantile(e[cls == nr.VALID], q)) for q in (0.5, 0.75, 0.9)]
    probe.close()

    print(f"C2 {RES[0]}x{RES[1]}, Optix7Gui rule, against {REFERENCE_SPP} spp seeded apart; adaptive = {FIRST} uniform iterations, then select + {INTERVAL} samples per round, at most {BUDGET_SPP} spp x pixels\n")
    print("| target | render | samples per pixel (mean, max) | rounds, last active share | relative RMSE | per-pixel relative RMSE | 0.95 quantile of e | mean e |")
    print("|---|---|---|---|---|---|---|---|")
    for target in targets:
        dev = device(twk, adaptive=True)
        for it in range(FIRST):
            dev.render(it)
        spent, rounds, share = FIRST * pixels, 0, 1.0
        ap = twk.Adaptive(targetNoise=target)
        while True:
            n = dev.adaptiveSelect(ap)
            share = n / pixels
            samples = min(INTERVAL, (BUDGET_SPP * pixels - spent) // n) if n else 0
            if samples == 0:
                break
            dev.renderAdaptive(samples)
            spent += n * samples
            rounds += 1
        a = errors(dev)
        largest = int(dev.readSampleCounts().max())
        dev.close()
        spp = -(-spent // pixels)
        uni = device(twk)
        for it in range(spp):
            uni.render(it)
        u = errors(uni)
        uni.close()
        print(f"| {target:.4f} | adaptive | {spent / pixels:.2f}, {largest} | {rounds}, {share:.4f} | {a[0]:.5f} | {a[1]:.5f} | {a[2]:.5f} | {a[3]:.5f} |")
        print(f"| {target:.4f} | uniform | {spp}, {spp} | | {u[0]:.5f} | {u[1]:.5f} | {u[2]:.5f} | {u[3]:.5f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
