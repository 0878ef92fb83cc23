#!/usr/bin/env python3
"""The planned adaptive loop beside the fixed-batch loop at equal total samples: C2 (Cornell box, Optix7Gui rule) at 320x180.

For each target (the 0.5, 0.75 and 0.9 quantile of the frame's own error map at 16 spp), after 16 uniform iterations:
  fixed    rounds of twk_adaptive_select + 8 samples on the selected pixels, until nothing is selected or 64 spp x pixels samples
           are spent (the loop of tools/adaptive_sweep.py); what it spends is the budget of the other loop
  planned  rounds of twk_adaptive_plan (the default batches) + twk_launch_adaptive_planned, until nothing is selected or that budget
           is spent; a plan that asks for more than is left gives every selected pixel the same share of the rest, as rtigo3_hip does
Both against a 512 spp reference that is seeded apart (twk_set_sample_offset 2^20). The measures of profiles/r13_adaptive.md:
  per-pixel relative RMSE  sqrt(mean(((L - Lref) / (Lref + 0.01))^2)), L the luminance of the picture
  0.95 quantile of e       twk_noise_quantile of the frame's own estimate (the upper edge of its bin)
  rounds                   select or plan calls that were followed by a pass
Nothing is asserted. Prints a markdown table.
usage (GPU box): python tools/adaptive_plan_sweep.py > table.md"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adaptive_sweep import BUDGET_SPP, DARK_FLOOR, FIRST, INTERVAL, REFERENCE_SPP, RES, device, luminance  # noqa: E402


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
        return float(np.sqrt((((L - reference) / (reference + DARK_FLOOR)) ** 2).mean())), s.quantile(0.95), s.mean

    def start():
        dev = device(twk, adaptive=True)
        for it in range(FIRST):
            dev.render(it)
        return dev

    probe = start()
    cls, e = nr.classify(probe.readMoments().reshape(-1, 4))
    targets = [float(np.quantile(e[cls == nr.VALID], q)) for q in (0.5, 0.75, 0.9)]
    probe.close()

    plan = twk.AdaptivePlan()
    print(f"C2 {RES[0]}x{RES[1]}, Optix7Gui rule, against {REFERENCE_SPP} spp seeded apart; {FIRST} uniform iterations, then fixed = select + {INTERVAL} samples per round, "
          f"at most {BUDGET_SPP} spp x pixels; planned = plan (minBatch {plan.minBatch}, maxBatch {plan.maxBatch}) + planned pass per round, at most what fixed spent\n")
    print("| target | loop | samples per pixel (mean, max) | rounds, last active share | per-pixel relative RMSE | 0.95 quantile of e | mean e |")
    print("|---|---|---|---|---|---|---|")
    for target in targets:
        ap = twk.Adaptive(targetNoise=target)
        dev = start()
        spent, rounds, share = FIRST * pixels, 0, 1.0
        while True:
            n = dev.adaptiveSelect(ap)
            share = n / pixels
            samples = min(INTERVAL, (BUDGET_SPP * pixels - spent) // n) if n else 0
            if samples == 0:
                break
            dev.renderAdaptive(samples)
            spent += n * samples
            rounds += 1
        f = errors(dev)
        print(f"| {target:.4f} | fixed | {spent / pixels:.2f}, {int(dev.readSampleCounts().max())} | {rounds}, {share:.4f} | {f[0]:.5f} | {f[1]:.5f} | {f[2]:.5f} |")
        dev.close()
        budget = spent
        dev = start()
        spent, rounds, share = FIRST * pixels, 0, 1.0
        while True:
            n, paths = dev.adaptivePlan(ap, plan)
            share = n / pixels
            if n and paths > budget - spent:
                each = min((budget - spent) // n, plan.maxBatch)
                n, paths = dev.adaptivePlan(ap, twk.AdaptivePlan(minBatch=each, maxBatch=each)) if each else (0, 0)
            if n == 0 or paths == 0 or paths > budget - spent:
                break
            dev.renderPlanned()
            spent += paths
            rounds += 1
        p = errors(dev)
        print(f"| {target:.4f} | planned | {spent / pixels:.2f}, {int(dev.readSampleCounts().max())} | {rounds}, {share:.4f} | {p[0]:.5f} | {p[1]:.5f} | {p[2]:.5f} |")
        dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
