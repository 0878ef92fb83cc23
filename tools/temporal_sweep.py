#!/usr/bin/env python3
"""What twk_temporal_accumulate buys on a moving camera, and what it and the geometry pass cost (GPU box).

Quality: the Cornell box over an orbit of FRAMES frames, SPP samples per pixel each, the sample offset advancing by SPP per frame
(twk_set_sample_offset), every frame merged into the history by the own-buffer form. The last frame is compared with a 512 spp
render from its camera in the two measures of tests/test_gpu_denoise.py (relative RMSE, per-pixel relative RMSE): the merged colour
on its own and fed through twk_denoise_variance_sampled with the merged moments, for every maxHistory x positionTolerance of the
sweep, beside the rows to beat — the last frame's own SPP samples, and those through twk_denoise_variance_sampled alone. The share
of pixels of the last frame that took history is printed per row.

Cost: twk_render_geometry and twk_temporal_accumulate at the same resolution, wall clock of N calls + one synchronisation after a
warm-up, the temporal kernel beside the floor of its compulsory bytes (three current and three history streams read once, three
outputs written) at the stream-copy rate twk_stream_peak_gbps reports in the same process.
usage (GPU box): python tools/temporal_sweep.py [width height] > profiles/rNN_temporal.md"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, SPP, STEP, REFERENCE_SPP = 8, 4, 0.002, 512
MAX_HISTORY = (8, 16, 32, 64)
TOLERANCE = (0.002, 0.005, 0.01, 0.02, 0.05)


def errors(x, r):
    x, r = x[..., :3].astype(np.float64), r[..., :3].astype(np.float64)
    return np.sqrt(((x - r) ** 2).sum() / (r ** 2).sum()), np.sqrt(np.mean((x - r) ** 2 / (r ** 2 + 0.01)))


def main():
    import tweeker_raytracer_amd as twk
    L = twk._lib
    res = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*res)
    i = app.info
    camera = lambda frame: twk.camera_frustum(tuple(i.center), i.phi + STEP * frame, i.theta, i.fov, i.distance, res[0] / res[1])
    dev = twk.Device(ordinal=0, miss=i.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableAov(True)
    dev.updateCamera(0, camera(FRAMES - 1))
    for it in range(REFERENCE_SPP):
        dev.render(it)
    reference = dev.getOutputBufferHost()
    dev.enableMoments(True)
    dev.enableGeometry(True)
    shape = (res[1], res[0])

    def orbit(tp):
        dev.temporalReset()
        for frame in range(FRAMES):
            dev.updateCamera(0, camera(frame))
            dev.setSampleOffset(frame * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.temporalAccumulate(tp)

    print(f"Cornell box, {res[0]}x{res[1]}, an orbit of {FRAMES} frames {STEP} of a turn apart, {SPP} spp per frame, sample offset {SPP} x frame; the last frame against {REFERENCE_SPP} spp from its camera.")
    print("Measures: relative RMSE / per-pixel relative RMSE (tests/test_gpu_denoise.py _errors). Filter: twk_denoise_variance_sampled at its defaults.\n")
    orbit(L.Temporal())
    noisy = dev.getOutputBufferHost()
    dev.denoise(minSamples=L.TWK_DENOISER_MIN_SAMPLES)
    alone = dev.readDenoised()
    print("| input | filter | relative RMSE | per-pixel relative RMSE |")
    print("|---|---|---|---|")
    print("| the last frame's {} spp (to beat) | none | {:.4f} | {:.4f} |".format(SPP, *errors(noisy, reference)))
    print("| the last frame's {} spp (to beat) | twk_denoise_variance_sampled | {:.4f} | {:.4f} |\n".format(SPP, *errors(alone, reference)))
    albedo, normal = dev.readAov(0), dev.readAov(1)
    hip = L.C.CDLL("libamdhip64.so")
    guide = []
    for a in (albedo, normal):
        p = L.C.c_void_p()
        assert hip.hipMalloc(L.C.byref(p), L.C.c_size_t(a.nbytes)) == 0 and hip.hipMemcpy(p, a.ctypes.data_as(L.C.c_void_p), L.C.c_size_t(a.nbytes), 1) == 0
        guide.append(p)
    print("| maxHistory | positionTolerance | share with history | mean n | merged | merged + filter |")
    print("|---|---|---|---|---|---|")
    for max_history in MAX_HISTORY:
        for tolerance in TOLERANCE:
            orbit(L.Temporal(maxHistory=max_history, positionTolerance=tolerance))
            merged, n = dev.readTemporal(), dev.readTemporalMoments()[..., 2]
            colour, _, moments, _ = dev.temporalDevicePointers()
            dev.denoise(beauty=colour, albedo=guide[0].value, normal=guide[1].value, shape=shape, moments=moments, minSamples=L.TWK_DENOISER_MIN_SAMPLES)
            both = dev.readDenoised(shape=shape)
            e, f = errors(merged, reference), errors(both, reference)
            print(f"| {max_history} | {tolerance} | {(n > SPP).mean():.3f} | {n.mean():.1f} | {e[0]:.4f} / {e[1]:.4f} | {f[0]:.4f} / {f[1]:.4f} |")
    for p in guide:
        hip.hipFree(p)

    calls = 100
    peak = dev.streamPeakGBps(1 << 30, 10)
    orbit(L.Temporal())

    def timed(call):
        for _ in range(5):
            call()
        dev.synchronizeStream()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        dev.synchronizeStream()
        return (time.perf_counter() - t0) * 1e3 / calls

    pixels = res[0] * res[1]
    print(f"\nCost at {res[0]}x{res[1]}, {calls} calls + 1 sync after 5 warm-up calls; stream peak {peak:.0f} GB/s (twk_stream_peak_gbps, 1 GiB x 10).\n")
    print("| format | twk_render_geometry ms | twk_temporal_accumulate ms (kernel + the geometry's copy) | compulsory bytes | floor ms | ms / floor |")
    print("|---|---|---|---|---|---|")
    for fmt, name, px in ((0, "RGBA32F", 16), (1, "RGBA16F", 8)):
        dev.setOutputFormat(fmt)
        for it in range(SPP):
            dev.render(it)
        dev.renderGeometry()
        dev.temporalAccumulate()
        dev.temporalAccumulate()
        geometry_ms = timed(dev.renderGeometry)
        temporal_ms = timed(dev.temporalAccumulate)
        compulsory = pixels * ((px + 16 + 16) + 48 + (px + 16 + 16))  # current, history, outputs
        floor = compulsory / (peak * 1e9) * 1e3
        print(f"| {name} | {geometry_ms:.3f} | {temporal_ms:.3f} | {compulsory / 1e6:.0f} MB | {floor:.3f} | {temporal_ms / floor:.2f} |")
    print(f"\n(the own-buffer form also copies the frame's geometry into the kept history: {pixels * 32 / 1e6:.0f} MB more, read and written, inside the time above and outside the floor)")
    dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
