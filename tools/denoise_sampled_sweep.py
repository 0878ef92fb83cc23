#!/usr/bin/env python3
"""Measures twk_denoise_variance_sampled against twk_denoise_variance, twk_denoise and the unfiltered picture, and chooses the
default minSamples, without a GPU: the CPU oracle renders the same bits as the device and has the AOVs, and the numpy restatements
of the filters (tests/test_gpu_denoise_sampled.py::restate_sampled, tests/test_gpu_denoise_variance.py::restate_variance,
tests/test_gpu_denoise.py::_restate) are the filters.

C2 (Cornell box, Optix7Gui rule) at 160x90: 4, 16 and 64 spp filtered against 512 spp, in the two measures of
tests/test_gpu_denoise.py::test_it_denoises (relative RMSE / per-pixel relative RMSE). The oracle keeps running means, not samples:
sample k is recovered in float64 as (k + 1) mean_k - k mean_{k-1} (exact enough for a sweep; no bit test uses it), and the
luminance moments are Welford's over those, in float64, rounded to f32. Prints a markdown table.
usage: python tools/denoise_sampled_sweep.py [--cache renders.npz] [--threads n] > table.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = (160, 90)
SPP = (4, 16, 64)
MIN_SAMPLES = (2, 4, 8, 16)


def renders(threads):
    import tweeker_raytracer_amd as twk
    from oracle import orc
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    ref = orc.Oracle(miss=app.info.miss)
    ref.loadApplication(app)
    ref.setShaderVariant(1)
    ref.enableAov(True)
    out, means = {}, []
    for it in range(512):
        ref.render(it, threads=threads)
        if it < max(SPP):
            means.append(ref.getOutputBufferHost().copy())
        if it + 1 in SPP + (512,):
            out[f"beauty{it + 1}"] = ref.getOutputBufferHost().copy()
            out[f"albedo{it + 1}"] = ref.readAov(0).copy()
            out[f"normal{it + 1}"] = ref.readAov(1).copy()
    out["means"] = np.stack(means)
    return out


def moments_of(means, spp):
    """(mean, M2, n, 0) of the luminance of samples 0 .. spp - 1, recovered from consecutive running means."""
    m = means[:spp, ..., :3].astype(np.float64)
    k = np.arange(spp, dtype=np.float64).reshape(-1, 1, 1, 1)
    samples = m.copy()
    samples[1:] = (k[1:] + 1) * m[1:] - k[1:] * m[:-1]
    l = (0.2126 * samples[..., 0] + 0.7152 * samples[..., 1]) + 0.0722 * samples[..., 2]
    out = np.zeros(means.shape[1:3] + (4,), np.float32)
    mean = l.mean(axis=0)
    out[..., 0], out[..., 1], out[..., 2] = mean, ((l - mean) ** 2).sum(axis=0), spp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache")
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    if args.cache and os.path.exists(args.cache):
        r = dict(np.load(args.cache))
    else:
        r = renders(args.threads)
        if args.cache:
            np.savez(args.cache, **r)
    import tweeker_raytracer_amd as twk
    from oracle import orc
    import test_gpu_denoise_sampled as S
    import test_gpu_denoise_variance as V
    from test_gpu_denoise import _errors, _exp, _restate
    L = twk._lib
    exp, sqrt = _exp(orc), V._sqrt(orc)
    reference = r["beauty512"]
    dn, dv = L.Denoiser(), L.DenoiserVariance()
    fmt = lambda e: f"{e[0]:.3f} / {e[1]:.3f}"
    print(f"C2 {RES[0]}x{RES[1]}, Optix7Gui rule, against 512 spp: relative RMSE / per-pixel relative RMSE; every filter at its defaults "
          f"(3 levels, k {dv.fireflyThreshold:g}, sigmaLuminance {dv.sigmaLuminance:g})\n")
    print("| input | unfiltered | twk_denoise | twk_denoise_variance | " + " | ".join(f"sampled, minSamples {n}" for n in MIN_SAMPLES) + " |")
    print("|---|---|---|---|" + "---|" * len(MIN_SAMPLES))
    wins = {n: [] for n in MIN_SAMPLES}
    for spp in SPP:
        guides = (r[f"beauty{spp}"], r[f"albedo{spp}"], r[f"normal{spp}"])
        moments = moments_of(r["means"], spp)
        spatial = _errors(V.restate_variance(*guides, dn, dv, exp, sqrt)[0], reference)
        cells = []
        for n in MIN_SAMPLES:
            e = _errors(S.restate_sampled(*guides, moments, n, dn, dv, exp, sqrt)[0], reference) if n <= spp else spatial  # n > spp: every pixel falls back
            wins[n].append(e[0] < spatial[0] and e[1] < spatial[1])
            cells.append(fmt(e) + (" (= spatial)" if n > spp else ""))
        print(f"| {spp} spp | {fmt(_errors(guides[0], reference))} | {fmt(_errors(_restate(*guides, dn, exp)[0], reference))} | {fmt(spatial)} | " + " | ".join(cells) + " |")
    print("\nstrictly below twk_denoise_variance in both measures: " + "; ".join(f"minSamples {n}: " + (", ".join(f"{s} spp" for s, w in zip(SPP, wins[n]) if w) or "nowhere") for n in MIN_SAMPLES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
