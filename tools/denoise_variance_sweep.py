#!/usr/bin/env python3
"""Chooses the defaults of twk_denoise_variance (fireflyThreshold, sigmaLuminance, the epsilon of the luminance edge-stop) without a
GPU: the CPU oracle renders the same bits as the device and has the AOVs, and the numpy restatement of the filter
(tests/test_gpu_denoise_variance.py::restate_variance, tests/test_gpu_denoise.py::_restate) is the filter.

C2 (Cornell box, Optix7Gui rule) at 160x90: 4 spp and 16 spp filtered against 512 spp, in the two measures of
tests/test_gpu_denoise.py::test_it_denoises (relative RMSE / per-pixel relative RMSE). Prints markdown tables.
usage: python tools/denoise_variance_sweep.py [--cache renders.npz] [--threads n] > table.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = (160, 90)


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
    out = {}
    for it in range(512):
        ref.render(it, threads=threads)
        if it + 1 in (4, 16, 512):
            out[f"beauty{it + 1}"] = ref.getOutputBufferHost().copy()
            out[f"albedo{it + 1}"] = ref.readAov(0).copy()
            out[f"normal{it + 1}"] = ref.readAov(1).copy()
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
    import test_gpu_denoise_variance as V
    from test_gpu_denoise import _errors, _exp, _restate
    L = twk._lib
    exp, sqrt = _exp(orc), V._sqrt(orc)
    reference = r["beauty512"]

    def plain(spp):
        return _errors(_restate(r[f"beauty{spp}"], r[f"albedo{spp}"], r[f"normal{spp}"], L.Denoiser(), exp)[0], reference)

    def guided(spp, k, sigma, eps, levels=3):
        V.EPSILON = np.float32(eps)
        return _errors(V.restate_variance(r[f"beauty{spp}"], r[f"albedo{spp}"], r[f"normal{spp}"], L.Denoiser(iterations=levels), L.DenoiserVariance(k, sigma), exp, sqrt)[0], reference)

    fmt = lambda e: f"{e[0]:.3f} / {e[1]:.3f}"
    print(f"C2 {RES[0]}x{RES[1]}, Optix7Gui rule, against 512 spp: relative RMSE / per-pixel relative RMSE\n")
    print("| input | unfiltered | twk_denoise (defaults) |")
    print("|---|---|---|")
    for spp in (4, 16):
        print(f"| {spp} spp | {fmt(_errors(r[f'beauty{spp}'], reference))} | {fmt(plain(spp))} |")
    for eps in (1e-3, 1e-2, 1e-1):
        sigmas = (1.0, 2.0, 4.0, 8.0, 16.0)
        print(f"\ntwk_denoise_variance, 4 spp, 3 levels, epsilon {eps:g}: rows fireflyThreshold k, columns sigmaLuminance\n")
        print("| k | " + " | ".join(f"{s:g}" for s in sigmas) + " |")
        print("|---|" + "---|" * len(sigmas))
        for k in (0.0, 1.0, 2.0, 3.0, 4.0, 6.0):
            print(f"| {k:g} | " + " | ".join(fmt(guided(4, k, s, eps)) for s in sigmas) + " |")
    dv = L.DenoiserVariance()
    print(f"\nthe defaults (k {dv.fireflyThreshold:g}, sigmaLuminance {dv.sigmaLuminance:g}, epsilon 1e-3) at 4 and 16 spp, 3 and 5 levels\n")
    print("| input | levels | twk_denoise_variance |")
    print("|---|---|---|")
    for spp in (4, 16):
        for levels in (3, 5):
            print(f"| {spp} spp | {levels} | {fmt(guided(spp, dv.fireflyThreshold, dv.sigmaLuminance, 1e-3, levels))} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
