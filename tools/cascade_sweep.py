#!/usr/bin/env python3
"""Measures the firefly cascade's resolve (twk_cascade_resolve) against the plain mean and chooses the default kappa, without a GPU:
the CPU oracle renders the same bits as the device, and the numpy restatement tests/cascade_restate.py is the cascade.

C2 (Cornell box, Optix7Gui rule) at 160x90: 4, 16 and 64 spp against 512 spp, in the two measures of
tests/test_gpu_denoise.py::_errors (relative RMSE / per-pixel relative RMSE); the plain mean against the resolve for kappa in
1 .. 32 and (layers, start, base) in (6, 1, 8), (8, 1, 4); and each of them through twk_denoise_variance_sampled's restatement as
its beauty (guides and moments: the frame's own). The oracle keeps running means, not samples: sample k is recovered in float64 as
(k + 1) mean_k - k mean_{k-1} and rounded to f32 (exact enough for a sweep; no bit test uses it).

The rule for the default kappa: the value with the lowest per-pixel relative RMSE at 16 spp among those whose relative RMSE at
64 spp is not above the plain mean's. Prints a markdown table and the choice.
usage: python tools/cascade_sweep.py [--cache renders.npz] [--threads n] > table.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KAPPAS = (1, 2, 4, 8, 16, 32)
CASCADES = ((6, 1.0, 8.0), (8, 1.0, 4.0))


def samples_of(means, spp):
    """[spp, H, W, 4] f32 samples 0 .. spp - 1 (w = 1), recovered from consecutive running means."""
    m = means[:spp, ..., :3].astype(np.float64)
    k = np.arange(spp, dtype=np.float64).reshape(-1, 1, 1, 1)
    s = np.ones(m.shape[:3] + (4,), np.float32)
    s[0, ..., :3] = m[0]
    s[1:, ..., :3] = (k[1:] + 1) * m[1:] - k[1:] * m[:-1]
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--no-denoiser", action="store_true", help="leave out the columns through twk_denoise_variance_sampled's restatement")
    args = ap.parse_args()
    import denoise_sampled_sweep as D
    if args.cache and os.path.exists(args.cache):
        r = dict(np.load(args.cache))
    else:
        r = D.renders(args.threads)
        if args.cache:
            np.savez(args.cache, **r)
    import cascade_restate as restate
    import tweeker_raytracer_amd as twk
    from test_gpu_denoise import _errors
    reference = r["beauty512"]
    fmt = lambda e: f"{e[0]:.3f} / {e[1]:.3f}"
    denoise = None
    if not args.no_denoiser:
        from oracle import orc
        import test_gpu_denoise_sampled as S
        import test_gpu_denoise_variance as V
        from test_gpu_denoise import _exp
        L = twk._lib
        dn, dv, exp, sqrt = L.Denoiser(), L.DenoiserVariance(), _exp(orc), V._sqrt(orc)
        denoise = lambda beauty, spp: S.restate_sampled(beauty, r[f"albedo{spp}"], r[f"normal{spp}"], D.moments_of(r["means"], spp), L.TWK_DENOISER_MIN_SAMPLES, dn, dv, exp, sqrt)[0]
    print(f"C2 {D.RES[0]}x{D.RES[1]}, Optix7Gui rule, against 512 spp: relative RMSE / per-pixel relative RMSE"
          + ("" if denoise is None else "; `-> filtered`: the picture as the beauty of twk_denoise_variance_sampled at its defaults") + "\n")
    print("| cascade | spp | plain mean | " + " | ".join(f"kappa {k}" for k in KAPPAS) + " |")
    print("|---|---|---|" + "---|" * len(KAPPAS))
    table = {}
    for cascade in CASCADES:
        b = restate.thresholds(*cascade)
        for spp in D.SPP:
            samples = samples_of(r["means"], spp)
            layers = restate.fold(samples, 0, np.zeros((len(b),) + samples.shape[1:], np.float32), b)
            plain = _errors(r[f"beauty{spp}"], reference)
            cells, filtered = [], []
            for kappa in KAPPAS:
                resolved = restate.resolve(layers, b, kappa)
                table[(cascade, spp, kappa)] = _errors(resolved, reference)
                cells.append(fmt(table[(cascade, spp, kappa)]))
                if denoise is not None:
                    filtered.append(fmt(_errors(denoise(resolved, spp), reference)))
            table[(cascade, spp, None)] = plain
            name = f"{cascade[0]} layers, start {cascade[1]:g}, base {cascade[2]:g}"
            print(f"| {name} | {spp} | {fmt(plain)} | " + " | ".join(cells) + " |")
            if denoise is not None:
                print(f"| {name} -> filtered | {spp} | {fmt(_errors(denoise(r[f'beauty{spp}'], spp), reference))} | " + " | ".join(filtered) + " |")
    print()
    for cascade in CASCADES:
        allowed = [k for k in KAPPAS if table[(cascade, 64, k)][0] <= table[(cascade, 64, None)][0]]
        name = f"{cascade[0]} layers, start {cascade[1]:g}, base {cascade[2]:g}"
        if not allowed:
            print(f"{name}: no kappa keeps the relative RMSE at 64 spp at or below the plain mean's {table[(cascade, 64, None)][0]:.4f}")
            continue
        best = min(allowed, key=lambda k: table[(cascade, 16, k)][1])
        print(f"{name}: kappa with relative RMSE at 64 spp not above the plain mean's: {allowed}; lowest per-pixel relative RMSE at 16 spp among them: "
              f"kappa {best} ({table[(cascade, 16, best)][1]:.4f} against the plain mean's {table[(cascade, 16, None)][1]:.4f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
