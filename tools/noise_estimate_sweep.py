#!/usr/bin/env python3
"""How far to trust twk_estimate_noise: its estimate beside the true error, without a GPU. The CPU oracle renders the same bits as
the device, and tests/noise_restate.py is the estimator.

C2 (Cornell box, Optix7Gui rule) at 160x90 and 4, 16 and 64 spp: the estimated relative standard error e of every pixel's
luminance mean (mean and 0.95 quantile edge of the summary, as twk_noise_mean and twk_noise_quantile return them) beside the TRUE
relative error of the same pixels against 512 spp, |lum(picture) - lum(reference)| / (lum(reference) + darkFloor): its mean, its
root mean square (what e estimates is a standard deviation: for a Gaussian error the mean absolute error is 0.80 of it) and its
0.95 quantile. The per-sample pictures are obtained as tools/denoise_sampled_sweep.py obtains them: the oracle keeps running
means, sample k is recovered in float64 as (k + 1) mean_k - k mean_{k-1}, and the luminance moments are Welford's over those,
rounded to f32 (exact enough for a sweep; no bit test uses it). The 512 spp reference has an error of its own, about
sqrt(spp / 512) of the picture's: 0.09, 0.18 and 0.35 of it at 4, 16 and 64 spp, which the true columns contain.
Nothing is asserted. Prints a markdown table.
usage: python tools/noise_estimate_sweep.py [--cache renders.npz] [--threads n] > table.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SPP = (4, 16, 64)
DARK_FLOOR = 0.01


def luminance(rgb):
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache")
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    import denoise_sampled_sweep as D
    import noise_restate as nr
    if args.cache and os.path.exists(args.cache):
        r = dict(np.load(args.cache))
    else:
        r = D.renders(args.threads)
        if args.cache:
            np.savez(args.cache, **r)
    reference = luminance(r["beauty512"][..., :3].astype(np.float64)).reshape(-1)
    print(f"C2 {D.RES[0]}x{D.RES[1]}, Optix7Gui rule: the estimate (minSamples 4, darkFloor {DARK_FLOOR:g}) beside the true relative error of the luminance against 512 spp\n")
    print("| input | valid pixels | estimated mean e | estimated 0.95 quantile (bin edge) | true mean | true RMS | true 0.95 quantile | estimated mean / true RMS |")
    print("|---|---|---|---|---|---|---|---|")
    for spp in SPP:
        moments = D.moments_of(r["means"], spp).reshape(-1, 4)
        s, emap = nr.summary(moments, 4, DARK_FLOOR)
        valid = emap >= 0
        picture = luminance(r[f"beauty{spp}"][..., :3].astype(np.float64)).reshape(-1)
        true = (np.abs(picture - reference) / (reference + DARK_FLOOR))[valid]
        rms = float(np.sqrt((true ** 2).mean()))
        print(f"| {spp} spp | {s['valid']} of {moments.shape[0]} | {float(nr.mean(s)):.4f} | {float(nr.quantile(s, 0.95)):.4f} | {true.mean():.4f} | {rms:.4f} | "
              f"{np.quantile(true, 0.95):.4f} | {float(nr.mean(s)) / rms:.2f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
