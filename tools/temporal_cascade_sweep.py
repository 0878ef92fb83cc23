#!/usr/bin/env python3
"""What carrying the firefly cascade's layers through the temporal merge buys on a moving camera, without a GPU: the CPU oracle
renders the same bits as the device, and the numpy restatements (tests/temporal_restate.py, tests/cascade_restate.py,
tests/temporal_cascade_restate.py) are the merge, the cascade and the merge of its layers.

C2 (Cornell box, Optix7Gui rule) at 160x90 over the orbit of tools/temporal_sweep.py: FRAMES frames STEP of a turn apart, SPP samples
each, frame f seeded as iterations f SPP .. f SPP + SPP - 1 (what twk_set_sample_offset does on the device). The oracle keeps running
means, not samples: sample k is recovered in float64 as (k + 1) mean_k - k mean_{k-1} and rounded to f32, as tools/cascade_sweep.py
does it (exact enough for a sweep; no bit test uses it), across the camera changes too. Every frame's samples are folded into fresh
layers (cascade_restate.fold from iteration 0), its geometry AOV is Oracle.traceRays on temporal_restate.centre_rays, and the frames
are merged in order: colour and moments by temporal_restate.restate_temporal, the layers by restate_temporal_cascade, both with
maxHistory 32 and positionTolerance 0.1 (the tolerance of tests/test_gpu_temporal.py at this size: a pixel of a 90-row picture is
0.013 of the distance wide, the default 0.01 is chosen at 1080 rows).

The reference is 512 spp from the last camera that shares no sample with the orbit: iterations FRAMES SPP .. FRAMES SPP + 511 rendered
on top of the orbit's running mean and separated from it in float64.

Prints, for the last frame, relative RMSE / per-pixel relative RMSE (tests/test_gpu_denoise.py::_errors) of: the frame's own mean, the
resolve of its own layers, the merged plain colour, the resolve of the merged layers — for kappa in KAPPAS — and each of them as the
beauty of twk_denoise_variance_sampled's restatement at its defaults (moments: the frame's own beside the frame's pictures, the merged
ones beside the merged pictures).
usage: python tools/temporal_cascade_sweep.py [--cache renders.npz] [--threads n] [--no-denoiser] > table.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RES = (160, 90)
FRAMES, SPP, STEP, REFERENCE_SPP = 8, 4, 0.002, 512
MAX_HISTORY, TOLERANCE = 32, 0.1
KAPPAS = (8, 16, 32)
CASCADE = (6, 1.0, 8.0)


def cameras(twk, app):
    i = app.info
    return [twk.camera_frustum(tuple(i.center), i.phi + STEP * frame, i.theta, i.fov, i.distance, RES[0] / RES[1]) for frame in range(FRAMES)]


def renders(threads):
    """means [FRAMES * SPP, H, W, 4] of the orbit, geometry [FRAMES, H, W, 4], cameras [FRAMES, 12], the last frame's albedo and
    normal, and the disjoint 512 spp reference."""
    import tweeker_raytracer_amd as twk
    from oracle import orc
    from temporal_restate import F, U32, camera_array, centre_rays
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    ref = orc.Oracle(miss=app.info.miss)
    ref.loadApplication(app)
    ref.setShaderVariant(1)
    ref.enableAov(True)
    width, height = RES
    epsilon = app.state.epsilonFactor * F(1.0e-7)
    means, geometry, cams, aov = [], [], [], {}
    for frame, cam in enumerate(cameras(twk, app)):
        ref.initCameras([cam])
        cams.append(camera_array(cam))
        P, d = centre_rays(cam, width, height)
        rays = np.empty((height, width, 8), F)
        rays[..., 0:3], rays[..., 3], rays[..., 4:7], rays[..., 7] = P, F(epsilon), d, F(1.0e27)
        tbg, ids = ref.traceRays(rays)
        t, inst = tbg[:, 0].reshape(height, width), ids[:, 0].reshape(height, width)
        g = np.zeros((height, width, 4), F)
        for k in range(3):
            g[..., k] = P[k] + t * d[..., k]
        g[..., 3] = (inst + 1).astype(U32).view(F)
        g[inst < 0] = 0
        geometry.append(g)
        for it in range(frame * SPP, (frame + 1) * SPP):
            ref.render(it, threads=threads)
            means.append(ref.getOutputBufferHost().copy())
            if it in (FRAMES * SPP - SPP - 1, FRAMES * SPP - 1):
                aov[it] = (ref.readAov(0).astype(np.float64), ref.readAov(1).astype(np.float64))
    n0 = FRAMES * SPP
    for it in range(n0, n0 + REFERENCE_SPP):  # the last camera; separated from the orbit's mean below
        ref.render(it, threads=threads)
    total = ref.getOutputBufferHost().astype(np.float64)
    reference = ((n0 + REFERENCE_SPP) * total - n0 * means[-1].astype(np.float64)) / REFERENCE_SPP
    last = lambda which: (((n0) * aov[n0 - 1][which] - (n0 - SPP) * aov[n0 - SPP - 1][which]) / SPP).astype(np.float32)
    return dict(means=np.stack(means), geometry=np.stack(geometry), cameras=np.stack(cams), albedo=last(0), normal=last(1), reference=reference.astype(np.float32))


def frame_samples(means, frame):
    """[SPP, H, W, 4] f32 samples of frame `frame` (w = 1), recovered from consecutive running means."""
    m = means[..., :3].astype(np.float64)
    s = np.ones((SPP,) + means.shape[1:3] + (4,), np.float32)
    for j in range(SPP):
        k = frame * SPP + j
        s[j, ..., :3] = m[0] if k == 0 else (k + 1) * m[k] - k * m[k - 1]
    return s


def frame_moments(samples):
    """(mean, M2, n, 0) of the luminance of the frame's samples, in float64, rounded to f32 (tools/denoise_sampled_sweep.py moments_of)."""
    s = samples[..., :3].astype(np.float64)
    l = (0.2126 * s[..., 0] + 0.7152 * s[..., 1]) + 0.0722 * s[..., 2]
    out = np.zeros(samples.shape[1:3] + (4,), np.float32)
    mean = l.mean(axis=0)
    out[..., 0], out[..., 1], out[..., 2] = mean, ((l - mean) ** 2).sum(axis=0), samples.shape[0]
    return out


def orbit(r, b):
    """The last frame's own (colour, moments, layers) and the merged (colour, moments, layers) after the whole orbit."""
    import cascade_restate
    from temporal_cascade_restate import restate_temporal_cascade
    from temporal_restate import restate_temporal
    history = None
    for frame in range(FRAMES):
        samples = frame_samples(r["means"], frame)
        colour = np.ones(samples.shape[1:], np.float32)
        colour[..., :3] = samples[..., :3].astype(np.float64).mean(axis=0)
        moments = frame_moments(samples)
        layers = cascade_restate.fold(samples, 0, np.zeros((len(b),) + samples.shape[1:], np.float32), b)
        g = r["geometry"][frame]
        if history is None:
            merged = (colour, moments, layers)
        else:
            hc, hm, hl, hg, cam = history
            mc, mm, _ = restate_temporal(colour, moments, g, (hc, hm, hg), cam, MAX_HISTORY, TOLERANCE)
            ml, took = restate_temporal_cascade(layers, g, (hl, hg), cam, MAX_HISTORY, TOLERANCE)
            merged = (mc, mm, ml)
        history = merged + (g, r["cameras"][frame])
    return (colour, moments, layers), merged, took


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--no-denoiser", action="store_true", help="leave out the columns through twk_denoise_variance_sampled's restatement")
    args = ap.parse_args()
    if args.cache and os.path.exists(args.cache):
        r = dict(np.load(args.cache))
    else:
        r = renders(args.threads)
        if args.cache:
            np.savez(args.cache, **r)
    import cascade_restate
    import tweeker_raytracer_amd as twk
    from test_gpu_denoise import _errors
    b = cascade_restate.thresholds(*CASCADE)
    (colour, moments, layers), (merged_colour, merged_moments, merged_layers), took = orbit(r, b)
    reference = r["reference"]
    fmt = lambda e: f"{e[0]:.3f} / {e[1]:.3f}"
    denoise = None
    if not args.no_denoiser:
        from oracle import orc
        import test_gpu_denoise_sampled as S
        import test_gpu_denoise_variance as V
        from test_gpu_denoise import _exp
        L = twk._lib
        dn, dv, exp, sqrt = L.Denoiser(), L.DenoiserVariance(), _exp(orc), V._sqrt(orc)
        denoise = lambda beauty, m: S.restate_sampled(beauty, r["albedo"], r["normal"], m, L.TWK_DENOISER_MIN_SAMPLES, dn, dv, exp, sqrt)[0]
    n = merged_layers[0, ..., 3]
    print(f"C2 {RES[0]}x{RES[1]}, Optix7Gui rule, an orbit of {FRAMES} frames {STEP} of a turn apart, {SPP} spp per frame seeded as iterations {SPP} x frame ...; "
          f"maxHistory {MAX_HISTORY}, positionTolerance {TOLERANCE}; cascade {CASCADE[0]} layers, start {CASCADE[1]:g}, base {CASCADE[2]:g}.")
    print(f"The last frame against {REFERENCE_SPP} spp from its camera that share no sample with the orbit: relative RMSE / per-pixel relative RMSE. "
          f"{took.mean():.3f} of the pixels took history in the last merge; mean merged n {n.mean():.1f}.\n")
    head = "| picture | as it is |" + ("" if denoise is None else " -> twk_denoise_variance_sampled |")
    print(head)
    print("|---|---|" + ("" if denoise is None else "---|"))

    def row(name, picture, m):
        cells = [fmt(_errors(picture, reference))]
        if denoise is not None:
            cells.append(fmt(_errors(denoise(picture, m), reference)))
        print(f"| {name} | " + " | ".join(cells) + " |")
        return _errors(picture, reference)

    own = row(f"the last frame's own {SPP} spp, plain mean", colour, moments)
    plain = row("merged plain colour (twk_temporal_accumulate)", merged_colour, merged_moments)
    verdict = []
    for kappa in KAPPAS:
        a = row(f"resolve of the last frame's own layers, kappa {kappa}", cascade_restate.resolve(layers, b, kappa), moments)
        m = row(f"resolve of the merged layers, kappa {kappa}", cascade_restate.resolve(merged_layers, b, kappa), merged_moments)
        verdict.append((kappa, m[1] < a[1] and m[1] < plain[1], m[1], a[1], plain[1]))
    print()
    for kappa, holds, m, a, p in verdict:
        print(f"kappa {kappa}: per-pixel relative RMSE of the resolve of the merged layers {m:.4f} against the resolve of the frame's own layers {a:.4f} and the merged plain colour {p:.4f}: "
              + ("strictly below both" if holds else "NOT below both"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
