#!/usr/bin/env python3
"""Measures the geometry guide of the denoiser (twk_denoise_geometry) against the three modes without it, and picks the default
sigmaPosition, without a GPU: the CPU oracle renders the same bits as the device and has the AOVs, and the numpy restatements
(tests/denoise_geometry_restate.py, tests/test_gpu_denoise*.py) are the filters.

C2 (Cornell box, Optix7Gui rule) at 160x90: 4, 16 and 64 spp filtered against 512 spp, in the two measures of
tests/test_gpu_denoise.py::test_it_denoises (relative RMSE / per-pixel relative RMSE), over the whole picture and restricted to a
band of BAND pixels around the silhouettes of the scene's two objects, the mirror and the glass sphere (from the instance ids:
where an object's pixel has a neighbour of another instance; the objects are the instances that are not one of the box's quads) —
where the guide acts. The oracle has no geometry AOV: the one used here is traced in numpy float64 through the
pixel centres of camera 0 against the application's triangles (Moeller-Trumbore, closest hit) and rounded to f32 — the device's
up to rounding, exact enough for a sweep; no bit test uses it. Luminance moments as in tools/denoise_sampled_sweep.py.

The rule for the default: over sigmaPosition in SIGMAS and instanceStop 0 / 1, the pair with the smallest sum, over the three modes
and the three sample counts, of the band's per-pixel relative RMSE, among the pairs whose whole-picture measures are no worse than
the unguided mode's in any cell; ties go to the larger sigma and to instanceStop 0 (the weaker stop). Prints markdown.
usage: python tools/denoise_geometry_sweep.py [--cache renders.npz] [--threads n] > table.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from denoise_sampled_sweep import RES, SPP, moments_of, renders  # noqa: E402  (tools/ is this script's directory)

SIGMAS = (0.002, 0.005, 0.01, 0.02, 0.05)
BAND = 3
MIN_SAMPLES = 4


def trace_geometry(app):
    """(geometry float32 [H, W, 4] = (world position, bits of instance + 1), camera as 12 floats, ids of the object instances)."""
    width, height = RES
    cam = app.cameras[0]
    P, U, V, W = (np.array(list(v), np.float64) for v in (cam.P, cam.U, cam.V, cam.W))
    ndc_x = ((np.arange(width) + 0.5) / width * 2 - 1)[None, :, None]
    ndc_y = ((np.arange(height) + 0.5) / height * 2 - 1)[:, None, None]
    d = (U * ndc_x + V * ndc_y + W).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    best_t = np.full(d.shape[0], np.inf)
    best_id = np.zeros(d.shape[0], np.uint32)
    objects = []
    for i, (g, transform, _, _) in enumerate(app.instances):
        attr, idx = app.geometry(g)
        if idx.size > 6:  # not one of the box's quads: the scene's two spheres
            objects.append(i + 1)
        m = transform.astype(np.float64).reshape(3, 4)
        v = attr[:, :3].astype(np.float64) @ m[:, :3].T + m[:, 3]
        tri = v[idx.reshape(-1, 3)]
        for c in range(0, tri.shape[0], 256):
            a, e1, e2 = tri[c:c + 256, 0], tri[c:c + 256, 1] - tri[c:c + 256, 0], tri[c:c + 256, 2] - tri[c:c + 256, 0]
            pv = np.cross(d[:, None, :], e2[None])
            det = (pv * e1[None]).sum(-1)
            with np.errstate(all="ignore"):
                inv = 1.0 / det
                tv = P - a
                u = (pv * tv[None]).sum(-1) * inv
                qv = np.cross(tv, e1)
                w = (d[:, None, :] * qv[None]).sum(-1) * inv
                t = (qv * e2).sum(-1)[None] * inv
            ok = (np.abs(det) > 1e-12) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 1e-6)
            t = np.where(ok, t, np.inf)
            k = t.argmin(axis=1)
            tk = t[np.arange(t.shape[0]), k]
            closer = tk < best_t
            best_t = np.where(closer, tk, best_t)
            best_id = np.where(closer, np.uint32(i + 1), best_id)
    hit = np.isfinite(best_t)
    geometry = np.zeros((height, width, 4), np.float32)
    position = P + d * np.where(hit, best_t, 0.0)[:, None]
    geometry[..., :3] = np.where(hit[:, None], position, 0.0).reshape(height, width, 3)
    geometry[..., 3] = np.where(hit, best_id, 0).astype(np.uint32).reshape(height, width).view(np.float32)
    return geometry, np.concatenate([P, U, V, W]).astype(np.float32), objects


def silhouette_band(geometry, objects):
    ids = geometry[..., 3].view(np.uint32)
    inside = np.isin(ids, objects)
    edge = np.zeros(ids.shape, bool)
    for dy, dx in ((0, 1), (1, 0)):
        a, b = ids[: ids.shape[0] - dy, : ids.shape[1] - dx], ids[dy:, dx:]
        differs = (a != b) & (inside[: ids.shape[0] - dy, : ids.shape[1] - dx] | inside[dy:, dx:])
        edge[: ids.shape[0] - dy, : ids.shape[1] - dx] |= differs
        edge[dy:, dx:] |= differs
    band = np.zeros_like(edge)
    ys, xs = np.nonzero(edge)
    for y, x in zip(ys, xs):
        band[max(0, y - BAND): y + BAND + 1, max(0, x - BAND): x + BAND + 1] = True
    return band


def errors(x, r, mask=None):
    x, r = x[..., :3].astype(np.float64), r[..., :3].astype(np.float64)
    if mask is not None:
        x, r = x[mask], r[mask]
    return np.sqrt(((x - r) ** 2).sum() / (r ** 2).sum()), np.sqrt(np.mean((x - r) ** 2 / (r ** 2 + 0.01)))


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
    from denoise_geometry_restate import restate
    from test_gpu_denoise import _exp, _restate
    L = twk._lib
    exp, sqrt = _exp(orc), V._sqrt(orc)
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    geometry, camera, objects = trace_geometry(app)
    band = silhouette_band(geometry, objects)
    reference = r["beauty512"]
    dn, dv = L.Denoiser(), L.DenoiserVariance()
    fmt = lambda e: f"{e[0]:.3f} / {e[1]:.3f}"
    hits = geometry[..., 3].view(np.uint32) != 0
    print(f"C2 {RES[0]}x{RES[1]}, Optix7Gui rule, against 512 spp: relative RMSE / per-pixel relative RMSE, whole picture and [band]; every filter at its "
          f"defaults (3 levels); {hits.mean() * 100:.0f} % of the pixels are hits, the band ({BAND} px around the silhouettes of instances {objects}) holds {band.sum()} of {band.size} pixels\n")
    modes = ("plain", "variance", "sampled")
    pairs = [(s, stop) for s in SIGMAS for stop in (0, 1)]
    print("| input | mode | unfiltered | without the guide | " + " | ".join(f"sigma {s:g}, stop {stop}" for s, stop in pairs) + " |")
    print("|---|---|---|---|" + "---|" * len(pairs))
    score = {p: 0.0 for p in pairs}
    admissible = {p: True for p in pairs}
    for spp in SPP:
        guides = (r[f"beauty{spp}"], r[f"albedo{spp}"], r[f"normal{spp}"])
        moments = moments_of(r["means"], spp)
        for mode in modes:
            if mode == "plain":
                base = _restate(*guides, dn, exp)[0]
                kw = {}
            elif mode == "variance":
                base = V.restate_variance(*guides, dn, dv, exp, sqrt)[0]
                kw = dict(dv=dv)
            else:
                n = min(MIN_SAMPLES, spp)
                base = S.restate_sampled(*guides, moments, n, dn, dv, exp, sqrt)[0]
                kw = dict(dv=dv, moments=moments, min_samples=n)
            whole, inband = errors(base, reference), errors(base, reference, band)
            cells = []
            for p in pairs:
                dg = L.DenoiserGeometry(sigmaPosition=p[0], instanceStop=p[1])
                out = restate(*guides, geometry, camera, dn, dg, exp, sqrt, **kw)[0]
                e, eb = errors(out, reference), errors(out, reference, band)
                score[p] += eb[1]
                if e[0] > whole[0] or e[1] > whole[1]:
                    admissible[p] = False
                cells.append(f"{fmt(e)} [{fmt(eb)}]")
            noisy = f"{fmt(errors(guides[0], reference))} [{fmt(errors(guides[0], reference, band))}]"
            print(f"| {spp} spp | {mode} | {noisy} | {fmt(whole)} [{fmt(inband)}] | " + " | ".join(cells) + " |")
    print("\nsum over the nine cells of the band's per-pixel relative RMSE (admissible: whole-picture measures no worse than without the guide in every cell):\n")
    for p in pairs:
        print(f"- sigma {p[0]:g}, stop {p[1]}: {score[p]:.3f}{'' if admissible[p] else ' (not admissible)'}")
    candidates = [p for p in pairs if admissible[p]] or pairs
    best = min(candidates, key=lambda p: (round(score[p], 3), -p[0], p[1]))
    edge = " — an edge of the range: provisional" if best[0] in (SIGMAS[0], SIGMAS[-1]) else ""
    print(f"\nthe rule picks sigmaPosition {best[0]:g}, instanceStop {best[1]}{edge}" + ("" if any(admissible.values()) else " (no pair is admissible: the whole-picture measures do not improve everywhere)"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
