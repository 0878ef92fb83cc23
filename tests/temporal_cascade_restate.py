"""The cascade's layers through the temporal merge (csrc/temporal_cascade_device.h) restated statement for statement in numpy
float32, with a count per branch, and the synthetic layers the tests feed both sides. The projection, the footprint's taps and
the test of a tap's geometry are temporal_restate's (temporal_device.h temporalProject / temporalFootprint / temporalTapGeometry), the
thresholds and the luminance cascade_restate's. No test in here: tests/test_temporal_cascade_host.py (CPU) and tests/test_gpu_temporal_cascade.py use it."""
import numpy as np

import cascade_restate
import temporal_restate
from temporal_restate import F, U32, _finite3, footprint_taps, project

BRANCHES = ("miss", "geometry_not_finite", "current_n_below_1", "behind", "off_screen", "outside", "id_mismatch", "position", "history_n_below_1",
            "history_rejected_not_finite", "weight_zero", "no_tap", "capped", "uncapped", "history_sum_not_finite", "took")


def merge_cascade(layers, g, history, cam, max_history, tolerance, info=None, taps=None, trust=None):
    """temporalCascadePixel on float32 arrays: layers [K, H, W, 4] the current frame's, g [H, W, 4] its geometry; history = (layers
    [K, H, W, 4], geometry [H, W, 4]) or None; cam the history's camera; trust [H, W]: the trusted build, None: the plain one.
    Returns (merged layers, took, hn) — took: the pixels that merged history, every other pixel holds the input's bits; hn: the
    history's count after the cap and before the trust, 0 where nothing was taken. info (a dict) receives one count per branch of
    the definition; taps (a list) receives, per tap in the definition's order, (counted mask, weight, qy, qx)."""
    Lc, g = np.ascontiguousarray(layers, F), np.ascontiguousarray(g, F)
    K, height, width = Lc.shape[:3]
    assert 2 <= K <= cascade_restate.MAX_LAYERS and g.shape == (height, width, 4)
    out = Lc.copy()
    if history is None:
        return out, np.zeros((height, width), bool), np.zeros((height, width), F)
    Hl, hg = (np.ascontiguousarray(a, F) for a in history)
    assert Hl.shape == Lc.shape and hg.shape == g.shape
    max_h = F(max_history)
    nc, rc = Lc[0, ..., 3], Lc[K - 1, ..., 3]
    with np.errstate(all="ignore"):
        hit = g[..., 3].view(U32) != 0
        gfinite = _finite3(g)
        enough_now = np.isfinite(nc) & ~(nc < F(1.0))
        cand = hit & gfinite & enough_now
        fx, fy, vv, front, inside = project(g, cam, width, height)
        ok = cand & front & inside
        s = np.zeros((K, height, width, 3), F)
        sn, srej, ws = (np.zeros((height, width), F) for _ in range(3))
        carried = np.zeros((height, width), bool)
        counts = dict(outside=0, id_mismatch=0, position=0, history_n_below_1=0, history_rejected_not_finite=0, weight_zero=0)
        for w, q, inpic, same, near in footprint_taps(g, hg, fx, fy, vv, ok, tolerance):
            hq = Hl[(slice(None),) + q]
            hn_q, hrej_q = hq[0, ..., 3], hq[K - 1, ..., 3]
            enough = np.isfinite(hn_q) & (hn_q >= F(1.0))
            rejected_finite = np.isfinite(hrej_q)
            positive = w > F(0.0)
            belongs = ok & inpic & same & near
            counted = belongs & enough & rejected_finite & positive
            s = np.where(counted[None, ..., None], s + w[None, ..., None] * hq[..., :3], s)
            sn = np.where(counted, sn + w * hn_q, sn)
            srej = np.where(counted, srej + w * hrej_q, srej)
            ws = np.where(counted, ws + w, ws)
            carried |= counted & ~np.isfinite(hq[..., :3]).all(axis=(0, -1))
            counts["outside"] += int((ok & ~inpic).sum())
            counts["id_mismatch"] += int((ok & inpic & ~same).sum())
            counts["position"] += int((ok & inpic & same & ~near).sum())
            counts["history_n_below_1"] += int((belongs & ~enough).sum())
            counts["history_rejected_not_finite"] += int((belongs & enough & ~rejected_finite).sum())
            counts["weight_zero"] += int((belongs & enough & rejected_finite & ~positive).sum())
            if taps is not None:
                taps.append((counted, w) + q)
        took = ws > F(0.0)
        h = s / ws[None, ..., None]
        hn, hrej = sn / ws, srej / ws
        capped = hn > max_h
        f = max_h / hn
        h = np.where(capped[None, ..., None], h * f[None, ..., None], h)
        hrej = np.where(capped, hrej * f, hrej)
        hn = np.where(capped, max_h, hn)
        hn_capped = hn
        if trust is not None:
            t = np.ascontiguousarray(trust, F).reshape(height, width)
            h, hrej, hn = h * t[None, ..., None], hrej * t, hn * t
        merged = np.zeros_like(Lc)
        merged[..., :3] = h + Lc[..., :3]
        merged[0, ..., 3] = hn + nc
        merged[K - 1, ..., 3] = hrej + rc
    assert merged.dtype == F
    out[:, took] = merged[:, took]
    if info is not None:
        info.update(counts)
        info.update(miss=int((~hit).sum()), geometry_not_finite=int((hit & ~gfinite).sum()), current_n_below_1=int((hit & gfinite & ~enough_now).sum()),
                    behind=int((cand & ~front).sum()), off_screen=int((cand & front & ~inside).sum()), no_tap=int((ok & ~took).sum()),
                    capped=int((took & capped).sum()), uncapped=int((took & ~capped).sum()), history_sum_not_finite=int((took & carried).sum()), took=int(took.sum()))
    return out, took, np.where(took, hn_capped, F(0.0)).astype(F)


def restate_temporal_cascade(layers, g, history, cam, max_history, tolerance, info=None, taps=None, trust=None):
    """twk_temporal_accumulate_cascade (trust [H, W]: twk_temporal_accumulate_cascade_trusted) on float32 arrays, merge_cascade's
    arguments. Returns (merged layers, took)."""
    return merge_cascade(layers, g, history, cam, max_history, tolerance, info, taps, trust)[:2]


# ---- synthetic frames and layers ---------------------------------------------------------------------------------------------------
MAX_HISTORY, TOLERANCE = 32, 0.06  # temporal_restate.synthetic_frames' own
_SPECIALS = 56                     # pixels temporal_restate.synthetic_frames plants its special values in


def synthetic_geometry(width, height, seed=0):
    """(current geometry, history geometry, history camera) of temporal_restate.synthetic_frames: its two cameras in front of its
    wall with the id edge, the depth step and the misses, and — where the picture has room for them — its planted points behind the
    previous camera and positions that are not finite. A picture of fewer than its 56 special pixels (1x1, 5x3) gets the same cameras
    and wall without the planted values (synthetic_frames itself cannot be called at such a size)."""
    if width * height > _SPECIALS:
        (_, _, g), (_, _, hg), cam_prev, max_history, tolerance = temporal_restate.synthetic_frames(width, height, seed)
        assert (max_history, tolerance) == (MAX_HISTORY, TOLERANCE)
        return g, hg, cam_prev
    aspect = width / height
    fov = 2.0 * np.degrees(np.arctan(0.05 * height / 3.0))
    cam_prev = temporal_restate.look_at((-0.25, 0.03, 3.0), (0.0, 0.0, 0.0), fov, aspect)
    cam_now = temporal_restate.look_at((0.2, 0.01, 2.9), (0.05, 0.0, 0.0), fov, aspect)
    top = 0.03 * height
    return temporal_restate._plane_geometry(cam_now, width, height, top), temporal_restate._plane_geometry(cam_prev, width, height, top), cam_prev


def _next_float(x, steps):
    """The float32 `steps` representable values away from x (positive x)."""
    return (np.array([x], F).view(np.int32) + np.int32(steps)).view(F)[0]


def _on_a_pixel_centre(g, hg, cam, width, height, pixel, q):
    """Moves the surface point of `pixel` onto history pixel q's so that its projection's fx is EXACTLY an integer (tx = 0: the taps at
    dx = 1 have weight exactly 0): the history's own point at q, its x stepped through neighbouring floats until the float32
    arithmetic of temporalProject lands on the integer. False: none within the search."""
    base = hg[q].copy()
    if base.view(U32)[3] == 0 or not np.isfinite(base[:3]).all() or base[0] <= 0:
        return False
    for step in sorted(range(-400, 401), key=abs):
        trial = base.copy()
        trial[0] = _next_float(base[0], step)
        fx, fy, _, front, inside = project(trial[None, :], cam, width, height)
        if front[0] and inside[0] and fx[0] == np.floor(fx[0]) and fx[0] >= 0:
            g[pixel] = trial
            return True
    return False


def synthetic_layers(width, height, K, seed=0, clean=False):
    """(current layers, current geometry, (history layers, history geometry), history camera, maxHistory, tolerance, b): float32
    layers [K, H, W, 4] of the cascade (K, start 1, base 8) over synthetic_geometry, with every branch of the definition in them
    where the picture has room: frame counts and history counts below 1 and not finite, points outside the previous view, rejected counts that are not finite,
    history counts below and above the cap, a history sum of +inf (which is carried into its layer: inf stays inf through a positive
    weight, the quotient, the cap's factor and the sum, so no NaN of undefined payload arises), surface points exactly on a history
    pixel's column (weights of exactly 0), and words in the unused .w of the inner layers (not read, written as 0 where history is
    merged, kept where it is not). clean: none of the planted values, and counts that stay below the cap."""
    rng = np.random.default_rng(seed + 1000 * width + height + 7 * K)
    g, hg, cam = synthetic_geometry(width, height, seed)
    g, hg = g.copy(), hg.copy()
    b = cascade_restate.thresholds(K, 1.0, 8.0)

    def layers(n_choices):
        L = np.zeros((K, height, width, 4), F)
        n = rng.choice(np.array(n_choices, F), (height, width))
        for j in range(K):  # a layer's sum: its share of the samples x a radiance around its threshold
            share = n * F(0.5) ** F(j + 1)
            L[j, ..., :3] = (rng.gamma(2.0, 0.5, (height, width, 3)).astype(F) * b[j]) * share[..., None]
            L[j, ..., 3] = rng.uniform(-1.0, 1.0, (height, width)).astype(F)
        L[0, ..., 3] = n
        L[K - 1, ..., 3] = rng.choice(np.array([0, 0, 0, 1, 2.5], F), (height, width))
        return L

    Lc = layers([1, 4, 4, 4, 8])
    Hl = layers([1, 3, 12, 20] if clean else [1, 3, 12, 40, 100.5])
    if clean:
        return Lc, g, (Hl, hg), cam, MAX_HISTORY, TOLERANCE, b
    flat = lambda a: a.reshape(K, -1, 4)
    taken = list(rng.permutation(width * height))
    special = lambda: int(taken.pop()) if taken else None
    for value in (0.0, 0.5, -1.0, np.inf, np.nan):  # the frame's count, the history's count
        for array in (Lc, Hl):
            p = special()
            if p is not None:
                flat(array)[0, p, 3] = value
    for value in (np.inf, -np.inf, np.nan):  # the history's rejected count
        p = special()
        if p is not None:
            flat(Hl)[K - 1, p, 3] = value
    for layer in sorted({0, K // 2, K - 1}):  # a history sum that is not finite, in the layers the kernel keeps in registers and in one it gathers
        for _ in range(3 if width * height > 64 else 1):
            p = special()
            if p is not None:
                flat(Hl)[layer, p, int(rng.integers(3))] = np.inf
    gflat, hgflat = g.reshape(-1, 4), hg.reshape(-1, 4)
    for x in (50.0, -50.0):  # surface points in front of the previous camera and far outside its view
        p = special()
        if p is not None and gflat[p].view(U32)[3] != 0:
            gflat[p, :3] = (x, 0.0, 0.0)
    for _ in range(12 if width * height > 64 else 2):  # surface points exactly on a history pixel's column
        p = special()
        if p is not None and hgflat.shape[0] > 1:
            _on_a_pixel_centre(gflat, hgflat, cam, width, height, p, int(rng.integers(width * height)))
    return Lc, g, (Hl, hg), cam, MAX_HISTORY, TOLERANCE, b
