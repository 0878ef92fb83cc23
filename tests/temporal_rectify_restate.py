"""The rectified temporal merge of csrc/temporal_rectify_device.h restated statement for statement in numpy float32 (no GPU needed),
with a count per branch, the trusted build of the cascade's temporal merge (csrc/temporal_cascade_device.h), and the frames the tests
feed both sides. The gather, the capped history and the synthetic frames are temporal_restate's, the cascade's merge
temporal_cascade_restate's.
No test in here: tests/test_temporal_rectify_host.py (CPU) and tests/test_gpu_temporal_rectify*.py use it."""
import numpy as np

import temporal_cascade_restate
import temporal_restate
from temporal_restate import F, U32, capped_history, gather

BRANCHES = ("no_history", "key_zero_with_history", "few_taps", "explained_by_noise", "discounted", "trust_zero", "merged", "passed_through")


def reproject(cur, mc, g, history, cam, max_history, tolerance):
    """Launch 1 on float32 [H, W, 4] arrays: temporal_restate's gather and capped history. Returns (h [H, W, 3], hmean, hM2, hn, took):
    the reprojected, capped history, all 0 where took is False (hn = 0: no history)."""
    height, width = cur.shape[:2]
    zero = np.zeros((height, width), F)
    if history is None:
        return np.zeros((height, width, 3), F), zero, zero.copy(), zero.copy(), np.zeros((height, width), bool)
    sums, took, _ = gather(cur, mc, g, history, cam, tolerance)
    hx, hy, hz, hmean, hm2, hn, _ = capped_history(sums, max_history)
    h = np.where(took[..., None], np.stack([hx, hy, hz], axis=-1), F(0.0)).astype(F)
    hmean, hm2, hn = (np.where(took, a, F(0.0)).astype(F) for a in (hmean, hm2, hn))
    return h, hmean, hm2, hn, took


def trust_of(mc, g, hmean, hn, radius, min_taps, gamma, info=None):
    """The test of launch 2: the trust t [H, W] from the frame's moments, its geometry and the reprojected history's mean and count."""
    height, width = hn.shape
    R = int(radius)
    g2 = F(gamma) * F(gamma)
    with np.errstate(all="ignore"):
        d = mc[..., 0] - hmean
        key = np.where((hn > F(0.0)) & np.isfinite(d), g[..., 3].view(U32), U32(0)).astype(U32)
        dp = np.zeros((height + 2 * R, width + 2 * R), F)
        kp = np.zeros((height + 2 * R, width + 2 * R), U32)
        dp[R:R + height, R:R + width] = d
        kp[R:R + height, R:R + width] = key
        window = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]  # row-major
        shifted = lambda a, dy, dx: a[R + dy:R + dy + height, R + dx:R + dx + width]
        m = np.zeros((height, width), np.int64)
        total = np.zeros((height, width), F)
        for dy, dx in window:
            counted = (shifted(kp, dy, dx) == key) & (key != 0)
            m += counted
            total = np.where(counted, total + shifted(dp, dy, dx), total)
        dbar = total / m.astype(F)
        ss = np.zeros((height, width), F)
        for dy, dx in window:
            counted = (shifted(kp, dy, dx) == key) & (key != 0)
            e = shifted(dp, dy, dx) - dbar
            ss = np.where(counted, ss + e * e, ss)
        s2 = ss / (m - 1).astype(F)
        b2 = dbar * dbar - g2 * (s2 / m.astype(F))
        tested = (key != 0) & (m >= int(min_taps))
        biased = tested & (b2 > F(0.0))
        rho = b2 / s2
        t = F(1.0) / (F(1.0) + rho * (F(1.0) + hn / mc[..., 2]))
        t = np.where(biased, t, F(1.0)).astype(F)
    assert t.dtype == F and d.dtype == F and s2.dtype == F and b2.dtype == F
    if info is not None:
        info.update(no_history=int((hn == 0).sum()), key_zero_with_history=int(((key == 0) & (hn > 0)).sum()), few_taps=int(((key != 0) & ~tested).sum()),
                    explained_by_noise=int((tested & ~biased).sum()), discounted=int((biased & (t > 0) & (t < 1)).sum()), trust_zero=int((biased & (t == 0)).sum()))
    return t


def restate_rectify(cur, mc, g, history, cam, max_history, tolerance, radius, min_taps, gamma, info=None):
    """twk_temporal_accumulate_rectified on float32 [H, W, 4] arrays (cur = the current colour WIDENED), history = (colour, moments,
    geometry) or None, cam the history's camera. Returns (colour f32, moments f32, trust f32 [H, W], merged) — merged: the pixels
    that merged history; the others pass through (the caller keeps the input's bits there, as with restate_temporal)."""
    cur, mc, g = (np.ascontiguousarray(a, F) for a in (cur, mc, g))
    h, hmean, hm2, hn, _ = reproject(cur, mc, g, history, cam, max_history, tolerance)
    t = trust_of(mc, g, hmean, hn, radius, min_taps, gamma, info)
    colour, moments = cur.copy(), mc.copy()
    with np.errstate(all="ignore"):
        hn2, hm22 = hn * t, hm2 * t
        merged = hn2 > F(0.0)
        n = hn2 + mc[..., 2]
        r = mc[..., 2] / n
        c = np.stack([h[..., 0] + (cur[..., 0] - h[..., 0]) * r, h[..., 1] + (cur[..., 1] - h[..., 1]) * r, h[..., 2] + (cur[..., 2] - h[..., 2]) * r, cur[..., 3]], axis=-1)
        d = mc[..., 0] - hmean
        mm = np.stack([hmean + d * r, (hm22 + mc[..., 1]) + (d * d) * (hn2 * r), n, np.zeros_like(n)], axis=-1)
    assert c.dtype == F and mm.dtype == F
    colour[merged] = c[merged]
    moments[merged] = mm[merged]
    trust = np.where(merged, t, np.where(hn > F(0.0), F(0.0), t)).astype(F)
    if info is not None:
        info.update(merged=int(merged.sum()), passed_through=int((~merged).sum()))
    return colour, moments, trust, merged


def expect_rectify(colour_raw, moments, geometry, history, cam, max_history, tolerance, radius, min_taps, gamma, info=None):
    """The four outputs as the device writes them: (colourOut in the format of colour_raw, historyOut f32, momentsOut f32, trustOut)."""
    colour, merged_moments, trust, merged = restate_rectify(colour_raw.astype(F), moments, geometry, history, cam, max_history, tolerance, radius, min_taps, gamma, info)
    narrow = colour
    if colour_raw.dtype == np.float16:
        with np.errstate(over="ignore"):
            narrow = colour.astype(np.float16)
    else:
        narrow = colour.copy()
    narrow[~merged] = colour_raw[~merged]
    return narrow, colour, merged_moments, trust, merged


def restate_temporal_cascade_trusted(layers, g, history, cam, max_history, tolerance, trust):
    """The trusted build of temporalCascadePixel: temporal_cascade_restate's merge with h[j] *= t, hrej *= t, hn *= t after the cap.
    Returns (merged layers, took, hn after the cap)."""
    return temporal_cascade_restate.merge_cascade(layers, g, history, cam, max_history, tolerance, trust=trust)


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def rectify_frames(width, height, seed=0):
    """temporal_restate.synthetic_frames (NaN and inf in every word, the id edge, the depth step, misses) with something for the test
    to find: in the right third of the picture the history's colour and luminance mean are twice what they were (a light that has been
    dimmed since: a bias the noise around it only partly explains), and in the lowest quarter frame and history are noise-free, the
    history at exactly twice the frame (s2 = 0: trust 0). A picture too small for synthetic_frames' 56 planted values (1x1) gets its
    cameras and wall with random, finite colours and moments."""
    if width * height > temporal_cascade_restate._SPECIALS:
        (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance = temporal_restate.synthetic_frames(width, height, seed)
    else:
        g, hg, cam = temporal_cascade_restate.synthetic_geometry(width, height, seed)
        rng = np.random.default_rng(seed + 1000 * width + height)
        cur, hc = (rng.gamma(2.0, 0.5, (height, width, 4)).astype(F) for _ in range(2))
        mc, hm = (np.stack([rng.gamma(2.0, 0.5, (height, width)).astype(F), rng.gamma(2.0, 0.5, (height, width)).astype(F), np.full((height, width), n, F),
                            np.zeros((height, width), F)], axis=-1) for n in (4, 20))
        max_history, tolerance = temporal_cascade_restate.MAX_HISTORY, temporal_cascade_restate.TOLERANCE
    cur, mc, hc, hm = (a.copy() for a in (cur, mc, hc, hm))
    right = slice(width - width // 3, width)
    hc[:, right, :3] *= F(2.0)
    hm[:, right, 0] *= F(2.0)
    low = slice(0, height // 4)
    finite = lambda a: np.isfinite(a[low][..., :3]).all(axis=-1)
    keep_c, keep_h = finite(cur) & finite(mc), finite(hc) & finite(hm)  # the planted NaN and inf stay where they are
    cur[low][keep_c, :3] = F(1.0)
    mc[low][keep_c, 0], mc[low][keep_c, 1] = F(1.0), F(0.0)
    hc[low][keep_h, :3] = F(2.0)
    hm[low][keep_h, 0], hm[low][keep_h, 1] = F(2.0), F(0.0)
    if width >= 12 and height >= 12:  # finite means whose difference is not: such a pixel has history, merges it, and is no tap of any window
        patch = (slice(height // 2, height // 2 + 5), slice(2, 8))
        mc[patch + (0,)] = np.where(np.isfinite(mc[patch + (0,)]), F(3e38), mc[patch + (0,)])
        hm[patch + (0,)] = np.where(np.isfinite(hm[patch + (0,)]), F(-3e38), hm[patch + (0,)])
    return (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance
