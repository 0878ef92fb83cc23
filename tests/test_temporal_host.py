"""CPU: the temporal merge of csrc/temporal_device.h through its numpy float32 restatement (tests/temporal_restate.py) — that the
definition merges two sample sets into the moments of their union, and that the cap does what the header says. The new calls must
exist in the library and its binding (no GPU needed to look)."""
import numpy as np

from temporal_restate import F, restate_temporal, synthetic_frames

U32 = np.uint32


def test_the_new_calls_exist(twk):
    L = twk._lib
    for name in ("twk_set_sample_offset", "twk_enable_geometry", "twk_render_geometry", "twk_read_geometry", "twk_get_geometry_device_pointer",
                 "twk_temporal_defaults", "twk_temporal_accumulate", "twk_temporal_reset", "twk_get_temporal_device_pointers", "twk_read_temporal",
                 "twk_read_temporal_moments"):
        assert name in L.SYMBOLS and getattr(L.lib, name) is not None
    for method in ("setSampleOffset", "enableGeometry", "renderGeometry", "readGeometry", "geometryDevicePointer", "temporalAccumulate", "temporalReset",
                   "readTemporal", "readTemporalMoments", "temporalDevicePointers"):
        assert callable(getattr(twk.Device, method))
    tp = L.Temporal()
    tp.maxHistory, tp.positionTolerance = -1, -1.0
    assert L.lib.twk_temporal_defaults(twk._lib.C.byref(tp)) == 0
    assert (tp.maxHistory, tp.positionTolerance) == (L.Temporal().maxHistory, L.Temporal().positionTolerance) == (L.TWK_TEMPORAL_MAX_HISTORY, F(L.TWK_TEMPORAL_POSITION_TOLERANCE))
    assert L.lib.twk_temporal_accumulate(None, None, None, None, 0, 0, None, None, None) == L.TWK_ERROR_INVALID_VALUE
    assert "twk_temporal_accumulate" in L.lib.twk_last_error().decode()
    assert twk.TemporalFrame().colour is None


def _welford(samples):
    """shade_device.h foldSamples over samples [n, ...] in float32: (mean, M2, n)."""
    mean, m2, n = (np.zeros(samples.shape[1:], F) for _ in range(3))
    for l in samples:
        n = n + F(1.0)
        d = l - mean
        mean = mean + d / n
        m2 = m2 + d * (l - mean)
    return mean, m2, n


def _exact_frame(width, height):
    """A camera and a wall whose arithmetic is exact: P = (0, 0, 1), U = (2, 0, 0), V = (0, 1, 0), W = (0, 0, -1), and the surface
    points P + W + ndcX U + ndcY V with ndc = (pixel + 0.5) / size * 2 - 1, dyadic for sizes that are powers of two. Then A, B, C, D
    and the three dot products are exact, a / c = ndcX, and fx = x, fy = y with tx = ty = 0: one tap of weight 1 per pixel."""
    cam = np.array([0, 0, 1, 2, 0, 0, 0, 1, 0, 0, 0, -1], F)
    ndcx = ((np.arange(width, dtype=F) + F(0.5)) / F(width)) * F(2.0) - F(1.0)
    ndcy = ((np.arange(height, dtype=F) + F(0.5)) / F(height)) * F(2.0) - F(1.0)
    g = np.zeros((height, width, 4), F)
    g[..., 0] = F(2.0) * ndcx[None, :]
    g[..., 1] = ndcy[:, None]
    g[..., 3] = np.full((height, width), 7, U32).view(F)
    return cam, g


def test_two_halves_merge_into_the_moments_of_the_whole():
    """Identical cameras, surface points exactly at the pixel centres (one tap, weight 1), no cap: the history holds the f32 Welford
    triple of the first k samples of every pixel and their mean colour, the frame those of the other k; the merge must be the triple
    and the mean of all n = 2k, compared with float64 moments of the union.

    The bound, relative n * 2^-23. A step of Welford's recurrence and the merge form the mean as a convex combination of positive
    values and M2 as a sum of non-negative terms, so relative errors add and are never amplified by cancellation. Each of the n
    samples enters through one step whose roundings (the difference, the quotient or product, the sum) are 2^-24 each at most and
    leave, to first order, at most 2 * 2^-24 = 2^-23 relative in the running value once the small terms' share is weighed; the
    merge adds a constant handful. n of them: n * 2^-23 — the f32 spacing times the number of samples, which is what n roundings
    cost at the very most. (Measured, it is an order of magnitude below.)"""
    width, height, k = 16, 8, 8
    rng = np.random.default_rng(5)
    cam, g = _exact_frame(width, height)
    colours = rng.gamma(2.0, 0.5, (2 * k, height, width, 3)).astype(F)
    lum = (F(0.2126) * colours[..., 0] + F(0.7152) * colours[..., 1]) + F(0.0722) * colours[..., 2]

    def frame(c, l):
        mean, m2, n = _welford(l)
        colour = np.ones((height, width, 4), F)
        colour[..., :3] = c.astype(np.float64).mean(axis=0).astype(F)
        return colour, np.stack([mean, m2, n, np.zeros_like(n)], axis=-1)

    (hc, hm), (cur, mc) = frame(colours[:k], lum[:k]), frame(colours[k:], lum[k:])
    info = {}
    colour, moments, took = restate_temporal(cur, mc, g, (hc, hm, g), cam, 1000, 0.01, info)
    assert took.all()  # (the three other taps have weight 0 and count, or are rejected, harmlessly: test_weight_zero_taps_change_nothing)
    assert info["capped"] == 0
    n = 2 * k
    bound = n * 2.0 ** -23
    l64 = lum.astype(np.float64)
    mean64, m264 = l64.mean(axis=0), ((l64 - l64.mean(axis=0)) ** 2).sum(axis=0)
    assert (moments[..., 2] == n).all() and (moments[..., 3] == 0).all()
    err_mean = np.abs(moments[..., 0] - mean64) / mean64
    err_m2 = np.abs(moments[..., 1] - m264) / m264
    colour64 = colours.astype(np.float64).mean(axis=0)
    err_colour = np.abs(colour[..., :3] - colour64) / colour64
    print(f"\nn = {n}: relative error of the mean {err_mean.max():.3e}, of M2 {err_m2.max():.3e}, of the colour {err_colour.max():.3e}; bound {bound:.3e}")
    assert err_mean.max() <= bound and err_m2.max() <= bound and err_colour.max() <= bound


def test_weight_zero_taps_change_nothing():
    """At exact pixel centres the taps at dx = 1 and dy = 1 have weight 0: a history that differs only there gives the same bits."""
    cam, g = _exact_frame(16, 8)
    rng = np.random.default_rng(6)
    cur, hc = (rng.gamma(2.0, 0.5, (8, 16, 4)).astype(F) for _ in range(2))
    mc, hm = (np.stack([rng.gamma(2.0, 0.5, (8, 16)).astype(F), rng.gamma(2.0, 0.5, (8, 16)).astype(F), np.full((8, 16), 4, F), np.zeros((8, 16), F)], axis=-1) for _ in range(2))
    colour, moments, took = restate_temporal(cur, mc, g, (hc, hm, g), cam, 32, 0.01)
    r = F(4.0) / F(8.0)
    assert took.all() and np.array_equal(colour[..., :3], hc[..., :3] + (cur[..., :3] - hc[..., :3]) * r) and np.array_equal(colour[..., 3], cur[..., 3])


def test_the_cap_leaves_the_variance_of_the_history_unchanged():
    """hn > maxHistory: hM2 is scaled by maxHistory / hn along with hn, so that M2 / n — the sample variance the history stands
    for — stays, and only its weight shrinks. Seen through a frame that adds nothing to M2 (mc.y = 0 and mean = the history's, d = 0):
    the merged M2 is the capped hM2, two roundings (the quotient, the product) away from hM2 * maxHistory / hn."""
    cam, g = _exact_frame(16, 8)
    rng = np.random.default_rng(7)
    shape = (8, 16)
    hn = rng.choice(np.array([33, 40, 100, 1000, 12345], F), shape)
    hmean, hm2 = rng.gamma(2.0, 0.5, shape).astype(F), rng.gamma(2.0, 50.0, shape).astype(F)
    hm = np.stack([hmean, hm2, hn, np.zeros(shape, F)], axis=-1)
    mc = np.stack([hmean, np.zeros(shape, F), np.full(shape, 4, F), np.zeros(shape, F)], axis=-1)
    cur = hc = np.ones(shape + (4,), F)
    info = {}
    _, moments, took = restate_temporal(cur, mc, g, (hc, hm, g), cam, 32, 0.01, info)
    assert took.all() and info["capped"] == took.sum() and (moments[..., 2] == 36).all()
    assert np.array_equal(moments[..., 0], hmean)
    variance_before = hm2.astype(np.float64) / hn.astype(np.float64)
    variance_after = moments[..., 1].astype(np.float64) / 32.0
    assert (np.abs(variance_after - variance_before) / variance_before).max() <= 2.0 ** -23 * 1.001
    # below the cap nothing is scaled: the same frame with maxHistory above every hn keeps hM2's bits
    _, uncapped, _ = restate_temporal(cur, mc, g, (hc, hm, g), cam, 20000, 0.01)
    assert np.array_equal(uncapped[..., 1], hm2) and np.array_equal(uncapped[..., 2], hn + F(4.0))


def test_the_synthetic_frames_reach_every_branch():
    """What tests/test_gpu_temporal.py feeds the device: no branch of the definition is empty at either size."""
    for width, height in ((37, 23), (64, 4)):
        current, history, cam, max_history, tolerance = synthetic_frames(width, height)
        info = {}
        colour, moments, took = restate_temporal(*current, history, cam, max_history, tolerance, info)
        for branch in ("miss", "id_mismatch", "outside", "behind", "position", "current_not_finite", "current_n_below_1", "history_not_finite",
                       "capped", "uncapped", "one_tap", "four_taps", "took"):
            assert info[branch] > 0, (width, height, branch, info)
        through = ~took
        assert np.array_equal(colour.view(U32)[through], current[0].view(U32)[through]) and np.array_equal(moments.view(U32)[through], current[1].view(U32)[through])
        assert np.isfinite(colour[took][:, :3]).all() and np.isfinite(moments[took]).all() and (moments[took][:, 2] > 1).all()
        none, _, took_none = restate_temporal(*current, None, cam, max_history, tolerance)
        assert not took_none.any() and np.array_equal(none.view(U32), current[0].view(U32))
