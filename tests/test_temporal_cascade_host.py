"""CPU: the cascade's layers through the temporal merge (csrc/temporal_cascade_device.h) — the host-only form
twk_temporal_cascade_host, the same header compiled for the host, against the numpy float32 restatement
tests/temporal_cascade_restate.py bit for bit, with every branch of the definition reached; and that the merge keeps what the
cascade's layers mean: the luminance count of the merged layers is the history's interpolated count plus the frame's."""
import ctypes as C

import numpy as np
import pytest

from temporal_cascade_restate import BRANCHES, F, U32, restate_temporal_cascade, synthetic_layers
from temporal_restate import camera_array

SIZES = ((1, 1), (5, 3), (37, 23))
LAYERS = (2, 6, 8)


def _camera(twk, cam12):
    c = twk.CameraDefinition()
    for k in range(3):
        c.P[k], c.U[k], c.V[k], c.W[k] = (float(cam12[3 * j + k]) for j in range(4))
    return c


def host_merge(twk, layers, g, history, cam, max_history, tolerance, K, expect=0):
    """twk_temporal_cascade_host on numpy arrays; returns the merged layers (or the refusal's code when one is expected)."""
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = g.shape[:2]
    out = np.full(layers.shape, 77.0, F)
    tp, cp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.Cascade(K, 1.0, 8.0)
    hl, hgeo = (None, None) if history is None else history
    rc = L.lib.twk_temporal_cascade_host(C.byref(tp), C.byref(cp), fp(layers), fp(g), fp(hl), fp(hgeo), None if cam is None else C.byref(_camera(twk, cam)),
                                         int(width), int(height), out.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == expect, L.lib.twk_last_error().decode()
    return out


def _same(got, expect, what):
    diff = got.view(U32) != expect.view(U32)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} words differ, first at {np.argwhere(diff)[:4].tolist()}"


def test_the_new_calls_exist(twk):
    L = twk._lib
    for name in ("twk_temporal_accumulate_cascade", "twk_temporal_enable_cascade", "twk_get_temporal_cascade_device_pointer", "twk_read_temporal_cascade",
                 "twk_temporal_cascade_host"):
        assert name in L.SYMBOLS and getattr(L.lib, name) is not None
    for method in ("temporalAccumulateCascade", "enableTemporalCascade", "temporalCascadeDevicePointer", "readTemporalCascade"):
        assert callable(getattr(twk.Device, method))
    assert L.lib.twk_temporal_accumulate_cascade(None, None, None, None, None, None, None, None, 0, 0, None) == L.TWK_ERROR_INVALID_VALUE
    assert "twk_temporal_accumulate_cascade" in L.lib.twk_last_error().decode()
    assert L.lib.twk_temporal_enable_cascade(None, 1) == L.TWK_ERROR_INVALID_VALUE and "twk_temporal_enable_cascade" in L.lib.twk_last_error().decode()


def test_the_host_form_equals_the_restatement_bit_for_bit_and_every_branch_is_reached(twk):
    """1x1, 5x3 and 37x23 with 2, 6 and 8 layers. Every branch of the definition must be reached at least once over the cases (the
    small pictures have no room for all of them), asserted from the restatement's counts; at 37x23 with 6 layers all of them are
    reached in the one case the device is given too (tests/test_gpu_temporal_cascade.py)."""
    total = dict.fromkeys(BRANCHES, 0)
    for width, height in SIZES:
        for K in LAYERS:
            Lc, g, history, cam, max_history, tolerance, _ = synthetic_layers(width, height, K)
            info = {}
            expect, took = restate_temporal_cascade(Lc, g, history, cam, max_history, tolerance, info)
            got = host_merge(twk, Lc, g, history, cam, max_history, tolerance, K)
            _same(got, expect, f"{width}x{height}, {K} layers")
            through = ~took
            assert np.array_equal(got.view(U32)[:, through], Lc.view(U32)[:, through]), "a pixel without history keeps the input's bits"
            if K > 2:
                assert (got[1:K - 1, took, 3] == 0).all(), "the inner layers' .w of a merged pixel is 0"
            for key in BRANCHES:
                total[key] += info[key]
            if (width, height) == (37, 23):
                for key in BRANCHES:
                    assert info[key] > 0, (K, key, info)
            none = host_merge(twk, Lc, g, None, None, max_history, tolerance, K)
            _same(none, Lc, f"{width}x{height}, {K} layers, no history")
    print("\nbranch counts over the nine cases:", total)
    for key in BRANCHES:  # a miss, geometry that is not finite, nc < 1, behind, outside the view, an instance mismatch, a tolerance failure,
        assert total[key] > 0, (key, total)  # hn < 1, a weight of exactly 0, the cap taken and not, a history sum that is not finite


def test_a_history_sum_that_is_not_finite_is_carried_into_its_layer_only(twk):
    """One tap of weight 1 (identical cameras, surface points on the pixel centres of a 16x8 picture, whose arithmetic is exact):
    +inf in one component of one history layer arrives in that component of that layer of the output and nowhere else."""
    from test_temporal_host import _exact_frame
    width, height, K = 16, 8, 6
    cam, g = _exact_frame(width, height)
    rng = np.random.default_rng(11)
    Lc, Hl = (rng.gamma(2.0, 0.5, (K, height, width, 4)).astype(F) for _ in range(2))
    Lc[0, ..., 3], Hl[0, ..., 3], Lc[K - 1, ..., 3], Hl[K - 1, ..., 3] = 4, 8, 0, 1
    Hl[3, 2, 5, 1] = np.inf
    info, taps = {}, []
    expect, took = restate_temporal_cascade(Lc, g, (Hl, g), cam, 1000, 0.01, info, taps)
    assert took.all() and info["history_sum_not_finite"] == 1 and all(counted.sum() == 0 for counted, _, _, _ in taps[1:])
    got = host_merge(twk, Lc, g, (Hl, g), cam, 1000, 0.01, K)
    _same(got, expect, "one tap of weight 1")
    bad = ~np.isfinite(got)
    assert bad.sum() == 1 and got[3, 2, 5, 1] == np.inf
    clean = Hl.copy()
    clean[3, 2, 5, 1] = 1.0
    other = host_merge(twk, Lc, g, (clean, g), cam, 1000, 0.01, K)
    assert (other.view(U32) != got.view(U32)).sum() == 1
    # weight 1, no cap: the merged layers are the plain sums of the two
    assert np.array_equal(other[..., :3], clean[..., :3] + Lc[..., :3])
    assert (other[0, ..., 3] == 12).all() and (other[K - 1, ..., 3] == 1).all()


def _count(layers, b):
    """sum_j luminance(layer j) / b[j] in float64: the number of samples the layers stand for (cascade_device.h FOLD)."""
    L = layers[..., :3].astype(np.float64)
    lam = (0.2126 * L[..., 0] + 0.7152 * L[..., 1]) + 0.0722 * L[..., 2]
    return (lam / b.astype(np.float64)[:, None, None]).sum(axis=0)


@pytest.mark.parametrize("K", LAYERS)
def test_the_merge_adds_the_luminance_counts(twk, K):
    """Below the cap the merge is linear, so the luminance count sum_j lambda_j / b_j of the merged layers must be the history's
    count interpolated with the taps' weights plus the frame's. Checked on the host form's output at 37x23, in float64, against
    sum_t w_t count(H[q_t]) / sum_t w_t + count(Lc) with the definition's own f32 weights w_t.

    The bound, relative 10 x 2^-24. Every sum of the synthetic layers is positive, so every term below is positive and relative
    errors add without amplification. A component of out[j] is ((sum_t w_t H[j][q_t]) / ws) + Lc[j]: each product rounds once (1),
    the four-term sum at most three times (the first addition, to 0, is exact) (3), the quotient once (1), the final sum once (1);
    ws itself is a four-term sum of the weights, three roundings (3). Nine roundings of at most 2^-24 each, to first order
    9 x 2^-24 on every term and so on their weighted sum; 10 x 2^-24 covers the second-order terms. The count is then evaluated
    in float64 on both sides, which adds nothing at this scale."""
    width, height = 37, 23
    Lc, g, (Hl, hg), cam, _, tolerance, b = synthetic_layers(width, height, K, clean=True)
    info, taps = {}, []
    expect, took = restate_temporal_cascade(Lc, g, (Hl, hg), cam, 1000, tolerance, info, taps)
    assert info["capped"] == 0 and took.sum() > 100
    got = host_merge(twk, Lc, g, (Hl, hg), cam, 1000, tolerance, K)
    _same(got, expect, "the clean layers")
    history_count = _count(Hl, b)
    num, den = np.zeros((height, width)), np.zeros((height, width))
    for counted, w, qy, qx in taps:
        w64 = np.where(counted, w.astype(np.float64), 0.0)
        num += w64 * history_count[qy, qx]
        den += w64
    want = num[took] / den[took] + _count(Lc, b)[took]
    have = _count(got, b)[took]
    error = np.abs(have - want) / want
    bound = 10 * 2.0 ** -24
    print(f"\n{K} layers: {took.sum()} merged pixels, relative error of the luminance count at most {error.max():.3e}; bound {bound:.3e}")
    assert error.max() <= bound
    # and n itself: the interpolated history count plus the frame's, the same way
    n_num = sum(np.where(counted, w.astype(np.float64), 0.0) * Hl[0, ..., 3].astype(np.float64)[qy, qx] for counted, w, qy, qx in taps)
    n_want = n_num[took] / den[took] + Lc[0, ..., 3][took]
    assert (np.abs(got[0, ..., 3][took] - n_want) / n_want).max() <= bound


def test_refusals_of_the_host_form(twk):
    L = twk._lib
    Lc, g, (Hl, hg), cam, max_history, tolerance, _ = synthetic_layers(5, 3, 6)
    bad = L.TWK_ERROR_INVALID_VALUE
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(Lc)
    camera = _camera(twk, cam)
    call = lambda tp, cp, a, b_, c, d, e, w, h, o: L.lib.twk_temporal_cascade_host(tp, cp, a, b_, c, d, e, w, h, o)
    ok = (None, None, fp(Lc), fp(g), fp(Hl), fp(hg), C.byref(camera), 5, 3, fp(out))
    assert call(*ok) == 0
    for index in (2, 3, 9):  # NULL current layers, geometry, output
        args = list(ok)
        args[index] = None
        assert call(*args) == bad and "twk_temporal_cascade_host" in L.lib.twk_last_error().decode()
    for index in (5, 6):  # history layers without their geometry / camera
        args = list(ok)
        args[index] = None
        assert call(*args) == bad
    for tp in (L.Temporal(maxHistory=0), L.Temporal(positionTolerance=-0.1), L.Temporal(positionTolerance=float("nan"))):
        assert call(C.byref(tp), *ok[1:]) == bad
    for cp in (L.Cascade(1, 1.0, 8.0), L.Cascade(9, 1.0, 8.0), L.Cascade(6, 0.0, 8.0), L.Cascade(6, 1.0, 1.0), L.Cascade(8, 1e30, 1e3)):
        assert call(None, C.byref(cp), *ok[2:]) == bad
    for size in ((0, 3), (5, 0), (1 << 15, 1 << 14)):  # the last: above 2^28 elements, refused before anything is read
        assert call(*ok[:7], size[0], size[1], ok[9]) == bad
    for degenerate in ([0] * 12, list(cam[:3]) + [1, 0, 0, 0, 1, 0, 2, 0, 0], list(cam[:3]) + [float("nan")] * 9, list(cam[:9]) + [float("inf"), 0, 0]):
        assert call(*ok[:6], C.byref(_camera(twk, np.array(degenerate, F))), *ok[7:]) == bad and "degenerate" in L.lib.twk_last_error().decode()
    # no history: the camera is not looked at
    assert call(None, None, fp(Lc), fp(g), None, None, None, 5, 3, fp(out)) == 0 and np.array_equal(out.view(U32), Lc.view(U32))
    assert camera_array(cam).shape == (12,)
