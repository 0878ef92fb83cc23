"""CPU: the rectified temporal merge (csrc/temporal_rectify_device.h) — the host-only form twk_temporal_rectify_host, the same header
compiled for the host, against the numpy float32 restatement tests/temporal_rectify_restate.py bit for bit; that a test which never
runs changes nothing; the exact cases; what the rule buys after a light is halved and what it costs when nothing changed; and the
trusted build of the cascade's merge. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from temporal_cascade_restate import synthetic_layers
from temporal_rectify_restate import BRANCHES, rectify_frames, restate_rectify, restate_temporal_cascade_trusted
from temporal_restate import F, U32, restate_temporal
from test_temporal_cascade_host import host_merge
from test_temporal_host import _exact_frame


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _same(got, expect, what):
    assert got.shape == expect.shape and got.dtype == expect.dtype, what
    diff = _bits(got) != _bits(expect)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} words differ, first at {np.argwhere(diff)[:4].tolist()}"


def _camera(twk, cam12):
    c = twk.CameraDefinition()
    for k in range(3):
        c.P[k], c.U[k], c.V[k], c.W[k] = (float(cam12[3 * j + k]) for j in range(4))
    return c


def host_rectify(twk, cur, mc, g, history, cam, max_history, tolerance, radius, min_taps, gamma, expect=0):
    """twk_temporal_rectify_host on numpy arrays: (colour, moments, trust), or the refusal's code when one is expected."""
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = cur.shape[:2]
    colour, moments, trust = np.full((height, width, 4), -7, F), np.full((height, width, 4), -7, F), np.full((height, width), -7, F)
    tp, rp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.TemporalRectify(radius, min_taps, gamma)
    hc, hm, hg = (None, None, None) if history is None else history
    rc = L.lib.twk_temporal_rectify_host(C.byref(tp), C.byref(rp), fp(cur), fp(mc), fp(g), fp(hc), fp(hm), fp(hg), None if history is None else C.byref(_camera(twk, cam)),
                                         int(width), int(height), fp(colour), fp(moments), fp(trust))
    assert rc == expect, L.lib.twk_last_error().decode()
    return (colour, moments, trust) if rc == 0 else rc


def test_the_new_calls_exist(twk):
    L = twk._lib
    for name in ("twk_temporal_rectify_defaults", "twk_temporal_accumulate_rectified", "twk_get_temporal_trust_device_pointer", "twk_read_temporal_trust",
                 "twk_temporal_accumulate_cascade_trusted", "twk_temporal_accumulate_assembled_rectified", "twk_temporal_rectify_host", "twk_temporal_cascade_trusted_host"):
        assert name in L.SYMBOLS and getattr(L.lib, name) is not None
    for method in ("temporalAccumulateRectified", "temporalAccumulateAssembledRectified", "temporalTrustDevicePointer", "readTemporalTrust", "temporalAccumulateCascadeTrusted"):
        assert callable(getattr(twk.Device, method))
    rp = L.TemporalRectify(-1, -1, -1.0)
    assert L.lib.twk_temporal_rectify_defaults(C.byref(rp)) == 0
    assert (rp.radius, rp.minTaps, rp.gamma) == (3, 8, 3.0) == (L.TWK_TEMPORAL_RECTIFY_RADIUS, L.TWK_TEMPORAL_RECTIFY_MIN_TAPS, L.TWK_TEMPORAL_RECTIFY_GAMMA)
    assert (twk.TemporalRectify().radius, twk.TemporalRectify().minTaps, twk.TemporalRectify().gamma) == (3, 8, 3.0)
    assert L.lib.twk_temporal_rectify_defaults(None) == L.TWK_ERROR_INVALID_VALUE
    for call, args in (("twk_temporal_accumulate_rectified", (None, None, None, None, None, 0, 0, None, None, None, None)),
                       ("twk_temporal_accumulate_assembled_rectified", (None, None, None)),
                       ("twk_temporal_accumulate_cascade_trusted", (None,) * 9 + (0, 0, None)),
                       ("twk_read_temporal_trust", (None, None, C.c_size_t(0))), ("twk_get_temporal_trust_device_pointer", (None, None, None))):
        assert getattr(L.lib, call)(*args) == L.TWK_ERROR_INVALID_VALUE, call
        assert call in L.lib.twk_last_error().decode(), call
    assert L.lib.twk_abi_version() == 9


def test_the_host_form_refuses_what_the_device_form_refuses(twk):
    L = twk._lib
    (cur, mc, g), history, cam, max_history, tolerance = rectify_frames(9, 7)
    ok = dict(radius=3, min_taps=8, gamma=3.0)
    for bad in (dict(radius=0), dict(radius=5), dict(radius=-1), dict(min_taps=1), dict(min_taps=0), dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf"))):
        assert host_rectify(twk, cur, mc, g, history, cam, max_history, tolerance, **{**ok, **bad}, expect=L.TWK_ERROR_INVALID_VALUE) == L.TWK_ERROR_INVALID_VALUE, bad
        assert "twk_temporal_rectify_host" in L.lib.twk_last_error().decode()
    assert host_rectify(twk, cur, mc, g, history, cam, 0, tolerance, **ok, expect=L.TWK_ERROR_INVALID_VALUE) == L.TWK_ERROR_INVALID_VALUE
    assert host_rectify(twk, cur, mc, g, history, cam, max_history, -1.0, **ok, expect=L.TWK_ERROR_INVALID_VALUE) == L.TWK_ERROR_INVALID_VALUE
    assert host_rectify(twk, cur, mc, g, (history[0], None, history[2]), cam, max_history, tolerance, **ok, expect=L.TWK_ERROR_INVALID_VALUE) == L.TWK_ERROR_INVALID_VALUE
    assert host_rectify(twk, cur, mc, g, history, np.zeros(12, F), max_history, tolerance, **ok, expect=L.TWK_ERROR_INVALID_VALUE) == L.TWK_ERROR_INVALID_VALUE  # a degenerate camera
    host_rectify(twk, cur, mc, g, history, cam, max_history, tolerance, radius=4, min_taps=2, gamma=0.0)  # the edges of the ranges are inside


@pytest.mark.parametrize("radius", [1, 3, 4])
@pytest.mark.parametrize("width,height", [(37, 23), (70, 20), (8, 8), (1, 1)])
def test_the_host_form_equals_the_restatement_bit_for_bit(twk, width, height, radius):
    """37x23: partial tiles and the halo over every border; 70x20: three tiles across; 8x8: a picture smaller than a tile; 1x1. The
    frames hold NaN and inf, an id edge, a depth step and misses, a region whose history is twice as bright and a noise-free one."""
    (cur, mc, g), history, cam, max_history, tolerance = rectify_frames(width, height)
    min_taps = {1: 4, 3: 20, 4: 30}[radius]  # enough that corners and the strips beside the id edge fall below it
    info = {}
    colour, moments, trust, merged = restate_rectify(cur, mc, g, history, cam, max_history, tolerance, radius, min_taps, 3.0, info)
    if width * height > 500:
        for branch in BRANCHES:
            assert info[branch] > 0, (branch, info)
    got = host_rectify(twk, cur, mc, g, history, cam, max_history, tolerance, radius, min_taps, 3.0)
    what = f"{width}x{height}, radius {radius}"
    _same(got[0], colour, what + ", colour")
    _same(got[1], moments, what + ", moments")
    _same(got[2], trust, what + ", trust")
    assert ((trust >= 0) & (trust <= 1)).all()
    assert np.array_equal(_bits(got[0])[~merged], _bits(cur)[~merged]) and np.array_equal(_bits(got[1])[~merged], _bits(mc)[~merged]), "a pass-through keeps the frame's bits"
    # no history: everything passes through with trust 1
    none = host_rectify(twk, cur, mc, g, None, cam, max_history, tolerance, radius, min_taps, 3.0)
    _same(none[0], cur, what + ", no history: colour")
    _same(none[1], mc, what + ", no history: moments")
    assert (none[2] == 1).all()


@pytest.mark.parametrize("width,height", [(37, 23), (8, 8)])
def test_no_test_means_no_change(twk, width, height):
    """minTaps = 50 at radius 3: a window has 49 taps, the test never runs. Every output has the bytes of restate_temporal — of the
    plain merge — and the trust is 1 everywhere."""
    (cur, mc, g), history, cam, max_history, tolerance = rectify_frames(width, height)
    plain_colour, plain_moments, took = restate_temporal(cur, mc, g, history, cam, max_history, tolerance)
    plain_colour[~took], plain_moments[~took] = cur[~took], mc[~took]
    assert took.sum() > 10
    colour, moments, trust = host_rectify(twk, cur, mc, g, history, cam, max_history, tolerance, 3, 50, 3.0)
    _same(colour, plain_colour, "colour against the plain merge")
    _same(moments, plain_moments, "moments against the plain merge")
    assert (trust == 1).all()
    again = restate_rectify(cur, mc, g, history, cam, max_history, tolerance, 3, 50, 3.0)
    _same(again[0], plain_colour, "the restatement's colour against the plain merge")
    _same(again[1], plain_moments, "the restatement's moments against the plain merge")


def _flat(value, mean, n, shape):
    colour = np.full(shape + (4,), value, F)
    colour[..., 3] = 1
    return colour, np.stack([np.full(shape, mean, F), np.zeros(shape, F), np.full(shape, n, F), np.zeros(shape, F)], axis=-1)


def test_exact_cases(twk):
    """Identical cameras with the surface points exactly at the pixel centres (test_temporal_host._exact_frame: one tap of weight 1).
    Noise-free equal frames, whatever their pattern: d = 0 everywhere, b2 = 0, trust 1, and the merge is the plain one. A noise-free
    history at twice the frame: d = -c everywhere, s2 = 0, rho = +inf, trust 0, and every pixel returns the frame's bits."""
    cam, g = _exact_frame(16, 8)
    shape = (8, 16)
    rng = np.random.default_rng(3)
    cur = rng.gamma(2.0, 0.5, shape + (4,)).astype(F)
    mc = np.stack([rng.gamma(2.0, 0.5, shape).astype(F), rng.gamma(2.0, 0.5, shape).astype(F), np.full(shape, 4, F), np.zeros(shape, F)], axis=-1)
    hm = mc.copy()
    hm[..., 2] = 20
    colour, moments, trust = host_rectify(twk, cur, mc, g, (cur, hm, g), cam, 32, 0.01, 3, 8, 3.0)
    plain_colour, plain_moments, took = restate_temporal(cur, mc, g, (cur, hm, g), cam, 32, 0.01)
    assert took.all() and (trust == 1).all()
    _same(colour, plain_colour, "equal frames: colour")
    _same(moments, plain_moments, "equal frames: moments")
    assert (moments[..., 2] == 24).all()
    (cur, mc), (hc, hm) = _flat(0.75, 0.75, 4, shape), _flat(1.5, 1.5, 32, shape)
    colour, moments, trust = host_rectify(twk, cur, mc, g, (hc, hm, g), cam, 32, 0.01, 3, 8, 3.0)
    assert (trust == 0).all()
    _same(colour, cur, "history at twice the frame: the frame's colour")
    _same(moments, mc, "history at twice the frame: the frame's moments")
    # ... and gamma does not matter there, nor does the radius
    assert (host_rectify(twk, cur, mc, g, (hc, hm, g), cam, 32, 0.01, 1, 2, 1000.0)[2] == 0).all()


# ---- statistics ----------------------------------------------------------------------------------------------------------------------
WALL = (64, 48)


def _wall(seed, light_then, light_now, spp=4, history_samples=32):
    """A 64x48 wall seen by identical cameras: a smooth luminance field with an edge inside one instance, gamma(2)-distributed samples
    (relative standard deviation 0.707 per sample). The history holds `history_samples` samples rendered at light_then x the field,
    the frame `spp` at light_now x the field. Returns (frame, history, camera, geometry, truth of the frame's lighting [H, W])."""
    width, height = WALL
    rng = np.random.default_rng(seed)
    cam, g = _exact_frame(width, height)
    y, x = np.mgrid[0:height, 0:width]
    field = (1.0 + 0.4 * np.sin(x / 9.0) * np.cos(y / 7.0)) * np.where(x > 40, 1.6, 1.0)

    def estimate(n, light):
        samples = rng.gamma(2.0, 0.5, (n, height, width)) * (field * light)
        mean, m2 = samples.mean(axis=0), ((samples - samples.mean(axis=0)) ** 2).sum(axis=0)
        colour = np.ones((height, width, 4), F)
        colour[..., :3] = mean[..., None].astype(F)
        return colour, np.stack([mean, m2, np.full_like(mean, n), np.zeros_like(mean)], axis=-1).astype(F)

    history = estimate(history_samples, light_then)
    frame = estimate(spp, light_now)
    return frame, history, cam, g, field * light_now


def _relative_rms(mean, truth):
    return float(np.sqrt((((mean.astype(np.float64) - truth) / truth) ** 2).mean()))


def test_unchanged_lighting_is_left_alone(twk):
    """Lighting unchanged, the defaults (radius 3, minTaps 8, gamma 3), 4 spp against a 32-sample history: the share of pixels whose
    history is discounted at all. The prototype the defaults come from measured at most 0.6 %; the cap of 5 % leaves 8 x room for
    another seed and for the field. The merged mean's error is printed beside the plain merge's."""
    shares = []
    for seed in (11, 12, 13):
        (cur, mc), (hc, hm), cam, g, truth = _wall(seed, 1.0, 1.0)
        colour, moments, trust = host_rectify(twk, cur, mc, g, (hc, hm, g), cam, 32, 0.01, 3, 8, 3.0)
        plain = restate_temporal(cur, mc, g, (hc, hm, g), cam, 32, 0.01)[1]
        share = float((trust < 1).mean())
        shares.append(share)
        print(f"\nseed {seed}: share of pixels with trust < 1 {share:.4f}; relative RMS error of the merged mean {_relative_rms(moments[..., 0], truth):.4f}, "
              f"plain merge {_relative_rms(plain[..., 0], truth):.4f}, frame alone {_relative_rms(mc[..., 0], truth):.4f}")
    assert max(shares) <= 0.05, shares


def test_a_halved_light_is_noticed(twk):
    """The light halves between the 32-sample history and the 4 spp frame. The plain merge keeps 32/36 of the old lighting (relative
    error about 0.9); the rectified merge must have at most half that error, and at most 1.15 x the error of the frame alone (0.354
    for 4 gamma(2) samples) — the prototype measured 0.351 against 0.913 and 0.353."""
    for seed in (21, 22, 23):
        (cur, mc), (hc, hm), cam, g, truth = _wall(seed, 2.0, 1.0)
        colour, moments, trust = host_rectify(twk, cur, mc, g, (hc, hm, g), cam, 32, 0.01, 3, 8, 3.0)
        plain = restate_temporal(cur, mc, g, (hc, hm, g), cam, 32, 0.01)[1]
        e_rect, e_plain, e_frame = _relative_rms(moments[..., 0], truth), _relative_rms(plain[..., 0], truth), _relative_rms(mc[..., 0], truth)
        print(f"\nseed {seed}: relative RMS error of the merged mean: rectified {e_rect:.4f}, plain merge {e_plain:.4f}, frame alone {e_frame:.4f}; mean trust {trust.mean():.4f}")
        assert e_rect <= 0.5 * e_plain, (seed, e_rect, e_plain)
        assert e_rect <= 1.15 * e_frame, (seed, e_rect, e_frame)
        _same(moments, restate_rectify(cur, mc, g, (hc, hm, g), cam, 32, 0.01, 3, 8, 3.0)[1], "the host form against the restatement")


# ---- the cascade's trusted build -----------------------------------------------------------------------------------------------------
def host_merge_trusted(twk, layers, g, history, cam, max_history, tolerance, K, trust):
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = g.shape[:2]
    out = np.full(layers.shape, -7, F)
    tp, cp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.Cascade(K, 1.0, 8.0)
    rc = L.lib.twk_temporal_cascade_trusted_host(C.byref(tp), C.byref(cp), fp(layers), fp(g), fp(history[0]), fp(history[1]), C.byref(_camera(twk, cam)), fp(trust),
                                                 int(width), int(height), fp(out))
    assert rc == 0, L.lib.twk_last_error().decode()
    return out


@pytest.mark.parametrize("width,height,K", [(37, 23, 6), (8, 8, 2)])
def test_the_trusted_cascade_merge(twk, width, height, K):
    """Trust all 1: the bytes of twk_temporal_cascade_host. A random trust in [0, 1] (with exact zeros and ones): the restatement bit
    for bit, and the merged count is the capped history count times the trust plus the frame's."""
    L = twk._lib
    Lc, g, history, cam, max_history, tolerance, _ = synthetic_layers(width, height, K)
    plain = host_merge(twk, Lc, g, history, cam, max_history, tolerance, K)
    ones = host_merge_trusted(twk, Lc, g, history, cam, max_history, tolerance, K, np.ones((height, width), F))
    _same(ones, plain, "trust 1 against twk_temporal_cascade_host")
    rng = np.random.default_rng(9)
    trust = rng.uniform(0.0, 1.0, (height, width)).astype(F)
    trust[rng.uniform(size=trust.shape) < 0.1] = 0
    trust[rng.uniform(size=trust.shape) < 0.1] = 1
    got = host_merge_trusted(twk, Lc, g, history, cam, max_history, tolerance, K, trust)
    expect, took, hn = restate_temporal_cascade_trusted(Lc, g, history, cam, max_history, tolerance, trust)
    assert took.sum() > 10
    _same(got, expect, "a random trust against the restatement")
    counts_ok = np.isfinite(got[0, ..., 3]) & took
    assert np.array_equal(got[0, ..., 3][counts_ok], (hn * trust + Lc[0, ..., 3])[counts_ok])
    assert np.array_equal(_bits(got)[:, ~took], _bits(Lc)[:, ~took]), "a pass-through keeps the frame's bits"
    null = L.lib.twk_temporal_cascade_trusted_host(None, None, Lc.ctypes.data_as(C.POINTER(C.c_float)), g.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None,
                                                   width, height, got.ctypes.data_as(C.POINTER(C.c_float)))
    assert null == L.TWK_ERROR_INVALID_VALUE and "twk_temporal_cascade_trusted_host" in L.lib.twk_last_error().decode()


# ---- the system description's keys ---------------------------------------------------------------------------------------------------
def _description(twk, text):
    """((enabled, radius, minTaps, gamma, keys), the description written back)"""
    from conftest import scene_path
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, rp, keys = app.temporalRectify
        return (on, rp.radius, rp.minTaps, rp.gamma, keys), app.systemDescription()
    finally:
        app.close()


def test_description_keys_of_the_rectified_merge(twk):
    from conftest import scene_path
    L = twk._lib
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    assert L.lib.twk_app_get_temporal_rectify(None, None, None, None) == L.TWK_ERROR_INVALID_VALUE and "twk_app_get_temporal_rectify" in L.lib.twk_last_error().decode()
    off, off_text = _description(twk, base)
    assert off == (False, 3, 8, 3.0, 0) and "temporalRectify" not in off_text, "off by default, nothing written back"
    keys = "\ntemporalAccumulation 1\ntemporalRectify 1\ntemporalRectifyGamma 2.5\ntemporalRectifyRadius 2\ntemporalRectifyMinTaps 12\n"
    on, on_text = _description(twk, base + keys)
    assert on == (True, 2, 12, 2.5, 4)
    for line in keys.strip().splitlines():
        assert line + "\n" in on_text, line
    assert _description(twk, on_text) == (on, on_text), "what is written back parses to the same"
    edges, _ = _description(twk, base + "\ntemporalRectifyGamma 0\ntemporalRectifyRadius 4\ntemporalRectifyMinTaps 2\n")
    assert edges == (False, 4, 2, 0.0, 3)
    # a value the call would refuse drops the line and keeps the previous value; the key still counts as seen
    for bad in ("temporalRectifyGamma -1", "temporalRectifyRadius 0", "temporalRectifyRadius 5", "temporalRectifyMinTaps 1", "temporalRectify 2"):
        got, text = _description(twk, base + f"\n{bad}\n")
        assert got == (False, 3, 8, 3.0, 1) and "temporalRectify" not in text, bad
