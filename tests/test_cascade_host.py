"""CPU: the firefly cascade's definition (csrc/cascade_device.h) through its host-only forms twk_cascade_fold_host and
twk_cascade_resolve_host, which are compiled from the header the kernels are compiled from, against the numpy restatement
tests/cascade_restate.py, bit for bit; the two properties the definition promises (the layers count samples, and they sum to the
plain sum below the top threshold); every refusal that needs no device; and the five keys of the system description."""
import ctypes as C

import numpy as np
import pytest

import cascade_restate as restate
from conftest import scene_path
from test_moments_host import F, luminance

H, W = 5, 7  # 35 elements: every pixel of the 3x3 window's border cases (corners, edges, interior)


def _bits(a):
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _same(a, b, what):
    diff = _bits(a) != _bits(b)
    assert a.shape == b.shape and not diff.any(), f"{what}: {diff.sum()} of {diff.size} words differ, first at {np.argwhere(diff)[:4].tolist()}"


def _pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def fold_host(twk, params, samples, first, layers, debug=False):
    L = twk._lib
    samples = np.ascontiguousarray(samples, F)
    out = np.array(layers, F)
    n = int(np.prod(samples.shape[1:-1]))
    L.check(L.lib.twk_cascade_fold_host(C.byref(params), _pf(samples), C.c_size_t(samples.shape[0]), C.c_size_t(n), C.c_uint(first), int(debug), _pf(out)))
    return out


def resolve_host(twk, params, kappa, layers):
    L = twk._lib
    layers = np.ascontiguousarray(layers, F)
    out = np.empty(layers.shape[1:], F)
    L.check(L.lib.twk_cascade_resolve_host(C.byref(params), C.byref(L.CascadeResolve(kappa)), _pf(layers), int(layers.shape[2]), int(layers.shape[1]), _pf(out)))
    return out


def synthetic(b, samples=9, seed=5):
    """Seeded samples [S, H, W, 4] around the thresholds b that take every branch of the fold: luminances below b[0], exactly b[j]
    for every j (grey samples: the luminance weights sum to 1 in float32 for these values or not — the test asserts what occurred),
    inside every interval, above the top threshold; negative and zero components; inf and NaN components; elements without any
    sample (w == 0) and one element whose every sample is a NaN (n = 0)."""
    rng = np.random.default_rng(seed)
    K = len(b)
    s = np.zeros((samples, H, W, 4), F)
    s[..., 3] = 1
    # log-uniform luminance scale from a quarter of b[0] to four times b[K-1], random chroma
    scale = np.exp(rng.uniform(np.log(b[0] / 4), np.log(b[-1] * 4), (samples, H, W))).astype(F)
    s[..., :3] = (rng.uniform(0.2, 1.8, (samples, H, W, 3)) * scale[..., None]).astype(F)
    flat = s.reshape(-1, 4)
    # exact thresholds: a sample whose three components are powers of two times b[j] need not have luminance b[j]; search one that has
    k = 0
    for j in range(K):
        for g in (b[j], np.nextafter(b[j], F(0)), np.nextafter(b[j], F(np.inf))):
            if luminance(np.array([g, g, g], F)) == b[j]:
                flat[3 * k + 1, :3] = g
                k += 1
                break
    flat[5, :3] = (-1.0, 0.5, 0.0)          # a negative component, luminance above 0
    flat[11, :3] = (-3.0, -2.0, -1.0)       # negative luminance
    flat[17, :3] = 0.0                      # black
    flat[23, :3] = (np.inf, 1.0, 1.0)
    flat[29, :3] = (1.0, -np.inf, 1.0)
    flat[37, :3] = (np.nan, 1.0, 1.0)
    flat[41, :3] = (3.0e38, 3.0e38, 3.0e38)  # finite components, a finite luminance far above the top threshold: clamped
    s[:2, 1, 1, :3] = (3.0e38, -9.0e37, 0.0)  # twice a negative luminance (weight 1 in layer 0) with huge components: the layer's sum
                                              # overflows, its lambda is inf, and the windows that hold it resolve to the plain quotient
    s[:, 2, 3, 3] = 0                       # an element outside the image: never sampled
    s[:, 4, 6, :3] = np.nan                 # every sample dropped: n stays 0
    s[samples // 2:, 0, 0, 3] = 0           # an element that stops receiving samples
    return s


PARAMETERS = [(6, 1.0, 8.0), (2, 0.5, 3.0), (8, 0.01, 2.0), (4, 0.01, 2.0)]


@pytest.mark.parametrize("layers,start,base", PARAMETERS, ids=["default", "K2", "K8", "K4"])
@pytest.mark.parametrize("debug", [False, True], ids=["plain", "debugExceptions"])
def test_fold_and_resolve_equal_the_restatement_bit_for_bit(twk, layers, start, base, debug):
    params = twk._lib.Cascade(layers, start, base)
    b = restate.thresholds(layers, start, base)
    assert len(b) == layers and b[0] == F(start) and b[1] == F(start) * F(base)
    s = synthetic(b)
    zero = np.zeros((layers, H, W, 4), F)
    branches = {}
    expect = restate.fold(s, 0, zero, b, debug, branches)
    got = fold_host(twk, params, s, 0, zero, debug)
    _same(got, expect, "one fold of all samples")
    # every branch occurs
    assert branches["below_start"] > 0 and branches["at_threshold"] >= (2 if layers > 2 else 1) and branches["interior"] > 0 and branches["clamp"] > 0, branches
    if debug:
        assert branches["rejected"] == 0, "under debugExceptions every sample is finite: its false colour"
        assert (got[0, ..., 3] == (s[..., 3] != 0).sum(axis=0)).all()
    else:
        assert branches["rejected"] >= 2 and got[layers - 1, ..., 3].sum() == branches["rejected"]
        assert got[0, 4, 6, 3] == 0 and not got[:, 4, 6].any(), "n = 0: every sample was a NaN"
    assert not got[:, 2, 3].any(), "never sampled"
    assert (got[1:layers - 1, ..., 3] == 0).all(), "the .w of the inner layers stays 0"
    assert all((got[j, ..., :3] != 0).any() for j in range(layers)), "every layer is populated"
    # in two parts, the second continuing at its iteration; and a restart at iteration 0 starts afresh
    part = fold_host(twk, params, s[:4], 0, zero, debug)
    _same(part, restate.fold(s[:4], 0, zero, b, debug), "the first four")
    _same(fold_host(twk, params, s[4:], 4, part, debug), expect, "... continued")
    again = fold_host(twk, params, s, 0, got, debug)
    _same(again, restate.fold(s, 0, got, b, debug), "folded again from iteration 0")
    from test_moments_host import kept_radiance
    afresh = kept_radiance(s[0], debug)[1]  # a kept sample of iteration 0 zeroes the element first
    assert afresh.any() and not afresh.all()
    _same(again[:, afresh], expect[:, afresh], "... which starts the element afresh")

    for kappa in (twk._lib.TWK_CASCADE_KAPPA, 1.0, 1e-6):
        fallback = []
        want = restate.resolve(expect, b, kappa, fallback)
        _same(resolve_host(twk, params, kappa, got), want, f"resolve at kappa {kappa}")
        n = expect[0, ..., 3]
        assert not want[n == 0].any() and (want[n > 0][:, 3] == 1).all()
        if not debug:
            assert fallback[0].any() and not fallback[0].all(), "the windows around the overflowed sum take the plain quotient, the others do not"


def test_a_small_kappa_gives_the_plain_quotient(twk):
    """Every weight is 1 once c_j >= kappa; a layer without energy has c_j that may be below any kappa, but then only when the three
    layers around j are empty in the whole window, and w_j multiplies a layer of zeros."""
    params, b = twk._lib.Cascade(), restate.thresholds()
    s = synthetic(b)
    s[~np.isfinite(s).all(axis=-1) | (s[..., 0] > 1e30)] = (0.25, 0.5, 0.75, 1.0)
    layers = fold_host(twk, params, s, 0, np.zeros((6, H, W, 4), F))
    out = resolve_host(twk, params, 1e-20, layers)
    n = layers[0, ..., 3]
    total = layers[0, ..., :3].copy()
    for j in range(1, 6):
        total = total + layers[j, ..., :3]
    with np.errstate(all="ignore"):
        _same(out[n > 0][:, :3], (total / n[..., None])[n > 0], "kappa 1e-20")


def test_the_layers_count_samples_and_keep_the_energy(twk):
    """For b[0] <= l < b[K-1] a sample adds wLo l / lo + wHi l / hi = 1 to sum_j lambda_j / b_j: per sample three rounded products
    (the weights' quotient, w r, the luminance's) and one sum, so the total is n within (n + 3) 2^-22 n. And below b[K-1] nothing is
    clamped: the layers sum to the f64 sum of the samples within (n + 3) 2^-23 sum |r| per component."""
    K, n = 6, 24
    params, b = twk._lib.Cascade(), restate.thresholds()
    rng = np.random.default_rng(11)
    s = np.ones((n, H, W, 4), F)
    scale = np.exp(rng.uniform(np.log(b[0] * 1.01), np.log(b[-1] * 0.99), (n, H, W)))
    chroma = rng.uniform(0.5, 1.5, (n, H, W, 3))
    chroma /= (0.2126 * chroma[..., 0] + 0.7152 * chroma[..., 1] + 0.0722 * chroma[..., 2])[..., None]
    s[..., :3] = (chroma * scale[..., None]).astype(F)
    l = luminance(s[..., :3])
    assert (l >= b[0]).all() and (l < b[-1]).all()
    layers = fold_host(twk, params, s, 0, np.zeros((K, H, W, 4), F))
    assert (layers[0, ..., 3] == n).all() and not layers[K - 1, ..., 3].any()
    lam = luminance(layers[..., :3]).astype(np.float64)
    counted = (lam / b.astype(np.float64)[:, None, None]).sum(axis=0)
    assert np.abs(counted - n).max() <= (n + 3) * 2.0 ** -22 * n, np.abs(counted - n).max()
    total = layers[..., :3].astype(np.float64).sum(axis=0)
    exact = s[..., :3].astype(np.float64).sum(axis=0)
    bound = (n + 3) * 2.0 ** -23 * np.abs(s[..., :3]).astype(np.float64).sum(axis=0)
    assert (np.abs(total - exact) <= bound).all(), (np.abs(total - exact) / bound).max()
    # with a sample above the top threshold the clamp removes energy, and only there
    s[0, 1, 1, :3] = F(4.0) * b[-1]
    clamped = fold_host(twk, params, s, 0, np.zeros((K, H, W, 4), F))
    assert clamped[..., :3].astype(np.float64).sum(axis=0)[1, 1, 0] < 0.9 * s[:, 1, 1, 0].astype(np.float64).sum()


def test_parameter_refusals(twk):
    L = twk._lib
    s = np.ones((1, 1, 1, 4), F)
    layers = np.zeros((8, 1, 1, 4), F)
    out = np.zeros((1, 1, 4), F)
    inf, nan = float("inf"), float("nan")
    bad = [((1, 1.0, 8.0), "layers"), ((9, 1.0, 8.0), "layers"), ((6, 0.0, 8.0), "start"), ((6, -1.0, 8.0), "start"), ((6, inf, 8.0), "start"), ((6, nan, 8.0), "start"),
           ((6, 1.0, 1.0), "base"), ((6, 1.0, 0.5), "base"), ((6, 1.0, inf), "base"), ((6, 1.0, nan), "base"), ((8, 1e30, 1e3), "reach inf")]
    for args, word in bad:
        p = L.Cascade(*args)
        for name, call in (("twk_cascade_fold_host", lambda: L.lib.twk_cascade_fold_host(C.byref(p), _pf(s), C.c_size_t(1), C.c_size_t(1), C.c_uint(0), 0, _pf(layers))),
                           ("twk_cascade_resolve_host", lambda: L.lib.twk_cascade_resolve_host(C.byref(p), None, _pf(layers), 1, 1, _pf(out)))):
            assert call() == L.TWK_ERROR_INVALID_VALUE, (name, args)
            text = L.lib.twk_last_error().decode()
            assert name in text and word in text, text
    assert L.lib.twk_cascade_fold_host(C.byref(L.Cascade(8, 1e30, 10.0)), _pf(s), C.c_size_t(1), C.c_size_t(1), C.c_uint(0), 0, _pf(layers)) == L.TWK_SUCCESS, "1e37 is finite"
    for kappa in (0.0, -1.0, inf, nan):
        assert L.lib.twk_cascade_resolve_host(None, C.byref(L.CascadeResolve(kappa)), _pf(layers), 1, 1, _pf(out)) == L.TWK_ERROR_INVALID_VALUE
        assert "kappa" in L.lib.twk_last_error().decode()
    assert L.lib.twk_cascade_resolve_host(None, None, _pf(layers), 0, 1, _pf(out)) == L.TWK_ERROR_INVALID_VALUE
    for call in (lambda: L.lib.twk_cascade_fold_host(None, None, C.c_size_t(1), C.c_size_t(1), C.c_uint(0), 0, _pf(layers)),
                 lambda: L.lib.twk_cascade_fold_host(None, _pf(s), C.c_size_t(1), C.c_size_t(1), C.c_uint(0), 0, None),
                 lambda: L.lib.twk_cascade_resolve_host(None, None, None, 1, 1, _pf(out)), lambda: L.lib.twk_cascade_resolve_host(None, None, _pf(layers), 1, 1, None),
                 lambda: L.lib.twk_cascade_defaults(None), lambda: L.lib.twk_cascade_resolve_defaults(None)):
        assert call() == L.TWK_ERROR_INVALID_VALUE and "NULL" in L.lib.twk_last_error().decode()
    # NULL parameters are the defaults, and the defaults are the header's
    cp, rp = L.Cascade(2, 3.0, 4.0), L.CascadeResolve(99.0)
    L.check(L.lib.twk_cascade_defaults(C.byref(cp)))
    L.check(L.lib.twk_cascade_resolve_defaults(C.byref(rp)))
    assert (cp.layers, cp.start, cp.base, rp.kappa) == (L.TWK_CASCADE_LAYERS, L.TWK_CASCADE_START, L.TWK_CASCADE_BASE, L.TWK_CASCADE_KAPPA) == (6, 1.0, 8.0, L.TWK_CASCADE_KAPPA)
    import os
    import re
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "tweeker_hip.h")).read()
    assert float(re.search(r"#define TWK_CASCADE_KAPPA ([0-9.]+)f", header).group(1)) == L.TWK_CASCADE_KAPPA
    assert "#define TWK_ABI_VERSION 9" in header


@pytest.mark.parametrize("name,args", [
    ("twk_enable_cascade", (1, None)), ("twk_read_cascade", (None, C.c_size_t(0))), ("twk_get_cascade_device_pointer", (None, None)),
    ("twk_cascade_resolve", (None, None, None, 0, 0, None)), ("twk_get_resolved_device_pointer", (None, None)), ("twk_read_resolved", (None, C.c_size_t(0)))])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    assert getattr(L.lib, name)(None, *args) == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_ctypes_mirrors_have_the_headers_layout(twk, tmp_path):
    """The two structs, as tests/test_cabi_layouts.py checks the others: sizeof and offsetof out of a C program against ctypes."""
    import test_cabi_layouts as layouts
    pairs = [("TwkCascade", twk._lib.Cascade), ("TwkCascadeResolve", twk._lib.CascadeResolve)]
    saved = layouts.PAIRS
    layouts.PAIRS = pairs
    try:
        layouts.test_ctypes_mirror_has_the_headers_layout(tmp_path)
    finally:
        layouts.PAIRS = saved


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, cp, rp = app.fireflyCascade
        return (on, cp.layers, cp.start, cp.base, rp.kappa), app.systemDescription()
    finally:
        app.close()


def test_cascade_keys_of_the_system_description(twk):
    L = twk._lib
    defaults = (False, 6, 1.0, 8.0, L.TWK_CASCADE_KAPPA)
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    off, text = _description(twk, base)
    assert off == defaults and "fireflyCascade" not in text
    assert _description(twk, text) == (off, text)
    assert _description(twk, base + f"\nfireflyCascade 0\nfireflyCascadeLayers 6\nfireflyCascadeStart 1\nfireflyCascadeBase 8\nfireflyCascadeKappa {L.TWK_CASCADE_KAPPA}\n") == (off, text)
    on, on_text = _description(twk, base + "\nfireflyCascade 1\nfireflyCascadeLayers 4\nfireflyCascadeStart 0.5\nfireflyCascadeBase 2\nfireflyCascadeKappa 16\n")
    assert on == (True, 4, 0.5, 2.0, 16.0)
    for line in ("fireflyCascade 1", "fireflyCascadeLayers 4", "fireflyCascadeStart 0.5", "fireflyCascadeBase 2", "fireflyCascadeKappa 16"):
        assert line + "\n" in on_text
    assert _description(twk, on_text) == (on, on_text)
    only, only_text = _description(twk, base + "\nfireflyCascade 1\n")
    assert only == (True,) + defaults[1:] and "fireflyCascade 1\n" in only_text and "fireflyCascadeLayers" not in only_text and "fireflyCascadeKappa" not in only_text
    # a value the calls would refuse drops the line
    for bad in ("fireflyCascadeLayers 1", "fireflyCascadeLayers 9", "fireflyCascadeStart 0", "fireflyCascadeStart -2", "fireflyCascadeBase 1", "fireflyCascadeBase 0.5",
                "fireflyCascadeKappa 0", "fireflyCascadeKappa -1"):
        assert _description(twk, base + "\nfireflyCascade 1\n" + bad + "\n")[0] == only, bad
    # thresholds that reach inf: all three dropped, in whichever order they came
    assert _description(twk, base + "\nfireflyCascade 1\nfireflyCascadeBase 1e6\nfireflyCascadeLayers 8\nfireflyCascadeStart 1e10\n")[0] == only
