"""Adaptive sampling (twk_adaptive_select, csrc/adaptive_device.h) where it needs no GPU: the new entry points refuse a NULL handle
and bad parameters before any HIP call, the defaults and the struct are what the header says, twk_adaptive_select_host equals
tests/adaptive_restate.py on moments that mix every class, and the system description's `adaptive*` keys are read, dropped when
invalid or without a target, and written back only when they differ from the defaults."""
import ctypes as C

import numpy as np
import pytest

import adaptive_restate as ar
import noise_restate as nr
from conftest import scene_path

F = np.float32


@pytest.mark.parametrize("name,args", [
    ("twk_enable_adaptive", (1,)),
    ("twk_adaptive_select", (None, None, None, C.c_size_t(0), None, C.byref(C.c_uint(0)))),
    ("twk_launch_adaptive", (1,)),
    ("twk_read_sample_counts", (None, C.c_size_t(0))),
    ("twk_get_sample_counts_device_pointer", (None, None)),
    ("twk_read_active", (None, C.c_size_t(0), None)),
    ("twk_app_get_adaptive", (None, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    rc = getattr(L.lib, name)(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def _bad_parameters(L):
    nan, inf = float("nan"), float("inf")
    return [L.Adaptive(targetNoise=0.0), L.Adaptive(targetNoise=-1.0), L.Adaptive(targetNoise=nan), L.Adaptive(targetNoise=inf),
            L.Adaptive(minSamples=1), L.Adaptive(minSamples=0), L.Adaptive(darkFloor=0.0), L.Adaptive(darkFloor=-1.0),
            L.Adaptive(darkFloor=inf), L.Adaptive(darkFloor=nan), L.Adaptive(maxSamples=0)]


def test_parameters_are_refused_before_any_device_call(twk):
    L = twk._lib
    handle = C.c_void_p(1)  # never dereferenced: the parameters are checked first
    n = C.c_uint(0)
    select = L.lib.twk_adaptive_select
    for bad in _bad_parameters(L):
        assert select(handle, C.byref(bad), None, None, C.c_size_t(0), None, C.byref(n)) == L.TWK_ERROR_INVALID_VALUE
        assert "twk_adaptive_select" in L.lib.twk_last_error().decode()
    assert select(handle, None, None, None, C.c_size_t(0), None, None) == L.TWK_ERROR_INVALID_VALUE  # nowhere to write the count
    m, c, a = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    for count in (0, (1 << 31) + 1):  # explicit buffers: 1 .. 2^31 elements
        assert select(handle, None, m, c, C.c_size_t(count), a, C.byref(n)) == L.TWK_ERROR_INVALID_VALUE
    assert select(handle, None, None, None, C.c_size_t(5), None, C.byref(n)) == L.TWK_ERROR_INVALID_VALUE  # a count without buffers
    for partial in ((m, None, None), (None, c, None), (None, None, a), (m, c, None), (m, None, a), (None, c, a)):
        assert select(handle, None, partial[0], partial[1], C.c_size_t(16), partial[2], C.byref(n)) == L.TWK_ERROR_INVALID_VALUE
    # overlaps: the list inside the moments (16 bytes each), inside the counts, and ending one word into either
    base = 1 << 20
    for active in (base, base + 16 * 100 - 4, (2 << 20) + 4 * 99, (2 << 20) - 4 * 100 + 4):
        assert select(handle, None, m, c, C.c_size_t(100), C.c_void_p(active), C.byref(n)) == L.TWK_ERROR_INVALID_VALUE, hex(active)
        assert "overlaps" in L.lib.twk_last_error().decode()
    for samples in (0, -1, 65):
        assert L.lib.twk_launch_adaptive(handle, samples) == L.TWK_ERROR_INVALID_VALUE
        assert "twk_launch_adaptive" in L.lib.twk_last_error().decode()


def test_defaults_and_layout(twk):
    L = twk._lib
    ap = L.Adaptive(targetNoise=9.0, minSamples=99, darkFloor=7.0, maxSamples=1)
    L.check(L.lib.twk_adaptive_defaults(C.byref(ap)))
    assert (F(ap.targetNoise), ap.minSamples, F(ap.darkFloor), ap.maxSamples) == (F(0.05), L.TWK_DENOISER_MIN_SAMPLES, F(L.TWK_NOISE_DARK_FLOOR), 4096)
    assert L.lib.twk_adaptive_defaults(None) == L.TWK_ERROR_INVALID_VALUE and "twk_adaptive_defaults" in L.lib.twk_last_error().decode()
    fresh = L.Adaptive()
    assert (F(fresh.targetNoise), fresh.minSamples, F(fresh.darkFloor), fresh.maxSamples) == (F(ap.targetNoise), ap.minSamples, F(ap.darkFloor), ap.maxSamples)
    assert C.sizeof(L.Adaptive) == 16
    assert [(name, getattr(L.Adaptive, name).offset) for name, _ in L.Adaptive._fields_] == [("targetNoise", 0), ("minSamples", 4), ("darkFloor", 8), ("maxSamples", 12)]
    assert L.lib.twk_abi_version() == 9


def _select_host(L, ap, moments, counts):
    moments = np.ascontiguousarray(moments, F)
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.full(counts.size, 0xFFFFFFFF, np.uint32)
    n = C.c_size_t(0)
    L.check(L.lib.twk_adaptive_select_host(None if ap is None else C.byref(ap), moments.ctypes.data_as(C.POINTER(C.c_float)), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           C.c_size_t(counts.size), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
    assert (out[n.value:] == 0xFFFFFFFF).all()  # nothing is written beyond the list
    return out[:n.value]


def test_host_select_equals_the_restatement(twk):
    L = twk._lib
    rng = np.random.default_rng(11)
    for target, min_samples, floor, cap in ((0.05, 4, 0.01, 4096), (0.125, 2, 0.01, 10), (2.0 ** -6, 8, 0.5, 3), (1.0, 4, 2.0 ** -10, 1)):
        ap = L.Adaptive(targetNoise=target, minSamples=min_samples, darkFloor=floor, maxSamples=cap)
        moments = ar.mixed_moments(rng, 20000, target, min_samples, floor)
        counts = rng.choice([0, 1, cap - 1, cap, cap + 1, 0xFFFFFFFF], 20000).astype(np.uint32)
        cls, e = nr.classify(moments, min_samples, floor)
        want = ar.selected(moments, counts, **ar.parameters(ap))
        # the mix holds every class on both sides of the cap, and valid elements above, below and exactly at the target
        for c in (nr.EMPTY, nr.UNKNOWN, nr.VALID):
            assert ((cls == c) & (counts < cap)).any() and ((cls == c) & (counts >= cap)).any()
        below = counts < cap
        assert ((cls == nr.VALID) & below & (e == F(target))).any() and ((cls == nr.VALID) & below & (e > F(target))).any() and ((cls == nr.VALID) & below & (e < F(target))).any()
        assert not want[cls == nr.EMPTY].any() and not want[counts >= cap].any()
        assert want[(cls == nr.UNKNOWN) & below].all() and not want[(cls == nr.VALID) & (e == F(target))].any()
        got = _select_host(L, ap, moments, counts)
        assert np.array_equal(got, np.flatnonzero(want).astype(np.uint32))
        assert np.array_equal(got, ar.active_list(moments, counts, **ar.parameters(ap)))
    # ap NULL: the defaults
    moments = ar.mixed_moments(rng, 5000)
    counts = rng.integers(0, 8192, 5000).astype(np.uint32)
    assert np.array_equal(_select_host(L, None, moments, counts), ar.active_list(moments, counts))
    # refusals of the host form
    n, one, word = C.c_size_t(0), (C.c_float * 4)(), (C.c_uint32 * 1)()
    for bad in _bad_parameters(L):
        assert L.lib.twk_adaptive_select_host(C.byref(bad), one, word, C.c_size_t(1), word, C.byref(n)) == L.TWK_ERROR_INVALID_VALUE
    assert L.lib.twk_adaptive_select_host(None, None, word, C.c_size_t(1), word, C.byref(n)) == L.TWK_ERROR_INVALID_VALUE
    assert "twk_adaptive_select_host" in L.lib.twk_last_error().decode()


def test_restated_order_of_the_tests():
    """The restatement's own rules on hand-made elements: empty before the cap, the cap before unknown, strictly above the target."""
    nan = float("nan")
    m = np.array([[1, 1, 0, 0], [nan, 1, -0.0, 0],            # empty whatever else holds
                  [1, 1, 3, 0], [nan, 1, 8, 0],                # unknown: selected below the cap
                  [0.99, 12, 4, 0], [0.99, 12, 4, 0], [0.99, 12, 4, 0], [0.99, 0, 4, 0]], F)  # e = 1, 1, 1, 0
    counts = np.array([0, 0, 5, 9, 5, 5, 10, 5], np.uint32)
    sel = lambda t, cap=10: ar.selected(m, counts, target_noise=t, max_samples=cap).tolist()
    assert sel(0.5) == [False, False, True, True, True, True, False, False]
    assert sel(1.0) == [False, False, True, True, False, False, False, False]  # e == target is done
    assert sel(0.5, cap=9) == [False, False, True, False, True, True, False, False]  # the cap ends an unknown pixel too
    assert ar.active_list(m, counts, target_noise=0.5, max_samples=10).tolist() == [2, 3, 4, 5]


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, ap = app.adaptive
        return (on, F(ap.targetNoise), ap.minSamples, F(ap.darkFloor), ap.maxSamples), app.systemDescription()
    finally:
        app.close()


def test_adaptive_keys_of_the_system_description(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    defaults = (False, F(0.05), 4, F(0.01), 4096)
    off, text = _description(twk, base)
    assert off == defaults and "adaptive" not in text
    assert _description(twk, text) == (off, text)
    assert _description(twk, base + "\nadaptiveSampling 0\nadaptiveMaxSamples 4096\n") == (off, text)
    # the key takes effect only with a target, in either order of the two lines; the target is the stopping rule's
    for lines in ("\ntargetNoise 0.125\nadaptiveSampling 1\n", "\nadaptiveSampling 1\ntargetNoise 0.125\n"):
        on, on_text = _description(twk, base + lines)
        assert on == (True, F(0.125), 4, F(0.01), 4096)
        assert on_text.count("adaptiveSampling 1\n") == 1 and "adaptiveMaxSamples" not in on_text
        assert on_text.replace("adaptiveSampling 1\n", "").replace("targetNoise 0.125\n", "") == text
        assert _description(twk, on_text) == (on, on_text)
    dropped, dropped_text = _description(twk, base + "\nadaptiveSampling 1\n")
    assert dropped == defaults and dropped_text == text
    assert _description(twk, base + "\nadaptiveSampling 1\ntargetNoise 0.25\ntargetNoise 0\n")[0][0] is False
    # a target without the key: the target is handed out, the switch is off
    assert _description(twk, base + "\ntargetNoise 0.25\n")[0] == (False, F(0.25), 4, F(0.01), 4096)
    custom, custom_text = _description(twk, base + "\ntargetNoise 0.0625\nadaptiveSampling 1\nadaptiveMaxSamples 300\n")
    assert custom == (True, F(0.0625), 4, F(0.01), 300) and custom_text.count("adaptiveMaxSamples 300\n") == 1
    assert _description(twk, custom_text) == (custom, custom_text)
    # a value the calls would refuse drops the line, the previous value stays
    assert _description(twk, base + "\nadaptiveMaxSamples 0\n")[0] == defaults
    assert _description(twk, base + "\nadaptiveMaxSamples 64\nadaptiveMaxSamples -3\n")[0] == (False, F(0.05), 4, F(0.01), 64)
    kept, kept_text = _description(twk, base + "\nadaptiveMaxSamples 1\n")
    assert kept == (False, F(0.05), 4, F(0.01), 1) and "adaptiveMaxSamples 1\n" in kept_text and "adaptiveSampling" not in kept_text
