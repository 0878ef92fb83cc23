"""The planned adaptive pass (twk_adaptive_plan, csrc/adaptive_plan_device.h) where it needs no GPU: twk_adaptive_plan_host equals
tests/adaptive_plan_restate.py word for word on crafted moments (e at the target and one ulp above it, a ratio that overflows, values
that are not finite, padding, the sample cap) and on a random field; the plan's list is the select's list, its offsets the
exclusive sum of the budgets, the budget grows with e; the new entry points refuse a NULL handle and bad parameters before any HIP
call; and the system description's `adaptiveBudget`, `adaptiveMinBatch`, `adaptiveMaxBatch` keys are read, dropped when invalid, and
written back only when they differ from the defaults."""
import ctypes as C

import numpy as np
import pytest

import adaptive_plan_restate as apr
import adaptive_restate as ar
import noise_restate as nr
from conftest import scene_path

F = np.float32
U32 = C.POINTER(C.c_uint32)
SENTINEL = 0xFFFFFFFF


def _plan_host(L, ap, pl, moments, counts, code=None):
    moments = np.ascontiguousarray(moments, F)
    counts = np.ascontiguousarray(counts, np.uint32)
    active = np.full(counts.size, SENTINEL, np.uint32)
    offsets = np.full(counts.size + 1, SENTINEL, np.uint32)
    n, paths = C.c_size_t(0), C.c_ulonglong(0)
    rc = L.lib.twk_adaptive_plan_host(None if ap is None else C.byref(ap), None if pl is None else C.byref(pl), moments.ctypes.data_as(C.POINTER(C.c_float)),
                                      counts.ctypes.data_as(U32), C.c_size_t(counts.size), active.ctypes.data_as(U32), offsets.ctypes.data_as(U32), C.byref(n), C.byref(paths))
    if code is not None:
        assert rc == code
        return None
    L.check(rc)
    assert (active[n.value:] == SENTINEL).all() and (offsets[n.value + 1:] == SENTINEL).all()  # nothing is written beyond the plan
    return active[:n.value], offsets[:n.value + 1], paths.value


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _budget_of(plan, n):
    """uint32 [n]: the budget of every element, from a plan."""
    b = np.zeros(n, np.uint32)
    b[plan[0]] = np.diff(plan[1].astype(np.int64)).astype(np.uint32)
    return b


def _ulp_above(target, floor=F(0.01)):
    """M2 of a triple (1 - floor, M2, 4) whose e is the float32 next above `target`: the first M2 above 12 target^2 that passes it."""
    m2 = F(12.0) * F(target) * F(target)
    for _ in range(64):
        m2 = np.nextafter(m2, F(np.inf))
        _, e = nr.classify(np.array([[F(1.0) - floor, m2, 4, 0]], F), 4, floor)
        if e[0] > F(target):
            assert e[0] == np.nextafter(F(target), F(np.inf))
            return m2
    raise AssertionError("no M2 gives the next e above the target")


def test_crafted_elements(twk):
    L = twk._lib
    t, floor = F(2.0 ** -4), F(0.01)
    one = F(1.0) - floor  # mean + floor = 1 in float32 arithmetic
    nan, inf = np.nan, np.inf
    ap = L.Adaptive(targetNoise=float(t), minSamples=4, darkFloor=float(floor), maxSamples=100)
    pl = L.AdaptivePlan(minBatch=3, maxBatch=40)
    rows = [
        ([one, F(12.0) * t * t, 4, 0], 0, 0),             # e == target: done
        ([one, _ulp_above(t), 4, 0], 0, 3),               # one ulp above: the prediction is below one sample, minBatch
        ([one, F(12.0) * F(4.0) * t * t, 4, 0], 0, 12),   # e = 2 target: 4 x 4 - 4
        ([one, F(12.0) * F(4.0) * t * t, 4, 0], 95, 5),   # ... clipped by the room the cap leaves
        ([one, F(12.0) * F(16.0) * t * t, 4, 0], 0, 40),  # e = 4 target: 60 more, maxBatch
        ([one, F(12.0) * F(16.0) * t * t, 4, 0], 99, 1),  # count = maxSamples - 1 with a large prediction
        ([one, F(12.0) * F(16.0) * t * t, 4, 0], 100, 0), ([one, F(12.0) * F(16.0) * t * t, 4, 0], 101, 0), ([one, 1, 4, 0], SENTINEL, 0),  # count >= maxSamples
        ([nan, 1, 8, 0], 0, 3), ([1, nan, 8, 0], 0, 3), ([1, 1, nan, 0], 0, 3), ([inf, 1, 8, 0], 0, 3), ([1, inf, 8, 0], 0, 3), ([1, 1, inf, 0], 0, 3),
        ([-1, 1, 8, 0], 0, 3), ([1, -1, 8, 0], 0, 3), ([1, 1, 3, 0], 0, 3), ([nan, 1, 8, 0], 98, 2),  # unknown: minBatch, within the cap
        ([1, 1, 0, 0], 0, 0), ([nan, inf, -0.0, 0], 0, 0),  # padding: n == 0
    ]
    m = np.array([r[0] for r in rows], F)
    counts = np.array([r[1] for r in rows], np.uint32)
    want = np.array([r[2] for r in rows], np.uint32)
    cls, e = nr.classify(m, 4, floor)
    assert e[0] == t and e[2] == F(2.0) * t and e[4] == F(4.0) * t  # the rows are what their comments say
    restated = apr.budgets(m, counts, **apr.parameters(ap, pl))
    assert restated.tolist() == want.tolist()
    got = _plan_host(L, ap, pl, m, counts)
    assert _same(got, apr.plan(m, counts, **apr.parameters(ap, pl)))
    assert _budget_of(got, len(rows)).tolist() == want.tolist()
    # one ulp above a target that is no power of two, whatever e / target rounds to: still minBatch
    for target in (0.05, 0.07, 0.3):
        ap2 = L.Adaptive(targetNoise=target, darkFloor=float(floor), maxSamples=100)
        m2 = np.array([[one, _ulp_above(F(target)), 4, 0]], F)
        assert apr.budgets(m2, [0], **apr.parameters(ap2, pl)).tolist() == [3]
        assert _same(_plan_host(L, ap2, pl, m2, [0]), apr.plan(m2, [0], **apr.parameters(ap2, pl)))


def test_a_ratio_that_overflows_gets_the_largest_batch(twk):
    L = twk._lib
    tiny = 1e-38  # positive and finite in float32
    ap = L.Adaptive(targetNoise=tiny, maxSamples=1000)
    pl = L.AdaptivePlan(minBatch=1, maxBatch=64)
    one = F(1.0) - F(0.01)
    m = np.array([[one, 12 * 1e6, 4, 0],     # e = 1000: e / target is infinite
                  [one, 12 * 4, 4, 0],       # e = 2: the ratio is finite, its square is not
                  [one, 12 * 1e-60, 4, 0]], F)  # M2 underflows to 0: e = 0, not selected
    with np.errstate(all="ignore"):
        _, e = nr.classify(m)
        r = e / F(tiny)
        assert np.isinf(r[0]) and np.isfinite(r[1]) and np.isinf(r[1] * r[1])
    want = apr.plan(m, [0, 0, 0], **apr.parameters(ap, pl))
    assert _budget_of(want, 3).tolist() == [64, 64, 0]
    assert _same(_plan_host(L, ap, pl, m, [0, 0, 0]), want)


def test_random_field_equals_the_restatement_and_the_selects_list(twk):
    L = twk._lib
    rng = np.random.default_rng(14)
    n = 5000
    for (target, min_samples, floor, cap), (lo, hi) in zip(((0.05, 4, 0.01, 4096), (0.125, 2, 0.01, 10), (2.0 ** -6, 8, 0.5, 3), (1.0, 4, 2.0 ** -10, 70)),
                                                           ((4, 64), (1, 7), (2, 2), (64, 64))):
        ap = L.Adaptive(targetNoise=target, minSamples=min_samples, darkFloor=floor, maxSamples=cap)
        pl = L.AdaptivePlan(minBatch=lo, maxBatch=hi)
        moments = ar.mixed_moments(rng, n, target, min_samples, floor)
        counts = rng.choice([0, 1, cap - 1, cap, cap + 1, SENTINEL], n).astype(np.uint32)
        want = apr.plan(moments, counts, **apr.parameters(ap, pl))
        got = _plan_host(L, ap, pl, moments, counts)
        assert _same(got, want)
        active, offsets, paths = got
        assert np.array_equal(active, ar.active_list(moments, counts, **ar.parameters(ap)))  # the plan's list IS the select's list
        b = apr.budgets(moments, counts, **apr.parameters(ap, pl))
        assert offsets[0] == 0 and np.array_equal(offsets[1:].astype(np.int64), np.cumsum(b[active].astype(np.int64))) and int(offsets[-1]) == paths == int(b.sum())
        assert (b[active] >= 1).all() and (b[active] <= hi).all() and (counts[active].astype(np.int64) + b[active] <= cap).all()
        cls, _ = nr.classify(moments, min_samples, floor)
        assert not b[cls == nr.EMPTY].any() and not b[counts >= cap].any()
    # ap and plan NULL: the defaults
    moments = ar.mixed_moments(rng, n)
    counts = rng.integers(0, 8192, n).astype(np.uint32)
    assert _same(_plan_host(L, None, None, moments, counts), apr.plan(moments, counts))
    assert len(set(apr.budgets(moments, counts).tolist())) >= 4


def test_budget_does_not_fall_as_the_error_grows(twk):
    L = twk._lib
    ap = L.Adaptive(targetNoise=0.05, maxSamples=4096)
    pl = L.AdaptivePlan(minBatch=2, maxBatch=48)
    for n in (4, 16, 61):
        m = np.zeros((4000, 4), F)
        m[:, 0] = F(1.0) - F(0.01)
        m[:, 2] = n
        m[:, 1] = (np.linspace(0.04, 0.5, 4000).astype(F) ** 2) * F((n - 1) * n)
        _, e = nr.classify(m)
        assert (np.diff(e) >= 0).all()
        b = _budget_of(_plan_host(L, ap, pl, m, np.zeros(4000, np.uint32)), 4000).astype(np.int64)
        assert (np.diff(b) >= 0).all(), n
        assert b[0] == 0 and b[-1] == 48 and 2 in b and len(set(b.tolist())) > 10


def _bad_plans(L):
    return [L.AdaptivePlan(0, 4), L.AdaptivePlan(0, 0), L.AdaptivePlan(5, 4), L.AdaptivePlan(1, 65), L.AdaptivePlan(65, 65), L.AdaptivePlan(64, 1), L.AdaptivePlan(SENTINEL, SENTINEL)]


def _bad_parameters(L):
    nan, inf = float("nan"), float("inf")
    return [L.Adaptive(targetNoise=0.0), L.Adaptive(targetNoise=nan), L.Adaptive(targetNoise=inf), L.Adaptive(minSamples=1), L.Adaptive(darkFloor=0.0),
            L.Adaptive(darkFloor=nan), L.Adaptive(maxSamples=0)]


def test_refusals_of_the_host_call(twk):
    L = twk._lib
    m, c = np.zeros((1, 4), F), np.zeros(1, np.uint32)
    for bad in _bad_plans(L):
        _plan_host(L, None, bad, m, c, code=L.TWK_ERROR_INVALID_VALUE)
        text = L.lib.twk_last_error().decode()
        assert "twk_adaptive_plan_host" in text and "minBatch" in text
    for bad in _bad_parameters(L):
        _plan_host(L, bad, None, m, c, code=L.TWK_ERROR_INVALID_VALUE)
        assert "twk_adaptive_plan_host" in L.lib.twk_last_error().decode()
    for ok in (L.AdaptivePlan(1, 1), L.AdaptivePlan(64, 64), L.AdaptivePlan(1, 64)):
        _plan_host(L, None, ok, m, c)
    n, paths, one, word = C.c_size_t(0), C.c_ulonglong(0), (C.c_float * 4)(), (C.c_uint32 * 2)()
    good = [None, None, one, word, C.c_size_t(1), word, word, C.byref(n), C.byref(paths)]
    for missing in (2, 3, 5, 6, 7, 8):
        args = list(good)
        args[missing] = None
        assert L.lib.twk_adaptive_plan_host(*args) == L.TWK_ERROR_INVALID_VALUE
        assert "twk_adaptive_plan_host" in L.lib.twk_last_error().decode()
    args = list(good)
    args[4] = C.c_size_t((1 << 31) + 1)
    assert L.lib.twk_adaptive_plan_host(*args) == L.TWK_ERROR_INVALID_VALUE


@pytest.mark.parametrize("name,args", [
    ("twk_adaptive_plan", (None, None, None, None, C.c_size_t(0), None, None, C.byref(C.c_uint(0)), C.byref(C.c_ulonglong(0)))),
    ("twk_launch_adaptive_planned", ()),
    ("twk_read_plan", (None, None, C.c_size_t(0), C.byref(C.c_uint(0)), C.byref(C.c_ulonglong(0)))),
    ("twk_app_get_adaptive_plan", (None, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    assert getattr(L.lib, name)(None, *args) == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_parameters_are_refused_before_any_device_call(twk):
    L = twk._lib
    handle = C.c_void_p(1)  # never dereferenced: the parameters are checked first
    n, paths = C.c_uint(0), C.c_ulonglong(0)
    plan = L.lib.twk_adaptive_plan

    def refused(ap, pl, m, c, count, a, o, nn=C.byref(n), pp=C.byref(paths), word=None):
        assert plan(handle, ap, pl, m, c, C.c_size_t(count), a, o, nn, pp) == L.TWK_ERROR_INVALID_VALUE
        text = L.lib.twk_last_error().decode()
        assert "twk_adaptive_plan" in text and (word is None or word in text), text

    for bad in _bad_plans(L):
        refused(None, C.byref(bad), None, None, 0, None, None, word="minBatch")
    for bad in _bad_parameters(L):
        refused(C.byref(bad), None, None, None, 0, None, None)
    refused(None, None, None, None, 0, None, None, nn=None)
    refused(None, None, None, None, 0, None, None, pp=None)
    m, c, a, o = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    for count in (0, (1 << 31) + 1):
        refused(None, None, m, c, count, a, o)
    refused(None, None, None, None, 5, None, None)  # a count without buffers
    for k in range(1, 15):  # some but not all of the four pointers
        refused(None, None, *[p if (k >> j) & 1 else None for j, p in enumerate((m, c))], 16, *[p if (k >> (j + 2)) & 1 else None for j, p in enumerate((a, o))])
    # overlaps at 100 elements: either output inside the moments (16 bytes each) or the counts, ending one word into either, and
    # the offsets (101 words) reaching one word into the list or the list one word into the offsets
    base = 1 << 20
    for at in (base, base + 16 * 100 - 4, (2 << 20) + 4 * 99, (2 << 20) - 4 * 100 + 4):
        refused(None, None, m, c, 100, C.c_void_p(at), o, word="activeOut overlaps an input")
    for at in (base, base + 16 * 100 - 4, (2 << 20) + 4 * 99, (2 << 20) - 4 * 101 + 4):
        refused(None, None, m, c, 100, a, C.c_void_p(at), word="pathOffsetOut overlaps an input")
    for at in ((3 << 20) - 4 * 100, (3 << 20) + 4 * 99):
        refused(None, None, m, c, 100, a, C.c_void_p(at), word="activeOut overlaps pathOffsetOut")
    assert L.lib.twk_adaptive_plan_defaults(None) == L.TWK_ERROR_INVALID_VALUE and "twk_adaptive_plan_defaults" in L.lib.twk_last_error().decode()


def test_defaults_and_layout(twk):
    L = twk._lib
    pl = L.AdaptivePlan(minBatch=9, maxBatch=9)
    L.check(L.lib.twk_adaptive_plan_defaults(C.byref(pl)))
    assert (pl.minBatch, pl.maxBatch) == (L.TWK_DENOISER_MIN_SAMPLES, 64)
    fresh = L.AdaptivePlan()
    assert (fresh.minBatch, fresh.maxBatch) == (pl.minBatch, pl.maxBatch)
    assert C.sizeof(L.AdaptivePlan) == 8 and [(name, getattr(L.AdaptivePlan, name).offset) for name, _ in L.AdaptivePlan._fields_] == [("minBatch", 0), ("maxBatch", 4)]
    assert L.lib.twk_abi_version() == 9


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, pl = app.adaptivePlan
        return (on, pl.minBatch, pl.maxBatch), app.systemDescription()
    finally:
        app.close()


def test_plan_keys_of_the_system_description(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    defaults = (False, 4, 64)
    off, text = _description(twk, base)
    assert off == defaults and "adaptiveBudget" not in text and "Batch" not in text
    assert _description(twk, base + "\nadaptiveBudget 0\nadaptiveMinBatch 4\nadaptiveMaxBatch 64\n") == (off, text)
    # in effect only where adaptive sampling itself is: the key alone, or with a target but without "adaptiveSampling 1", is kept but off
    alone, alone_text = _description(twk, base + "\nadaptiveBudget 1\n")
    assert alone == defaults and alone_text.count("adaptiveBudget 1\n") == 1
    assert _description(twk, base + "\nadaptiveBudget 1\ntargetNoise 0.125\n")[0] == defaults
    adaptive = "\ntargetNoise 0.125\nadaptiveSampling 1\n"
    assert _description(twk, base + adaptive)[0] == defaults
    on, on_text = _description(twk, base + adaptive + "adaptiveBudget 1\n")
    assert on == (True, 4, 64) and on_text.count("adaptiveBudget 1\n") == 1 and "Batch" not in on_text
    assert _description(twk, on_text) == (on, on_text)
    custom, custom_text = _description(twk, base + adaptive + "adaptiveBudget 1\nadaptiveMaxBatch 7\nadaptiveMinBatch 1\n")
    assert custom == (True, 1, 7) and "adaptiveMinBatch 1\n" in custom_text and "adaptiveMaxBatch 7\n" in custom_text
    assert _description(twk, custom_text) == (custom, custom_text)
    # a value outside 1..64 drops the line, the previous value stays; a minimum above the maximum drops both
    assert _description(twk, base + "\nadaptiveMinBatch 0\n")[0] == defaults
    assert _description(twk, base + "\nadaptiveMaxBatch 65\n")[0] == defaults
    assert _description(twk, base + "\nadaptiveMaxBatch 32\nadaptiveMaxBatch -1\nadaptiveMinBatch 8\nadaptiveMinBatch 100\n")[0] == (False, 8, 32)
    assert _description(twk, base + "\nadaptiveMinBatch 9\nadaptiveMaxBatch 8\n")[0] == defaults
    assert _description(twk, base + "\nadaptiveMaxBatch 2\n")[0] == defaults  # below the default minimum of 4
    assert _description(twk, base + "\nadaptiveMaxBatch 2\nadaptiveMinBatch 2\n")[0] == (False, 2, 2)
