"""-m gpu: twk_adaptive_plan (csrc/adaptive_plan_kernels.hip) against tests/adaptive_plan_restate.py, word for word in the list, the
path offsets and both totals: the explicit form on synthetic buffers of every size at which the compaction and the scans take another
path (a part of a wave, whole waves, a part of a tile, several tiles, more tiles than the scan block has lanes, so that its carry is
crossed), filled from a seeded generator that mixes all three classes and many budgets, its inputs unwritten; every element at the
largest batch (tile sums at their maximum); nothing selected, whose planned launch is a successful no-op."""
import numpy as np
import pytest

import adaptive_plan_restate as apr
import adaptive_restate as ar
import noise_restate as nr
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
TILE = 1024  # elements per tile; the scan block takes 1024 tiles at a time
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 65537, 1048577]
assert (SIZES[-1] + TILE - 1) // TILE > 1024
TARGET, CAP = 0.05, 100
SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def small_device(twk):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    dev.enableAdaptive(True)
    yield dev
    dev.close()


def _mixed(rng, n):
    """Moments of every class (adaptive_restate.mixed_moments) whose valid errors are spread from a quarter of the target to
    twelve times it, so that the budgets take many values, and counts on both sides of the cap."""
    m = ar.mixed_moments(rng, n, TARGET)
    m[:, 1] *= rng.uniform(1.0, 9.0, n).astype(F)
    counts = rng.choice([0, 1, 7, CAP - 9, CAP - 1, CAP, CAP + 1, SENTINEL], n).astype(np.uint32)
    return m, counts


def _run(twk, dev, ap, pl, m, counts):
    """The explicit form on fresh device buffers; returns (numActive, numPaths, active [n], pathOffset [n + 1]) and checks that the
    inputs were not written."""
    n = counts.size
    d_moments, d_counts, d_active, d_offsets = _DeviceBuffer(twk, n * 16), _DeviceBuffer(twk, n * 4), _DeviceBuffer(twk, n * 4), _DeviceBuffer(twk, (n + 1) * 4)
    try:
        d_moments.upload(m)
        d_counts.upload(counts)
        d_active.upload(np.full(n, SENTINEL, np.uint32))
        d_offsets.upload(np.full(n + 1, SENTINEL, np.uint32))
        num_active, num_paths = dev.adaptivePlan(ap, pl, d_moments.ptr.value, d_counts.ptr.value, n, d_active.ptr.value, d_offsets.ptr.value)
        active, offsets = d_active.download((n,), np.uint32), d_offsets.download((n + 1,), np.uint32)
        assert np.array_equal(d_moments.download(m.shape, np.uint32), m.view(np.uint32)), "the moments were written"
        assert np.array_equal(d_counts.download(counts.shape, np.uint32), counts), "the counts were written"
        return num_active, num_paths, active, offsets
    finally:
        d_moments.free(); d_counts.free(); d_active.free(); d_offsets.free()


def _compare(got, want, name):
    num_active, num_paths, active, offsets = got
    w_active, w_offsets, w_paths = want
    assert (num_active, num_paths) == (w_active.size, w_paths), name
    for label, g, w in (("active", active[:num_active], w_active), ("pathOffset", offsets[:num_active + 1], w_offsets)):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{name}: {bad.size} words of {label} differ, first at {bad[:4].tolist()}: {g[bad[:4]].tolist()} for {w[bad[:4]].tolist()}"
    assert (active[num_active:] == SENTINEL).all() and (offsets[num_active + 1:] == SENTINEL).all(), f"{name}: written beyond the plan"


@pytest.mark.parametrize("n", SIZES)
def test_explicit_buffers_equal_the_restatement(twk, small_device, n):
    rng = np.random.default_rng(n)
    ap = twk.Adaptive(targetNoise=TARGET, maxSamples=CAP)
    for lo, hi in ((4, 64), (1, 7)):
        pl = twk.AdaptivePlan(minBatch=lo, maxBatch=hi)
        m, counts = _mixed(rng, n)
        want = apr.plan(m, counts, **apr.parameters(ap, pl))
        if n >= 1023:  # the field holds every class, selected and not, and more than two budgets
            cls, _ = nr.classify(m)
            b = apr.budgets(m, counts, **apr.parameters(ap, pl))
            assert all(((cls == c) & (b > 0)).any() for c in (nr.VALID, nr.UNKNOWN)) and all(((cls == c) & (b == 0)).any() for c in (nr.VALID, nr.UNKNOWN, nr.EMPTY))
            assert len(set(b.tolist())) >= 5
        _compare(_run(twk, small_device, ap, pl, m, counts), want, f"n {n} batch {lo}..{hi}")


def test_every_element_at_the_largest_batch(twk, small_device):
    n = SIZES[-1]
    ap = twk.Adaptive(targetNoise=2.0 ** -4, maxSamples=4096)
    pl = twk.AdaptivePlan(minBatch=1, maxBatch=64)
    m = np.zeros((n, 4), F)
    m[:] = [F(1.0) - F(0.01), F(12.0) * F(64.0) * F(2.0 ** -8), 4, 0]  # e = 8 target: 252 more samples predicted
    counts = np.zeros(n, np.uint32)
    want = apr.plan(m, counts, **apr.parameters(ap, pl))
    assert want[0].size == n and want[2] == 64 * n == 67108928
    _compare(_run(twk, small_device, ap, pl, m, counts), want, "all at maxBatch")


def test_nothing_selected(twk, small_device):
    n = 3 * TILE + 5
    ap = twk.Adaptive(targetNoise=TARGET, maxSamples=CAP)
    m = np.zeros((n, 4), F)
    m[:] = [F(1.0) - F(0.01), 0, 16, 0]  # e = 0
    m[::3, 2] = 0                          # and padding
    counts = np.zeros(n, np.uint32)
    got = _run(twk, small_device, ap, None, m, counts)
    assert got[:2] == (0, 0) and got[3][0] == 0
    _compare(got, apr.plan(m, counts, **apr.parameters(ap, twk.AdaptivePlan())), "none")
    # the handle's own buffers: an empty plan is read back as such and its planned launch is a successful no-op
    dev = small_device
    for it in range(4):
        dev.render(it)
    before = [dev.getOutputBufferHost().copy(), dev.readMoments().copy()]
    assert dev.adaptivePlan(twk.Adaptive(targetNoise=1e30, minSamples=2)) == (0, 0)
    active, offsets = dev.readPlan()
    assert active.size == 0 and offsets.tolist() == [0]
    dev.renderPlanned()
    dev.renderPlanned()  # nothing advanced: the empty plan stays
    assert (dev.readSampleCounts() == 4).all()
    assert np.array_equal(before[0].view(np.uint32), dev.getOutputBufferHost().view(np.uint32)) and np.array_equal(before[1].view(np.uint32), dev.readMoments().view(np.uint32))
    dev.render(4)  # and the picture is still uniform
