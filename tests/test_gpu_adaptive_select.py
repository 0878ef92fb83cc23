"""-m gpu: twk_adaptive_select (csrc/adaptive_kernels.hip) against tests/adaptive_restate.py, word for word: the explicit form on
synthetic buffers of every size at which the compaction takes another path (a part of a wave, whole waves, a part of a tile, several
tiles, more tiles than the scan block has lanes) with every selection pattern, its inputs unwritten; and the own-buffer form on the
packed tile buffers of two handles that share a frame, whose padding is never selected."""
import numpy as np
import pytest

import adaptive_restate as ar
import noise_restate as nr
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
TILE = 1024  # elements per tile of the compaction; the scan block takes 1024 tiles at a time
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17, 1024 * 1025 + 3]
assert (SIZES[-1] + TILE - 1) // TILE > 1024  # more tiles than one scan block has lanes
TARGET, CAP = 0.05, 100


def _pattern(name, n, rng):
    if name == "none":
        return np.zeros(n, bool)
    if name == "all":
        return np.ones(n, bool)
    if name == "alternating":
        return np.arange(n) % 2 == 1
    if name == "first":
        return np.arange(n) == 0
    if name == "last":
        return np.arange(n) == n - 1
    return rng.random(n) < float(name)


PATTERNS = ["none", "all", "alternating", "first", "last", "0.001", "0.5", "0.999"]


def _elements(want, rng):
    """Moments and counts whose predicate is `want`, each side made in every way the definition knows."""
    n = want.size
    one = F(1.0) - F(0.01)
    m = np.zeros((n, 4), F)
    m[:, 3] = rng.random(n)
    counts = rng.integers(0, CAP, n).astype(np.uint32)
    how = rng.integers(0, 4, n)
    yes = [[one, 12 * 4, 4, 0], [one, 12, 3, 0], [np.nan, 1, 8, 0], [one, np.inf, 8, 0]]      # e = 2; too few samples; not finite
    no = [[one, 12, 0, 0], [one, 0, 16, 0], [one, 12 * 4, 4, 0], [one, F(12.0) * F(TARGET) * F(TARGET), 4, 0]]  # empty; e = 0; capped; e == target
    for k in range(4):
        m[want & (how == k), :3] = yes[k][:3]
        m[~want & (how == k), :3] = no[k][:3]
    capped = ~want & (how == 2)
    counts[capped] = rng.choice([CAP, CAP + 1, 0xFFFFFFFF], capped.sum())
    return m, counts


@pytest.fixture(scope="module")
def small_device(twk):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    yield dev
    dev.close()


@pytest.mark.parametrize("n", SIZES)
def test_explicit_buffers_equal_the_restatement(twk, small_device, n):
    rng = np.random.default_rng(n)
    ap = twk.Adaptive(targetNoise=TARGET, maxSamples=CAP)
    d_moments, d_counts, d_active = _DeviceBuffer(twk, n * 16), _DeviceBuffer(twk, n * 4), _DeviceBuffer(twk, n * 4)
    try:
        cases = []
        for name in PATTERNS:
            mask = _pattern(name, n, rng)
            cases.append((name, mask, *_elements(mask, rng)))
        cases.append(("mixed", None, ar.mixed_moments(rng, n, TARGET), rng.choice([0, 1, CAP - 1, CAP, CAP + 1], n).astype(np.uint32)))
        for name, mask, m, counts in cases:
            want = ar.selected(m, counts, **ar.parameters(ap))
            assert mask is None or np.array_equal(want, mask), name  # the made elements select the pattern
            expect = np.flatnonzero(want).astype(np.uint32)
            d_moments.upload(m)
            d_counts.upload(counts)
            d_active.upload(np.full(n, 0xFFFFFFFF, np.uint32))
            got_n = small_device.adaptiveSelect(ap, d_moments.ptr.value, d_counts.ptr.value, n, d_active.ptr.value)
            active = d_active.download((n,), np.uint32)
            assert got_n == expect.size, (name, got_n, expect.size)
            bad = np.nonzero(active[:got_n] != expect)[0]
            assert bad.size == 0, f"{name}: {bad.size} entries differ, first at {bad[:4].tolist()}: {active[bad[:4]].tolist()} for {expect[bad[:4]].tolist()}"
            assert (active[got_n:] == 0xFFFFFFFF).all(), f"{name}: written beyond the list"
            assert np.array_equal(d_moments.download(m.shape, np.uint32), m.view(np.uint32)), f"{name}: the moments were written"
            assert np.array_equal(d_counts.download(counts.shape, np.uint32), counts), f"{name}: the counts were written"
    finally:
        d_moments.free(); d_counts.free(); d_active.free()


def test_random_patterns_have_the_density_they_claim():
    """The test data's own check: the made elements select exactly the wanted mask, on both sides in every way."""
    rng = np.random.default_rng(5)
    for name in PATTERNS:
        want = _pattern(name, 5000, rng)
        m, counts = _elements(want, rng)
        assert np.array_equal(ar.selected(m, counts, target_noise=F(TARGET), max_samples=CAP), want), name
    m, counts = _elements(_pattern("0.5", 5000, rng), rng)
    cls, e = nr.classify(m)
    assert set(cls.tolist()) == {nr.VALID, nr.UNKNOWN, nr.EMPTY} and (e == F(TARGET)).any() and (counts >= CAP).any()


def test_own_buffers_of_two_tiled_handles(twk):
    """61 x 37 over two handles: launchWidth 32 each, so 3 columns of the packed tile buffers are padding, which is EMPTY and
    never selected; each handle's list equals the restatement of its own moments and counts."""
    res = (61, 37)
    total = 0
    for index in range(2):
        app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
        dev = twk.Device(ordinal=0, index=index, count=2, miss=app.info.miss)
        app.initDevice(dev, distribution=1)
        dev.enableMoments(True)
        dev.enableAdaptive(True)
        for it in range(6):
            dev.render(it)
        assert dev.launchWidth == 32
        m = dev.readMoments().reshape(-1, 4)
        counts = dev.readSampleCounts().reshape(-1)
        assert (counts == 6).all()
        cls, e = nr.classify(m)
        ap = twk.Adaptive(targetNoise=float(np.median(e[cls == nr.VALID])))
        n = dev.adaptiveSelect(ap)
        active = dev.readActive()
        assert n == active.size and np.array_equal(active, ar.active_list(m, counts, **ar.parameters(ap)))
        assert 0 < n < (cls == nr.VALID).sum()
        assert (cls == nr.EMPTY).sum() >= 1 and not (cls[active] == nr.EMPTY).any()
        total += int((cls != nr.EMPTY).sum())
        assert np.array_equal(dev.readMoments().reshape(-1, 4).view(np.uint32), m.view(np.uint32))
        dev.close()
    assert total == res[0] * res[1]  # what is not padding is the picture, once
