"""-m gpu: twk_estimate_noise (csrc/noise_kernels.hip) against tests/noise_restate.py, every field of the summary and every bit of
the error map equal: on crafted moments through explicit device buffers, on the handle's own moments of a render, merged over two
handles that share the frame as tiles; and a render's picture, moments and AOVs are the same bytes with estimates in between."""
import ctypes as C

import numpy as np
import pytest

import noise_restate as nr
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
RES = (160, 90)
# the kernel's grid is at most numCUs (256 on this part) blocks of 1024 lanes: 262 144 elements per sweep of the grid-stride loop
GRID_SPAN = 256 * 1024
SIZES = [1, 63, 64, 65, 257 * 3, 160 * 90, 640 * 480]
assert SIZES[-1] > GRID_SPAN  # the last size runs the loop more than once in some blocks


def _specials(min_samples, dark_floor):
    nan, inf = float("nan"), float("inf")
    d = F(min_samples - 1) * F(min_samples)
    one = F(1.0) - F(dark_floor)  # mean + darkFloor is 1 up to a rounding
    at = lambda e: [one, F(e) * F(e) * d, min_samples, 0]  # a triple whose e is about `e`
    rows = [[1, 1, 0, 0], [nan, nan, 0, 5], [0, 0, -0.0, 0],                                # n == 0: empty, whatever the rest
            [1, 2, min_samples - 1, 0], [1, 2, min_samples, 0],                             # one short of minSamples, and just enough
            [nan, 1, 8, 0], [inf, 1, 8, 0], [-inf, 1, 8, 0], [1, nan, 8, 0], [1, inf, 8, 0], [1, -inf, 8, 0],
            [1, 1, nan, 0], [1, 1, inf, 0], [1, 1, -inf, 0],
            [1, -1, 8, 0], [-1, 1, 8, 0], [1, 1, -8, 0],                                    # M2 < 0, mean < 0, n < 0
            [0.5, 0, 8, 0], [0, 0, 8, 0], [one, -0.0, 8, 0],                                # M2 = 0 (and -0): e = 0, bin 0
            [3e38, 1.2e-5, 4, 0],                                                           # a denormal e
            at(2.0 ** -16 * 0.98), at(2.0 ** -16 * 1.02), at(2.0 ** -17), at(2.0 ** -16),   # around the histogram's lower end
            at(2.0 ** 16 * 0.98), at(2.0 ** 16 * 1.02), at(2.0 ** 17), at(2.0 ** 16),       # around its upper end, and the fixed point's cap
            [0, 3e38, 4, 0], at(1.0), at(0.1), at(1.124), at(1.126)]                        # the largest e there is; ordinary ones
    return np.array(rows, F)


def _crafted(n, seed, min_samples=4, dark_floor=0.01):
    """n triples: random valid ones, every special of _specials scattered over them (all of them from 63 elements on), and from
    771 elements on a run of equal triples that fills whole waves, from 14 400 on whole blocks, with one bin."""
    rng = np.random.default_rng(seed)
    count = rng.integers(min_samples, 65, n).astype(F)
    mean = rng.gamma(2.0, 0.5, n).astype(F)
    rel = (10.0 ** rng.uniform(-4, 1, n)).astype(F)
    m = np.zeros((n, 4), F)
    m[:, 0], m[:, 2] = mean, count
    m[:, 1] = (rel * mean) ** 2 * (count - F(1.0)) * count
    m[:, 3] = rng.random(n).astype(F)  # the fourth component is not the kernel's business
    free = np.ones(n, bool)  # where the specials may go: not into the runs
    if n >= 771:
        m[128:128 + 200] = [F(1.0) - F(dark_floor), 12, 4, 0]     # waves 2 and 3 of block 0 entirely, 4 in part
        free[128:128 + 200] = False
    if n >= 14400:
        m[1000:1000 + 2100] = [0.25, 0, 16, 0]                     # block 1 entirely, blocks 0 and 2 in part: e = 0
        m[5 * 1024:6 * 1024 + 7] = [F(1.0) - F(dark_floor), 12 * 4, 4, 0]
        free[1000:1000 + 2100] = False
        free[5 * 1024:6 * 1024 + 7] = False
    special = _specials(min_samples, dark_floor)
    if n == 1:
        m[0] = special[seed % len(special)]
    else:
        where = rng.permutation(np.nonzero(free)[0])[:len(special)] if n >= 2 * len(special) else np.arange(min(n, len(special)))
        m[where] = special[:len(where)]
    return m


@pytest.fixture(scope="module")
def small_device(twk):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    yield dev
    dev.close()


def _estimate_explicit(twk, dev, moments, noise=None, with_map=True):
    n = moments.shape[0]
    src = _DeviceBuffer(twk, moments.nbytes)
    src.upload(moments)
    dst = _DeviceBuffer(twk, n * 4) if with_map else None
    try:
        s = dev.estimateNoise(noise=noise, moments=src.ptr.value, numElements=n, errorMap=dst.ptr.value if dst else None)
        emap = dst.download((n,), F) if dst else None
        assert np.array_equal(src.download(moments.shape, np.uint32), moments.view(np.uint32)), "the input was written"
    finally:
        src.free()
        if dst:
            dst.free()
    return s, emap


def _assert_equal(got, emap, moments, min_samples=4, dark_floor=0.01):
    expect, expect_map = nr.summary(moments, min_samples, dark_floor)
    g = nr.as_dict(got)
    for key in ("valid", "unknown", "empty", "sumFixed", "maxErrorBits"):
        assert g[key] == expect[key], (key, g[key], expect[key])
    differ = np.nonzero(g["histogram"] != expect["histogram"])[0]
    assert differ.size == 0, f"bins {differ[:8].tolist()}: {g['histogram'][differ[:8]].tolist()} for {expect['histogram'][differ[:8]].tolist()}"
    assert got.valid + got.unknown + got.empty == moments.shape[0] and got.reserved == 0
    if emap is not None:
        bad = np.nonzero(emap.view(np.uint32) != expect_map.view(np.uint32))[0]
        assert bad.size == 0, f"{bad.size} map values differ, first at {bad[:4].tolist()}: {emap[bad[:4]].tolist()} for {expect_map[bad[:4]].tolist()}"
    return expect


@pytest.mark.parametrize("n", SIZES)
def test_explicit_moments_equal_the_restatement(twk, small_device, n):
    m = _crafted(n, seed=n)
    got, emap = _estimate_explicit(twk, small_device, m)
    expect = _assert_equal(got, emap, m)
    if n >= 63:  # every special is in: the data do what the case list says
        cls, e = nr.classify(m)
        v = e[cls == nr.VALID]
        assert expect["empty"] >= 3 and expect["unknown"] >= 13 and expect["histogram"][0] > 0 and expect["histogram"][255] > 0
        assert ((v > 0) & (v < F(2.0 ** -126))).any(), "no denormal e"
        assert ((v > 0) & (v < F(2.0 ** -16))).any() and ((v >= F(2.0 ** -16)) & (v < F(2.0 ** -15))).any(), "nothing on one side of 2^-16"
        assert ((v > F(32768.0)) & (v < F(65536.0))).any() and (v > F(65536.0)).any(), "nothing on one side of 2^16"
        assert expect["sumFixed"] < int(np.rint(v.astype(np.float64) * 2 ** 20).sum())  # the cap at 65536 took something off
        assert got.maxError == float(v.max()) and F(got.mean) == nr.mean(expect) and F(got.quantile(0.95)) == nr.quantile(expect, 0.95)


def test_explicit_moments_with_parameters_and_without_a_map(twk, small_device):
    """minSamples and darkFloor reach the kernel; a darkFloor of 1e-30 lets e overflow: not finite, so unknown."""
    L = twk._lib
    for min_samples, dark_floor in ((2, 0.5), (9, 1e-30)):
        m = _crafted(771, seed=5, min_samples=min_samples, dark_floor=dark_floor)
        m[700] = [0, 3e38, 4, 0] if min_samples <= 4 else [0, 3e38, 16, 0]
        got, emap = _estimate_explicit(twk, small_device, m, noise=L.Noise(min_samples, dark_floor))
        _assert_equal(got, emap, m, min_samples, dark_floor)
        assert not nr.same(nr.as_dict(got), nr.summary(m)[0])  # and the defaults would have said something else
        if dark_floor < 1e-20:
            assert emap[700] == -1.0
        again, none = _estimate_explicit(twk, small_device, m, noise=L.Noise(min_samples, dark_floor), with_map=False)
        assert none is None and nr.same(nr.as_dict(again), nr.as_dict(got))  # the summary is zeroed before every estimate


def test_no_valid_element(twk, small_device):
    m = _crafted(1000, seed=3)
    m[::2, 2] = 0            # empty
    m[1::2, 2] = 3           # below minSamples
    got, emap = _estimate_explicit(twk, small_device, m)
    _assert_equal(got, emap, m)
    assert (got.valid, got.unknown, got.empty) == (0, 500, 500) and not got.histogram.any() and got.sumFixed == 0 and got.maxErrorBits == 0
    for call in (lambda: got.quantile(0.95), lambda: got.mean):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE


def test_refusals_on_a_device(twk):
    L = twk._lib
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    out = L.NoiseSummary()
    assert L.lib.twk_read_noise(dev.handle, C.byref(out)) == L.TWK_ERROR_INVALID_STATE  # no estimate on this handle yet
    with pytest.raises(twk.TwkError) as e:
        dev.estimateNoise()  # no state
    assert e.value.code == L.TWK_ERROR_INVALID_STATE
    app.initDevice(dev)
    with pytest.raises(twk.TwkError) as e:
        dev.estimateNoise()  # a state, but no moments
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_enable_moments" in str(e.value)
    buf = _DeviceBuffer(twk, 64 * 16)
    for moments, n, emap in ((buf.ptr.value, 64, buf.ptr.value), (buf.ptr.value, 64, buf.ptr.value + 63 * 16), (buf.ptr.value + 112, 32, buf.ptr.value)):
        with pytest.raises(twk.TwkError) as e:
            dev.estimateNoise(moments=moments, numElements=n, errorMap=emap)
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "overlaps" in str(e.value)
    assert L.lib.twk_read_noise(dev.handle, C.byref(out)) == L.TWK_ERROR_INVALID_STATE  # a refused estimate is none
    dev.estimateNoise(moments=buf.ptr.value, numElements=32, errorMap=buf.ptr.value + 32 * 16)  # side by side is no overlap
    buf.free()
    dev.close()


def _render(twk, res, iterations, index=0, count=1, moments=True, aov=False):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    dev = twk.Device(ordinal=0, index=index, count=count, miss=app.info.miss)
    app.initDevice(dev, distribution=1 if count > 1 else None)
    dev.enableMoments(moments)
    if aov:
        dev.enableAov(True)
    for it in range(iterations):
        dev.render(it)
    return dev


def test_own_moments_of_a_render(twk):
    dev = _render(twk, RES, 16)
    first = dev.estimateNoise()  # renders the recorded launches first
    m = dev.readMoments()
    assert (m[..., 2] == 16).all()
    _assert_equal(first, None, m.reshape(-1, 4))
    assert first.valid == RES[0] * RES[1] and first.unknown == 0 and first.empty == 0
    for it in range(16, 32):
        dev.render(it)
    second = dev.estimateNoise()
    _assert_equal(second, None, dev.readMoments().reshape(-1, 4))
    print(f"\nC2 {RES[0]}x{RES[1]}: mean e {first.mean:.5f} at 16 spp, {second.mean:.5f} at 32; 0.95 quantile edge {first.quantile(0.95):.5f}, {second.quantile(0.95):.5f}")
    assert second.sumFixed < first.sumFixed
    dev.enableMoments(False)
    with pytest.raises(twk.TwkError) as e:
        dev.estimateNoise()
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE
    dev.close()


def test_two_tiled_handles_merge_to_the_single_device_summary(twk):
    """150 x 90 over two handles: launchWidth 80 each, so 10 columns of a packed tile buffer are padding, which no sample reaches."""
    res = (150, 90)
    single = _render(twk, res, 16)
    whole = single.estimateNoise()
    single.close()
    halves = [_render(twk, res, 16, index=i, count=2) for i in range(2)]
    assert [d.launchWidth for d in halves] == [80, 80]
    parts = [d.estimateNoise() for d in halves]
    for d, part in zip(halves, parts):
        _assert_equal(part, None, d.readMoments().reshape(-1, 4))
        d.close()
    padding = 2 * 80 * 90 - 150 * 90
    assert parts[0].empty + parts[1].empty == padding
    merged = twk.NoiseSummary().merge(parts[0]).merge(parts[1])
    g, w = nr.as_dict(merged), nr.as_dict(whole)
    assert g["empty"] == w["empty"] + padding
    g["empty"] = w["empty"]
    assert nr.same(g, w), (g, w)
    assert F(merged.mean) == F(whole.mean) and merged.quantile(0.95) == whole.quantile(0.95) and merged.maxError == whole.maxError


def test_estimates_in_between_change_no_byte_of_a_render(twk):
    plain = _render(twk, RES, 8, aov=True)
    expect = [plain.getOutputBufferHost(), plain.readMoments(), plain.readAov(0), plain.readAov(1)]
    plain.close()
    dev = _render(twk, RES, 3, aov=True)
    dev.estimateNoise()
    emap = _DeviceBuffer(twk, RES[0] * RES[1] * 4)
    for it in range(3, 8):
        dev.render(it)
        if it == 5:
            dev.estimateNoise(errorMap=emap.ptr.value)
    dev.estimateNoise(noise=twk.Noise(2, 1.0))
    got = [dev.getOutputBufferHost(), dev.readMoments(), dev.readAov(0), dev.readAov(1)]
    for a, b, what in zip(got, expect, ("picture", "moments", "albedo", "normal")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    emap.free()
    dev.close()
