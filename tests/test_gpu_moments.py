"""-m gpu: the luminance moments of the integrator's samples (twk_enable_moments): the MOMENTS builds of the accumulate kernels
fold Welford's recurrence over the luminance of every sample they keep, in the same read that folds the running mean
(csrc/shade_device.h foldSamples), into one f32 float4 (mean, M2, n, 0) per launch index.

The oracle's progressive lerp does not give a raw sample back, so the tests read the samples through the debug tap
twk_debug_read_path_radiance, first pin the tap to the oracle (the running mean of its samples, restated in numpy float32, is the
oracle's picture after every iteration, in every bit; and single samples against oracles that render one iteration only), and then
use it as the input of the restatement tests/test_moments_host.py welford(), which the moments must equal bit for bit."""
import numpy as np
import pytest

from conftest import load_app
from test_moments_host import F, fold_mean, kept_radiance, luminance, welford

pytestmark = pytest.mark.gpu

RES = (61, 37)  # no multiple of a tile, a block or a wave; 2 257 launch indices: 9 blocks of the accumulate kernel, the last one ragged
ITERATIONS = 7


def _bits(a):
    """The words of a; every NaN as ONE pattern: which NaN an invalid operation (inf - inf) yields is the processor's choice."""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _same(a, b, what):
    diff = _bits(a) != _bits(b)
    assert a.shape == b.shape and not diff.any(), f"{what}: {diff.sum()} of {diff.size} words differ, first at {np.argwhere(diff)[:4].tolist()}"


def _app(twk):
    return load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", RES)


def _device(twk, app, moments=True, half=False, aov=False, debug=False, lights=None, materials=None, index=0, count=1):
    dev = twk.Device(ordinal=0, index=index, count=count, miss=app.info.miss)
    app.initDevice(dev, distribution=1 if count > 1 else None)
    if lights is not None:
        dev.initLights(lights)
    if materials is not None:
        dev.initMaterials(materials)
    dev.setDebugExceptions(debug)
    if aov:
        dev.enableAov(True)
    if half:
        dev.setOutputFormat(1)
    if moments:
        dev.enableMoments(True)
    return dev


def _passes(dev, batch, iterations=ITERATIONS, first=0):
    """Renders iterations first .. first + iterations - 1 in passes of `batch`; returns the tap's samples of all of them [iterations, H, W, 4]."""
    dev.setLaunchBatch(batch)
    taps = []
    for start in range(first, first + iterations, batch):
        count = min(batch, first + iterations - start)
        for it in range(start, start + count):
            dev.render(it)
        taps.append(dev.debugReadPathRadiance(count))
    return np.concatenate(taps, axis=0)


@pytest.fixture(scope="module")
def seven(twk):
    """Iterations 0 .. 6 of C2 at 61x37 as ONE pass of 7 samples per launch index (two lanes by the default choice: 15 799 paths),
    moments and AOVs on: (samples of the tap, moments, picture, albedo AOV, normal AOV). Read-only, shared."""
    dev = _device(twk, _app(twk), aov=True)
    tap = _passes(dev, ITERATIONS)
    out = (tap, dev.readMoments(), dev.getOutputBufferHost(), dev.readAov(0), dev.readAov(1))
    dev.close()
    for a in out:
        a.setflags(write=False)
    return out


def test_the_tap_is_the_oracles_samples(twk, orc, seven):
    tap = seven[0]
    assert tap.shape == (ITERATIONS, RES[1], RES[0], 4) and (tap[..., 3] == 1).all() and np.isfinite(tap).all() and tap[..., :3].max() > 0.5
    app = _app(twk)
    ref = orc.Oracle(miss=app.info.miss)
    ref.loadApplication(app)
    assert not ref.getOutputBufferHost().any(), "the oracle's picture starts at zero"
    for it in range(ITERATIONS):
        ref.render(it, threads=8)
        _same(fold_mean(tap[:it + 1], 0, np.zeros(tap.shape[1:], F)), ref.getOutputBufferHost(), f"running mean of the tap's samples 0 .. {it} against the oracle")
    ref.close()
    _same(fold_mean(tap, 0, np.zeros(tap.shape[1:], F)), seven[2], "... and against the device's own picture")
    # single samples: an oracle that renders ONLY iteration k folds lerp(0, r, t) = 0 + t * (r - 0) = t r, t = 1 / (k + 1); exact
    # for a power of two t (checked on the CPU: F(0) + F(0.5) * (r - F(0)) == F(0.5) * r for every finite normal r whose half is normal)
    for k, t in ((1, F(0.5)), (3, F(0.25))):
        assert F(1.0) / F(k + 1) == t
        one = orc.Oracle(miss=app.info.miss)
        one.loadApplication(app)
        one.render(k, threads=8)
        alone = one.getOutputBufferHost()
        one.close()
        r = tap[k, ..., :3]
        normal = np.isfinite(r) & ((np.abs(r) >= np.finfo(F).tiny / t) | (r == 0))
        assert normal.mean() > 0.99
        assert np.array_equal(_bits(t * r)[normal], _bits(alone[..., :3])[normal]), f"sample {k} of the tap is not the oracle's sample of iteration {k}"


def test_moments_equal_the_restatement_bit_for_bit(twk, seven):
    tap, moments = seven[0], seven[1]
    expect = welford(tap, 0, np.zeros(tap.shape[1:], F))
    _same(moments, expect, "moments of one pass of 7 against Welford over the tap's samples")
    assert (moments[..., 2] == ITERATIONS).all() and (moments[..., 3] == 0).all()
    assert np.isfinite(moments).all()
    # what the triple means: the running mean of the luminances, and their squared deviations, in float64
    l = luminance(tap[..., :3]).astype(np.float64)
    # M2 is 0 exactly where the seven luminances coincide (the black background, a light seen directly: d = 0 at every step) and
    # positive wherever they differ by more than what the product d (l - mean) could lose to underflow
    spread = l.max(axis=0) - l.min(axis=0)
    assert (spread > 1e-15).any() and (spread == 0).any()
    assert (moments[..., 1][spread == 0] == 0).all() and (moments[..., 1][spread > 1e-15] > 0).all()
    assert np.allclose(moments[..., 0], l.mean(axis=0), rtol=1e-5, atol=1e-7)
    assert np.allclose(moments[..., 1], ((l - l.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-3, atol=1e-9)


@pytest.mark.parametrize("batch", [1, 3])
def test_moments_do_not_depend_on_the_launch_batch(twk, seven, batch):
    dev = _device(twk, _app(twk), aov=True)
    tap = _passes(dev, batch)
    _same(tap, seven[0], f"the samples of passes of {batch}")
    _same(dev.readMoments(), seven[1], f"moments after passes of {batch}")
    _same(dev.getOutputBufferHost(), seven[2], "picture")
    dev.close()


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_moments_do_not_depend_on_the_lanes_of_a_pass(twk, seven, lanes, monkeypatch):
    """TWK_PASS_LANES=2 at one pass of 7: 15 799 paths, lanes of 8 192 and 7 607 (>= 4 096 each, or chooseLanes drops one)."""
    monkeypatch.setenv("TWK_PASS_LANES", lanes)
    dev = _device(twk, _app(twk))
    _same(_passes(dev, ITERATIONS), seven[0], "samples")
    _same(dev.readMoments(), seven[1], f"moments, {lanes} lane(s)")
    dev.close()


def test_moments_in_half_mode_are_the_float_runs(twk, seven):
    """RGBA16F output: the picture is rounded to half after every sample, the moments never are."""
    dev = _device(twk, _app(twk), half=True, aov=True)
    tap = _passes(dev, 3)
    _same(tap, seven[0], "samples")
    got = dev.readMoments()
    assert got.dtype == F
    _same(got, seven[1], "moments of the RGBA16F run")
    ptr, nbytes = dev.momentsDevicePointer()
    assert ptr and nbytes == RES[0] * RES[1] * 16
    assert dev.getOutputBufferHalf().dtype == np.float16 and not np.array_equal(dev.getOutputBufferHost(), seven[2])
    dev.close()


def test_tiled_moments_are_the_single_devices_at_the_mapped_pixels(twk, seven):
    app = _app(twk)
    seen = np.zeros(RES[::-1], bool)
    for index in range(2):
        dev = _device(twk, app, index=index, count=2)
        _passes(dev, ITERATIONS)
        got, lw = dev.readMoments(), dev.launchWidth
        assert lw == twk.launch_width(RES[0], 8, 2) and got.shape == (RES[1], lw, 4)
        for y in range(RES[1]):
            for x in range(lw):
                px = twk.tile_column(x, y, (8, 8), 2, index)
                if px < RES[0]:
                    assert np.array_equal(_bits(got[y, x]), _bits(seven[1][y, px])), (index, x, y)
                    seen[y, px] = True
                else:
                    assert not got[y, x].any(), "a launch index outside the image has no samples: its triple stays zero"
        dev.close()
    assert seen.all()


def test_a_restart_at_iteration_zero_starts_the_triple_over(twk, seven):
    dev = _device(twk, _app(twk))
    _passes(dev, ITERATIONS)
    _same(dev.readMoments(), seven[1], "first run")
    tap = _passes(dev, 3, iterations=3)
    _same(tap, seven[0][:3], "the samples of the restart")
    got = dev.readMoments()
    assert (got[..., 2] == 3).all()
    _same(got, welford(seven[0][:3], 0, np.zeros(got.shape, F)), "moments after the restart")
    # and it goes on from there
    _passes(dev, 4, iterations=4, first=3)
    _same(dev.readMoments(), seven[1], "iterations 3 .. 6 after the restart")
    dev.close()


@pytest.mark.parametrize("emission", [(float("inf"),) * 3, (-10.0, -10.0, -10.0)], ids=["infinite", "negative"])
def test_dropped_and_replaced_samples(twk, emission):
    """The lights of tests/test_gpu_nee.py test_debug_exceptions_false_colours: infinite emission makes infinite samples and, where a
    zero factor meets it, NaN — the zero factor here is the red albedo of the white walls' material set to 0 (throughput.x = 0 on
    a path that goes on, times an infinite emission), without which this scene makes no NaN; negative emission makes negative
    samples. Switch off: a NaN sample does not count, every other
    does (an infinite one makes the triple not finite). Switch on: every sample counts, as its false colour."""
    app = _app(twk)
    lights = app.lights
    for light in lights:
        light.emission[0], light.emission[1], light.emission[2] = emission
    materials = app.materials
    assert materials[1].indexBSDF == 0 and materials[1].albedo[0] > 0.5
    materials[1].albedo[0] = 0.0
    count = 4
    zero = np.zeros((RES[1], RES[0], 4), F)
    dev = _device(twk, app, lights=lights, materials=materials)
    tap = _passes(dev, count, iterations=count)
    got = dev.readMoments()
    picture = dev.getOutputBufferHost()
    dev.close()
    nan = np.isnan(tap[..., :3]).any(axis=-1)
    if emission[0] > 0:
        assert nan.any() and not nan.all(axis=0).all(), "the scene makes NaN samples, and not only NaN samples"
    else:
        assert not nan.any() and (tap[..., :3] < 0).any()
    assert np.array_equal(got[..., 2], (count - nan.sum(axis=0)).astype(F)), "n is the iteration count less the NaN samples of the pixel"
    _same(got, welford(tap, 0, zero), "switch off")
    _same(picture, fold_mean(tap, 0, zero), "the running mean keeps the same samples")

    dev = _device(twk, app, lights=lights, materials=materials, debug=True)
    tap_on = _passes(dev, count, iterations=count)
    got = dev.readMoments()
    dev.close()
    _same(tap_on, tap, "the tap holds the raw samples: the switch replaces them in the fold")
    assert (got[..., 2] == count).all() and np.isfinite(got).all()
    _same(got, welford(tap, 0, zero, debug_exceptions=True), "switch on")
    # "l is the false colour's": a pixel whose samples are all the same false colour has that colour's luminance as its mean, exactly
    # (mean = 0 + l / 1, then d = 0 for every further sample), and no deviation
    replaced, _ = kept_radiance(tap, True)
    uniform = (replaced == replaced[0]).all(axis=-1).all(axis=0) & (replaced[0] == 1000000.0).any(axis=-1)
    assert uniform.any()
    assert np.array_equal(got[uniform][:, 0], luminance(replaced[0][uniform])) and (got[uniform][:, 1] == 0).all()


def test_with_moments_off_nothing_changes(twk, seven):
    """The picture and the AOVs of a handle that never heard of moments, of one that had them on and off again, and of one that has
    them on, are the same bits."""
    app = _app(twk)
    plain = _device(twk, app, moments=False, aov=True)
    with pytest.raises(twk.TwkError) as e:
        plain.readMoments()
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE and "twk_read_moments" in str(e.value)
    with pytest.raises(twk.TwkError) as e:
        plain.debugReadPathRadiance(1)
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE and "twk_debug_read_path_radiance" in str(e.value)
    _same(_passes(plain, ITERATIONS), seven[0], "samples")
    reference = (plain.getOutputBufferHost(), plain.readAov(0), plain.readAov(1))
    plain.close()
    toggled = _device(twk, app, aov=True)
    toggled.enableMoments(False)
    _passes(toggled, ITERATIONS)
    for name, a, b, c in zip(("picture", "albedo", "normal"), (toggled.getOutputBufferHost(), toggled.readAov(0), toggled.readAov(1)), reference, seven[2:]):
        _same(a, b, f"{name}, moments switched off again")
        _same(c, b, f"{name}, moments on")
    with pytest.raises(twk.TwkError):
        toggled.readMoments()
    toggled.enableMoments(True)
    assert not toggled.readMoments().any(), "enabled again: a zeroed buffer"
    toggled.close()
