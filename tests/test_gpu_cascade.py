"""-m gpu: the fold of the firefly cascade (twk_enable_cascade): the CascadeOn builds of the accumulate kernel split every kept
sample over the launch index's brightness layers in the read that folds the running mean (csrc/cascade_device.h). The samples come
from the tap twk_debug_read_path_radiance, which tests/test_gpu_moments.py pins to the oracle; the layers must equal the numpy
restatement tests/cascade_restate.py over them, bit for bit. C2 at 61 x 37, 7 iterations, as there."""
import numpy as np
import pytest

import cascade_restate as restate
from test_gpu_adaptive import NAMES, _read
from test_gpu_half_output import _DeviceBuffer
from test_gpu_moments import ITERATIONS, RES, _app, _bits, _device, _passes, _same
from test_moments_host import F, fold_mean, luminance, welford

pytestmark = pytest.mark.gpu

WIDE = (4, 0.01, 2.0)  # thresholds 0.01 .. 0.08: C2's samples reach past the top layer, so the clamp and every layer are in use


def _cascade_device(twk, params=None, **kw):
    dev = _device(twk, _app(twk), **kw)
    dev.enableCascade(True, None if params is None else twk.Cascade(*params))
    return dev


def _expect(tap, params=(6, 1.0, 8.0), debug=False, branches=None):
    b = restate.thresholds(*params)
    return restate.fold(tap, 0, np.zeros((len(b),) + tap.shape[1:], F), b, debug, branches)


@pytest.fixture(scope="module")
def seven(twk):
    """One pass of 7 with the cascade at its defaults, moments and AOVs on: (tap, layers, picture, albedo, normal, moments)."""
    dev = _cascade_device(twk, aov=True)
    tap = _passes(dev, ITERATIONS)
    out = (tap, dev.readCascade(), dev.getOutputBufferHost(), dev.readAov(0), dev.readAov(1), dev.readMoments())
    ptr, nbytes = dev.cascadeDevicePointer()
    assert ptr and nbytes == 6 * RES[0] * RES[1] * 16
    dev.close()
    for a in out:
        a.setflags(write=False)
    return out


def test_layers_equal_the_restatement_bit_for_bit(twk, seven):
    tap, layers = seven[0], seven[1]
    assert layers.shape == (6, RES[1], RES[0], 4) and layers.dtype == F
    branches = {}
    _same(layers, _expect(tap, branches=branches), "layers of one pass of 7 against the restatement over the tap's samples")
    assert (layers[0, ..., 3] == ITERATIONS).all() and not layers[1:, ..., 3].any()
    assert branches["below_start"] > 0 and branches["interior"] > 0, branches
    # what they mean: below the top threshold nothing is clamped, and the layers sum to the samples' sum
    b = restate.thresholds()
    assert luminance(tap[..., :3]).max() < b[-1]
    total, exact = layers[..., :3].astype(np.float64).sum(axis=0), tap[..., :3].astype(np.float64).sum(axis=0)
    assert (np.abs(total - exact) <= (ITERATIONS + 3) * 2.0 ** -23 * np.abs(tap[..., :3]).astype(np.float64).sum(axis=0)).all()


def test_with_the_cascade_on_picture_aovs_and_moments_are_the_bits_they_are_with_it_off(twk, seven):
    plain = _device(twk, _app(twk), aov=True)
    with pytest.raises(twk.TwkError) as e:
        plain.readCascade()
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE and "twk_read_cascade" in str(e.value)
    _same(_passes(plain, ITERATIONS), seven[0], "samples")
    for name, a, b in zip(("picture", "albedo", "normal", "moments"), (plain.getOutputBufferHost(), plain.readAov(0), plain.readAov(1), plain.readMoments()), seven[2:]):
        _same(a, b, name)
    plain.close()
    _same(seven[2], fold_mean(seven[0], 0, np.zeros(seven[2].shape, F)), "the running mean over the tap")
    _same(seven[5], welford(seven[0], 0, np.zeros(seven[5].shape, F)), "the moments over the tap")


@pytest.mark.parametrize("half,aov,moments", [(False, False, False), (True, True, True), (True, False, False), (False, False, True)],
                         ids=["f32", "f16-aov-moments", "f16", "f32-moments"])
def test_every_uniform_build_folds_the_same_layers(twk, seven, half, aov, moments):
    """accumulateKernel on float4 and Half4 pixels, with and without MOMENTS: the layers are f32 in half mode too, and need neither AOVs
    nor moments."""
    dev = _cascade_device(twk, half=half, aov=aov, moments=moments)
    _same(_passes(dev, ITERATIONS), seven[0], "samples")
    got = dev.readCascade()
    assert got.dtype == F
    _same(got, seven[1], "layers")
    if half:
        assert dev.getOutputBufferHalf().dtype == np.float16
    elif not moments:
        _same(dev.getOutputBufferHost(), seven[2], "picture without moments")
    dev.close()


@pytest.mark.parametrize("batch", [1, 3])
def test_layers_do_not_depend_on_the_launch_batch(twk, seven, batch):
    dev = _cascade_device(twk)
    _same(_passes(dev, batch), seven[0], f"the samples of passes of {batch}")
    _same(dev.readCascade(), seven[1], f"layers after passes of {batch}")
    dev.close()


def test_layers_do_not_depend_on_the_lanes_of_a_pass(twk, seven, monkeypatch):
    monkeypatch.setenv("TWK_PASS_LANES", "2")
    dev = _cascade_device(twk)
    _same(_passes(dev, ITERATIONS), seven[0], "samples")
    _same(dev.readCascade(), seven[1], "layers, 2 lanes")
    dev.close()


def test_iteration_zero_starts_afresh_and_new_parameters_zero_the_layers(twk, seven):
    dev = _cascade_device(twk)
    _passes(dev, ITERATIONS)
    _same(dev.readCascade(), seven[1], "first run")
    tap = _passes(dev, 3, iterations=3)
    _same(dev.readCascade(), _expect(tap), "layers after the restart")
    _passes(dev, 4, iterations=4, first=3)
    _same(dev.readCascade(), seven[1], "iterations 3 .. 6 after the restart")
    dev.enableCascade(True)  # the same parameters again: nothing changes
    _same(dev.readCascade(), seven[1], "enabled again with the same parameters")
    dev.enableCascade(True, twk.Cascade(*WIDE))
    got = dev.readCascade()
    assert got.shape == (4, RES[1], RES[0], 4) and not got.any(), "new parameters: zeroed layers"
    dev.enableCascade(False)
    with pytest.raises(twk.TwkError):
        dev.readCascade()
    _same(_passes(dev, ITERATIONS), seven[0], "samples with the cascade off again")
    _same(dev.getOutputBufferHost(), seven[2], "picture with the cascade off again")
    dev.close()


def test_narrow_thresholds_populate_every_layer_and_the_clamp(twk, seven):
    dev = _cascade_device(twk, WIDE, half=True)
    tap = _passes(dev, 3)
    _same(tap, seven[0], "samples")
    got = dev.readCascade()
    dev.close()
    branches = {}
    _same(got, _expect(tap, WIDE, branches=branches), "start 0.01, base 2, layers 4")
    assert branches["clamp"] > 0 and branches["interior"] > 0 and branches["below_start"] > 0, branches
    assert all((got[j, ..., :3] != 0).any() for j in range(4)), "every layer is populated"
    b = restate.thresholds(*WIDE)
    above = luminance(tap[..., :3]).max(axis=0) >= b[-1]
    assert above.any()
    total, exact = got[..., :3].astype(np.float64).sum(axis=(0, -1)), tap[..., :3].astype(np.float64).sum(axis=(0, -1))
    assert (total[above] < exact[above]).all(), "the clamp removes energy above the top layer"


@pytest.mark.parametrize("emission", [(float("inf"),) * 3, (-10.0, -10.0, -10.0)], ids=["infinite", "negative"])
def test_samples_that_are_not_finite_are_counted_and_add_nothing(twk, emission):
    """The lights and the material of tests/test_gpu_moments.py test_dropped_and_replaced_samples: infinite emission makes infinite
    samples (rejected: counted in n and in the last layer's .w, added nowhere) and NaN samples (dropped by the keep rule: not in n);
    negative emission makes negative samples (kept, weight 1 in layer 0). Under debugExceptions every sample counts as its false colour."""
    app = _app(twk)
    lights = app.lights
    for light in lights:
        light.emission[0], light.emission[1], light.emission[2] = emission
    materials = app.materials
    materials[1].albedo[0] = 0.0
    count = 4
    for debug in (False, True):
        dev = _device(twk, app, lights=lights, materials=materials, debug=debug)
        dev.enableCascade(True)
        tap = _passes(dev, count, iterations=count)
        got, moments = dev.readCascade(), dev.readMoments()
        dev.close()
        branches = {}
        _same(got, _expect(tap, debug=debug, branches=branches), f"debugExceptions {debug}")
        assert np.array_equal(got[0, ..., 3], moments[..., 2]), "n is the moments' n: the same keep rule"
        assert np.isfinite(got).all(), "what is not finite is never added"
        nan = np.isnan(tap[..., :3]).any(axis=-1)
        inf = ~nan & np.isinf(tap[..., :3]).any(axis=-1)
        if debug:
            assert (got[0, ..., 3] == count).all() and not got[5, ..., 3].any() and branches["rejected"] == 0
        elif emission[0] > 0:
            assert nan.any() and inf.any()
            assert np.array_equal(got[5, ..., 3], inf.sum(axis=0).astype(F)) and np.array_equal(got[0, ..., 3], (count - nan.sum(axis=0)).astype(F))
        else:
            assert (tap[..., :3] < 0).any() and not got[5, ..., 3].any() and (got[0, ..., :3] < 0).any()


_uniform_cache = {}


def _uniform_layers(twk, counts, half=False):
    """{c: (layers, [colour, albedo, normal, moments] as test_gpu_adaptive._read reads them) after twk_launch(0 .. c-1)} for every c
    asked for: a fresh handle in the output format per request that the cache cannot serve, read as it passes each c."""
    have = _uniform_cache.setdefault(half, {})
    need = sorted(set(int(c) for c in counts) - set(have))
    if need:
        dev = _cascade_device(twk, aov=True, half=half)
        done = 0
        for c in need:
            for it in range(done, c):
                dev.render(it)
            done = c
            have[c] = (dev.readCascade(), _read(dev, half))
        dev.close()
    return have


@pytest.mark.parametrize("planned,half", [(False, False), (True, False), (False, True), (True, True)], ids=["select", "plan", "select-RGBA16F", "plan-RGBA16F"])
def test_after_adaptive_passes_a_pixel_with_count_c_holds_the_layers_of_c_uniform_launches(twk, planned, half):
    """accumulateKernel's listed form (twk_adaptive_select + twk_launch_adaptive) and its planned form (twk_adaptive_plan +
    twk_launch_adaptive_planned) with the cascade on, in either output format, two rounds after four uniform iterations; the target
    of a round is the median of its valid errors. RGBA16F: the raw colour, both raw AOVs and the moments are compared too, per
    count, with uniform launches on a fresh handle in the same format (as tests/test_gpu_adaptive.py does with the cascade off)."""
    import noise_restate as nr
    dev = _cascade_device(twk, aov=True, half=half)
    dev.enableAdaptive(True)
    for it in range(4):
        dev.render(it)
    for r in range(2):
        cls, e = nr.classify(dev.readMoments().reshape(-1, 4))
        ap = twk.Adaptive(targetNoise=float(np.median(e[cls == nr.VALID])), maxSamples=4096)
        if planned:
            n, paths = dev.adaptivePlan(ap, twk.AdaptivePlan(1, 5))
            assert 0 < n < RES[0] * RES[1] and paths > n
            dev.renderPlanned()
        else:
            assert 0 < dev.adaptiveSelect(ap) < RES[0] * RES[1]
            dev.renderAdaptive(3)
    counts, got, buffers = dev.readSampleCounts(), dev.readCascade(), _read(dev, half)
    picture = dev.getOutputBufferHost()
    dev.close()
    distinct = np.unique(counts)
    assert distinct.size >= 3 and distinct.min() == 4
    ref = _uniform_layers(twk, distinct, half)
    for c in distinct:
        where = counts == c
        layers, uniform = ref[int(c)]
        assert np.array_equal(_bits(got[:, where]), _bits(layers[:, where])), f"layers differ from twk_launch(0..{int(c) - 1}) at pixels with count {int(c)}"
        assert (got[0][where][:, 3] == c).all()
        if half:
            for name, g, w in zip(NAMES, buffers, uniform):
                bad = np.nonzero((g[where] != w[where]).any(axis=-1))[0]
                assert bad.size == 0, f"{name} differs from twk_launch(0..{int(c) - 1}) at {bad.size} of {int(where.sum())} pixels with count {int(c)}"
    assert np.isfinite(picture).all()


def test_two_tiled_handles_assemble_to_the_single_devices_layers_and_resolve(twk, seven):
    """Index 0 and 1 of 2 on one GPU, distribution 1: packed tile buffers. Every layer assembled with twk_compositor is the single
    device's layer; the explicit resolve of the assembled layers is the single device's own-buffer resolve; the own-buffer resolve on
    a tile handle is refused."""
    handles = [_cascade_device(twk, index=i, count=2) for i in range(2)]
    for d in handles:
        _passes(d, ITERATIONS)
    tiles = np.stack([d.readCascade() for d in handles])  # [device, K, H, launchWidth, 4]
    lw = handles[0].launchWidth
    assert tiles.shape == (2, 6, RES[1], lw, 4) and lw == twk.launch_width(RES[0], 8, 2)
    with pytest.raises(twk.TwkError) as e:
        handles[1].cascadeResolve()
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE and "twk_cascade_resolve" in str(e.value) and "tile" in str(e.value)
    handles[1].close()
    dev = handles[0]
    pixels = RES[0] * RES[1]
    block, frame = _DeviceBuffer(twk, 2 * RES[1] * lw * 16), _DeviceBuffer(twk, 6 * pixels * 16)
    for j in range(6):
        block.upload(tiles[:, j])
        dev.compositor(block.ptr.value, frame.ptr.value + j * pixels * 16)
        dev.synchronizeStream()
    assembled = frame.download((6, RES[1], RES[0], 4), F)
    _same(assembled, seven[1], "the layers assembled with twk_compositor against the single device's")
    resolved = _DeviceBuffer(twk, pixels * 16)
    dev.cascadeResolve(layers=frame.ptr.value, shape=(RES[1], RES[0]), resolved=resolved.ptr.value)
    dev.synchronizeStream()
    explicit = resolved.download((RES[1], RES[0], 4), F)
    dev.close()
    for buffer in (block, frame, resolved):
        buffer.free()
    single = _cascade_device(twk)
    _passes(single, ITERATIONS)
    single.cascadeResolve()
    own = single.readResolved()
    single.close()
    _same(explicit, own, "the explicit resolve of the assembled layers against the single device's own-buffer resolve")
    _same(own, restate.resolve(seven[1], restate.thresholds(), twk._lib.TWK_CASCADE_KAPPA), "... and against the restatement")
