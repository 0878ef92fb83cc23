"""-m gpu: assembling a tiled frame (twk_assemble, twk_assemble_devices; csrc/assemble_device.h) on the device.
  * synthetic planes: all six planes in one launch equal the numpy restatement byte for byte, in both output formats, for 2, 3 and 5
    devices, on the 16-byte path, the element-wise path and a shape that mixes them, with 2 and 8 cascade layers; planes that are not
    requested keep their bytes,
  * rendered planes: the assembled planes of 2 and of 3 tiled handles equal the single-device handle's own planes byte for byte (the
    renderer seeds by absolute pixel), directly, staged, and through twk_assemble on a block the test gathered,
  * the pipeline on the assembled frame equals the single-device pipeline,
  * every refusal, and the life of the assembled buffers across a resize."""
import ctypes as C

import numpy as np
import pytest

import assemble_restate as R
import lifecycle as lc
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

PLANES = range(6)
OUTPUT, ALBEDO, NORMAL, MOMENTS, COUNTS, CASCADE = PLANES


def _primary(twk, width, height, tile, n, index=0):
    shape = lc.Shape(width, height, tile, 1)
    app = lc.make_app(twk, load_app, shape)
    return app, shape, lc.new_device(twk, app, shape, index=index, count=n)


def _plane_sources(width, height, tile, n, half, layers, salt):
    """Per plane the packed iota buffers of every device, in the element size the plane has on a handle."""
    pixel = 8 if half else 16
    sizes = {OUTPUT: (pixel, 1), ALBEDO: (pixel, 1), NORMAL: (pixel, 1), MOMENTS: (16, 1), COUNTS: (4, 1), CASCADE: (16, layers)}
    return {p: R.iota_sources(width, height, tile, n, eb, k, salt=salt + 17 * p) for p, (eb, k) in sizes.items()}


def _upload_sources(twk, per_plane, n):
    """(list of n {plane: device pointer}, the buffers to free)"""
    buffers, sources = [], [dict() for _ in range(n)]
    for p, arrays in per_plane.items():
        for d, a in enumerate(arrays):
            b = _DeviceBuffer(twk, a.nbytes)
            b.upload(a)
            buffers.append(b)
            sources[d][p] = b.ptr.value
    return sources, buffers


def _read_words(dev, plane):
    return lc._words(dev.readAssembled(plane))


def _expect_words(arrays, width, height, tile, plane):
    out = R.assemble(arrays, width, height, tile)
    return lc._words(out if plane == CASCADE else out[0])


SYNTHETIC = [(61, 37, (8, 8)), (96, 64, (8, 8)), (64, 16, (2, 4))]


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("width,height,tile", SYNTHETIC, ids=["61x37-mixed", "96x64-wide", "64x16-elementwise"])
def test_synthetic_planes_equal_the_restatement(twk, width, height, tile, n):
    L = twk._lib
    app, shape, dev = _primary(twk, width, height, tile, n)
    for half in (False, True):
        dev.setOutputFormat(L.TWK_OUTPUT_HALF4 if half else L.TWK_OUTPUT_FLOAT4)
        for layers in (2, 8):
            dev.enableCascade(True, L.Cascade(layers=layers, start=1.0, base=2.0))
            with pytest.raises(twk.TwkError):  # a new format or layer count dropped what was assembled before
                dev.assembledDevicePointer(MOMENTS)
            first = _plane_sources(width, height, tile, n, half, layers, salt=1)
            sources, buffers = _upload_sources(twk, first, n)
            dev.assembleFrom(sources, PLANES)
            for p in PLANES:
                got, want = _read_words(dev, p), _expect_words(first[p], width, height, tile, p)
                assert lc.first_difference(got, want) is None, (p, half, layers, lc.first_difference(got, want))
            # a second launch of two planes, other values: those two change, the other four keep their bytes
            second = _plane_sources(width, height, tile, n, half, layers, salt=900001)
            sources2, buffers2 = _upload_sources(twk, {p: second[p] for p in (MOMENTS, COUNTS)}, n)
            dev.assembleFrom(sources2, (MOMENTS, COUNTS))
            for p in PLANES:
                want = _expect_words((second if p in (MOMENTS, COUNTS) else first)[p], width, height, tile, p)
                assert lc.first_difference(_read_words(dev, p), want) is None, (p, half, layers)
            ptr, nbytes = dev.assembledDevicePointer(CASCADE)
            assert ptr and nbytes == layers * height * width * 16
            assert dev.assembledDevicePointer(OUTPUT)[1] == height * width * (8 if half else 16)
            assert dev.assembledDevicePointer(COUNTS)[1] == height * width * 4
            dev.synchronizeStream()
            for b in buffers + buffers2:
                b.free()
    dev.close()
    app.close()


def _render(twk, dev, target):
    """Four uniform iterations, then one adaptive pass of two samples on the pixels above `target`: the counts differ by pixel."""
    for it in range(4):
        dev.render(it)
    dev.adaptiveSelect(twk.Adaptive(targetNoise=target))
    dev.renderAdaptive(2)


def _own_planes(dev, half):
    return {OUTPUT: lc._output(dev), ALBEDO: lc._words(dev.readAov(0, raw=True)), NORMAL: lc._words(dev.readAov(1, raw=True)),
            MOMENTS: lc._words(dev.readMoments()), COUNTS: dev.readSampleCounts(), CASCADE: lc._words(dev.readCascade())}


@pytest.fixture(scope="module")
def single(twk):
    """The single-device Cornell box at 61x37 in both formats: {half: (planes, denoised, resolved, noise summary)}; computed once."""
    L = twk._lib
    shape = lc.Shape(61, 37, (8, 8), 1)
    app = lc.make_app(twk, load_app, shape)
    out = {}
    for half in (False, True):
        dev = lc.new_device(twk, app, shape, half=half)
        _render(twk, dev, TARGET)
        planes = _own_planes(dev, half)
        assert len(np.unique(planes[COUNTS])) > 1, "the adaptive pass must leave different counts"
        dev.denoise(L.Denoiser(iterations=2), minSamples=4)
        denoised = lc._words(dev.readDenoised(raw=True))
        layers, _ = dev.cascadeDevicePointer()
        resolved = _DeviceBuffer(twk, 61 * 37 * (8 if half else 16))
        dev.cascadeResolve(layers=layers, shape=(37, 61), resolved=resolved.ptr.value)
        dev.synchronizeStream()
        resolved_words = lc._words(resolved.download((37, 61, 4), np.float16 if half else np.float32))
        resolved.free()
        noise = lc._summary(dev.estimateNoise())
        out[half] = (planes, denoised, resolved_words, noise)
        dev.close()
    app.close()
    return out


TARGET = 0.05


def _tiled_handles(twk, n, half):
    shape = lc.Shape(61, 37, (8, 8), 1)
    app = lc.make_app(twk, load_app, shape)
    devs = [lc.new_device(twk, app, shape, index=i, count=n, half=half) for i in range(n)]
    for d in devs:
        _render(twk, d, TARGET)
    return app, devs


def _assert_planes(dev, want, what):
    for p in PLANES:
        diff = lc.first_difference(_read_words(dev, p), want[p])
        assert diff is None, f"{what}, plane {p}: {diff}"


@pytest.mark.parametrize("stage", [False, True], ids=["direct", "staged"])
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("n", [2, 3])
def test_rendered_planes_equal_the_single_device(twk, single, n, half, stage, monkeypatch):
    if stage:
        monkeypatch.setenv("TWK_ASSEMBLE_STAGE", "1")  # read when a handle is created
    app, devs = _tiled_handles(twk, n, half)
    devs[0].assemble(devs[::-1], PLANES)  # any order: the handles' indices place them
    _assert_planes(devs[0], single[half][0], f"{n} handles")
    for d in devs:
        d.close()
    app.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_gathered_block_and_the_pipeline_on_the_assembled_frame(twk, single, half):
    """twk_assemble on a block the test gathered (every handle's planes read to the host and uploaded side by side), then the
    post steps on the assembled pointers against the single-device handle's own."""
    L = twk._lib
    planes, denoised, resolved, noise = single[half]
    app, devs = _tiled_handles(twk, 3, half)
    lw = devs[0].launchWidth
    gathered = {p: [] for p in PLANES}
    merged = L.NoiseSummary()
    for d in devs:
        own = _own_planes(d, half)
        for p in PLANES:
            gathered[p].append(own[p])
        merged.merge(d.estimateNoise())
    block = {p: np.ascontiguousarray(np.stack(gathered[p])) for p in PLANES}
    buffers = {p: _DeviceBuffer(twk, block[p].nbytes) for p in PLANES}
    for p in PLANES:
        buffers[p].upload(block[p])
    stride = {p: block[p].nbytes // 3 for p in PLANES}
    primary = devs[0]
    primary.assembleFrom([{p: buffers[p].ptr.value + d * stride[p] for p in PLANES} for d in range(3)], PLANES)
    _assert_planes(primary, planes, "gathered block")

    ptr = {p: primary.assembledDevicePointer(p)[0] for p in PLANES}
    primary.denoise(L.Denoiser(iterations=2), ptr[OUTPUT], ptr[ALBEDO], ptr[NORMAL], shape=(37, 61), moments=ptr[MOMENTS], minSamples=4)
    assert lc.first_difference(lc._words(primary.readDenoised(raw=True, shape=(37, 61))), denoised) is None
    out = _DeviceBuffer(twk, 61 * 37 * (8 if half else 16))
    primary.cascadeResolve(layers=ptr[CASCADE], shape=(37, 61), resolved=out.ptr.value)
    primary.synchronizeStream()
    got = lc._words(out.download((37, 61, 4), np.float16 if half else np.float32))
    assert lc.first_difference(got, resolved) is None
    whole = lc._summary(primary.estimateNoise(moments=ptr[MOMENTS], numElements=61 * 37))
    # the host merge of the per-handle summaries, which also counts every padding element of the packed buffers as empty
    expect = lc._summary(merged)
    assert expect[2] >= 3 * lw * 37 - 61 * 37
    expect[2] -= 3 * lw * 37 - 61 * 37
    assert np.array_equal(whole, expect), "the assembled moments give the host merge of the per-handle summaries"
    assert np.array_equal(whole, noise)
    out.free()
    for b in buffers.values():
        b.free()
    for d in devs:
        d.close()
    app.close()


def _refused(twk, code, call, *words):
    with pytest.raises(twk.TwkError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(twk):
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    shape = lc.Shape(61, 37, (8, 8), 1)
    app = lc.make_app(twk, load_app, shape)
    a, b = (lc.new_device(twk, app, shape, index=i, count=2) for i in range(2))
    pair = [a, b]
    name = "twk_assemble_devices"
    _refused(twk, STATE, lambda: a.readAssembled(OUTPUT), "twk_read_assembled", "not been assembled")
    _refused(twk, STATE, lambda: a.assembledDevicePointer(MOMENTS), "twk_get_assembled_device_pointer")
    _refused(twk, VALUE, lambda: a.assembledDevicePointer(6), "twk_get_assembled_device_pointer")
    _refused(twk, VALUE, lambda: a.assemble(pair, ()), name, "mask")
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble_devices(a.handle, C.c_uint(1 << 6), (C.c_void_p * 2)(a.handle.value, b.handle.value), 2)), name, "mask")
    _refused(twk, VALUE, lambda: a.assemble([a], (OUTPUT,)), name, "count")
    _refused(twk, VALUE, lambda: a.assemble([a, a], (OUTPUT,)), name, "exactly once")
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble_devices(a.handle, C.c_uint(1), (C.c_void_p * 2)(a.handle.value, None), 2)), name, "NULL")
    # the explicit form
    _refused(twk, VALUE, lambda: a.assembleFrom([{OUTPUT: 4096}, {}], (OUTPUT,)), "twk_assemble", "NULL source")
    _refused(twk, VALUE, lambda: a.assembleFrom([{OUTPUT: 4096}], (OUTPUT,)), "twk_assemble", "deviceCount")
    _refused(twk, VALUE, lambda: a.assembleFrom([{OUTPUT: 4096}, {OUTPUT: 4096}], ()), "twk_assemble", "mask")
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble(a.handle, C.c_uint(1), None, 2)), "twk_assemble", "NULL sources")
    # handles that disagree
    for other_shape, what in ((lc.Shape(64, 37, (8, 8), 1), "resolution"), (lc.Shape(61, 37, (8, 16), 1), "tile"), (lc.Shape(61, 37, (8, 8), 0), "distribution")):
        b.setState(lc.state_of(app, other_shape))
        _refused(twk, VALUE, lambda: a.assemble(pair, (OUTPUT,)), name, "disagree")
    b.setState(lc.state_of(app, shape))
    c = lc.new_device(twk, app, shape, index=1, count=3)
    _refused(twk, VALUE, lambda: a.assemble([a, c], (OUTPUT,)), name, "disagree")
    c.close()
    b.setOutputFormat(L.TWK_OUTPUT_HALF4)
    _refused(twk, VALUE, lambda: a.assemble(pair, (OUTPUT,)), name, "output format")
    b.setOutputFormat(L.TWK_OUTPUT_FLOAT4)
    b.enableCascade(True, L.Cascade(layers=4))
    _refused(twk, VALUE, lambda: a.assemble(pair, (CASCADE,)), name, "cascade parameters")
    a.assemble(pair, (OUTPUT,))  # the cascade is not asked for: its parameters do not matter
    b.enableCascade(True)
    # a requested plane whose switch is off on some handle
    switches = ((b.enableAov, (ALBEDO, NORMAL), "twk_enable_aov"), (b.enableCascade, (CASCADE,), "twk_enable_cascade"), (b.enableAdaptive, (COUNTS,), "twk_enable_adaptive"),
                (b.enableMoments, (MOMENTS,), "twk_enable_moments"))
    for switch, planes, text in switches:
        switch(False)
        for p in planes:
            _refused(twk, STATE, lambda: a.assemble(pair, (p,)), name, text)
        a.assemble(pair, (OUTPUT,))
    b.enableMoments(True); b.enableAdaptive(True); b.enableCascade(True); b.enableAov(True)
    a.enableAov(False)
    _refused(twk, STATE, lambda: a.assembleFrom([{ALBEDO: 4096}, {ALBEDO: 4096}], (ALBEDO,)), "twk_assemble", "twk_enable_aov")
    a.enableAov(True)
    # a shared frame holds the beauty already; the other planes are still packed
    frame = _DeviceBuffer(twk, 61 * 37 * 16)
    b.setSharedFrame(frame.ptr.value, frame.nbytes)
    _refused(twk, STATE, lambda: a.assemble(pair, (OUTPUT, MOMENTS)), name, "shared frame")
    a.assemble(pair, (MOMENTS,))
    b.setSharedFrame(0, 0)
    # before twk_set_state
    fresh = twk.Device(ordinal=0, index=1, count=2, miss=app.info.miss)
    _refused(twk, STATE, lambda: fresh.assembleFrom([{OUTPUT: 4096}, {OUTPUT: 4096}], (OUTPUT,)), "twk_assemble", "twk_set_state")
    _refused(twk, STATE, lambda: a.assemble([a, fresh], (OUTPUT,)), name, "twk_set_state")
    fresh.close()
    # distribution 0 with several devices: nothing is tiled
    for d in pair:
        d.setState(lc.state_of(app, lc.Shape(61, 37, (8, 8), 0)))
    _refused(twk, STATE, lambda: a.assemble(pair, (OUTPUT,)), name, "distribution 0")
    a.synchronizeStream()
    frame.free()
    for d in pair:
        d.close()
    app.close()


def test_one_device_is_the_identity(twk):
    shape = lc.Shape(61, 37, (8, 8), 1)
    app = lc.make_app(twk, load_app, shape)
    dev = lc.new_device(twk, app, shape)
    _render(twk, dev, TARGET)
    dev.assemble([dev], PLANES)
    _assert_planes(dev, _own_planes(dev, False), "one device")
    dev.close()
    app.close()


def test_a_resize_drops_the_assembled_buffers_and_the_next_assembly_is_a_fresh_pairs(twk):
    """After twk_set_state with another resolution the getter refuses until the next assemble; that assemble then gives what a fresh
    pair of handles gives at the new size."""
    before, after = lc.Shape(96, 64, (8, 8), 1), lc.Shape(61, 37, (8, 8), 1)
    app_before, app_after = lc.make_app(twk, load_app, before), lc.make_app(twk, load_app, after)
    devs = [lc.new_device(twk, app_before, before, index=i, count=2) for i in range(2)]
    for d in devs:
        _render(twk, d, TARGET)
    devs[0].assemble(devs, PLANES)
    assert devs[0].readAssembled(OUTPUT).shape == (64, 96, 4)
    for d in devs:
        lc.move(d, app_after, after)
    for p in PLANES:
        _refused(twk, twk._lib.TWK_ERROR_INVALID_STATE, lambda: devs[0].assembledDevicePointer(p), "not been assembled")
        _refused(twk, twk._lib.TWK_ERROR_INVALID_STATE, lambda: devs[0].readAssembled(p), "not been assembled")
    for d in devs:
        _render(twk, d, TARGET)
    devs[0].assemble(devs, PLANES)
    reused = {p: _read_words(devs[0], p) for p in PLANES}
    for d in devs:
        d.close()
    fresh = [lc.new_device(twk, app_after, after, index=i, count=2) for i in range(2)]
    for d in fresh:
        _render(twk, d, TARGET)
    fresh[0].assemble(fresh, PLANES)
    _assert_planes(fresh[0], reused, "a fresh pair against the resized pair")
    for d in fresh:
        d.close()
    app_before.close()
    app_after.close()
