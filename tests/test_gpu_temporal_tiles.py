"""-m gpu: the moving-camera loop on a frame tiled over several handles (twk_render_geometry_tile,
twk_assemble_devices_with_geometry, twk_temporal_accumulate_assembled) against the existing own-buffer loop on one handle. Every
comparison is byte equality.

The orbit: the Cornell box at 61x37 with 8x8 tiles, three frames of 2 spp, 0.004 of a turn apart, Temporal(maxHistory=32,
positionTolerance=0.1) — the shape, step and parameters of test_gpu_temporal.test_own_buffers_equal_the_explicit_form — with the
cascade and its temporal merge on, on 2 and on 3 handles sharing this GPU, in both output formats. After EVERY frame the primary's
merged colour, moments and layers equal the single handle's; after the last, the sampled-variance denoiser on the merged buffers
and the resolve of the merged layers do. The equality is not vacuous: on the single handle, in frames 2 and 3, more than half of
the pixels hold a merged n above the frame's own. Then the negative controls, the reset and the refusals."""
import numpy as np
import pytest

import lifecycle as lc
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, TILE = 61, 37, (8, 8)
SHAPE = (HEIGHT, WIDTH)
FRAMES, SPP, STEP = 3, 2, 0.004
OUTPUT, MOMENTS, CASCADE = 0, 3, 5
MERGED = (OUTPUT, MOMENTS, CASCADE)


def _tp(twk):
    return twk._lib.Temporal(maxHistory=32, positionTolerance=0.1)


def _camera(twk, app, frame):
    i = app.info
    return twk.camera_frustum(tuple(i.center), i.phi + frame * STEP, i.theta, i.fov, i.distance, i.resolution[0] / i.resolution[1])


def _render(devs, camera, frame, geometry=True, skip_camera=()):
    for k, d in enumerate(devs):
        if k not in skip_camera:
            d.updateCamera(0, camera)
        d.setSampleOffset(frame * SPP)
        for it in range(SPP):
            d.render(it)
        if geometry:
            d.renderGeometryTile()


def _device(twk, app, shape, index=0, count=1, half=False):
    """lifecycle.new_device in the output format asked for: Application.initDevice sets the description's format (RGBA32F), so
    RGBA16F is chosen after it, before anything is rendered."""
    dev = lc.new_device(twk, app, shape, index=index, count=count)
    if half:
        dev.setOutputFormat(lc.HALF4)
    assert dev.outputFormat == (lc.HALF4 if half else lc.FLOAT4)
    return dev


def _merged(dev):
    return {"colour": lc._words(dev.readTemporal()), "moments": lc._words(dev.readTemporalMoments()), "layers": lc._words(dev.readTemporalCascade())}


def _post(twk, dev, half):
    """The sampled-variance denoiser on the merged colour and moments, and the resolve of the merged layers."""
    L = twk._lib
    colour, _, moments, _ = dev.temporalDevicePointers()
    dev.denoise(beauty=colour, albedo=None, normal=None, params=L.Denoiser(inputKind=0), shape=SHAPE, moments=moments, minSamples=4)
    denoised = lc._words(dev.readDenoised(raw=True, shape=SHAPE))
    out = _DeviceBuffer(twk, WIDTH * HEIGHT * (8 if half else 16))
    dev.cascadeResolve(layers=dev.temporalCascadeDevicePointer()[0], shape=SHAPE, resolved=out.ptr.value)
    dev.synchronizeStream()
    resolved = lc._words(out.download((HEIGHT, WIDTH, 4), np.float16 if half else np.float32))
    out.free()
    return {"denoised": denoised, "resolved": resolved}


@pytest.fixture(scope="module")
def single(twk):
    """{half: ([the merged buffers after each frame], the post steps after the last)} of ONE handle running the existing own-buffer
    loop; computed once."""
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    app = lc.make_app(twk, load_app, shape)
    out = {}
    for half in (False, True):
        dev = _device(twk, app, shape, half=half)
        dev.enableTemporalCascade(True)
        frames = []
        for f in range(FRAMES):
            dev.updateCamera(0, _camera(twk, app, f))
            dev.setSampleOffset(f * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.temporalAccumulate(_tp(twk))
            frames.append(_merged(dev))
            took = dev.readTemporalMoments()[..., 2] > dev.readMoments()[..., 2]
            assert (dev.readMoments()[..., 2] == SPP).all()
            # the share test_own_buffers_equal_the_explicit_form asserts at this shape and step: most pixels take history
            assert (took.mean() > 0.5) if f > 0 else not took.any(), (f, took.mean())
        out[half] = (frames, _post(twk, dev, half))
        dev.close()
    app.close()
    return out


def _tiled(twk, n, half):
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    app = lc.make_app(twk, load_app, shape)
    devs = [_device(twk, app, shape, index=i, count=n, half=half) for i in range(n)]
    devs[0].enableTemporalCascade(True)
    return app, devs


def _close(app, devs):
    for d in devs:
        d.close()
    app.close()


def _assert_same(got, want, what):
    for key in want:
        diff = lc.first_difference(got[key], want[key])
        assert diff is None, f"{what}, {key}: {diff}"


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("n", [2, 3])
def test_the_orbit_on_tiles_equals_the_orbit_on_one_device(twk, single, n, half):
    frames, post = single[half]
    app, devs = _tiled(twk, n, half)
    primary = devs[0]
    for f in range(FRAMES):
        _render(devs, _camera(twk, app, f), f)
        primary.assembleWithGeometry(devs, MERGED)
        primary.temporalAccumulateAssembled(_tp(twk))
        _assert_same(_merged(primary), frames[f], f"{n} handles, frame {f}")
    colour, colour_bytes, moments, moments_bytes = primary.temporalDevicePointers()
    assert colour and moments and colour_bytes == WIDTH * HEIGHT * (8 if half else 16) and moments_bytes == WIDTH * HEIGHT * 16
    assert primary.temporalCascadeDevicePointer()[1] == primary._cascadeLayers * WIDTH * HEIGHT * 16
    _assert_same(_post(twk, primary, half), post, f"{n} handles, after the last frame")
    _close(app, devs)


def _refused(twk, code, call, *words):
    with pytest.raises(twk.TwkError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_negative_controls_and_the_reset(twk, single):
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    name = "twk_assemble_devices_with_geometry"
    frames, _ = single[False]
    app, devs = _tiled(twk, 2, False)
    primary = devs[0]
    # assembling before renderGeometryTile is refused
    _render(devs, _camera(twk, app, 0), 0, geometry=False)
    _refused(twk, STATE, lambda: primary.assembleWithGeometry(devs, MERGED), name, "twk_render_geometry_tile")
    _render(devs, _camera(twk, app, 0), 0)
    primary.assembleWithGeometry(devs, MERGED)
    primary.temporalAccumulateAssembled(_tp(twk))
    _assert_same(_merged(primary), frames[0], "frame 0")
    # a handle that skipped the camera update: its share is of the last view, the assembly is refused
    _render(devs, _camera(twk, app, 1), 1, skip_camera=(1,))
    _refused(twk, VALUE, lambda: primary.assembleWithGeometry(devs, MERGED), name, "camera 0", "index 1")
    # ... and the merge refuses what the primary assembled for the last view
    _refused(twk, STATE, lambda: primary.temporalAccumulateAssembled(_tp(twk)), "twk_temporal_accumulate_assembled", "geometry", "stale")
    _render(devs, _camera(twk, app, 1), 1)
    primary.assembleWithGeometry(devs, MERGED)
    primary.temporalAccumulateAssembled(_tp(twk))
    _assert_same(_merged(primary), frames[1], "frame 1, after the refused attempt")
    # twk_temporal_reset: the getters refuse, and the next call passes the assembled frame through
    primary.temporalReset()
    _refused(twk, STATE, primary.readTemporal, "twk_read_temporal")
    _refused(twk, STATE, primary.readTemporalCascade, "twk_read_temporal_cascade")
    primary.temporalAccumulateAssembled(_tp(twk))
    through = {"colour": lc._words(primary.readAssembled(OUTPUT)), "moments": lc._words(primary.readAssembled(MOMENTS)), "layers": lc._words(primary.readAssembled(CASCADE))}
    _assert_same(_merged(primary), through, "after twk_temporal_reset")
    assert through["colour"].any() and not np.array_equal(through["moments"], frames[1]["moments"])
    _close(app, devs)


def test_refusals_of_the_assembled_merge(twk):
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    name = "twk_temporal_accumulate_assembled"
    app, devs = _tiled(twk, 2, False)
    primary = devs[0]
    merge = lambda tp=None: primary.temporalAccumulateAssembled(tp)
    _refused(twk, VALUE, lambda: merge(L.Temporal(maxHistory=0)), name, "maxHistory")
    _refused(twk, VALUE, lambda: merge(L.Temporal(positionTolerance=-0.1)), name, "positionTolerance")
    # nothing assembled yet; then plane by plane, each refusal naming what is missing
    _refused(twk, STATE, merge, name, "TWK_PLANE_OUTPUT", "not been assembled")
    _render(devs, _camera(twk, app, 0), 0)
    primary.assemble(devs, (OUTPUT,))
    _refused(twk, STATE, merge, name, "TWK_PLANE_MOMENTS", "not been assembled")
    primary.assemble(devs, (MOMENTS,))
    _refused(twk, STATE, merge, name, "TWK_PLANE_CASCADE", "not been assembled")
    primary.enableTemporalCascade(False)
    _refused(twk, STATE, merge, name, "geometry", "not been assembled")
    primary.assembleWithGeometry(devs, ())
    merge()  # beauty, moments and geometry are there and the layers are not asked for
    primary.enableTemporalCascade(True)
    _refused(twk, STATE, merge, name, "TWK_PLANE_CASCADE")
    primary.assembleWithGeometry(devs, (CASCADE,))
    merge()
    # the primary's camera changed: what it assembled is of the old view
    primary.updateCamera(0, _camera(twk, app, 1))
    _refused(twk, STATE, merge, name, "geometry", "stale")
    # the switches
    primary.enableMoments(False)
    _refused(twk, STATE, merge, name, "twk_enable_moments")
    primary.enableMoments(True)
    primary.enableGeometry(False)
    _refused(twk, STATE, merge, name, "twk_enable_geometry")
    primary.enableGeometry(True)
    # a handle that is not tiled is pointed to the own-buffer form; the own-buffer form on a tiled handle stays refused
    _refused(twk, STATE, lambda: primary.temporalAccumulate(), "twk_temporal_accumulate:", "packed tile")
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    one = _device(twk, app, shape)
    _refused(twk, STATE, lambda: one.temporalAccumulateAssembled(), name, "not tiled", "twk_temporal_accumulate ")
    one.close()
    fresh = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    _refused(twk, STATE, lambda: fresh.temporalAccumulateAssembled(), name, "twk_set_state")
    fresh.close()
    _close(app, devs)
