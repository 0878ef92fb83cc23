"""-m gpu: the geometry-guided denoiser on a frame tiled over several handles. The filter on the assembled planes and the assembled
geometry of 2 and of 3 tiled handles (sharing this GPU) equals the single handle's own-buffer result byte for byte, in both output
formats: after one frame (the sampled-variance mode on the frame's own moments), and after a three-frame temporal orbit (the same
mode on the merged colour and merged moments, guided by the last frame's AOVs and geometry). The Cornell box at 61x37, 8x8 tiles,
2 spp a frame, the orbit of tests/test_gpu_temporal_tiles.py."""
import numpy as np
import pytest

import lifecycle as lc
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer
from test_gpu_temporal_tiles import FRAMES, HEIGHT, SHAPE, SPP, TILE, WIDTH, _camera, _device, _render, _tp

pytestmark = pytest.mark.gpu

OUTPUT, ALBEDO, NORMAL, MOMENTS = 0, 1, 2, 3
MIN_SAMPLES = 2


def _guide(twk):
    return twk._lib.DenoiserGeometry(sigmaPosition=0.02, instanceStop=1)


def _copies(twk, dev):
    """Device copies of the handle's AOVs, which have no pointer getter."""
    arrays = (dev.readAov(0, raw=True), dev.readAov(1, raw=True))
    buffers = [_DeviceBuffer(twk, a.nbytes) for a in arrays]
    for buf, a in zip(buffers, arrays):
        buf.upload(a)
    return buffers


@pytest.fixture(scope="module")
def single(twk):
    """{half: (denoised after the first frame, denoised after the orbit)} of ONE handle; computed once."""
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    app = lc.make_app(twk, load_app, shape)
    out = {}
    for half in (False, True):
        dev = _device(twk, app, shape, half=half)
        first = None
        for f in range(FRAMES):
            dev.updateCamera(0, _camera(twk, app, f))
            dev.setSampleOffset(f * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.temporalAccumulate(_tp(twk))
            if f == 0:
                dev.denoise(minSamples=MIN_SAMPLES, geometry=_guide(twk))
                first = lc._words(dev.readDenoised(raw=True))
                dev.denoise(minSamples=MIN_SAMPLES)
                assert not np.array_equal(lc._words(dev.readDenoised(raw=True)), first), "the guide changes the picture"
        colour, _, moments, _ = dev.temporalDevicePointers()
        guides = _copies(twk, dev)
        dev.denoise(None, colour, guides[0].ptr.value, guides[1].ptr.value, shape=SHAPE, moments=moments, minSamples=MIN_SAMPLES,
                    geometry=_guide(twk), geometryBuffer=dev.geometryDevicePointer()[0])
        orbit = lc._words(dev.readDenoised(raw=True, shape=SHAPE))
        for g in guides:
            g.free()
        assert not np.array_equal(orbit, first)
        out[half] = (first, orbit)
        dev.close()
    app.close()
    return out


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("n", [2, 3])
def test_the_filter_on_assembled_planes_equals_the_single_handle(twk, single, n, half):
    first, orbit = single[half]
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    app = lc.make_app(twk, load_app, shape)
    devs = [_device(twk, app, shape, index=i, count=n, half=half) for i in range(n)]
    primary = devs[0]
    planes = (OUTPUT, ALBEDO, NORMAL, MOMENTS)
    for f in range(FRAMES):
        _render(devs, _camera(twk, app, f), f)
        primary.assembleWithGeometry(devs, planes)
        primary.temporalAccumulateAssembled(_tp(twk))
        if f == 0:
            # the frame's own planes; the camera is the primary's camera 0 (camera=None)
            primary.denoise(None, *[primary.assembledDevicePointer(p)[0] for p in (OUTPUT, ALBEDO, NORMAL)], shape=SHAPE,
                            moments=primary.assembledDevicePointer(MOMENTS)[0], minSamples=MIN_SAMPLES, geometry=_guide(twk),
                            geometryBuffer=primary.assembledGeometryDevicePointer()[0])
            diff = lc.first_difference(lc._words(primary.readDenoised(raw=True, shape=SHAPE)), first)
            assert diff is None, f"{n} handles, one frame: {diff}"
    colour, _, moments, _ = primary.temporalDevicePointers()
    primary.denoise(None, colour, primary.assembledDevicePointer(ALBEDO)[0], primary.assembledDevicePointer(NORMAL)[0], shape=SHAPE, moments=moments,
                    minSamples=MIN_SAMPLES, geometry=_guide(twk), geometryBuffer=primary.assembledGeometryDevicePointer()[0])
    diff = lc.first_difference(lc._words(primary.readDenoised(raw=True, shape=SHAPE)), orbit)
    assert diff is None, f"{n} handles, after the orbit: {diff}"
    for d in devs:
        d.close()
    app.close()
