"""-m gpu: the rectified merge on a frame tiled over several handles (twk_temporal_accumulate_assembled_rectified) against the
own-buffer twk_temporal_accumulate_rectified on one handle: byte equality after every frame.

The orbit of tests/test_gpu_temporal_tiles.py — the Cornell box at 61x37 with 8x8 tiles, three frames of 2 spp, 0.004 of a turn
apart, Temporal(maxHistory=32, positionTolerance=0.1), the cascade and its temporal merge on — with the emission halved by
twk_update_light on EVERY handle before the third frame, on 2 and on 3 handles sharing this GPU, in both output formats. The merged
colour, moments, layers and the trust plane are compared. The equality is not vacuous: in the third frame the single handle's trust
is below 1 on some pixels."""
import pytest

import lifecycle as lc
from conftest import load_app
from test_gpu_temporal_tiles import FRAMES, HEIGHT, MERGED, SPP, TILE, WIDTH, _assert_same, _camera, _close, _device, _tp

pytestmark = pytest.mark.gpu


def _halve(app, devs):
    (light,) = app.lights
    for k in range(3):
        light.emission[k] = light.emission[k] * 0.5
    for d in devs:
        d.updateLight(0, light)


def _merged(dev):
    return {"colour": lc._words(dev.readTemporal()), "moments": lc._words(dev.readTemporalMoments()), "layers": lc._words(dev.readTemporalCascade()),
            "trust": lc._words(dev.readTemporalTrust())}


@pytest.fixture(scope="module")
def single(twk):
    """{half: [the merged buffers and the trust after each frame]} of ONE handle running the own-buffer rectified loop; computed once."""
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    out = {}
    for half in (False, True):
        app = lc.make_app(twk, load_app, shape)
        dev = _device(twk, app, shape, half=half)
        dev.enableTemporalCascade(True)
        frames = []
        for f in range(FRAMES):
            dev.updateCamera(0, _camera(twk, app, f))
            if f == FRAMES - 1:
                _halve(app, [dev])
            dev.setSampleOffset(f * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.temporalAccumulateRectified(_tp(twk))
            frames.append(_merged(dev))
        trust = dev.readTemporalTrust()
        assert trust.shape == (HEIGHT, WIDTH) and (trust < 1).any() and (trust == 1).any()
        out[half] = frames
        dev.close()
        app.close()
    return out


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("n", [2, 3])
def test_the_rectified_orbit_on_tiles_equals_the_orbit_on_one_device(twk, single, n, half):
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    app = lc.make_app(twk, load_app, shape)
    devs = [_device(twk, app, shape, index=i, count=n, half=half) for i in range(n)]
    primary = devs[0]
    primary.enableTemporalCascade(True)
    for f in range(FRAMES):
        for d in devs:
            d.updateCamera(0, _camera(twk, app, f))
        if f == FRAMES - 1:
            _halve(app, devs)
        for d in devs:
            d.setSampleOffset(f * SPP)
            for it in range(SPP):
                d.render(it)
            d.renderGeometryTile()
        primary.assembleWithGeometry(devs, MERGED)
        primary.temporalAccumulateAssembledRectified(_tp(twk))
        _assert_same(_merged(primary), single[half][f], f"{n} handles, frame {f}")
    assert primary.temporalTrustDevicePointer()[1] == WIDTH * HEIGHT * 4
    # the refusals are twk_temporal_accumulate_assembled's, under this call's name, plus the parameters'
    L = twk._lib
    with pytest.raises(twk.TwkError) as e:
        primary.temporalAccumulateAssembledRectified(_tp(twk), L.TemporalRectify(radius=7))
    assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_temporal_accumulate_assembled_rectified" in str(e.value) and "radius" in str(e.value)
    primary.updateCamera(0, _camera(twk, app, FRAMES))
    with pytest.raises(twk.TwkError) as e:
        primary.temporalAccumulateAssembledRectified(_tp(twk))
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_temporal_accumulate_assembled_rectified" in str(e.value) and "stale" in str(e.value)
    _close(app, devs)
