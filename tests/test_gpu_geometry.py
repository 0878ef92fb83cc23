"""-m gpu: the geometry AOV (twk_enable_geometry, twk_render_geometry) — one closest-hit ray through the centre of every pixel,
(world position, bits of instance + 1) or zeros for a miss. The centre rays are restated in numpy float32 (tests/temporal_restate.py
centre_rays: primaryRay's pinhole branch with the jitter 0.5) and traced with Device.traceRays, the same single-ray traversal; the
AOV must equal P + t d in every bit and the instance words everywhere."""
import numpy as np
import pytest

from conftest import load_app
from temporal_restate import F, U32, centre_rays
from test_gpu_denoise_sampled import _rendered

pytestmark = pytest.mark.gpu

RES = (61, 37)


def _expected(twk, dev, cam, width, height, epsilon):
    P, d = centre_rays(cam, width, height)
    rays = np.empty((height, width, 8), F)
    rays[..., 0:3], rays[..., 3], rays[..., 4:7], rays[..., 7] = P, F(epsilon), d, F(1.0e27)
    tbg, ids = dev.traceRays(rays)
    t, inst = tbg[:, 0].reshape(height, width), ids[:, 0].reshape(height, width)
    g = np.zeros((height, width, 4), F)
    for k in range(3):
        g[..., k] = P[k] + t * d[..., k]
    g[..., 3] = (inst + 1).astype(U32).view(F)
    g[inst < 0] = 0
    return g, inst


@pytest.mark.parametrize("flatten", [None, (0, 0)], ids=["flattened", "two-level"])
def test_the_aov_is_the_centre_rays_first_hit(twk, flatten):
    """The scene the denoiser tests render, under the default flatten policy (one world-space tree) and (0, 0) (every instance entered)."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", RES)
    if flatten is None:
        dev = _rendered(twk, 1, res=RES)
    else:  # _rendered's scene with the policy set before the build
        dev = twk.Device(ordinal=0, miss=app.info.miss)
        dev.setFlattenPolicy(*flatten)
        app.initDevice(dev)
        dev.setShaderVariant(1)
        dev.render(0)
    flattened = dev.buildInfo()["flattenedInstances"]
    assert (flattened > 0) if flatten is None else (flattened == 0)
    cam = app.cameras[0]
    dev.enableGeometry(True)
    assert not dev.readGeometry().any(), "the buffer starts zeroed"
    dev.renderGeometry()
    got = dev.readGeometry()
    expect, inst = _expected(twk, dev, cam, RES[0], RES[1], app.state.epsilonFactor * F(1.0e-7))
    assert np.array_equal(got[..., 3].view(U32), expect[..., 3].view(U32)), "instance words"
    assert np.array_equal(got.view(U32), expect.view(U32)), "positions"
    assert (inst >= 0).mean() > 0.5 and len(np.unique(inst[inst >= 0])) >= 4
    ptr, nbytes = dev.geometryDevicePointer()
    assert ptr and nbytes == RES[0] * RES[1] * 16
    # a camera that looks away from the box: every ray misses, every word is zero
    away = twk.CameraDefinition()
    for k in range(3):
        away.P[k], away.U[k], away.V[k], away.W[k] = cam.P[k] - 100.0 * cam.W[k], -cam.U[k], cam.V[k], -cam.W[k]
    dev.updateCamera(0, away)
    dev.renderGeometry()
    missed = dev.readGeometry()
    expect_away, inst_away = _expected(twk, dev, away, RES[0], RES[1], app.state.epsilonFactor * F(1.0e-7))
    assert (inst_away < 0).all() and not missed.view(U32).any() and np.array_equal(missed.view(U32), expect_away.view(U32))
    # rendering does not touch the AOV, and the AOV does not touch the picture
    dev.updateCamera(0, cam)
    dev.renderGeometry()
    before = dev.getOutputBufferHost()
    dev.render(1)
    assert np.array_equal(dev.readGeometry().view(U32), expect.view(U32))
    dev.enableGeometry(False)
    dev.enableGeometry(True)
    assert not dev.readGeometry().any() and not np.array_equal(before, dev.getOutputBufferHost())
    dev.close()


def test_misses_are_zero_words(twk):
    """Whatever the shipped camera sees: a miss word is 0 with the position (0, 0, 0); a hit word is an instance index + 1."""
    dev = _rendered(twk, 1, res=RES)
    dev.enableGeometry(True)
    dev.renderGeometry()
    g = dev.readGeometry()
    w = g[..., 3].view(U32)
    assert not g[w == 0].any() and (w > 0).any() and w.max() <= 64
    dev.close()


def test_refusals(twk):
    L = twk._lib
    INVALID_STATE = L.TWK_ERROR_INVALID_STATE

    def refused(call, name="twk_render_geometry"):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == INVALID_STATE and name in str(e.value), str(e.value)

    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", RES)
    bare = twk.Device(ordinal=0, miss=app.info.miss)
    bare.enableGeometry(True)
    refused(bare.renderGeometry)                       # before twk_build
    bare.close()
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    refused(dev.renderGeometry)                        # geometry off
    refused(dev.readGeometry, "twk_read_geometry")
    refused(dev.geometryDevicePointer, "twk_get_geometry_device_pointer")
    dev.enableGeometry(True)
    dev.renderGeometry()
    for lens in (1, 2):                                # fisheye, sphere
        st = app.state
        st.lensShader = lens
        dev.setState(st)
        refused(dev.renderGeometry)
    dev.setState(app.state)
    dev.renderGeometry()
    dev.close()
    tile = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tile, distribution=1)
    tile.enableGeometry(True)
    refused(tile.renderGeometry)                       # a packed tile buffer
    tile.close()
    cut = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", RES)
    dev = twk.Device(ordinal=0, miss=cut.info.miss)
    dev.initTexture(1, np.ones((4, 4, 4), F))
    cut.initDevice(dev)
    mats = cut.materials
    mats[0].useCutoutTexture = 1
    dev.initMaterials(mats)
    dev.enableGeometry(True)
    refused(dev.renderGeometry)                        # a cutout texture in use
    dev.close()
