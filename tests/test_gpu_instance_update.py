"""-m gpu: twk_update_instance_transform — the handle renders like a fresh handle built with the new transform, byte for byte, in
both output formats, flattened and two-level, and again after the update back; the temporal history survives the update, and the
own-buffer merges (plain and rectified, with the cascade's layers) look it up where the instance was: they equal the explicit moving
forms fed the read-back buffers and the table twk_read_temporal_motion hands out, and equal the restatement
tests/temporal_motion_restate.py; and the refusals.

The scene is the Cornell box at 61x37, 4 spp. The moved instance is the mirror sphere (instance 6, radius 0.5 at (-0.4, 0.5, -0.25));
the camera looks down -z from (0, 1, 3.41). The step (0, 0.6, 0.5) lifts the sphere clear of the glass sphere and brings it 0.5
towards the camera: 0.78 in all, against a tolerance of 0.1 x the distance to the camera (about 2.7 at its new place: 0.27)."""
import numpy as np
import pytest

import lifecycle as lc
from conftest import load_app
from temporal_motion_restate import RECORD, expect_rectify_moving, expect_temporal_moving, instance_motion, restate_cascade_moving
from temporal_restate import F, U32, camera_array
from test_gpu_denoise_variance import _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_temporal import _frame, _moved, _same

pytestmark = pytest.mark.gpu

RES, SPP = (61, 37), 4
SPHERE, LIGHT = 6, 0
STEP = (0.0, 0.6, 0.5)
SYSTEM, SCENE = "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt"


def _stepped(transform, step=STEP):
    t = np.array(transform, F).reshape(12).copy()
    t[[3, 7, 11]] += np.array(step, F)
    return t


def _device(twk, app, half=False, two_level=False, transforms=None, cascade=False):
    """A handle on the application's scene. transforms: {instance: transform} — the scene is then handed over again with them, the
    only way to move an instance there was: twk_clear_scene, every geometry and instance again, twk_build."""
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.enableAov(True)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    if cascade:
        dev.enableCascade(True)
    app.initDevice(dev)
    if half:
        dev.setOutputFormat(lc.HALF4)
    if two_level:
        dev.setFlattenPolicy(0, 0)
    if transforms is not None:
        dev.clearScene()
        for k in range(app.info.numGeometries):
            dev.addGeometry(*app.geometry(k))
        for i, (g, t, m, l) in enumerate(app.instances):
            dev.addInstance(g, transforms.get(i, t), m, l)
    if two_level or transforms is not None:
        dev.build()
    return dev


def _pictures(dev, half):
    """4 spp from iteration 0 and the geometry AOV: every buffer a frame leaves, as words."""
    dev.setSampleOffset(0)
    for it in range(SPP):
        dev.render(it)
    dev.renderGeometry()
    return {"colour": lc._words(dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()), "albedo": lc._words(dev.readAov(0, raw=True)),
            "normal": lc._words(dev.readAov(1, raw=True)), "moments": lc._words(dev.readMoments()), "geometry": lc._words(dev.readGeometry())}


def _assert_same(got, want, what):
    for key in want:
        diff = lc.first_difference(got[key], want[key])
        assert diff is None, f"{what}, {key}: {diff}"


@pytest.mark.parametrize("two_level", [False, True], ids=["flattened", "two-level"])
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_an_updated_handle_renders_like_a_fresh_one(twk, half, two_level):
    app = load_app(twk, SYSTEM, SCENE, RES)
    original = app.instance(SPHERE)[1]
    moved = _stepped(original)
    dev = _device(twk, app, half, two_level)
    info = dev.buildInfo()
    assert info["flattenedInstances"] == (0 if two_level else info["instances"])
    before = _pictures(dev, half)
    assert np.array_equal(dev.instanceTransform(SPHERE), original)
    dev.updateInstanceTransform(SPHERE, moved)
    assert np.array_equal(dev.instanceTransform(SPHERE), moved)
    with pytest.raises(twk.TwkError) as e:  # the geometry AOV is stale
        dev.temporalAccumulate()
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE and "twk_render_geometry" in str(e.value)
    fresh = _device(twk, app, half, two_level, {SPHERE: moved})
    want = _pictures(fresh, half)
    fresh.close()
    assert lc.first_difference(want["geometry"], before["geometry"]) is not None and lc.first_difference(want["colour"], before["colour"]) is not None, "the move shows"
    _assert_same(_pictures(dev, half), want, "after the update, against a fresh handle built with the new transform")
    dev.updateInstanceTransform(SPHERE, original)
    _assert_same(_pictures(dev, half), before, "after the update back")
    dev.close()
    app.close()


def test_refusals(twk):
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    name = "twk_update_instance_transform"

    def refused(code, call, *words):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and name in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    app = load_app(twk, SYSTEM, SCENE, (32, 32))
    identity = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    unbuilt = twk.Device(ordinal=0, miss=app.info.miss)
    refused(STATE, lambda: unbuilt.updateInstanceTransform(0, identity), "twk_build")
    unbuilt.close()
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    original = dev.instanceTransform(SPHERE)
    refused(VALUE, lambda: dev.updateInstanceTransform(-1, identity), "instance id")
    refused(VALUE, lambda: dev.updateInstanceTransform(app.info.numInstances, identity), "instance id")
    for word, value in ((0, np.nan), (7, np.inf), (11, -np.inf)):
        bad = identity.copy()
        bad[word] = value
        refused(VALUE, lambda: dev.updateInstanceTransform(SPHERE, bad), "finite")
    flat = identity.copy()
    flat[5] = 0.0
    refused(VALUE, lambda: dev.updateInstanceTransform(SPHERE, flat), "determinant")
    assert app.instance(LIGHT)[3] >= 0
    refused(VALUE, lambda: dev.updateInstanceTransform(LIGHT, identity), "light")
    assert L.lib.twk_update_instance_transform(dev.handle, SPHERE, None) == VALUE and name in L.lib.twk_last_error().decode()
    assert np.array_equal(dev.instanceTransform(SPHERE), original), "a refused update changes nothing"
    dev.render(0)  # ... and the handle still renders
    dev.synchronizeStream()
    name = "twk_get_instance_transform"
    refused(VALUE, lambda: dev.instanceTransform(app.info.numInstances), "instance id")
    count = L.C.c_int(-1)
    assert L.lib.twk_read_temporal_motion(dev.handle, None, L.C.c_size_t(0), L.C.byref(count)) == 0 and count.value == 0
    dev.close()
    app.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("rectified", [False, True], ids=["plain", "rectified"])
def test_the_history_survives_the_update(twk, rectified, half):
    """Frame 1 merged, the sphere moved (two updates: the first to somewhere else), the camera a small step along its orbit, frame 2
    rendered and merged with the cascade's layers through the merge. The own-buffer results equal the restatement on the buffers read
    back with the table read back, and equal the explicit moving forms on the same buffers. And the input check: on the sphere's pixels
    the restatement takes history at more than half of them with the table, and at strictly fewer without it."""
    L = twk._lib
    tp, rp = L.Temporal(maxHistory=32, positionTolerance=0.1), (L.TemporalRectify() if rectified else None)
    app = load_app(twk, SYSTEM, SCENE, RES)
    original = app.instance(SPHERE)[1]
    moved = _stepped(original)
    dev = _device(twk, app, half, cascade=True)
    dev.enableTemporalCascade(True)
    raw = lambda: dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()
    merge = (lambda: dev.temporalAccumulateRectified(tp, rp)) if rectified else (lambda: dev.temporalAccumulate(tp))
    cameras = [app.cameras[0], _moved(twk, app, 0.004)]
    dev.updateCamera(0, cameras[0])
    _frame(dev, 0, SPP)
    first = (raw(), dev.readMoments(), dev.readGeometry(), dev.readCascade())
    merge()
    assert len(dev.readTemporalMotion()) == 0, "no history, no table"
    kept = (first[0].astype(F), first[1], first[2])  # the first merge copies the frame through
    _same(dev.readTemporal(), kept[0], "frame 1: colour")
    _same(dev.readTemporalCascade(), first[3], "frame 1: layers")
    dev.updateInstanceTransform(SPHERE, _stepped(original, (0.1, 0.1, 0.1)))
    dev.updateInstanceTransform(SPHERE, moved)
    dev.updateCamera(0, cameras[1])
    _frame(dev, SPP, SPP)
    colour_raw, mc, g, layers = raw(), dev.readMoments(), dev.readGeometry(), dev.readCascade()
    merge()
    table = np.frombuffer(bytes(dev.readTemporalMotion()), RECORD).copy()
    assert table.shape == (app.info.numInstances,) and table["moved"].tolist() == [int(i == SPHERE) for i in range(app.info.numInstances)]
    assert table[SPHERE].tobytes() == instance_motion(original, moved).tobytes() == bytes(twk.instance_motion(original, moved))
    cam = camera_array(cameras[0])
    what = f"frame 2, {'rectified' if rectified else 'plain'}"
    if rectified:
        expect = expect_rectify_moving(colour_raw, mc, g, kept, cam, 32, 0.1, rp.radius, rp.minTaps, rp.gamma, table)
        trust = expect[3]
        _same(dev.readTemporalTrust(), trust, what + ": trust")
        took, took_without = expect[4], expect_rectify_moving(colour_raw, mc, g, kept, cam, 32, 0.1, rp.radius, rp.minTaps, rp.gamma, None)[4]
    else:
        colour, history_out, moments, took = expect_temporal_moving(colour_raw, mc, g, kept, cam, 32, 0.1, table)
        expect, trust = (colour, history_out, moments), None
        took_without = expect_temporal_moving(colour_raw, mc, g, kept, cam, 32, 0.1, None)[3]
    _same(dev.readTemporal(), expect[0].astype(F), what + ": colour")
    _same(dev.readTemporalMoments(), expect[2], what + ": moments")
    expect_layers = restate_cascade_moving(layers, g, (first[3], kept[2]), cam, 32, 0.1, table, trust)[0]
    own_layers = dev.readTemporalCascade()
    _same(own_layers, expect_layers, what + ": layers")
    # the input check
    sphere = g[..., 3].view(U32) == SPHERE + 1
    print(f"\nsphere pixels {sphere.sum()}, took history with the table {(sphere & took).sum()}, without {(sphere & took_without).sum()}")
    assert sphere.sum() > 40 and (sphere & took).sum() > 0.5 * sphere.sum() and (sphere & took).sum() > (sphere & took_without).sum()
    # the explicit moving forms on the buffers read back
    height, width = mc.shape[:2]
    buffers = _upload(twk, (colour_raw, mc, g) + kept + (layers, first[3], table.view(np.uint8)) + ((trust,) if rectified else ()))
    p = [b.ptr.value for b in buffers]
    outs = [_DeviceBuffer(twk, colour_raw.nbytes), _DeviceBuffer(twk, mc.nbytes), _DeviceBuffer(twk, mc.nbytes), _DeviceBuffer(twk, width * height * 4), _DeviceBuffer(twk, layers.nbytes)]
    o = [b.ptr.value for b in outs]
    dev.temporalAccumulateMoving(tp, rp, L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], cameras[0]), p[8], len(table), (height, width), o[0], o[1], o[2],
                                 o[3] if rectified else None)
    dev.temporalAccumulateCascadeMoving(tp, None, p[6], p[2], p[7], p[5], cameras[0], p[9] if rectified else None, p[8], len(table), (height, width), o[4])
    dev.synchronizeStream()
    _same(outs[0].download(colour_raw.shape, colour_raw.dtype).astype(F), dev.readTemporal(), what + ": the explicit form's colourOut against the own-buffer form")
    _same(outs[2].download(mc.shape, F), dev.readTemporalMoments(), what + ": the explicit form's momentsOut against the own-buffer form")
    if rectified:
        _same(outs[3].download((height, width), F), dev.readTemporalTrust(), what + ": the explicit form's trustOut against the own-buffer form")
    _same(outs[4].download(layers.shape, F), own_layers, what + ": the explicit cascade form against the own-buffer form")
    for buf in buffers + outs:
        buf.free()
    # a third frame with nothing moved since: no table again, the existing kernels
    _frame(dev, 2 * SPP, SPP)
    merge()
    assert len(dev.readTemporalMotion()) == 0
    dev.close()
    app.close()
