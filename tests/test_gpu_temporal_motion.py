"""-m gpu: the temporal merges with a table of instance motion (twk_temporal_accumulate_moving, twk_temporal_accumulate_cascade_moving;
csrc/temporal_motion_device.h) against the numpy restatement tests/temporal_motion_restate.py: the plain, the rectified, the cascade's
and the trusted cascade's merge equal it in every bit, in both output formats, at the existing temporal tests' shapes; without a
table the calls are the existing ones byte for byte; the inputs are untouched; the refusals; and on a small rendered scene whose box
moves between two frames, the merge with the table beats the frame alone and is not beaten by the merge without it."""
import numpy as np
import pytest

from shading_fuzz import Scene, default_state, feed, material, parallelogram_light, transform
from temporal_motion_restate import (RECORD, expect_rectify_moving, expect_temporal_moving, moving_frames, moving_layers, restate_cascade_moving,
                                     restate_temporal_moving)
from temporal_restate import F, U32, camera_array, restate_temporal
from test_gpu_denoise_variance import _small_device, _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_temporal import _camera, _same

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (64, 4)]
K = 6


def _table_buffer(twk, table):
    buf = _DeviceBuffer(twk, max(64, table.nbytes))
    buf.upload(table.view(np.uint8))
    return buf


def _merge(twk, dev, tp, rp, arrays, table, num_motion, moving=True):
    """The explicit form on uploaded frames: (colourOut, historyOut, momentsOut, trustOut or None) downloaded; the inputs and the
    table are checked to be untouched. moving False: the existing calls, twk_temporal_accumulate / twk_temporal_accumulate_rectified."""
    L = twk._lib
    cur, mc, g, hc, hm, hg, cam = arrays
    height, width = mc.shape[:2]
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg))
    motion = _table_buffer(twk, table)
    outs = [_DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, hc.nbytes), _DeviceBuffer(twk, hm.nbytes), _DeviceBuffer(twk, width * height * 4)]
    p = [b.ptr.value for b in buffers]
    o = [b.ptr.value for b in outs]
    current, hist = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    if moving:
        dev.temporalAccumulateMoving(tp, rp, current, hist, motion.ptr.value if num_motion is not None else None, num_motion or 0, (height, width), o[0], o[1], o[2],
                                     o[3] if rp is not None else None)
    elif rp is not None:
        dev.temporalAccumulateRectified(tp, rp, current, hist, (height, width), *o)
    else:
        dev.temporalAccumulate(tp, current, hist, (height, width), *o[:3])
    dev.synchronizeStream()
    got = (outs[0].download(cur.shape, cur.dtype), outs[1].download(hc.shape, F), outs[2].download(hm.shape, F), outs[3].download((height, width), F) if rp is not None else None)
    for buf, arr in zip(buffers, (cur, mc, g, hc, hm, hg)):
        _same(buf.download(arr.shape, arr.dtype), arr, "an input after twk_temporal_accumulate_moving")
    assert motion.download(table.shape, RECORD).tobytes() == table.tobytes(), "the table after twk_temporal_accumulate_moving"
    for buf in buffers + outs + [motion]:
        buf.free()
    return got


def _merge_layers(twk, dev, tp, arrays, trust, table, num_motion, moving=True):
    """The explicit form of the cascade's merge on uploaded layers; moving False: the existing calls."""
    L = twk._lib
    Lc, g, Hl, hg, cam = arrays
    height, width = g.shape[:2]
    uploads = (Lc, g, Hl, hg) + ((trust,) if trust is not None else ())
    buffers = _upload(twk, uploads)
    motion = _table_buffer(twk, table)
    out = _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    cp = L.Cascade(Lc.shape[0], 1.0, 8.0)
    t = p[4] if trust is not None else None
    if moving:
        dev.temporalAccumulateCascadeMoving(tp, cp, p[0], p[1], p[2], p[3], _camera(twk, cam), t, motion.ptr.value if num_motion is not None else None, num_motion or 0,
                                            (height, width), out.ptr.value)
    elif trust is not None:
        dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], p[2], p[3], _camera(twk, cam), t, (height, width), out.ptr.value)
    else:
        dev.temporalAccumulateCascade(tp, cp, p[0], p[1], p[2], p[3], _camera(twk, cam), (height, width), out.ptr.value)
    dev.synchronizeStream()
    got = out.download(Lc.shape, F)
    for buf, arr in zip(buffers, uploads):
        _same(buf.download(arr.shape, arr.dtype), arr, "an input after twk_temporal_accumulate_cascade_moving")
    for buf in buffers + [out, motion]:
        buf.free()
    return got


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("width,height", SIZES)
def test_explicit_forms_equal_the_restatement_bit_for_bit(twk, width, height, half):
    """37x23 (no multiple of a wave or a block, partial tiles of the rectified merge's second launch) and 64x4 (one block, four rows:
    most reprojections leave the picture). The table: an unmoved record, a translation, a NaN matrix, a rotation with non-uniform
    scale — with numMotion 3 (instance 4 beyond the table: unmoved), 4, and 70 (a table the kernels read from global memory instead of
    their block's LDS copy: csrc/temporal_motion_device.h TWK_MOTION_STAGED_RECORDS). Then without a table: the existing calls' bytes."""
    L = twk._lib
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance, table = moving_frames(width, height)
    Lc, gl, (Hl, hgl), cam_l, _, _, _ = moving_layers(width, height, K)
    if half:
        with np.errstate(over="ignore"):
            cur = cur.astype(np.float16)
    dev = _small_device(twk, half)
    tp, rp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.TemporalRectify(3, 8, 3.0)
    frames, layers = (cur, mc, g, hc, hm, hg, cam), (Lc, gl, Hl, hgl, cam_l)
    trust = np.random.default_rng(5).uniform(0.0, 1.0, (height, width)).astype(F)
    what = f"{width}x{height}, {'rgba16f' if half else 'rgba32f'}"
    long = np.concatenate([table, np.repeat(table[:1], 66)])  # 70 records, above what a block stages in LDS: read from global memory
    for num_motion, table in ((3, table), (4, table), (70, long)):
        used = table[:num_motion]
        expect = expect_temporal_moving(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, used)
        got = _merge(twk, dev, tp, None, frames, table, num_motion)
        for k, name in enumerate(("colourOut", "historyOut", "momentsOut")):
            _same(got[k], expect[k], f"{what}, numMotion {num_motion}, plain {name}")
        assert expect[3].sum() > 10
        expect = expect_rectify_moving(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, rp.radius, rp.minTaps, rp.gamma, used)
        got = _merge(twk, dev, tp, rp, frames, table, num_motion)
        for k, name in enumerate(("colourOut", "historyOut", "momentsOut", "trustOut")):
            _same(got[k], expect[k], f"{what}, numMotion {num_motion}, rectified {name}")
        _same(_merge_layers(twk, dev, tp, layers, None, table, num_motion), restate_cascade_moving(Lc, gl, (Hl, hgl), cam_l, max_history, tolerance, used)[0],
              f"{what}, numMotion {num_motion}, cascade")
        _same(_merge_layers(twk, dev, tp, layers, trust, table, num_motion), restate_cascade_moving(Lc, gl, (Hl, hgl), cam_l, max_history, tolerance, used, trust)[0],
              f"{what}, numMotion {num_motion}, trusted cascade")
    # the table does something here: with it the plain merge differs from the merge without
    table = long[:4]
    moved = _merge(twk, dev, tp, None, frames, table, 4)
    for num_motion, label in ((None, "motion NULL"), (0, "numMotion 0")):
        for r in (None, rp):
            got, existing = _merge(twk, dev, tp, r, frames, table, num_motion), _merge(twk, dev, tp, r, frames, table, 0, moving=False)
            for k, name in enumerate(("colourOut", "historyOut", "momentsOut", "trustOut")):
                if got[k] is not None:
                    _same(got[k], existing[k], f"{what}, {label}, {'rectified' if r else 'plain'} {name} against the existing call")
            if r is None and num_motion is None:
                assert (got[1].view(U32) != moved[1].view(U32)).any(axis=-1).sum() > 10
        for t in (None, trust):
            _same(_merge_layers(twk, dev, tp, layers, t, table, num_motion), _merge_layers(twk, dev, tp, layers, t, table, 0, moving=False),
                  f"{what}, {label}, {'trusted ' if t is not None else ''}cascade against the existing call")
    dev.close()


def test_refusals(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE

    def refused(call, name, *words):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == VALUE and name in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    width, height = 37, 23
    (cur, mc, g), (hc, hm, hg), cam, _, _, table = moving_frames(width, height)
    Lc, gl, (Hl, hgl), cam_l, _, _, _ = moving_layers(width, height, K)
    shape = (height, width)
    dev = _small_device(twk)
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg, Lc, gl, Hl, hgl))
    motion = _table_buffer(twk, table)
    out, trust, layers_out = _DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, width * height * 4), _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    m = motion.ptr.value
    current, history = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    name = "twk_temporal_accumulate_moving"
    merge = lambda rp=None, tp=None, c=current, h=history, t=m, n=4, s=shape, outs=(out.ptr.value, None, None, None): dev.temporalAccumulateMoving(tp, rp, c, h, t, n, s, *outs)
    merge()
    merge(L.TemporalRectify(), outs=(out.ptr.value, None, None, trust.ptr.value))
    refused(lambda: merge(c=None, h=None, s=None, outs=(None,) * 4), name, "explicit form")
    refused(lambda: merge(outs=(out.ptr.value, None, None, trust.ptr.value)), name, "trustOut")
    refused(lambda: merge(n=-1), name, "numMotion")
    refused(lambda: merge(t=m + 4), name, "16-byte aligned")
    refused(lambda: merge(outs=(m, None, None, None)), name, "overlaps the motion table")
    refused(lambda: merge(outs=(None, None, m + 128, None)), name, "overlaps the motion table")
    refused(lambda: merge(L.TemporalRectify(), outs=(None, None, None, m + 64)), name, "overlaps the motion table")
    # ... and every refusal of the calls it stands for
    refused(lambda: merge(tp=L.Temporal(maxHistory=0)), name, "maxHistory")
    refused(lambda: merge(L.TemporalRectify(radius=5)), name, "radius")
    refused(lambda: merge(outs=(p[3], None, None, None)), name, "overlaps an input")
    refused(lambda: merge(c=L.TemporalFrame(p[0], None, p[2])), name, "NULL")
    refused(lambda: merge(h=L.TemporalFrame(p[3], p[4], p[5], _camera(twk, np.zeros(12, F)))), name, "degenerate")
    refused(lambda: merge(s=(0, width)), name, "width and height")
    name = "twk_temporal_accumulate_cascade_moving"
    camera = _camera(twk, cam_l)
    cascade = lambda a=p[6], b=p[7], c=p[8], d=p[9], e=camera, t=None, tb=m, n=4, s=shape, o=layers_out.ptr.value: dev.temporalAccumulateCascadeMoving(None, None, a, b, c, d, e, t, tb, n, s, o)
    cascade()
    refused(lambda: cascade(n=-1), name, "numMotion")
    refused(lambda: cascade(tb=m + 8), name, "16-byte aligned")
    refused(lambda: cascade(o=m), name, "overlaps the motion table")
    refused(lambda: cascade(a=None), name, "NULL")
    refused(lambda: cascade(o=p[8]), name, "overlaps an input")
    refused(lambda: cascade(t=layers_out.ptr.value + 16), name, "overlaps the trust")
    for buf in buffers + [motion, out, trust, layers_out]:
        buf.free()
    dev.close()


# ---- quality: a box that moves between two frames ----------------------------------------------------------------------------------
WIDTH, HEIGHT, SPP, REFERENCE_SPP = 96, 54, 4, 256
BOX = 2  # the box's instance: floor 0, light 1, box 2
STEP = (0.45, 0.0, 0.4)  # 0.05 x the distance to the camera (4.5) is 0.225: each visible side face moves by more, perpendicular to itself


def _box_scene(twk, box_at):
    """A diffuse floor, a diffuse box standing on it and a square light above, through the ABI (no specular surface: the comparison
    must not depend on what a moved object reflects)."""
    s = Scene()
    s.miss = 0
    s.camera = twk.camera_frustum((0.0, 0.5, 0.0), 0.8, 0.62, 45.0, 4.5, WIDTH / HEIGHT)
    s.materials = [material(1, albedo=(0.0, 0.0, 0.0), thinwalled=1), material(0, albedo=(0.7, 0.7, 0.7)), material(0, albedo=(0.75, 0.4, 0.2))]
    light = parallelogram_light((-1.0, 3.5, -1.0), 2.0, (12.0, 12.0, 12.0))
    s.lights = [light]
    geometry = lambda mesh: (s.geometries.append((np.ascontiguousarray(mesh[0], np.float32), np.ascontiguousarray(mesh[1], np.uint32))), len(s.geometries) - 1)[1]
    s.instances.append((geometry(twk.mesh_plane(1, 1, 1)), transform(4.0), 1, -1))
    s.instances.append((geometry(twk.mesh_parallelogram(list(light.position), list(light.vecU), list(light.vecV), list(light.normal))), transform(), 0, 0))
    s.instances.append((geometry(twk.mesh_box()), transform(0.5, box_at), 2, -1))
    state = default_state(s, pathLengths=(2, 6))
    state.resolution[0], state.resolution[1] = WIDTH, HEIGHT
    return s, state


def _relative_rmse(image, reference, mask):
    d = (image[..., :3].astype(np.float64) - reference[..., :3])[mask]
    return float(np.sqrt((d * d).mean()) / reference[..., :3][mask].mean())


def test_a_moved_box_keeps_its_history(twk):
    """Two frames of 4 spp at 96x54, the box translated by STEP between them with updateInstanceTransform; the reference is 256 spp of
    the moved scene from samples the frames do not share. On the box's pixels that took history the merged colour's relative RMSE is
    strictly below the 4 spp frame's, and the plain merge WITHOUT the table (the explicit form on the same buffers) is not better than
    the merge with it."""
    L = twk._lib
    tp = L.Temporal(maxHistory=32, positionTolerance=0.05)
    first, moved = (0.0, 0.5, 0.0), (STEP[0], 0.5 + STEP[1], STEP[2])
    scene, state = _box_scene(twk, first)
    dev = twk.Device(ordinal=0, miss=0)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    feed(dev, scene, state)

    def frame(offset, spp):
        dev.setSampleOffset(offset)
        for it in range(spp):
            dev.render(it)
        dev.renderGeometry()

    frame(0, SPP)
    dev.temporalAccumulate(tp)
    history = (dev.readTemporal(), dev.readTemporalMoments(), dev.readGeometry())
    dev.updateInstanceTransform(BOX, transform(0.5, moved))
    frame(SPP, SPP)
    alone, mc, g = dev.getOutputBufferHost().copy(), dev.readMoments(), dev.readGeometry()
    dev.temporalAccumulate(tp)
    merged = dev.readTemporal()
    table = np.frombuffer(bytes(dev.readTemporalMotion()), RECORD)
    assert table.shape == (3,) and table["moved"].tolist() == [0, 0, 1]
    cam = camera_array(scene.camera)
    expect, _, took = restate_temporal_moving(alone, mc, g, history, cam, 32, 0.05, table)
    _same(merged, expect, "the own-buffer merge against the restatement")
    without, _, took_without = restate_temporal(alone, mc, g, history, cam, 32, 0.05)
    box = g[..., 3].view(U32) == BOX + 1
    carried = box & took
    print(f"\nbox pixels {box.sum()}, took history with the table {carried.sum()}, without {(box & took_without).sum()}")
    assert box.sum() > 300 and carried.sum() > 0.5 * box.sum() and carried.sum() > (box & took_without).sum()
    frame(1000, REFERENCE_SPP)
    reference = dev.getOutputBufferHost().astype(np.float64)
    dev.close()
    e_alone, e_merged, e_without = (_relative_rmse(a, reference, carried) for a in (alone, merged, without))
    print(f"relative RMSE on the box's pixels that took history: 4 spp {e_alone:.4f}, merged with the table {e_merged:.4f}, merged without {e_without:.4f}")
    assert e_merged < e_alone
    assert e_merged <= e_without
