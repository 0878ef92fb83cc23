"""-m gpu: the previous-position plane (twk_render_geometry_motion, csrc/temporal_carry_device.h). The centre rays are restated in
numpy (tests/temporal_restate.py centre_rays) and their hits taken with twk_trace_rays, the same single-ray traversal; the plane
restated from those hits (tests/temporal_carry_restate.py) must equal twk_read_previous_positions bit for bit, and the geometry AOV
the call writes must have the bytes of twk_render_geometry's. An independent check of what the plane MEANS: a deformation that is
also an affine map (the sphere scaled by 1.3 about its centre) must give the g' of the equivalent transform pair."""
import numpy as np
import pytest

import selective_scenes as S
from temporal_carry_restate import CARRY, previous_positions, to_ctypes
from temporal_motion_restate import RECORD
from temporal_restate import F, U32, centre_rays
from test_gpu_selective_update import QUALITIES, RES, SPP, _device, _instances, _step, app, parts  # noqa: F401  (app, parts: fixtures)
from vertex_update_scenes import deformed

pytestmark = pytest.mark.gpu


def _frame(dev, offset):
    dev.setSampleOffset(offset)
    for it in range(SPP):
        dev.render(it)


def _hits(dev, app):
    """The centre rays' hits with the scene as it is: (tbg [n, 3], instance [n], primitive [n], the geometry AOV they give [n, 4])."""
    width, height = RES
    P, d = centre_rays(app.cameras[0], width, height)
    rays = np.empty((height, width, 8), F)
    rays[..., 0:3], rays[..., 3], rays[..., 4:7], rays[..., 7] = P, F(app.state.epsilonFactor * F(1.0e-7)), d, F(1.0e27)
    tbg, ids = dev.traceRays(rays)
    t, inst = tbg[:, 0].reshape(height, width), ids[:, 0].reshape(height, width)
    g = np.zeros((height, width, 4), F)
    for k in range(3):
        g[..., k] = P[k] + t * d[..., k]
    g[..., 3] = (inst + 1).astype(U32).view(F)
    g[inst < 0] = 0
    return tbg, ids[:, 0].copy(), ids[:, 1].copy(), g.reshape(-1, 4)


def _tables(twk, parts, name, previous_transforms, current_transforms, previous_vertices):
    """The two tables of the restatement, built as the header says: previous_vertices {geometry: attributes as of the history's frame}."""
    instances = _instances(name, parts)
    index_base = np.concatenate([[0], np.cumsum([np.asarray(i).size for _, i in parts[0]])])
    positions, position_base = [], {}
    for geometry in sorted(previous_vertices):
        position_base[geometry] = sum(p.shape[0] for p in positions)
        a = np.array(previous_vertices[geometry], F).reshape(-1, 12)
        positions.append(np.concatenate([a[:, 0:3], np.zeros((a.shape[0], 1), F)], axis=1))
    motion, carry = np.zeros(len(instances), RECORD), np.zeros(len(instances), CARRY)
    for i, (geometry, _, _, _) in enumerate(instances):
        record = twk.instance_motion(previous_transforms[i], current_transforms[i])
        motion[i] = np.frombuffer(bytes(record), RECORD)[0]
        carry[i] = (previous_transforms[i], int(geometry in previous_vertices), position_base.get(geometry, 0), index_base[geometry], 0)
    indices = np.concatenate([np.asarray(i, U32).reshape(-1) for _, i in parts[0]])
    return indices, (np.concatenate(positions) if positions else np.zeros((0, 4), F)), motion, carry


@QUALITIES
@pytest.mark.parametrize("selective", [True, False], ids=["selective", "full"])
@pytest.mark.parametrize("name", ["flat", "two-level"])
def test_the_plane_equals_the_restatement(twk, app, parts, name, selective, quality):
    """flat: the sphere deformed, the box moved, the walls still. two-level: the shared sphere geometry deformed (twice: the oldest
    positions are the previous ones), one of its three instances also moved."""
    L = twk._lib
    width, height = RES
    instances = _instances(name, parts)
    moved_instance = {"flat": 4, "two-level": 5}[name]
    previous = [np.array(t, F).reshape(12) for _, t, _, _ in instances]
    dev = _device(twk, app, parts, name, quality, selective)

    # without a history: the plane is the geometry AOV, and the AOV is twk_render_geometry's
    dev.renderGeometry()
    aov = dev.readGeometry()
    dev.renderGeometryMotion()
    assert np.array_equal(dev.readGeometry().view(U32), aov.view(U32))
    assert np.array_equal(dev.readPreviousPositions().view(U32), aov.view(U32)), "no history: g' = g"
    pointer, nbytes = dev.previousPositionsDevicePointer()
    assert pointer and pointer % 16 == 0 and nbytes == width * height * 16

    # a frame merged: the history. Then the deformation and the move.
    _frame(dev, 0)
    dev.temporalAccumulate(L.Temporal(maxHistory=32, positionTolerance=0.1))
    with pytest.raises(twk.TwkError) as e:
        dev.readPreviousPositions()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_render_geometry_motion" in str(e.value), "the merge swapped the history: the plane is stale"
    dev.updateGeometryVertices(S.SPHERE, deformed(parts, S.SPHERE, 3))
    new = deformed(parts, S.SPHERE, 4)
    dev.updateGeometryVertices(S.SPHERE, new)
    current = [p.copy() for p in previous]
    current[moved_instance] = _step(previous[moved_instance], (0.05, 0.08, 0.04))
    dev.updateInstanceTransform(moved_instance, current[moved_instance])
    for call in (dev.readPreviousPositions, dev.previousPositionsDevicePointer):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == L.TWK_ERROR_INVALID_STATE, "an update leaves the plane stale, with the geometry AOV"

    dev.renderGeometry()
    aov = dev.readGeometry()
    dev.renderGeometryMotion()
    got = dev.readPreviousPositions()
    assert np.array_equal(dev.readGeometry().view(U32), aov.view(U32)), "the geometry AOV has the bytes of twk_render_geometry's"
    tbg, instance, primitive, g = _hits(dev, app)
    assert np.array_equal(g.view(U32), aov.reshape(-1, 4).view(U32))
    indices, positions, motion, carry = _tables(twk, parts, name, previous, current, {S.SPHERE: parts[0][S.SPHERE][0]})
    want = previous_positions(tbg, instance, primitive, g, indices, positions, motion, carry)
    assert np.array_equal(got.reshape(-1, 4).view(U32), want.view(U32)), "the plane against the restatement"
    host = twk.previous_positions_host(tbg, instance, primitive, g, indices, positions, to_ctypes(motion, L.InstanceMotion), to_ctypes(carry, L.InstanceCarry))
    assert np.array_equal(host.view(U32), want.view(U32)), "the host form on the same hits"

    # what the picture holds: misses, still walls (g' = g), the deformed sphere and, in flat, the moved box
    flat = got.reshape(-1, 4)
    same = np.all(flat[:, :3].view(U32) == g[:, :3].view(U32), axis=1)
    geometry_of = np.array([i[0] for i in instances])
    on_sphere = (instance >= 0) & (geometry_of[np.maximum(instance, 0)] == S.SPHERE)
    assert not flat[instance < 0].any()
    assert on_sphere.sum() >= 8 and not same[on_sphere].any(), "the sphere is in the picture (a 33 x 21 picture shows it on a dozen pixels), and every pixel of it was elsewhere"
    walls = (instance >= 0) & (instance < 4)
    assert walls.sum() > 100 and same[walls].all(), "the walls are where they were"
    if name == "flat":
        assert (instance == 4).sum() >= 4 and not same[instance == 4].any(), "the moved box"
    assert np.isfinite(flat).all()

    # a merge swaps the history: nothing is deformed, the plane is stale, and the next one is the geometry AOV again
    _frame(dev, SPP)
    dev.temporalAccumulate(L.Temporal(maxHistory=32, positionTolerance=0.1))
    assert not dev.geometryDeformed(S.SPHERE)
    dev.renderGeometryMotion()
    assert np.array_equal(dev.readPreviousPositions().view(U32), dev.readGeometry().view(U32))
    dev.close()


@QUALITIES
def test_a_scaled_sphere_gives_the_motion_of_the_equivalent_transform(twk, app, parts, quality):
    """The flat scene's sphere with its vertices scaled by 1.3 about its centre: a deformation that is also the affine map S. A point of
    it now at g was at g' = M (M S)^-1 g — X g of twk_instance_motion(previous = M, current = M S), evaluated here in float64. The
    plane must agree to 1e-4 absolute on every sphere pixel: its g' is about twenty float32 operations on coordinates of magnitude at
    most 4, which round to about 5e-6; 1e-4 is an order of magnitude above that."""
    L = twk._lib
    instance = 5
    M = np.array(_instances("flat", parts)[instance][1], np.float64).reshape(3, 4)
    old = np.array(parts[0][S.SPHERE][0], F).reshape(-1, 12)
    centre = ((old[:, 0:3].min(axis=0).astype(np.float64) + old[:, 0:3].max(axis=0)) / 2).astype(F)
    new = old.copy()
    new[:, 0:3] = centre + F(1.3) * (old[:, 0:3] - centre)
    dev = _device(twk, app, parts, "flat", quality, True)
    _frame(dev, 0)
    dev.renderGeometry()
    dev.temporalAccumulate(L.Temporal(maxHistory=32, positionTolerance=0.1))
    dev.updateGeometryVertices(S.SPHERE, new)
    dev.renderGeometryMotion()
    g, gp = dev.readGeometry().reshape(-1, 4), dev.readPreviousPositions().reshape(-1, 4)
    on_sphere = g[:, 3].view(U32) == instance + 1
    assert on_sphere.sum() >= 8, "the sphere is in the picture"
    Sm = np.concatenate([1.3 * np.eye(3), ((1.0 - 1.3) * centre.astype(np.float64)).reshape(3, 1)], axis=1)
    MS = M[:, :3] @ Sm
    MS[:, 3] += M[:, 3]
    record = twk.instance_motion(M.astype(F).reshape(12), MS.astype(F).reshape(12))
    X = np.array(list(record.previousFromCurrent), np.float64).reshape(3, 4)
    want = g[on_sphere, :3].astype(np.float64) @ X[:, :3].T + X[:, 3]
    error = np.abs(gp[on_sphere, :3].astype(np.float64) - want).max()
    moved_by = np.linalg.norm(gp[on_sphere, :3].astype(np.float64) - g[on_sphere, :3], axis=1)
    print(f"scaled sphere: {on_sphere.sum()} pixels, max |g' - X g| = {error:.3e}, the surface moved by {moved_by.min():.3f} .. {moved_by.max():.3f}")
    assert np.abs(g[:, :3]).max() <= 4.0 and np.abs(gp[:, :3]).max() <= 4.0, "the bound's premise: coordinates of magnitude at most 4"
    assert error <= 1e-4
    assert moved_by.min() > 0.01, "the deformation shows on every sphere pixel"
    dev.close()


def test_refusals(twk, app, parts):
    """twk_render_geometry's refusals, with its texts, under the new call's name."""
    L = twk._lib

    def refused(call, *words):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_render_geometry_motion" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    bare = twk.Device(ordinal=0, miss=app.info.miss)
    bare.enableGeometry(True)
    refused(bare.renderGeometryMotion, "twk_build")
    bare.close()
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    refused(dev.renderGeometryMotion, "twk_enable_geometry")
    dev.enableGeometry(True)
    for call in (dev.readPreviousPositions, dev.previousPositionsDevicePointer):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == L.TWK_ERROR_INVALID_STATE
    dev.renderGeometryMotion()
    assert dev.readPreviousPositions().shape == (RES[1], RES[0], 4)
    st = app.state
    st.lensShader = 1
    dev.setState(st)
    refused(dev.renderGeometryMotion, "pinhole")
    dev.setState(app.state)
    dev.close()
    tile = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tile, distribution=1)
    tile.enableGeometry(True)
    refused(tile.renderGeometryMotion, "packed tile")
    tile.close()


# ---- the merges read the plane: the Carried builds -------------------------------------------------------------------------------
from shading_fuzz import Scene, default_state, feed, material, parallelogram_light, transform  # noqa: E402
from temporal_carry_restate import (expect_rectify_carried, expect_temporal_carried, restate_cascade_carried, restate_temporal_carried,  # noqa: E402
                                    seeded_plane)
from temporal_motion_restate import moved_geometry, moving_frames, moving_layers  # noqa: E402
from temporal_restate import camera_array, restate_temporal  # noqa: E402
from test_gpu_denoise_variance import _small_device, _upload  # noqa: E402
from test_gpu_half_output import _DeviceBuffer  # noqa: E402
from test_gpu_temporal import _camera, _same  # noqa: E402
from test_gpu_temporal_motion import _merge as _merge_moving, _merge_layers as _merge_layers_moving  # noqa: E402

SIZES = [(37, 23), (64, 4)]
K = 6


def _merge(twk, dev, tp, rp, arrays, plane):
    """twk_temporal_accumulate_carried on uploaded frames: (colourOut, historyOut, momentsOut, trustOut or None) downloaded; the
    inputs and the plane are checked to be untouched. plane None: previousPositions NULL."""
    L = twk._lib
    cur, mc, g, hc, hm, hg, cam = arrays
    height, width = mc.shape[:2]
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg) + ((plane,) if plane is not None else ()))
    outs = [_DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, hc.nbytes), _DeviceBuffer(twk, hm.nbytes), _DeviceBuffer(twk, width * height * 4)]
    p = [b.ptr.value for b in buffers]
    o = [b.ptr.value for b in outs]
    current, hist = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    dev.temporalAccumulateCarried(tp, rp, current, hist, p[6] if plane is not None else None, (height, width), o[0], o[1], o[2], o[3] if rp is not None else None)
    dev.synchronizeStream()
    got = (outs[0].download(cur.shape, cur.dtype), outs[1].download(hc.shape, F), outs[2].download(hm.shape, F), outs[3].download((height, width), F) if rp is not None else None)
    for buf, arr in zip(buffers, (cur, mc, g, hc, hm, hg) + ((plane,) if plane is not None else ())):
        _same(buf.download(arr.shape, arr.dtype), arr, "an input after twk_temporal_accumulate_carried")
    for buf in buffers + outs:
        buf.free()
    return got


def _merge_layers(twk, dev, tp, arrays, trust, plane):
    """twk_temporal_accumulate_cascade_carried on uploaded layers; plane None: previousPositions NULL."""
    L = twk._lib
    Lc, g, Hl, hg, cam = arrays
    height, width = g.shape[:2]
    uploads = (Lc, g, Hl, hg) + ((trust,) if trust is not None else ()) + ((plane,) if plane is not None else ())
    buffers = _upload(twk, uploads)
    out = _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    t = p[4] if trust is not None else None
    pl = p[-1] if plane is not None else None
    dev.temporalAccumulateCascadeCarried(tp, L.Cascade(Lc.shape[0], 1.0, 8.0), p[0], p[1], p[2], p[3], _camera(twk, cam), t, pl, (height, width), out.ptr.value)
    dev.synchronizeStream()
    got = out.download(Lc.shape, F)
    for buf, arr in zip(buffers, uploads):
        _same(buf.download(arr.shape, arr.dtype), arr, "an input after twk_temporal_accumulate_cascade_carried")
    for buf in buffers + [out]:
        buf.free()
    return got


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("width,height", SIZES)
def test_explicit_carried_merges_equal_the_restatement_bit_for_bit(twk, width, height, half):
    """37 x 23 and 64 x 4 (neither pixel count is a multiple of 256). The four merges on a seeded plane (a deformation, rigid motion,
    w mismatches, elements that are not finite, plane misses); the identity plane and previousPositions NULL: the existing calls'
    bytes; the rigid-only plane: the *_moving calls' bytes with the table. The inputs are untouched (checked in the helpers)."""
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
    plane, plane_l = seeded_plane(g, table), seeded_plane(gl, table)
    expect = expect_temporal_carried(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, plane)
    got = _merge(twk, dev, tp, None, frames, plane)
    for k, name in enumerate(("colourOut", "historyOut", "momentsOut")):
        _same(got[k], expect[k], f"{what}, plain {name}")
    assert expect[3].sum() > 10
    expect = expect_rectify_carried(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, rp.radius, rp.minTaps, rp.gamma, plane)
    got = _merge(twk, dev, tp, rp, frames, plane)
    for k, name in enumerate(("colourOut", "historyOut", "momentsOut", "trustOut")):
        _same(got[k], expect[k], f"{what}, rectified {name}")
    for t in (None, trust):
        _same(_merge_layers(twk, dev, tp, layers, t, plane_l), restate_cascade_carried(Lc, gl, (Hl, hgl), cam_l, max_history, tolerance, plane_l, t)[0],
              f"{what}, {'trusted ' if t is not None else ''}cascade")
    # the identity plane and no plane: the existing calls; the rigid-only plane: the *_moving calls with the table
    for r in (None, rp):
        existing = _merge_moving(twk, dev, tp, r, frames, table, 0, moving=False)
        moving = _merge_moving(twk, dev, tp, r, frames, table, len(table))
        for given, want, label in ((g, existing, "identity plane"), (None, existing, "previousPositions NULL"), (moved_geometry(g, table), moving, "rigid-only plane")):
            got = _merge(twk, dev, tp, r, frames, given)
            for k, name in enumerate(("colourOut", "historyOut", "momentsOut", "trustOut")):
                if got[k] is not None:
                    _same(got[k], want[k], f"{what}, {label}, {'rectified' if r else 'plain'} {name}")
    for t in (None, trust):
        existing = _merge_layers_moving(twk, dev, tp, layers, t, table, 0, moving=False)
        moving = _merge_layers_moving(twk, dev, tp, layers, t, table, len(table))
        for given, want, label in ((gl, existing, "identity plane"), (None, existing, "previousPositions NULL"), (moved_geometry(gl, table), moving, "rigid-only plane")):
            _same(_merge_layers(twk, dev, tp, layers, t, given), want, f"{what}, {label}, {'trusted ' if t is not None else ''}cascade")
    dev.close()


def test_carried_refusals(twk):
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
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg, Lc, gl, Hl, hgl, seeded_plane(g, table)))
    out, trust, layers_out = _DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, width * height * 4), _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    m = p[10]
    current, history = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    name = "twk_temporal_accumulate_carried"
    merge = lambda rp=None, tp=None, c=current, h=history, t=m, s=shape, outs=(out.ptr.value, None, None, None): dev.temporalAccumulateCarried(tp, rp, c, h, t, s, *outs)
    merge()
    merge(L.TemporalRectify(), outs=(out.ptr.value, None, None, trust.ptr.value))
    refused(lambda: merge(c=None, h=None, s=None, outs=(None,) * 4), name, "explicit form")
    refused(lambda: merge(outs=(out.ptr.value, None, None, trust.ptr.value)), name, "trustOut")
    refused(lambda: merge(t=m + 4), name, "16-byte aligned")
    refused(lambda: merge(outs=(m, None, None, None)), name, "overlaps the previous positions")
    refused(lambda: merge(outs=(None, None, m + 128, None)), name, "overlaps the previous positions")
    refused(lambda: merge(L.TemporalRectify(), outs=(None, None, None, m + 64)), name, "overlaps the previous positions")
    refused(lambda: merge(tp=L.Temporal(maxHistory=0)), name, "maxHistory")
    refused(lambda: merge(L.TemporalRectify(radius=5)), name, "radius")
    refused(lambda: merge(outs=(p[3], None, None, None)), name, "overlaps an input")
    refused(lambda: merge(c=L.TemporalFrame(p[0], None, p[2])), name, "NULL")
    refused(lambda: merge(h=L.TemporalFrame(p[3], p[4], p[5], _camera(twk, np.zeros(12, F)))), name, "degenerate")
    refused(lambda: merge(s=(0, width)), name, "width and height")
    name = "twk_temporal_accumulate_cascade_carried"
    camera = _camera(twk, cam_l)
    cascade = lambda a=p[6], b=p[7], c=p[8], d=p[9], e=camera, t=None, pl=m, s=shape, o=layers_out.ptr.value: dev.temporalAccumulateCascadeCarried(None, None, a, b, c, d, e, t, pl, s, o)
    cascade()
    refused(lambda: cascade(pl=m + 8), name, "16-byte aligned")
    refused(lambda: cascade(o=m), name, "overlaps the previous positions")
    refused(lambda: cascade(a=None), name, "NULL")
    refused(lambda: cascade(o=p[8]), name, "overlaps an input")
    refused(lambda: cascade(t=layers_out.ptr.value + 16), name, "overlaps the trust")
    for buf in buffers + [out, trust, layers_out]:
        buf.free()
    dev.close()


# ---- quality: a sphere that swells between two frames ---------------------------------------------------------------------------------
WIDTH, HEIGHT, LOOP_SPP, REFERENCE_SPP = 96, 54, 4, 256
BALL = 2  # the sphere's instance: floor 0, light 1, sphere 2
TOLERANCE = 0.02  # x the distance to the camera (4.5) is 0.09; the swelling moves the surface by 0.3 x 0.5 = 0.15, more than that


def _sphere_scene(twk):
    """tests/test_gpu_temporal_motion.py's diffuse scene with a sphere (radius 0.5, its centre at (0, 0.5, 0)) in place of the box;
    returns the scene, the state and the sphere's geometry id."""
    s = Scene()
    s.miss = 0
    s.camera = twk.camera_frustum((0.0, 0.5, 0.0), 0.8, 0.62, 45.0, 4.5, WIDTH / HEIGHT)
    s.materials = [material(1, albedo=(0.0, 0.0, 0.0), thinwalled=1), material(0, albedo=(0.7, 0.7, 0.7)), material(0, albedo=(0.75, 0.4, 0.2))]
    light = parallelogram_light((-1.0, 3.5, -1.0), 2.0, (12.0, 12.0, 12.0))
    s.lights = [light]
    geometry = lambda mesh: (s.geometries.append((np.ascontiguousarray(mesh[0], np.float32), np.ascontiguousarray(mesh[1], np.uint32))), len(s.geometries) - 1)[1]
    s.instances.append((geometry(twk.mesh_plane(1, 1, 1)), transform(4.0), 1, -1))
    s.instances.append((geometry(twk.mesh_parallelogram(list(light.position), list(light.vecU), list(light.vecV), list(light.normal))), transform(), 0, 0))
    ball = geometry(twk.mesh_sphere(32, 16, 1.0, np.pi))
    s.instances.append((ball, transform(0.5, (0.0, 0.5, 0.0)), 2, -1))
    state = default_state(s, pathLengths=(2, 6))
    state.resolution[0], state.resolution[1] = WIDTH, HEIGHT
    return s, state, ball


def _relative_rmse(image, reference, mask):
    d = (image[..., :3].astype(np.float64) - reference[..., :3])[mask]
    return float(np.sqrt((d * d).mean()) / reference[..., :3][mask].mean())


def test_a_swollen_sphere_keeps_its_history(twk):
    """Two frames of 4 spp at 96 x 54, the sphere's vertices scaled by 1.3 about its centre between them with updateGeometryVertices:
    the surface moves by 0.15, more than positionTolerance x the camera distance (0.09), so the plain gather finds nothing there. A
    merge without renderGeometryMotion is refused; with it the own-buffer merge equals the restatement on the plane; of the sphere's
    pixels more than half take history, strictly more than the explicit plain merge takes on the same buffers (run on the device and
    equal to its restatement, whose count of pixels is used); and on those pixels the merged colour's relative RMSE against 256 spp from samples the frames do not share is below the
    4 spp frame's."""
    L = twk._lib
    tp = L.Temporal(maxHistory=32, positionTolerance=TOLERANCE)
    scene, state, ball = _sphere_scene(twk)
    dev = twk.Device(ordinal=0, miss=0)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    feed(dev, scene, state)

    def frame(offset, spp):
        dev.setSampleOffset(offset)
        for it in range(spp):
            dev.render(it)
        dev.renderGeometry()

    frame(0, LOOP_SPP)
    dev.temporalAccumulate(tp)
    history = (dev.readTemporal(), dev.readTemporalMoments(), dev.readGeometry())
    swollen = scene.geometries[ball][0].copy().reshape(-1, 12)
    swollen[:, 0:3] *= np.float32(1.3)  # (the mesh's centre is its origin)
    dev.updateGeometryVertices(ball, swollen)
    assert dev.geometryDeformed(ball)
    frame(LOOP_SPP, LOOP_SPP)
    with pytest.raises(twk.TwkError) as e:
        dev.temporalAccumulate(tp)
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_render_geometry_motion first" in str(e.value), str(e.value)
    with pytest.raises(twk.TwkError) as e:
        dev.temporalAccumulateRectified(tp, L.TemporalRectify())
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_render_geometry_motion first" in str(e.value), str(e.value)
    assert dev.geometryDeformed(ball), "a refused merge changes nothing"
    dev.renderGeometryMotion()
    alone, mc, g, plane = dev.getOutputBufferHost().copy(), dev.readMoments(), dev.readGeometry(), dev.readPreviousPositions()
    dev.temporalAccumulate(tp)
    merged = dev.readTemporal()
    assert len(dev.readTemporalMotion()) == 0 and not dev.geometryDeformed(ball)
    cam = camera_array(scene.camera)
    expect, _, took = restate_temporal_carried(alone, mc, g, history, cam, 32, TOLERANCE, plane)
    _same(merged, expect, "the own-buffer merge against the restatement")
    without, _, took_without = restate_temporal(alone, mc, g, history, cam, 32, TOLERANCE)
    # the explicit plain merge on the same buffers, on the device: it has the restatement's bits, so took_without is what it takes
    plain = _merge_moving(twk, dev, tp, None, (alone, mc, g) + history + (cam,), np.zeros(1, RECORD), 0, moving=False)
    _same(plain[1], without, "the explicit plain merge on the same buffers against its restatement")
    on_ball = g[..., 3].view(U32) == BALL + 1
    carried = on_ball & took
    print(f"\nsphere pixels {on_ball.sum()}, took history with the plane {carried.sum()}, without {(on_ball & took_without).sum()}")
    # pi (0.65 x 14.5 pixels per unit)^2 = 279 pixels of sphere, less what the picture's edge and the floor's horizon do not hide: none
    assert on_ball.sum() > 200 and carried.sum() > 0.5 * on_ball.sum() and carried.sum() > (on_ball & took_without).sum()
    frame(1000, REFERENCE_SPP)
    reference = dev.getOutputBufferHost().astype(np.float64)
    dev.close()
    e_alone, e_merged, e_without = (_relative_rmse(a, reference, carried) for a in (alone, merged, without))
    print(f"relative RMSE on the sphere's pixels that took history: 4 spp {e_alone:.4f}, merged with the plane {e_merged:.4f}, merged without {e_without:.4f}")
    assert e_merged < e_alone
