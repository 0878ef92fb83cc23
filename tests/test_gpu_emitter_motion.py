"""-m gpu: moving a light (twk_enable_emitter_motion; include/tweeker_hip.h "Moving a light", csrc/light_motion.h). With the switch on,
the five transform entries — twk_update_instance_transform[s], twk_refit_instance_transform[s] and twk_refit_scene's moved list —
accept the instance that carries the light and carry the light's definition along.

The scenes are tests/selective_scenes.py's that have walls (flat, two-level, mixed, many; `single` has no light): instance 0 is the
light, a direct leaf of the top level in flat, mixed and many, entered in two-level. Picture size and samples are
tests/test_gpu_selective_update.py's (33 x 21, 2 spp); both update modes, both build qualities, both output formats where pictures are
compared. After each entry:
  * fresh-handle equality: the handle equals a fresh handle built with the new transforms and twk_get_light's definition — the light
    table, the instance records and the pictures always; for the update calls and for the single refit of the light (a direct leaf is
    rebuilt, an entered instance gets its world box: the rebuild's path) also the acceleration structure, the scene arrays and the
    build info; for the refit calls that also refit a box's tree, tests/test_gpu_instance_refit.py's contract instead: the audit of
    the scene as it is now, and 4096 aimed rays against the fresh build (hit / miss and the bits of t on every ray, ids on all but 4);
  * oracle equality: the first 2 iterations equal the oracle fed that fresh scene, bit for bit;
  * the definition twk_get_light returns is tests/light_motion_restate.py's, bit for bit.
Then reversibility (A -> B -> A), re-anchoring by twk_update_light, the refusals with the switch off (today's texts) and on (the
three new ones, each leaving the handle as it was), the own-buffer temporal merge against the explicit moving form, and two tiled
handles against one."""
import ctypes as C

import numpy as np
import pytest

import bvh_audit as A
import lifecycle as lc
import light_motion_restate as R
import scene_snapshot as snapshot
import selective_scenes as S
import shading_fuzz as FZ
from conftest import load_app
from test_gpu_bvh_audit import _aimed_rays
from test_gpu_selective_update import CORNELL_WALLS, RES, SCENE, SPP, SYSTEM, _assert_same, _everything, _instances, _pictures, _step, _structure

pytestmark = pytest.mark.gpu

F, U32 = np.float32, np.uint32
QUALITIES = pytest.mark.parametrize("quality", [1, 0], ids=["sah", "lbvh"])
NAMES = [n for n in sorted(S.SCENES) if S.SCENES[n][2]]  # the scenes with walls: instance 0 carries the light
ENTRIES = ("update", "updates", "refit", "refits", "scene")
LIGHT = 0
RAYS, RAY_SEED, TIES = 4096, 5, 4  # tests/test_gpu_refit.py's


@pytest.fixture(scope="module")
def app(twk):
    a = load_app(twk, SYSTEM, SCENE, RES)
    yield a
    a.close()


@pytest.fixture(scope="module")
def parts(twk, app):
    walls = [app.instance(i) for i in CORNELL_WALLS]
    assert walls[0][3] >= 0 and all(w[3] < 0 for w in walls[1:]), "the first wall carries the light"
    geometries = [app.geometry(w[0]) for w in walls] + [twk.mesh_box(), twk.mesh_sphere(8, 4, 1.0, np.pi)]
    assert tuple(g[1].size // 3 for g in geometries) == S.TRIANGLES
    return geometries, [(w[1], w[2], w[3]) for w in walls]


def _light_id(parts):
    return parts[1][0][2]


def _moved_light(transform, k=0):
    """Another transform for the light's instance: its own, turned about y, scaled unequally and stepped; k = 2 mirrors it in x."""
    t = np.array(transform, np.float64).reshape(3, 4)
    c, s = np.cos(0.3 + 0.2 * k), np.sin(0.3 + 0.2 * k)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([-0.9 if k == 2 else 0.9, 1.0, 1.2])
    return np.concatenate([r @ t[:, :3], r @ t[:, 3:] + np.array([[0.05 + 0.03 * k], [-0.1], [0.05]])], 1).astype(F).reshape(12)


def _handle(twk, app, parts, name, quality, selective, transforms=None, lights=None, half=False, instances=None, emitters=True):
    """tests/test_gpu_selective_update.py's _device with the light table of the caller's choice and the switch."""
    L = twk._lib
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.enableAov(True)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    app.initDevice(dev)
    if lights is not None:
        dev.initLights(lights)
    if half:
        dev.setOutputFormat(lc.HALF4)
    dev.setBuildQuality(quality)
    dev.setFlattenPolicy(*S.policy(name))
    dev.setUpdateMode(L.TWK_UPDATE_SELECTIVE if selective else L.TWK_UPDATE_FULL)
    dev.clearScene()
    for attributes, indices in parts[0]:
        dev.addGeometry(attributes, indices)
    for i, (g, t, m, l) in enumerate(instances or _instances(name, parts)):
        dev.addInstance(g, (transforms or {}).get(i, t), m, l)
    dev.build()
    if emitters:
        assert not dev.emitterMotion(), "off by default"
        dev.enableEmitterMotion()
        assert dev.emitterMotion()
    return dev


def _light_table(dev, app):
    return np.frombuffer(b"".join(bytes(dev.getLight(k)) for k in range(app.info.numLights)), U32).copy()


def _moves(name, parts, entry, k=0):
    """{instance: new transform} of an entry: the light, and in the batch forms the first movable instance beside it."""
    base = _instances(name, parts)
    out = {LIGHT: _moved_light(base[LIGHT][1], k)}
    if entry in ("updates", "refits", "scene"):
        box = S.first_movable(name)
        out[box] = _step(base[box][1], (0.05, 0.1, 0.1))
    return out


def _apply(dev, entry, moves):
    ids = sorted(moves, reverse=True)  # the light last: the entry that carries it is not entry 0
    if entry == "update":
        dev.updateInstanceTransform(LIGHT, moves[LIGHT])
    elif entry == "refit":
        dev.refitInstanceTransform(LIGHT, moves[LIGHT])
    elif entry == "updates":
        dev.updateInstanceTransforms(ids, [moves[i] for i in ids])
    elif entry == "refits":
        dev.refitInstanceTransforms(ids, [moves[i] for i in ids])
    else:
        dev.refitScene(ids=ids, transforms=[moves[i] for i in ids])


def _fresh_lights(app, parts, definition):
    lights = app.lights
    lights[_light_id(parts)] = definition
    return lights


def _oracle_two(orc, app, parts, name, transforms, lights):
    ref = orc.Oracle(miss=app.info.miss)
    ref.loadApplication(app)
    ref.initLights(lights)
    ref.clearScene()
    ref.setFlattenPolicy(*S.policy(name))
    for attributes, indices in parts[0]:
        ref.addGeometry(attributes, indices)
    for i, (g, t, m, l) in enumerate(_instances(name, parts)):
        ref.addInstance(g, transforms.get(i, t), m, l)
    for it in range(SPP):
        ref.render(it)
    out = ref.getOutputBufferHost().copy()
    ref.close()
    return out


def _audit_scene(name, parts, transforms):
    geometries = list(parts[0])
    return geometries, [(g, transforms.get(n, t)) for n, (g, t, _, _) in enumerate(_instances(name, parts))]


@QUALITIES
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", NAMES)
def test_a_moved_light_equals_a_fresh_handle_and_the_oracle(twk, orc, app, parts, name, entry, quality):
    moves = _moves(name, parts, entry)
    base = _instances(name, parts)
    light = _light_id(parts)
    want_definition = R.light_moved(R.record(app.lights[light]), base[LIGHT][1], moves[LIGHT])
    exact = entry in ("update", "updates", "refit")  # the rebuild's path for every moved instance: the handle IS the fresh one
    modes = (True, False) if entry.startswith("update") else (True,)  # a refit needs a selective handle
    oracle = None
    for selective in modes:
        for half in (False, True):
            what = f"{name}, {entry}, {'selective' if selective else 'full'}, half {half}"
            dev = _handle(twk, app, parts, name, quality, selective, half=half)
            fresh = None
            try:
                before = _light_table(dev, app)
                _apply(dev, entry, moves)
                got_definition = dev.getLight(light)
                assert bytes(got_definition) == want_definition.tobytes(), what + ": twk_get_light against the restatement"
                assert bytes(got_definition) == bytes(twk.light_moved_host(app.lights[light], base[LIGHT][1], moves[LIGHT])), what
                assert not np.array_equal(_light_table(dev, app), before), what + ": the move shows in the light table"
                for i, t in moves.items():
                    assert np.array_equal(dev.instanceTransform(i), t), what
                fresh = _handle(twk, app, parts, name, quality, False, moves, _fresh_lights(app, parts, got_definition), half=half, emitters=False)
                assert np.array_equal(_light_table(dev, app), _light_table(fresh, app)), what + ": the light table"
                if exact and not half:
                    got, want = _everything(twk, orc, dev), _everything(twk, orc, fresh)
                    _assert_same(got[0], want[0], what + ": against a fresh handle")
                    pictures = got[0]
                else:
                    pictures = _pictures(dev, half)
                    _assert_same(pictures, _pictures(fresh, half), what + ": the pictures against a fresh handle's")
                    assert np.array_equal(dev.readAcceleration()[3].view(U32), fresh.readAcceleration()[3].view(U32)), what + ": the instance records"
                if not exact and not half:
                    geometries, instances = _audit_scene(name, parts, moves)
                    A.audit(A.Scene(geometries, instances, S.policy(name), quality), snapshot.readback(twk, orc, dev))
                    rays = _aimed_rays(geometries, instances, RAYS, RAY_SEED)
                    (t_got, id_got), (t_want, id_want) = dev.traceRays(rays), fresh.traceRays(rays)
                    hit = id_want[:, 0] >= 0
                    assert 0.3 < hit.mean() < 1.0, hit.mean()
                    assert np.array_equal(id_got[:, 0] >= 0, hit), what + ": hit / miss"
                    assert np.array_equal(t_got[hit, 0].view(U32), t_want[hit, 0].view(U32)), what + ": the bits of t"
                    assert int((id_got != id_want).any(1).sum()) <= TIES, what + ": the ids"
                if not half:
                    if oracle is None:
                        oracle = _oracle_two(orc, app, parts, name, moves, _fresh_lights(app, parts, got_definition))
                        assert np.isfinite(oracle).all() and oracle[..., :3].max() > 0.0
                    bad = FZ.mismatch(dev.getOutputBufferHost(), oracle)
                    assert bad is None, f"{what}: the first {SPP} iterations against the oracle: {bad}"
            finally:
                dev.close()
                if fresh is not None:
                    fresh.close()


@QUALITIES
@pytest.mark.parametrize("name", NAMES)
def test_there_and_back_leaves_the_light_and_the_pictures_of_a(twk, orc, app, parts, name, quality):
    """A -> B -> A through the update and through the refit call, and A -> B -> C (a mirror) -> A: the light table and the pictures of
    A byte for byte — every moved definition is derived from the anchor, and the anchor's transform gives back the anchor's bytes."""
    a = _instances(name, parts)[LIGHT][1]
    for half in (False, True):
        dev = _handle(twk, app, parts, name, quality, True, half=half)
        try:
            table, pictures = _light_table(dev, app), _pictures(dev, half)
            for calls in ((dev.updateInstanceTransform,), (dev.refitInstanceTransform,), (dev.updateInstanceTransform, dev.refitInstanceTransform)):
                for k, call in enumerate(calls):
                    call(LIGHT, _moved_light(a, 2 * k))
                    assert not np.array_equal(_light_table(dev, app), table)
                calls[-1](LIGHT, a)
                assert np.array_equal(_light_table(dev, app), table), f"{name}: the light table after the way back"
                _assert_same(_pictures(dev, half), pictures, f"{name}, half {half}: the pictures after the way back")
        finally:
            dev.close()


@QUALITIES
def test_an_updated_light_anchors_anew(twk, app, parts, quality):
    """B, then twk_update_light with another emission and another shape, then C: the definition is light_moved_host(the updated
    definition, the transform at the update (B), C) — not derived from the first anchor. Then twk_build, which drops the anchor too."""
    name = "flat"
    light = _light_id(parts)
    a = _instances(name, parts)[LIGHT][1]
    b, c = _moved_light(a, 0), _moved_light(a, 2)
    dev = _handle(twk, app, parts, name, quality, True)
    try:
        dev.updateInstanceTransform(LIGHT, b)
        updated = R.record(dev.getLight(light))
        updated["emission"] = (3.0, 5.0, 7.0)
        updated["vecU"] = updated["vecU"] * F(0.5)
        _, updated["area"], updated["normal"] = R.cross_area_normal(updated["vecU"], updated["vecV"])
        dev.updateLight(light, R.definition(twk, updated))
        assert bytes(dev.getLight(light)) == updated.tobytes()
        dev.refitInstanceTransform(LIGHT, c)
        want = R.light_moved(updated, b, c)
        assert bytes(dev.getLight(light)) == want.tobytes() == bytes(twk.light_moved_host(R.definition(twk, updated), b, c))
        assert bytes(dev.getLight(light)) != R.light_moved(R.record(app.lights[light]), a, c).tobytes(), "not from the first anchor"
        dev.updateInstanceTransform(LIGHT, b)  # back at the anchor's transform: the updated definition's bytes
        assert bytes(dev.getLight(light)) == updated.tobytes()
        dev.updateInstanceTransform(LIGHT, c)
        dev.build()  # the anchor goes: the next move anchors on what the light is now, under c
        now = R.record(dev.getLight(light))
        dev.updateInstanceTransform(LIGHT, a)
        assert bytes(dev.getLight(light)) == R.light_moved(now, c, a).tobytes()
    finally:
        dev.close()


TODAY = "the instance carries a light (idLight >= 0): its light definition holds the emitter's position and would disagree; moving emitters is not supported"


def _refused(twk, f, call, *words):
    with pytest.raises(twk.TwkError) as e:
        f()
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_VALUE and call + ":" in str(e.value), str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def _calls(dev, ids, transforms):
    """The five entries on `ids` (the single ones on the last of them), as (name, call)."""
    return (("twk_update_instance_transform", lambda: dev.updateInstanceTransform(ids[-1], transforms[-1])),
            ("twk_update_instance_transforms", lambda: dev.updateInstanceTransforms(ids, transforms)),
            ("twk_refit_instance_transform", lambda: dev.refitInstanceTransform(ids[-1], transforms[-1])),
            ("twk_refit_instance_transforms", lambda: dev.refitInstanceTransforms(ids, transforms)),
            ("twk_refit_scene", lambda: dev.refitScene(ids=ids, transforms=transforms)))


def _state(twk, orc, dev, app):
    out = _everything(twk, orc, dev)[0]
    out["lights"] = _light_table(dev, app)  # (the transforms are in the instance records)
    return out


@QUALITIES
def test_with_the_switch_off_every_entry_refuses_as_it_always_did(twk, orc, app, parts, quality):
    name = "flat"
    base = _instances(name, parts)
    box = S.first_movable(name)
    ids, transforms = [box, LIGHT], [_step(base[box][1]), _moved_light(base[LIGHT][1])]
    dev = _handle(twk, app, parts, name, quality, True, emitters=False)
    try:
        before = _state(twk, orc, dev, app)
        for on in (None, 0):  # never switched on, and switched on and off again
            if on is not None:
                dev.enableEmitterMotion(True)
                dev.enableEmitterMotion(False)
            assert not dev.emitterMotion()
            for call, f in _calls(dev, ids, transforms):
                _refused(twk, f, call, TODAY, *(("entry 1: ",) if call.endswith("s") or call == "twk_refit_scene" else ()))
        _assert_same(_state(twk, orc, dev, app), before, "after the refusals")
        L = twk._lib
        assert L.lib.twk_enable_emitter_motion(None, 1) == L.TWK_ERROR_INVALID_VALUE and "twk_enable_emitter_motion" in L.lib.twk_last_error().decode()
        assert L.lib.twk_enable_emitter_motion(dev.handle, 2) == L.TWK_ERROR_INVALID_VALUE and "neither 0 nor 1" in L.lib.twk_last_error().decode()
        assert L.lib.twk_get_emitter_motion(dev.handle, None) == L.TWK_ERROR_INVALID_VALUE
        assert L.lib.twk_get_light(dev.handle, app.info.numLights, C.byref(twk.LightDefinition())) == L.TWK_ERROR_INVALID_VALUE and "bad light id" in L.lib.twk_last_error().decode()
        assert L.lib.twk_get_light(dev.handle, 0, None) == L.TWK_ERROR_INVALID_VALUE
    finally:
        dev.close()


@QUALITIES
def test_the_new_refusals_change_nothing(twk, orc, app, parts, quality):
    """With the switch on: a light that is no parallelogram (an instance that carries a light of the environment's type), a light two instances
    carry (the text names both), a move that makes the light degenerate (scaled by 1e-30: the determinant is fine in double, the
    area underflows to zero in float). Each through all five entries, after a valid entry 0, and the handle is as it was."""
    name = "flat"
    light = _light_id(parts)
    lights = app.lights + [FZ.environment_light()]  # one more light, of the environment's type: no parallelogram
    other = len(lights) - 1
    assert all(l.type == 1 for l in lights[:-1]) and lights[other].type == 0
    base = _instances(name, parts)
    box = S.first_movable(name)
    wall = 1
    good_light, good_box = _moved_light(base[LIGHT][1]), _step(base[box][1])
    tiny = (np.array(base[LIGHT][1], F) * F(1e-30)).astype(F)
    cases = []
    env = list(base)
    env[wall] = env[wall][:3] + (other,)    # the floor carries that light
    cases.append(("environment", env, wall, _step(base[wall][1], (0.0, 0.05, 0.0)), ("not a TWK_LIGHT_PARALLELOGRAM", f"instance {wall} carries light {other}")))
    twice = list(base)
    twice[wall] = twice[wall][:3] + (light,)  # the floor carries the area light too
    cases.append(("two instances", twice, LIGHT, good_light, ("more than one instance", f"instances {LIGHT} and {wall}")))
    cases.append(("two instances, the other one", twice, wall, _step(base[wall][1], (0.0, 0.05, 0.0)), ("more than one instance", f"instances {LIGHT} and {wall}")))
    cases.append(("degenerate", base, LIGHT, tiny, ("degenerate", "area is zero or not finite")))
    for what, instances, target, transform, words in cases:
        dev = _handle(twk, app, parts, name, quality, True, lights=lights, instances=instances)

        def scene():
            """What twk_debug_snapshot_scene and the read-backs hand out (nothing is rendered), and the light table."""
            out = _structure(twk, orc, dev)[0]
            out["lights"] = np.frombuffer(b"".join(bytes(dev.getLight(k)) for k in range(len(lights))), U32).copy()
            return out

        try:
            before = scene()
            for call, f in _calls(dev, [box, target], [good_box, transform]):
                _refused(twk, f, call, *words, *(("entry 1: ",) if call.endswith("s") or call == "twk_refit_scene" else ()))
            _assert_same(scene(), before, what + ": after the refusals")
            for reader in (dev.updateInfo, dev.refitInfo):
                with pytest.raises(twk.TwkError):
                    reader()
            # the checks the calls always had still come first, and in entry order: a bad id behind the emitter is refused as before
            _refused(twk, lambda: dev.updateInstanceTransforms([target, 99], [transform, good_box]), "twk_update_instance_transforms", "entry 1: bad instance id")
        finally:
            dev.close()


def test_the_own_buffer_merge_follows_the_moved_light(twk, app, parts):
    """A frame merged, the light moved, a second frame merged: the own-buffer twk_temporal_accumulate uses the table twk_instance_motion
    gives for (the light's transform at the history's frame, its transform now) — the light's record alone says moved — and equals the
    explicit twk_temporal_accumulate_moving on the buffers read back, byte for byte."""
    from test_gpu_denoise_variance import _upload
    from test_gpu_half_output import _DeviceBuffer
    from test_gpu_temporal import _frame, _same
    L = twk._lib
    name = "flat"
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    a = _instances(name, parts)[LIGHT][1]
    b = _step(a, (0.15, -0.2, 0.1))
    count = len(_instances(name, parts))
    dev = _handle(twk, app, parts, name, 1, True)
    try:
        camera = app.cameras[0]
        dev.updateCamera(0, camera)
        _frame(dev, 0, SPP)
        first = (dev.getOutputBufferHost(), dev.readMoments(), dev.readGeometry())
        dev.temporalAccumulate(tp)
        assert len(dev.readTemporalMotion()) == 0
        dev.refitInstanceTransform(LIGHT, b)
        _frame(dev, SPP, SPP)
        colour, mc, g = dev.getOutputBufferHost(), dev.readMoments(), dev.readGeometry()
        dev.temporalAccumulate(tp)
        table = dev.readTemporalMotion()
        assert [r.moved for r in table] == [int(i == LIGHT) for i in range(count)]
        assert bytes(table[LIGHT]) == bytes(twk.instance_motion(a, b))
        records = np.frombuffer(b"".join(bytes(twk.instance_motion(t, dev.instanceTransform(i))) for i, (_, t, _, _) in enumerate(_instances(name, parts))), np.uint8)
        assert records.tobytes() == bytes(table)
        emitter = g[..., 3].view(U32) == LIGHT + 1
        took = dev.readTemporalMoments()[..., 2] > mc[..., 2]
        assert emitter.sum() >= 4 and (took & emitter).any(), (emitter.sum(), (took & emitter).sum())
        height, width = mc.shape[:2]
        buffers = _upload(twk, (colour, mc, g) + first + (records,))
        p = [x.ptr.value for x in buffers]
        outs = [_DeviceBuffer(twk, colour.nbytes), _DeviceBuffer(twk, mc.nbytes), _DeviceBuffer(twk, mc.nbytes)]
        o = [x.ptr.value for x in outs]
        dev.temporalAccumulateMoving(tp, None, L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], camera), p[6], count, (height, width), o[0], o[1], o[2])
        dev.synchronizeStream()
        _same(outs[0].download(colour.shape, colour.dtype), dev.readTemporal(), "the explicit form's colourOut against the own-buffer form")
        _same(outs[2].download(mc.shape, F), dev.readTemporalMoments(), "the explicit form's momentsOut against the own-buffer form")
        for x in buffers + outs:
            x.free()
    finally:
        dev.close()


def test_two_tiled_handles_moved_by_the_caller_assemble_to_one(twk):
    """tests/test_gpu_temporal_motion_tiles.py's loop with the LIGHT stepped instead of the sphere, on every handle by the caller: after
    every frame the primary's merged planes equal one handle's, byte for byte."""
    from test_gpu_temporal_tiles import FRAMES, HEIGHT, MERGED, TILE, WIDTH, _assert_same as same, _camera, _close, _device, _merged, _render, _tiled, _tp
    from test_gpu_temporal_tiles import SPP as TILE_SPP
    step = np.array((0.1, -0.05, 0.05), F)

    def move(devs, frame):
        if frame == 0:
            for d in devs:
                d.enableEmitterMotion()
            return
        for d in devs:
            t = d.instanceTransform(LIGHT)
            t[[3, 7, 11]] += step
            d.updateInstanceTransform(LIGHT, t)

    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    one_app = lc.make_app(twk, load_app, shape)
    one = _device(twk, one_app, shape)
    one.enableTemporalCascade(True)
    single, lights = [], []
    for f in range(FRAMES):
        move([one], f)
        one.updateCamera(0, _camera(twk, one_app, f))
        one.setSampleOffset(f * TILE_SPP)
        for it in range(TILE_SPP):
            one.render(it)
        one.renderGeometry()
        one.temporalAccumulate(_tp(twk))
        single.append(_merged(one))
        lights.append(bytes(one.getLight(one_app.info.numLights - 1)))
        assert [r.moved for r in one.readTemporalMotion()] == ([] if f == 0 else [int(i == LIGHT) for i in range(one_app.info.numInstances)])
    assert len(set(lights)) == FRAMES, "the light's definition moved with every frame"
    one.close()
    one_app.close()
    tile_app, devs = _tiled(twk, 2, False)
    primary = devs[0]
    for f in range(FRAMES):
        move(devs, f)
        _render(devs, _camera(twk, tile_app, f), f)
        primary.assembleWithGeometry(devs, MERGED)
        primary.temporalAccumulateAssembled(_tp(twk))
        same(_merged(primary), single[f], f"2 handles, frame {f}")
        assert all(bytes(d.getLight(tile_app.info.numLights - 1)) == lights[f] for d in devs)
    _close(tile_app, devs)
