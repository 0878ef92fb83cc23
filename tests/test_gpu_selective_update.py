"""-m gpu: selective instance updates (twk_set_update_mode, twk_update_instance_transforms, twk_get_update_info). A handle built in
selective mode rebuilds only what a moved instance changes, and must then EQUAL a fresh handle that was given the final transforms
through twk_clear_scene ... twk_build: the acceleration read-back (info, quantised nodes, slots, instance records), the scene arrays of
twk_debug_snapshot_scene (binary nodes, shading records, the two top-of-tree caches), twk_get_build_info except its time, and every
buffer a render leaves — byte for byte, no tolerance: the same kernels run on the same inputs at the same bases.

The scenes are tests/selective_scenes.py's (flat, two-level, mixed, single, many), at 33 x 21 and 2 spp, in SAH and LBVH quality; cameras,
lights and materials are the Cornell box's."""

import numpy as np
import pytest

import lifecycle as lc
import scene_snapshot as snapshot
import selective_scenes as S
from conftest import load_app

pytestmark = pytest.mark.gpu

RES, SPP = (33, 21), 2
SYSTEM, SCENE = "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt"
CORNELL_WALLS = (0, 1, 3, 4)  # the Cornell box's light, floor, back wall and left wall: instance ids there
QUALITIES = pytest.mark.parametrize("quality", [1, 0], ids=["sah", "lbvh"])
F = np.float32


# scenes with two movable objects and a wall: what a sequence and a batch need. `single` has one instance and cannot take part.
SEVERAL = ["flat", "two-level", "mixed", "many"]


@pytest.fixture(scope="module")
def app(twk):
    a = load_app(twk, SYSTEM, SCENE, RES)
    yield a
    a.close()


@pytest.fixture(scope="module")
def parts(twk, app):
    """The six geometries of selective_scenes.py and the walls' instances (transform, material, light)."""
    walls = [app.instance(i) for i in CORNELL_WALLS]
    assert walls[0][3] >= 0 and all(w[3] < 0 for w in walls[1:]), "the first wall carries the light"
    geometries = [app.geometry(w[0]) for w in walls] + [twk.mesh_box(), twk.mesh_sphere(8, 4, 1.0, np.pi)]
    assert tuple(g[1].size // 3 for g in geometries) == S.TRIANGLES
    return geometries, [(w[1], w[2], w[3]) for w in walls]


def _instances(name, parts):
    """[(geometry, transform, material, light)] of a scene."""
    _, rest, with_walls = S.SCENES[name]
    out = [(g, t, m, l) for g, (t, m, l) in zip(S.WALLS, parts[1])] if with_walls else []
    return out + [(g, t, m, -1) for g, t, m in rest]


def _device(twk, app, parts, name, quality, selective, transforms=None, half=False, instances=None, policy=None):
    """A handle on scene `name` (or on `instances` under `policy`). transforms: {instance: transform} replace the scene's own — the
    fresh handle of a comparison."""
    L = twk._lib
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.enableAov(True)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    app.initDevice(dev)  # state, cameras, lights, materials (and the Cornell box itself, which is cleared again)
    if half:
        dev.setOutputFormat(lc.HALF4)
    dev.setBuildQuality(quality)
    dev.setFlattenPolicy(*(policy or S.policy(name)))
    dev.setUpdateMode(L.TWK_UPDATE_SELECTIVE if selective else L.TWK_UPDATE_FULL)
    dev.clearScene()
    for attributes, indices in parts[0]:
        dev.addGeometry(attributes, indices)
    for i, (g, t, m, l) in enumerate(instances or _instances(name, parts)):
        dev.addInstance(g, (transforms or {}).get(i, t), m, l)
    dev.build()
    return dev


def _structure(twk, orc, dev):
    """Everything the build leaves that a reader can get at, as words (scene_snapshot.py reads it)."""
    arrays, info, build = snapshot.read_scene(twk, orc, dev)
    out = {key: (value if key == "topRoots" else lc._words(value)) for key, value in arrays.items()}
    out["info"] = np.array([info[k] for k in sorted(info)], np.int64)
    out["buildInfo"] = np.array([build[k] for k in sorted(build) if k != "buildMilliseconds"], np.float64).view(np.uint64)
    return out, info, build


def _pictures(dev, half=False):
    """2 spp from iteration 0 and the geometry AOV: colour, both AOVs, moments, geometry, as words."""
    dev.setSampleOffset(0)
    for it in range(SPP):
        dev.render(it)
    dev.renderGeometry()
    return {"colour": lc._words(dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()), "albedo": lc._words(dev.readAov(0, raw=True)),
            "normal": lc._words(dev.readAov(1, raw=True)), "moments": lc._words(dev.readMoments()), "geometry": lc._words(dev.readGeometry())}


def _everything(twk, orc, dev, half=False):
    out, info, build = _structure(twk, orc, dev)
    out.update(_pictures(dev, half))
    return out, info, build


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want)
    for key in want:
        diff = lc.first_difference(got[key], want[key])
        assert diff is None, f"{what}, {key}: {diff}"


def _step(transform, step=(0.1, 0.15, 0.2)):
    t = np.array(transform, F).reshape(12).copy()
    t[[3, 7, 11]] += np.array(step, F)
    return t


def _cases(name, parts):
    """{case: (instance, new transform)}: what the scene has of a flattened tree instance, a direct-leaf wall, an entered instance, and
    a move with rotation and non-uniform scale."""
    instances = _instances(name, parts)
    plan_flat = {"flat": 5, "mixed": 7, "single": 0, "many": 7}
    entered = {"two-level": 5, "mixed": 4}
    wall = {"flat": 1, "mixed": 3, "many": 2, "two-level": 2}  # a wall without the light: a direct leaf where it is flattened
    first = S.first_movable(name)
    out = {}
    if name in plan_flat:
        out["flattened-tree"] = (plan_flat[name], _step(instances[plan_flat[name]][1]))
    if name in wall:
        out["wall"] = (wall[name], _step(instances[wall[name]][1], (0.0, 0.05, -0.05) if wall[name] != 1 else (0.0, -0.1, 0.0)))
    if name in entered:
        out["entered"] = (entered[name], _step(instances[entered[name]][1]))
    at = instances[first][1][[3, 7, 11]] + np.array([0.05, 0.1, 0.1], F)
    out["rotated-scaled"] = (first, S.rotated(at))
    return out


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_one_selective_update_equals_a_fresh_build(twk, orc, app, parts, name, quality):
    """Per case of the scene: the updated handle against a fresh one, structure and pictures; updateInfo against the plan. Once per
    scene (the first case) also in RGBA16F."""
    L = twk._lib
    geometry = S.instance_geometry(name)
    dev = _device(twk, app, parts, name, quality, True)
    original = [t for _, t, _, _ in _instances(name, parts)]
    before, info, build = _everything(twk, orc, dev)
    layout = twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name))
    assert (build["nodes"], build["triangleSlots"], build["flattenedInstances"], build["directLeafInstances"]) == \
        (layout["nodes"], layout["triangleSlots"], layout["flattenedInstances"], layout["directLeafInstances"]), "the plan lays the scene out as the build does"
    assert info["twoLevel"] == int(layout["flattenedInstances"] < layout["instances"])
    if name == "many" and quality == 1:
        # the binned-SAH top level over the twelve boxes and four walls takes the 8-wide root; the Morton tree over the same boxes does
        # not (measured), so the LBVH case runs the selective path without it and the Cornell box below covers LBVH
        assert info["root2"] != -1, "the twelve boxes reach the 8-wide root"
    with pytest.raises(twk.TwkError) as e:
        dev.updateInfo()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE
    for k, (case, (instance, moved)) in enumerate(_cases(name, parts).items()):
        what = f"{name}, {case} (instance {instance})"
        dev.updateInstanceTransform(instance, moved)
        assert np.array_equal(dev.instanceTransform(instance), moved)
        plan = twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name), [instance])
        u = dev.updateInfo()
        assert u["selective"] == 1 and u["instancesMoved"] == 1 and u["instanceRecordsUploaded"] == 1, what
        assert (u["treesRebuilt"], u["topLevelRebuilt"], u["nodesRequantised"], u["slotsRewritten"]) == \
            (plan["treesRebuilt"], plan["topLevelRebuilt"], plan["nodesRequantised"], plan["slotsRewritten"]), what
        if case == "entered":
            assert u["treesRebuilt"] == 0 and u["topLevelRebuilt"] == 1, what
        if case in ("flattened-tree", "wall") and plan["flattened"][instance]:
            assert u["treesRebuilt"] == 1, what
        assert u["keptBytes"] >= 128 * (build["nodes"] + 2) and u["milliseconds"] > 0.0, what
        assert dev.buildInfo()["buildMilliseconds"] == u["milliseconds"], what
        got, _, _ = _everything(twk, orc, dev)
        fresh = _device(twk, app, parts, name, quality, False, {instance: moved})
        want, _, _ = _everything(twk, orc, fresh)
        fresh.close()
        assert lc.first_difference(want["geometry"], before["geometry"]) is not None, what + ": the move shows"
        _assert_same(got, want, what + ": against a fresh handle")
        if k == 0:
            half_dev = _device(twk, app, parts, name, quality, True, half=True)
            half_dev.updateInstanceTransform(instance, moved)
            half_fresh = _device(twk, app, parts, name, quality, False, {instance: moved}, half=True)
            _assert_same(_pictures(half_dev, True), _pictures(half_fresh, True), what + ": RGBA16F")
            half_dev.close()
            half_fresh.close()
        dev.updateInstanceTransform(instance, original[instance])
        _assert_same(_everything(twk, orc, dev)[0], before, what + ": after the update back")
    dev.close()


@QUALITIES
def test_the_eight_wide_root_of_the_cornell_box_follows_an_update(twk, orc, quality):
    """The Cornell box at 61 x 37, whose build takes the 8-wide root in both qualities: the mirror sphere (instance 6, flattened, 32 040
    triangles) moved selectively, against a fresh handle, and moved back, against the original build; the two root slots are part of
    the read-back. With the sphere at its new place the SAH build keeps the root and the LBVH build does NOT take it: the update makes
    it disappear, and the update back makes it appear again."""
    L = twk._lib
    app = load_app(twk, SYSTEM, SCENE, (61, 37))
    original = app.instance(6)[1]
    moved = _step(original, (0.0, 0.6, 0.5))
    devices = []
    for selective in (True, False):
        dev = twk.Device(ordinal=0, miss=app.info.miss)
        dev.enableAov(True)
        dev.enableMoments(True)
        dev.enableGeometry(True)
        dev.setBuildQuality(quality)
        dev.setUpdateMode(L.TWK_UPDATE_SELECTIVE if selective else L.TWK_UPDATE_FULL)
        app.initDevice(dev)
        if not selective:  # the fresh handle: the scene again with the new transform
            dev.clearScene()
            for k in range(app.info.numGeometries):
                dev.addGeometry(*app.geometry(k))
            for i, (g, t, m, l) in enumerate(app.instances):
                dev.addInstance(g, moved if i == 6 else t, m, l)
            dev.build()
        devices.append(dev)
    updated, fresh = devices
    before, info, _ = _everything(twk, orc, updated)
    assert info["root2"] != -1, "the Cornell box's build takes the 8-wide root"
    updated.updateInstanceTransform(6, moved)
    u = updated.updateInfo()
    assert u["selective"] == 1 and u["treesRebuilt"] == 1 and u["slotsRewritten"] == 32040, u
    got, info, _ = _everything(twk, orc, updated)
    if quality == 1:
        assert info["root2"] != -1, "SAH: the root stays 8-wide with the sphere moved"
    else:
        assert info["root2"] == -1, "LBVH: with the sphere moved the 8-wide root does not pay, and the update takes it away"
    _assert_same(got, _everything(twk, orc, fresh)[0], "the Cornell box after a selective update against a fresh handle")
    updated.updateInstanceTransform(6, original)
    got, info, _ = _everything(twk, orc, updated)
    assert info["root2"] != -1, "back at its place: the 8-wide root again"
    _assert_same(got, before, "the Cornell box after the update back against its original build")
    for dev in devices:
        dev.close()
    app.close()


@QUALITIES
def test_more_ranges_than_the_tail_keeps_in_lds(twk, orc, app, parts, quality):
    """The light wall and 1100 flattened boxes, every box moved in ONE batch: 1102 node ranges, so the ranged tail searches its table
    in global memory (above 1024 ranges). The handle equals a fresh one."""
    boxes = S.thousand_boxes()
    instances = [(S.LIGHT,) + parts[1][0]] + [(g, t, m, -1) for g, t, m in boxes]
    geometry = [g for g, _, _, _ in instances]
    ids = list(range(1, len(instances)))
    plan = twk.update_plan_host(geometry, S.TRIANGLES, S.THOUSAND_POLICY, ids)
    assert plan["numRanges"] == S.THOUSAND + 2 > 1024 and plan["treesRebuilt"] == S.THOUSAND
    moved = {i: _step(instances[i][1], (0.01, 0.02 + 0.0001 * i, 0.03)) for i in ids}
    dev = _device(twk, app, parts, None, quality, True, instances=instances, policy=S.THOUSAND_POLICY)
    dev.updateInstanceTransforms(ids, [moved[i] for i in ids])
    u = dev.updateInfo()
    assert u["selective"] == 1 and u["instancesMoved"] == S.THOUSAND and u["treesRebuilt"] == S.THOUSAND and u["nodesRequantised"] == plan["nodesRequantised"]
    fresh = _device(twk, app, parts, None, quality, False, moved, instances=instances, policy=S.THOUSAND_POLICY)
    _assert_same(_everything(twk, orc, dev)[0], _everything(twk, orc, fresh)[0], "1100 boxes moved in one batch against a fresh handle")
    fresh.close()
    dev.close()


@QUALITIES
@pytest.mark.parametrize("name", SEVERAL)
def test_a_sequence_of_updates_and_the_way_back(twk, orc, app, parts, name, quality):
    """Three updates of different instances, then a batch of two, then everything back: equal to a fresh handle with the final
    transforms after the batch, and to the original build after the way back. (`single` has one instance: no sequence.)"""
    instances = _instances(name, parts)
    first = S.first_movable(name)
    a, b, c = first, first + 1, 1  # two objects and a wall
    dev = _device(twk, app, parts, name, quality, True)
    before = _everything(twk, orc, dev)[0]
    now = {}
    for i, step in ((a, (0.1, 0.2, 0.1)), (c, (0.0, -0.05, 0.0)), (b, (-0.1, 0.1, 0.2))):
        now[i] = _step(instances[i][1], step)
        dev.updateInstanceTransform(i, now[i])
    now[a], now[b] = S.rotated(now[a][[3, 7, 11]], 0.3, (0.2, 0.3, 0.25)), _step(now[b], (0.05, 0.0, 0.0))
    dev.updateInstanceTransforms([b, a], [now[b], now[a]])
    u = dev.updateInfo()
    plan = twk.update_plan_host(S.instance_geometry(name), S.TRIANGLES, S.policy(name), [b, a])
    assert u["selective"] == 1 and u["instancesMoved"] == 2 and u["treesRebuilt"] == plan["treesRebuilt"] and u["nodesRequantised"] == plan["nodesRequantised"]
    fresh = _device(twk, app, parts, name, quality, False, now)
    _assert_same(_everything(twk, orc, dev)[0], _everything(twk, orc, fresh)[0], f"{name}: after three updates and a batch")
    fresh.close()
    dev.updateInstanceTransforms([a, b, c], [instances[i][1] for i in (a, b, c)])
    _assert_same(_everything(twk, orc, dev)[0], before, f"{name}: all back")
    dev.close()


@QUALITIES
@pytest.mark.parametrize("selective", [True, False], ids=["selective", "full"])
@pytest.mark.parametrize("name", SEVERAL)
def test_a_batch_leaves_what_singles_leave(twk, orc, app, parts, name, selective, quality):
    """(`single` has one instance: a batch of one IS the single call, which the one-update test runs.)"""
    instances = _instances(name, parts)
    first = S.first_movable(name)
    moves = {first: _step(instances[first][1]), first + 1: S.rotated(instances[first + 1][1][[3, 7, 11]]), 2: _step(instances[2][1], (0.0, 0.0, -0.1))}
    batch, singles = _device(twk, app, parts, name, quality, selective), _device(twk, app, parts, name, quality, selective)
    batch.updateInstanceTransforms(list(moves), list(moves.values()))
    for i, t in moves.items():
        singles.updateInstanceTransform(i, t)
    assert batch.updateInfo()["selective"] == singles.updateInfo()["selective"] == int(selective)
    assert batch.updateInfo()["instancesMoved"] == 3 and singles.updateInfo()["instancesMoved"] == 1
    if not selective:
        assert batch.updateInfo()["keptBytes"] == 0
    want = _everything(twk, orc, singles)[0]
    _assert_same(_everything(twk, orc, batch)[0], want, f"{name}: one batch of three against three singles")
    if not selective:  # full mode with the batch call equals a fresh handle
        fresh = _device(twk, app, parts, name, quality, False, moves)
        _assert_same(want, _everything(twk, orc, fresh)[0], f"{name}: full mode against a fresh handle")
        fresh.close()
    batch.close()
    singles.close()


def _movable(name):
    """The instance the per-scene tests below move: the scene's flattened tree instance where it has one, else an entered sphere."""
    return {"flat": 5, "mixed": 7, "single": 0, "many": 7, "two-level": 5}[name]


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_the_mode_takes_effect_at_the_next_build(twk, orc, app, parts, name, quality):
    L = twk._lib
    m = _movable(name)
    geometry = S.instance_geometry(name)
    dev = _device(twk, app, parts, name, quality, False)
    dev.setUpdateMode(L.TWK_UPDATE_SELECTIVE)
    moved = _step(_instances(name, parts)[m][1])
    dev.updateInstanceTransform(m, moved)
    u = dev.updateInfo()
    assert u["selective"] == 0 and u["keptBytes"] == 0 and u["topLevelRebuilt"] == int(name != "single") and u["treesRebuilt"] == dev.buildInfo()["trees"], u
    dev.build()
    dev.updateInstanceTransform(m, _step(moved))
    u = dev.updateInfo()
    plan = twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name), [m])
    assert u["selective"] == 1 and u["keptBytes"] > 0 and u["treesRebuilt"] == plan["treesRebuilt"], u
    fresh = _device(twk, app, parts, name, quality, False, {m: _step(moved)})
    _assert_same(_everything(twk, orc, dev)[0], _everything(twk, orc, fresh)[0], f"{name}: built full, switched, built again, updated")
    fresh.close()
    dev.setUpdateMode(L.TWK_UPDATE_FULL)  # ... and back: the kept build goes with the next build
    dev.build()
    dev.updateInstanceTransform(m, moved)
    assert dev.updateInfo()["selective"] == 0 and dev.updateInfo()["keptBytes"] == 0
    dev.close()


@QUALITIES
def test_the_temporal_history_survives_a_selective_update(twk, app, parts, quality):
    """One frame of the flat scene merged (the scene the issue names for this), the sphere moved, a second frame merged: the own-buffer
    merge's colour and moments and the motion table equal those of a twin handle in full mode, byte for byte."""
    L = twk._lib
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    moved = _step(_instances("flat", parts)[5][1], (0.1, 0.1, 0.05))
    results = []
    for selective in (True, False):
        dev = _device(twk, app, parts, "flat", quality, selective)
        for frame in range(2):
            if frame:
                dev.updateInstanceTransform(5, moved)
                assert dev.updateInfo()["selective"] == int(selective)
            dev.setSampleOffset(frame * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.temporalAccumulate(tp)
        table = dev.readTemporalMotion()
        assert len(table) == 6 and [int(r.moved) for r in table] == [0, 0, 0, 0, 0, 1]
        results.append({"colour": lc._words(dev.readTemporal()), "moments": lc._words(dev.readTemporalMoments()), "motion": np.frombuffer(bytes(table), np.uint32).copy()})
        dev.close()
    _assert_same(results[0], results[1], "the merge after a selective update against the twin in full mode")


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_depth_refusal_leaves_the_handle_unbuilt_and_build_recovers(twk, orc, app, parts, monkeypatch, name, quality):
    """With the limit at 0 every tree is too deep (the hook only lowers the limit): the selective update is refused with twk_build's
    text, the handle is unbuilt and has no update record, and twk_build without the limit recovers it."""
    L = twk._lib
    m = _movable(name)
    dev = _device(twk, app, parts, name, quality, True)
    before = _everything(twk, orc, dev)[0]
    assert dev.buildInfo()["maxTraversalDepth"] >= 1
    original = _instances(name, parts)[m][1]
    dev.updateInstanceTransform(m, original)  # an update that succeeds: there is a record
    assert dev.updateInfo()["selective"] == 1
    monkeypatch.setenv("TWK_MAX_TRAVERSAL_DEPTH", "0")
    with pytest.raises(twk.TwkError) as e:
        dev.updateInstanceTransform(m, _step(original))
    assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_build: the acceleration structure is" in str(e.value) and "levels deep" in str(e.value) and "traversal stacks hold 92" in str(e.value)
    with pytest.raises(twk.TwkError) as e:
        dev.render(0)
    with pytest.raises(twk.TwkError) as e:
        dev.updateInfo()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE, "a failed update leaves no record"
    with pytest.raises(twk.TwkError) as e:
        dev.updateInstanceTransform(m, original)
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_build has not been called" in str(e.value)
    monkeypatch.delenv("TWK_MAX_TRAVERSAL_DEPTH")
    dev.build()  # the transform the refused update set stays, as the scene stays after a failed twk_build
    fresh = _device(twk, app, parts, name, quality, False, {m: _step(original)})
    _assert_same(_everything(twk, orc, dev)[0], _everything(twk, orc, fresh)[0], f"{name}: twk_build after the refused update")
    fresh.close()
    dev.updateInstanceTransform(m, original)
    assert dev.updateInfo()["selective"] == 1
    _assert_same(_everything(twk, orc, dev)[0], before, f"{name}: a selective update on the recovered handle")
    dev.close()


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_refusals(twk, app, parts, name, quality):
    """Per scene, in both modes. `single` has no wall, so no light-carrying instance and no second instance: it runs the refusals that
    need neither (mode, count, duplicate, bad id, bad transform)."""
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    call = "twk_update_instance_transforms"

    def refused(code, f, *words):
        with pytest.raises(twk.TwkError) as e:
            f()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    instances = _instances(name, parts)
    count = len(instances)
    a = S.first_movable(name)
    b = a + 1 if name != "single" else a
    identity = S.affine(1.0, (0, 0, 0))
    for selective in (True, False):
        dev = _device(twk, app, parts, name, quality, selective)
        for mode in (-1, 2, 7):
            refused(VALUE, lambda: dev.setUpdateMode(mode), "twk_set_update_mode", "mode")
        before = _pictures(dev)
        transforms = [dev.instanceTransform(i) for i in range(count)]
        ok = _step(instances[a][1])
        refused(VALUE, lambda: dev.updateInstanceTransforms([a, b, a] if b != a else [a, a], [ok] * (3 if b != a else 2)), call, "entry 2" if b != a else "entry 1", "twice")
        refused(VALUE, lambda: dev.updateInstanceTransforms([], []), call, "count")
        assert L.lib.twk_update_instance_transforms(dev.handle, -3, None, None) == VALUE
        refused(VALUE, lambda: dev.updateInstanceTransforms([a, count], [ok, identity]), call, "entry 1", "bad instance id")
        bad = identity.copy()
        bad[7] = np.nan
        refused(VALUE, lambda: dev.updateInstanceTransforms([a, count + 1], [bad, ok]), call, "entry 0", "finite")
        if name != "single":
            refused(VALUE, lambda: dev.updateInstanceTransforms([a, 0], [ok, identity]), call, "entry 1", "light")
            refused(VALUE, lambda: dev.updateInstanceTransforms([a, b], [ok, bad]), call, "entry 1", "finite")
            flat = identity.copy()
            flat[5] = 0.0
            refused(VALUE, lambda: dev.updateInstanceTransforms([b, a], [flat, ok]), call, "entry 0", "determinant")
            refused(VALUE, lambda: dev.updateInstanceTransform(0, identity), "twk_update_instance_transform:", "light")
        refused(STATE, lambda: dev.updateInfo(), "twk_get_update_info")
        for i in range(count):
            assert np.array_equal(dev.instanceTransform(i), transforms[i]), "a refused batch changes no transform"
        _assert_same(_pictures(dev), before, "a refused batch changes no picture")
        dev.close()
    unbuilt = twk.Device(ordinal=0, miss=app.info.miss)
    refused(STATE, lambda: unbuilt.updateInstanceTransforms([0], [identity]), call, "twk_build")
    unbuilt.close()
