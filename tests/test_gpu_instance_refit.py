"""-m gpu: the refit of MOVED flattened instances (twk_refit_instance_transform[s], csrc/bvh_refit.hip). A refit handle is not a
fresh build's, so it is held to what a LEGAL tree is — tests/bvh_audit.py, whole — and to the exact invariants of a refit:
  (a) the audit of the scene with the new transforms passes whole
  (b) binary nodes, wide nodes, node costs and slots of every refit tree equal twk_refit_tree_host applied, with the new transform, to
      the read-back taken before the call, bit for bit — for all instances moved by ONE batch call and for the same moves made one by
      one; the shading records equal the host form's AND the read-back from before the call (a transform does not change them); the
      root box the host form returns is the one the refit root node holds (the top level over it is (a)'s); sahNow of the batch equals
      the sum of what the single calls report
  (c) a refit with the transforms the scene was built with changes no readable or kept byte
  (d) A -> B -> A equals a fresh handle built with A byte for byte (structure, scene arrays, build info except its time; on the
      selective_scenes also a 4 spp picture at 64 x 36 in both output formats)
  (e) refit to B, then updateInstanceTransforms(B), equals a fresh handle built with B
  (f) no reference word, primitive word, instance word or pair flag changes
  (g) 4096 aimed rays against a fresh handle built with B: hit / miss and the bits of t equal on every ray, the ids on all but at most 4
  (h) on the five selective_scenes instance refits, vertex refits, rebuilding transform updates and vertex updates interleaved: (a)
      after every step, refitInfo / updateInfo counts against the layout, the refit counts reset by a rebuild
  (i) on the Cornell box with a temporal history and the mirror sphere stepped by the refit call, the motion table marks exactly the
      sphere and the own-buffer merge takes history on more than half of its pixels
  (j) every refusal, after which the read-back is unchanged.
Scenes: tests/refit_scenes.py's meshes of 1 .. 1025 build primitives (trees of 1, 256 and more than 1024 nodes; two direct leaves),
"flat" (every tree of its own) and "entered" (world boxes only); both build qualities. Moves: a translation by 1e4, another
bvh_audit_scenes.place, a mirror (negative determinant), a squash (one axis scaled by 1e-3) — and, beyond those, `turned`: another
rotation angle and other scales than every place() has, so that the boxes really grow.

The seed of (g): tests/test_gpu_bvh_audit.py's aimed rays, starting with seed 5. B gives instance k the k-th of the moves in turn, so
that every kind is in the scene. The premise — the SAH-built and the LBVH-built fresh handle of B, two different trees over the same
triangles, differ on NO ray, ids included — holds for seed 5, the first one tried (3010 of 4096 rays hit in the flat scene, 2956 in
the entered one), and is asserted on every run, before the refit handle is compared."""
import numpy as np
import pytest

import bvh_audit as A
import bvh_audit_scenes as M
import lifecycle as lc
import refit_scenes as RS
import scene_snapshot as snapshot
import selective_scenes as S
from conftest import load_app
from test_gpu_bvh_audit import _aimed_rays
from test_gpu_refit import QUALITIES, KINDS, RAYS, TIES, _check_against_the_host_form, _mesh_device, _pictures, _scene, _state, app, parts  # noqa: F401 (fixtures)
from test_gpu_selective_update import _assert_same, _device, _instances, _step
from vertex_update_scenes import deformed

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
MOVES = ("translate", "place", "mirror", "squash", "turned")
RAY_SEED = 5


def moved(transform, move, k):
    """Transform B of instance k, whose built transform is `transform`."""
    m = np.array(transform, F32).reshape(3, 4).copy()
    if move == "translate":
        m[:, 3] += F32(1.0e4)
    elif move == "place":
        m = np.array(M.place(k + 19), F32).reshape(3, 4)
    elif move == "mirror":
        m[:, 0] = -m[:, 0]
    elif move == "squash":
        m[:, 1] *= F32(1.0e-3)
    elif move == "turned":
        m = np.array(S.rotated((3.0 * (k % 8) + 0.5, 3.0 * (k // 8) - 0.25, 1.0), angle=2.1, scale=(0.2, 0.35, 0.15)), F32).reshape(3, 4)
    else:
        raise KeyError(move)
    return m.reshape(12)


def _moved_scene(kind, move):
    """(ids, [transform B per instance], instances with B) — move None: the k-th move in turn."""
    base = RS.instances(kind)
    new = [moved(t, move or MOVES[k % len(MOVES)], k) for k, (_, t) in enumerate(base)]
    return list(range(len(base))), new, [(g, t) for (g, _), t in zip(base, new)]


def _expect(trees, ids):
    """(treesRefit, treesRebuilt, nodesRefit, slotsRewritten) of a refit of the instances `ids`."""
    mine = [t for t in trees if t["instance"] in ids]
    return (sum(not t["directLeaf"] for t in mine), sum(t["directLeaf"] for t in mine), sum(t["nodes"] for t in mine if not t["directLeaf"]), sum(t["slots"] for t in mine))


def _check_infos(dev, trees, ids, what, top=1):
    r, u = dev.refitInfo(), dev.updateInfo()
    assert (r["treesRefit"], r["treesRebuilt"], r["nodesRefit"], r["slotsRewritten"]) == _expect(trees, ids), (what, r)
    assert r["topLevelRebuilt"] == top and u["topLevelRebuilt"] == top and r["milliseconds"] > 0.0, (what, r)
    assert (u["selective"], u["instancesMoved"], u["instanceRecordsUploaded"], u["treesRebuilt"], u["slotsRewritten"]) == (1, len(ids), len(ids), r["treesRebuilt"], r["slotsRewritten"]), (what, u)
    assert dev.buildInfo()["buildMilliseconds"] == u["milliseconds"] == r["milliseconds"], what
    return r


@QUALITIES
@KINDS
@pytest.mark.parametrize("move", MOVES)
def test_a_moved_scene_passes_the_audit_and_equals_the_host_form(twk, orc, kind, quality, move):
    """(a), (b), (f): all instances in one batch call on one handle, one by one on another."""
    geometries = list(RS.meshes())
    ids, new, instances = _moved_scene(kind, move)
    trees, _ = RS.trees(geometries, instances, RS.POLICY)  # with the new transforms: what the host form is given
    what = f"{kind}, {move}"
    results = {}
    for mode in ("batch", "single"):
        dev = _mesh_device(twk, orc, kind, quality)
        try:
            before, kept_before = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
            with pytest.raises(twk.TwkError):
                dev.refitInfo()
            if mode == "batch":
                dev.refitInstanceTransforms(ids, new)
                info = _check_infos(dev, trees, ids, what)
                assert info["refitsSinceBuild"] == (1 if info["treesRefit"] else 0), info
                sah = (info["sahBuilt"], info["sahNow"])
            else:
                singles = []
                for i in ids:
                    dev.refitInstanceTransform(i, new[i])
                    singles.append(_check_infos(dev, trees, [i], f"{what}, instance {i}"))
                sah = (sum(r["sahBuilt"] for r in singles), sum(r["sahNow"] for r in singles))
            for i in ids:
                assert np.array_equal(dev.instanceTransform(i), new[i])
            after, kept_after = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
        finally:
            dev.close()
        A.audit(A.Scene(geometries, instances, RS.POLICY, quality), after)
        assert not np.array_equal(after.instances.view(U32), before.instances.view(U32)), what + ": the move shows"
        _check_against_the_host_form(twk, f"{what}, {mode}", trees, geometries, geometries, before, kept_before, after, kept_after)
        assert np.array_equal(after.shade.view(U32), before.shade.view(U32)), f"{what}, {mode}: a transform changes no shading record"
        for t in trees:
            if t["directLeaf"] or t["instance"] < 0:
                continue
            nb, nn, sb, ns = t["nodeBase"], t["nodes"], t["slotBase"], t["slots"]
            a, i = geometries[t["geometry"]]
            want = twk.refit_tree_host(before.nodes[nb:nb + nn], kept_before[0][nb:nb + nn], kept_before[1][nb:nb + nn], before.slots[sb:sb + ns], kept_before[2][sb:sb + ns],
                                       a, i, nb, sb, t["leafFlag"], t["transform"], t["instance"])
            root = after.nodes[nb]
            box = root[0:6] if (root[6] == np.inf and root[9] == np.inf) else np.concatenate([np.minimum(root[0:3], root[6:9]), np.maximum(root[3:6], root[9:12])])
            assert np.array_equal(box.view(U32), want["rootBounds"].view(U32)), f"{what}, {mode}, {t['name']}: the root box"
            assert not np.array_equal(after.slots[sb:sb + ns].view(U32), before.slots[sb:sb + ns].view(U32)), f"{what}, {t['name']}: the slots moved"
        results[mode] = (after, kept_after, sah)
    # the batch and the single calls leave the same handle, and the batch's SAH sums are the single calls' added up
    (b_after, b_kept, b_sah), (s_after, s_kept, s_sah) = results["batch"], results["single"]
    for key in ("nodes", "wideQ", "slots", "shade", "instances", "topNodes", "topNodes7"):
        assert np.array_equal(getattr(b_after, key).view(U32), getattr(s_after, key).view(U32)), f"{what}: {key}, batch against single calls"
    for k in range(3):
        assert np.array_equal(lc._words(b_kept[k]), lc._words(s_kept[k])), f"{what}: kept array {k}, batch against single calls"
    assert b_sah == s_sah, f"{what}: sahBuilt / sahNow of the batch {b_sah}, of the single calls added up {s_sah}"
    if kind == "flat":
        assert b_sah[0] > 0.0 and b_sah[1] > 0.0, b_sah
        if move in ("translate", "place"):
            print(f"{what}: sahNow / sahBuilt {b_sah[1] / b_sah[0]:.6f}")


@QUALITIES
@KINDS
def test_a_refit_in_place_changes_no_byte_and_a_refit_back_restores_a_fresh_build(twk, orc, kind, quality):
    """(c), (d), (e) on the meshes, B the moves in turn."""
    ids, new, instances = _moved_scene(kind, None)
    old = [t for _, t in RS.instances(kind)]
    dev = _mesh_device(twk, orc, kind, quality)
    fresh = _mesh_device(twk, orc, kind, quality, selective=False)
    fresh_new = None
    try:
        built, want = _state(twk, orc, dev), _state(twk, orc, fresh, kept=False)
        dev.refitInstanceTransforms(ids, old)
        _assert_same(_state(twk, orc, dev), built, f"{kind}: (c) a batch refit with the transforms the scene was built with")
        for i in ids[::3]:
            dev.refitInstanceTransform(i, old[i])
        _assert_same(_state(twk, orc, dev), built, f"{kind}: (c) single refits with the transforms the scene was built with")
        dev.refitInstanceTransforms(ids, new)
        assert lc.first_difference(_state(twk, orc, dev)["slots"], built["slots"]) is not None or kind == "entered"
        dev.refitInstanceTransforms(ids, old)
        got = _state(twk, orc, dev)
        _assert_same(got, built, f"{kind}: (d) there and back, against the handle's own build")
        _assert_same({k: got[k] for k in want}, want, f"{kind}: (d) there and back, against a fresh handle")
        fresh.close()
        fresh = None
        fresh_new = twk_fresh(twk, orc, kind, quality, instances)
        want_new = _state(twk, orc, fresh_new, kept=False)
        dev.refitInstanceTransforms(ids, new)
        dev.updateInstanceTransforms(ids, new)
        got = _state(twk, orc, dev)
        _assert_same({k: got[k] for k in want_new}, want_new, f"{kind}: (e) a rebuild after a refit, against a fresh handle")
    finally:
        for d in (dev, fresh, fresh_new):
            if d is not None:
                d.close()


def twk_fresh(twk, orc, kind, quality, instances, selective=False):
    """A handle on the meshes under `instances` (their transforms as given), full mode unless asked."""
    from test_gpu_bvh_audit import _renderers
    dev = _renderers(twk, orc, list(RS.meshes()), instances, RS.POLICY, quality, oracle=False)[0]
    if selective:
        dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
        dev.build()
    return dev


@QUALITIES
@KINDS
def test_rays_through_a_moved_scene(twk, orc, kind, quality):
    """(g): B the moves in turn; the refit handle once moved by one batch call."""
    geometries = list(RS.meshes())
    ids, new, instances = _moved_scene(kind, None)
    rays = _aimed_rays(geometries, instances, RAYS, RAY_SEED)
    traced = {}
    for name, q, refit in (("sah", 1, False), ("lbvh", 0, False), ("refit", quality, True)):
        dev = _mesh_device(twk, orc, kind, q) if refit else twk_fresh(twk, orc, kind, q, instances)
        try:
            if refit:
                dev.refitInstanceTransforms(ids, new)
            traced[name] = dev.traceRays(rays)
        finally:
            dev.close()
    (t_sah, id_sah), (t_lbvh, id_lbvh), (t_refit, id_refit) = traced["sah"], traced["lbvh"], traced["refit"]
    hit = id_sah[:, 0] >= 0
    assert 0.3 < hit.mean() < 1.0, hit.mean()
    # the premise of the seed: two different fresh trees over the same triangles agree on every ray, ids included
    assert np.array_equal(id_sah, id_lbvh) and np.array_equal(t_sah[hit].view(U32), t_lbvh[hit].view(U32)), "the seed's premise: no equal-t tie among the rays"
    assert np.array_equal(id_refit[:, 0] >= 0, hit), "hit / miss"
    assert np.array_equal(t_refit[hit, 0].view(U32), t_sah[hit, 0].view(U32)), "the bits of t"
    ties = int((id_refit != id_sah).any(1).sum())
    print(f"{kind}: {int(hit.sum())} of {RAYS} rays hit, ids differ on {ties}")
    assert ties <= TIES, f"the ids differ on {ties} rays"


# ---- the five selective_scenes ---------------------------------------------------------------------------------------------------------
def _movable(name, parts):
    return [i for i, (_, _, _, light) in enumerate(_instances(name, parts)) if light < 0]


def _move_b(name, parts, i, k=0):
    """Another transform for instance i of the scene: its own, turned about y, scaled unequally and stepped."""
    t = np.array(_instances(name, parts)[i][1], np.float64).reshape(3, 4)
    c, s = np.cos(0.4 + 0.3 * k), np.sin(0.4 + 0.3 * k)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.1, 0.8, 1.25])
    out = np.concatenate([t[:, :3] @ r, t[:, 3:] + np.array([[0.03], [0.05 + 0.02 * k], [0.04]])], 1)
    return out.astype(F32).reshape(12)


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_the_selective_scenes_move_and_return(twk, orc, app, parts, name, quality):
    """(a), (b), (d), (e), (f) with pictures: every movable instance refit to another transform in one batch — the audit, the host form;
    then back — the handle's own build and a fresh handle, structure and a 4 spp picture at 64 x 36 in both output formats; then refit
    and rebuilt — a fresh handle built with the new transforms, with its pictures."""
    ids = _movable(name, parts)
    new = {i: _move_b(name, parts, i) for i in ids}
    old = {i: _instances(name, parts)[i][1] for i in ids}
    geometries, instances = _scene(name, parts, {}, new)
    trees, _ = RS.trees(geometries, instances, S.policy(name))
    for half in (False, True):
        dev = _device(twk, app, parts, name, quality, True, half=half)
        fresh = _device(twk, app, parts, name, quality, False, half=half)
        fresh_new = _device(twk, app, parts, name, quality, False, new, half=half)
        try:
            built = _state(twk, orc, dev)
            before, kept_before = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
            want, want_new = _state(twk, orc, fresh, kept=False), _state(twk, orc, fresh_new, kept=False)
            dev.refitInstanceTransforms(ids, [new[i] for i in ids])
            _check_infos(dev, trees, ids, name, top=int(name != "single"))
            if not half:
                after, kept_after = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
                A.audit(A.Scene(geometries, instances, S.policy(name), quality), after)
                _check_against_the_host_form(twk, name, [t for t in trees if t["instance"] in ids], geometries, geometries, before, kept_before, after, kept_after)
                assert np.array_equal(after.shade.view(U32), before.shade.view(U32)), name + ": a transform changes no shading record"
            dev.refitInstanceTransforms(ids, [old[i] for i in ids])
            got = _state(twk, orc, dev)
            _assert_same(got, built, name + ": there and back, against the handle's own build")
            _assert_same({k: got[k] for k in want}, want, name + ": there and back, against a fresh handle")
            _assert_same(_pictures(dev, half), _pictures(fresh, half), name + f": the picture after the refit back, half {half}")
            dev.refitInstanceTransforms(ids, [new[i] for i in ids])
            dev.updateInstanceTransforms(ids, [new[i] for i in ids])
            got = _state(twk, orc, dev)
            _assert_same({k: got[k] for k in want_new}, want_new, name + ": a rebuild after a refit, against a fresh handle")
            _assert_same(_pictures(dev, half), _pictures(fresh_new, half), name + f": the picture after the rebuild, half {half}")
        finally:
            for d in (dev, fresh, fresh_new):
                d.close()


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_instance_refits_interleaved_with_the_other_updates(twk, orc, app, parts, name, quality):
    """(h): per scene a batch refit of every movable instance, a vertex refit, a rebuilding transform update, single refits, a vertex
    update and another batch; the audit after every step, the counts against the layout, and the refit count of every tree kept here
    as the calls must change it: up by one per refit, back to none by a rebuild of the tree."""
    ids = _movable(name, parts)
    base = _instances(name, parts)
    geometry_of = [g for g, _, _, _ in base]
    trees, _ = RS.trees(*_scene(name, parts, {}), S.policy(name))
    own = {t["instance"]: t for t in trees if t["instance"] >= 0}
    counted = {i: 0 for i, t in own.items() if not t["directLeaf"]}  # refits since its last build, per flattened tree
    now, where = {}, {}
    dev = _device(twk, app, parts, name, quality, True)

    def audited(step):
        geometries, instances = _scene(name, parts, now, where)
        try:
            A.audit(A.Scene(geometries, instances, S.policy(name), quality), snapshot.readback(twk, orc, dev))
        except A.AuditError as e:
            raise AssertionError(f"{name} after {step}: {e}")

    def instance_refit(which, k, step):
        for i in which:
            where[i] = _move_b(name, parts, i, k)
            if i in counted:
                counted[i] += 1
        if len(which) == 1:
            dev.refitInstanceTransform(which[0], where[which[0]])
        else:
            dev.refitInstanceTransforms(which, [where[i] for i in which])
        r = _check_infos(dev, trees, which, f"{name}, {step}", top=int(name != "single"))
        assert r["refitsSinceBuild"] == max([counted[i] for i in which if i in counted], default=0), (step, r, counted)
        audited(step)
        return r

    try:
        instance_refit(ids, 0, "the batch refit")
        deformable = [g for g in (S.SPHERE, S.BOX) if g in geometry_of]
        for g in deformable:
            now[g] = deformed(parts, g, 1)
            dev.refitGeometryVertices(g, now[g])
            for i in counted:
                counted[i] += int(geometry_of[i] == g)
            assert dev.updateInfo()["instancesMoved"] == 0
            audited(f"the vertex refit of geometry {g}")
        target = next((i for i in ids if i in counted), ids[-1])
        where[target] = _step(where[target])
        dev.updateInstanceTransform(target, where[target])  # rebuilds the tree: its count starts again
        if target in counted:
            counted[target] = 0
        assert dev.updateInfo()["treesRebuilt"] == (1 if target in own else 0)
        audited("the rebuilding transform update")
        again = instance_refit([target], 1, "the single refit after the rebuild")
        if target in counted:
            assert again["refitsSinceBuild"] == 1, again
        for g in deformable:
            now[g] = deformed(parts, g, 2)
            dev.updateGeometryVertices(g, now[g])  # rebuilds every tree of the geometry
            for i in counted:
                if geometry_of[i] == g:
                    counted[i] = 0
            audited(f"the vertex update of geometry {g}")
        instance_refit(ids, 2, "the batch refit after the rebuilds")
        instance_refit(ids[-1:], 3, "the last single refit")
    finally:
        dev.close()


def test_the_temporal_history_follows_an_instance_refit(twk):
    """(i): the Cornell box at 61 x 37, three frames of the orbit with the mirror sphere stepped by the refit call."""
    from test_gpu_temporal_motion_tiles import SPHERE, STEP
    from test_gpu_temporal_tiles import FRAMES, HEIGHT, SPP, TILE, WIDTH, _camera, _device as _tile_device, _tp
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    tile_app = lc.make_app(twk, load_app, shape)
    dev = _tile_device(twk, tile_app, shape)
    try:
        dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
        dev.build()
        for f in range(FRAMES):
            if f:
                t = dev.instanceTransform(SPHERE)
                t[[3, 7, 11]] += np.array(STEP, F32)
                dev.refitInstanceTransform(SPHERE, t)
                assert dev.refitInfo()["treesRefit"] == 1 and dev.refitInfo()["refitsSinceBuild"] == f
            dev.updateCamera(0, _camera(twk, tile_app, f))
            dev.setSampleOffset(f * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.temporalAccumulate(_tp(twk))
            table = dev.readTemporalMotion()
            assert [r.moved for r in table] == ([] if f == 0 else [int(i == SPHERE) for i in range(tile_app.info.numInstances)])
            sphere = dev.readGeometry()[..., 3].view(np.uint32) == SPHERE + 1
            took = dev.readTemporalMoments()[..., 2] > dev.readMoments()[..., 2]
            assert sphere.sum() > 40 and ((took & sphere).sum() > 0.5 * sphere.sum() if f > 0 else not took.any()), (f, sphere.sum(), (took & sphere).sum())
    finally:
        dev.close()
        tile_app.close()


@QUALITIES
def test_refusals(twk, orc, app, parts, quality):
    """(j): each refusal under the call's own name with the transform update's text, and the read-back unchanged after them."""
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    name = "flat"
    good = {i: _move_b(name, parts, i) for i in _movable(name, parts)}
    a, b = sorted(good)[:2]

    def refused(code, call, f, *words):
        with pytest.raises(twk.TwkError) as e:
            f()
        assert e.value.code == code and call + ":" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    one, many = "twk_refit_instance_transform", "twk_refit_instance_transforms"
    singular = good[a].copy()
    singular[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0.0  # the translation alone
    broken = good[a].copy()
    broken[7] = np.nan
    for selective in (True, False):
        dev = _device(twk, app, parts, name, quality, selective)
        try:
            before = _state(twk, orc, dev, kept=selective)
            if not selective:
                refused(STATE, one, lambda: dev.refitInstanceTransform(a, good[a]), "twk_set_update_mode", "TWK_UPDATE_SELECTIVE")
                refused(STATE, many, lambda: dev.refitInstanceTransforms([a, b], [good[a], good[b]]), "twk_set_update_mode", "TWK_UPDATE_SELECTIVE")
            else:
                n = len(_instances(name, parts))
                refused(VALUE, one, lambda: dev.refitInstanceTransform(n, good[a]), "bad instance id")
                refused(VALUE, one, lambda: dev.refitInstanceTransform(-1, good[a]), "bad instance id")
                refused(VALUE, one, lambda: dev.refitInstanceTransform(a, singular), "determinant")
                refused(VALUE, one, lambda: dev.refitInstanceTransform(a, broken), "finite")
                refused(VALUE, one, lambda: dev.refitInstanceTransform(0, good[a]), "light")
                refused(VALUE, many, lambda: dev.refitInstanceTransforms([a, 0], [good[a], good[b]]), "entry 1", "light")
                refused(VALUE, many, lambda: dev.refitInstanceTransforms([a, b, a], [good[a], good[b], good[a]]), "entry 2", "listed twice")
                refused(VALUE, many, lambda: dev.refitInstanceTransforms([a, b], [good[a], singular]), "entry 1", "determinant")
                refused(VALUE, many, lambda: dev.refitInstanceTransforms([a, n], [good[a], good[b]]), "entry 1", "bad instance id")
                refused(VALUE, many, lambda: dev.refitInstanceTransforms([], []), "count")
                assert L.lib.twk_refit_instance_transform(dev.handle, a, None) == VALUE and "NULL transform" in L.lib.twk_last_error().decode()
                # the same refusals in the same order as the update call makes them: a bad id before a bad transform before a light
                for f_refit, f_update in ((dev.refitInstanceTransform, dev.updateInstanceTransform),):
                    texts = []
                    for f, call in ((f_refit, one), (f_update, "twk_update_instance_transform")):
                        with pytest.raises(twk.TwkError) as e:
                            f(-1, singular)
                        texts.append(str(e.value).replace(call, "<call>"))
                        with pytest.raises(twk.TwkError) as e:
                            f(0, singular)
                        texts.append(str(e.value).replace(call, "<call>"))
                    assert texts[0] == texts[2] and texts[1] == texts[3], texts
            for reader in (dev.updateInfo, dev.refitInfo):
                with pytest.raises(twk.TwkError) as e:
                    reader()
                assert e.value.code == STATE, "a refused refit is no refit and no update"
            for i in good:
                assert np.array_equal(dev.instanceTransform(i), _instances(name, parts)[i][1]), "a refused batch changes nothing"
            _assert_same(_state(twk, orc, dev, kept=selective), before, "a refused refit changes nothing")
        finally:
            dev.close()
    unbuilt = twk.Device(ordinal=0, miss=app.info.miss)
    refused(STATE, one, lambda: unbuilt.refitInstanceTransform(0, good[a]), "twk_build")
    refused(STATE, many, lambda: unbuilt.refitInstanceTransforms([0], [good[a]]), "twk_build")
    unbuilt.close()
