"""-m gpu: a frame's edits in one call (twk_refit_scene, csrc/bvh_refit.hip). THE SEQUENCE is refitGeometryVertices (or its
device form) per geometry entry in order, then refitInstanceTransforms. Every comparison is bit for bit:
  (1) a handle that took refitScene equals a handle that took the sequence: the read-back, the scene arrays, the kept arrays,
      readGeometryVertices, instanceTransform, and on the selective_scenes and "three-kinds" a 4 spp picture at 64 x 36 in both output
      formats; host records, device records, device positions with recomputed frames, and both mixed
  (2) the audit of the new scene passes whole; every refit tree equals twk_refit_tree_host applied to the read-back from before the
      call; no reference, primitive or instance word and no pair flag changes; a kind-2 tree's shading records are the bytes from before
  (3) refitInfo / updateInfo against the restated plan; refitsSinceBuild up by exactly one, also for a tree edited AND moved; sahNow the
      sum of the host form's terms over the refit trees in the plan's order; where no tree is both edited and moved (and the sums
      associate alike: each call of the sequence refits one tree) sahBuilt / sahNow equal the sequence's reports added up
  (4) a call with the built vertices and transforms changes no byte; A -> B -> A equals a fresh build of A; refitScene(B) then the
      rebuilding updates of B equals a fresh build of B
  (5) 4096 aimed rays against a fresh build of B: hit / miss and the bits of t equal, ids differ on at most TIES rays; the seed's
      premise (the SAH and the LBVH fresh build agree on every ray) is asserted first
  (6) no geometry entries: refitInstanceTransforms; one geometry and no instances: refitGeometryVertices — handle and info counts
  (7) the Cornell box at 61 x 37 with a history, three frames: the sphere mesh scaled and its instance stepped by one refitScene in
      every frame, against a handle that made the sequence: previous-position plane, motion table, merged colour and moments
  (8) the refusals that need the device, after which nothing has changed.
Scenes: refit_scenes' meshes of 1 .. 1025 build primitives (trees of 1, 256 and more than 1024 nodes, a 257-slot tree whose last slot
block has one live thread, two direct leaves), "flat" and "entered"; the five selective_scenes; scene_refit_scenes' "three-kinds". Both
build qualities."""
import ctypes as C

import numpy as np
import pytest

import bvh_audit as A
import lifecycle as lc
import refit_scenes as RS
import scene_refit_scenes as SR
import scene_snapshot as snapshot
import selective_scenes as S
from conftest import load_app
from test_gpu_bvh_audit import _aimed_rays
from test_gpu_instance_refit import _move_b, _movable, _moved_scene
from test_gpu_refit import QUALITIES, KINDS, RAYS, TIES, _check_against_the_host_form, _mesh_device, _pictures, _state, app, parts  # noqa: F401 (fixtures)
from test_gpu_selective_update import _assert_same, _device, _instances
from test_gpu_vertex_source import _tensor, torch  # noqa: F401 (fixture)
from vertex_update_scenes import deformed

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
RAY_SEED = 5
SCENE_NAMES = sorted(S.SCENES) + ["three-kinds"]


def _sequence(dev, entries, ids, transforms):
    for g, what in entries:
        if isinstance(what, dict):
            dev.refitGeometryVerticesDevice(g, **what)
        else:
            dev.refitGeometryVertices(g, what)
    if len(ids):
        dev.refitInstanceTransforms(ids, transforms)


def _whole(twk, orc, dev, vertex_counts, num_instances):
    """_state and what the host keeps: every geometry's records and every instance's transform."""
    out = _state(twk, orc, dev)
    # two handles that live side by side are compared: the cost of a node the leaf collapse left unused (an all-zero binary node) is
    # never written and never read — what the allocation held — so it is no part of either handle's state
    unused = ~out["binaryNodes"].reshape(out["keptCost"].shape[0], -1).any(1)
    out["keptCost"] = np.where(unused, 0, out["keptCost"])
    for g, n in enumerate(vertex_counts):
        out[f"vertices {g}"] = lc._words(dev.readGeometryVertices(g, n))
    out["transforms"] = lc._words(np.stack([dev.instanceTransform(i) for i in range(num_instances)]))
    return out


def _counts(info):
    """What an info says the call DID. Not its time, and not keptBytes, which is the device memory the handle holds: the one call
    writes no soup descriptors, so its handle never grows the descriptor scratch the sequence's batch needs (16 B per slot)."""
    return {k: v for k, v in info.items() if k not in ("milliseconds", "keptBytes")}


def _check_infos(dev, plan, moved, what):
    r, u = dev.refitInfo(), dev.updateInfo()
    assert (r["treesRefit"], r["treesRebuilt"], r["nodesRefit"], r["slotsRewritten"], r["topLevelRebuilt"]) == \
        (plan["numTrees"], plan["directLeaves"], plan["nodes"], plan["slotsRewritten"], plan["topLevelRebuilt"]), (what, r, plan)
    assert r["refitsSinceBuild"] == (1 if plan["numTrees"] else 0), (what, r)
    assert (u["selective"], u["instancesMoved"], u["instanceRecordsUploaded"], u["treesRebuilt"], u["slotsRewritten"]) == \
        (1, len(moved), len(moved), plan["directLeaves"], plan["slotsRewritten"]), (what, u)
    assert dev.buildInfo()["buildMilliseconds"] == u["milliseconds"] == r["milliseconds"] > 0.0, what
    return r


def _sah_built(ref, plan, vertices, transforms):
    """The build's terms of the plan's trees, once each, added in the plan's order: per tree ONE single-tree refit on `ref` — a handle on
    the same build, whatever refits it has taken since: sahBuilt is as of a tree's last real build — with the vertices and the transform
    `ref` has now (vertices[geometry], transforms[instance]), and that call's sahBuilt read back."""
    total = 0.0
    for t in plan["treeList"]:
        if t["kind"] == 0:
            ref.refitGeometryVertices(t["geometry"], vertices[t["geometry"]])
        else:
            ref.refitInstanceTransform(t["tree"], transforms[t["tree"]])
        r = ref.refitInfo()
        assert r["treesRefit"] == 1 and r["treesRebuilt"] == 0, (t, r)
        total += r["sahBuilt"]
    return total


# ---- the meshes ------------------------------------------------------------------------------------------------------------------------
@QUALITIES
@KINDS
@pytest.mark.parametrize("deformation,edited", [("noise", "all"), ("noise", "even"), ("translate", "all"), ("collapse", "all")])
def test_the_meshes_equal_the_sequence(twk, orc, kind, quality, deformation, edited):
    """(1), and for the noise (2) and (3): every instance moved (the moves in turn); "even": every second geometry edited, so that the
    trees of the others are kind 2."""
    geometries, deformed_meshes = list(RS.meshes()), RS.deformed_meshes(deformation)
    ids, new, instances = _moved_scene(kind, None)
    which = [g for g in range(len(geometries)) if edited == "all" or g % 2 == 0]
    entries = [(g, deformed_meshes[g][0]) for g in which]
    now = [deformed_meshes[g] if g in which else geometries[g] for g in range(len(geometries))]
    counts = [a.shape[0] for a, _ in geometries]
    what = f"{kind}, {deformation}, {edited}"
    one, seq = _mesh_device(twk, orc, kind, quality), _mesh_device(twk, orc, kind, quality)
    try:
        before, kept_before = snapshot.readback(twk, orc, one), one.debugReadKeptBuild()
        one.refitScene(entries, ids, new)
        _sequence(seq, entries, ids, new)
        _assert_same(_whole(twk, orc, one, counts, len(ids)), _whole(twk, orc, seq, counts, len(ids)), what + ": the one call against the sequence")
        if deformation != "noise":
            return
        gi, gt = [g for g, _ in instances], [i.size // 3 for _, i in geometries]
        plan = SR.restate(gi, gt, RS.POLICY, which, ids)
        info = _check_infos(one, plan, ids, what)
        after, kept_after = snapshot.readback(twk, orc, one), one.debugReadKeptBuild()
        # (3) sahBuilt: each refit tree's built terms once — also the trees that are edited AND moved — from single-tree refits on the other handle
        sah_built = _sah_built(seq, plan, [a for a, _ in now], new)
    finally:
        one.close()
        seq.close()
    A.audit(A.Scene(now, instances, RS.POLICY, quality), after)
    trees, _ = RS.trees(geometries, instances, RS.POLICY)  # with the new transforms: what the host form is given
    refit = {t["tree"] for t in plan["treeList"]}
    mine = [t for t in trees if (~t["geometry"] if t["instance"] < 0 else t["instance"]) in refit]
    assert len(mine) == plan["numTrees"]
    _check_against_the_host_form(twk, what, mine, geometries, now, before, kept_before, after, kept_after)
    # (2) kind 2: the shading records are the bytes from before the call; (3) sahNow in the plan's order
    sah_now = 0.0
    for p in plan["treeList"]:
        t = next(t for t in mine if t["nodeBase"] == p["nodeBase"])
        nb, nn, sb, ns = t["nodeBase"], t["nodes"], t["slotBase"], t["slots"]
        if p["kind"] == 2:
            assert np.array_equal(after.shade[sb:sb + ns].view(U32), before.shade[sb:sb + ns].view(U32)), f"{what}, {t['name']}: a moved tree's shading records"
        a, i = now[t["geometry"]]
        want = twk.refit_tree_host(before.nodes[nb:nb + nn], kept_before[0][nb:nb + nn], kept_before[1][nb:nb + nn], before.slots[sb:sb + ns], kept_before[2][sb:sb + ns],
                                   a, i, nb, sb, t["leafFlag"], t["transform"], t["instance"])
        sah_now += want["terms"][0] + want["terms"][1]
    assert info["sahNow"] == sah_now and info["sahBuilt"] == sah_built and (info["sahBuilt"] > 0.0) == (plan["numTrees"] > 0), (what, info, sah_now, sah_built)


@QUALITIES
def test_the_reports_equal_the_sequences_added_up(twk, orc, quality):
    """(3), last part, on "flat": geometries 2 .. 6 edited (one tree each), instance 7 moved — no tree is both, every call of the
    sequence refits one tree, and the trees come in the plan's order, so that the sums associate alike."""
    deformed_meshes = RS.deformed_meshes("noise")
    ids, new, _ = _moved_scene("flat", None)
    entries = [(g, deformed_meshes[g][0]) for g in range(2, 7)]
    one, seq = _mesh_device(twk, orc, "flat", quality), _mesh_device(twk, orc, "flat", quality)
    try:
        one.refitScene(entries, [7], [new[7]])
        got = one.refitInfo()
        built = now_ = 0.0
        for g, a in entries:
            seq.refitGeometryVertices(g, a)
            r = seq.refitInfo()
            assert r["treesRefit"] == 1
            built, now_ = built + r["sahBuilt"], now_ + r["sahNow"]
        seq.refitInstanceTransforms([7], [new[7]])
        r = seq.refitInfo()
        built, now_ = built + r["sahBuilt"], now_ + r["sahNow"]
        assert got["treesRefit"] == 6 and (got["sahBuilt"], got["sahNow"]) == (built, now_), (got, built, now_)
    finally:
        one.close()
        seq.close()


@QUALITIES
@KINDS
@pytest.mark.parametrize("mode", ["records", "positions", "mixed"])
def test_device_sources_equal_the_sequence(twk, orc, torch, kind, quality, mode):  # noqa: F811
    """(1) with device sources from torch.empty: all entries records; all positions with recomputeFrames; host and device entries mixed."""
    geometries, deformed_meshes = list(RS.meshes()), RS.deformed_meshes("noise")
    ids, new, _ = _moved_scene(kind, None)
    counts = [a.shape[0] for a, _ in geometries]

    def entries():
        out = []
        for g, (a, _) in enumerate(deformed_meshes):
            if mode == "records" or (mode == "mixed" and g % 3 == 0):
                out.append((g, dict(source=_tensor(torch, a))))
            elif mode == "positions" or (mode == "mixed" and g % 3 == 1):
                out.append((g, dict(source=_tensor(torch, a[:, 0:3]), recomputeFrames=True)))
            else:
                out.append((g, a))
        return out

    one, seq = _mesh_device(twk, orc, kind, quality), _mesh_device(twk, orc, kind, quality)
    try:
        one.refitScene(entries(), ids, new)
        _sequence(seq, entries(), ids, new)
        torch.cuda.synchronize()
        _assert_same(_whole(twk, orc, one, counts, len(ids)), _whole(twk, orc, seq, counts, len(ids)), f"{kind}, {mode}: the one call against the sequence")
        assert _counts(one.updateInfo())["slotsRewritten"] == _counts(one.refitInfo())["slotsRewritten"]
    finally:
        one.close()
        seq.close()


@QUALITIES
@KINDS
def test_refit_invariants_on_the_meshes(twk, orc, kind, quality):
    """(4): the built data changes no byte; A -> B -> A is a fresh build of A; refitScene(B) then the rebuilds of B is a fresh build of B."""
    geometries, deformed_meshes = list(RS.meshes()), RS.deformed_meshes("noise")
    ids, new, instances = _moved_scene(kind, None)
    old = [t for _, t in RS.instances(kind)]
    a_entries, b_entries = [(g, a) for g, (a, _) in enumerate(geometries)], [(g, a) for g, (a, _) in enumerate(deformed_meshes)]
    dev = _mesh_device(twk, orc, kind, quality)
    fresh = _mesh_device(twk, orc, kind, quality, selective=False)
    fresh_new = None
    try:
        built, want = _state(twk, orc, dev), _state(twk, orc, fresh, kept=False)
        dev.refitScene(a_entries, ids, old)
        _assert_same(_state(twk, orc, dev), built, f"{kind}: a call with the built vertices and transforms")
        dev.refitScene(b_entries, ids, new)
        assert lc.first_difference(_state(twk, orc, dev)["slots"], built["slots"]) is not None
        dev.refitScene(a_entries, ids, old)
        got = _state(twk, orc, dev)
        _assert_same(got, built, f"{kind}: there and back, against the handle's own build")
        _assert_same({k: got[k] for k in want}, want, f"{kind}: there and back, against a fresh handle")
        fresh.close()
        fresh = None
        from test_gpu_bvh_audit import _renderers
        fresh_new = _renderers(twk, orc, deformed_meshes, instances, RS.POLICY, quality, oracle=False)[0]
        want_new = _state(twk, orc, fresh_new, kept=False)
        dev.refitScene(b_entries, ids, new)
        for g, a in b_entries:
            dev.updateGeometryVertices(g, a)
        dev.updateInstanceTransforms(ids, new)
        got = _state(twk, orc, dev)
        _assert_same({k: got[k] for k in want_new}, want_new, f"{kind}: the rebuilds after the one call, against a fresh handle")
    finally:
        for d in (dev, fresh, fresh_new):
            if d is not None:
                d.close()


@QUALITIES
@KINDS
def test_rays_through_a_refit_scene(twk, orc, kind, quality):
    """(5) on the meshes: B the noise and the moves in turn."""
    from test_gpu_bvh_audit import _renderers
    geometries, deformed_meshes = list(RS.meshes()), RS.deformed_meshes("noise")
    ids, new, instances = _moved_scene(kind, None)
    rays = _aimed_rays(deformed_meshes, instances, RAYS, RAY_SEED)
    traced = {}
    for name, q, refit in (("sah", 1, False), ("lbvh", 0, False), ("refit", quality, True)):
        dev = _mesh_device(twk, orc, kind, q) if refit else _renderers(twk, orc, deformed_meshes, instances, RS.POLICY, q, oracle=False)[0]
        try:
            if refit:
                dev.refitScene([(g, a) for g, (a, _) in enumerate(deformed_meshes)], ids, new)
            traced[name] = dev.traceRays(rays)
        finally:
            dev.close()
    (t_sah, id_sah), (t_lbvh, id_lbvh), (t_refit, id_refit) = traced["sah"], traced["lbvh"], traced["refit"]
    hit = id_sah[:, 0] >= 0
    assert 0.3 < hit.mean() < 1.0, hit.mean()
    assert np.array_equal(id_sah, id_lbvh) and np.array_equal(t_sah[hit].view(U32), t_lbvh[hit].view(U32)), f"the premise of seed {RAY_SEED}: no equal-t tie among the rays"
    assert np.array_equal(id_refit[:, 0] >= 0, hit), "hit / miss"
    assert np.array_equal(t_refit[hit, 0].view(U32), t_sah[hit, 0].view(U32)), "the bits of t"
    ties = int((id_refit != id_sah).any(1).sum())
    print(f"{kind}: {int(hit.sum())} of {RAYS} rays hit, ids differ on {ties}")
    assert ties <= TIES, f"the ids differ on {ties} rays"


THREE_KINDS_RAY_SEED = 5  # the first seed tried; its premise is asserted on every run


def _three_kinds_b(parts):
    """(parts of "three-kinds", instances as built, policy, entries, moved, new transforms, geometries of B, instances of B)."""
    scene_parts, instances, policy, edited, moved = _scene_of("three-kinds", parts)
    entries = [(g, deformed(scene_parts, g, 1)) for g in edited]
    new = [_moved_to(instances, i) for i in moved]
    now = [(dict(entries).get(g, np.array(a, F32).reshape(-1, 12)), i) for g, (a, i) in enumerate(scene_parts[0])]
    where = dict(zip(moved, new))
    return scene_parts, instances, policy, entries, moved, new, now, [(g, where.get(n, t), m, l) for n, (g, t, m, l) in enumerate(instances)]


def _three_kinds_fresh_traces(twk, app, parts, rays):  # noqa: F811
    """The rays through a fresh SAH and a fresh LBVH build of B."""
    _, _, policy, _, _, _, now, instances_b = _three_kinds_b(parts)
    out = {}
    for name, q in (("sah", 1), ("lbvh", 0)):
        dev = _device(twk, app, (now, parts[1]), "three-kinds", q, False, instances=instances_b, policy=policy)
        try:
            out[name] = dev.traceRays(rays)
        finally:
            dev.close()
    return out


@QUALITIES
def test_rays_through_three_kinds(twk, app, parts, quality):  # noqa: F811
    """(5) on "three-kinds": a kind-0 tree (entered through two instances, one of them moved), a tree edited AND moved and a kind-2 tree
    side by side, the walls rebuilt around them."""
    scene_parts, instances, policy, entries, moved, new, now, instances_b = _three_kinds_b(parts)
    rays = _aimed_rays(now, [(g, t) for g, t, _, _ in instances_b], RAYS, THREE_KINDS_RAY_SEED)
    traced = _three_kinds_fresh_traces(twk, app, parts, rays)
    dev = _device(twk, app, scene_parts, "three-kinds", quality, True, instances=instances, policy=policy)
    try:
        dev.refitScene(entries, moved, new)
        traced["refit"] = dev.traceRays(rays)
    finally:
        dev.close()
    (t_sah, id_sah), (t_lbvh, id_lbvh), (t_refit, id_refit) = traced["sah"], traced["lbvh"], traced["refit"]
    hit = id_sah[:, 0] >= 0
    assert 0.3 < hit.mean() <= 1.0, hit.mean()
    assert np.array_equal(id_sah, id_lbvh) and np.array_equal(t_sah[hit].view(U32), t_lbvh[hit].view(U32)), f"the premise of seed {THREE_KINDS_RAY_SEED}: no equal-t tie among the rays"
    assert np.array_equal(id_refit[:, 0] >= 0, hit), "hit / miss"
    assert np.array_equal(t_refit[hit, 0].view(U32), t_sah[hit, 0].view(U32)), "the bits of t"
    ties = int((id_refit != id_sah).any(1).sum())
    for i in (4, 5, 6, 7):
        assert (id_sah[hit, 0] == i).sum() > 20, f"rays reach instance {i}"
    print(f"three-kinds, seed {THREE_KINDS_RAY_SEED}: {int(hit.sum())} of {RAYS} rays hit, ids differ on {ties}")
    assert ties <= TIES, f"the ids differ on {ties} rays"


@QUALITIES
@KINDS
def test_the_degenerate_forms(twk, orc, kind, quality):
    """(6): handle and info counts."""
    geometries, deformed_meshes = list(RS.meshes()), RS.deformed_meshes("noise")
    ids, new, _ = _moved_scene(kind, None)
    counts = [a.shape[0] for a, _ in geometries]
    one, seq = _mesh_device(twk, orc, kind, quality), _mesh_device(twk, orc, kind, quality)
    try:
        one.refitScene([], ids, new)
        seq.refitInstanceTransforms(ids, new)
        _assert_same(_whole(twk, orc, one, counts, len(ids)), _whole(twk, orc, seq, counts, len(ids)), f"{kind}: no geometry entries")
        assert _counts(one.refitInfo()) == _counts(seq.refitInfo()) and _counts(one.updateInfo()) == _counts(seq.updateInfo()), (one.refitInfo(), seq.refitInfo())
        assert one.updateInfo()["keptBytes"] <= seq.updateInfo()["keptBytes"]
        for g in (5, 7, 1):  # the odd mesh, the largest, a direct leaf
            one.refitScene([(g, deformed_meshes[g][0])])
            seq.refitGeometryVertices(g, deformed_meshes[g][0])
            assert _counts(one.refitInfo()) == _counts(seq.refitInfo()) and _counts(one.updateInfo()) == _counts(seq.updateInfo()), (g, one.refitInfo(), seq.refitInfo())
        _assert_same(_whole(twk, orc, one, counts, len(ids)), _whole(twk, orc, seq, counts, len(ids)), f"{kind}: one geometry entry, no instances")
    finally:
        one.close()
        seq.close()


# ---- the selective_scenes and "three-kinds": pictures ----------------------------------------------------------------------------------
def _scene_of(name, parts):
    """(parts, instances [(geometry, transform, material, light)], policy, edited geometries, moved instances) of a scene."""
    if name != "three-kinds":
        used = set(S.instance_geometry(name))
        return parts, _instances(name, parts), S.policy(name), [g for g in (S.SPHERE, S.BOX, S.FLOOR) if g in used], _movable(name, parts)
    walls = [(g, t, m, l) for g, (t, m, l) in zip(S.WALLS, parts[1])]
    more = (list(parts[0]) + [SR.odd_mesh()], parts[1])
    return more, walls + [(g, t, m, -1) for g, t, m in SR.three_kinds_rest()], SR.THREE_KINDS_POLICY, list(SR.THREE_KINDS_EDITED), list(SR.THREE_KINDS_MOVED)


def _moved_to(instances, i, k=0):
    """test_gpu_instance_refit._move_b for any instance list."""
    t = np.array(instances[i][1], np.float64).reshape(3, 4)
    c, s = np.cos(0.4 + 0.3 * k), np.sin(0.4 + 0.3 * k)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.1, 0.8, 1.25])
    return np.concatenate([t[:, :3] @ r, t[:, 3:] + np.array([[0.03], [0.05 + 0.02 * k], [0.04]])], 1).astype(F32).reshape(12)


@QUALITIES
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_scenes_equal_the_sequence_with_pictures(twk, orc, app, parts, name, quality):  # noqa: F811
    """(1), (3), (4) with pictures, in both output formats: the one call against the sequence; the infos against the plan; back to A
    against a fresh handle; on "three-kinds" the tree that is edited and moved counts one refit."""
    scene_parts, instances, policy, edited, moved = _scene_of(name, parts)
    entries = [(g, deformed(scene_parts, g, 1)) for g in edited]
    back = [(g, np.array(scene_parts[0][g][0], F32).reshape(-1, 12)) for g in edited]
    new, old = [_moved_to(instances, i) for i in moved], [instances[i][1] for i in moved]
    counts = [np.asarray(a).reshape(-1, 12).shape[0] for a, _ in scene_parts[0]]
    plan = SR.restate([g for g, _, _, _ in instances], [np.asarray(i).size // 3 for _, i in scene_parts[0]], policy, edited, moved)
    for half in (False, True):
        make = lambda selective=True: _device(twk, app, scene_parts, name, quality, selective, half=half, instances=instances, policy=policy)
        one, seq, fresh = make(), make(), make(False)
        try:
            one.refitScene(entries, moved, new)
            _sequence(seq, entries, moved, new)
            what = f"{name}, half {half}"
            info = _check_infos(one, plan, moved, what)
            _assert_same(_whole(twk, orc, one, counts, len(instances)), _whole(twk, orc, seq, counts, len(instances)), what + ": the one call against the sequence")
            _assert_same(_pictures(one, half), _pictures(seq, half), what + ": the pictures")
            now_vertices = [dict(entries).get(g, np.array(a, F32).reshape(-1, 12)) for g, (a, _) in enumerate(scene_parts[0])]
            now_transforms = [dict(zip(moved, new)).get(n, t) for n, (_, t, _, _) in enumerate(instances)]
            assert info["sahBuilt"] == _sah_built(seq, plan, now_vertices, now_transforms), (what, info)
            if not half:
                now = [(dict(entries).get(g, a), i) for g, (a, i) in enumerate(scene_parts[0])]
                where = dict(zip(moved, new))
                A.audit(A.Scene(now, [(g, where.get(n, t)) for n, (g, t, _, _) in enumerate(instances)], policy, quality), snapshot.readback(twk, orc, one))
            one.refitScene(back, moved, old)
            assert one.refitInfo()["refitsSinceBuild"] == (2 if plan["numTrees"] else 0)
            want = _state(twk, orc, fresh, kept=False)
            got = _state(twk, orc, one)
            _assert_same({k: got[k] for k in want}, want, what + ": there and back, against a fresh handle")
            _assert_same(_pictures(one, half), _pictures(fresh, half), what + ": the picture after the call back")
        finally:
            for d in (one, seq, fresh):
                d.close()


# ---- the temporal history --------------------------------------------------------------------------------------------------------------
def test_the_temporal_history_follows_the_one_call(twk):
    """(7)."""
    from test_gpu_temporal_motion_tiles import SPHERE, STEP
    from test_gpu_temporal_tiles import FRAMES, HEIGHT, SPP, TILE, WIDTH, _camera, _device as _tile_device, _tp
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    tile_app = lc.make_app(twk, load_app, shape)
    devices = [_tile_device(twk, tile_app, shape) for _ in range(2)]
    try:
        geometry = tile_app.instance(SPHERE)[0]
        built = np.array(tile_app.geometry(geometry)[0], F32).reshape(-1, 12)
        for dev in devices:
            dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
            dev.build()
        for f in range(FRAMES):
            frames = []
            for k, dev in enumerate(devices):
                vertices = built.copy()
                vertices[:, 0:3] *= F32(1.0 + 0.04 * (f + 1))
                t = dev.instanceTransform(SPHERE)
                t[[3, 7, 11]] += np.array(STEP, F32)
                if k == 0:
                    dev.refitScene([(geometry, vertices)], [SPHERE], [t])  # one call per frame, the first frame included
                    assert dev.refitInfo()["refitsSinceBuild"] == (f + 1 if dev.refitInfo()["treesRefit"] else 0)
                else:
                    dev.refitGeometryVertices(geometry, vertices)
                    dev.refitInstanceTransforms([SPHERE], [t])
                assert dev.geometryDeformed(geometry) == (f > 0), "previous positions are kept once there is a history"
                dev.updateCamera(0, _camera(twk, tile_app, f))
                dev.setSampleOffset(f * SPP)
                for it in range(SPP):
                    dev.render(it)
                dev.renderGeometryMotion()
                plane = dev.readPreviousPositions()
                dev.temporalAccumulate(_tp(twk))
                table = np.concatenate([np.frombuffer(bytes(r), U32) for r in dev.readTemporalMotion()]) if len(dev.readTemporalMotion()) else np.zeros(0, U32)
                frames.append({"plane": lc._words(plane), "motion": table.astype(np.int64), "colour": lc._words(dev.readTemporal()), "moments": lc._words(dev.readTemporalMoments())})
            _assert_same(frames[0], frames[1], f"frame {f}: the one call against the sequence")
    finally:
        for dev in devices:
            dev.close()
        tile_app.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@QUALITIES
def test_refusals(twk, orc, app, parts, torch, quality):  # noqa: F811
    """(8), and the order of the refusals that need a built handle; after all of them the handle is what it was."""
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    name = "flat"
    instances = _instances(name, parts)
    sphere, box = (np.array(parts[0][g][0], F32).reshape(-1, 12) for g in (S.SPHERE, S.BOX))
    good = {i: _move_b(name, parts, i) for i in _movable(name, parts)}
    a, b = sorted(good)[:2]

    def refused(code, f, *words):
        with pytest.raises(twk.TwkError) as e:
            f()
        assert e.value.code == code and str(e.value).count("twk_refit_scene: ") == 1, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    for selective in (True, False):
        dev = _device(twk, app, parts, name, quality, selective)
        try:
            before = _state(twk, orc, dev, kept=selective)
            if not selective:
                refused(STATE, lambda: dev.refitScene([(S.SPHERE, sphere)], [a], [good[a]]), "twk_set_update_mode", "TWK_UPDATE_SELECTIVE")
            else:
                broken = sphere.copy()
                broken[3, 1] = np.nan
                singular = good[a].copy()
                singular[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0.0
                # the geometry entries in order, each with its index, before the instance entries
                refused(VALUE, lambda: dev.refitScene([(S.SPHERE, sphere), (S.BOX, box[:-1])], [a], [singular]), "geometry entry 1: ", "vertices")
                refused(VALUE, lambda: dev.refitScene([(S.SPHERE, sphere), (len(S.TRIANGLES), box)], [a], [good[a]]), "geometry entry 1: ", "bad geometry id")
                refused(VALUE, lambda: dev.refitScene([(S.SPHERE, broken), (S.BOX, box[:-1])]), "geometry entry 0: ", "vertex 3", "finite")
                refused(VALUE, lambda: dev.refitScene([(S.SPHERE, sphere), (S.BOX, box), (S.SPHERE, sphere)]), "geometry entry 2: ", "listed twice")
                refused(VALUE, lambda: dev.refitScene([(S.BOX, box), (S.LIGHT, parts[0][S.LIGHT][0])]), "geometry entry 1: ", "instance 0", "light")
                refused(VALUE, lambda: dev.refitScene([(S.SPHERE, sphere)], [a, 0], [good[a], good[b]]), "entry 1: ", "light")
                refused(VALUE, lambda: dev.refitScene([(S.SPHERE, sphere)], [a, b], [good[a], singular]), "entry 1: ", "determinant")
                refused(VALUE, lambda: dev.refitScene([], [a, b, a], [good[a], good[b], good[a]]), "entry 2: ", "listed twice")
                refused(VALUE, lambda: dev.refitScene([], [a, len(instances)], [good[a], good[b]]), "entry 1: ", "bad instance id")
                # neither or both of attributes and source; reserved
                edit = (L.GeometryEdit * 1)()
                edit[0].idGeometry, edit[0].numVertices = S.SPHERE, sphere.shape[0]
                assert L.lib.twk_refit_scene(dev.handle, 1, edit, 0, None, None) == VALUE and "geometry entry 0: the entry sets exactly one" in L.lib.twk_last_error().decode()
                source = L.VertexSource()
                source.attributes = _tensor(torch, sphere).data_ptr()
                edit[0].attributes, edit[0].source = sphere.ctypes.data, C.pointer(source)
                assert L.lib.twk_refit_scene(dev.handle, 1, edit, 0, None, None) == VALUE and "geometry entry 0: the entry sets exactly one" in L.lib.twk_last_error().decode()
                edit[0].attributes, edit[0].reserved = None, 7
                assert L.lib.twk_refit_scene(dev.handle, 1, edit, 0, None, None) == VALUE and "geometry entry 0: the reserved word" in L.lib.twk_last_error().decode()
                # device sources: an emitter's geometry, and LAST the finite check —
                # the second of two sources, its entry and its vertex; the first source's geometry is unwritten
                good_box, bad_sphere = _tensor(torch, deformed(parts, S.BOX, 1)), _tensor(torch, broken)
                refused(VALUE, lambda: dev.refitScene([(S.BOX, dict(source=good_box)), (S.SPHERE, dict(source=bad_sphere))], [a], [good[a]]), "geometry entry 1: vertex 3: ", "finite")
                refused(VALUE, lambda: dev.refitScene([(S.BOX, dict(source=good_box)), (S.SPHERE, dict(source=bad_sphere))], [a], [singular]), "entry 0: ", "determinant")
                refused(VALUE, lambda: dev.refitScene([(S.BOX, dict(source=good_box)), (S.LIGHT, dict(source=_tensor(torch, np.array(parts[0][S.LIGHT][0], F32).reshape(-1, 12))))]), "geometry entry 1: ", "light")
                # (a source that overlaps the handle's own attribute array is refused with the device call's text; no call hands that pointer
                # out, so no test can name it: tests/test_gpu_vertex_source.py says the same)
                assert np.array_equal(dev.readGeometryVertices(S.BOX, box.shape[0]).view(U32), box.view(U32)), "the first source's geometry is unwritten"
            for reader in (dev.updateInfo, dev.refitInfo):
                with pytest.raises(twk.TwkError) as e:
                    reader()
                assert e.value.code == STATE, "a refused call is no refit and no update"
            for i in good:
                assert np.array_equal(dev.instanceTransform(i), instances[i][1]), "a refused call changes nothing"
            _assert_same(_state(twk, orc, dev, kept=selective), before, "a refused call changes nothing")
        finally:
            dev.close()
    unbuilt = twk.Device(ordinal=0, miss=app.info.miss)
    refused(STATE, lambda: unbuilt.refitScene([(S.SPHERE, sphere)], [a], [good[a]]), "twk_build")
    unbuilt.close()
