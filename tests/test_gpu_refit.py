"""-m gpu: the refit (twk_refit_geometry_vertices, csrc/bvh_refit.h; its trees are one batch of csrc/bvh_refit.hip). A refit
handle is not a fresh build's, so it is held to what a LEGAL tree is — tests/bvh_audit.py, whole — and to the exact invariants a refit has of its own:
  (a) the audit of the scene with the new vertices passes whole
  (b) binary nodes, wide nodes, node costs, slots and shading records of the refit ranges equal twk_refit_tree_host applied to the
      read-back taken before the refit, bit for bit
  (c) a refit with the same vertices leaves the whole read-back and the kept arrays byte-identical
  (d) A -> B -> A equals a fresh handle built with A byte for byte (acceleration structure, scene arrays, build info except its time),
      and a 4 spp picture at 64 x 36 equals too, in both output formats
  (e) refit B, then updateGeometryVertices(B), equals a fresh handle built with B: a refit damages nothing a rebuild does not rewrite
  (f) every reference word and the pair flags equal those before the refit
  (g) 4096 seeded rays against a fresh handle built with B: hit / miss and the bits of t equal on every ray, the ids on all but at most 4
  (h) refits interleaved with transform updates still pass (a) after every step; refitInfo counts as specified and resets on a rebuild
  (i) with a temporal history the geometry is deformed after a refit, and the motion plane and the own-buffer merge run
  (j) every refusal, after which the read-back is unchanged.
Scenes: tests/refit_scenes.py's meshes of 1 .. 1025 build primitives, entered and flattened (with a direct-leaf instance of 2
triangles), under the four deformations, and the five selective_scenes; both build qualities.

The seed of (g): tests/test_gpu_bvh_audit.py's aimed rays with seed 5. The premise — the SAH-built and the LBVH-built fresh handle of B,
two different trees over the same triangles, differ on NO ray, ids included, so that no equal-t tie is among the rays — holds for this
seed (the first one tried: 3107 of 4096 rays hit in the flat scene, 3103 in the entered one). Both fresh handles are built by the
parent's code — the build's kernels have the parent's ISA instruction for instruction, profiles/r28_refit.md section 4 — and the test
asserts the premise itself on every run, before the refit handle is compared."""
import numpy as np
import pytest

import bvh_audit as A
import lifecycle as lc
import refit_scenes as RS
import scene_snapshot as snapshot
import selective_scenes as S
from conftest import load_app
from test_gpu_bvh_audit import _aimed_rays, _renderers
from test_gpu_selective_update import CORNELL_WALLS, SCENE, SYSTEM, _assert_same, _device, _instances, _step, _structure
from vertex_update_scenes import deformed, with_geometry

pytestmark = pytest.mark.gpu

QUALITIES = pytest.mark.parametrize("quality", [1, 0], ids=["sah", "lbvh"])
KINDS = pytest.mark.parametrize("kind", RS.KINDS)
F32, U32 = np.float32, np.uint32
RAYS, RAY_SEED, TIES = 4096, 5, 4


def _mesh_device(twk, orc, kind, quality, geometries=None, selective=True):
    """A handle on the meshes of refit_scenes (or on `geometries` in their place), built in selective mode."""
    dev = _renderers(twk, orc, geometries or list(RS.meshes()), RS.instances(kind), RS.POLICY, quality, oracle=False)[0]
    if selective:
        dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)  # read by the next build
        dev.build()
    return dev


def _state(twk, orc, dev, kept=True):
    """Everything a reader can get at (test_gpu_selective_update._structure) and the three kept arrays, as words."""
    out = _structure(twk, orc, dev)[0]
    if kept:
        wide, cost, flags = dev.debugReadKeptBuild()
        out["keptWide"], out["keptCost"], out["keptFlags"] = lc._words(wide), lc._words(cost), flags.astype(np.int64)
    return out


def _check_against_the_host_form(twk, what, trees, geometries, new, before, kept_before, after, kept_after):
    """(b) and (f) for every tree that was refit: `before` / `after` are bvh_audit.Readbacks, kept_*: debugReadKeptBuild."""
    for t in trees:
        if t["directLeaf"]:
            continue  # rebuilt, not refit
        nb, nn, sb, ns = t["nodeBase"], t["nodes"], t["slotBase"], t["slots"]
        flags = kept_before[2][sb:sb + ns]
        a, i = new[t["geometry"]]
        want = twk.refit_tree_host(before.nodes[nb:nb + nn], kept_before[0][nb:nb + nn], kept_before[1][nb:nb + nn], before.slots[sb:sb + ns], flags, a, i, nb, sb,
                                   t["leafFlag"], t["transform"], t["instance"])
        for got, key in ((after.nodes[nb:nb + nn], "nodes"), (kept_after[0][nb:nb + nn], "wideNodes"), (kept_after[1][nb:nb + nn].reshape(-1, 1), "nodeCost"),
                         (after.slots[sb:sb + ns], "slots"), (after.shade[sb:sb + ns], "shadeRecords")):
            expect = np.ascontiguousarray(want[key], F32).reshape(got.shape)
            bad = np.nonzero((np.ascontiguousarray(got, F32).view(U32) != expect.view(U32)).reshape(got.shape[0], -1).any(1))[0]
            assert bad.size == 0, f"{what}, {t['name']}: {key} differs from the host form in {bad.size} rows, first {bad[0]}: {got[bad[0]]} against {expect[bad[0]]}"
        # (f)
        assert np.array_equal(after.nodes[nb:nb + nn].view(np.int32)[:, 12:16], before.nodes[nb:nb + nn].view(np.int32)[:, 12:16]), f"{what}, {t['name']}: binary references"
        assert np.array_equal(RS.wide_entries(kept_after[0][nb:nb + nn])[2], RS.wide_entries(kept_before[0][nb:nb + nn])[2]), f"{what}, {t['name']}: wide references"
        assert np.array_equal(after.slots[sb:sb + ns].view(np.int32)[:, [3, 7]], before.slots[sb:sb + ns].view(np.int32)[:, [3, 7]]), f"{what}, {t['name']}: primitive and instance words"
        assert np.array_equal(after.wideQ[nb:nb + nn].view(np.int32)[:, 12:16], before.wideQ[nb:nb + nn].view(np.int32)[:, 12:16]), f"{what}, {t['name']}: quantised references"
    assert np.array_equal(kept_after[2], kept_before[2]), f"{what}: pair flags"


@QUALITIES
@KINDS
@pytest.mark.parametrize("deformation", RS.DEFORMATIONS)
def test_a_refit_scene_passes_the_audit_and_equals_the_host_form(twk, orc, kind, quality, deformation):
    """(a), (b), (f) on the meshes, every geometry refit in turn; refitInfo and updateInfo against the layout."""
    geometries, new, instances = list(RS.meshes()), RS.deformed_meshes(deformation), RS.instances(kind)
    trees, lay = RS.trees(geometries, instances, RS.POLICY)
    dev = _mesh_device(twk, orc, kind, quality)
    try:
        before, kept_before = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
        with pytest.raises(twk.TwkError):
            dev.refitInfo()
        for g in range(len(geometries)):
            dev.refitGeometryVertices(g, new[g][0])
            mine = [t for t in trees if t["geometry"] == g]
            r, u = dev.refitInfo(), dev.updateInfo()
            assert (r["treesRefit"], r["treesRebuilt"]) == (sum(not t["directLeaf"] for t in mine), sum(t["directLeaf"] for t in mine)), (g, r)
            assert r["nodesRefit"] == sum(t["nodes"] for t in mine if not t["directLeaf"]) and r["slotsRewritten"] == sum(t["slots"] for t in mine), (g, r)
            assert r["refitsSinceBuild"] == (1 if r["treesRefit"] else 0) and r["topLevelRebuilt"] == 1 and r["milliseconds"] > 0.0, (g, r)
            assert u["selective"] == 1 and u["treesRebuilt"] == r["treesRebuilt"] and u["instancesMoved"] == 0 and u["slotsRewritten"] == r["slotsRewritten"], (g, u)
            assert dev.buildInfo()["buildMilliseconds"] == u["milliseconds"] == r["milliseconds"]
        after, kept_after = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
    finally:
        dev.close()
    what = f"{kind}, {deformation}"
    A.audit(A.Scene(new, instances, RS.POLICY, quality), after)
    assert not np.array_equal(after.slots.view(U32), before.slots.view(U32)), what + ": the deformation shows"
    _check_against_the_host_form(twk, what, trees, geometries, new, before, kept_before, after, kept_after)


@QUALITIES
@KINDS
def test_a_refit_with_the_same_vertices_changes_no_byte_and_a_refit_back_restores_a_fresh_build(twk, orc, kind, quality):
    """(c), (d), (e) on the meshes: idempotence on everything readable and kept; A -> B -> A against a fresh handle built with A;
    refit B then the rebuild with B against a fresh handle built with B."""
    geometries, new = list(RS.meshes()), RS.deformed_meshes("noise")
    dev = _mesh_device(twk, orc, kind, quality)
    fresh = _mesh_device(twk, orc, kind, quality, selective=False)
    fresh_new = _mesh_device(twk, orc, kind, quality, geometries=new, selective=False)
    try:
        built, want, want_new = _state(twk, orc, dev), _state(twk, orc, fresh, kept=False), _state(twk, orc, fresh_new, kept=False)
        for g in range(len(geometries)):
            dev.refitGeometryVertices(g, geometries[g][0])
        _assert_same(_state(twk, orc, dev), built, f"{kind}: (c) a refit with the vertices the trees were built from")
        for vertices in (new, geometries):
            for g in range(len(geometries)):
                dev.refitGeometryVertices(g, vertices[g][0])
        got = _state(twk, orc, dev)
        _assert_same(got, built, f"{kind}: (d) there and back, against the handle's own build")
        _assert_same({k: got[k] for k in want}, want, f"{kind}: (d) there and back, against a fresh handle")
        for g in range(len(geometries)):
            dev.refitGeometryVertices(g, new[g][0])
        for g in range(len(geometries)):
            dev.updateGeometryVertices(g, new[g][0])
        got = _state(twk, orc, dev)
        _assert_same({k: got[k] for k in want_new}, want_new, f"{kind}: (e) a rebuild after a refit, against a fresh handle")
    finally:
        for d in (dev, fresh, fresh_new):
            d.close()


@QUALITIES
@KINDS
def test_rays_through_a_refit_scene(twk, orc, kind, quality):
    """(g), on the noise deformation."""
    geometries, new, instances = list(RS.meshes()), RS.deformed_meshes("noise"), RS.instances(kind)
    rays = _aimed_rays(new, instances, RAYS, RAY_SEED)
    traced = {}
    for name, q, refit in (("sah", 1, False), ("lbvh", 0, False), ("refit", quality, True)):
        dev = _mesh_device(twk, orc, kind, q, geometries=geometries if refit else new, selective=refit)
        try:
            if refit:
                for g in range(len(geometries)):
                    dev.refitGeometryVertices(g, new[g][0])
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


# ---- the five selective_scenes: pictures, sequences, the temporal history, refusals ---------------------------------------------------
@pytest.fixture(scope="module")
def app(twk):
    a = load_app(twk, SYSTEM, SCENE, (64, 36))
    yield a
    a.close()


@pytest.fixture(scope="module")
def parts(twk, app):
    walls = [app.instance(i) for i in CORNELL_WALLS]
    geometries = [app.geometry(w[0]) for w in walls] + [twk.mesh_box(), twk.mesh_sphere(8, 4, 1.0, np.pi)]
    assert tuple(g[1].size // 3 for g in geometries) == S.TRIANGLES
    return geometries, [(w[1], w[2], w[3]) for w in walls]


def _pictures(dev, half):
    """4 spp from iteration 0 and the geometry AOV, as words."""
    dev.setSampleOffset(0)
    for it in range(4):
        dev.render(it)
    dev.renderGeometry()
    return {"colour": lc._words(dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()), "geometry": lc._words(dev.readGeometry())}


def _deformable(name):
    used = set(S.instance_geometry(name))
    return [g for g in (S.SPHERE, S.BOX, S.FLOOR) if g in used]


def _scene(name, parts, geometry_now, transforms=None):
    """bvh_audit.Scene of selective scene `name` with {geometry: attributes} and {instance: transform} as they are now."""
    geometries = [(geometry_now.get(k, a), i) for k, (a, i) in enumerate(parts[0])]
    instances = [(g, (transforms or {}).get(n, t)) for n, (g, t, _, _) in enumerate(_instances(name, parts))]
    return geometries, instances


@QUALITIES
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_the_selective_scenes_refit(twk, orc, app, parts, name, quality):
    """(a), (b), (d), (e), (f) with pictures: every deformable geometry of the scene refit to vertex_update_scenes.deformed — the audit,
    the host form; then back — the handle's own build and a fresh handle, structure and a 4 spp picture at 64 x 36 in both output
    formats; then refit and rebuilt — a fresh handle built with the new vertices, with its pictures."""
    what = f"{name}"
    new = {g: deformed(parts, g) for g in _deformable(name)}
    geometries, instances = _scene(name, parts, {})
    trees, _ = RS.trees(geometries, instances, S.policy(name))
    for half in (False, True):
        dev = _device(twk, app, parts, name, quality, True, half=half)
        fresh = _device(twk, app, parts, name, quality, False, half=half)
        fresh_new = _device(twk, app, with_geometry(parts, new), name, quality, False, half=half)
        try:
            built = _state(twk, orc, dev)
            before, kept_before = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
            want, want_new = _state(twk, orc, fresh, kept=False), _state(twk, orc, fresh_new, kept=False)
            for g, attributes in new.items():
                dev.refitGeometryVertices(g, attributes)
                assert not dev.geometryDeformed(g), "without a temporal history nothing is kept"
            if not half:
                after, kept_after = snapshot.readback(twk, orc, dev), dev.debugReadKeptBuild()
                new_geometries, _ = _scene(name, parts, new)
                A.audit(A.Scene(new_geometries, instances, S.policy(name), quality), after)
                refit_trees = [t for t in trees if t["geometry"] in new]
                _check_against_the_host_form(twk, what, refit_trees, geometries, new_geometries, before, kept_before, after, kept_after)
            for g in new:
                dev.refitGeometryVertices(g, parts[0][g][0])
            got = _state(twk, orc, dev)
            _assert_same(got, built, what + ": there and back, against the handle's own build")
            _assert_same({k: got[k] for k in want}, want, what + ": there and back, against a fresh handle")
            _assert_same(_pictures(dev, half), _pictures(fresh, half), what + f": the picture after the refit back, half {half}")
            for g, attributes in new.items():
                dev.refitGeometryVertices(g, attributes)
            for g, attributes in new.items():
                dev.updateGeometryVertices(g, attributes)
            got = _state(twk, orc, dev)
            _assert_same({k: got[k] for k in want_new}, want_new, what + ": a rebuild after a refit, against a fresh handle")
            _assert_same(_pictures(dev, half), _pictures(fresh_new, half), what + f": the picture after the rebuild, half {half}")
        finally:
            for d in (dev, fresh, fresh_new):
                d.close()


@QUALITIES
def test_refits_interleaved_with_transform_updates(twk, orc, app, parts, quality):
    """(h) on `mixed`: three entered spheres (one bottom-level tree), walls and a flattened box (instance 7, a world-space tree)."""
    name = "mixed"
    dev = _device(twk, app, parts, name, quality, True)
    now, moved = {}, {}

    def audited(step):
        geometries, instances = _scene(name, parts, now, moved)
        try:
            A.audit(A.Scene(geometries, instances, S.policy(name), quality), snapshot.readback(twk, orc, dev))
        except A.AuditError as e:
            raise AssertionError(f"after {step}: {e}")

    try:
        base = _instances(name, parts)
        now[S.SPHERE] = deformed(parts, S.SPHERE, 1)
        dev.refitGeometryVertices(S.SPHERE, now[S.SPHERE])
        first = dev.refitInfo()
        assert (first["treesRefit"], first["treesRebuilt"], first["refitsSinceBuild"]) == (1, 0, 1) and first["sahBuilt"] > 0.0 and first["sahNow"] > 0.0, first
        audited("the sphere's refit")
        moved[7] = _step(base[7][1])
        dev.updateInstanceTransform(7, moved[7])  # another instance: the flattened box
        audited("the box moved")
        moved[4] = _step(base[4][1], (0.05, 0.0, 0.1))
        dev.updateInstanceTransform(4, moved[4])  # an instance of the refit geometry: its box comes from the refit root box
        audited("a sphere moved")
        now[S.SPHERE] = deformed(parts, S.SPHERE, 2)
        dev.refitGeometryVertices(S.SPHERE, now[S.SPHERE])
        second = dev.refitInfo()
        assert second["refitsSinceBuild"] == 2 and second["sahBuilt"] == first["sahBuilt"], (first, second)
        audited("the sphere's second refit")
        now[S.BOX] = deformed(parts, S.BOX)
        dev.refitGeometryVertices(S.BOX, now[S.BOX])
        box = dev.refitInfo()
        assert (box["treesRefit"], box["refitsSinceBuild"]) == (1, 1), box
        audited("the box's refit")
        moved[7] = _step(moved[7], (0.0, 0.05, 0.0))
        dev.updateInstanceTransform(7, moved[7])  # rebuilds the box's world-space tree: its count starts again
        audited("the refit box moved")
        dev.refitGeometryVertices(S.BOX, now[S.BOX])
        again = dev.refitInfo()
        assert again["refitsSinceBuild"] == 1 and again["sahBuilt"] != box["sahBuilt"], (box, again)
        audited("the box's refit after its rebuild")
        dev.updateGeometryVertices(S.SPHERE, now[S.SPHERE])  # a rebuild of the bottom-level tree
        rebuilt_cost = dev.buildInfo()
        dev.refitGeometryVertices(S.SPHERE, now[S.SPHERE])
        last = dev.refitInfo()
        assert last["refitsSinceBuild"] == 1 and last["sahBuilt"] == last["sahNow"] and last["sahBuilt"] != first["sahBuilt"], (first, last)
        assert dev.buildInfo()["sahInnerCost"] == rebuilt_cost["sahInnerCost"], "a refit with the built vertices leaves the terms"
        audited("the sphere's refit after its rebuild")
        # a floor wall is a direct leaf of two triangles: rebuilt, not refit
        now[S.FLOOR] = deformed(parts, S.FLOOR)
        dev.refitGeometryVertices(S.FLOOR, now[S.FLOOR])
        wall = dev.refitInfo()
        assert (wall["treesRefit"], wall["treesRebuilt"], wall["refitsSinceBuild"], wall["sahBuilt"], wall["sahNow"]) == (0, 1, 0, 0.0, 0.0), wall
        assert dev.updateInfo()["treesRebuilt"] == 1
        audited("the floor's refit")
    finally:
        dev.close()


@QUALITIES
def test_the_temporal_history_survives_a_refit(twk, app, parts, quality):
    """(i) on `flat`: a frame merged, the sphere refit, a second frame with the motion plane merged."""
    tp = twk._lib.Temporal(maxHistory=32, positionTolerance=0.1)
    dev = _device(twk, app, parts, "flat", quality, True)
    try:
        for frame in range(2):
            if frame:
                dev.refitGeometryVertices(S.SPHERE, deformed(parts, S.SPHERE, 2))
                assert dev.geometryDeformed(S.SPHERE) and not dev.geometryDeformed(S.BOX)
            dev.setSampleOffset(2 * frame)
            for it in range(2):
                dev.render(it)
            dev.renderGeometryMotion()
            dev.temporalAccumulate(tp)
            assert not dev.geometryDeformed(S.SPHERE), "the merge swapped the history"
        assert np.isfinite(dev.readTemporal()).all()
    finally:
        dev.close()


@QUALITIES
def test_refusals(twk, orc, app, parts, quality):
    """(j): each refusal under the call's own name with the vertex update's text, and the read-back unchanged after all of them."""
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, f, *words):
        with pytest.raises(twk.TwkError) as e:
            f()
        assert e.value.code == code and "twk_refit_geometry_vertices" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    sphere = np.array(parts[0][S.SPHERE][0], F32).reshape(-1, 12)
    for selective in (True, False):
        dev = _device(twk, app, parts, "flat", quality, selective)
        try:
            before = _state(twk, orc, dev, kept=selective)
            if not selective:
                refused(STATE, lambda: dev.refitGeometryVertices(S.SPHERE, sphere), "twk_set_update_mode", "TWK_UPDATE_SELECTIVE")
                with pytest.raises(twk.TwkError) as e:
                    dev.debugReadKeptBuild()
                assert e.value.code == STATE
            else:
                refused(VALUE, lambda: dev.refitGeometryVertices(len(S.TRIANGLES), sphere), "bad geometry id")
                refused(VALUE, lambda: dev.refitGeometryVertices(-1, sphere), "bad geometry id")
                refused(VALUE, lambda: dev.refitGeometryVertices(S.SPHERE, sphere[:-1]), "vertices")
                refused(VALUE, lambda: dev.refitGeometryVertices(S.BOX, sphere), "vertices")
                for bad in (np.nan, np.inf):
                    broken = sphere.copy()
                    broken[3, 1] = bad
                    refused(VALUE, lambda: dev.refitGeometryVertices(S.SPHERE, broken), "vertex 3", "finite")
                refused(VALUE, lambda: dev.refitGeometryVertices(S.LIGHT, parts[0][S.LIGHT][0]), "instance 0", "light")
                assert L.lib.twk_refit_geometry_vertices(dev.handle, S.SPHERE, None, 0) == VALUE and "NULL attributes" in L.lib.twk_last_error().decode()
            for reader in (dev.updateInfo, dev.refitInfo):
                with pytest.raises(twk.TwkError) as e:
                    reader()
                assert e.value.code == STATE, "a refused refit is no refit and no update"
            _assert_same(_state(twk, orc, dev, kept=selective), before, "a refused refit changes nothing")
        finally:
            dev.close()
    unbuilt = twk.Device(ordinal=0, miss=app.info.miss)
    refused(STATE, lambda: unbuilt.refitGeometryVertices(0, sphere), "twk_build")
    unbuilt.close()
