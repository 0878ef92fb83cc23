"""What tests/test_scene_refit_host.py and tests/test_gpu_scene_refit.py share: the scene "three-kinds", the scenes of the plan tests as
(instance geometry, geometry triangles, policy), and the plan of a twk_refit_scene call restated in plain Python from
bvh_reference.scene_layout. A helper module, not a conftest.

"three-kinds", policy (0, 1): the walls of selective_scenes (instances 0 .. 3, one reference each: flattened, two triangles: direct
leaves), two instances of the 48-triangle sphere (4, 5: two references, entered), one box (6: flattened), one instance of
refit_scenes' 65-primitive "odd" mesh of 127 triangles (7: flattened; geometry 6, behind selective_scenes' six). EDIT sphere and box,
MOVE the box, the odd mesh and sphere 4: the batch is the sphere's bottom-level tree (kind 0), the box's tree (kind 1: edited AND
moved), the odd mesh's tree (kind 2) — every kind next to a different kind in the block tables; sphere 4 gets its box as a moved
instance, sphere 5 as an instance of an edited geometry."""
import numpy as np

import bvh_reference as R
import refit_scenes as RS
import selective_scenes as S

BLOCK = 256
SLOT_BYTES = (176, 176, 48)  # written per slot by kind
ODD = 6  # the odd mesh's geometry index in "three-kinds"
THREE_KINDS_POLICY = (0, 1)
THREE_KINDS_EDITED = (S.SPHERE, S.BOX)
THREE_KINDS_MOVED = (6, 7, 4)


def odd_mesh():
    assert RS.SIZES[5] == (65, "odd")
    return RS.meshes()[5]


def three_kinds_rest():
    """[(geometry, transform, material)] after the walls."""
    return [(S.SPHERE, S.affine(0.35, S.SPHERE_AT[0]), 6), (S.SPHERE, S.affine(0.35, S.SPHERE_AT[1]), 7), (S.BOX, S.affine(0.22, (0.45, 0.23, -0.35)), 2),
            (ODD, S.rotated((-0.35, 1.2, 0.35), angle=0.9, scale=(0.35, 0.3, 0.4)), 3)]


def three_kinds_geometry():
    return list(S.WALLS) + [g for g, _, _ in three_kinds_rest()]


def three_kinds_triangles():
    return list(S.TRIANGLES) + [odd_mesh()[1].size // 3]


def plan_scenes():
    """{name: (instance geometry, geometry triangles, policy)}: refit_scenes' two ("meshes-flat", "meshes-entered"), selective_scenes' five,
    "three-kinds"."""
    mesh_triangles = [i.size // 3 for _, i in RS.meshes()]
    out = {"meshes-" + kind: ([g for g, _ in RS.instances(kind)], mesh_triangles, RS.POLICY) for kind in RS.KINDS}
    out.update({name: (S.instance_geometry(name), list(S.TRIANGLES), S.policy(name)) for name in S.SCENES})
    out["three-kinds"] = (three_kinds_geometry(), three_kinds_triangles(), THREE_KINDS_POLICY)
    return out


def restate(instance_geometry, geometry_triangles, policy, updated, moved):
    """The batch of refitScene(updated geometries, moved instances), in plain Python: the bottom-level trees of the updated entered
    geometries ascending (listed ~geometry, kind 0), then the flattened instances that are moved or of an updated geometry and no
    direct leaves, ascending (kind 1 where the geometry is updated, else 2); refit_batch_plan.h's offsets and block tables over them."""
    gi, gt = list(instance_geometry), list(geometry_triangles)
    lay = R.scene_layout(gi, gt, policy)
    count = lambda n: n - 1 if n > 1 else 1
    updated, moved = set(int(g) for g in updated), set(int(i) for i in moved)
    trees = [dict(tree=~g, kind=0, geometry=g, nodeBase=lay["geometryNodeBase"][g], nodes=count(gt[g]), slotBase=lay["geometrySlotBase"][g], slots=gt[g])
             for g in sorted(updated) if lay["needsBlas"][g]]
    touched = [i for i, g in enumerate(gi) if i in moved or g in updated]
    direct = [i for i in touched if lay["flattened"][i] and lay["directLeaf"][i]]
    for i in touched:
        if lay["flattened"][i] and not lay["directLeaf"][i]:
            trees.append(dict(tree=i, kind=1 if gi[i] in updated else 2, geometry=gi[i], nodeBase=lay["flatNodeBase"][i], nodes=count(gt[gi[i]]), slotBase=lay["flatSlotBase"][i], slots=gt[gi[i]]))
    out = {key: np.array([t[src] for t in trees], np.int64) for key, src in
           (("trees", "tree"), ("kinds", "kind"), ("nodeBases", "nodeBase"), ("nodeCounts", "nodes"), ("slotBases", "slotBase"), ("slotCounts", "slots"))}
    for key, counts in (("node", out["nodeCounts"]), ("slot", out["slotCounts"])):
        blocks = (counts + BLOCK - 1) // BLOCK
        out[key + "Offsets"] = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int64) if counts.size else np.zeros(0, np.int64)
        out[key + "BlockFirst"] = np.concatenate(([0], np.cumsum(blocks)[:-1])).astype(np.int64) if counts.size else np.zeros(0, np.int64)
        out[key + "BlockTable"] = np.array([(k, BLOCK * b) for k in range(counts.size) for b in range(int(blocks[k]))], np.int64).reshape(-1, 2)
    out.update(numTrees=len(trees), nodeBlocks=out["nodeBlockTable"].shape[0], slotBlocks=out["slotBlockTable"].shape[0], blockThreads=BLOCK,
               directLeaves=len(direct), boxes=sum(not lay["flattened"][i] for i in touched), topLevelRebuilt=int(not lay["single"]),
               nodes=int(out["nodeCounts"].sum()), slots=int(out["slotCounts"].sum()),
               slotsRewritten=int(out["slotCounts"].sum()) + sum(gt[gi[i]] for i in direct),
               slotBytes=sum(int(s) * SLOT_BYTES[int(k)] for s, k in zip(out["slotCounts"], out["kinds"])))
    out["directLeafInstances"] = direct
    out["boxInstances"] = [i for i in touched if not lay["flattened"][i]]
    out["treeList"] = trees
    return out


SCALARS = ("numTrees", "nodeBlocks", "slotBlocks", "blockThreads", "directLeaves", "boxes", "topLevelRebuilt", "nodes", "slots", "slotsRewritten", "slotBytes")
TABLES = ("trees", "kinds", "nodeBases", "nodeCounts", "slotBases", "slotCounts", "nodeOffsets", "slotOffsets", "nodeBlockFirst", "slotBlockFirst", "nodeBlockTable", "slotBlockTable")


def assert_plan(got, want, what):
    for key in SCALARS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in TABLES:
        assert np.array_equal(np.asarray(got[key], np.int64).reshape(want[key].shape), want[key]), (what, key, got[key], want[key])
