"""What tests/test_refit_host.py and tests/test_gpu_refit.py share: the meshes, the scenes, the deformations, and the plain-numpy side
of a tree's refit (the kept arrays a read-back does not hold, the quantised copy of refit wide nodes). A helper module, not a conftest.

Meshes: 1, 2, 3, 5, 64, 65, 257 and 1025 build primitives from bvh_audit_scenes (quads, soups, one odd mix with a quad that does not
pair and a trailing triangle). Scenes: "flat" — every mesh under one instance, flattened (the 1-quad and the 2-triangle mesh become
direct leaves of 2 triangles); "entered" — every mesh under two instances, so that it is entered and keeps a bottom-level tree. Every
transform is bvh_audit_scenes.place: a rotation with unequal scales."""
import functools

import numpy as np

import bvh_audit_scenes as M
import bvh_reference as R

F32 = np.float32
SIZES = ((1, "quads"), (2, "soup"), (3, "quads"), (5, "soup"), (64, "quads"), (65, "odd"), (257, "soup"), (1025, "quads"))
POLICY = (0, 1)  # a geometry with one reference is flattened, one with two is entered
KINDS = ("flat", "entered")
DEFORMATIONS = ("noise", "scale", "translate", "collapse")
INF = F32(np.inf)


@functools.lru_cache(maxsize=None)
def meshes():
    rng = np.random.default_rng(2028)
    return tuple(M.sized(n, kind, rng) for n, kind in SIZES)


def instances(kind):
    n = len(SIZES)
    return [(k, M.place(k)) for k in range(n)] + ([(k, M.place(n + k)) for k in range(n)] if kind == "entered" else [])


def deform(attributes, name, seed=0):
    """B of the built vertices A: seeded noise of at most 0.08 per coordinate (vertex_update_scenes.deformed's), a scale by 1.3, a
    translation by 1e4, every vertex on one point."""
    a = np.array(attributes, F32).reshape(-1, 12).copy()
    if name == "noise":
        a[:, 0:3] += np.random.default_rng(7 + seed).uniform(-0.08, 0.08, (a.shape[0], 3)).astype(F32)
    elif name == "scale":
        a[:, 0:3] *= F32(1.3)
    elif name == "translate":
        a[:, 0:3] += F32(1.0e4)
    elif name == "collapse":
        a[:, 0:3] = a[0, 0:3]
    else:
        raise KeyError(name)
    return a


def deformed_meshes(name):
    return [(deform(a, name, seed=k), i) for k, (a, i) in enumerate(meshes())]


def trees(geometries, scene_instances, policy):
    """Every tree of the scene that has nodes of its own: dicts with name, geometry, nodeBase, nodes, slotBase, slots, leafFlag,
    transform, instance, directLeaf."""
    gi = [g for g, _ in scene_instances]
    gt = [np.asarray(i).size // 3 for _, i in geometries]
    lay = R.scene_layout(gi, gt, policy)
    count = lambda n: n - 1 if n > 1 else 1
    out = []
    for g in range(len(gt)):
        if lay["needsBlas"][g]:
            out.append(dict(name=f"geometry {g}", geometry=g, nodeBase=lay["geometryNodeBase"][g], nodes=count(gt[g]), slotBase=lay["geometrySlotBase"][g], slots=gt[g],
                            leafFlag=0, transform=None, instance=-1, directLeaf=False))
    for i, (g, m) in enumerate(scene_instances):
        if lay["flattened"][i]:
            out.append(dict(name=f"instance {i}", geometry=g, nodeBase=lay["flatNodeBase"][i], nodes=count(gt[g]), slotBase=lay["flatSlotBase"][i], slots=gt[g],
                            leafFlag=R.LEAF_WORLD, transform=np.asarray(m, F32).reshape(12), instance=i, directLeaf=bool(lay["directLeaf"][i])))
    return out, lay


def pair_flags(indices, slots):
    """Per slot whether a pair begins there (BvhBuilder::buildTriangles' outPairFlags), from the slots' primitive words."""
    first, is_pair = R.build_primitives(indices)
    begins = np.zeros(np.asarray(indices).size // 3 + 1, bool)
    begins[first[is_pair]] = True
    return begins[slots.view(np.int32)[:, 3]].astype(np.int32)


def wide_of(nodes, base, count):
    """The full-precision wide nodes [count, 32] of the binary nodes [base, base + count) under the plain grandchildren cut, the one
    bvh_reference.emit quantises: (lo_k, ref_k) / (hi_k, -) as writeWideNode lays them out; an unused node stays zero."""
    words = nodes.view(np.int32)
    wide = np.zeros((count, 32), F32)
    for i in range(count):
        row, c = nodes[base + i], words[base + i, 12:14]
        if c[0] == 0 and c[1] == 0:
            continue
        entries = []
        for k in range(2):
            lo, hi, ref = row[6 * k:6 * k + 3], row[6 * k + 3:6 * k + 6], int(c[k])
            if lo[0] == INF and hi[0] == INF:
                continue
            if ref < 0:
                entries.append((lo, hi, ref))
            else:
                entries += [(nodes[ref, 6 * j:6 * j + 3], nodes[ref, 6 * j + 3:6 * j + 6], int(words[ref, 12 + j])) for j in range(2)]
        entries += [(np.full(3, INF), np.full(3, INF), -1)] * (4 - len(entries))
        w = wide[i].view(np.int32)
        for k, (lo, hi, ref) in enumerate(entries):
            wide[i, 8 * k:8 * k + 3], wide[i, 8 * k + 4:8 * k + 7] = lo, hi
            w[4 * k + 3] = ref
    return wide


def wide_entries(wide):
    """(lo, hi [n, 4, 3], refs [n, 4], valid [n, 4]) of full-precision wide nodes [n, 32]."""
    w = wide.reshape(-1, 32)
    lo = np.stack([w[:, 8 * k:8 * k + 3] for k in range(4)], 1)
    hi = np.stack([w[:, 8 * k + 4:8 * k + 7] for k in range(4)], 1)
    refs = np.stack([w.view(np.int32)[:, 4 * k + 3] for k in range(4)], 1)
    return lo, hi, refs, ~((lo[:, :, 0] == INF) & (hi[:, :, 0] == INF))


def half_area32(lo, hi):
    d = (hi - lo).astype(F32)
    return F32(F32(F32(d[0] * d[1]) + F32(d[1] * d[2])) + F32(d[2] * d[0]))


def node_costs(nodes, wide, base, count):
    """nodeCost [count] as refitKernel leaves it for the cuts `wide` holds: 1 + per child, in order, the sum over the inner entries it
    put into the wide node of min(area(entry) / area(node), 1) cost(entry), every operation in float32; 1 for a one-primitive tree."""
    words = nodes.view(np.int32)
    lo, hi, refs, valid = wide_entries(wide)
    cost = np.zeros(count, F32)
    order = [0]
    for i in order:
        order += [int(c) - base for c in words[base + i, 12:14] if c >= 0]
    # a node inside a collapsed subtree is written although nothing references it: two leaves, cost 1
    inside = [i for i in range(1, count) if i not in set(order) and words[base + i, 12:14].any()]
    assert all((words[base + i, 12:14] < 0).all() for i in inside)
    cost[inside] = 1.0
    for i in reversed(order):
        row, c = nodes[base + i], words[base + i, 12:14]
        if row[6] == INF and row[9] == INF:
            cost[i] = 1.0
            continue
        area = half_area32(np.minimum(row[0:3], row[6:9]), np.maximum(row[3:6], row[9:12]))
        scale = F32(1.0) / area if area > 0 else F32(0.0)
        child0 = [0, 1] if (c[0] >= 0 and refs[i, 0] != c[0]) else [0]
        first1 = len(child0)
        child1 = [first1, first1 + 1] if (c[1] >= 0 and refs[i, first1] != c[1]) else [first1]
        total = F32(1.0)
        for entries in (child0, child1):
            below = F32(0.0)
            for k in entries:
                if valid[i, k] and refs[i, k] >= 0:
                    below = F32(below + F32(min(F32(half_area32(lo[i, k], hi[i, k]) * scale), F32(1.0)) * cost[refs[i, k] - base]))
            total = F32(total + below)
        cost[i] = total
    return cost


def quantised(wide):
    """The quantised copy [n, 16] of full-precision wide nodes [n, 32] by bvh_reference.quantise, packed as bvh_reference.emit packs it;
    an all-zero (unused) node stays zero."""
    lo, hi, refs, valid = wide_entries(wide)
    unused = ~wide.reshape(-1, 32).view(np.uint32).any(1)
    valid = valid & ~unused[:, None]
    origin, cell, ql, qh = R.quantise(lo, hi, valid)
    q = np.zeros((lo.shape[0], 16), np.uint32)
    q[:, 0:3], q[:, 3:6] = origin.view(np.uint32), cell.view(np.uint32)
    for c in range(3):
        q[:, 6 + c] = sum(ql[:, k, c] << (8 * k) for k in range(4))
        q[:, 9 + c] = sum(qh[:, k, c] << (8 * k) for k in range(4))
    refs = np.where(valid, refs, refs[:, :1]).astype(np.int32)
    q[:, 12:16] = refs.view(np.uint32)
    q[unused] = 0
    return q.view(F32)
