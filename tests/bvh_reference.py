"""Plain numpy builders of the trees twk_build emits (the comments at the top of csrc/bvh_sah.hip), for
tests/bvh_audit.py: no GPU, no product code. A helper module, not a conftest.

  build_primitives  the pairing rule of bvh_build.h trianglePairs
  binned_sah        the SAH build, in float64 or float32
  median_split      object median on the longest centroid axis: the weaker builder the SAH build must beat
  emit              a whole scene in the formats the audit reads, so that the audit can be run and attacked on the CPU
  sah_terms         sahInnerCost / sahLeafCost of one tree as TwkBuildInfo defines them, in float64

A tree is topology over SORTED POSITIONS, as both device builders hand it to their shared refit: `order[p]` is the build
primitive at position p, inner node i covers positions first[i] .. first[i] + count[i] - 1 and has the children left[i],
right[i] — an inner node's index, or ~p for the single position p. Node 0 is the root; n primitives give n - 1 inner nodes."""
import numpy as np

BINS, SMALL, FORCE_LEVEL, MAX_LEAF = 16, 8, 40, 2
LEAF_WORLD, NODE_CACHED, SENTINEL = 0x40000000, 0x20000000, 0x7fffffff
TOP_NODES, TOP_NODES7 = 64, 32
F32, F64 = np.float32, np.float64


def build_primitives(indices):
    """(first triangle, is a pair) per build primitive: triangles 2k, 2k + 1 with the index triples (a, b, c), (c, d, a) are one
    primitive, every other triangle is one of its own. Indices are compared, not positions. (A pair can only begin at an even
    triangle and takes the odd one after it, so every even triangle is asked, whatever came before it.)"""
    idx = np.asarray(indices).reshape(-1, 3)
    n = idx.shape[0]
    k = np.arange(n // 2)
    pairs = (idx[2 * k + 1, 0] == idx[2 * k, 2]) & (idx[2 * k + 1, 2] == idx[2 * k, 0])
    second = np.zeros(n, bool)
    second[2 * k[pairs] + 1] = True
    first = np.nonzero(~second)[0]
    is_pair = np.zeros(n, bool)
    is_pair[2 * k[pairs]] = True
    return first.astype(np.int64), is_pair[first]


def half_area(lo, hi):
    d = hi - lo
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


class Tree:
    def __init__(self, n):
        self.order = np.arange(n)
        m = max(n - 1, 1)
        self.left, self.right = np.zeros(m, np.int64), np.zeros(m, np.int64)
        self.first, self.count = np.zeros(m, np.int64), np.zeros(m, np.int64)
        self.used = 1 if n > 1 else 0
        self.levels = []  # binned_sah: per level of the level loop (level, nodes, candidate planes of each, left count of each)

    def node(self, first, count):
        i = self.used
        self.used += 1
        self.first[i], self.count[i] = first, count
        return i


def _exact_sweep(tree, node, lo, hi, dtype):
    """Nodes of at most SMALL primitives: every split by an exact sweep over the three axes, the first strictly cheapest one."""
    stack = [node]
    while stack:
        i = stack.pop()
        first, count = int(tree.first[i]), int(tree.count[i])
        ids = tree.order[first:first + count].copy()
        blo, bhi = lo[ids], hi[ids]
        best, best_left, best_perm = np.inf, count // 2, np.arange(count)
        if count > 2:
            for axis in range(3):
                perm = np.argsort((blo[:, axis] + bhi[:, axis]).astype(dtype), kind="stable")
                slo, shi = blo[perm], bhi[perm]
                left_area = half_area(np.minimum.accumulate(slo, 0), np.maximum.accumulate(shi, 0))[:-1]
                right_area = half_area(np.minimum.accumulate(slo[::-1], 0), np.maximum.accumulate(shi[::-1], 0))[::-1][1:]
                k = np.arange(1, count).astype(dtype)
                cost = (left_area * k + right_area * (dtype(count) - k)).astype(dtype)
                j = int(np.argmin(cost))
                if cost[j] < best:
                    best, best_left, best_perm = cost[j], j + 1, perm
        tree.order[first:first + count] = ids[best_perm]
        refs = []
        for f, c in ((first, best_left), (first + best_left, count - best_left)):
            if c == 1:
                refs.append(~f)
            else:
                refs.append(tree.node(f, c))
                stack.append(refs[-1])
        tree.left[i], tree.right[i] = refs


def binned_sah(boxes, dtype=F64, force_level=FORCE_LEVEL):
    """Top-down binned SAH over boxes [n, 2, 3]: 16 bins per axis over the centroid bounds, cost area(L) n(L) + area(R) n(R) over the
    3 x 15 planes, the first strictly cheapest; a node no plane separates (and every node from level `force_level` on) is cut in the
    middle of its range; nodes of at most 8 primitives by the exact sweep. All arithmetic in `dtype`."""
    boxes = np.asarray(boxes, dtype)
    lo, hi = boxes[:, 0], boxes[:, 1]
    n = lo.shape[0]
    tree = Tree(n)
    if n < 2:
        return tree
    tree.first[0], tree.count[0] = 0, n
    centre = (dtype(0.5) * (lo + hi)).astype(dtype)
    level_nodes, small = ([0], []) if n > SMALL else ([], [0])
    level = 0
    while level_nodes:
        next_nodes, record = [], []
        for i in level_nodes:
            first, count = int(tree.first[i]), int(tree.count[i])
            ids = tree.order[first:first + count]
            c, blo, bhi = centre[ids], lo[ids], hi[ids]
            cmin, cmax = c.min(0), c.max(0)
            best, best_axis, best_bin, best_left, candidates, bins_of = np.inf, -1, 0, count // 2, 0, None
            if level < force_level:
                for axis in range(3):
                    extent = dtype(cmax[axis] - cmin[axis])
                    if extent > 0:
                        b = np.clip(((c[:, axis] - cmin[axis]).astype(dtype) * dtype(dtype(BINS) / extent)).astype(dtype).astype(np.int64), 0, BINS - 1)
                    else:
                        b = np.zeros(count, np.int64)
                    bin_lo, bin_hi = np.full((BINS, 3), np.inf, dtype), np.full((BINS, 3), -np.inf, dtype)
                    np.minimum.at(bin_lo, b, blo)
                    np.maximum.at(bin_hi, b, bhi)
                    counts = np.bincount(b, minlength=BINS)
                    n_left, n_right = np.cumsum(counts)[:-1], np.cumsum(counts[::-1])[::-1][1:]
                    ok = (n_left > 0) & (n_right > 0)
                    if not ok.any():
                        continue
                    with np.errstate(invalid="ignore", over="ignore"):
                        a_left = half_area(np.minimum.accumulate(bin_lo, 0), np.maximum.accumulate(bin_hi, 0))[:-1]
                        a_right = half_area(np.minimum.accumulate(bin_lo[::-1], 0), np.maximum.accumulate(bin_hi[::-1], 0))[::-1][1:]
                        cost = np.where(ok, (a_left * n_left.astype(dtype) + a_right * n_right.astype(dtype)).astype(dtype), np.inf)
                    candidates += len(set(n_left[ok]))
                    tree.areas_finite = getattr(tree, "areas_finite", True) and bool(np.isfinite(a_left[ok]).all() and np.isfinite(a_right[ok]).all())
                    j = int(np.argmin(cost))
                    if cost[j] < best:
                        best, best_axis, best_bin, best_left, bins_of = cost[j], axis, j + 1, int(n_left[j]), b
            if best_axis >= 0:
                go_left = bins_of < best_bin
                tree.order[first:first + count] = np.concatenate([ids[go_left], ids[~go_left]])  # stable
            record.append((candidates, best_left if best_axis >= 0 else -best_left))
            refs = []
            for f, k in ((first, best_left), (first + best_left, count - best_left)):
                if k == 1:
                    refs.append(~f)
                    continue
                refs.append(tree.node(f, k))
                (small if k <= SMALL else next_nodes).append(refs[-1])
            tree.left[i], tree.right[i] = refs
        tree.levels.append(record)
        level_nodes = next_nodes
        level += 1
    for i in small:
        _exact_sweep(tree, i, lo, hi, dtype)
    return tree


def median_split(boxes):
    """Object median on the longest axis of the centroid bounds, down to single primitives, in float64."""
    boxes = np.asarray(boxes, F64)
    lo, hi = boxes[:, 0], boxes[:, 1]
    n = lo.shape[0]
    tree = Tree(n)
    if n < 2:
        return tree
    tree.first[0], tree.count[0] = 0, n
    centre = 0.5 * (lo + hi)
    stack = [0]
    while stack:
        i = stack.pop()
        first, count = int(tree.first[i]), int(tree.count[i])
        ids = tree.order[first:first + count]
        c = centre[ids]
        axis = int(np.argmax(c.max(0) - c.min(0)))
        tree.order[first:first + count] = ids[np.argsort(c[:, axis], kind="stable")]
        refs = []
        for f, k in ((first, count // 2), (first + count // 2, count - count // 2)):
            if k == 1:
                refs.append(~f)
            else:
                refs.append(tree.node(f, k))
                stack.append(refs[-1])
        tree.left[i], tree.right[i] = refs
    return tree


def height(tree, triangles_of):
    """Inner nodes on the longest root-to-leaf path after the leaf collapse (a tree over one primitive: its one node)."""
    n = tree.order.size
    if n < 2:
        return 1
    offsets = np.concatenate([[0], np.cumsum(triangles_of[tree.order])])
    frontier, levels = np.array([0]), 0
    while frontier.size:
        levels += 1
        refs = np.concatenate([tree.left[frontier], tree.right[frontier]])
        refs = refs[refs >= 0]
        keep = ~((tree.count[refs] <= MAX_LEAF) & (offsets[tree.first[refs] + tree.count[refs]] - offsets[tree.first[refs]] <= MAX_LEAF))
        frontier = refs[keep]
    return levels


def pad_box(lo, hi):
    """padBox of csrc/bvh_build.hip in float32: every primitive box grows on all axes by 2^-17 (largest coordinate magnitude + diagonal)
    + 1e-30."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    with np.errstate(over="ignore"):
        m = np.maximum(np.abs(lo), np.abs(hi)).max(-1)
        d = hi - lo
        e = F32(2.0 ** -17) * (m + np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2], dtype=F32)) + F32(1.0e-30)
    e = e.astype(F32)[..., None]
    return (lo - e).astype(F32), (hi + e).astype(F32)


def sah_terms(tree, boxes, triangles_of):
    """(sahInnerCost, sahLeafCost) of one tree in float64: half-area(node) / half-area(root) over the inner nodes that survive the leaf
    collapse, half-area(leaf) / half-area(root) x triangles over the leaves. Node boxes are unions of the PADDED primitive boxes; a leaf of
    one build primitive right below an inner node counts with its unpadded box, a collapsed subtree with its node box (sahCostKernel).
    A tree over one build primitive has no terms."""
    n = tree.order.size
    if n < 2:
        return 0.0, 0.0
    boxes = np.asarray(boxes, F32)
    plo, phi = pad_box(boxes[:, 0], boxes[:, 1])
    nlo, nhi = _node_boxes(tree, plo, phi)
    offsets = np.concatenate([[0], np.cumsum(triangles_of[tree.order])])
    tris = lambda f, c: offsets[f + c] - offsets[f]
    root = float(half_area(nlo[0].astype(F64), nhi[0].astype(F64)))
    inner = leaf = 0.0
    frontier = np.array([0])
    while frontier.size:
        inner += float(half_area(nlo[frontier].astype(F64), nhi[frontier].astype(F64)).sum()) / root
        refs = np.concatenate([tree.left[frontier], tree.right[frontier]])
        single = ~refs[refs < 0]
        prim = tree.order[single]
        leaf += float((half_area(boxes[prim, 0].astype(F64), boxes[prim, 1].astype(F64)) * tris(single, 1)).sum()) / root
        refs = refs[refs >= 0]
        collapsed = (tree.count[refs] <= MAX_LEAF) & (tris(tree.first[refs], tree.count[refs]) <= MAX_LEAF)
        c = refs[collapsed]
        leaf += float((half_area(nlo[c].astype(F64), nhi[c].astype(F64)) * tris(tree.first[c], tree.count[c])).sum()) / root
        frontier = refs[~collapsed]
    return inner, leaf


def _node_boxes(tree, plo, phi):
    """Box of every inner node: the union of the (padded) boxes of the primitives in its range."""
    m = tree.left.size
    nlo, nhi = np.zeros((m, 3), F32), np.zeros((m, 3), F32)
    slo, shi = plo[tree.order], phi[tree.order]
    for i in range(m):
        f, c = int(tree.first[i]), int(tree.count[i])
        nlo[i], nhi[i] = slo[f:f + c].min(0), shi[f:f + c].max(0)
    return nlo, nhi


# ---------------------------------------------------------------------------------------------------------------------------------
# emit: a scene in the formats the audit reads

def scene_layout(instance_geometry, geometry_triangles, policy):
    """Where every tree of a scene stands (csrc/update_plan.h sceneLayout, restated): which instances are flattened, which are leaves of
    the top level themselves, and the node and slot bases of the bottom-level trees, the world-space trees and the top level."""
    gi, gt = list(instance_geometry), list(geometry_triangles)
    refs = [gi.count(g) for g in range(len(gt))]
    tree_nodes = lambda n: n - 1 if n > 1 else 1
    out = {"flattened": [gt[g] <= policy[0] or refs[g] <= policy[1] for g in gi]}
    out["directLeaf"] = [f and gt[g] <= MAX_LEAF for f, g in zip(out["flattened"], gi)]
    out["needsBlas"] = [any(g == k and not f for g, f in zip(gi, out["flattened"])) for k in range(len(gt))]
    nodes = slots = 0
    out["geometryNodeBase"], out["geometrySlotBase"] = [], []
    for k, n in enumerate(gt):
        out["geometryNodeBase"].append(nodes)
        out["geometrySlotBase"].append(slots)
        if out["needsBlas"][k]:
            nodes, slots = nodes + tree_nodes(n), slots + n
    out["flatNodeBase"], out["flatSlotBase"] = [], []
    for f, g in zip(out["flattened"], gi):
        out["flatNodeBase"].append(nodes if f else -1)
        out["flatSlotBase"].append(slots if f else -1)
        if f:
            nodes, slots = nodes + tree_nodes(gt[g]), slots + gt[g]
    out["tlasBase"], out["nodes"], out["slots"] = nodes, nodes + tree_nodes(len(gi)), slots
    out["single"] = len(gi) == 1 and out["flattened"][0]
    out["entered"] = sum(not f for f in out["flattened"])
    return out


def transform_f32(m, points):
    """m0 x + m1 y + m2 z + m3 per row of the 3 x 4 matrix, every operation rounded to float32, left to right."""
    m, p = np.asarray(m, F32).reshape(3, 4), np.asarray(points, F32)
    out = np.zeros(p.shape, F32)
    for r in range(3):
        out[..., r] = ((m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]).astype(F32) + m[r, 2] * p[..., 2]).astype(F32) + m[r, 3]
    return out


def shade_records(attributes, tri_indices):
    """The 128-byte shading records of triangles given as index triples [n, 3] into attributes [v, 12] (position, tangent, normal,
    texcoord): geometric normal cross(v1 - v0, v2 - v0), the three normals, the three tangents, the three texcoords."""
    a, b, c = (np.asarray(attributes, F32)[tri_indices[:, k]] for k in range(3))
    e1, e2 = (b[:, 0:3] - a[:, 0:3]).astype(F32), (c[:, 0:3] - a[:, 0:3]).astype(F32)
    ng = np.stack([(e1[:, 1] * e2[:, 2]).astype(F32) - (e1[:, 2] * e2[:, 1]).astype(F32), (e1[:, 2] * e2[:, 0]).astype(F32) - (e1[:, 0] * e2[:, 2]).astype(F32),
                   (e1[:, 0] * e2[:, 1]).astype(F32) - (e1[:, 1] * e2[:, 0]).astype(F32)], 1).astype(F32)
    zero = np.zeros((a.shape[0], 2), F32)
    return np.concatenate([ng, a[:, 6:9], b[:, 6:9], c[:, 6:9], a[:, 3:6], b[:, 3:6], c[:, 3:6], a[:, 9:12], b[:, 9:12], c[:, 9:12], zero], 1)


def quantise(lo, hi, valid):
    """Conservative quantisation of wide nodes [n, 4, 3] -> (origin [n, 3], cell [n, 3], qlo, qhi [n, 4, 3] uint): the smallest power of
    two with extent / cell < 254 (exponent kept in -125 .. 126), lo planes down, hi planes up, each checked against the float32
    expression origin + q cell."""
    big = np.where(valid[:, :, None], lo, np.inf).min(1)
    origin = np.where(np.isfinite(big), big, 0.0).astype(F32)
    top = np.where(valid[:, :, None], hi, -np.inf).max(1)
    extent = np.maximum(np.where(np.isfinite(top), top, 0.0).astype(F32) - origin, F32(0.0)).astype(F32)
    _, e = np.frexp((extent * F32(1.0 / 254.0)).astype(F32))
    e = np.where(extent > 0, np.clip(e, -125, 126), -125)
    cell = np.ldexp(F32(1.0), e).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        ql = np.clip(np.floor(((lo - origin[:, None]).astype(F32) / cell[:, None]).astype(F32)), 0, 255)
        qh = np.clip(np.ceil(((hi - origin[:, None]).astype(F32) / cell[:, None]).astype(F32)), 0, 255)
        ql, qh = np.nan_to_num(ql).astype(np.int64), np.nan_to_num(qh).astype(np.int64)
        plane = lambda q: (q.astype(F64) * cell[:, None].astype(F64) + origin[:, None].astype(F64)).astype(F32)
        ql -= ((ql > 0) & (plane(ql) > lo)).astype(np.int64)
        qh += ((qh < 255) & (plane(qh) < hi)).astype(np.int64)
    ql, qh = np.where(valid[:, :, None], ql, 255), np.where(valid[:, :, None], qh, 0)
    return origin, cell, ql.astype(np.uint32), qh.astype(np.uint32)


def top_cache(wide_q, root, root2, slots):
    """The first `slots` quantised wide nodes in breadth-first order from root (root2 second), references among them rewritten to
    NODE_CACHED | slot; slots never reached are zero."""
    words = wide_q.view(np.uint32)
    queue = [root] + ([root2] if root2 not in (SENTINEL, -1) else [])
    i = 0
    while i < len(queue):
        w = words[queue[i]]
        for k in range(4):
            unused = ((w[6] >> (8 * k)) & 0xff) > ((w[9] >> (8 * k)) & 0xff)
            r = int(w[12 + k].view(np.int32))
            if not unused and r >= 0 and r != SENTINEL and len(queue) < slots:
                queue.append(r)
        i += 1
    out = np.zeros((slots, 16), np.uint32)
    for s, node in enumerate(queue):
        out[s] = words[node]
        for k in range(4):
            r = int(out[s, 12 + k].view(np.int32))
            if r >= 0 and r != SENTINEL and r in queue:
                out[s, 12 + k] = NODE_CACHED | queue.index(r)
    return out.view(F32)


def _emit_tree(tree, plo, phi, leaf_ref, child_ref, nodes, wide, node_base):
    """Binary nodes and plain grandchildren wide nodes of one tree. plo / phi: padded primitive boxes; leaf_ref(position) the
    reference of a single position, child_ref(i) the reference of inner node i (a collapsed leaf's, or node_base + i)."""
    n = tree.order.size
    inf3 = np.full(3, np.inf, F32)
    if n == 1:
        ref = leaf_ref(0)
        nodes[node_base, 0:3], nodes[node_base, 3:6], nodes[node_base, 6:9], nodes[node_base, 9:12] = plo[tree.order[0]], phi[tree.order[0]], inf3, inf3
        nodes[node_base, 12:14] = np.array([ref, -1], np.int32).view(F32)
        wide[node_base] = [(plo[tree.order[0]], phi[tree.order[0]], ref)]
        return
    nlo, nhi = _node_boxes(tree, plo, phi)
    entry = {}
    for i in range(n - 1):
        sides = []
        for r in (int(tree.left[i]), int(tree.right[i])):
            if r < 0:
                sides.append((plo[tree.order[~r]], phi[tree.order[~r]], leaf_ref(~r)))
            else:
                sides.append((nlo[r], nhi[r], child_ref(r)))
        entry[i] = sides
        row = nodes[node_base + i]
        row[0:3], row[3:6], row[6:9], row[9:12] = sides[0][0], sides[0][1], sides[1][0], sides[1][1]
        row[12:14] = np.array([sides[0][2], sides[1][2]], np.int32).view(F32)
    for i, sides in entry.items():
        cut = []
        for lo, hi, ref in sides:
            # an inner child gives way to its own two children; the root of a spliced tree is an inner child like any other
            cut += [(lo, hi, ref)] if ref < 0 else (entry[ref - node_base] if node_base <= ref < node_base + n - 1 else _children(nodes, ref))
        wide[node_base + i] = cut


def emit(geometries, instances, policy, builder):
    """The scene (geometries [(attributes [v, 12], indices)], instances [(geometry, transform[12])], flatten policy) built with
    `builder(boxes) -> Tree` and written as bvh_audit.Readback reads a handle. Wide nodes are the plain grandchildren cut, there is no
    8-wide root, the top-of-tree caches are on."""
    from bvh_audit import Readback
    geo = [(np.asarray(a, F32).reshape(-1, 12), np.asarray(i, np.uint32).reshape(-1, 3)) for a, i in geometries]
    gi = [g for g, _ in instances]
    gt = [idx.shape[0] for _, idx in geo]
    lay = scene_layout(gi, gt, policy)
    nodes = np.zeros((lay["nodes"], 16), F32)
    slots, shade = np.zeros((lay["slots"], 12), F32), np.zeros((lay["slots"], 32), F32)
    wide, pair_flags = {}, np.zeros(lay["slots"], bool)
    terms, heights, root_box, pair_leaves, trees = [], {}, {}, 0, 0
    prims = [build_primitives(idx) for _, idx in geo]

    def tree_of(key, g, node_base, slot_base, transform, instance):
        nonlocal pair_leaves, trees
        attrs, idx = geo[g]
        first, is_pair = prims[g]
        triangles_of = np.where(is_pair, 2, 1)
        pos = attrs[idx, 0:3] if transform is None else transform_f32(transform, attrs[idx, 0:3])  # [t, 3, 3]
        tlo, thi = pos.min(1), pos.max(1)
        lo = np.where(is_pair[:, None], np.minimum(tlo[first], tlo[np.minimum(first + 1, gt[g] - 1)]), tlo[first])
        hi = np.where(is_pair[:, None], np.maximum(thi[first], thi[np.minimum(first + 1, gt[g] - 1)]), thi[first])
        boxes = np.stack([lo, hi], 1)
        tree = builder(boxes)
        plo, phi = pad_box(lo, hi)
        offsets = np.concatenate([[0], np.cumsum(triangles_of[tree.order])])
        flag = 0 if transform is None else LEAF_WORLD
        leaf = lambda f, c: ~int((slot_base + offsets[f]) | ((offsets[f + c] - offsets[f] - 1) << 28) | flag)
        collapsed = lambda i: tree.count[i] <= MAX_LEAF and offsets[tree.first[i] + tree.count[i]] - offsets[tree.first[i]] <= MAX_LEAF
        _emit_tree(tree, plo, phi, lambda p: leaf(p, 1), lambda i: leaf(tree.first[i], tree.count[i]) if collapsed(i) else node_base + i,
                   nodes, wide, node_base)
        for p, b in enumerate(tree.order):
            for k in range(triangles_of[b]):
                t, s = first[b] + k, slot_base + offsets[p] + k
                slots[s, 0:3], slots[s, 4:7], slots[s, 8:11] = pos[t]
                slots[s, 3] = np.array([t], np.int32).view(F32)[0]
                if transform is not None:
                    slots[s, 7] = np.array([instance], np.int32).view(F32)[0]
                shade[s] = shade_records(attrs, idx[t:t + 1])[0]
            pair_flags[slot_base + offsets[p]] = is_pair[b]
        terms.append(sah_terms(tree, boxes, triangles_of))
        heights[key] = height(tree, triangles_of)
        if tree.order.size == 1:
            root_box[key] = (plo[0], phi[0])
        else:
            root_box[key] = (np.minimum(nodes[node_base, 0:3], nodes[node_base, 6:9]), np.maximum(nodes[node_base, 3:6], nodes[node_base, 9:12]))
        pair_leaves += int(is_pair.sum())
        trees += 1

    for g in range(len(geo)):
        if lay["needsBlas"][g]:
            tree_of(("g", g), g, lay["geometryNodeBase"][g], lay["geometrySlotBase"][g], None, -1)
    records = np.zeros((len(instances), 32), F32)
    top_boxes, payload = np.zeros((len(instances), 2, 3), F32), []
    for i, (g, m) in enumerate(instances):
        m = np.asarray(m, F32).reshape(12)
        records[i, 16:28] = m
        m4 = np.vstack([m.reshape(3, 4).astype(F64), [0, 0, 0, 1]])
        records[i, 0:12] = np.linalg.inv(m4)[:3].reshape(12).astype(F32)
        rec = records[i].view(np.int32)
        rec[12] = lay["flatNodeBase"][i] if lay["flattened"][i] else lay["geometryNodeBase"][g]
        rec[13] = lay["flatSlotBase"][i] if lay["flattened"][i] else lay["geometrySlotBase"][g]
        rec[14], rec[15], rec[28], rec[29] = gt[g], g, 0, -1
        if lay["flattened"][i]:
            tree_of(("i", i), g, lay["flatNodeBase"][i], lay["flatSlotBase"][i], m, i)
            top_boxes[i] = root_box[("i", i)]
            payload.append(int(lay["flatSlotBase"][i] | ((gt[g] - 1) << 28) | LEAF_WORLD) if lay["directLeaf"][i] else ~lay["flatNodeBase"][i])
        else:
            # the float64 image of the root box's corners, padded by 1e-5 max(1, |coordinate|): what the host code of the build adds
            lo, hi = (v.astype(F64) for v in root_box[("g", g)])
            corners = np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])
            w = corners @ m.reshape(3, 4)[:, :3].astype(F64).T + m.reshape(3, 4)[:, 3].astype(F64)
            wlo, whi = w.min(0), w.max(0)
            e = 1.0e-5 * np.maximum(1.0, np.maximum(np.abs(wlo), np.abs(whi)))
            top_boxes[i] = (np.nextafter((wlo - e).astype(F32), F32(-np.inf)), np.nextafter((whi + e).astype(F32), F32(np.inf)))
            payload.append(i)
    top_height = 0
    root = lay["flatNodeBase"][0] if lay["single"] else lay["tlasBase"]
    if not lay["single"]:
        top = builder(top_boxes)
        # leafMode 1: no padding of an instance's box beyond padBox, no collapse, the payload decides the reference
        plo, phi = pad_box(top_boxes[:, 0], top_boxes[:, 1])
        _emit_tree(top, plo, phi, lambda p: ~payload[top.order[p]], lambda i: lay["tlasBase"] + i, nodes, wide, lay["tlasBase"])
        top_height = height(top, np.full(len(instances), MAX_LEAF + 1, np.int64))  # nothing collapses at the top level
    num_wide = lay["nodes"] + 0
    wlo, whi = np.full((num_wide, 4, 3), np.inf, F32), np.full((num_wide, 4, 3), np.inf, F32)
    refs, valid = np.full((num_wide, 4), -1, np.int32), np.zeros((num_wide, 4), bool)
    for i, cut in wide.items():
        for k, (lo, hi, ref) in enumerate(cut):
            wlo[i, k], whi[i, k], refs[i, k], valid[i, k] = lo, hi, ref, True
        refs[i, len(cut):] = cut[0][2]
    origin, cell, ql, qh = quantise(wlo, whi, valid)
    q = np.zeros((num_wide, 16), np.uint32)
    q[:, 0:3], q[:, 3:6] = origin.view(np.uint32), cell.view(np.uint32)
    for c in range(3):
        q[:, 6 + c] = sum(ql[:, k, c] << (8 * k) for k in range(4))
        q[:, 9 + c] = sum(qh[:, k, c] << (8 * k) for k in range(4))
    q[:, 12:16] = refs.view(np.uint32)
    unbuilt = ~valid.any(1)
    q[unbuilt] = 0
    canonical = q.copy().view(F32)
    # pair leaves: in a scene whose instances are all flattened the persistent kernel's structures name them without LEAF_WORLD
    pairs = None
    if lay["entered"] == 0 and pair_leaves > 0:
        pairs = np.zeros((lay["slots"] // 2 + 1, 16), F32)
        r = q[:, 12:16].view(np.int32)
        payloads = ~r
        first = payloads & 0x0fffffff
        is_pair_leaf = (r < 0) & ((payloads & LEAF_WORLD) != 0) & (((payloads >> 28) & 3) == 1) & pair_flags[np.minimum(first, lay["slots"] - 1)] & ~unbuilt[:, None]
        r[is_pair_leaf] = ~(payloads[is_pair_leaf] & ~LEAF_WORLD)
        for s in np.unique(first[is_pair_leaf]):
            rec = pairs[s >> 1]
            rec[0:4], rec[4:7], rec[7], rec[8:11], rec[11], rec[12:15] = slots[s, 0:4], slots[s, 4:7], slots[s + 1, 3], slots[s, 8:11], slots[s, 7], slots[s + 1, 4:7]
            rec[15] = np.array([s], np.int32).view(F32)[0]
    raw = q.view(F32)
    sah_inner, sah_leaf = sum(t[0] for t in terms), sum(t[1] for t in terms)
    flat_h = max([heights[("i", i)] for i in range(len(instances)) if lay["flattened"][i]], default=0)
    ent_h = max([heights[("g", g)] for g in range(len(geo)) if lay["needsBlas"][g]], default=0)
    build = {"quality": 1, "trees": trees, "sahInnerCost": sah_inner, "sahLeafCost": sah_leaf, "triangleSlots": lay["slots"], "nodes": lay["nodes"],
             "instances": len(instances), "flattenedInstances": len(instances) - lay["entered"], "directLeafInstances": sum(lay["directLeaf"]),
             "maxTraversalDepth": top_height + max(flat_h, 1 + ent_h if lay["entered"] else 0), "pairLeaves": pair_leaves, "pairTriangles": 2 * pair_leaves}
    info = {"root": root, "root2": -1, "twoLevel": int(lay["entered"] > 0), "numNodes": num_wide, "numTriangleSlots": lay["slots"], "numInstances": len(instances)}
    return Readback(nodes=nodes, wideQ=canonical, slots=slots, shade=shade, instances=records, topNodes=top_cache(raw, root, -1, TOP_NODES),
                    topNodes7=top_cache(raw, root, -1, TOP_NODES7), topRoot=NODE_CACHED | 0, topRoot2=SENTINEL, pairs=pairs, info=info, build=build)


def _children(nodes, ref):
    row = nodes[ref]
    r = row[12:14].view(np.int32)
    return [(row[0:3].copy(), row[3:6].copy(), int(r[0])), (row[6:9].copy(), row[9:12].copy(), int(r[1]))]
