"""The audit of everything twk_build emits, in float64 on the host: pure numpy, no GPU, no product code. A helper module, not a
conftest. `audit(scene, readback)` takes what the scene was fed (Scene) and what the handle hands out (Readback: tests/scene_snapshot.py
reads one from a handle, bvh_reference.emit writes one from a reference tree) and raises an AuditError that names the check, the tree
and the node at the first thing that is not as csrc/device_types.h, csrc/bvh_build.hip and DESIGN.md 4.4 say. It returns what it
measured (per tree: SAH terms, height), for the checks that compare trees with each other.

Trees are walked level by level with arrays. The checks, in the order they run per tree:
  partition          the leaves reachable through the binary nodes tile the tree's slot range in ascending runs
  leaf-size          of 1 or 2 slots
  triangles-once     the slots hold every triangle of the geometry exactly once (.w of the first vertex), world slots their instance
  vertices           object-space slots equal the input bit for bit, world-space slots the float64 transform within its rounding
  pair-leaf / pair-split / pair-record   a leaf is a pair leaf exactly when bvh_reference.build_primitives says so; halves stay together
  leaf-contains      a leaf's box contains every vertex below it (exact)
  pad-present / pad-once   it contains the tight box grown by 0.999 e and lies inside the one grown by 1.001 e (padBox's e)
  inner-union        an inner child's box is the union of that child's two child boxes, bit for bit
  wide-cut / wide-unused    the quantised wide node of inner node i holds the child, or the child's two children, per child
  cell-size / origin / quantised-contains / quantised-tight     the quantisation, in both directions
then per scene: top-level (boxes, references), reachability, cache-order / cache-references / top-root, height, sah-terms, counts,
pair-counts, shading."""
import numpy as np

from bvh_reference import LEAF_WORLD, MAX_LEAF, NODE_CACHED, SENTINEL, TOP_NODES, TOP_NODES7, build_primitives, half_area, scene_layout

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of float32


class AuditError(AssertionError):
    def __init__(self, check, tree, node, detail=""):
        super().__init__(f"{check}: tree {tree}, node {node}: {detail}")
        self.check, self.tree, self.node = check, tree, node


class Scene:
    """What the scene was fed: geometries [(attributes [v, 12], indices)], instances [(geometry, transform[12])], the flatten policy,
    the build quality, and whether the top-of-tree caches are on."""
    def __init__(self, geometries, instances, policy, quality=1, top_cache=True):
        self.geometries = [(np.asarray(a, F32).reshape(-1, 12), np.asarray(i, np.uint32).reshape(-1, 3)) for a, i in geometries]
        self.instances = [(int(g), np.asarray(m, F32).reshape(12)) for g, m in instances]
        self.policy, self.quality, self.top_cache = tuple(policy), quality, top_cache


class Readback:
    """What a handle hands out: binary nodes [n, 16], quantised wide nodes [n (+ 2), 16] as twk_debug_read_acceleration shows them (a
    pair leaf's reference with TWK_LEAF_WORLD), slots [t, 12], shading records [t, 32], instance records [i, 32], the two top-of-tree
    caches, topRoot / topRoot2, the pair records [t / 2 + 1, 16] or None where the handle gives none out, TwkAccelerationInfo and
    TwkBuildInfo as dicts. All float32 arrays; integer words are read through views."""
    def __init__(self, **kw):
        for k in ("nodes", "wideQ", "slots", "shade", "instances", "topNodes", "topNodes7"):
            setattr(self, k, np.ascontiguousarray(kw[k], F32))
        self.topRoot, self.topRoot2, self.pairs, self.info, self.build = kw["topRoot"], kw["topRoot2"], kw.get("pairs"), dict(kw["info"]), dict(kw["build"])

    def copy(self):
        return Readback(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})


def _fail(cond, check, tree, nodes, detail):
    """Raises at the first element of `cond` that is set."""
    cond = np.atleast_1d(cond)
    if cond.any():
        k = int(np.argmax(cond))
        nodes = np.atleast_1d(nodes)
        raise AuditError(check, tree, int(nodes[min(k, nodes.size - 1)]), detail(k) if callable(detail) else detail)


def walk(nodes, root, first, count):
    """Every (node, side) below `root` that stays inside the node range [first, first + count): arrays parent, side, ref, lo, hi, level.
    A child whose box is (+inf, +inf) is the never-hit second child of a one-primitive tree and is left out."""
    words = nodes.view(np.int32)
    frontier, out, level, seen = np.array([root], np.int64), [], 0, 0
    while frontier.size:
        seen += frontier.size
        if seen > count or level > 4096:
            raise AuditError("partition", root, int(frontier[0]), "the binary nodes do not form a tree (a node is reached twice)")
        ref = words[frontier][:, 12:14].reshape(-1).astype(np.int64)
        lo = np.stack([nodes[frontier, 0:3], nodes[frontier, 6:9]], 1).reshape(-1, 3)
        hi = np.stack([nodes[frontier, 3:6], nodes[frontier, 9:12]], 1).reshape(-1, 3)
        parent, side = np.repeat(frontier, 2), np.tile([0, 1], frontier.size)
        keep = ~((lo[:, 0] == np.inf) & (hi[:, 0] == np.inf))
        out.append((parent[keep], side[keep], ref[keep], lo[keep], hi[keep], np.full(int(keep.sum()), level)))
        inner = keep & (ref >= 0) & (ref >= first) & (ref < first + count)
        frontier = ref[inner]
        level += 1
    return tuple(np.concatenate([o[k] for o in out]) for k in range(6)) + (level,)


def child_boxes_union(nodes, ref):
    """Union of the two child boxes of the inner nodes `ref` (a one-primitive tree's node: its first child)."""
    lo1 = np.where(nodes[ref, 6:9] == np.inf, nodes[ref, 0:3], nodes[ref, 6:9])
    hi1 = np.where(nodes[ref, 9:12] == np.inf, nodes[ref, 3:6], nodes[ref, 9:12])
    return np.minimum(nodes[ref, 0:3], lo1), np.maximum(nodes[ref, 3:6], hi1)


def decode(wide_q):
    """(lo, hi [n, 4, 3] float32 as the kernel evaluates origin + q cell, refs [n, 4], valid [n, 4], origin, cell, qlo, qhi)."""
    w = wide_q.view(np.uint32)
    origin, cell = wide_q[:, 0:3], wide_q[:, 3:6]
    shifts = np.array([0, 8, 16, 24], np.uint32)
    ql = ((w[:, 6:9, None] >> shifts) & 0xff).transpose(0, 2, 1)
    qh = ((w[:, 9:12, None] >> shifts) & 0xff).transpose(0, 2, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        # q cell is exact (a power of two times at most 255), so the fused multiply-add of the kernel rounds once, like this sum
        lo = (ql.astype(F64) * cell[:, None].astype(F64) + origin[:, None].astype(F64)).astype(F32)
        hi = (qh.astype(F64) * cell[:, None].astype(F64) + origin[:, None].astype(F64)).astype(F32)
    return lo, hi, wide_q.view(np.int32)[:, 12:16].astype(np.int64), ql[:, :, 0] <= qh[:, :, 0], origin, cell, ql, qh


def tight_boxes(pos, group_first, group_size):
    """Per slot, the tight float box of its BUILD PRIMITIVE: pos [t, 3, 3]; a pair's two slots share the box of both triangles."""
    lo, hi = pos.min(1), pos.max(1)
    second = np.zeros(pos.shape[0], bool)
    second[group_first[group_size == 2] + 1] = True
    first = np.zeros(pos.shape[0], bool)
    first[group_first[group_size == 2]] = True
    out_lo, out_hi = lo.copy(), hi.copy()
    nxt, prv = np.roll(lo, -1, 0), np.roll(lo, 1, 0)
    out_lo[first], out_lo[second] = np.minimum(lo, nxt)[first], np.minimum(lo, prv)[second]
    nxt, prv = np.roll(hi, -1, 0), np.roll(hi, 1, 0)
    out_hi[first], out_hi[second] = np.maximum(hi, nxt)[first], np.maximum(hi, prv)[second]
    return out_lo, out_hi


def pad_window(lo, hi):
    """The float32 values a padded box may take: padBox grows a primitive's box by e = 2^-17 (m + diagonal) + 1e-30, m the largest
    coordinate magnitude, computed in float32 with six roundings (below 2^-20 relative together), and then subtracts / adds e with ONE
    rounding to nearest. Rounding is monotone, so the result lies between the float32 roundings of the exact values for 0.999 e and
    1.001 e: (lo for 1.001 e, lo for 0.999 e, hi for 0.999 e, hi for 1.001 e)."""
    lo, hi = lo.astype(F64), hi.astype(F64)
    m = np.maximum(np.abs(lo), np.abs(hi)).max(-1)
    e = (2.0 ** -17 * (m + np.sqrt(((hi - lo) ** 2).sum(-1))) + 1.0e-30)[:, None]
    with np.errstate(over="ignore"):
        return (lo - 1.001 * e).astype(F32), (lo - 0.999 * e).astype(F32), (hi + 0.999 * e).astype(F32), (hi + 1.001 * e).astype(F32)


def _runs(values, first, count):
    """min / max of values over the runs [first, first + count), count 1 or 2."""
    second = first + count - 1
    return np.minimum(values[first], values[second]), np.maximum(values[first], values[second])


def audit_tree(name, scene, rb, geometry, root, node_first, node_count, slot_first, transform, instance):
    """One bottom-level tree (transform None) or the world-space tree of a flattened instance. Returns its measurements."""
    attrs, idx = scene.geometries[geometry]
    nt = idx.shape[0]
    nodes, slots = rb.nodes, rb.slots
    parent, side, ref, lo, hi, level, levels = walk(nodes, root, node_first, node_count)
    flag = 0 if transform is None else LEAF_WORLD
    # partition
    _fail((ref >= 0) & ((ref < node_first) | (ref >= node_first + node_count)), "partition", name, parent, "an inner reference leaves the tree's node range")
    leaf = ref < 0
    all_parent, all_ref, all_lo, all_hi = parent, ref, lo, hi
    parent, ref, lo, hi = parent[leaf], ref[leaf], lo[leaf], hi[leaf]
    payload = ~ref
    _fail((payload & LEAF_WORLD) != flag, "partition", name, parent, "TWK_LEAF_WORLD is not what the tree's space says")
    _fail((payload & ~(LEAF_WORLD | 0x3fffffff)) != 0, "partition", name, parent, "a leaf reference with stray bits")
    first, count = payload & 0x0fffffff, ((payload >> 28) & 3) + 1
    _fail(count > MAX_LEAF, "leaf-size", name, parent, lambda k: f"a leaf of {count[k]} triangles")
    order = np.argsort(first, kind="stable")
    f, c, p = first[order], count[order], parent[order]
    _fail(f[:1] != slot_first, "partition", name, p[:1], lambda k: f"the first leaf begins at slot {f[0]}, the tree's range at {slot_first}")
    _fail(f[1:] != f[:-1] + c[:-1], "partition", name, p[1:], lambda k: f"after the leaf at slot {f[k]} ({c[k]} slots) comes the leaf at slot {f[k + 1]}")
    _fail(f[-1:] + c[-1:] != slot_first + nt, "partition", name, p[-1:], lambda k: f"the leaves end at slot {f[-1] + c[-1]}, the tree's range at {slot_first + nt}")
    # triangles-once
    sw = slots.view(np.int32)
    mine = np.arange(slot_first, slot_first + nt)
    prim = sw[mine, 3].astype(np.int64)
    _fail(np.sort(prim) != np.arange(nt), "triangles-once", name, mine, lambda k: f"the slots do not hold every triangle once: sorted position {k} holds {np.sort(prim)[k]}")
    if transform is not None:
        _fail(sw[mine, 7] != instance, "triangles-once", name, mine, lambda k: f"slot {mine[k]} carries instance {sw[mine[k], 7]}")
    # vertices
    got = slots[mine][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(nt, 3, 3)
    src = attrs[idx[prim], 0:3]
    if transform is None:
        _fail((got.view(np.uint32) != src.view(np.uint32)).any((1, 2)), "vertices", name, mine, lambda k: f"slot {mine[k]} is not triangle {prim[k]} bit for bit")
    else:
        m = transform.reshape(3, 4).astype(F64)
        terms = np.abs(src.astype(F64))[..., None, :] * np.abs(m[:, :3])
        want = src.astype(F64) @ m[:, :3].T + m[:, 3]
        # m0 x + m1 y + m2 z + m3 in float32: three products and three sums, every partial result bounded by the sum of the four
        # magnitudes, so six roundings of at most u times that sum each (a contraction to fused multiply-adds makes fewer)
        bound = 6.0 * U * (terms.sum(-1) + np.abs(m[:, 3])) * (1.0 + 2.0 ** -20) + 1e-45
        _fail((np.abs(got.astype(F64) - want) > bound).any((1, 2)), "vertices", name, mine, lambda k: f"slot {mine[k]} is not the world image of triangle {prim[k]}: off by {np.abs(got[k] - want[k]).max()}")
    # pairs
    prim_first, prim_pair = build_primitives(idx)
    pairs_at = np.zeros(nt + 1, bool)
    pairs_at[prim_first[prim_pair]] = True
    slot_of = np.zeros(nt, np.int64)
    slot_of[prim] = mine
    leaf_prim0, leaf_prim1 = prim[f - slot_first], prim[f + c - 1 - slot_first]
    is_pair_leaf = (c == 2) & pairs_at[leaf_prim0] & (leaf_prim1 == leaf_prim0 + 1)
    starts = prim_first[prim_pair]
    _fail(slot_of[starts + 1] != slot_of[starts] + 1, "pair-split", name, starts, lambda k: f"the halves {starts[k]}, {starts[k] + 1} of a pair are in slots {slot_of[starts[k]]}, {slot_of[starts[k] + 1]}")
    leaf_of_slot = np.repeat(np.arange(f.size), c)
    _fail(leaf_of_slot[slot_of[starts] - slot_first] != leaf_of_slot[slot_of[starts + 1] - slot_first], "pair-split", name, starts,
          lambda k: f"the halves {starts[k]}, {starts[k] + 1} of a pair are in different leaves")
    in_leaf_first = np.isin(slot_of[starts], f)
    _fail(~in_leaf_first, "pair-split", name, starts, lambda k: f"the pair {starts[k]} does not begin its leaf")
    _fail(is_pair_leaf.sum() != starts.size, "pair-leaf", name, p, f"{int(is_pair_leaf.sum())} pair leaves for {starts.size} pairs")
    # leaf boxes, both directions
    group_first = f - slot_first
    tlo, thi = tight_boxes(got, group_first[is_pair_leaf], np.full(int(is_pair_leaf.sum()), 2))
    vlo, vhi = got.min(1), got.max(1)
    blo, bhi = lo[order], hi[order]
    run_lo, _ = _runs(vlo, group_first, c)
    _, run_hi = _runs(vhi, group_first, c)
    _fail(((blo > run_lo) | (bhi < run_hi)).any(1), "leaf-contains", name, p, lambda k: f"the box of the leaf at slot {f[k]} does not contain its vertices: {blo[k]} {bhi[k]} against {run_lo[k]} {run_hi[k]}")
    lo_out, lo_in, hi_in, hi_out = pad_window(tlo, thi)
    lo_in_run, _ = _runs(lo_in, group_first, c)
    _, hi_in_run = _runs(hi_in, group_first, c)
    lo_out_run, _ = _runs(lo_out, group_first, c)
    _, hi_out_run = _runs(hi_out, group_first, c)
    _fail(((blo > lo_in_run) | (bhi < hi_in_run)).any(1), "pad-present", name, p, lambda k: f"the box of the leaf at slot {f[k]} is not its tight box grown by 0.999 e: {blo[k]} {bhi[k]} against {lo_in_run[k]} {hi_in_run[k]}")
    _fail(((blo < lo_out_run) | (bhi > hi_out_run)).any(1), "pad-once", name, p, lambda k: f"the box of the leaf at slot {f[k]} exceeds its tight box grown by 1.001 e: {blo[k]} {bhi[k]} against {lo_out_run[k]} {hi_out_run[k]}")
    measured = {"levels": levels, "leaf_first": f, "leaf_count": c, "pair_leaf": is_pair_leaf, "pairs": int(starts.size), "primitives": int(prim_first.size)}
    _inner_checks(name, rb, all_parent, all_ref, all_lo, all_hi)
    measured["sah"] = _sah(nodes, root, all_ref, lo, hi, order, tlo, thi, group_first, c, is_pair_leaf, prim_first.size)
    return measured


def _inner_checks(name, rb, parent, ref, lo, hi):
    """inner-union over the walked children; wide nodes and their quantisation for every walked parent."""
    nodes = rb.nodes
    inner = ref >= 0
    ulo, uhi = child_boxes_union(nodes, ref[inner])
    bad = (ulo.view(np.uint32) != lo[inner].view(np.uint32)).any(1) | (uhi.view(np.uint32) != hi[inner].view(np.uint32)).any(1)
    _fail(bad, "inner-union", name, parent[inner], lambda k: f"the box of inner child {ref[inner][k]} is {lo[inner][k]} {hi[inner][k]}, its children's union {ulo[k]} {uhi[k]}")
    audit_wide(name, rb, np.unique(parent))


def candidates(nodes, parents):
    """Per inner node, what its wide node may hold: entry lists for the four cuts (child / the child's two children, per child) as
    refs [n, 4 cuts, 4], boxes lo / hi [n, 4, 4, 3] and lengths [n, 4]; a cut that opens a leaf has length 0."""
    words = nodes.view(np.int32)
    n = parents.size
    refs, lo, hi = np.full((n, 4, 4), SENTINEL, np.int64), np.zeros((n, 4, 4, 3), F32), np.zeros((n, 4, 4, 3), F32)
    length, ok = np.zeros((n, 4), np.int64), np.ones((n, 4), bool)
    rows = np.arange(n)
    for mask in range(4):
        at = np.zeros(n, np.int64)
        for k in range(2):
            cref = words[parents, 12 + k].astype(np.int64)
            clo, chi = nodes[parents, 6 * k:6 * k + 3], nodes[parents, 6 * k + 3:6 * k + 6]
            present = ~((clo[:, 0] == np.inf) & (chi[:, 0] == np.inf))
            if mask & (1 << k):
                ok[:, mask] &= present & (cref >= 0)
                g = np.where(cref >= 0, cref, 0)
                for j in range(2):
                    refs[rows, mask, at] = words[g, 12 + j]
                    lo[rows, mask, at], hi[rows, mask, at] = nodes[g, 6 * j:6 * j + 3], nodes[g, 6 * j + 3:6 * j + 6]
                    at = at + 1
            else:
                refs[rows, mask, at] = cref
                lo[rows, mask, at], hi[rows, mask, at] = clo, chi
                at = at + present
        length[:, mask] = np.where(ok[:, mask], at, 0)
    return refs, lo, hi, length


def audit_wide(name, rb, parents):
    """The quantised wide nodes of the inner nodes `parents`: a cut of the binary tree, and its quantisation in both directions."""
    qlo, qhi, qref, valid, origin, cell, ql, qh = decode(rb.wideQ[parents])
    crefs, clo, chi, clen = candidates(rb.nodes, parents)
    nvalid = valid.sum(1)
    _fail(valid != (np.arange(4) < nvalid[:, None]), "wide-unused", name, parents, "the valid entries of a wide node are not its first")
    k4 = np.arange(4)
    match = np.zeros((parents.size, 4), bool)
    for mask in range(4):
        used = k4 < clen[:, mask, None]
        match[:, mask] = (clen[:, mask] > 0) & (clen[:, mask] == nvalid) & ((crefs[:, mask] == qref) | ~used).all(1)
    _fail(~match.any(1), "wide-cut", name, parents, lambda k: f"the entries {qref[k][:nvalid[k]]} are no cut of the node's children {crefs[k, 0, :2]} and their children {crefs[k, 3]}")
    pick = np.argmax(match, 1)
    rows = np.arange(parents.size)
    elo, ehi = clo[rows, pick], chi[rows, pick]
    # unused entries: the inverted box on every axis and the first entry's reference
    unused = ~valid
    _fail((unused[:, :, None] & ((ql != 255) | (qh != 0))).any((1, 2)), "wide-unused", name, parents, "an unused entry is not the inverted box (lo 255, hi 0)")
    _fail((unused & (qref != qref[:, :1])).any(1), "wide-unused", name, parents, "an unused entry does not repeat the first entry's reference")
    audit_quantisation(name, parents, valid, elo, ehi, qlo, qhi, origin, cell)


def audit_quantisation(name, parents, valid, elo, ehi, qlo, qhi, origin, cell):
    v3 = valid[:, :, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mant, expo = np.frexp(cell)
        _fail(((mant != 0.5) | ~np.isfinite(cell)).any(1), "cell-size", name, parents, lambda k: f"cell {cell[k]} is not a power of two")
        want_origin = np.where(v3, elo, np.inf).min(1)
        top = np.where(v3, ehi, -np.inf).max(1)
        _fail((origin.view(np.uint32) != want_origin.astype(F32).view(np.uint32)).any(1), "origin", name, parents, lambda k: f"origin {origin[k]}, the minimum of the entries {want_origin[k]}")
        extent = (top.astype(F32) - want_origin.astype(F32)).astype(F64)
        # the smallest power of two with extent / cell < 254: a cell of half the size would give 254 or more, so the ratio is at least
        # 127. frexp of the float32 product extent * (1 / 254) decides on the device; its rounding (2^-23 relative, two roundings)
        # can put a ratio within that of 127 or 254 on either side, which the comparison allows for.
        ratio = extent / cell.astype(F64)
        free = (extent > 0) & (expo - 1 > -125) & (expo - 1 < 126)
        slack = 1.0 + 2.0 ** -21
        _fail((free & ((ratio * slack < 127.0) | (ratio >= 254.0 * slack))).any(1), "cell-size", name, parents, lambda k: f"extent / cell = {ratio[k]}, not in [127, 254)")
        _fail((v3 & ((qlo > elo) | (qhi < ehi))).any((1, 2)), "quantised-contains", name, parents, lambda k: f"decoded {qlo[k]} {qhi[k]} does not contain {elo[k]} {ehi[k]}")
        # one cell for floor / ceil, one for the correction step; the decoded plane itself is rounded to float32 once more
        c64 = cell[:, None].astype(F64)
        room = 2.0 * c64 + 2.0 * U * np.maximum(np.abs(elo), np.abs(ehi)).astype(F64)
        loose = v3 & ((qlo.astype(F64) < elo.astype(F64) - room) | (qhi.astype(F64) > ehi.astype(F64) + room))
        _fail(loose.any((1, 2)), "quantised-tight", name, parents, lambda k: f"decoded {qlo[k]} {qhi[k]} is more than two cells {cell[k]} outside {elo[k]} {ehi[k]}")


def _sah(nodes, root, ref, lo, hi, order, tlo, thi, group_first, c, is_pair_leaf, primitives):
    """sahInnerCost and sahLeafCost of one tree in float64, from what was read back, as sahCostKernel adds them up: every inner node
    with the union of its child boxes; a leaf of ONE build primitive (a triangle, a pair) with that primitive's UNPADDED box, a leaf
    that is a collapsed subtree of two primitives with its (padded) node box; all over the root's box. One primitive: nothing."""
    if primitives < 2:
        return 0.0, 0.0
    rlo, rhi = child_boxes_union(nodes, np.array([root]))
    with np.errstate(over="ignore", invalid="ignore"):
        root_area = float(half_area(rlo.astype(F32), rhi.astype(F32))[0])
        if not (root_area > 0.0 and np.isfinite(root_area)):
            return None  # the device divides float32 half-areas: beyond their range the terms mean nothing
        inner = ref >= 0
        ulo, uhi = child_boxes_union(nodes, ref[inner])
        inner_cost = 1.0 + float(half_area(ulo.astype(F64), uhi.astype(F64)).sum()) / root_area
        single = (c == 1) | is_pair_leaf
        blo, bhi = lo[order], hi[order]
        unpadded = half_area(tlo[group_first].astype(F64), thi[group_first].astype(F64))
        padded = half_area(blo.astype(F64), bhi.astype(F64))
        leaf_cost = float((np.where(single, unpadded, padded) * c).sum()) / root_area
    return inner_cost, leaf_cost


def _instance_box(scene, i, tree_root_box):
    g, m = scene.instances[i]
    lo, hi = (v.astype(F64) for v in tree_root_box)
    m = m.reshape(3, 4).astype(F64)
    corners = np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])
    w = corners @ m[:, :3].T + m[:, 3]
    mag = np.abs(corners) @ np.abs(m[:, :3]).T + np.abs(m[:, 3])
    return w.min(0), w.max(0), mag.max(0)


def audit(scene, rb):
    """The whole scene. Returns {"trees": {name: measurements}, "top": ..., "sahInner", "sahLeaf", "height"}."""
    gi = [g for g, _ in scene.instances]
    gt = [idx.shape[0] for _, idx in scene.geometries]
    lay = scene_layout(gi, gt, scene.policy)
    all_flat = lay["entered"] == 0
    build, info = rb.build, rb.info
    counted = {"nodes": lay["nodes"], "triangleSlots": lay["slots"], "instances": len(gi), "flattenedInstances": len(gi) - lay["entered"],
               "directLeafInstances": sum(lay["directLeaf"]), "trees": sum(lay["needsBlas"]) + sum(lay["flattened"])}
    for key, value in counted.items():
        _fail(build[key] != value, "counts", "scene", -1, f"TwkBuildInfo.{key} = {build[key]}, counted {value}")
    _fail(rb.nodes.shape[0] != lay["nodes"] or rb.slots.shape[0] != lay["slots"] or rb.shade.shape[0] != lay["slots"], "counts", "scene", -1, "the arrays read back are not of the counted sizes")
    _fail(info["twoLevel"] != int(not all_flat), "counts", "scene", -1, "twoLevel")
    tree_nodes = lambda n: n - 1 if n > 1 else 1
    out = {"trees": {}}
    root_box = {}
    for g in range(len(gt)):
        if lay["needsBlas"][g]:
            name = f"geometry {g}"
            out["trees"][name] = audit_tree(name, scene, rb, g, lay["geometryNodeBase"][g], lay["geometryNodeBase"][g], tree_nodes(gt[g]), lay["geometrySlotBase"][g], None, -1)
            root_box[("g", g)] = child_boxes_union(rb.nodes, np.array([lay["geometryNodeBase"][g]]))
    for i, (g, m) in enumerate(scene.instances):
        if lay["flattened"][i]:
            name = f"instance {i}"
            out["trees"][name] = audit_tree(name, scene, rb, g, lay["flatNodeBase"][i], lay["flatNodeBase"][i], tree_nodes(gt[g]), lay["flatSlotBase"][i], m, i)
            root_box[("i", i)] = child_boxes_union(rb.nodes, np.array([lay["flatNodeBase"][i]]))
    top_levels = 0
    binary_root = lay["flatNodeBase"][0] if lay["single"] else lay["tlasBase"]
    if not lay["single"]:
        top_levels = _audit_top(scene, rb, lay, root_box)
    _audit_reachability(scene, rb, lay, binary_root, out)
    _audit_caches(scene, rb, lay, out, all_flat)
    # height: the top level, then the deepest tree below it — a spliced world-space tree, or an instance entry and its geometry's tree
    flat_h = max([out["trees"][f"instance {i}"]["levels"] for i in range(len(gi)) if lay["flattened"][i]], default=0)
    ent_h = max([out["trees"][f"geometry {g}"]["levels"] for g in range(len(gt)) if lay["needsBlas"][g]], default=0)
    out["height"] = top_levels + max(flat_h, 1 + ent_h if lay["entered"] else 0)
    _fail(build["maxTraversalDepth"] != out["height"], "height", "scene", -1, f"maxTraversalDepth = {build['maxTraversalDepth']}, measured {out['height']} (top {top_levels}, flattened {flat_h}, entered {ent_h})")
    # SAH terms: the sum over the trees; each term is a positive float32 quotient of two half-areas (three products, two sums, a
    # division: fewer than 8 roundings of 2^-24) accumulated in double, so the sums agree within 2^-20 relative
    terms = [t["sah"] for t in out["trees"].values()]
    out["sahDefined"] = all(t is not None for t in terms)
    if out["sahDefined"]:
        out["sahInner"], out["sahLeaf"] = sum(t[0] for t in terms), sum(t[1] for t in terms)
        for key, want in (("sahInnerCost", out["sahInner"]), ("sahLeafCost", out["sahLeaf"])):
            _fail(not abs(build[key] - want) <= 2.0 ** -20 * abs(want), "sah-terms", "scene", -1, f"TwkBuildInfo.{key} = {build[key]!r}, summed over the tree read back {want!r}")
    pairs = sum(t["pairs"] for t in out["trees"].values())
    _fail(build["pairLeaves"] != pairs or build["pairTriangles"] != 2 * pairs, "pair-counts", "scene", -1, f"pairLeaves = {build['pairLeaves']}, pairTriangles = {build['pairTriangles']}, counted {pairs} pairs")
    _audit_pair_records(scene, rb, lay, out, all_flat)
    _audit_shading(scene, rb, lay)
    # instance records: the transform as given, and where the instance's tree and slots stand
    rec = rb.instances.view(np.int32)
    for i, (g, m) in enumerate(scene.instances):
        flat = lay["flattened"][i]
        want = (lay["flatNodeBase"][i] if flat else lay["geometryNodeBase"][g], lay["flatSlotBase"][i] if flat else lay["geometrySlotBase"][g], gt[g], g)
        _fail([tuple(int(v) for v in rec[i, 12:16]) != want or (rb.instances[i, 16:28].view(np.uint32) != m.view(np.uint32)).any()], "instances", f"instance {i}", -1,
              f"the record holds (root, first slot, triangles, geometry) = {rec[i, 12:16]}, expected {want}, or not the transform")
    return out


def _audit_top(scene, rb, lay, root_box):
    """The top level: every instance once, with the reference and the box its kind asks for; the usual checks of its own nodes."""
    n = len(scene.instances)
    base, count = lay["tlasBase"], max(n - 1, 1)
    parent, side, ref, lo, hi, level, levels = walk(rb.nodes, base, base, count)
    name = "top level"
    want_ref, kind = np.zeros(n, np.int64), []
    for i, (g, m) in enumerate(scene.instances):
        gt = scene.geometries[g][1].shape[0]
        if not lay["flattened"][i]:
            want_ref[i] = ~i
        elif lay["directLeaf"][i]:
            want_ref[i] = ~(lay["flatSlotBase"][i] | ((gt - 1) << 28) | LEAF_WORLD)
        else:
            want_ref[i] = lay["flatNodeBase"][i]
    outer = np.nonzero(~((ref >= base) & (ref < base + count)))[0]
    order = outer[np.argsort(ref[outer], kind="stable")]
    found = np.minimum(np.searchsorted(ref[order], want_ref), order.size - 1)
    _fail(ref[order][found] != want_ref, "top-level", name, np.arange(n), lambda k: f"instance {k} is not referenced ({want_ref[k]})")
    _fail(order.size != n, "top-level", name, parent, f"{order.size} references for {n} instances")
    at = order[found]
    for i, (g, m) in enumerate(scene.instances):
        blo, bhi = lo[at[i]], hi[at[i]]
        if lay["flattened"][i]:
            rlo, rhi = root_box[("i", i)]
            tlo, thi = rlo[0], rhi[0]
            lo_out, lo_in, hi_in, hi_out = pad_window(tlo[None], thi[None])
            # the top level's build pads every primitive box like any other (refitKernel calls padBox for both levels)
            bad = (blo > lo_in[0]).any() or (bhi < hi_in[0]).any() or (blo < lo_out[0]).any() or (bhi > hi_out[0]).any()
            _fail(bad, "top-level", name, parent[at[i]], f"the box of flattened instance {i} is {blo} {bhi}, its tree's root box {tlo} {thi}")
        else:
            wlo, whi, mag = _instance_box(scene, i, (root_box[("g", g)][0][0], root_box[("g", g)][1][0]))
            _fail((blo > wlo).any() or (bhi < whi).any(), "top-level", name, parent[at[i]], f"the box of instance {i} {blo} {bhi} does not contain the world image {wlo} {whi} of its tree's root box")
            # how far beyond: the eight corners go through m0 x + m1 y + m2 z + m3 in float32 (six roundings of the magnitudes' sum),
            # then the host pads by 1e-5 max(1, |lo|, |hi|) per axis (the float32 constant 1e-5 and two roundings: 2^-22 relative),
            # and the top level's build pads once more like every primitive box (padBox: 1.001 e, e from the padded box)
            reach = np.maximum(1.0, np.maximum(np.abs(wlo), np.abs(whi)) + 6.0 * U * mag)
            room = 6.0 * U * mag + 1.0e-5 * (1.0 + 2.0 ** -20) * reach * (1.0 + 1.0e-5)
            ilo, ihi = wlo - room, whi + room
            mmax = np.maximum(np.abs(ilo), np.abs(ihi)).max()
            e = 1.001 * (2.0 ** -17 * (mmax + np.sqrt(((ihi - ilo) ** 2).sum())) + 1.0e-30) + 2.0 * U * mmax
            _fail((blo.astype(F64) < ilo - e).any() or (bhi.astype(F64) > ihi + e).any(), "top-level", name, parent[at[i]], f"the box of instance {i} {blo} {bhi} exceeds the world image {wlo} {whi} by more than the transform's rounding and the two pads")
    inner = (ref >= base) & (ref < base + count)
    ulo, uhi = child_boxes_union(rb.nodes, ref[inner])
    bad = (ulo.view(np.uint32) != lo[inner].view(np.uint32)).any(1) | (uhi.view(np.uint32) != hi[inner].view(np.uint32)).any(1)
    _fail(bad, "inner-union", name, parent[inner], lambda k: f"the box of inner child {ref[inner][k]} is not its children's union")
    audit_wide(name, rb, np.unique(parent))
    return levels


def _leaf_multiset_binary(rb, root):
    """Every leaf and instance reference below `root` through the binary nodes, across spliced trees."""
    words = rb.nodes.view(np.int32)
    frontier, leaves, seen = np.array([root], np.int64), [], 0
    while frontier.size:
        seen += frontier.size
        if seen > rb.nodes.shape[0]:
            raise AuditError("reachability", "scene", int(frontier[0]), "the binary nodes reach a node twice")
        ref = words[frontier][:, 12:14].reshape(-1).astype(np.int64)
        lo = np.stack([rb.nodes[frontier, 0], rb.nodes[frontier, 6]], 1).reshape(-1)
        ref = ref[lo != np.inf]
        leaves.append(ref[ref < 0])
        frontier = ref[ref >= 0]
    return np.sort(np.concatenate(leaves))


def _audit_reachability(scene, rb, lay, binary_root, out):
    """Through the quantised wide nodes from root (and root2) the same leaf and instance references, each once, as through the binary
    nodes from the binary root; the two nodes of an 8-wide root hold at most 8 entries together."""
    info = rb.info
    want = _leaf_multiset_binary(rb, binary_root)
    roots = [info["root"]] + ([info["root2"]] if info["root2"] >= 0 else [])
    _fail(info["root2"] < 0 and info["root"] != binary_root, "reachability", "scene", info["root"], f"root {info['root']} is not the binary root {binary_root}")
    if info["root2"] >= 0:
        _fail([info["root"] != lay["nodes"] or info["root2"] != lay["nodes"] + 1], "reachability", "scene", info["root"], "an 8-wide root stands behind the last node")
    _, _, qref, valid, *_ = decode(rb.wideQ)
    frontier, leaves, seen = np.array(roots, np.int64), [], 0
    while frontier.size:
        seen += frontier.size
        if seen > rb.wideQ.shape[0]:
            raise AuditError("reachability", "scene", int(frontier[0]), "the wide nodes reach a node twice")
        ref = qref[frontier][valid[frontier]]
        leaves.append(ref[ref < 0])
        frontier = ref[ref >= 0]
    got = np.sort(np.concatenate(leaves))
    _fail(got.size != want.size or (got != want[:got.size]).any(), "reachability", "scene", info["root"], f"{got.size} leaf references through the wide nodes, {want.size} through the binary nodes, or not the same ones")
    if info["root2"] >= 0:
        # the two root nodes are no inner node's wide node: their entries are checked against the binary children they name
        # every child the binary nodes reach from the binary root (nodes a tree over pairs leaves unused are zero and never reached)
        _, _, cref, clo, chi, _, _ = walk(rb.nodes, binary_root, 0, lay["nodes"])
        nodes2 = np.array(roots)
        qlo, qhi, qr, v, origin, cell, ql, qh = decode(rb.wideQ[nodes2])
        _fail([v.sum() > 8 or v.sum() <= 4], "wide-cut", "scene", info["root"], f"the 8-wide root holds {int(v.sum())} entries")
        elo, ehi = np.full((2, 4, 3), np.inf, F32), np.full((2, 4, 3), np.inf, F32)
        for a in range(2):
            for k in range(4):
                if not v[a, k]:
                    continue
                where = np.nonzero(cref == qr[a, k])[0]
                _fail([where.size != 1], "wide-cut", "scene", nodes2[a], f"entry {qr[a, k]} of the 8-wide root is not a child of exactly one binary node")
                elo[a, k], ehi[a, k] = clo[where[0]], chi[where[0]]
        _fail((~v & (qr != qr[:, :1])).any(1), "wide-unused", "scene", nodes2, "an unused entry of the 8-wide root does not repeat the first entry's reference")
        audit_quantisation("8-wide root", nodes2, v, elo, ehi, qlo, qhi, origin, cell)


def _pair_leaf_refs(out, lay):
    """The references (as the binary nodes hold them) of every pair leaf of the scene."""
    refs = []
    for t in out["trees"].values():
        f = t["leaf_first"][t["pair_leaf"]]
        refs.append(~(f | (1 << 28) | LEAF_WORLD))
    return np.concatenate(refs) if refs else np.zeros(0, np.int64)


def _audit_caches(scene, rb, lay, out, all_flat):
    """topNodes / topNodes7: the first wide nodes in breadth-first order from root (root2 second), references among them rewritten to
    TWK_NODE_CACHED | slot and nothing else touched — but a pair leaf's reference, which in a scene without entered instances stands
    there (and in the device's wideQ) without TWK_LEAF_WORLD while binary nodes and twk_debug_read_acceleration show it set."""
    info = rb.info
    two = info["root2"] >= 0
    want_root = (NODE_CACHED | 0) if scene.top_cache else info["root"]
    want_root2 = SENTINEL if not two else ((NODE_CACHED | 1) if scene.top_cache else info["root2"])
    _fail([rb.topRoot != want_root or rb.topRoot2 != want_root2], "top-root", "scene", info["root"], f"topRoot {rb.topRoot:#x}, topRoot2 {rb.topRoot2:#x}: expected {want_root:#x}, {want_root2:#x}")
    pair_refs = _pair_leaf_refs(out, lay) if all_flat else np.zeros(0, np.int64)
    _, _, qref, valid, *_ = decode(rb.wideQ)
    words = rb.wideQ.view(np.uint32)
    _fail(np.isin(qref[valid], ~((~pair_refs) & ~LEAF_WORLD)), "cache-references", "scene", -1, "the canonical wide nodes show a pair leaf without TWK_LEAF_WORLD")
    for name, cache, slots in (("topNodes", rb.topNodes, TOP_NODES), ("topNodes7", rb.topNodes7, TOP_NODES7)):
        queue = [info["root"]] + ([info["root2"]] if two else [])
        i = 0
        while i < len(queue) and len(queue) < slots:
            node = queue[i]
            for k in range(4):
                r = int(qref[node, k])
                if valid[node, k] and r >= 0 and r != SENTINEL and len(queue) < slots:
                    queue.append(r)
            i += 1
        queue = np.array(queue, np.int64)
        got = cache.view(np.uint32)
        n = queue.size
        _fail((got[:n, 0:12] != words[queue, 0:12]).any(1), "cache-order", name, queue, lambda k: f"slot {k} is not wide node {queue[k]}, the next in breadth-first order")
        _fail((got[n:] != 0).any(1), "cache-order", name, np.arange(n, slots), "a slot that is never referenced is not zero")
        want = qref[queue].copy()
        slot_of = {int(q): s for s, q in enumerate(queue)}
        inner = (want >= 0) & (want != SENTINEL)
        rewritten = np.vectorize(lambda r: (NODE_CACHED | slot_of[r]) if r in slot_of else r, otypes=[np.int64])(want)
        want = np.where(inner, rewritten, want)
        is_pair = np.isin(want, pair_refs) & (want < 0)
        want = np.where(is_pair, ~((~want) & ~LEAF_WORLD), want)
        have = cache.view(np.int32)[:n, 12:16].astype(np.int64)
        _fail((have != want).any(1), "cache-references", name, queue, lambda k: f"slot {k} (wide node {queue[k]}) holds the references {have[k]}, expected {want[k]}")


def _audit_pair_records(scene, rb, lay, out, all_flat):
    """The 64-byte record of a pair leaf at first >> 1: w0 | primitive of T0, w1 | primitive of T1, w2 | instance, w3 | first slot, with
    T0 = (w0, w1, w2) slot `first`, T1 = (w2, w3, w0) slot `first + 1`. Only where the handle gives the records out."""
    if rb.pairs is None or not all_flat:
        return
    s = np.concatenate([t["leaf_first"][t["pair_leaf"]] for t in out["trees"].values()] or [np.zeros(0, np.int64)])
    rec, sl = rb.pairs.view(np.uint32)[s >> 1], rb.slots.view(np.uint32)
    want = np.concatenate([sl[s, 0:4], sl[s, 4:7], sl[s + 1, 3:4], sl[s, 8:11], sl[s, 7:8], sl[s + 1, 4:7], s[:, None].astype(np.uint32)], 1)
    _fail((rec != want).any(1), "pair-record", "scene", s, lambda k: f"the pair record of the leaf at slot {s[k]} is not its two slots")
    closes = (sl[s + 1, 0:3] == sl[s, 8:11]).all(1) & (sl[s + 1, 8:11] == sl[s, 0:3]).all(1)
    _fail(~closes, "pair-record", "scene", s, lambda k: f"the second triangle of the pair at slot {s[k]} is not (w2, w3, w0)")


def _audit_shading(scene, rb, lay):
    """The 128-byte record of slot s: geometric normal cross(v1 - v0, v2 - v0) of the OBJECT-space vertices, then the three normals, the
    three tangents, the three texcoords, copied from the attributes bit for bit in every tree (the emission leaves shading records
    in object space). The cross product is six products and three differences of float32 differences: it is compared with float64
    within 8 u (|a||b| summed per component), the copies bit for bit."""
    sw = rb.slots.view(np.int32)
    for i, (g, m) in enumerate(scene.instances):
        first = lay["flatSlotBase"][i] if lay["flattened"][i] else lay["geometrySlotBase"][g]
        attrs, idx = scene.geometries[g]
        s = np.arange(first, first + idx.shape[0])
        a, b, c = (attrs[idx[sw[s, 3], k]] for k in range(3))
        want = np.concatenate([a[:, 6:9], b[:, 6:9], c[:, 6:9], a[:, 3:6], b[:, 3:6], c[:, 3:6], a[:, 9:12], b[:, 9:12], c[:, 9:12], np.zeros((s.size, 2), F32)], 1)
        got = rb.shade[s]
        _fail((got[:, 3:].view(np.uint32) != want.view(np.uint32)).any(1), "shading", f"instance {i}", s, lambda k: f"the shading record of slot {s[k]} does not hold the attributes of triangle {sw[s[k], 3]}")
        e1, e2 = (b[:, 0:3] - a[:, 0:3]).astype(F32).astype(F64), (c[:, 0:3] - a[:, 0:3]).astype(F32).astype(F64)
        ng = np.cross(e1, e2)
        mag = np.abs(e1)[:, [1, 2, 0]] * np.abs(e2)[:, [2, 0, 1]] + np.abs(e1)[:, [2, 0, 1]] * np.abs(e2)[:, [1, 2, 0]]
        _fail((np.abs(got[:, 0:3].astype(F64) - ng) > 8.0 * U * mag + 1e-45).any(1), "shading", f"instance {i}", s, lambda k: f"the geometric normal of slot {s[k]} is {got[k, 0:3]}, expected {ng[k]}")
