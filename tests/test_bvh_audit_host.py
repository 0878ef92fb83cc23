"""CPU: the audit of tests/bvh_audit.py on the reference's own trees, and against itself.

1. Both reference builders (bvh_reference.binned_sah, median_split) on every input of tests/test_gpu_bvh_audit.py, entered and
   flattened, written by bvh_reference.emit: the audit passes. This is the evidence that the reference alone meets every condition the
   device test asks of the device: binned SAH costs no more than the median split on the well-behaved meshes, the forced-middle input
   peels one primitive per level for 40 levels with finite areas and stays under the traversal stacks' height.
2. One reference tree of 257 build primitives with pairs, one mutation at a time: the AuditError names the check the mutation breaks.
3. bvh_reference.build_primitives equals bvh_build.h trianglePairs, through a stand-alone program compiled here (with the address
   and undefined-behaviour sanitizers) on random index lists with odd counts and broken pairs."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bvh_audit as A
import bvh_audit_scenes as M
import bvh_reference as R
import selective_scenes as S
from conftest import ROOT

F32, F64 = np.float32, np.float64
CASES, MESHES = M.cases()


def _scene(names, policy):
    geometries = [MESHES[n] for n in names]
    return geometries, [(k, M.place(k)) for k in range(len(names))], policy


@pytest.mark.parametrize("policy", [(0, 0), M.EVERYTHING_FLAT], ids=["entered", "flattened"])
@pytest.mark.parametrize("builder", ["binned_sah", "median_split"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_audit_passes_on_the_reference_trees(case, builder, policy):
    geometries, instances, policy = _scene(CASES[case], policy)
    rb = R.emit(geometries, instances, policy, getattr(R, builder))
    out = A.audit(A.Scene(geometries, instances, policy), rb)
    assert len(out["trees"]) == len(geometries) and out["sahDefined"]


def test_binned_sah_beats_the_median_split_on_the_well_behaved_meshes():
    for name, (c64, c32, median) in M.reference_costs().items():
        print(f"{name}: binned SAH float64 {c64:.4f}, float32 {c32:.4f} (ratio {c32 / c64:.6f}), median split {median:.4f}")
        assert c64 <= median and c32 <= median, name
    print(f"margin {M.quality_margin():.4f}")
    assert 0.01 <= M.quality_margin() < 0.1


def test_forced_middle_input_peels_one_primitive_per_level():
    """(a) every level up to 40 has exactly one candidate partition and peels one primitive, (b) every area of the sweep is finite and
    the root's is positive, (c) the height stays under what the traversal stacks hold — in float32, as the device builds."""
    boxes, triangles = M.boxes_of(M.forced_middle())
    tree = R.binned_sah(boxes, F32)
    assert len(tree.levels) > R.FORCE_LEVEL
    for level in range(R.FORCE_LEVEL):
        (candidates, left), = tree.levels[level]
        assert candidates == 1 and left == 57 - level - 1, (level, candidates, left)
    assert all(left < 0 for record in tree.levels[R.FORCE_LEVEL:] for _, left in record), "from level 40 on every range is cut in the middle"
    root_area = R.half_area(boxes[:, 0].min(0), boxes[:, 1].max(0))
    assert tree.areas_finite and np.isfinite(root_area) and root_area > 0
    height = R.height(tree, triangles)
    print(f"forced-middle reference: {len(tree.levels)} levels of the level loop, height {height}")
    assert R.FORCE_LEVEL + 1 <= height < M.stack_height()
    geometries, instances, policy = [M.forced_middle()], [(0, S.affine(1.0, (0.0, 0.0, 0.0)))], M.EVERYTHING_FLAT  # as the device test builds it
    out = A.audit(A.Scene(geometries, instances, policy), R.emit(geometries, instances, policy, lambda b: R.binned_sah(b, F32)))
    assert not out["sahDefined"], "the padded root box's half-area is beyond float32: the terms of this tree are not compared"


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations

@functools.lru_cache(maxsize=None)
def _subject():
    """One tree of 257 build primitives (254 pairs, a quad that does not pair, a trailing triangle) as the whole scene of one
    flattened instance — pair leaves, pair records and cleared bits in the caches — and what the audit measured of it."""
    geometries, instances, policy = [MESHES["odd-257"]], [(0, S.rotated((0.5, 0.25, -1.0)))], M.EVERYTHING_FLAT
    scene = A.Scene(geometries, instances, policy)
    rb = R.emit(geometries, instances, policy, R.binned_sah)
    return scene, rb, A.audit(scene, rb)["trees"]["instance 0"]


def _find(rb, ref):
    """(node, side) of the binary child with reference `ref`."""
    at = np.argwhere(rb.nodes.view(np.int32)[:, 12:14] == ref)
    assert at.shape[0] == 1
    return int(at[0, 0]), int(at[0, 1])


def _leaf_ref(first, count):
    return ~(int(first) | ((int(count) - 1) << 28) | R.LEAF_WORLD)


def _set_ref(rb, node, side, ref):
    rb.nodes.view(np.int32)[node, 12 + side] = ref


def _leaf_box(rb, tree, k):
    """Views of the box of the k-th leaf (in slot order): lo, hi."""
    node, side = _find(rb, _leaf_ref(tree["leaf_first"][k], tree["leaf_count"][k]))
    return rb.nodes[node, 6 * side:6 * side + 3], rb.nodes[node, 6 * side + 3:6 * side + 6]


def _tight(rb, tree, k):
    s, c = tree["leaf_first"][k], tree["leaf_count"][k]
    v = rb.slots[s:s + c][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
    return v.min(0), v.max(0)


def _single_leaves(tree):
    return np.nonzero(tree["leaf_count"] == 1)[0]


def m_slot_dropped(rb, tree):
    k = int(np.nonzero(tree["leaf_count"] == 2)[0][3])
    node, side = _find(rb, _leaf_ref(tree["leaf_first"][k], 2))
    _set_ref(rb, node, side, _leaf_ref(tree["leaf_first"][k], 1))


def m_slot_duplicated(rb, tree):
    rb.slots[11] = rb.slots[40]


def m_slots_swapped(rb, tree):
    a, b = (int(tree["leaf_first"][k]) for k in np.nonzero(~tree["pair_leaf"])[0][:2])  # leaves of single triangles: no pair moves
    rb.slots[[a, b]] = rb.slots[[b, a]]


def m_pair_split(rb, tree):
    f, c, pair = tree["leaf_first"], tree["leaf_count"], tree["pair_leaf"]
    for k in _single_leaves(tree):
        if k + 1 < f.size and pair[k + 1]:  # (s, 1) (s + 1, 2) becomes (s, 2) (s + 2, 1)
            (n0, s0), (n1, s1) = _find(rb, _leaf_ref(f[k], 1)), _find(rb, _leaf_ref(f[k + 1], 2))
            _set_ref(rb, n0, s0, _leaf_ref(f[k], 2))
            _set_ref(rb, n1, s1, _leaf_ref(f[k] + 2, 1))
            return
        if k > 0 and pair[k - 1]:  # (s, 2) (s + 2, 1) becomes (s, 1) (s + 1, 2)
            (n0, s0), (n1, s1) = _find(rb, _leaf_ref(f[k - 1], 2)), _find(rb, _leaf_ref(f[k], 1))
            _set_ref(rb, n0, s0, _leaf_ref(f[k - 1], 1))
            _set_ref(rb, n1, s1, _leaf_ref(f[k - 1] + 1, 2))
            return
    raise AssertionError("no single-triangle leaf beside a pair leaf")


def m_leaf_box_one_ulp(rb, tree):
    """The face with the largest coordinate of the tree, where one ulp is the largest part of the pad (1 / 64 to 1 / 128 of it)."""
    best = max(range(tree["leaf_first"].size), key=lambda k: float(_leaf_box(rb, tree, k)[1].max()))
    lo, hi = _leaf_box(rb, tree, best)
    axis = int(np.argmax(hi))
    hi[axis] = np.nextafter(hi[axis], F32(-np.inf))


def m_leaf_box_unpadded(rb, tree):
    k = int(np.nonzero(tree["pair_leaf"])[0][5])
    lo, hi = _leaf_box(rb, tree, k)
    lo[:], hi[:] = _tight(rb, tree, k)


def m_leaf_box_padded_twice(rb, tree):
    k = int(np.nonzero(tree["pair_leaf"])[0][5])
    lo, hi = _leaf_box(rb, tree, k)
    tlo, thi = _tight(rb, tree, k)
    lo[:], hi[:] = tlo - 2 * (tlo - lo), thi + 2 * (hi - thi)


def _inner_child(rb, depth=3):
    """(node, side) of an inner child a few levels below the root."""
    node = 0
    for _ in range(depth):
        refs = rb.nodes.view(np.int32)[node, 12:14]
        node = int(refs[refs >= 0][0])
    refs = rb.nodes.view(np.int32)[node, 12:14]
    return node, int(np.nonzero(refs >= 0)[0][0])


def m_inner_box_grown(rb, tree):
    node, side = _inner_child(rb)
    lo, hi = rb.nodes[node, 6 * side:6 * side + 3], rb.nodes[node, 6 * side + 3:6 * side + 6]
    hi += F32(0.01) * (hi - lo)


def m_wide_great_grandchild(rb, tree):
    node, _ = _inner_child(rb, 2)
    refs = rb.wideQ.view(np.int32)[node, 12:16]
    k = int(np.nonzero(refs >= 0)[0][0])
    refs[k] = rb.nodes.view(np.int32)[refs[k], 12]


def _plane_bytes(rb, node, word):
    return rb.wideQ.view(np.uint8)[node, 4 * word:4 * word + 4]


def m_plane_inwards(rb, tree):
    node, _ = _inner_child(rb, 2)
    lo, hi = _plane_bytes(rb, node, 6), _plane_bytes(rb, node, 9)
    k = int(np.argmax(hi.astype(int) - lo.astype(int)))
    assert hi[k] > lo[k] + 1
    lo[k] += 1


def m_cell_doubled(rb, tree):
    node, _ = _inner_child(rb, 2)
    rb.wideQ[node, 3] *= F32(2.0)


def m_cache_order(rb, tree):
    rb.topNodes[[2, 3]] = rb.topNodes[[3, 2]]


def m_cache_stale_reference(rb, tree):
    refs = rb.topNodes7.view(np.int32)[0, 12:16]
    k = int(np.nonzero((refs >= 0) & ((refs & R.NODE_CACHED) != 0))[0][0])
    refs[k] = R.NODE_CACHED | ((refs[k] & 0xff) + 1)


def m_depth(rb, tree):
    rb.build["maxTraversalDepth"] += 1


def m_sah_leaf(rb, tree):
    rb.build["sahLeafCost"] *= 1.0 + 1.0e-4


def m_pair_leaves(rb, tree):
    rb.build["pairLeaves"] += 1


def m_shading_swapped(rb, tree):
    rb.shade[[20, 21]] = rb.shade[[21, 20]]


def m_pair_record(rb, tree):
    s = int(tree["leaf_first"][tree["pair_leaf"]][7])
    rb.pairs[s >> 1, 12] += F32(0.125)


def m_cache_pair_bit(rb, tree):
    refs = rb.topNodes.view(np.int32)
    at = np.argwhere((refs[:, 12:16] < 0) & ((~refs[:, 12:16] & R.LEAF_WORLD) == 0))[0]
    refs[at[0], 12 + at[1]] = ~(~refs[at[0], 12 + at[1]] | R.LEAF_WORLD)


MUTATIONS = [(m_slot_dropped, "partition"), (m_slot_duplicated, "triangles-once"), (m_slots_swapped, "leaf-contains"), (m_pair_split, "pair-split"),
             (m_leaf_box_one_ulp, "pad-present"), (m_leaf_box_unpadded, "pad-present"), (m_leaf_box_padded_twice, "pad-once"), (m_inner_box_grown, "inner-union"),
             (m_wide_great_grandchild, "wide-cut"), (m_plane_inwards, "quantised-contains"), (m_cell_doubled, "cell-size"), (m_cache_order, "cache-order"),
             (m_cache_stale_reference, "cache-references"), (m_depth, "height"), (m_sah_leaf, "sah-terms"), (m_pair_leaves, "pair-counts"),
             (m_shading_swapped, "shading"), (m_pair_record, "pair-record"), (m_cache_pair_bit, "cache-references")]


@pytest.mark.parametrize("mutate,check", MUTATIONS, ids=[m.__name__[2:] for m, _ in MUTATIONS])
def test_the_audit_catches(mutate, check):
    scene, original, tree = _subject()
    rb = original.copy()
    mutate(rb, tree)
    with pytest.raises(A.AuditError) as e:
        A.audit(scene, rb)
    assert e.value.check == check, str(e.value)
    A.audit(scene, original)  # and the subject itself is still clean


def test_a_4097_primitive_tree_audits_in_well_under_a_second():
    import time
    geometries, instances, policy = [MESHES["quads-4097"]], [(0, M.place(0))], M.EVERYTHING_FLAT
    rb = R.emit(geometries, instances, policy, R.median_split)
    scene = A.Scene(geometries, instances, policy)
    start = time.perf_counter()
    A.audit(scene, rb)
    seconds = time.perf_counter() - start
    print(f"audit of 4097 pairs: {seconds * 1e3:.0f} ms")
    assert seconds < 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# build_primitives against trianglePairs

def test_build_primitives_equals_triangle_pairs(tmp_path):
    out = str(tmp_path / "triangle_pairs_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused-function",
                    "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    "-o", out, os.path.join(ROOT, "tests", "triangle_pairs_host.cpp")], check=True)
    rng = np.random.default_rng(31)
    lists = [MESHES["odd-9"][1], MESHES["quads-5"][1], MESHES["soup-7"][1], np.zeros(0, np.uint32), np.array([0, 1, 2], np.uint32)]
    for t in list(range(1, 12)) + [63, 64, 65, 257]:
        idx = rng.integers(0, 6, (t, 3)).astype(np.uint32)  # few distinct indices: chance pairs, also at odd triangles, where none may begin
        for k in range(0, t - 1, 2):
            if rng.random() < 0.5:  # a proper pair (a, b, c), (c, d, a)
                idx[k + 1, 0], idx[k + 1, 2] = idx[k, 2], idx[k, 0]
            elif rng.random() < 0.5:  # a broken one: (d, a, c)
                idx[k + 1, 1], idx[k + 1, 2] = idx[k, 0], idx[k, 2]
        lists.append(idx.reshape(-1))
    text = "".join(f"{l.size // 3} " + " ".join(str(int(i)) for i in l) + "\n" for l in lists)
    r = subprocess.run([out], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(lists)
    pairs_seen = 0
    for line, l in zip(lines, lists):
        words = [int(w) for w in line.split()]
        first, pair = R.build_primitives(l)
        assert words[0] == int(pair.sum()) and words[1::2] == list(first) and words[2::2] == [int(p) for p in pair], (l.reshape(-1, 3), line)
        pairs_seen += words[0]
    assert pairs_seen > 100
