"""CPU: the refit of one tree (csrc/bvh_refit.h) through its host form twk_refit_tree_host, on trees written by tests/bvh_reference.py —
no GPU, no product tree. The scenes and deformations are tests/refit_scenes.py's: trees of 1, 2, 3, 5, 64, 65, 257 and 1025 build
primitives, each as a bottom-level tree and as the world-space tree of a flattened instance under a rotation with unequal scales.
  - refit to B (noise, scale by 1.3, translation by 1e4, every vertex on one point), quantised with bvh_reference.quantise, passes
    bvh_audit.audit_tree against the scene with B, and its SAH terms are the audit's within the 2^-20 relative the audit allows
  - refit to the vertices the tree was built from leaves every byte: binary nodes, slots and shading records are bvh_reference.emit's,
    wide nodes and node costs the plain-numpy restatement's (refit_scenes.wide_of, node_costs)
  - A -> B -> A restores every byte of the input
  - references, primitive words, instance words and pair flags are unchanged by any refit
  - every refusal
  - the same host code under the address and undefined-behaviour sanitizers, in a stand-alone program (tests/refit_host.cpp)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bvh_audit as A
import bvh_reference as R
import refit_scenes as RS
from conftest import ROOT

F32, U32 = np.float32, np.uint32


@functools.lru_cache(maxsize=None)
def built(kind):
    """The scene of `kind` with the built vertices A, as bvh_reference.emit writes it under the float64 binned SAH, and per tree the
    arrays a selective handle keeps beside it: full-precision wide nodes, node costs, pair flags."""
    geometries, instances = list(RS.meshes()), RS.instances(kind)
    rb = R.emit(geometries, instances, RS.POLICY, R.binned_sah)
    trees, lay = RS.trees(geometries, instances, RS.POLICY)
    kept = []
    for t in trees:
        nb, nn, sb, ns = t["nodeBase"], t["nodes"], t["slotBase"], t["slots"]
        wide = RS.wide_of(rb.nodes, nb, nn)
        kept.append(dict(t, wide=wide, cost=RS.node_costs(rb.nodes, wide, nb, nn), flags=RS.pair_flags(geometries[t["geometry"]][1], rb.slots[sb:sb + ns])))
    return rb, kept


def refit(twk, tree, state, attributes, indices):
    """twk_refit_tree_host on one tree. state: (nodes, wide, cost, slots) of the tree's ranges."""
    nodes, wide, cost, slots = state
    return twk.refit_tree_host(nodes, wide, cost, slots, tree["flags"], attributes, indices, tree["nodeBase"], tree["slotBase"], tree["leafFlag"], tree["transform"], tree["instance"])


def state_of(rb, tree):
    nb, nn, sb, ns = tree["nodeBase"], tree["nodes"], tree["slotBase"], tree["slots"]
    return rb.nodes[nb:nb + nn].copy(), tree["wide"].copy(), tree["cost"].copy(), rb.slots[sb:sb + ns].copy()


def same(got, want, what):
    got, want = np.ascontiguousarray(got, F32).view(U32), np.ascontiguousarray(want, F32).view(U32)
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {bad[0]}: {got[bad[0]].view(F32)} against {want[bad[0]].view(F32)}"


@pytest.mark.parametrize("kind", RS.KINDS)
def test_a_refit_to_the_built_vertices_leaves_every_byte(twk, kind):
    rb, trees = built(kind)
    geometries = RS.meshes()
    for t in trees:
        a, i = geometries[t["geometry"]]
        nodes, wide, cost, slots = state_of(rb, t)
        out = refit(twk, t, (nodes, wide, cost, slots), a, i)
        sb, ns = t["slotBase"], t["slots"]
        same(out["nodes"], nodes, f"{kind}, {t['name']}: binary nodes")
        same(out["wideNodes"], wide, f"{kind}, {t['name']}: wide nodes")
        same(out["nodeCost"].reshape(-1, 1), cost.reshape(-1, 1), f"{kind}, {t['name']}: node costs")
        same(out["slots"], slots, f"{kind}, {t['name']}: slots")
        same(out["shadeRecords"], rb.shade[sb:sb + ns], f"{kind}, {t['name']}: shading records")
        # a second refit of what the first left: the same bytes again, without the restatement in between
        again = refit(twk, t, (out["nodes"], out["wideNodes"], out["nodeCost"], out["slots"]), a, i)
        for key in ("nodes", "wideNodes", "slots", "shadeRecords"):
            same(again[key], out[key], f"{kind}, {t['name']}: {key}, refit twice")
        # the root box is the tree's, the terms are bvh_reference.sah_terms' (the audit's tolerance)
        root = rb.nodes[t["nodeBase"]]
        lo, hi = (root[0:3], root[3:6]) if root[6] == np.inf else (np.minimum(root[0:3], root[6:9]), np.maximum(root[3:6], root[9:12]))
        same(out["rootBounds"].reshape(1, 6), np.concatenate([lo, hi]).reshape(1, 6), f"{kind}, {t['name']}: root box")


@pytest.mark.parametrize("deformation", RS.DEFORMATIONS)
@pytest.mark.parametrize("kind", RS.KINDS)
def test_a_refit_tree_passes_the_audit(twk, kind, deformation):
    rb, trees = built(kind)
    geometries, deformed, instances = RS.meshes(), RS.deformed_meshes(deformation), RS.instances(kind)
    scene = A.Scene(deformed, instances, RS.POLICY)
    after = rb.copy()
    terms = {}
    for t in trees:
        a, i = deformed[t["geometry"]]
        out = refit(twk, t, state_of(rb, t), a, i)
        nb, nn, sb, ns = t["nodeBase"], t["nodes"], t["slotBase"], t["slots"]
        after.nodes[nb:nb + nn], after.slots[sb:sb + ns], after.shade[sb:sb + ns] = out["nodes"], out["slots"], out["shadeRecords"]
        after.wideQ[nb:nb + nn] = RS.quantised(out["wideNodes"])
        terms[t["name"]] = out["terms"]
        # what no refit changes: the references of binary and wide nodes, primitive and instance words, the pair flags, the input
        assert np.array_equal(out["nodes"].view(np.int32)[:, 12:16], rb.nodes[nb:nb + nn].view(np.int32)[:, 12:16]), t["name"]
        assert np.array_equal(RS.wide_entries(out["wideNodes"])[2], RS.wide_entries(t["wide"])[2]), t["name"]
        assert np.array_equal(out["slots"].view(np.int32)[:, [3, 7, 11]], rb.slots[sb:sb + ns].view(np.int32)[:, [3, 7, 11]]), t["name"]
        assert np.array_equal(t["flags"], RS.pair_flags(geometries[t["geometry"]][1], out["slots"])), t["name"]
        if deformation != "collapse" or ns > 2:
            assert not np.array_equal(out["slots"].view(U32), rb.slots[sb:sb + ns].view(U32)), f"{t['name']}: the deformation shows"
    for t in trees:
        measured = A.audit_tree(t["name"], scene, after, t["geometry"], t["nodeBase"], t["nodeBase"], t["nodes"], t["slotBase"], None if t["leafFlag"] == 0 else t["transform"], t["instance"])
        if measured["sah"] is not None:
            for got, want, what in zip(terms[t["name"]], measured["sah"], ("sahInner", "sahLeaf")):
                assert abs(got - want) <= 2.0 ** -20 * abs(want), f"{kind}, {deformation}, {t['name']}: {what} {got!r}, the audit's {want!r}"


@pytest.mark.parametrize("deformation", RS.DEFORMATIONS)
@pytest.mark.parametrize("kind", RS.KINDS)
def test_a_refit_there_and_back_restores_every_byte(twk, kind, deformation):
    rb, trees = built(kind)
    geometries, deformed = RS.meshes(), RS.deformed_meshes(deformation)
    for t in trees:
        g = t["geometry"]
        there = refit(twk, t, state_of(rb, t), deformed[g][0], deformed[g][1])
        back = refit(twk, t, (there["nodes"], there["wideNodes"], there["nodeCost"], there["slots"]), geometries[g][0], geometries[g][1])
        nodes, wide, cost, slots = state_of(rb, t)
        sb, ns = t["slotBase"], t["slots"]
        for got, want, what in ((back["nodes"], nodes, "binary nodes"), (back["wideNodes"], wide, "wide nodes"), (back["nodeCost"].reshape(-1, 1), cost.reshape(-1, 1), "node costs"),
                                (back["slots"], slots, "slots"), (back["shadeRecords"], rb.shade[sb:sb + ns], "shading records")):
            same(got, want, f"{kind}, {deformation}, {t['name']}: {what}")


def test_without_costs_and_without_pair_flags(twk):
    """nodeCost NULL: the wide nodes and everything else as with costs. pairFlags NULL on a soup (no pairs): the same bytes; on a quad
    mesh every triangle is padded on its own, so a pair leaf's box is the union of two padded boxes and differs."""
    rb, trees = built("entered")
    geometries = RS.meshes()
    for t in trees:
        a, i = geometries[t["geometry"]]
        nodes, wide, cost, slots = state_of(rb, t)
        out = twk.refit_tree_host(nodes, wide, None, slots, t["flags"], a, i, t["nodeBase"], t["slotBase"])
        assert out["nodeCost"] is None
        same(out["wideNodes"], wide, t["name"])
        out = twk.refit_tree_host(nodes, wide, cost, slots, None, a, i, t["nodeBase"], t["slotBase"])
        if not t["flags"].any():
            same(out["nodes"], nodes, t["name"])
    quad = next(t for t in trees if t["flags"].any() and t["slots"] > 4)
    a, i = geometries[quad["geometry"]]
    nodes, wide, cost, slots = state_of(rb, quad)
    out = twk.refit_tree_host(nodes, wide, cost, slots, None, a, i, quad["nodeBase"], quad["slotBase"])
    assert not np.array_equal(out["nodes"].view(U32), nodes.view(U32))


def test_refusals(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE
    rb, trees = built("flat")
    geometries = RS.meshes()
    t = next(t for t in trees if t["slots"] == 127)  # the odd mix of 65 build primitives, world space
    a, i = geometries[t["geometry"]]
    nodes, wide, cost, slots = state_of(rb, t)

    def refused(word, **change):
        args = dict(nodes=nodes, wideNodes=wide, nodeCost=cost, slots=slots, pairFlags=t["flags"], attributes=a, indices=i, nodeBase=t["nodeBase"], slotBase=t["slotBase"],
                    leafFlag=t["leafFlag"], transform=t["transform"], idInstance=t["instance"])
        args.update(change)
        with pytest.raises(twk.TwkError) as e:
            twk.refit_tree_host(**args)
        assert e.value.code == VALUE and "twk_refit_tree_host" in str(e.value) and word in str(e.value), str(e.value)

    refit(twk, t, (nodes, wide, cost, slots), a, i)  # the arguments as they are pass
    refused("numIndices", indices=i[:-3])
    refused("beyond the attributes", attributes=a[:-1])
    refused("leafFlag", leafFlag=1)
    refused("TWK_LEAF_WORLD is not leafFlag", leafFlag=0)
    refused("transform", transform=None)
    refused("instance id", idInstance=-1)
    refused("node range", nodeBase=t["nodeBase"] + t["nodes"])
    refused("slot range", slotBase=t["slotBase"] + 1)
    refused("bases at least 0", nodeBase=-1)
    bad = nodes.copy()
    inner = np.nonzero(bad.view(np.int32)[:, 12] >= t["nodeBase"])[0]  # (an unused node holds 0, below this tree's base)
    assert t["nodeBase"] > 0 and inner.size > 4
    bad.view(np.int32)[inner[-1], 12] = t["nodeBase"]  # an inner reference back to the root
    refused("twice", nodes=bad)
    bad = nodes.copy()
    bad.view(np.int32)[inner[0], 12] = t["nodeBase"] + t["nodes"] + 5
    refused("node range", nodes=bad)
    bad = nodes.copy()
    bad[0] = 0
    refused("root", nodes=bad)
    bad = slots.copy()
    bad.view(np.int32)[7, 3] = t["slots"]
    refused("primitive word", slots=bad)
    # NULL arrays and counts, through the C call itself
    fp = C.POINTER(C.c_float)
    shade = np.zeros((t["slots"], 32), F32)
    idx = np.ascontiguousarray(i, U32)
    att = np.ascontiguousarray(a, F32)
    args = lambda: [nodes.copy().ctypes.data_as(fp), wide.copy().ctypes.data_as(fp), cost.copy().ctypes.data_as(fp), slots.copy().ctypes.data_as(fp), shade.ctypes.data_as(fp),
                    t["flags"].ctypes.data_as(C.POINTER(C.c_int)), att.ctypes.data_as(C.c_void_p), C.c_size_t(att.shape[0]), idx.ctypes.data_as(C.POINTER(C.c_uint)), C.c_size_t(idx.size),
                    int(t["nodeBase"]), int(t["nodes"]), int(t["slotBase"]), int(t["slots"]), int(t["leafFlag"]), t["transform"].ctypes.data_as(fp), int(t["instance"]), None, None]
    assert L.lib.twk_refit_tree_host(*args()) == L.TWK_SUCCESS, L.lib.twk_last_error().decode()
    for k in (0, 1, 3, 4, 6, 8):
        x = args()
        x[k] = None
        assert L.lib.twk_refit_tree_host(*x) == VALUE and "NULL" in L.lib.twk_last_error().decode(), k
    for k, value in ((11, 0), (13, 0), (7, C.c_size_t(0)), (12, -1), (13, 1 << 28)):
        x = args()
        x[k] = value
        assert L.lib.twk_refit_tree_host(*x) == VALUE, k
    # the device forms refuse a NULL handle before any HIP call, under their own names
    assert L.lib.twk_refit_geometry_vertices(None, 0, att.ctypes.data_as(C.c_void_p), C.c_size_t(1)) == VALUE and "twk_refit_geometry_vertices: NULL device handle" in L.lib.twk_last_error().decode()
    assert L.lib.twk_get_refit_info(None, None) == VALUE and "twk_get_refit_info" in L.lib.twk_last_error().decode()
    assert L.lib.twk_debug_read_kept_build(None, None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_size_t(0)) == VALUE and "twk_debug_read_kept_build" in L.lib.twk_last_error().decode()
    for method in ("refitGeometryVertices", "refitInfo", "debugReadKeptBuild"):
        assert callable(getattr(twk.Device, method))
    assert L.lib.twk_abi_version() == 9


def test_the_host_form_runs_clean_under_the_sanitizers(twk, tmp_path):
    """The 65- and the 257-primitive tree, world space and object space, refit to the noise deformation through the stand-alone program
    (tests/refit_host.cpp): it exits 0 with nothing on stderr, and what it computed has twk_refit_tree_host's bits. Nothing is loaded
    into Python under a sanitizer."""
    out = str(tmp_path / "refit_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"),
                    "-o", out, os.path.join(ROOT, "tests", "refit_host.cpp")], check=True)
    deformed = RS.deformed_meshes("noise")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    ran = 0
    for kind in RS.KINDS:
        rb, trees = built(kind)
        for t in trees:
            if t["slots"] not in (127, 257):  # the odd mix of 65 build primitives (127 triangles), the soup of 257
                continue
            a, i = deformed[t["geometry"]]
            nodes, wide, cost, slots = state_of(rb, t)
            case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
            with open(case, "wb") as f:
                f.write(np.array([t["nodes"], t["slots"], a.shape[0], t["nodeBase"], t["slotBase"], t["leafFlag"], max(t["instance"], 0), 1, 1], np.int32).tobytes())
                for array, kind_of in ((nodes, F32), (wide, F32), (cost, F32), (slots, F32), (t["flags"], np.int32), (a, F32), (i, U32),
                                       (t["transform"] if t["transform"] is not None else np.zeros(12), F32)):
                    f.write(np.ascontiguousarray(array, kind_of).tobytes())
            run = subprocess.run([out, case, result], capture_output=True, text=True, env=env)
            assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
            want = refit(twk, t, (nodes, wide, cost, slots), a, i)
            raw = np.fromfile(result, np.uint8)
            sizes = [64 * t["nodes"], 128 * t["nodes"], 4 * t["nodes"], 48 * t["slots"], 128 * t["slots"], 16, 24]
            assert raw.size == sum(sizes)
            parts = np.split(raw, np.cumsum(sizes)[:-1])
            for got, key in zip(parts[:5], ("nodes", "wideNodes", "nodeCost", "slots", "shadeRecords")):
                assert np.array_equal(got.view(U32), np.ascontiguousarray(want[key]).view(U32).reshape(-1)), f"{kind}, {t['name']}: {key}"
            assert np.array_equal(parts[5].view(np.float64), np.array(want["terms"])) and np.array_equal(parts[6].view(U32), want["rootBounds"].view(U32))
            ran += 1
    assert ran == 4
