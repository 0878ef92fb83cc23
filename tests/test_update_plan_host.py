"""CPU: twk_update_plan_host — the layout twk_build gives a scene and the plan of a selective update (csrc/update_plan.h), against
expectations written out by hand for the scenes of tests/selective_scenes.py; and the refusals of the new calls that need no device.

The hand calculation: a tree over n triangles reserves max(1, n - 1) nodes; the entered geometries' trees come first in geometry
order, then the flattened instances' in instance order, then the top level with max(1, instances - 1) nodes, then the two root slots."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import selective_scenes as S
from conftest import ROOT

# scene: (flattened flags, direct leaves, entered geometries, tlasBase, nodes, slots, {moved: (trees, topLevel, ranges, slotsRewritten)})
EXPECT = {
    # walls: nodes 0..3, slots 0..7; box: nodes 4..14, slots 8..19; sphere: nodes 15..61, slots 20..67; top level 62..66
    "flat": ([1] * 6, 4, 0, 62, 67, 68, {
        (5,): ([5], 1, [(15, 47), (62, 5), (67, 2)], 48),
        (1,): ([1], 1, [(1, 1), (62, 5), (67, 2)], 2),
        (5, 4): ([4, 5], 1, [(4, 11), (15, 47), (62, 5), (67, 2)], 60),
        (0, 1, 2, 3, 4, 5): ([0, 1, 2, 3, 4, 5], 1, [(0, 1), (1, 1), (2, 1), (3, 1), (4, 11), (15, 47), (62, 5), (67, 2)], 68)}),
    # bottom levels: the walls' nodes 0..3, the sphere's 4..50 (slots 8..55); top level 51..56
    "two-level": ([0] * 7, 0, 5, 51, 57, 56, {
        (5,): ([], 1, [(51, 6), (57, 2)], 0),
        (4, 6): ([], 1, [(51, 6), (57, 2)], 0),
        (0, 1, 2, 3, 4, 5, 6): ([], 1, [(51, 6), (57, 2)], 0)}),
    # the sphere's bottom level: nodes 0..46, slots 0..47; walls: nodes 47..50, slots 48..55; box (instance 7): nodes 51..61, slots 56..67; top 62..68
    "mixed": ([1, 1, 1, 1, 0, 0, 0, 1], 4, 1, 62, 69, 68, {
        (7,): ([7], 1, [(51, 11), (62, 7), (69, 2)], 12),
        (4,): ([], 1, [(62, 7), (69, 2)], 0),
        (7, 4): ([7], 1, [(51, 11), (62, 7), (69, 2)], 12),
        (0, 1, 2, 3, 4, 5, 6, 7): ([0, 1, 2, 3, 7], 1, [(47, 1), (48, 1), (49, 1), (50, 1), (51, 11), (62, 7), (69, 2)], 20)}),
    # the one tree: nodes 0..46; the top level's node 47 is reserved and never built
    "single": ([1], 0, 0, 47, 48, 48, {
        (0,): ([0], 0, [(0, 47), (48, 2)], 48)}),
    # walls: nodes 0..3; box k (instance 4 + k): nodes 4 + 11 k .. 14 + 11 k, slots 8 + 12 k ..; top level 136..150
    "many": ([1] * 16, 4, 0, 136, 151, 152, {
        (7,): ([7], 1, [(37, 11), (136, 15), (151, 2)], 12),
        (15, 4): ([4, 15], 1, [(4, 11), (125, 11), (136, 15), (151, 2)], 24)}),
}


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_plan_of_each_scene(twk, name):
    flattened, direct, entered, tlas, nodes, slots, moves = EXPECT[name]
    geometry = S.instance_geometry(name)
    layout = twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name))
    assert layout["flattened"] == [bool(f) for f in flattened]
    assert (layout["instances"], layout["flattenedInstances"], layout["directLeafInstances"], layout["enteredGeometries"]) == (len(geometry), sum(flattened), direct, entered)
    assert (layout["tlasBase"], layout["nodes"], layout["triangleSlots"]) == (tlas, nodes, slots)
    assert layout["numRanges"] == 0 and layout["ranges"] == [] and layout["nodesRequantised"] == 0, "no move, no plan"
    for moved, (trees, top, ranges, rewritten) in moves.items():
        plan = twk.Device.updatePlanHost(geometry, S.TRIANGLES, S.policy(name), moved)
        assert plan["trees"] == trees and plan["treesRebuilt"] == len(trees), moved
        assert plan["topLevelRebuilt"] == top, moved
        assert plan["ranges"] == ranges and plan["numRanges"] == len(ranges), moved
        assert plan["nodesRequantised"] == sum(n for _, n in ranges) and plan["slotsRewritten"] == rewritten, moved
        # disjoint and ascending, the root slots last
        for (a, n), (b, _) in zip(plan["ranges"], plan["ranges"][1:]):
            assert n >= 1 and a + n <= b, moved
        assert plan["ranges"][-1] == (nodes, 2), moved
        assert plan["flattened"] == layout["flattened"] and plan["nodes"] == nodes, "a move changes no layout"


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_every_instance_moved_plans_every_flattened_tree_and_no_bottom_level(twk, name):
    geometry = S.instance_geometry(name)
    plan = twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name), range(len(geometry)))
    assert plan["trees"] == [i for i, f in enumerate(plan["flattened"]) if f]
    tree_ranges = plan["ranges"][:len(plan["trees"])]
    # every range before the top level's belongs to a flattened instance: the bottom levels stand before the first of them
    bottom = sum(max(1, S.TRIANGLES[g] - 1) for g in sorted({g for g, f in zip(geometry, plan["flattened"]) if not f}))
    assert all(first >= bottom for first, _ in tree_ranges)
    assert sum(n for _, n in tree_ranges) == sum(max(1, S.TRIANGLES[g] - 1) for g, f in zip(geometry, plan["flattened"]) if f)
    assert plan["slotsRewritten"] == sum(S.TRIANGLES[g] for g, f in zip(geometry, plan["flattened"]) if f)


def test_max_leaf_decides_the_direct_leaves(twk):
    geometry = S.instance_geometry("flat")
    assert twk.update_plan_host(geometry, S.TRIANGLES, (4, 2), maxLeaf=1)["directLeafInstances"] == 0
    assert twk.update_plan_host(geometry, S.TRIANGLES, (4, 2), maxLeaf=2)["directLeafInstances"] == 4
    assert twk.update_plan_host(geometry, S.TRIANGLES, (4, 2), maxLeaf=2)["nodes"] == twk.update_plan_host(geometry, S.TRIANGLES, (4, 2), maxLeaf=1)["nodes"]


def test_the_meshes_have_the_triangles_the_table_says(twk):
    assert twk.mesh_box()[1].size // 3 == S.TRIANGLES[S.BOX]
    assert twk.mesh_sphere(8, 4, 1.0, np.pi)[1].size // 3 == S.TRIANGLES[S.SPHERE]


def test_refusals_without_a_device(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE

    def refused(rc, *words):
        text = L.lib.twk_last_error().decode()
        assert rc == VALUE, text
        for w in words:
            assert w in text, text

    refused(L.lib.twk_set_update_mode(None, L.TWK_UPDATE_SELECTIVE), "twk_set_update_mode", "NULL")
    ids, transforms = (C.c_int * 1)(0), (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    refused(L.lib.twk_update_instance_transforms(None, 1, ids, transforms), "twk_update_instance_transforms", "NULL device handle")
    refused(L.lib.twk_update_instance_transform(None, 0, transforms), "twk_update_instance_transform:", "NULL device handle")
    refused(L.lib.twk_get_update_info(None, None), "twk_get_update_info", "NULL")
    # the batch's own arguments are refused before the handle is looked at: no handle is needed, and none is passed
    refused(L.lib.twk_update_instance_transforms(None, 1, None, transforms), "twk_update_instance_transforms", "NULL array")
    refused(L.lib.twk_update_instance_transforms(None, 1, ids, None), "twk_update_instance_transforms", "NULL array")
    refused(L.lib.twk_update_instance_transforms(None, 0, ids, transforms), "twk_update_instance_transforms", "count")
    # the plan
    geometry = S.instance_geometry("flat")
    for moved, word in (((6,), "bad instance id"), ((-1,), "bad instance id"), ((5, 4, 5), "twice")):
        with pytest.raises(twk.TwkError) as e:
            twk.update_plan_host(geometry, S.TRIANGLES, (4, 2), moved)
        assert e.value.code == VALUE and "twk_update_plan_host" in str(e.value) and word in str(e.value) and "entry" in str(e.value)
    with pytest.raises(twk.TwkError) as e:
        twk.update_plan_host([0, 6], S.TRIANGLES, (4, 2))
    assert e.value.code == VALUE and "geometry index" in str(e.value)
    plan = L.UpdatePlan()
    refused(L.lib.twk_update_plan_host(None, 1, None, 1, 4, 2, 2, None, 0, C.byref(plan), None, None, None), "twk_update_plan_host", "NULL")


def test_the_plan_header_runs_clean_under_the_sanitizers(twk, tmp_path):
    """csrc/update_plan.h in a stand-alone program (tests/update_plan_host.cpp) under the address and undefined-behaviour sanitizers:
    it exits 0 with nothing on stderr, and its plans are twk_update_plan_host's."""
    out = str(tmp_path / "update_plan_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "update_plan_host.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = {line.split()[0]: line for line in r.stdout.strip().splitlines()}
    moved = {"flat": (5, 4), "two-level": (5,), "mixed": tuple(range(8)), "single": (0,), "many": (15, 4)}
    for name, ids in moved.items():
        plan = twk.update_plan_host(S.instance_geometry(name), S.TRIANGLES, S.policy(name), ids)
        want = (f"{name} nodes {plan['nodes']} slots {plan['triangleSlots']} tlas {plan['tlasBase']} trees {plan['treesRebuilt']} top {plan['topLevelRebuilt']} "
                f"total {plan['nodesRequantised']} rewritten {plan['slotsRewritten']} : " + " ".join(f"{a}+{n}" for a, n in plan["ranges"]))
        assert lines[name].strip() == want.strip(), name
    assert lines["one-triangle"].strip() == "one-triangle nodes 2 slots 1 tlas 1 trees 1 top 0 total 3 rewritten 1 : 0+1 2+2"
    assert lines["nothing-moved"].strip() == "nothing-moved nodes 4 slots 4 tlas 3 trees 0 top 1 total 3 rewritten 0 : 3+1 4+2"


def test_the_mirrors_have_the_headers_layouts(twk, tmp_path):
    """The ctypes mirrors UpdateInfo and UpdatePlan, and what tests/selective_scenes.py says of LaunchParams' leading fields and of
    the sizes of the scene arrays, against a program compiled from the headers (tests/selective_layout_host.cpp)."""
    L = twk._lib
    out = str(tmp_path / "selective_layout_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wno-unused-function", "-Wno-invalid-offsetof", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc,
                    "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", out,
                    os.path.join(ROOT, "tests", "selective_layout_host.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60, check=True)
    header = {name: int(value) for name, value in (line.split() for line in r.stdout.strip().splitlines())}

    class SceneHead(C.Structure):
        _fields_ = [(name, getattr(C, kind)) for name, kind in S.SCENE_HEAD]

    assert {f"LaunchParams.{name}": getattr(SceneHead, name).offset for name, _ in S.SCENE_HEAD} == {k: v for k, v in header.items() if k.startswith("LaunchParams.")}
    for name in ("NODE_BYTES", "SLOT_BYTES", "SHADE_RECORD_BYTES", "TOP_NODES", "TOP_NODES7", "QUANTISED_NODE_BYTES"):
        assert getattr(S, name) == header[name], name
    for cname, mirror in (("TwkUpdateInfo", L.UpdateInfo), ("TwkUpdatePlan", L.UpdatePlan)):
        want = {k.split(".", 1)[1]: v for k, v in header.items() if k.startswith(cname + ".")}
        assert C.sizeof(mirror) == want.pop("size"), cname
        assert {name: getattr(mirror, name).offset for name, _ in mirror._fields_} == want, cname
