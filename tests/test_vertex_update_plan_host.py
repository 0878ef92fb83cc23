"""CPU: twk_vertex_update_plan_host — the plan of a vertex update (csrc/update_plan.h updatePlanWith), against expectations written
out by hand for the scenes of tests/selective_scenes.py; the refusals of the new calls that need no device; the structs against the
header.

The hand calculation is tests/test_update_plan_host.py's: a tree over n triangles reserves max(1, n - 1) nodes; the entered
geometries' trees come first in geometry order, then the flattened instances' in instance order, then the top level with
max(1, instances - 1) nodes, then the two root slots. A vertex update of geometry g rebuilds g's bottom-level tree if some instance
enters g (listed as ~g), the world box of every entered instance of g, and the tree of every flattened instance of g."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import selective_scenes as S
from conftest import ROOT

B = lambda g: ~g  # a bottom-level tree in `trees`

# scene: (nodes, {(updated geometries, moved instances): (trees, entered boxes, topLevel, ranges, slotsRewritten)})
EXPECT = {
    # walls: nodes 0..3, slots 0..7; box: nodes 4..14, slots 8..19; sphere: nodes 15..61, slots 20..67; top level 62..66
    "flat": (67, {
        ((S.SPHERE,), ()): ([5], [], 1, [(15, 47), (62, 5), (67, 2)], 48),
        ((S.BOX,), ()): ([4], [], 1, [(4, 11), (62, 5), (67, 2)], 12),
        ((S.FLOOR,), ()): ([1], [], 1, [(1, 1), (62, 5), (67, 2)], 2),          # a direct leaf: its one-node range
        ((S.SPHERE,), (5,)): ([5], [], 1, [(15, 47), (62, 5), (67, 2)], 48),     # moved and deformed: one tree, once
        ((S.SPHERE, S.BOX), (1,)): ([1, 4, 5], [], 1, [(1, 1), (4, 11), (15, 47), (62, 5), (67, 2)], 62)}),
    # bottom levels: the walls' nodes 0..3, the sphere's 4..50 (slots 8..55); the box geometry has no instance and no tree; top level 51..56
    "two-level": (57, {
        ((S.SPHERE,), ()): ([B(S.SPHERE)], [4, 5, 6], 1, [(4, 47), (51, 6), (57, 2)], 48),
        ((S.FLOOR,), ()): ([B(S.FLOOR)], [1], 1, [(1, 1), (51, 6), (57, 2)], 2),
        ((S.BOX,), ()): ([], [], 1, [(51, 6), (57, 2)], 0),
        ((S.SPHERE,), (5,)): ([B(S.SPHERE)], [4, 5, 6], 1, [(4, 47), (51, 6), (57, 2)], 48)}),
    # the sphere's bottom level: nodes 0..46, slots 0..47; walls: nodes 47..50; box (instance 7): nodes 51..61, slots 56..67; top 62..68
    "mixed": (69, {
        ((S.SPHERE,), ()): ([B(S.SPHERE)], [4, 5, 6], 1, [(0, 47), (62, 7), (69, 2)], 48),
        ((S.BOX,), ()): ([7], [], 1, [(51, 11), (62, 7), (69, 2)], 12),
        ((S.BOX, S.SPHERE), ()): ([B(S.SPHERE), 7], [4, 5, 6], 1, [(0, 47), (51, 11), (62, 7), (69, 2)], 60),
        ((S.SPHERE,), (7, 4)): ([B(S.SPHERE), 7], [4, 5, 6], 1, [(0, 47), (51, 11), (62, 7), (69, 2)], 60)}),
    # the one tree: nodes 0..46; no top level
    "single": (48, {
        ((S.SPHERE,), ()): ([0], [], 0, [(0, 47), (48, 2)], 48)}),
    # walls: nodes 0..3; box k (instance 4 + k): nodes 4 + 11 k ..; top level 136..150
    "many": (151, {
        ((S.BOX,), ()): (list(range(4, 16)), [], 1, [(4 + 11 * k, 11) for k in range(12)] + [(136, 15), (151, 2)], 144)}),
}


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_vertex_plan_of_each_scene(twk, name):
    nodes, updates = EXPECT[name]
    geometry = S.instance_geometry(name)
    layout = twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name))
    nothing = twk.vertex_update_plan_host(geometry, S.TRIANGLES, S.policy(name))
    assert nothing == layout, "no update, no move: the layout only, as twk_update_plan_host gives it"
    for (updated, moved), (trees, _, top, ranges, rewritten) in updates.items():
        what = f"{name}: updated {updated}, moved {moved}"
        plan = twk.vertex_update_plan_host(geometry, S.TRIANGLES, S.policy(name), updated, moved)
        assert plan["trees"] == trees and plan["treesRebuilt"] == len(trees), what
        assert plan["topLevelRebuilt"] == top, what
        assert plan["ranges"] == ranges and plan["numRanges"] == len(ranges), what
        assert plan["nodesRequantised"] == sum(n for _, n in ranges) and plan["slotsRewritten"] == rewritten, what
        for (a, n), (b, _) in zip(plan["ranges"], plan["ranges"][1:]):
            assert n >= 1 and a + n <= b, what + ": ascending and disjoint"
        assert plan["ranges"][-1] == (nodes, 2), what
        assert plan["flattened"] == layout["flattened"] and plan["nodes"] == nodes == layout["nodes"], "an update changes no layout"
        if not updated:
            continue
        # a bottom-level range lies before every flattened one
        bottom = [r for t, r in zip(plan["trees"], plan["ranges"]) if t < 0]
        flat = [r for t, r in zip(plan["trees"], plan["ranges"]) if t >= 0]
        assert all(b[0] + b[1] <= f[0] for b in bottom for f in flat), what


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_without_updated_geometries_it_is_the_transform_plan(twk, name):
    geometry = S.instance_geometry(name)
    for moved in ([S.first_movable(name)], list(range(len(geometry)))):
        assert twk.vertex_update_plan_host(geometry, S.TRIANGLES, S.policy(name), (), moved) == twk.update_plan_host(geometry, S.TRIANGLES, S.policy(name), moved)


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_every_geometry_updated_plans_every_tree(twk, name):
    geometry = S.instance_geometry(name)
    plan = twk.vertex_update_plan_host(geometry, S.TRIANGLES, S.policy(name), range(len(S.TRIANGLES)))
    entered = sorted({g for g, f in zip(geometry, plan["flattened"]) if not f})
    assert plan["trees"] == [~g for g in entered] + [i for i, f in enumerate(plan["flattened"]) if f]
    assert plan["slotsRewritten"] == plan["triangleSlots"] and plan["nodesRequantised"] == plan["nodes"] + 2 - (0 if plan["topLevelRebuilt"] else 1)


def test_refusals_without_a_device(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE

    def refused(rc, *words):
        text = L.lib.twk_last_error().decode()
        assert rc == VALUE, text
        for w in words:
            assert w in text, text

    attributes = (C.c_float * 12)()
    refused(L.lib.twk_update_geometry_vertices(None, 0, attributes, C.c_size_t(1)), "twk_update_geometry_vertices", "NULL device handle")
    refused(L.lib.twk_render_geometry_motion(None), "twk_render_geometry_motion", "NULL device handle")
    refused(L.lib.twk_get_geometry_deformed(None, 0, None), "twk_get_geometry_deformed", "NULL")
    geometry = S.instance_geometry("flat")
    for updated, word in (((6,), "bad geometry id"), ((-1,), "bad geometry id"), ((5, 4, 5), "twice")):
        with pytest.raises(twk.TwkError) as e:
            twk.vertex_update_plan_host(geometry, S.TRIANGLES, (4, 2), updated)
        assert e.value.code == VALUE and "twk_vertex_update_plan_host" in str(e.value) and word in str(e.value) and "updated entry" in str(e.value)
    for moved, word in (((6,), "bad instance id"), ((5, 5), "twice")):
        with pytest.raises(twk.TwkError) as e:
            twk.vertex_update_plan_host(geometry, S.TRIANGLES, (4, 2), (5,), moved)
        assert e.value.code == VALUE and "twk_vertex_update_plan_host" in str(e.value) and word in str(e.value)
    with pytest.raises(twk.TwkError) as e:
        twk.vertex_update_plan_host([0, 6], S.TRIANGLES, (4, 2), (5,))
    assert e.value.code == VALUE and "geometry index" in str(e.value)
    plan = L.UpdatePlan()
    ids = (C.c_int * 1)(0)
    refused(L.lib.twk_vertex_update_plan_host(None, 1, None, 1, 4, 2, 2, None, 0, ids, 1, C.byref(plan), None, None, None), "twk_vertex_update_plan_host", "NULL")
    ig, gt = (C.c_int * 1)(0), (C.c_int * 1)(2)
    refused(L.lib.twk_vertex_update_plan_host(ig, 1, gt, 1, 4, 2, 2, None, 0, None, 1, C.byref(plan), None, None, None), "twk_vertex_update_plan_host", "NULL")
    refused(L.lib.twk_vertex_update_plan_host(ig, 1, gt, 1, 4, 2, 2, None, 0, ids, -1, C.byref(plan), None, None, None), "twk_vertex_update_plan_host", "counts")


def test_the_plan_runs_clean_under_the_sanitizers(twk, tmp_path):
    """updatePlanWith in a stand-alone program (tests/vertex_update_plan_host.cpp) under the address and undefined-behaviour
    sanitizers: it exits 0 with nothing on stderr, its plans are twk_vertex_update_plan_host's, and its entered boxes — which the C
    struct does not carry — are the hand-written ones."""
    out = str(tmp_path / "vertex_update_plan_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "vertex_update_plan_host.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = {line.split()[0]: line.strip() for line in r.stdout.strip().splitlines()}

    def line(label, scene, updated, moved, boxes):
        plan = twk.vertex_update_plan_host(S.instance_geometry(scene), S.TRIANGLES, S.policy(scene), updated, moved)
        words = [label, "geometries"] + [str(~t) for t in plan["trees"] if t < 0] + ["boxes"] + [str(i) for i in boxes] + ["trees"] + [str(t) for t in plan["trees"] if t >= 0]
        words += ["top", str(plan["topLevelRebuilt"]), "total", str(plan["nodesRequantised"]), "rewritten", str(plan["slotsRewritten"]), ":"] + [f"{a}+{n}" for a, n in plan["ranges"]]
        return " ".join(words)

    assert lines["flat"] == line("flat", "flat", (5,), (), EXPECT["flat"][1][((5,), ())][1])
    assert lines["two-level"] == line("two-level", "two-level", (5,), (), [4, 5, 6])
    assert lines["mixed"] == line("mixed", "mixed", (4, 5), (), [4, 5, 6])
    assert lines["mixed-moved"] == line("mixed-moved", "mixed", (5,), (7, 4), [4, 5, 6])
    assert lines["single"] == line("single", "single", (5,), (), [])
    assert lines["many"] == line("many", "many", (4,), (), [])
    assert lines["unreferenced"] == line("unreferenced", "two-level", (4,), (), [])
    assert lines["one-triangle"] == "one-triangle geometries boxes trees 0 top 0 total 3 rewritten 1 : 0+1 2+2"
    assert lines["nothing"] == "nothing geometries boxes trees top 1 total 3 rewritten 0 : 3+1 4+2"
    # the hand-written boxes of EXPECT are the ones compared above
    assert EXPECT["two-level"][1][((S.SPHERE,), ())][1] == [4, 5, 6] and EXPECT["mixed"][1][((S.SPHERE,), ())][1] == [4, 5, 6]


def test_the_mirrors_have_the_headers_layouts(twk, tmp_path):
    """The ctypes mirrors UpdateInfo, UpdatePlan, InstanceMotion and InstanceCarry against a program compiled from the public header
    (tests/vertex_update_layout_host.cpp); a vertex is twelve floats."""
    L = twk._lib
    out = str(tmp_path / "vertex_update_layout_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "vertex_update_layout_host.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60, check=True)
    header = {name: int(value) for name, value in (line.split() for line in r.stdout.strip().splitlines())}
    for cname, mirror in (("TwkUpdateInfo", L.UpdateInfo), ("TwkUpdatePlan", L.UpdatePlan), ("TwkInstanceMotion", L.InstanceMotion), ("TwkInstanceCarry", L.InstanceCarry)):
        want = {k.split(".", 1)[1]: v for k, v in header.items() if k.startswith(cname + ".")}
        assert C.sizeof(mirror) == want.pop("size"), cname
        assert {name: getattr(mirror, name).offset for name, _ in mirror._fields_} == want, cname
    assert header["TwkInstanceCarry.size"] == 64 and header["TwkTriangleAttributes.size"] == 48 == 12 * np.dtype(np.float32).itemsize
