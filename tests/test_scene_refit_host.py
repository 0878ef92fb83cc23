"""CPU: twk_scene_refit_plan_host (csrc/refit_scene_plan.h, the code twk_refit_scene plans its one batch with) against a plain-Python
restatement (tests/scene_refit_scenes.py restate, written from bvh_reference.scene_layout): the trees, their order, their kinds, their
node and slot ranges and refit_batch_plan.h's block tables, on refit_scenes' "flat" and "entered", the five selective_scenes and
"three-kinds", with hand-picked and seeded random edits; the refusals twk_refit_scene makes before any HIP call, in their order, also
through the Device methods on a closed handle; the
layout of TwkGeometryEdit and TwkSceneRefitPlan against the header; and the plan header through a stand-alone program built with
-fsanitize=address,undefined (tests/scene_refit_plan_host.cpp), whose output the library's host call must equal. Nothing is loaded
into Python under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scene_refit_scenes as SR
import selective_scenes as S
from conftest import ROOT

SCENES = SR.plan_scenes()


def _everything(name):
    gi, gt, _ = SCENES[name]
    return sorted(set(gi)), list(range(len(gi)))


def _cases(name):
    """[(updated, moved)]: everything, only geometries, only instances, halves, and four seeded random subsets."""
    geometries, instances = _everything(name)
    rng = np.random.default_rng(32 + sorted(SCENES).index(name))
    out = [(geometries, instances), (geometries, []), ([], instances), (geometries[::2], instances[1::2]), (geometries[-1:], instances[:1])]
    for _ in range(4):
        out.append(([g for g in range(len(SCENES[name][1])) if rng.random() < 0.5], [i for i in instances if rng.random() < 0.4]))
    return [(u, m) for u, m in out if u or m]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_plan_equals_its_restatement(twk, name):
    gi, gt, policy = SCENES[name]
    for updated, moved in _cases(name):
        what = f"{name}: updated {updated}, moved {moved}"
        got, want = twk.scene_refit_plan_host(gi, gt, policy, updated, moved), SR.restate(gi, gt, policy, updated, moved)
        SR.assert_plan(got, want, what)
        # the plan's slots are the vertex update plan's: what TwkUpdateInfo.slotsRewritten reports
        assert got["slotsRewritten"] == twk.vertex_update_plan_host(gi, gt, policy, updated, moved)["slotsRewritten"], what
        # ascending within either part, bottom-level trees first
        trees = [int(t) for t in got["trees"]]
        blas, flat = [~t for t in trees if t < 0], [t for t in trees if t >= 0]
        assert trees == [~g for g in blas] + flat and blas == sorted(blas) and flat == sorted(flat), what


def test_three_kinds_puts_every_kind_next_to_another(twk):
    gi, gt, policy = SCENES["three-kinds"]
    got = twk.scene_refit_plan_host(gi, gt, policy, SR.THREE_KINDS_EDITED, SR.THREE_KINDS_MOVED)
    assert [int(t) for t in got["trees"]] == [~S.SPHERE, 6, 7] and [int(k) for k in got["kinds"]] == [0, 1, 2]
    assert [int(n) for n in got["slotCounts"]] == [48, 12, 127] and [int(n) for n in got["nodeCounts"]] == [47, 11, 126]
    assert got["slotBlockTable"].tolist() == [[0, 0], [1, 0], [2, 0]] and got["nodeBlockTable"].tolist() == [[0, 0], [1, 0], [2, 0]]
    assert (got["directLeaves"], got["boxes"], got["slotBytes"]) == (0, 2, 176 * 60 + 48 * 127)
    # the box is edited AND moved: one tree, once; moving the walls too adds their rebuilds, not trees
    with_walls = twk.scene_refit_plan_host(gi, gt, policy, SR.THREE_KINDS_EDITED, (1, 2, 3) + SR.THREE_KINDS_MOVED)
    assert [int(t) for t in with_walls["trees"]] == [~S.SPHERE, 6, 7] and with_walls["directLeaves"] == 3 and with_walls["slotsRewritten"] == got["slotsRewritten"] + 6


def test_an_edit_of_the_box_of_many_is_twelve_trees_of_kind_one(twk):
    gi, gt, policy = SCENES["many"]
    got = twk.scene_refit_plan_host(gi, gt, policy, (S.BOX,), ())
    assert [int(t) for t in got["trees"]] == list(range(4, 16)) and [int(k) for k in got["kinds"]] == [1] * 12
    assert got["nodeBlocks"] == got["slotBlocks"] == 12 and got["slotBytes"] == 176 * 144
    moved_only = twk.scene_refit_plan_host(gi, gt, policy, (), range(4, 16))
    assert [int(k) for k in moved_only["kinds"]] == [2] * 12 and moved_only["slotBytes"] == 48 * 144


def test_the_meshes_cover_the_block_edges(twk):
    """refit_scenes' "flat" with everything edited: trees of 256 nodes / 257 slots (a second slot block with one live thread) and of more than 1024."""
    gi, gt, policy = SCENES["meshes-flat"]
    got = twk.scene_refit_plan_host(gi, gt, policy, range(len(gt)), range(len(gi)))
    slots = [int(s) for s in got["slotCounts"]]
    assert 257 in slots and max(slots) > 1025 and got["directLeaves"] == 2
    k = slots.index(257)
    mine = got["slotBlockTable"][got["slotBlockTable"][:, 0] == k]
    assert mine[:, 1].tolist() == [0, 256] and int(got["nodeCounts"][k]) == 256


def test_the_plans_refusals(twk):
    L = twk._lib
    gi, gt, policy = SCENES["mixed"]
    for kwargs, word in ((dict(updated=(len(gt),)), "bad geometry id"), (dict(updated=(S.BOX, S.BOX)), "listed twice"), (dict(moved=(len(gi),)), "bad instance id"),
                         (dict(moved=(4, 4)), "listed twice")):
        with pytest.raises(twk.TwkError) as e:
            twk.scene_refit_plan_host(gi, gt, policy, **kwargs)
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_scene_refit_plan_host:" in str(e.value) and word in str(e.value), str(e.value)
    assert L.lib.twk_scene_refit_plan_host(*([None, 0, None, 0, 0, 0, 2, None, 0, None, 0] + [None] * 13)) == L.TWK_ERROR_INVALID_VALUE
    assert "twk_scene_refit_plan_host" in L.lib.twk_last_error().decode()


def test_refit_scene_refuses_its_own_arguments_and_a_null_handle_before_any_hip_call(twk):
    """The order: the call's own arguments (without the handle being looked at), then the handle."""
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE
    edits = (L.GeometryEdit * 1)()
    ids = (C.c_int * 1)(0)
    t = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    call = L.lib.twk_refit_scene
    for args, word in (((None, -1, edits, 1, ids, t), "counts"), ((None, 1, edits, -1, ids, t), "counts"), ((None, 0, None, 0, None, None), "both counts are 0"),
                       ((None, 1, None, 0, None, None), "NULL array of geometry entries"), ((None, 0, None, 1, None, t), "NULL array of ids or transforms"),
                       ((None, 0, None, 1, ids, None), "NULL array of ids or transforms"), ((None, 1, edits, 1, ids, t), "NULL device handle")):
        assert call(*args) == VALUE, args
        text = L.lib.twk_last_error().decode()
        assert text.startswith("twk_refit_scene: ") and word in text, text
    assert callable(twk.scene_refit_plan_host) and L.lib.twk_abi_version() == 9


def test_the_device_methods_on_a_closed_handle(twk):
    """Device.close() leaves a NULL handle behind; such a Device needs no GPU to be made. The call's own arguments are still refused
    first, then the handle, each under the call's name, before any HIP call."""
    L = twk._lib
    dev = object.__new__(twk.Device)
    dev._h = C.c_void_p()  # what close() leaves
    records = np.zeros((4, 12), np.float32)
    identity = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    for call, words in ((lambda: dev.refitScene([(0, records)], [0], [identity]), ("twk_refit_scene: NULL device handle",)),
                        (lambda: dev.refitScene([(0, records)]), ("twk_refit_scene: NULL device handle",)),
                        (lambda: dev.refitScene([], [0], [identity]), ("twk_refit_scene: NULL device handle",)),
                        (lambda: dev.refitScene(), ("twk_refit_scene: ", "both counts are 0")),
                        (dev.refitInfo, ("twk_get_refit_info",)), (dev.updateInfo, ("twk_get_update_info",))):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        dev.refitScene([], [0, 1], [identity])  # 12 floats per id: refused before the library is called


def _header_fields(text, name):
    """The field names of `typedef struct name { ... } name;`: per declaration the identifiers its comma-separated declarators end in."""
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            first, *more = decl.split(",")
            fields += [re.search(r"(\w+)\s*(\[.*\])?$", part.strip()).group(1) for part in [first] + more]
    return fields


def test_the_new_structs_have_the_headers_layout(twk, tmp_path):
    L = twk._lib
    pairs = [("TwkGeometryEdit", L.GeometryEdit), ("TwkSceneRefitPlan", L.SceneRefitPlan)]
    header = os.path.join(ROOT, "include", "tweeker_hip.h")
    text = open(header).read()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void) {"]
    for cname, _ in pairs:
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in _header_fields(text, cname):
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    layout = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        struct, field, value = line.split()
        layout.setdefault(struct, {})[field] = int(value)
    for cname, mirror in pairs:
        assert C.sizeof(mirror) == layout[cname].pop("size"), cname
        assert {name: getattr(mirror, name).offset for name, *_ in mirror._fields_} == layout[cname], cname
    assert C.sizeof(L.GeometryEdit) == 32 and L.GeometryEdit.numVertices.offset == 8 and L.GeometryEdit.attributes.offset == 16 and L.GeometryEdit.source.offset == 24


# trees of 1, 256 and 257 nodes as bottom-level trees (a flattened instance of two triangles would be a direct leaf), and one tree alone
DEGENERATE = ([0, 0, 1, 1, 2, 2], [2, 257, 258], (0, 1))


def test_the_plan_header_runs_clean_under_the_sanitizers(twk, tmp_path):
    exe = str(tmp_path / "scene_refit_plan_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "scene_refit_plan_host.cpp")], check=True)
    cases = [(name, SCENES[name], u, m) for name in sorted(SCENES) for u, m in _cases(name)]
    cases += [("degenerate", DEGENERATE, [0, 1, 2], []), ("degenerate", DEGENERATE, [1], []), ("degenerate", DEGENERATE, [0], [0])]
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for _, (gi, gt, policy), updated, moved in cases:
            f.write(" ".join(str(int(x)) for x in [len(gi), len(gt), policy[0], policy[1], 2, len(moved), len(updated)] + list(gi) + list(gt) + list(moved) + list(updated)) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    blocks = run.stdout.split("case ")[1:]
    assert run.stdout.strip().endswith(f"cases {len(cases)}") and len(blocks) == len(cases)
    for block, (name, (gi, gt, policy), updated, moved) in zip(blocks, cases):
        rows = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in block.splitlines()[1:] if not line.startswith("cases")}
        got = twk.scene_refit_plan_host(gi, gt, policy, updated, moved)
        what = f"{name}: updated {updated}, moved {moved}"
        assert rows["totals"] == [got[k] for k in ("numTrees", "nodeBlocks", "slotBlocks", "blockThreads", "directLeaves", "topLevelRebuilt", "nodes", "slots", "slotsRewritten", "slotBytes")], what
        for key in SR.TABLES:
            assert rows[key] == np.asarray(got[key]).reshape(-1).tolist(), (what, key)
        want = SR.restate(gi, gt, policy, updated, moved)
        assert rows["directLeafInstances"] == want["directLeafInstances"] and rows["boxInstances"] == want["boxInstances"] and got["boxes"] == len(want["boxInstances"]), what
        if name == "degenerate" and len(updated) == 3:
            assert rows["nodeCounts"] == [1, 256, 257] and rows["kinds"] == [0, 0, 0] and rows["nodeBlockTable"] == [0, 0, 1, 0, 2, 0, 2, 256]
