#!/usr/bin/env python3
"""Cost of an instance-transform update in selective mode beside full mode (include/tweeker_hip.h "Selective instance updates"), in
the form of tools/temporal_motion_time.py `update`: TwkBuildInfo.buildMilliseconds (host wall time, uploads and synchronisations
included) of three updates in a row that lift one sphere by 0.05 each.

Configurations: the Cornell box (C2); the C2 room with the spheres tessellated 1000 x 500 (2.0 M triangles), flattened and two-level;
and a batch of 8 instances of scenes/scene_rtigo3_instances.txt in one twk_update_instance_transforms. Per configuration: selective
mode and full mode on handles of one process, and — with `parent=<path to a libtweeker_hip.so built from the parent commit>` — the
same full update through that library, in a child process. The measuring core speaks to the library with ctypes alone, so that one
code path serves all three. Also printed: keptBytes, what the update touched, and the floor of the ranged tail's compulsory bytes
(192 B per requantised node at the stream-copy rate twk_stream_peak_gbps reports in the same process), and the default bench.py line,
three runs; the kernel's own time comes from a kernel trace of `tail` (one selective update of the flattened room, nothing else).

usage (GPU box): python tools/selective_update_time.py [parent=<lib>] > table.md
                 python tools/selective_update_time.py tail            (under a kernel trace)"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
DEFAULT_LIB = os.path.join(ROOT, "tweeker_raytracer_amd", "libtweeker_hip.so")
UPDATES = 3


class BuildInfo(C.Structure):
    _fields_ = [("quality", C.c_int), ("trees", C.c_int), ("sahInnerCost", C.c_double), ("sahLeafCost", C.c_double), ("buildMilliseconds", C.c_double),
                ("triangleSlots", C.c_uint64), ("nodes", C.c_uint64), ("instances", C.c_uint64), ("flattenedInstances", C.c_uint64), ("maxTraversalDepth", C.c_uint64),
                ("directLeafInstances", C.c_uint64), ("traceBlocksPerCU", C.c_uint64), ("wide8Nodes", C.c_uint64), ("wide8Levels", C.c_uint64),
                ("pairLeaves", C.c_uint64), ("pairTriangles", C.c_uint64)]


class UpdateInfo(C.Structure):
    _fields_ = [("selective", C.c_int), ("instancesMoved", C.c_int), ("treesRebuilt", C.c_int), ("topLevelRebuilt", C.c_int), ("nodesRequantised", C.c_uint64),
                ("slotsRewritten", C.c_uint64), ("instanceRecordsUploaded", C.c_uint64), ("keptBytes", C.c_uint64), ("milliseconds", C.c_double)]


def configurations():
    system = open(os.path.join(SCENES, "system_rtigo3_cornell_box.txt")).read()
    scene = open(os.path.join(SCENES, "scene_rtigo3_cornell_box.txt")).read()
    room = scene.replace("sphere 180 90", "sphere 1000 500")
    instanced = (open(os.path.join(SCENES, "system_rtigo3_instances.txt")).read(), open(os.path.join(SCENES, "scene_rtigo3_instances.txt")).read())
    return [("C2", system, scene, None, 1), ("C2 room 2.0 M, flattened", system, room, None, 1), ("C2 room 2.0 M, two-level", system, room, (0, 0), 1),
            ("instanced scene, batch of 8", instanced[0], instanced[1], None, 8)]


def measure(lib_path, selective, only=None):
    """[{name, build ms, update ms x UPDATES, info}] through the library at lib_path; selective needs the new calls."""
    lib = C.CDLL(lib_path)
    lib.twk_last_error.restype = C.c_char_p

    def ok(rc):
        assert rc == 0, lib.twk_last_error().decode()

    rows = []
    for name, system, scene, flatten, moves in configurations():
        if only is not None and name != only:
            continue
        app, dev = C.c_void_p(), C.c_void_p()
        ok(lib.twk_app_create_from_strings(C.byref(app), system.encode(), scene.encode()))
        ok(lib.twk_app_set_resolution(app, 256, 256))
        app_info = (C.c_int * 64)()  # TwkAppInfo: strategy, devicesMask, light, miss, ...
        ok(lib.twk_app_info(app, app_info))
        ok(lib.twk_device_create(C.byref(dev), 0, 0, 1, app_info[3]))
        if selective:
            ok(lib.twk_set_update_mode(dev, 1))
        ok(lib.twk_app_init_device(app, dev))
        if flatten is not None:
            ok(lib.twk_set_flatten_policy(dev, *flatten))
            ok(lib.twk_build(dev))
        info = BuildInfo()
        ok(lib.twk_get_build_info(dev, C.byref(info)))
        built = info.buildMilliseconds
        # the instances to move: those with the most triangles that carry no light (the spheres; the instanced scene's objects)
        candidates = []
        for i in range(int(info.instances)):
            g, m, l, t = C.c_int(0), C.c_int(0), C.c_int(0), (C.c_float * 12)()
            ok(lib.twk_app_get_instance(app, i, C.byref(g), t, C.byref(m), C.byref(l)))
            na, ni = C.c_size_t(0), C.c_size_t(0)
            ok(lib.twk_app_get_geometry_sizes(app, g.value, C.byref(na), C.byref(ni)))
            if l.value < 0:
                candidates.append((-ni.value, i))
        ids = [i for _, i in sorted(candidates)[:moves]]
        transforms = (C.c_float * (12 * len(ids)))()
        for k, i in enumerate(ids):
            ok(lib.twk_get_instance_transform(dev, i, C.cast(C.byref(transforms, 48 * k), C.POINTER(C.c_float))))
        times, update = [], UpdateInfo()
        for _ in range(UPDATES):
            for k in range(len(ids)):
                transforms[12 * k + 7] += 0.05
            if len(ids) == 1:
                ok(lib.twk_update_instance_transform(dev, ids[0], transforms))
            elif hasattr(lib, "twk_update_instance_transforms"):
                ok(lib.twk_update_instance_transforms(dev, len(ids), (C.c_int * len(ids))(*ids), transforms))
            else:  # the parent has no batch call: one rebuild per move, summed
                total = 0.0
                for k, i in enumerate(ids):
                    ok(lib.twk_update_instance_transform(dev, i, C.cast(C.byref(transforms, 48 * k), C.POINTER(C.c_float))))
                    ok(lib.twk_get_build_info(dev, C.byref(info)))
                    total += info.buildMilliseconds
                times.append(total)
                continue
            ok(lib.twk_get_build_info(dev, C.byref(info)))
            times.append(info.buildMilliseconds)
        row = {"name": name, "slots": int(info.triangleSlots), "nodes": int(info.nodes), "build": built, "updates": times}
        if hasattr(lib, "twk_get_update_info"):
            ok(lib.twk_get_update_info(dev, C.byref(update)))
            row.update({f: getattr(update, f) for f, _ in UpdateInfo._fields_})
            peak = C.c_float(0)
            ok(lib.twk_stream_peak_gbps(dev, C.c_size_t(1 << 30), 10, C.byref(peak)))
            row["peak"] = peak.value
        rows.append(row)
        ok(lib.twk_device_destroy(dev))
        lib.twk_app_destroy(app)
    return rows


def main():
    args = sys.argv[1:]
    if args and args[0] == "child":  # child <lib> <selective 0|1>: one JSON line
        print(json.dumps(measure(args[1], args[2] == "1")))
        return 0
    if args and args[0] == "tail":
        rows = measure(DEFAULT_LIB, True, only="C2 room 2.0 M, flattened")
        print(json.dumps(rows))
        return 0
    parent = next((a.split("=", 1)[1] for a in args if a.startswith("parent=")), None)

    def child(lib, selective):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", lib, "1" if selective else "0"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        return {r["name"]: r for r in json.loads(out.stdout.strip().splitlines()[-1])}

    selective, full = child(DEFAULT_LIB, True), child(DEFAULT_LIB, False)
    old = child(parent, False) if parent else {}
    ms = lambda xs: ", ".join(f"{x:.2f}" for x in xs)
    print(f"buildMilliseconds of {UPDATES} updates in a row, host wall time; each column a process of its own on the same GPU.\n")
    print("| configuration | triangle slots | twk_build ms (full mode) | selective update ms | full update ms | parent commit's update ms |")
    print("|---|---|---|---|---|---|")
    for name, s in selective.items():
        f = full[name]
        print(f"| {name} | {s['slots']} | {f['build']:.1f} | {ms(s['updates'])} | {ms(f['updates'])} | {ms(old[name]['updates']) if name in old else 'not measured'} |")
    print("\n| configuration | keptBytes | trees rebuilt | nodes requantised of all | slots rewritten of all | ranged tail's compulsory bytes | floor at the stream-copy rate |")
    print("|---|---|---|---|---|---|---|")
    for name, s in selective.items():
        nbytes = 192 * s["nodesRequantised"]
        print(f"| {name} | {s['keptBytes']} ({s['keptBytes'] / 2 ** 20:.1f} MiB) | {s['treesRebuilt']} | {s['nodesRequantised']} of {s['nodes'] + 2} | {s['slotsRewritten']} of {s['slots']} | "
              f"{nbytes} | {nbytes / (s['peak'] * 1e9) * 1e6:.2f} us at {s['peak']:.0f} GB/s |")
    # the default bench line, three runs: no timed kernel changes, so it must lie inside the parent's spread (profiles/r23_temporal_motion.md)
    print("\n`python bench.py --gpus 1`, Msamples/s: ", end="")
    values = []
    for _ in range(3):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stdout + out.stderr
        values.append(json.loads(out.stdout.strip().splitlines()[-1])["value"])
    print(", ".join(f"{v:.0f}" for v in values))
    return 0


if __name__ == "__main__":
    sys.exit(main())
