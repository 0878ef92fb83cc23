#!/usr/bin/env python3
"""Cost and quality of the refit of a moved instance (include/tweeker_hip.h "Refit of a moved instance") beside the selective
transform update it stands in for, the full rebuild, and the vertex refit of the same tree.

Time: host clock around the synchronising call, one warm-up round, then RUNS rounds in which the calls alternate in one process, the
mirror sphere stepped a little each time: twk_refit_instance_transform and twk_update_instance_transform on ONE selective handle,
twk_refit_geometry_vertices (the same tree, the same vertices) on it too, twk_update_instance_transform on a full-mode handle.
Configurations: the Cornell box (C2; the sphere has 32 040 triangles, flattened) and the C2 room with the spheres tessellated
1000 x 500 (2.0 M triangles), flattened and two-level (there the sphere is entered: all three calls move a world box).

Batch: eight flattened instances of one 32 040-triangle sphere moved by one twk_refit_instance_transforms call, by eight
twk_refit_instance_transform calls, and by one twk_update_instance_transforms call.

Kernels: a child of this tool under `rocprofv3 --kernel-trace` refits the moved C2 sphere RUNS + 1 times; the durations of the
batch's four kernels stand beside the stream-copy floor (twk_stream_peak_gbps, same process) of the compulsory bytes of
refitSceneSlotsKernel on a moved tree: 48 B written per slot, 3 x 12 B of positions and 12 B of indices read.

Quality: sahNow / sahBuilt after each of four moves of the C2 sphere (a translation by 1e4, a rotation with unequal scales, a mirror,
a squash of one axis to 1e-3) and after 100 rotation steps of 3.6 degrees; and a 1920 x 1080 sample pass on the refit handle over
that on a handle REBUILT with the same transform, passes alternating.

usage (GPU box): python tools/instance_refit_time.py [--no-room] [--no-kernels] > table.md"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tweeker_raytracer_amd as twk  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
RUNS = 5
SPHERE = 6  # the mirror sphere's instance in the Cornell box


def clock(call):
    start = time.perf_counter()
    call()
    return 1.0e3 * (time.perf_counter() - start)


def med(values):
    return f"{statistics.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def texts():
    system = open(os.path.join(SCENES, "system_rtigo3_cornell_box.txt")).read()
    scene = open(os.path.join(SCENES, "scene_rtigo3_cornell_box.txt")).read()
    return system, scene, scene.replace("sphere 180 90", "sphere 1000 500")


def device(app, selective=True, flatten=None):
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE if selective else twk._lib.TWK_UPDATE_FULL)
    if flatten is not None:
        dev.setFlattenPolicy(*flatten)
    app.initDevice(dev)
    dev.build()
    return dev


def stepped(transform, k):
    t = np.array(transform, np.float32).reshape(12).copy()
    t[[3, 7, 11]] += np.float32(0.002) * np.array([1.0, 0.5, -0.5], np.float32) * (1 + k % 3)
    return t


def turned(transform, degrees, scale=(1.0, 1.0, 1.0)):
    """The transform with its linear part turned about y and scaled, the position kept."""
    m = np.array(transform, np.float64).reshape(3, 4)
    a = np.radians(degrees)
    r = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.diag(scale)
    return np.concatenate([m[:, :3] @ r, m[:, 3:]], 1).astype(np.float32).reshape(12)


def times(room_too):
    system, scene, room = texts()
    print("| configuration | instance refit ms | selective transform update ms | full rebuild ms | vertex refit of the same tree ms | refit / selective update | trees refit | nodes refit | slots rewritten |")
    print("|---|---|---|---|---|---|---|---|---|")
    rows = [("C2", scene, None)] + ([("C2 room 2.0 M, flattened", room, None), ("C2 room 2.0 M, two-level", room, (0, 0))] if room_too else [])
    for name, text, flatten in rows:
        app = twk.Application(system_text=system, scene_text=text)
        app.setResolution(256, 256)
        geometry, base = app.instance(SPHERE)[0], app.instance(SPHERE)[1]
        attributes = np.array(app.geometry(geometry)[0], np.float32)
        dev, full = device(app, True, flatten), device(app, False, flatten)
        out = {"refit": [], "update": [], "full": [], "vertex": []}
        info = None
        for run in range(RUNS + 1):
            ms = {}
            ms["refit"] = clock(lambda: dev.refitInstanceTransform(SPHERE, stepped(base, 2 * run)))
            info = dev.refitInfo()
            ms["update"] = clock(lambda: dev.updateInstanceTransform(SPHERE, stepped(base, 2 * run + 1)))
            ms["vertex"] = clock(lambda: dev.refitGeometryVertices(geometry, attributes))
            ms["full"] = clock(lambda: full.updateInstanceTransform(SPHERE, stepped(base, 2 * run)))
            if run:  # the first round warms up
                for key in out:
                    out[key].append(ms[key])
        print(f"| {name} | {med(out['refit'])} | {med(out['update'])} | {med(out['full'])} | {med(out['vertex'])} | {statistics.median(out['refit']) / statistics.median(out['update']):.2f} | "
              f"{info['treesRefit']} | {info['nodesRefit']} | {info['slotsRewritten']} |", flush=True)
        dev.close()
        full.close()
        app.close()


def eight_spheres():
    """A selective handle on eight flattened instances of one 180 x 90 sphere (cameras, lights and materials the Cornell box's)."""
    system, scene, _ = texts()
    app = twk.Application(system_text=system, scene_text=scene)
    app.setResolution(256, 256)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
    dev.setFlattenPolicy(1 << 28, 1 << 20)
    dev.clearScene()
    dev.addGeometry(*twk.mesh_sphere(180, 90, 1.0, np.pi))
    base = [np.array([0.2, 0, 0, -0.8 + 0.45 * (k % 4), 0, 0.2, 0, 0.4 + 0.6 * (k // 4), 0, 0, 0.2, -0.3], np.float32) for k in range(8)]
    for t in base:
        dev.addInstance(0, t, 2, -1)
    dev.build()
    return app, dev, base


def batch():
    app, dev, base = eight_spheres()
    ids = list(range(8))
    out = {"one": [], "eight": [], "update": []}
    for run in range(RUNS + 1):
        ms = {}
        new = [stepped(t, 3 * run) for t in base]
        ms["one"] = clock(lambda: dev.refitInstanceTransforms(ids, new))
        info = dev.refitInfo()
        new = [stepped(t, 3 * run + 1) for t in base]
        ms["eight"] = clock(lambda: [dev.refitInstanceTransform(i, new[i]) for i in ids])
        new = [stepped(t, 3 * run + 2) for t in base]
        ms["update"] = clock(lambda: dev.updateInstanceTransforms(ids, new))
        if run:
            for key in out:
                out[key].append(ms[key])
    print()
    print("| eight flattened spheres of 32 040 triangles | one twk_refit_instance_transforms ms | eight twk_refit_instance_transform ms | one twk_update_instance_transforms ms | one / eight | one / update | trees refit | nodes refit |")
    print("|---|---|---|---|---|---|---|---|")
    print(f"| selective handle | {med(out['one'])} | {med(out['eight'])} | {med(out['update'])} | {statistics.median(out['one']) / statistics.median(out['eight']):.2f} | "
          f"{statistics.median(out['one']) / statistics.median(out['update']):.2f} | {info['treesRefit']} | {info['nodesRefit']} |", flush=True)
    dev.close()
    app.close()


def kernels_child(path):
    """Under the kernel trace: RUNS + 1 refits of the moved C2 sphere's tree."""
    system, scene, _ = texts()
    app = twk.Application(system_text=system, scene_text=scene)
    app.setResolution(256, 256)
    base = app.instance(SPHERE)[1]
    dev = device(app)
    rate = dev.streamPeakGBps()
    for run in range(RUNS + 1):
        dev.refitInstanceTransform(SPHERE, stepped(base, run))
        info = dev.refitInfo()
    json.dump({"rate": rate, "slots": info["slotsRewritten"], "nodes": info["nodesRefit"]}, open(path, "w"))
    dev.close()
    app.close()


def kernels():
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "ir", "--", sys.executable, os.path.abspath(__file__), "--kernels-child", run],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        facts = json.load(open(run))
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        names = ("refitSceneSlotsKernel", "refitBatchParentsKernel", "refitBatchNodesKernel", "refitBatchTermsKernel")
        groups = {}
        for r in csv.DictReader(open(traces[0])):
            name = next((k for k in names if k in r["Kernel_Name"]), None)
            if name:
                groups.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1.0e3)
    slots, rate = facts["slots"], facts["rate"]
    compulsory = (48 + 3 * 12 + 12) * slots
    floor = 1.0e6 * compulsory / (rate * 1.0e9)
    print()
    print(f"Kernel trace, the C2 sphere's tree ({slots} slots, {facts['nodes']} nodes), microseconds: median (min .. max) over the dispatches after the first. "
          f"Floor of refitSceneSlotsKernel's compulsory bytes on a moved tree ({compulsory / 1e6:.2f} MB at {rate:.0f} GB/s): {floor:.2f} us.")
    print()
    print("| kernel | dispatches | us |")
    print("|---|---|---|")
    for name in names:
        if name in groups:
            print(f"| {name} | {len(groups[name])} | {med(groups[name][1:] or groups[name])} |")


def quality():
    system, scene, _ = texts()
    app = twk.Application(system_text=system, scene_text=scene)
    app.setResolution(1920, 1080)
    base = np.array(app.instance(SPHERE)[1], np.float32)
    refit_dev, rebuilt_dev = device(app), device(app)

    def passes():
        out = {"refit": [], "rebuilt": []}
        for run in range(RUNS + 1):
            for key, dev in (("refit", refit_dev), ("rebuilt", rebuilt_dev)):
                dev.synchronizeStream()
                ms = clock(lambda: (dev.render(run), dev.synchronizeStream()))
                if run:
                    out[key].append(ms)
        return out

    def row(label, transform):
        rebuilt_dev.updateInstanceTransform(SPHERE, transform)
        info = refit_dev.refitInfo()
        p = passes()
        print(f"| {label} | {info['refitsSinceBuild']} | {info['sahBuilt']:.3f} | {info['sahNow']:.3f} | {info['sahNow'] / info['sahBuilt']:.3f} | {med(p['refit'])} | {med(p['rebuilt'])} | "
              f"{statistics.median(p['refit']) / statistics.median(p['rebuilt']):.3f} |", flush=True)

    print()
    print("| C2 sphere, 1920 x 1080 sample pass (host clock, ms: median (min .. max)) | refits since build | sahBuilt | sahNow | sahNow / sahBuilt | pass on the refit handle | pass on the rebuilt handle | refit / rebuilt |")
    print("|---|---|---|---|---|---|---|---|")
    far = base.copy()
    far[[3, 7, 11]] += np.float32(1.0e4)
    mirror = base.copy()
    mirror[[0, 4, 8]] = -mirror[[0, 4, 8]]
    squash = base.copy()
    squash[[1, 5, 9]] *= np.float32(1.0e-3)
    for label, transform in (("the built transform", base), ("a translation by 1e4 (out of the camera's sight)", far), ("a rotation by 35 degrees with scales 1.2, 0.7, 1", turned(base, 35.0, (1.2, 0.7, 1.0))),
                             ("a mirror", mirror), ("a squash of one axis to 1e-3", squash)):
        refit_dev.updateInstanceTransform(SPHERE, base)  # a real build at the built transform: the count starts again
        refit_dev.refitInstanceTransform(SPHERE, transform)
        row(label, transform)
    refit_dev.updateInstanceTransform(SPHERE, base)
    done, worst = 0, (0.0, 0)
    for steps in (1, 10, 100):
        while done < steps:
            done += 1
            refit_dev.refitInstanceTransform(SPHERE, turned(base, 3.6 * done))
            info = refit_dev.refitInfo()
            worst = max(worst, (info["sahNow"] / info["sahBuilt"], done))
        row(f"{steps} rotation steps of 3.6 degrees (the largest sahNow / sahBuilt so far: {worst[0]:.3f} after step {worst[1]})", turned(base, 3.6 * done))
    for dev in (refit_dev, rebuilt_dev):
        dev.close()
    app.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--kernels-child" in args:
        kernels_child(args[args.index("--kernels-child") + 1])
    else:
        times("--no-room" not in args)
        batch()
        if "--no-kernels" not in args:
            kernels()
        quality()
