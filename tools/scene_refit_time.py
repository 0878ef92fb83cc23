#!/usr/bin/env python3
"""Cost of a frame's edits in one call (include/tweeker_hip.h "A frame's edits in one call") beside THE SEQUENCE it stands for:
twk_refit_geometry_vertices[_device] per edited geometry, then twk_refit_instance_transforms.

Time: host clock around calls that end in the library's own waits; two handles on the same build, one takes refitScene, the other the
sequence, alternating in one process; WARM warm-up rounds, then RUNS rounds; median (min .. max). Configurations: the Cornell box
(C2) with the sphere mesh edited and both its instances moved; the C2 room with the spheres tessellated 1000 x 500 (2.0 M triangles),
flattened and two-level; a "crowd" of CROWD flattened meshes of about 2 k triangles (32 x 32 spheres), each edited from a device
source (torch, records) and each moved.

Kernel trace: a child of this tool under `rocprofv3 --kernel-trace` (a run of its own) makes one refitScene call with 2 trees and
one with 16 trees after a warm-up call each; the launches between two markers (a stream-copy probe launch before and after the call)
are listed by name. The slots kernel's time stands beside the stream-copy floor of its
compulsory bytes (the rate: tools/probes/stream_copy_probe where it has been built), computed from the plan (twk_scene_refit_plan_host): per slot 12 index bytes, three 48-byte vertex records, the
16-byte primitive word, and the bytes written by kind.

Unchanged behaviour: `--parent ROOT` names a tree that holds a build of the parent commit (its package and bench.py); the four
existing refit calls on C2 and the default bench.py line are measured on both trees in turn, each in a process of its own, and both
ranges are printed.

usage (GPU box): python tools/scene_refit_time.py [--no-room] [--no-kernels] [--no-crowd] [--only-kernels] [--parent ROOT] > table.md"""
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
if "--package-root" in sys.argv:  # a child measuring another build: that tree's package, this tree's scenes
    sys.path.insert(0, sys.argv[sys.argv.index("--package-root") + 1])
else:
    sys.path.insert(0, ROOT)

SCENES = os.path.join(ROOT, "scenes")
WARM, RUNS = 3, 20
CROWD = 16


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


def device(twk, app, flatten=None):
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
    if flatten is not None:
        dev.setFlattenPolicy(*flatten)
    app.initDevice(dev)
    dev.build()
    return dev


def stepped(transform, k):
    t = np.array(transform, np.float32).reshape(12).copy()
    t[[3, 7, 11]] += np.float32(0.002) * np.array([1.0, 0.5, -0.5], np.float32) * (1 + k % 3)
    return t


def breathing(attributes, k):
    a = np.array(attributes, np.float32).reshape(-1, 12).copy()
    a[:, 0:3] *= np.float32(1.0 + 0.002 * (1 + k % 3))
    return a


def sphere_of(app):
    """(geometry, [its instances]) of the Cornell box's sphere mesh."""
    by_geometry = {}
    for i in range(app.info.numInstances):
        by_geometry.setdefault(app.instance(i)[0], []).append(i)
    geometry = max(by_geometry, key=lambda g: (len(by_geometry[g]), np.asarray(app.geometry(g)[1]).size))
    return geometry, by_geometry[geometry]


def alternate(one_call, sequence_call):
    out = {"one": [], "sequence": []}
    for run in range(WARM + RUNS):
        ms = {"one": clock(lambda: one_call(run)), "sequence": clock(lambda: sequence_call(run))}
        if run >= WARM:
            for key in out:
                out[key].append(ms[key])
    return out


def row(name, out, info):
    print(f"| {name} | {med(out['one'])} | {med(out['sequence'])} | {statistics.median(out['one']) / statistics.median(out['sequence']):.2f} | "
          f"{info['treesRefit']} | {info['treesRebuilt']} | {info['nodesRefit']} | {info['slotsRewritten']} |", flush=True)


def times(twk, room_too):
    system, scene, room = texts()
    print(f"| configuration | refitScene ms | the sequence ms | one / sequence | trees refit | trees rebuilt | nodes refit | slots rewritten |")
    print("|---|---|---|---|---|---|---|---|")
    rows = [("C2: the sphere mesh edited, both its instances moved", scene, None)]
    if room_too:
        rows += [("C2 room 2.0 M, flattened", room, (1 << 28, 1 << 20)), ("C2 room 2.0 M, two-level", room, (0, 0))]
    for name, text, flatten in rows:
        app = twk.Application(system_text=system, scene_text=text)
        app.setResolution(256, 256)
        geometry, ids = sphere_of(app)
        base = [app.instance(i)[1] for i in ids]
        attributes = np.array(app.geometry(geometry)[0], np.float32)
        one, seq = device(twk, app, flatten), device(twk, app, flatten)

        def sequence(run):
            seq.refitGeometryVertices(geometry, breathing(attributes, run))
            seq.refitInstanceTransforms(ids, [stepped(t, run) for t in base])

        out = alternate(lambda run: one.refitScene([(geometry, breathing(attributes, run))], ids, [stepped(t, run) for t in base]), sequence)
        row(name, out, one.refitInfo())
        for d in (one, seq):
            d.close()
        app.close()


def crowd_devices(twk, count, handles=2):
    """Selective handles on `count` flattened instances of `count` 32 x 32 spheres (cameras, lights and materials the Cornell box's)."""
    system, scene, _ = texts()
    app = twk.Application(system_text=system, scene_text=scene)
    app.setResolution(256, 256)
    mesh = twk.mesh_sphere(32, 32, 1.0, np.pi)
    base = [np.array([0.1, 0, 0, -0.8 + 0.45 * (k % 4), 0, 0.1, 0, 0.3 + 0.4 * (k // 4), 0, 0, 0.1, -0.3], np.float32) for k in range(count)]
    devices = []
    for _ in range(handles):
        dev = twk.Device(ordinal=0, miss=app.info.miss)
        app.initDevice(dev)
        dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
        dev.setFlattenPolicy(1 << 28, 1 << 20)
        dev.clearScene()
        for k in range(count):
            dev.addGeometry(*mesh)
            dev.addInstance(k, base[k], 2, -1)
        dev.build()
        devices.append(dev)
    return app, devices, np.array(mesh[0], np.float32).reshape(-1, 12), base


def crowd(twk):
    import torch
    app, (one, seq), attributes, base = crowd_devices(twk, CROWD)
    ids = list(range(CROWD))
    sources = []
    for k in range(3):
        t = torch.empty(attributes.shape, dtype=torch.float32, device="cuda")
        t.copy_(torch.from_numpy(breathing(attributes, k)))
        sources.append(t)
    torch.cuda.synchronize()

    def sequence(run):
        for g in ids:
            seq.refitGeometryVerticesDevice(g, sources[run % 3])
        seq.refitInstanceTransforms(ids, [stepped(t, run) for t in base])

    out = alternate(lambda run: one.refitScene([(g, dict(source=sources[run % 3])) for g in ids], ids, [stepped(t, run) for t in base]), sequence)
    row(f"crowd: {CROWD} meshes of {attributes.shape[0]} vertices / {one.buildInfo()['triangleSlots'] // CROWD} triangles, each from a device source and moved", out, one.refitInfo())
    for d in (one, seq):
        d.close()
    app.close()


# ---- the kernel trace --------------------------------------------------------------------------------------------------------------------
def kernels_child(twk, path):
    """Under the kernel trace: per tree count a warm-up call, a marker, the call, a marker (streamPeakGBps launches the copy probe).
    Half of the meshes are edited, each from a DEVICE source (torch, records), and every instance is moved: count trees, count / 2
    check launches and count / 2 ingest launches."""
    import torch
    facts = {}
    for count in (2, 16):
        app, (dev,), attributes, base = crowd_devices(twk, count, handles=1)
        ids = list(range(count))
        rate = dev.streamPeakGBps(1 << 26, 1)
        sources = []
        for run in range(2):
            t = torch.empty(attributes.shape, dtype=torch.float32, device="cuda")
            t.copy_(torch.from_numpy(breathing(attributes, run)))
            sources.append(t)
        torch.cuda.synchronize()
        for run in range(2):
            if run:
                dev.streamPeakGBps(1 << 20, 1)
            dev.refitScene([(g, dict(source=sources[run])) for g in ids[:count // 2]], ids, [stepped(t, run) for t in base])
            if run:
                dev.streamPeakGBps(1 << 20, 1)
        triangles = [dev.buildInfo()["triangleSlots"] // count] * count
        plan = twk.scene_refit_plan_host(ids, triangles, (1 << 28, 1 << 20), ids[:count // 2], ids)
        facts[str(count)] = {"rate": dev.streamPeakGBps(), "slots": int(plan["slots"]), "slotBytes": int(plan["slotBytes"]), "kinds": [int(k) for k in plan["kinds"]], "first_rate": rate}
        dev.close()
        app.close()
    json.dump(facts, open(path, "w"))


def kernels():
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "sr", "--", sys.executable, os.path.abspath(__file__), "--kernels-child", run],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        facts = json.load(open(run))
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    marker = [k for k, r in enumerate(rows) if "streamCopy" in r["Kernel_Name"] or "StreamCopy" in r["Kernel_Name"]]
    # per tree count: the copy probes of the first rate, then [marker, call, marker], then the probes of the last rate; the call is
    # the span between the two single markers that hold a refitSceneSlotsKernel
    spans = []
    for a, b in zip(marker, marker[1:]):
        inside = rows[a + 1:b]
        if any("refitSceneSlotsKernel" in r["Kernel_Name"] for r in inside):
            spans.append(inside)
    # the floor's rate: the best float4 copy of tools/probes/stream_copy_probe.hip (built beside its source, its "Build:" line) where
    # that program is there, else the library's own copy probe in the child's process
    probe, probe_rate = os.path.join(ROOT, "tools", "probes", "stream_copy_probe"), None
    if os.path.exists(probe):
        import re
        out = subprocess.run([probe], check=True, capture_output=True, text=True, timeout=120).stdout
        probe_rate = max(float(x) for x in re.findall(r"([0-9.]+) GB/s", out))
    print()
    print(f"The copy rate of the floors: {'tools/probes/stream_copy_probe, its best variant' if probe_rate else 'twk_stream_peak_gbps in the traced process'}.")
    # per tree count the spans are [the warm-up call, the call]
    for count, inside in zip((2, 16), spans[1::2]):
        f = facts[str(count)]
        if probe_rate:
            f["rate"] = probe_rate
        short = lambda n: n.split("(")[0].split("::")[-1]
        names = [short(r["Kernel_Name"]) for r in inside]
        batch = [n for n in names if n.startswith("refitScene") or n.startswith("refitBatch")]
        tally = {}
        for n in names:
            tally[n] = tally.get(n, 0) + 1
        print(f"A call with {count} trees (kinds {f['kinds']}): {len(names)} launches, {len(batch)} of them the batch's kernels: {', '.join(batch)}.")
        print(f"  all launches by name: {', '.join(f'{k} x {v}' for k, v in tally.items())}")
        print(f"  in order: {', '.join(names)}")
        slot_us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1.0e3 for r in inside if "refitSceneSlotsKernel" in r["Kernel_Name"]]
        compulsory = f["slots"] * (12 + 3 * 48 + 16) + f["slotBytes"]
        floor = 1.0e6 * compulsory / (f["rate"] * 1.0e9)
        print(f"  refitSceneSlotsKernel: {slot_us[0]:.2f} us for {f['slots']} slots; compulsory bytes {compulsory / 1e6:.3f} MB ({f['slotBytes'] / 1e6:.3f} MB written), "
              f"floor at {f['rate']:.0f} GB/s {floor:.2f} us, measured / floor {slot_us[0] / floor:.1f}")
        print()


# ---- unchanged behaviour -----------------------------------------------------------------------------------------------------------------
def existing_child(twk):
    """The four existing refit calls on C2, WARM + RUNS rounds each; one JSON line."""
    system, scene, _ = texts()
    app = twk.Application(system_text=system, scene_text=scene)
    app.setResolution(256, 256)
    geometry, ids = sphere_of(app)
    base = [app.instance(i)[1] for i in ids]
    attributes = np.array(app.geometry(geometry)[0], np.float32)
    dev = device(twk, app)
    import torch
    source = torch.empty(attributes.shape, dtype=torch.float32, device="cuda")
    source.copy_(torch.from_numpy(attributes))
    torch.cuda.synchronize()
    out = {"twk_refit_geometry_vertices": [], "twk_refit_geometry_vertices_device": [], "twk_refit_instance_transform": [], "twk_refit_instance_transforms": []}
    for run in range(WARM + RUNS):
        ms = {"twk_refit_geometry_vertices": clock(lambda: dev.refitGeometryVertices(geometry, attributes)),
              "twk_refit_geometry_vertices_device": clock(lambda: dev.refitGeometryVerticesDevice(geometry, source)),
              "twk_refit_instance_transform": clock(lambda: dev.refitInstanceTransform(ids[0], stepped(base[0], run))),
              "twk_refit_instance_transforms": clock(lambda: dev.refitInstanceTransforms(ids, [stepped(t, run) for t in base]))}
        if run >= WARM:
            for key in out:
                out[key].append(ms[key])
    dev.close()
    app.close()
    print(json.dumps(out))


def unchanged(parent):
    rounds = 3
    results = {"this tree": [], "the parent": []}
    bench = {"this tree": [], "the parent": []}
    for _ in range(rounds):
        for name, root in (("this tree", ROOT), ("the parent", parent)):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-child", "--package-root", root], check=True, capture_output=True, text=True, timeout=300)
            results[name].append(json.loads(run.stdout.strip().splitlines()[-1]))
            run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "64", "--warmup", "4"], check=True, capture_output=True, text=True, timeout=300)
            bench[name].append(json.loads(run.stdout.strip().splitlines()[-1])["value"])
    print()
    print(f"| call on C2, ms: range of the {rounds} processes' medians (each {RUNS} rounds) | this tree | the parent |")
    print("|---|---|---|")
    for key in results["this tree"][0]:
        cells = []
        for name in ("this tree", "the parent"):
            medians = [statistics.median(r[key]) for r in results[name]]
            cells.append(f"{min(medians):.3f} .. {max(medians):.3f}")
        print(f"| {key} | {cells[0]} | {cells[1]} |")
    print(f"| bench.py --gpus 1 --steps 64 --warmup 4, Msamples/s | {min(bench['this tree']):.1f} .. {max(bench['this tree']):.1f} | {min(bench['the parent']):.1f} .. {max(bench['the parent']):.1f} |", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--existing-child" in args:
        import torch  # noqa: F401  (first: see below)
        import tweeker_raytracer_amd as twk
        existing_child(twk)
    elif "--kernels-child" in args:
        import torch  # noqa: F401  (first: see below)
        import tweeker_raytracer_amd as twk
        kernels_child(twk, args[args.index("--kernels-child") + 1])
    else:
        import torch  # noqa: F401  (first, so that the library binds to torch's HIP runtime: the crowd's sources are torch tensors)
        import tweeker_raytracer_amd as twk
        if "--only-kernels" not in args:
            times(twk, "--no-room" not in args)
        if "--no-crowd" not in args and "--only-kernels" not in args:
            crowd(twk)
        if "--no-kernels" not in args:
            kernels()
        if "--parent" in args:
            unchanged(os.path.abspath(args[args.index("--parent") + 1]))
