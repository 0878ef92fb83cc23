#!/usr/bin/env python3
"""Cost of a refit from a device-pointer source (include/tweeker_hip.h "A device-pointer source") beside the host-source refit.

Time: host clock around the synchronising call, one warm-up round, then RUNS rounds in which, in ONE process and on ONE selective
handle, three calls alternate: twk_refit_geometry_vertices from a host array (what a caller with device vertices pays AFTER its own
copy to the host, which is timed beside it), twk_refit_geometry_vertices_device from a tensor of records, and the same from a tensor
of positions with the frames recomputed. Every vertex of the mirror sphere's geometry is displaced each time. Configurations: the
rows of profiles/r28_refit.md — the Cornell box (C2; the sphere has 32 040 triangles, flattened) and the C2 room with the spheres
tessellated 1000 x 500 (2.0 M triangles), flattened and two-level.

Floor: the compulsory bytes of the ingest — attributes: 48 read + 48 written per vertex; positions with frames: 12 + 48 read, 48
written, 8 of offsets per vertex and 4 + 12 of table and indices per adjacent triangle (the neighbours' positions counted once, as
the 12 above) — at the stream-copy rate twk_stream_peak_gbps reports in the same process.

--host-only: the host-source refit alone (runs on the parent commit's tree too: the figure both are compared by).

Kernel time comes from a kernel trace in a run of its own, not from the host clock:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o vs -- python tools/vertex_source_time.py --kernels DIR/run.json
    python tools/vertex_source_time.py --summarize DIR
--kernels runs only the two device-source refits, RUNS + 1 rounds per configuration, and writes the vertex and triangle counts and the
stream-copy rate; --summarize reads the trace's per-dispatch rows of vertexSourceCheckKernel, ingestAttributesKernel and
ingestPositionsKernel<true>, groups them by grid size (the two rooms have the same sphere, so they share a row), drops each group's
first dispatch and prints the kernel time beside the floor of its compulsory bytes.

usage (GPU box): python tools/vertex_source_time.py [--host-only] > table.md"""
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library, as in bench.py: the library then binds to the HIP runtime torch has loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tweeker_raytracer_amd as twk  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
RUNS = 7
SPHERE = 6  # the mirror sphere's instance in the Cornell box


def clock(call):
    start = time.perf_counter()
    call()
    return 1.0e3 * (time.perf_counter() - start)


def med(values):
    return f"{statistics.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def floors(n, triangles):
    """Compulsory bytes of the check, the records ingest and the frames ingest."""
    return {"vertexSourceCheckKernel": 12 * n, "ingestAttributesKernel": 96 * n, "ingestPositionsKernel<true>": (12 + 48 + 48 + 8) * n + 3 * 16 * triangles}


def summarize(directory):
    run = json.load(open(os.path.join(directory, "run.json")))
    traces = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(traces) != 1:
        sys.exit(f"{directory}: {len(traces)} kernel traces")
    groups = {}
    for r in csv.DictReader(open(traces[0])):
        name = next((k for k in floors(0, 0) if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        grid = int(r.get("Grid_Size") or r.get("Grid_Size_X"))
        groups.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1.0e3)
    print("| kernel | vertices | dispatches | kernel us: median (min .. max) | compulsory MB | floor us | kernel / floor | GB/s of the compulsory bytes |")
    print("|---|---|---|---|---|---|---|---|")
    for n, triangles in sorted({(c["vertices"], c["triangles"]) for c in run["configurations"]}):
        for name, nbytes in floors(n, triangles).items():
            grids = [g for (k, g) in groups if k == name and (g == n or g == (n + 255) // 256 * 256 or g == (n + 255) // 256)]
            us = [t for g in grids for t in groups[(name, g)][1:]]
            if not us:
                print(f"| `{name}` | {n} | 0 | not in the trace | | | | |")
                continue
            m, floor = statistics.median(us), 1.0e6 * nbytes / (run["rate"] * 1.0e9)
            print(f"| `{name}` | {n} | {len(us)} | {m:.2f} ({min(us):.2f} .. {max(us):.2f}) | {nbytes / 1e6:.2f} | {floor:.2f} | {m / floor:.1f} | {nbytes / m / 1e3:.0f} |")
    print(f"\nstream-copy rate of the traced process: {run['rate']:.0f} GB/s")


def main(host_only, kernels=None):
    configurations = []
    system = open(os.path.join(SCENES, "system_rtigo3_cornell_box.txt")).read()
    scene = open(os.path.join(SCENES, "scene_rtigo3_cornell_box.txt")).read()
    room = scene.replace("sphere 180 90", "sphere 1000 500")
    if kernels:
        pass
    elif host_only:
        print("| configuration | host-source refit ms |")
        print("|---|---|")
    else:
        print("| configuration | vertices | host-source refit ms | the caller's copy to the host before it ms | device source, records ms | device source, positions + frames ms | "
              "records / host | frames / host | floor of the records ingest ms | floor of the frames ingest ms |")
        print("|---|---|---|---|---|---|---|---|---|---|")
    for name, text, flatten in (("C2", scene, None), ("C2 room 2.0 M, flattened", room, None), ("C2 room 2.0 M, two-level", room, (0, 0))):
        app = twk.Application(system_text=system, scene_text=text)
        app.setResolution(256, 256)
        geometry = app.instance(SPHERE)[0]
        attributes, indices = app.geometry(geometry)
        attributes = np.array(attributes, np.float32).reshape(-1, 12)
        n, triangles = attributes.shape[0], np.asarray(indices).size // 3
        rng = np.random.default_rng(3)
        dev = twk.Device(ordinal=0, miss=app.info.miss)
        dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
        if flatten is not None:
            dev.setFlattenPolicy(*flatten)
        app.initDevice(dev)
        dev.build()
        rate = dev.streamPeakGBps()
        records = torch.empty((n, 12), dtype=torch.float32, device="cuda")
        positions = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        host, copy, from_records, from_positions = [], [], [], []
        for run in range(RUNS + 1):
            new = attributes.copy()
            new[:, 0:3] += rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32)
            records.copy_(torch.from_numpy(new))
            positions.copy_(torch.from_numpy(np.ascontiguousarray(new[:, 0:3])))
            torch.cuda.synchronize()
            ms = [0.0 if kernels else clock(lambda: dev.refitGeometryVertices(geometry, new))]
            if not host_only:
                ms.append(clock(lambda: records.cpu().numpy()))
                ms.append(clock(lambda: dev.refitGeometryVerticesDevice(geometry, records)))
                ms.append(clock(lambda: dev.refitGeometryVerticesDevice(geometry, positions, recomputeFrames=True)))
            if run:  # the first round warms up (and builds the adjacency table)
                host.append(ms[0])
                if not host_only:
                    copy.append(ms[1]); from_records.append(ms[2]); from_positions.append(ms[3])
        configurations.append({"name": name, "vertices": int(n), "triangles": int(triangles)})
        if kernels:
            json.dump({"rate": rate, "configurations": configurations}, open(kernels, "w"))
        elif host_only:
            print(f"| {name} | {med(host)} |", flush=True)
        else:
            floor_records = 1.0e3 * (96 * n) / (rate * 1.0e9)
            floor_frames = 1.0e3 * ((12 + 48 + 48 + 8) * n + 3 * 16 * triangles) / (rate * 1.0e9)
            h = statistics.median(host)
            print(f"| {name} | {n} | {med(host)} | {med(copy)} | {med(from_records)} | {med(from_positions)} | {statistics.median(from_records) / h:.2f} | "
                  f"{statistics.median(from_positions) / h:.2f} | {floor_records:.4f} | {floor_frames:.4f} (at {rate:.0f} GB/s) |", flush=True)
        dev.close()
        app.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--summarize" in args:
        summarize(args[args.index("--summarize") + 1])
    else:
        main("--host-only" in args, args[args.index("--kernels") + 1] if "--kernels" in args else None)
