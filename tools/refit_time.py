#!/usr/bin/env python3
"""Cost and quality of a refit (include/tweeker_hip.h "Refit") beside the selective vertex update it stands in for.

Time: host clock around the synchronising call, one warm-up round, then RUNS rounds in which twk_refit_geometry_vertices and
twk_update_geometry_vertices alternate on one selective handle, every vertex of the mirror sphere's geometry displaced each time.
(The rebuild's path is the parent's: its kernels' ISA is unchanged, profiles/r28_refit.md.) Configurations: the three rows of
profiles/r25_vertex_update.md — the Cornell box (C2; the sphere has 32 040 triangles, flattened) and the C2 room with the spheres
tessellated 1000 x 500 (2.0 M triangles), flattened and two-level.

Floor: the compulsory bytes of the refit's kernels — 3 x 48 attribute bytes and 12 index bytes read, 48 + 128 slot and shading-record
bytes written per triangle; 64 + 128 node and wide-node bytes written per node — at the stream-copy rate twk_stream_peak_gbps
reports in the same process, beside the whole call (upload, four launches per tree, the top level, the ranged tail, the caches).

Quality: the C2 sphere displaced by growing amplitudes (relative to its radius) in one step, and by 1, 10 and 100 successive noise
steps of 1 % each: sahNow / sahBuilt of TwkRefitInfo, and the time of a 1920 x 1080 sample pass on the refit handle over that on a
handle REBUILT with the same vertices (twk_update_geometry_vertices: a fresh build's trees), passes alternating.

usage (GPU box): python tools/refit_time.py > table.md"""
import os
import statistics
import sys
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


def selective_device(app, flatten=None):
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
    if flatten is not None:
        dev.setFlattenPolicy(*flatten)
    app.initDevice(dev)
    dev.build()
    return dev


def times():
    system, scene, room = texts()
    print("| configuration | refit ms | selective vertex update ms | refit / update | trees refit | nodes refit | slots rewritten | floor of the refit's bytes ms | refit / floor |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, text, flatten in (("C2", scene, None), ("C2 room 2.0 M, flattened", room, None), ("C2 room 2.0 M, two-level", room, (0, 0))):
        app = twk.Application(system_text=system, scene_text=text)
        app.setResolution(256, 256)
        geometry = app.instance(SPHERE)[0]
        attributes = np.array(app.geometry(geometry)[0], np.float32)
        rng = np.random.default_rng(3)
        dev = selective_device(app, flatten)
        rate = dev.streamPeakGBps()
        refit, update, info = [], [], None
        for run in range(RUNS + 1):
            ms = []
            for call in (dev.refitGeometryVertices, dev.updateGeometryVertices):
                new = attributes.copy()
                new[:, 0:3] += rng.uniform(-0.01, 0.01, (new.shape[0], 3)).astype(np.float32)
                ms.append(clock(lambda: call(geometry, new)))
                if call == dev.refitGeometryVertices:
                    info = dev.refitInfo()
            if run:  # the first round warms up
                refit.append(ms[0]); update.append(ms[1])
        compulsory = (3 * 48 + 12 + 48 + 128) * info["slotsRewritten"] + (64 + 128) * info["nodesRefit"]
        floor = 1.0e3 * compulsory / (rate * 1.0e9)
        print(f"| {name} | {med(refit)} | {med(update)} | {statistics.median(refit) / statistics.median(update):.2f} | {info['treesRefit']} | {info['nodesRefit']} | "
              f"{info['slotsRewritten']} | {floor:.4f} ({compulsory / 1e6:.1f} MB at {rate:.0f} GB/s) | {statistics.median(refit) / floor:.0f} |", flush=True)
        dev.close()
        app.close()


def quality():
    system, scene, _ = texts()
    app = twk.Application(system_text=system, scene_text=scene)
    app.setResolution(1920, 1080)
    geometry = app.instance(SPHERE)[0]
    attributes = np.array(app.geometry(geometry)[0], np.float32)
    radius = float(np.abs(attributes[:, 0:3]).max())
    refit_dev, rebuilt_dev = selective_device(app), selective_device(app)

    def passes():
        out = {"refit": [], "rebuilt": []}
        for run in range(RUNS + 1):
            for key, dev in (("refit", refit_dev), ("rebuilt", rebuilt_dev)):
                dev.synchronizeStream()
                ms = clock(lambda: (dev.render(run), dev.synchronizeStream()))
                if run:
                    out[key].append(ms)
        return out

    def row(label, new):
        rebuilt_dev.updateGeometryVertices(geometry, new)
        info = refit_dev.refitInfo()
        p = passes()
        print(f"| {label} | {info['refitsSinceBuild']} | {info['sahBuilt']:.3f} | {info['sahNow']:.3f} | {info['sahNow'] / info['sahBuilt']:.3f} | {med(p['refit'])} | {med(p['rebuilt'])} | "
              f"{statistics.median(p['refit']) / statistics.median(p['rebuilt']):.3f} |", flush=True)

    print()
    print("| C2 sphere, 1920 x 1080 sample pass (host clock, ms: median (min .. max)) | refits since build | sahBuilt | sahNow | sahNow / sahBuilt | pass on the refit handle | pass on the rebuilt handle | refit / rebuilt |")
    print("|---|---|---|---|---|---|---|---|")
    rng = np.random.default_rng(11)
    for amplitude in (0.0, 0.01, 0.05, 0.2, 0.5):
        refit_dev.updateGeometryVertices(geometry, attributes)  # a real build of the undeformed sphere: the count starts again
        new = attributes.copy()
        new[:, 0:3] += (radius * amplitude * rng.uniform(-1.0, 1.0, (new.shape[0], 3))).astype(np.float32)
        refit_dev.refitGeometryVertices(geometry, new)
        row(f"one step of amplitude {amplitude:g} r", new)
    refit_dev.updateGeometryVertices(geometry, attributes)
    new, done = attributes.copy(), 0
    for steps in (1, 10, 100):
        while done < steps:
            new[:, 0:3] += (radius * 0.01 * rng.uniform(-1.0, 1.0, (new.shape[0], 3))).astype(np.float32)
            refit_dev.refitGeometryVertices(geometry, new)
            done += 1
        row(f"{steps} successive steps of 0.01 r", new)
    for dev in (refit_dev, rebuilt_dev):
        dev.close()
    app.close()


if __name__ == "__main__":
    times()
    quality()
