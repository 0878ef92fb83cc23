#!/usr/bin/env python3
"""Cost of a vertex update (include/tweeker_hip.h "Deforming an object") beside its baselines, and of twk_render_geometry_motion
beside twk_render_geometry.

Updates: host clock around the synchronising call, one warm-up, then RUNS rounds in which the calls alternate — the vertex update of
the mirror sphere's geometry (every vertex displaced), the transform update of the same instance, and the full twk_build — in full
and in selective mode. Configurations: the Cornell box (C2; the sphere has 32 040 triangles, flattened) and the C2 room with the
spheres tessellated 1000 x 500 (2.0 M triangles), flattened and two-level.

Geometry AOV: at 1920 x 1080 on C2, the median of RUNS timed calls each (host clock, synchronised before and after), alternating —
twk_render_geometry; twk_render_geometry_motion without a history (every g' = g); and with the sphere deformed after a merged frame.
Beside them the floor of the extra bytes: one 16-byte write per pixel, two 64-byte records per hit pixel, three index words and three
16-byte vertex reads per deformed hit, at the stream-copy rate twk_stream_peak_gbps reports in the same process.

Merges: the own-buffer plain and rectified merge at 1920 x 1080 with nothing moved, an instance moved and the mesh deformed — the parent,
the Moving and the Carried build of each, alternating (`merges` alone: only this table).

usage (GPU box): python tools/vertex_update_time.py [merges] > table.md"""
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


def updates():
    L = twk._lib
    system = open(os.path.join(SCENES, "system_rtigo3_cornell_box.txt")).read()
    scene = open(os.path.join(SCENES, "scene_rtigo3_cornell_box.txt")).read()
    room = scene.replace("sphere 180 90", "sphere 1000 500")
    print("| configuration | mode | vertex update ms | transform update ms | twk_build ms | trees rebuilt | slots rewritten |")
    print("|---|---|---|---|---|---|---|")
    for name, text, flatten in (("C2", scene, None), ("C2 room 2.0 M, flattened", room, None), ("C2 room 2.0 M, two-level", room, (0, 0))):
        app = twk.Application(system_text=system, scene_text=text)
        app.setResolution(256, 256)
        geometry, transform = app.instance(SPHERE)[0], np.array(app.instance(SPHERE)[1], np.float32)
        attributes = np.array(app.geometry(geometry)[0], np.float32)
        rng = np.random.default_rng(3)
        for selective in (True, False):
            dev = twk.Device(ordinal=0, miss=app.info.miss)
            dev.setUpdateMode(L.TWK_UPDATE_SELECTIVE if selective else L.TWK_UPDATE_FULL)
            if flatten is not None:
                dev.setFlattenPolicy(*flatten)
            app.initDevice(dev)
            dev.build()
            times = {"vertex": [], "transform": [], "build": []}
            info = None
            for run in range(RUNS + 1):
                new = attributes.copy()
                new[:, 0:3] += rng.uniform(-0.01, 0.01, (new.shape[0], 3)).astype(np.float32)
                moved = transform.copy()
                moved[7] += np.float32(0.01 * (run + 1))
                v = clock(lambda: dev.updateGeometryVertices(geometry, new))
                info = dev.updateInfo()
                t = clock(lambda: dev.updateInstanceTransform(SPHERE, moved))
                b = clock(dev.build)
                if run:  # the first round warms up
                    times["vertex"].append(v); times["transform"].append(t); times["build"].append(b)
            print(f"| {name} | {'selective' if selective else 'full'} | {med(times['vertex'])} | {med(times['transform'])} | {med(times['build'])} | {info['treesRebuilt']} | {info['slotsRewritten']} |", flush=True)
            dev.close()
        app.close()


def planes():
    L = twk._lib
    width, height = 1920, 1080
    app = twk.Application(os.path.join(SCENES, "system_rtigo3_cornell_box.txt"), os.path.join(SCENES, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(width, height)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    app.initDevice(dev)
    geometry = app.instance(SPHERE)[0]
    attributes = np.array(app.geometry(geometry)[0], np.float32)

    def timed(call):
        dev.synchronizeStream()
        return clock(lambda: (call(), dev.synchronizeStream()))

    def rounds(calls):
        out = {k: [] for k in calls}
        for run in range(RUNS + 1):
            for k, call in calls.items():
                ms = timed(call)
                if run:
                    out[k].append(ms)
        return out

    first = rounds({"geometry": dev.renderGeometry, "motion": dev.renderGeometryMotion})
    dev.render(0)
    dev.renderGeometry()
    dev.temporalAccumulate(L.Temporal())
    new = attributes.copy()
    new[:, 0:3] *= np.float32(1.2)
    dev.updateGeometryVertices(geometry, new)
    second = rounds({"geometry": dev.renderGeometry, "motion": dev.renderGeometryMotion})
    g = dev.readGeometry()
    hit = g[..., 3].view(np.uint32) != 0
    deformed = g[..., 3].view(np.uint32) == SPHERE + 1
    rate = dev.streamPeakGBps()
    extra = 16 * width * height + 128 * int(hit.sum()) + (12 + 48) * int(deformed.sum())
    print()
    print(f"1920 x 1080, C2: {int(hit.sum())} hit pixels, {int(deformed.sum())} of them on the deformed sphere; stream copy {rate:.0f} GB/s")
    print()
    print("| call (host clock, ms: median (min .. max)) | no history | sphere deformed |")
    print("|---|---|---|")
    print(f"| twk_render_geometry | {med(first['geometry'])} | {med(second['geometry'])} |")
    print(f"| twk_render_geometry_motion | {med(first['motion'])} | {med(second['motion'])} |")
    print(f"| floor of the extra bytes ({extra / 1e6:.1f} MB) | | {1.0e3 * extra / (rate * 1.0e9):.4f} |")
    dev.close()
    app.close()


def merges():
    """The own-buffer merges at 1920 x 1080 on C2, host clock around the call and a synchronisation, the three builds alternating:
    nothing moved (the parent build), the sphere's instance moved (the Moving build), the sphere's mesh deformed (the Carried build).
    What makes the condition — the update and the geometry AOV or the plane — is not timed."""
    L = twk._lib
    width, height = 1920, 1080
    app = twk.Application(os.path.join(SCENES, "system_rtigo3_cornell_box.txt"), os.path.join(SCENES, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(width, height)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    dev.setUpdateMode(L.TWK_UPDATE_SELECTIVE)
    app.initDevice(dev)
    geometry, transform = app.instance(SPHERE)[0], np.array(app.instance(SPHERE)[1], np.float32)
    attributes = np.array(app.geometry(geometry)[0], np.float32)
    dev.render(0)
    dev.renderGeometry()
    tp, rp = L.Temporal(), L.TemporalRectify()
    dev.temporalAccumulate(tp)
    state = {"n": 0}

    def prepare(kind):
        state["n"] += 1
        if kind == "moved":
            moved = transform.copy()
            moved[7] += np.float32(0.02 * (state["n"] % 2))
            dev.updateInstanceTransform(SPHERE, moved)
            dev.renderGeometry()
        elif kind == "deformed":
            new = attributes.copy()
            new[:, 0:3] *= np.float32(1.0 + 0.05 * (state["n"] % 2 + 1))
            dev.updateGeometryVertices(geometry, new)
            dev.renderGeometryMotion()
        else:
            dev.renderGeometry()
        dev.synchronizeStream()

    print()
    print("| own-buffer merge at 1920 x 1080 (host clock, ms: median (min .. max)) | nothing moved (parent build) | instance moved (Moving build) | mesh deformed (Carried build) |")
    print("|---|---|---|---|")
    for name, merge in (("twk_temporal_accumulate", lambda: dev.temporalAccumulate(tp)), ("twk_temporal_accumulate_rectified", lambda: dev.temporalAccumulateRectified(tp, rp))):
        times = {"still": [], "moved": [], "deformed": []}
        for run in range(RUNS + 1):
            for kind in times:
                prepare(kind)
                ms = clock(lambda: (merge(), dev.synchronizeStream()))
                if run:
                    times[kind].append(ms)
        print(f"| {name} | {med(times['still'])} | {med(times['moved'])} | {med(times['deformed'])} |", flush=True)
    dev.close()
    app.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["merges"]:
        merges()
    else:
        updates()
        planes()
        merges()
