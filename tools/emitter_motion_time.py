#!/usr/bin/env python3
"""Cost of moving a light (include/tweeker_hip.h "Moving a light"): twk_refit_instance_transform on the instance that carries the light
beside the same call on a wall of the same scene, and twk_update_instance_transform likewise. The light's quad and a wall's quad are
both two-triangle direct leaves of the top level, so the calls do the same work but for the light's own: the rule on the host
(csrc/light_motion.h) and ONE 80-byte upload.

Time: host clock around the synchronising call, RUNS warm rounds after one warm-up round, the two instances ALTERNATING in one
process, each stepped a little every time. Scene: the Cornell box on a selective handle (instance 0 the light, instance 1 the floor).
The expectation the table is read against: the light's median lies inside the wall's own spread (min .. max).

usage (GPU box): python tools/emitter_motion_time.py > table.md"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tweeker_raytracer_amd as twk  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
RUNS = 25
LIGHT, WALL = 0, 1


def clock(call):
    start = time.perf_counter()
    call()
    return 1.0e3 * (time.perf_counter() - start)


def med(values):
    return f"{statistics.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def stepped(transform, k):
    t = np.array(transform, np.float32).reshape(12).copy()
    t[[3, 7, 11]] += np.float32(0.002) * np.array([1.0, -0.5, 0.5], np.float32) * (1 + k % 3)
    return t


def main():
    app = twk.Application(os.path.join(SCENES, "system_rtigo3_cornell_box.txt"), os.path.join(SCENES, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(256, 256)
    assert app.instance(LIGHT)[3] >= 0 and app.instance(WALL)[3] < 0
    assert len(app.geometry(app.instance(LIGHT)[0])[1]) == len(app.geometry(app.instance(WALL)[0])[1]) == 6, "two triangles each"
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
    app.initDevice(dev)
    dev.build()
    dev.enableEmitterMotion()
    base = {i: app.instance(i)[1] for i in (LIGHT, WALL)}
    print("| call | the light's instance ms | a wall's instance ms | light / wall | the light's median inside the wall's spread |")
    print("|---|---|---|---|---|")
    for name, call in (("twk_refit_instance_transform", dev.refitInstanceTransform), ("twk_update_instance_transform", dev.updateInstanceTransform)):
        out = {LIGHT: [], WALL: []}
        for run in range(RUNS + 1):
            for i in ((LIGHT, WALL) if run % 2 == 0 else (WALL, LIGHT)):
                ms = clock(lambda: call(i, stepped(base[i], run)))
                if run:  # the first round warms up
                    out[i].append(ms)
        light, wall = statistics.median(out[LIGHT]), statistics.median(out[WALL])
        print(f"| {name} | {med(out[LIGHT])} | {med(out[WALL])} | {light / wall:.3f} | {'yes' if min(out[WALL]) <= light <= max(out[WALL]) else 'NO'} |", flush=True)
    dev.close()
    app.close()


if __name__ == "__main__":
    main()
