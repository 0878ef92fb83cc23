#!/usr/bin/env python3
"""Cost of the planned adaptive pass on a 1920x1080 Cornell frame (C2): the plan call beside the select, and a planned pass beside
the fixed adaptive pass over the same list.

calls: twk_adaptive_plan and twk_adaptive_select on the handle's own buffers after 16 uniform iterations, at the target that selects
about half of the pixels; both synchronise, so the wall clock of N calls divided by N is the call as a loop pays it. Measured in
the same process, one after the other.

passes: at the shares 1.0, 0.1 and 0.01 of the pixels (the targets of tools/adaptive_time.py), twk_launch_adaptive(8) on the select's
list beside twk_launch_adaptive_planned on the plan of the same parameters with every budget forced to 8 (minBatch = maxBatch = 8):
the two passes trace and shade the same paths at the same iterations, in another order (fixed: sample-major, planned: entry-major).
Each pass between two synchronisations, REPEATS times after one warm-up; then one more pass with twk_profile_enable for the time of
each kernel class. A pass lowers the errors it was selected by, so before every pass the frame is restarted (16 uniform iterations
from 0, the same bits every time) and selected or planned anew, outside the clock: every repeat of either pass renders the same list.
Each configuration runs in a child process of its own under a time limit; the first failure ends the run.
usage (GPU box): python tools/adaptive_plan_time.py > table.md"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = (1920, 1080)
SAMPLES, UNIFORM, REPEATS = 8, 16, 5
SHARES = (1.0, 0.1, 0.01)
CHILD_SECONDS = 240


def _device():
    import tweeker_raytracer_amd as twk
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableMoments(True)
    dev.enableAdaptive(True)
    dev.setLaunchBatch(SAMPLES)
    for it in range(UNIFORM):
        dev.render(it)
    dev.synchronizeStream()
    return twk, dev


def _target(dev, share):
    import numpy as np
    import noise_restate as nr
    cls, e = nr.classify(dev.readMoments().reshape(-1, 4))
    return float(np.quantile(e[cls == nr.VALID], 1.0 - share))


def child(mode, share):
    twk, dev = _device()
    if mode == "calls":
        ap = twk.Adaptive(targetNoise=_target(dev, 0.5))
        out = {"mode": mode}
        for name, call in (("select", lambda: dev.adaptiveSelect(ap)), ("plan", lambda: dev.adaptivePlan(ap)[0])):
            for _ in range(10):
                n = call()
            windows = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                for _ in range(50):
                    call()
                windows.append((time.perf_counter() - t0) * 1e6 / 50)
            out[name] = {"active": n, "us_per_call": min(windows), "windows": windows}
        print(json.dumps(out))
        dev.close()
        return
    # share 1.0: a minSamples no pixel has makes every pixel UNKNOWN, and so selected (tools/adaptive_time.py)
    ap = twk.Adaptive(targetNoise=1.0, minSamples=1 << 24, maxSamples=1 << 30) if share >= 1.0 else twk.Adaptive(targetNoise=_target(dev, share), maxSamples=1 << 30)
    forced = twk.AdaptivePlan(minBatch=SAMPLES, maxBatch=SAMPLES)
    if mode == "fixed":
        prepare, launch = (lambda: (dev.adaptiveSelect(ap),) * 2), (lambda: dev.renderAdaptive(SAMPLES))
    else:
        prepare, launch = (lambda: dev.adaptivePlan(ap, forced)), dev.renderPlanned

    def one_pass():
        for it in range(UNIFORM):  # restart the frame: the list of every repeat is the list of the first
            dev.render(it)
        n, paths = prepare()
        dev.synchronizeStream()
        t0 = time.perf_counter()
        launch()
        dev.synchronizeStream()
        return n, paths, time.perf_counter() - t0

    n, paths, _ = one_pass()
    if mode == "fixed":
        paths = n * SAMPLES
    assert paths == n * SAMPLES
    walls = []
    for _ in range(REPEATS + 1):
        again, _, wall = one_pass()
        assert again == n
        walls.append(wall)
    dev.profileEnable(True)
    dev.profileReset()
    for it in range(UNIFORM):
        dev.render(it)
    prepare()
    dev.synchronizeStream()
    dev.profileReset()
    launch()
    dev.synchronizeStream()
    kernels = {k: v["ms"] for k, v in dev.profileGet().items()}
    dev.profileEnable(False)
    print(json.dumps({"mode": mode, "share": share, "active": n, "paths": paths, "ms": min(walls[1:]) * 1e3, "all_ms": [w * 1e3 for w in walls], "kernels": kernels}))
    dev.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], float(sys.argv[3]))
        return 0
    rows = []
    for mode, share in [("calls", 0.5)] + [(m, s) for s in SHARES for m in ("fixed", "planned")]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(share)], capture_output=True, text=True, timeout=CHILD_SECONDS)
        if r.returncode != 0:
            print(f"configuration {mode} {share} failed with status {r.returncode}; stopping\n{r.stdout}{r.stderr}", file=sys.stderr)
            return 1
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    pixels = RES[0] * RES[1]
    c = rows[0]
    print(f"synchronising calls on the handle's own buffers, {RES[0]}x{RES[1]}, C2 at {UNIFORM} spp, {c['plan']['active']} of {pixels} selected: the smallest of {REPEATS} windows of 50 calls\n")
    print("| call | us per call (smallest window) | every window |")
    print("|---|---|---|")
    for name in ("select", "plan"):
        print(f"| twk_adaptive_{name} | {c[name]['us_per_call']:.1f} | " + ", ".join(f"{w:.1f}" for w in c[name]["windows"]) + " |")
    print(f"\none pass of {SAMPLES} samples per selected pixel between two synchronisations: the smallest of {REPEATS} after two warm-up passes, the spread (largest - smallest of the {REPEATS}), and one profiled pass's time per kernel class\n")
    print("| pass | active share | paths | ms per pass | spread ms | generate ms | trace ms | shade ms | accumulate ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows[1:]:
        ms = [w for w in r["all_ms"][1:]]
        k = r["kernels"]
        print(f"| {r['mode']} | {r['active'] / pixels:.4f} | {r['paths']} | {min(ms):.3f} | {max(ms) - min(ms):.3f} | {k['generate']:.3f} | {k['trace']:.3f} | {k['shade']:.3f} | {k['accumulate']:.3f} |")
    print("\nevery pass, ms:\n")
    for r in rows[1:]:
        print(f"- {r['mode']} {r['share']}: " + ", ".join(f"{w:.3f}" for w in r["all_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
