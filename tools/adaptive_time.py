#!/usr/bin/env python3
"""Cost of adaptive sampling on a 1920x1080 Cornell frame (C2): the select, and an adaptive pass beside a uniform one.

select: twk_adaptive_select on the handle's own buffers after 16 uniform iterations, at the target that selects about half of the
pixels; the call synchronises, so the wall clock of N calls divided by N is the call as a loop pays it (three launches, a 4-byte
copy, one synchronisation). Its compulsory bytes (16 B moments + 4 B count read per pixel, 4 B written per selected pixel; the
ballot words are 1/8 B per pixel each way) over the stream-copy peak of the same process is the floor printed beside it.

pass: twk_launch_adaptive(SAMPLES) on lists of 1.0 and about 0.5, 0.1 and 0.01 of the pixels (the target is the matching quantile of
the frame's own error map at 16 spp, for 1.0 every pixel is made UNKNOWN; the list stays valid, so the same list is rendered again
and again), between two
synchronisations, beside SAMPLES uniform iterations of the same library as one pass (the fused-primary path). Nanoseconds per path
= wall clock / (paths of the pass). A uniform pass starts at the tile entry points and never writes queue 0; an adaptive pass
pays the generate kernel's queue write and starts at the root: at share 1.0 it is expected to be slower per path. The interesting
figure is the share below which the adaptive pass takes less TIME than the uniform pass over all pixels.
Each configuration runs in a child process of its own under a time limit; the first failure ends the run.
usage (GPU box): python tools/adaptive_time.py > table.md"""
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
SHARES = (1.0, 0.5, 0.1, 0.01)
CHILD_SECONDS = 240


def _device(adaptive):
    import tweeker_raytracer_amd as twk
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableMoments(True)
    if adaptive:
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
    pixels = RES[0] * RES[1]
    if mode == "uniform":
        twk, dev = _device(False)
        walls, first = [], UNIFORM
        for _ in range(REPEATS + 1):
            dev.synchronizeStream()
            t0 = time.perf_counter()
            for it in range(first, first + SAMPLES):
                dev.render(it)
            dev.synchronizeStream()
            walls.append(time.perf_counter() - t0)
            first += SAMPLES
        print(json.dumps({"mode": mode, "paths": pixels * SAMPLES, "ms": min(walls[1:]) * 1e3, "all_ms": [w * 1e3 for w in walls]}))
    elif mode == "select":
        twk, dev = _device(True)
        ap = twk.Adaptive(targetNoise=_target(dev, 0.5))
        peak = dev.streamPeakGBps(1 << 30, 10)
        for _ in range(10):
            n = dev.adaptiveSelect(ap)
        windows = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(50):
                dev.adaptiveSelect(ap)
            windows.append((time.perf_counter() - t0) * 1e6 / 50)
        nbytes = pixels * (16 + 4 + 0.25) + n * 4
        print(json.dumps({"mode": mode, "active": n, "us_per_call": min(windows), "windows": windows, "stream_peak_gbps": peak, "bytes": nbytes,
                          "floor_us": nbytes / (peak * 1e9) * 1e6}))
    else:
        twk, dev = _device(True)
        # share 1.0: a minSamples no pixel has makes every pixel UNKNOWN, and so selected (a target alone leaves out the pixels whose
        # samples were all equal, e = 0: the background and the light's face, about half of this frame)
        ap = twk.Adaptive(targetNoise=1.0, minSamples=1 << 24, maxSamples=1 << 30) if share >= 1.0 else twk.Adaptive(targetNoise=_target(dev, share), maxSamples=1 << 30)
        n = dev.adaptiveSelect(ap)
        walls = []
        for _ in range(REPEATS + 1):
            dev.synchronizeStream()
            t0 = time.perf_counter()
            dev.renderAdaptive(SAMPLES)
            dev.synchronizeStream()
            walls.append(time.perf_counter() - t0)
        print(json.dumps({"mode": mode, "share": share, "active": n, "paths": n * SAMPLES, "ms": min(walls[1:]) * 1e3, "all_ms": [w * 1e3 for w in walls]}))
    dev.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], float(sys.argv[3]))
        return 0
    rows = []
    for mode, share in [("select", 0.5), ("uniform", 1.0)] + [("adaptive", s) for s in SHARES]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(share)], capture_output=True, text=True, timeout=CHILD_SECONDS)
        if r.returncode != 0:
            print(f"configuration {mode} {share} failed with status {r.returncode}; stopping\n{r.stdout}{r.stderr}", file=sys.stderr)
            return 1
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    pixels = RES[0] * RES[1]
    s = rows[0]
    print(f"twk_adaptive_select on the handle's own buffers, {RES[0]}x{RES[1]}, C2 at {UNIFORM} spp, {s['active']} of {pixels} selected: the smallest of {REPEATS} windows of 50 calls, each call synchronising\n")
    print("| us per call | stream peak GB/s | compulsory bytes | floor us | us / floor |")
    print("|---|---|---|---|---|")
    print(f"| {s['us_per_call']:.1f} | {s['stream_peak_gbps']:.0f} | {s['bytes'] / 1e6:.1f} MB | {s['floor_us']:.1f} | {s['us_per_call'] / s['floor_us']:.2f} |")
    print("\nevery window, us per call: " + ", ".join(f"{w:.1f}" for w in s["windows"]))
    u = rows[1]
    print(f"\none pass of {SAMPLES} samples between two synchronisations, the smallest of {REPEATS} after one warm-up pass\n")
    print("| pass | active share | paths | ms per pass | ns per path | time / uniform pass |")
    print("|---|---|---|---|---|---|")
    print(f"| uniform (fused primary, tile entry points) | 1 | {u['paths']} | {u['ms']:.3f} | {u['ms'] * 1e6 / u['paths']:.3f} | 1 |")
    for r in rows[2:]:
        print(f"| adaptive | {r['active'] / pixels:.4f} | {r['paths']} | {r['ms']:.3f} | {r['ms'] * 1e6 / max(1, r['paths']):.3f} | {r['ms'] / u['ms']:.3f} |")
    print("\nevery pass, ms:\n")
    for r in rows[1:]:
        print(f"- {r['mode']} {r.get('share', 1.0)}: " + ", ".join(f"{w:.3f}" for w in r["all_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
