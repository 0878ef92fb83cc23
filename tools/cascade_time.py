#!/usr/bin/env python3
"""Cost of the firefly cascade on a 1920x1080 Cornell frame (C2): a batch-8 uniform pass with the cascade off and on, the resolve
alone, and the bytes of the layers.

pass: iterations 0 .. 7 rendered as one wavefront pass between two synchronisations, wall clock, the smallest of `repeats`; the
accumulate kernel's own share is the profile's (twk_profile_enable: a hipEvent pair around every launch), which is where the
cascade's cost sits: K more float4 read and written per launch index and the split of every sample. With --parent DIR (a built
checkout of the commit before the cascade) the off case is also timed on that library: the CascadeOff builds are meant to cost
what the kernels cost before.
resolve: a window of N asynchronous twk_cascade_resolve on the handle's own layers between two synchronisations, divided by N (the
form of tools/noise_time.py); its floor is its compulsory bytes — K x 16 B read and K x 4 B written by the first launch, K x 16 B
and K x 4 B read (the nine taps of a lambda share its cache lines) and one pixel written by the second — over the stream-copy peak.
Each configuration runs in a child process of its own under a time limit; the first failure ends the run.
usage (GPU box): python tools/cascade_time.py [--parent DIR] [repeats] > table.md"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RES = (1920, 1080)
BATCH = 8
CHILD_SECONDS = 240


def _device(root, cascade):
    sys.path.insert(0, root)
    import tweeker_raytracer_amd as twk
    scenes = os.path.join(root, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    if cascade:
        dev.enableCascade(True)
    dev.setLaunchBatch(BATCH)
    return twk, dev


def child_pass(root, cascade, repeats):
    twk, dev = _device(root, cascade)
    dev.profileEnable(True)

    def one():
        dev.synchronizeStream()
        dev.profileReset()
        t0 = time.perf_counter()
        for it in range(BATCH):
            dev.render(it)
        dev.synchronizeStream()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, dev.profileGet()["accumulate"]["ms"]

    for _ in range(3):
        one()
    runs = [one() for _ in range(repeats)]
    print(json.dumps({"cascade": bool(cascade), "root": root, "pass_ms": min(r[0] for r in runs), "accumulate_ms": min(r[1] for r in runs), "runs": runs,
                      "layer_bytes": (dev.cascadeDevicePointer()[1] if cascade else 0)}))
    dev.close()


def child_resolve(root, calls):
    twk, dev = _device(root, True)
    for it in range(BATCH):
        dev.render(it)
    dev.synchronizeStream()
    peak = dev.streamPeakGBps(1 << 30, 10)

    def window():
        dev.synchronizeStream()
        t0 = time.perf_counter()
        for _ in range(calls):
            dev.cascadeResolve()
        t1 = time.perf_counter()
        dev.synchronizeStream()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e6 / calls, (t1 - t0) * 1e6 / calls

    for _ in range(10):
        dev.cascadeResolve()
    windows = [window() for _ in range(5)]
    layers = twk._lib.TWK_CASCADE_LAYERS
    nbytes = RES[0] * RES[1] * (layers * (16 + 4) + layers * (16 + 4) + 16)
    print(json.dumps({"calls": calls, "us_per_call": min(w[0] for w in windows), "us_submit_per_call": min(w[1] for w in windows), "windows": windows,
                      "stream_peak_gbps": peak, "bytes": nbytes, "floor_us": nbytes / (peak * 1e9) * 1e6, "layers": layers}))
    dev.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child-pass":
        child_pass(args[1], int(args[2]), int(args[3]))
        return 0
    if args and args[0] == "--child-resolve":
        child_resolve(args[1], int(args[2]))
        return 0
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    repeats = int(args[0]) if args else 10
    jobs = [("off", ["--child-pass", ROOT, "0", str(repeats)]), ("on", ["--child-pass", ROOT, "1", str(repeats)]), ("resolve", ["--child-resolve", ROOT, "100"])]
    if parent:
        jobs.insert(0, ("parent", ["--child-pass", parent, "0", str(repeats)]))
    rows = {}
    for name, job in jobs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + job, capture_output=True, text=True, timeout=CHILD_SECONDS)
        if r.returncode != 0:
            print(f"configuration {name} failed with status {r.returncode}; stopping\n{r.stdout}{r.stderr}", file=sys.stderr)
            return 1
        rows[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"C2 {RES[0]}x{RES[1]}, one uniform pass of {BATCH} iterations (0 .. {BATCH - 1}) between two synchronisations, the smallest of {repeats} after 3 warm-up passes\n")
    print("| cascade | pass ms (wall clock) | accumulate kernel ms (hipEvent pair) | layers |")
    print("|---|---|---|---|")
    names = {"parent": "off, the commit before", "off": "off", "on": "on (6 layers)"}
    for name in ("parent", "off", "on"):
        if name in rows:
            r = rows[name]
            print(f"| {names[name]} | {r['pass_ms']:.3f} | {r['accumulate_ms']:.3f} | {r['layer_bytes'] / 1e6:.1f} MB |")
    r = rows["resolve"]
    print(f"\ntwk_cascade_resolve on the handle's own layers ({r['layers']} layers): {r['us_per_call']:.1f} us per call (the smallest of 5 windows of {r['calls']} calls; "
          f"the host's submission alone {r['us_submit_per_call']:.1f} us), compulsory bytes {r['bytes'] / 1e6:.1f} MB, stream peak {r['stream_peak_gbps']:.0f} GB/s, "
          f"floor {r['floor_us']:.1f} us, us / floor {r['us_per_call'] / r['floor_us']:.2f}")
    print("\nevery run, pass ms / accumulate ms:\n")
    for name in ("parent", "off", "on"):
        if name in rows:
            print(f"- {names[name]}: " + "; ".join(f"{a:.3f} / {b:.3f}" for a, b in rows[name]["runs"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
