#!/usr/bin/env python3
"""Cost of the geometry guide (twk_denoise_geometry) on a 1920x1080 Cornell frame, beside the call without it and beside its floor.

For each mode of the filter (plain, variance-guided, sampled variance), RGBA32F, at 3 and at 5 levels: ms per frame of the
ungeometric call and of twk_denoise_geometry on the handle's own buffers, timed in the same process in alternating windows (the
smaller of 3 windows of N calls + one synchronisation each, after 5 warm-up calls); their difference; and the floor of the guide's
compulsory bytes — one more 16-byte read per pixel and level (and per pixel in the moments pass of the variance modes) — over the
stream-copy peak measured in the same process (twk_stream_peak_gbps). Every configuration runs in a child process of its own under
a time limit; the first failure ends the run. A second table is the A/B of the two builds of the level kernel with four streams,
per step, as tools/denoise_time.py has it for three: the plain mode at 5 levels with the LDS-staged build up to step M
(TWK_DENOISE_LDS_MAX_STEP=M), M = 0, 1, 2, 4, 8, 16.
usage (GPU box): python tools/denoise_geometry_time.py [calls] > table.md"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (1920, 1080)
CHILD_SECONDS = 180
MODES = ("plain", "variance", "sampled")


def child(mode, levels, calls):
    import tweeker_raytracer_amd as twk
    L = twk._lib
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableAov(True)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    for it in range(4):
        dev.render(it)
    dev.renderGeometry()
    dev.synchronizeStream()
    peak = dev.streamPeakGBps(1 << 30, 10)
    dn, dg = L.Denoiser(iterations=levels), L.DenoiserGeometry()
    older = {"plain": {}, "variance": {"variance": L.DenoiserVariance()}, "sampled": {"variance": L.DenoiserVariance(), "moments": True}}[mode]

    def window(geometry):
        t0 = time.perf_counter()
        for _ in range(calls):
            dev.denoise(dn, geometry=geometry, **older)
        dev.synchronizeStream()
        return (time.perf_counter() - t0) * 1e3 / calls

    for geometry in (None, dg):
        for _ in range(5):
            dev.denoise(dn, geometry=geometry, **older)
    dev.synchronizeStream()
    windows = [[window(None), window(dg)] for _ in range(3)]  # alternating: without, with, without, ...
    pixels = RES[0] * RES[1]
    extra = pixels * 16 * (levels + (0 if mode == "plain" else 1))
    out = dev.readDenoised()
    print(json.dumps({"mode": mode, "levels": levels, "calls": calls, "ms_without": min(w[0] for w in windows), "ms_with": min(w[1] for w in windows), "windows": windows,
                      "stream_peak_gbps": peak, "extra_bytes": extra, "floor_ms": extra / (peak * 1e9) * 1e3, "mean": float(out[..., :3].mean())}))
    dev.close()


def run_child(mode, levels, calls, lds_max_step=None):
    env = dict(os.environ)
    if lds_max_step is not None:
        env["TWK_DENOISE_LDS_MAX_STEP"] = str(lds_max_step)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(levels), str(calls)], capture_output=True, text=True, timeout=CHILD_SECONDS, env=env)
    if r.returncode != 0:
        print(f"configuration {mode}, {levels} levels, LDS up to step {lds_max_step} failed with status {r.returncode}; stopping\n{r.stdout}{r.stderr}", file=sys.stderr)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return 0
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rows = []
    for mode in MODES:
        for levels in (3, 5):
            row = run_child(mode, levels, calls)
            if row is None:
                return 1
            rows.append(row)
    ab = []
    for m in (0, 1, 2, 4, 8, 16):
        row = run_child("plain", 5, calls, m)
        if row is None:
            return 1
        ab.append((m, row))
    print(f"twk_denoise_geometry beside the call without the guide, {RES[0]}x{RES[1]}, RGBA32F, inputKind RGB_ALBEDO_NORMAL, demodulated, the handle's own buffers; "
          f"the smaller of 3 alternating windows of {calls} calls + 1 sync each, after 5 warm-up calls\n")
    print("| mode | levels | without ms | with the guide ms | difference ms | ratio | stream peak GB/s | the guide's compulsory bytes | their floor ms | difference / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        d = r["ms_with"] - r["ms_without"]
        print(f"| {r['mode']} | {r['levels']} | {r['ms_without']:.3f} | {r['ms_with']:.3f} | {d:+.3f} | {r['ms_with'] / r['ms_without']:.3f} | {r['stream_peak_gbps']:.0f} | "
              f"{r['extra_bytes'] / 1e6:.0f} MB | {r['floor_ms']:.3f} | {d / r['floor_ms']:.2f} |")
    print("\nevery window, ms per frame (without, with):\n")
    for r in rows:
        print(f"- {r['mode']}, {r['levels']} levels: " + "; ".join(f"{a:.3f}, {b:.3f}" for a, b in r["windows"]))
    print("\nthe two builds of the level kernel with four streams, plain mode, 5 levels (steps 1 - 16): LDS-staged up to step M, direct-load above\n")
    print("| M | with the guide ms | the staged build on step M alone, ms | without ms |")
    print("|---|---|---|---|")
    for i, (m, r) in enumerate(ab):
        delta = "" if i == 0 else f"{r['ms_with'] - ab[i - 1][1]['ms_with']:+.3f}"
        print(f"| {m} | {r['ms_with']:.3f} | {delta} | {r['ms_without']:.3f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
