#!/usr/bin/env python3
"""Cost of twk_denoise (the a-trous wavelet filter at the optixDenoiserInvoke seam) on a 1920x1080 Cornell frame, beside its floor.

For RGBA32F and RGBA16F, with the defaults (3 levels) and with 5 levels: wall clock of N calls plus one synchronisation after a
warm-up, in ms per frame; the floor = the compulsory stream bytes of the levels (per level and pixel one float4 of colour read,
one written, one float4 per guide in use read) divided by the stream-copy peak measured in the same process
(twk_stream_peak_gbps); and their ratio. Every configuration runs in a child process of its own under a time limit; the first
failure ends the run. A second table is the A/B of the two builds of the level kernel, per step: RGBA32F at 5 levels with the
LDS-staged build on the steps up to M (TWK_DENOISE_LDS_MAX_STEP=M) and the direct-load build above, M = 0, 1, 2, 4, 8, 16; the
difference of two neighbouring rows is what the staged build gains or loses on that one step.
With --variance the tables are those of twk_denoise_variance (the variance-guided, firefly-clamping mode) instead: per format and
level count its ms per frame beside twk_denoise's, both timed in the same process in alternating windows, and the floor of the moments
pass (its compulsory stream bytes: the colour read and written, one float4 per guide read) over the same stream-copy peak. The
moments kernel's own time comes from a kernel trace of one child (rocprofv3 --kernel-trace --stats -- python tools/denoise_time.py
--child 0 3 50 1), in a run of its own.
With --sampled the same table compares twk_denoise_variance_sampled (the handle's own luminance moments, the default minSamples)
with twk_denoise_variance, again in alternating windows: the expected extra is one 16-byte load per pixel in the moments pass.
usage (GPU box): python tools/denoise_time.py [--variance | --sampled] [calls] > table.md"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (1920, 1080)
CHILD_SECONDS = 180


def child(fmt, levels, calls, variance=False):  # variance: 0 / False twk_denoise alone, 1 beside twk_denoise_variance, 2 twk_denoise_variance beside twk_denoise_variance_sampled
    import tweeker_raytracer_amd as twk
    L = twk._lib
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableAov(True)
    if variance == 2:
        dev.enableMoments(True)
    dev.setOutputFormat(fmt)
    for it in range(4):
        dev.render(it)
    dev.synchronizeStream()
    peak = dev.streamPeakGBps(1 << 30, 10)
    dn = L.Denoiser(iterations=levels)

    def denoise(dv):
        if dv == "sampled":
            dev.denoise(dn, variance=L.DenoiserVariance(), moments=True)
        else:
            dev.denoise(dn, variance=dv)

    def window(dv):
        t0 = time.perf_counter()
        for _ in range(calls):
            denoise(dv)
        dev.synchronizeStream()
        return (time.perf_counter() - t0) * 1e3 / calls

    modes = [L.DenoiserVariance(), "sampled"] if variance == 2 else ([None, L.DenoiserVariance()] if variance else [None])
    for dv in modes:
        for _ in range(5):
            denoise(dv)
    dev.synchronizeStream()
    windows = [[window(dv) for dv in modes] for _ in range(3 if variance else 1)]  # alternating: plain, variance, plain, ...
    ms = min(w[0] for w in windows) if variance else windows[0][0]
    pixels = RES[0] * RES[1]
    guides = {0: 0, 1: 1, 2: 2}[dn.inputKind]
    level_bytes = levels * pixels * 16 * (2 + guides)
    px = 8 if fmt else 16
    ends_bytes = pixels * (px * (1 + guides) + 16 * (1 + guides)) + pixels * (px * 2 + 16 * (1 + (1 if dn.demodulateAlbedo else 0)))  # prepare + finish
    extra = {}
    if variance:
        moments_bytes = pixels * 16 * (2 + guides)
        extra = {"ms_per_frame_variance": min(w[1] for w in windows), "windows": windows, "moments_stream_bytes": moments_bytes, "floor_ms_moments": moments_bytes / (peak * 1e9) * 1e3}
    out = dev.readDenoised()
    print(json.dumps({**extra, "format": "RGBA16F" if fmt else "RGBA32F", "levels": levels, "calls": calls, "ms_per_frame": ms, "stream_peak_gbps": peak,
                      "level_stream_bytes": level_bytes, "floor_ms_levels": level_bytes / (peak * 1e9) * 1e3,
                      "floor_ms_with_prepare_and_finish": (level_bytes + ends_bytes) / (peak * 1e9) * 1e3, "mean": float(out[..., :3].mean())}))
    dev.close()


def run_child(fmt, levels, calls, lds_max_step=None, variance=False):
    env = dict(os.environ)
    if lds_max_step is not None:
        env["TWK_DENOISE_LDS_MAX_STEP"] = str(lds_max_step)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(fmt), str(levels), str(calls), str(int(variance))], capture_output=True, text=True, timeout=CHILD_SECONDS, env=env)
    if r.returncode != 0:
        print(f"configuration format {fmt}, {levels} levels, LDS up to step {lds_max_step} failed with status {r.returncode}; stopping\n{r.stdout}{r.stderr}", file=sys.stderr)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def main_variance(calls, sampled=False):
    rows = []
    for fmt in (0, 1):
        for levels in (3, 5):
            row = run_child(fmt, levels, calls, variance=2 if sampled else 1)
            if row is None:
                return 1
            rows.append(row)
    if sampled:
        print(f"twk_denoise_variance_sampled beside twk_denoise_variance, {RES[0]}x{RES[1]}, inputKind RGB_ALBEDO_NORMAL, demodulated, the smaller of 3 alternating windows of {calls} calls + 1 sync each, after 5 warm-up calls\n")
        print("| format | levels | twk_denoise_variance ms | twk_denoise_variance_sampled ms | ratio | extra load bytes | its floor ms |")
        print("|---|---|---|---|---|---|---|")
        for r in rows:
            extra = RES[0] * RES[1] * 16
            print(f"| {r['format']} | {r['levels']} | {r['ms_per_frame']:.3f} | {r['ms_per_frame_variance']:.3f} | {r['ms_per_frame_variance'] / r['ms_per_frame']:.3f} | {extra / 1e6:.0f} MB | {extra / (r['stream_peak_gbps'] * 1e9) * 1e3:.4f} |")
        print("\nevery window, ms per frame (twk_denoise_variance, twk_denoise_variance_sampled):\n")
        for r in rows:
            print(f"- {r['format']}, {r['levels']} levels: " + "; ".join(f"{a:.3f}, {b:.3f}" for a, b in r["windows"]))
        return 0
    print(f"twk_denoise_variance beside twk_denoise, {RES[0]}x{RES[1]}, inputKind RGB_ALBEDO_NORMAL, demodulated, the smaller of 3 alternating windows of {calls} calls + 1 sync each, after 5 warm-up calls\n")
    print("| format | levels | twk_denoise ms | twk_denoise_variance ms | ratio | stream peak GB/s | moments stream bytes | floor ms (moments) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['format']} | {r['levels']} | {r['ms_per_frame']:.3f} | {r['ms_per_frame_variance']:.3f} | {r['ms_per_frame_variance'] / r['ms_per_frame']:.2f} | {r['stream_peak_gbps']:.0f} | "
              f"{r['moments_stream_bytes'] / 1e6:.0f} MB | {r['floor_ms_moments']:.3f} |")
    print("\nevery window, ms per frame (twk_denoise, twk_denoise_variance):\n")
    for r in rows:
        print(f"- {r['format']}, {r['levels']} levels: " + "; ".join(f"{a:.3f}, {b:.3f}" for a, b in r["windows"]))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else 0)
        return 0
    argv = [a for a in sys.argv[1:] if a not in ("--variance", "--sampled")]
    calls = int(argv[0]) if argv else 100
    if "--sampled" in sys.argv[1:]:
        return main_variance(calls, sampled=True)
    if "--variance" in sys.argv[1:]:
        return main_variance(calls)
    rows = []
    for fmt in (0, 1):
        for levels in (3, 5):
            row = run_child(fmt, levels, calls)
            if row is None:
                return 1
            rows.append(row)
    ab = []
    for m in (0, 1, 2, 4, 8, 16):
        row = run_child(0, 5, calls, m)
        if row is None:
            return 1
        ab.append((m, row))
    print(f"twk_denoise, {RES[0]}x{RES[1]}, inputKind RGB_ALBEDO_NORMAL, demodulated, {calls} calls + 1 sync after 5 warm-up calls\n")
    print("| format | levels | ms per frame | stream peak GB/s | level stream bytes | floor ms (levels) | ms / floor | floor ms (with prepare + finish) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['format']} | {r['levels']} | {r['ms_per_frame']:.3f} | {r['stream_peak_gbps']:.0f} | {r['level_stream_bytes'] / 1e6:.0f} MB | {r['floor_ms_levels']:.3f} | "
              f"{r['ms_per_frame'] / r['floor_ms_levels']:.2f} | {r['floor_ms_with_prepare_and_finish']:.3f} |")
    print(f"\nthe two builds of the level kernel, RGBA32F, 5 levels (steps 1 - 16): LDS-staged up to step M, direct-load above\n")
    print("| M | ms per frame | the staged build on step M alone, ms |")
    print("|---|---|---|")
    for i, (m, r) in enumerate(ab):
        delta = "" if i == 0 else f"{r['ms_per_frame'] - ab[i - 1][1]['ms_per_frame']:+.3f}"
        print(f"| {m} | {r['ms_per_frame']:.3f} | {delta} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
