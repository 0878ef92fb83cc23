#!/usr/bin/env python3
"""Cost of twk_estimate_noise (csrc/noise_kernels.hip) on the luminance moments of a 1920x1080 Cornell frame, beside its floor.

Without and with the error map: the time of one call (the summary's hipMemsetAsync and the kernel), in microseconds; the floor =
its compulsory bytes (16 B per pixel read, plus 4 B written with the map) divided by the stream-copy peak measured in the same
process (twk_stream_peak_gbps); and their ratio. The handle's stream is not reachable through the C ABI, so no hipEvent can be
recorded around the call from here: a window of N asynchronous calls is bracketed by two synchronisations and its wall clock is
divided by N, the form tools/denoise_time.py uses. The call is short, so that figure is an UPPER bound of the device time: the
host's submission time per call (the loop alone, before the second synchronisation) is printed beside it, and where the two
agree the figure is the host's, not the kernel's. The kernel's own time then comes from a kernel trace of one child, in a run of
its own:
    rocprofv3 --kernel-trace --stats -- python tools/noise_time.py --child 0 200
Each configuration runs in a child process of its own under a time limit; the first failure ends the run.
usage (GPU box): python tools/noise_time.py [calls] > table.md"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (1920, 1080)
CHILD_SECONDS = 180


def child(with_map, calls):
    import ctypes as C
    import tweeker_raytracer_amd as twk
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableMoments(True)
    for it in range(16):
        dev.render(it)
    dev.synchronizeStream()
    peak = dev.streamPeakGBps(1 << 30, 10)
    pixels = RES[0] * RES[1]
    hip = twk._lib.lib  # the HIP runtime the library links
    emap = C.c_void_p()
    if with_map:
        assert hip.hipMalloc(C.byref(emap), C.c_size_t(pixels * 4)) == 0
    estimate = lambda: twk._lib.check(twk._lib.lib.twk_estimate_noise(dev.handle, None, None, C.c_size_t(0), emap if with_map else None))

    def window():
        dev.synchronizeStream()
        t0 = time.perf_counter()
        for _ in range(calls):
            estimate()
        t1 = time.perf_counter()
        dev.synchronizeStream()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e6 / calls, (t1 - t0) * 1e6 / calls

    for _ in range(20):
        estimate()
    windows = [window() for _ in range(5)]
    summary = dev.estimateNoise(errorMap=emap.value if with_map else None)
    nbytes = pixels * (16 + (4 if with_map else 0))
    print(json.dumps({"map": bool(with_map), "calls": calls, "us_per_call": min(w[0] for w in windows), "us_submit_per_call": min(w[1] for w in windows),
                      "windows": windows, "stream_peak_gbps": peak, "bytes": nbytes, "floor_us": nbytes / (peak * 1e9) * 1e6,
                      "valid": summary.valid, "mean": summary.mean, "q95": summary.quantile(0.95)}))
    if with_map:
        hip.hipFree(emap)
    dev.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
        return 0
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rows = []
    for with_map in (0, 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(with_map), str(calls)], capture_output=True, text=True, timeout=CHILD_SECONDS)
        if r.returncode != 0:
            print(f"configuration map={with_map} failed with status {r.returncode}; stopping\n{r.stdout}{r.stderr}", file=sys.stderr)
            return 1
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(f"twk_estimate_noise on the handle's own moments, {RES[0]}x{RES[1]}, C2 at 16 spp, the smallest of 5 windows of {calls} calls between two synchronisations, after 20 warm-up calls\n")
    print("| error map | us per call (window / calls) | of which the host's submission | stream peak GB/s | compulsory bytes | floor us | us / floor |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {'yes' if r['map'] else 'no'} | {r['us_per_call']:.1f} | {r['us_submit_per_call']:.1f} | {r['stream_peak_gbps']:.0f} | {r['bytes'] / 1e6:.1f} MB | "
              f"{r['floor_us']:.1f} | {r['us_per_call'] / r['floor_us']:.2f} |")
    print(f"\nthe frame: {rows[0]['valid']} valid pixels, mean e {rows[0]['mean']:.5f}, 0.95 quantile at most {rows[0]['q95']:.5f}")
    print("\nevery window, us per call (whole window, submission alone):\n")
    for r in rows:
        print(f"- map {'yes' if r['map'] else 'no'}: " + "; ".join(f"{a:.1f}, {b:.1f}" for a, b in r["windows"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
