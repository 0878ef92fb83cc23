#!/usr/bin/env python3
"""Time of one twk_assemble launch against two yardsticks, for 1920x1080 and 3840x2160, 2 / 3 / 8 handles on one device, three
plane sets and both output formats.

the launch: a window of CALLS asynchronous twk_assemble on pre-gathered blocks (device memory on the handle's own device, one
[N][H][launchWidth] block per plane and layer) between two synchronisations, divided by CALLS; the smallest of WINDOWS windows after
a warm-up window.
yardstick (i): the floor of the compulsory bytes — every in-picture element read once and written once, padding excluded — at the
stream-copy peak measured in the same process (twk_stream_peak_gbps).
yardstick (ii): the same planes moved by one twk_compositor / twk_compositor_half launch each, on the same blocks, each into a
destination of its own as large as the assembled plane (one destination shared by all of them would stay in the last-level cache
between the launches, which no caller's do), timed the same way; the sample counts have no compositor path (it knows 8- and
16-byte pixels only) and are left out of that sum, which is said in the table.
Both are called through ctypes with their arguments built beforehand; the host's share of a call (the window's time before the
closing synchronisation) is printed beside the assemble time, since a window cannot be shorter than what the host takes to submit it.
The path column is the rule of csrc/assemble_device.h applied to the shape: a plane takes the 16-byte path when tileSize.x x
elementBytes >= 16 and width x elementBytes is a multiple of 16 (the blocks here are 16-byte aligned).
usage (GPU box): python tools/assemble_time.py > table.md"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESOLUTIONS = [(1920, 1080), (3840, 2160)]
HANDLES = [2, 3, 8]
CALLS, WINDOWS = 20, 5
LAYERS = 6


def main():
    import tweeker_raytracer_amd as twk
    L = twk._lib
    hip = L.lib  # the HIP runtime the library links, through its own handle
    OUTPUT, ALBEDO, NORMAL, MOMENTS, COUNTS, CASCADE = range(6)
    sets = [("beauty", (OUTPUT,)), ("beauty + AOVs + moments", (OUTPUT, ALBEDO, NORMAL, MOMENTS)),
            ("those + counts + 6 cascade layers", (OUTPUT, ALBEDO, NORMAL, MOMENTS, COUNTS, CASCADE))]
    names = ["beauty", "albedo", "normal", "moments", "counts", "cascade"]
    scenes = os.path.join(ROOT, "scenes")

    def malloc(nbytes):
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) != 0 or hip.hipMemset(p, 0x3c, C.c_size_t(nbytes)) != 0:
            raise RuntimeError(f"hipMalloc / hipMemset of {nbytes} bytes failed")
        return p

    def timed(dev, call):
        def window():
            dev.synchronizeStream()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            t1 = time.perf_counter()
            dev.synchronizeStream()
            return (time.perf_counter() - t0) * 1e6 / CALLS, (t1 - t0) * 1e6 / CALLS
        window()
        return min(window() for _ in range(WINDOWS))

    print(f"one twk_assemble launch on pre-gathered blocks, us per call: the smallest of {WINDOWS} windows of {CALLS} asynchronous calls between two synchronisations, "
          f"after one warm-up window; tile 8x8\n")
    print("| resolution | handles | format | planes | path per plane | assemble us | of it host submission us | floor us (i) | assemble / floor | compositor launches us (ii) | assemble / compositors |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    peak = None
    for width, height in RESOLUTIONS:
        app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
        app.setResolution(width, height)
        for n in HANDLES:
            for half in (False, True):
                dev = twk.Device(ordinal=0, index=0, count=n, miss=app.info.miss)
                dev.enableAov(True)
                dev.enableMoments(True)
                dev.enableAdaptive(True)
                dev.enableCascade(True, L.Cascade(layers=LAYERS))
                dev.setOutputFormat(L.TWK_OUTPUT_HALF4 if half else L.TWK_OUTPUT_FLOAT4)
                state = app.state
                state.distribution = 1
                dev.setState(state)
                if peak is None:
                    peak = dev.streamPeakGBps(1 << 30, 10)
                lw, tile_x = dev.launchWidth, state.tileSize[0]
                pixel = 8 if half else 16
                element = {OUTPUT: pixel, ALBEDO: pixel, NORMAL: pixel, MOMENTS: 16, COUNTS: 4, CASCADE: 16}
                layers = {p: (LAYERS if p == CASCADE else 1) for p in range(6)}
                blocks = {p: malloc(n * layers[p] * height * lw * element[p]) for p in range(6)}
                full = {p: malloc(width * height * layers[p] * element[p]) for p in range(6) if p != COUNTS}  # the compositor launches' destinations
                # device d's buffer of plane p inside the block: [N][layers][H][launchWidth]
                sources = (L.AssemblySource * n)(*[L.AssemblySource({p: blocks[p].value + d * layers[p] * height * lw * element[p] for p in range(6)}) for d in range(n)])
                for label, planes in sets:
                    mask = C.c_uint(sum(1 << p for p in planes))
                    us, submit = timed(dev, lambda: L.check(L.lib.twk_assemble(dev.handle, mask, sources, n)))
                    nbytes = 2 * width * height * sum(element[p] * layers[p] for p in planes)
                    floor = nbytes / (peak * 1e9) * 1e6

                    # (a layer's block: the devices' k-th layers are not contiguous in the block above, so this times the launch on a
                    # block of the same size and shape, which is what its cost depends on)
                    launches = [(L.lib.twk_compositor_half if element[p] == 8 else L.lib.twk_compositor, C.c_void_p(blocks[p].value + k * n * height * lw * element[p]),
                                 C.c_void_p(full[p].value + k * width * height * element[p])) for p in planes if p != COUNTS for k in range(layers[p])]

                    def compositors():
                        for fn, tiles, out in launches:
                            L.check(fn(dev.handle, tiles, out))
                    other, _ = timed(dev, compositors)
                    path = ", ".join(f"{names[p]} {'16 B' if tile_x * element[p] >= 16 and (width * element[p]) % 16 == 0 else 'element'}" for p in planes)
                    left_out = " (counts left out)" if COUNTS in planes else ""
                    print(f"| {width}x{height} | {n} | {'RGBA16F' if half else 'RGBA32F'} | {label} | {path} | {us:.1f} | {submit:.1f} | {floor:.1f} | {us / floor:.2f} | {other:.1f}{left_out} | {us / other:.2f} |")
                    sys.stdout.flush()
                dev.synchronizeStream()
                for b in list(blocks.values()) + list(full.values()):
                    hip.hipFree(b)
                dev.close()
        app.close()
    print(f"\nstream-copy peak (twk_stream_peak_gbps, 1 GiB, 10 repeats): {peak:.0f} GB/s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
