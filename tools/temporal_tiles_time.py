#!/usr/bin/env python3
"""Times of the moving-camera loop on a tiled frame (profiles/r19_temporal_tiles.md), 1920x1080 and 3840x2160, 2 / 3 / 8 handles
sharing ONE device (said in the output), tiles of 8x8, RGBA32F, the Cornell box, 6 cascade layers.

table 1: twk_render_geometry_tile on each handle beside twk_render_geometry of the whole frame on one handle.
table 2: one twk_assemble_devices_with_geometry of the planes the loop's merge reads (beauty, moments, the cascade's layers) beside
         the same twk_assemble_devices without the geometry, and beside the floor of its compulsory bytes (every in-picture element
         read once and written once) at the stream-copy peak measured in the same process.
table 3: the post chain of one frame on the primary, call by call: that assembly, twk_temporal_accumulate_assembled (both merges),
         twk_cascade_resolve of the merged layers, twk_denoise_variance_sampled on the merged colour and moments.
--geometry-only: twk_render_geometry alone on one handle, REPEATS times over, smallest / median / largest: run once as it is and once
         with --tree <a checkout of the commit before, built> to compare the kernel across the change in one session.

A time is a window of CALLS asynchronous calls between two synchronisations divided by CALLS, the smallest of WINDOWS windows after
a warm-up window (table 1's per-handle times: each handle alone, the others idle).
usage (GPU box): python tools/temporal_tiles_time.py > tables.md"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

RESOLUTIONS = [(1920, 1080), (3840, 2160)]
HANDLES = [2, 3, 8]
CALLS, WINDOWS, REPEATS = 20, 5, 9
OUTPUT, MOMENTS, CASCADE = 0, 3, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package and library are timed")
    args = ap.parse_args()
    root = os.path.abspath(args.tree)
    sys.path.insert(0, root)
    import tweeker_raytracer_amd as twk
    L = twk._lib
    scenes = os.path.join(root, "scenes")

    def window(sync, call):
        sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        sync()
        return (time.perf_counter() - t0) * 1e6 / CALLS

    def timed(sync, call):
        window(sync, call)
        return min(window(sync, call) for _ in range(WINDOWS))

    def handle(app, index, count, distribution):
        dev = twk.Device(ordinal=0, index=index, count=count, miss=app.info.miss)
        dev.enableMoments(True)
        dev.enableGeometry(True)
        dev.enableCascade(True)
        app.initDevice(dev, distribution=distribution)
        dev.render(0)
        dev.synchronizeStream()
        return dev

    def application(width, height):
        app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
        app.setResolution(width, height)
        return app

    if args.geometry_only:
        print(f"twk_render_geometry on one handle, us per call ({CALLS} calls per window, the smallest of {WINDOWS} windows), {REPEATS} repeats; library {L.LIB_PATH}\n")
        print("| resolution | smallest | median | largest |")
        print("|---|---|---|---|")
        for width, height in RESOLUTIONS:
            app = application(width, height)
            dev = handle(app, 0, 1, 0)
            times = sorted(timed(dev.synchronizeStream, dev.renderGeometry) for _ in range(REPEATS))
            print(f"| {width}x{height} | {times[0]:.1f} | {statistics.median(times):.1f} | {times[-1]:.1f} |")
            sys.stdout.flush()
            dev.close()
            app.close()
        return 0

    hip = L.lib  # the HIP runtime the library links, through its own handle
    peak = None
    rows = {1: [], 2: [], 3: []}
    for width, height in RESOLUTIONS:
        app = application(width, height)
        one = handle(app, 0, 1, 0)
        if peak is None:
            peak = one.streamPeakGBps(1 << 30, 10)
        whole = timed(one.synchronizeStream, one.renderGeometry)
        one.close()
        for n in HANDLES:
            devs = [handle(app, i, n, 1) for i in range(n)]
            primary = devs[0]
            primary.enableTemporalCascade(True)
            layers = primary._cascadeLayers

            def sync_all():
                for d in devs:
                    d.synchronizeStream()
            share = [timed(d.synchronizeStream, d.renderGeometryTile) for d in devs]
            rows[1].append(f"| {width}x{height} | {n} | {devs[0].launchWidth} | {whole:.1f} | {min(share):.1f} | {max(share):.1f} | {sum(share):.1f} | {sum(share) / whole:.2f} |")

            planes = (OUTPUT, MOMENTS, CASCADE)
            plain = timed(sync_all, lambda: primary.assemble(devs, planes))
            with_geometry = timed(sync_all, lambda: primary.assembleWithGeometry(devs, planes))
            elements = 16 + 16 + 16 * layers
            floor = 2 * width * height * elements / (peak * 1e9) * 1e6
            floor_g = 2 * width * height * (elements + 16) / (peak * 1e9) * 1e6
            rows[2].append(f"| {width}x{height} | {n} | {plain:.1f} | {floor:.1f} | {plain / floor:.2f} | {with_geometry:.1f} | {floor_g:.1f} | {with_geometry / floor_g:.2f} | "
                           f"{with_geometry - plain:.1f} | {floor_g - floor:.1f} |")

            merge = timed(primary.synchronizeStream, lambda: primary.temporalAccumulateAssembled())
            colour, _, moments, _ = primary.temporalDevicePointers()
            merged_layers, _ = primary.temporalCascadeDevicePointer()
            resolved = C.c_void_p()
            assert hip.hipMalloc(C.byref(resolved), C.c_size_t(width * height * 16)) == 0
            resolve = timed(primary.synchronizeStream, lambda: primary.cascadeResolve(layers=merged_layers, shape=(height, width), resolved=resolved.value))
            denoise = timed(primary.synchronizeStream, lambda: primary.denoise(beauty=colour, albedo=None, normal=None, params=L.Denoiser(inputKind=0), shape=(height, width),
                                                                               moments=moments, minSamples=4))
            total = with_geometry + merge + resolve + denoise
            rows[3].append(f"| {width}x{height} | {n} | {with_geometry:.1f} | {merge:.1f} | {resolve:.1f} | {denoise:.1f} | {total:.1f} | {with_geometry / total:.2f} |")
            primary.synchronizeStream()
            hip.hipFree(resolved)
            for d in devs:
                d.close()
        app.close()

    print(f"us per call: the smallest of {WINDOWS} windows of {CALLS} asynchronous calls between two synchronisations, after one warm-up window. The handles of a frame "
          f"share ONE device; tiles 8x8, RGBA32F, 6 cascade layers.\n")
    print("table 1 — the geometry AOV: twk_render_geometry of the whole frame on one handle, twk_render_geometry_tile on each handle of N (each alone)\n")
    print("| resolution | handles | launchWidth | whole frame us | share, fastest handle us | share, slowest handle us | sum of the shares us | sum / whole |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows[1]))
    print("\ntable 2 — one assembly launch of beauty + moments + 6 cascade layers (8 planes and layers), without and with the geometry (a ninth)\n")
    print("| resolution | handles | without us | floor us | without / floor | with geometry us | floor us | with / floor | the geometry's share us | its floor us |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows[2]))
    print("\ntable 3 — the post chain of one frame on the primary\n")
    print("| resolution | handles | assembly with geometry us | both merges us | resolve us | denoise (sampled variance, defaults) us | chain us | assembly / chain |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows[3]))
    print(f"\nstream-copy peak (twk_stream_peak_gbps, 1 GiB, 10 repeats): {peak:.0f} GB/s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
