#!/usr/bin/env python3
"""Cost of twk_temporal_accumulate_cascade on a 1920x1080 Cornell frame (C2, GPU box), beside the floor of its compulsory bytes.

Two frames of 4 spp a small orbit step apart with the cascade on: the first frame's layers and geometry AOV are copied aside as the
history, the second frame's are the handle's own. Timed: a window of N asynchronous explicit-form calls between two synchronisations,
divided by N, the smallest of 5 windows after a warm-up (the form of tools/cascade_time.py), for every layer count given. The floor:
32 + 48 K bytes per pixel — the current geometry and K layers read once, the history geometry and K layers read once in aggregate
(every history pixel is gathered by about one pixel's four taps, which share it with their neighbours' through the cache), K layers
written — at the stream-copy rate twk_stream_peak_gbps reports in the same process. The share of pixels that took history is printed:
a pixel that passes through reads no history layers.
usage (GPU box): python tools/temporal_cascade_time.py [layers ...] > table.md"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (1920, 1080)
SPP, STEP, CALLS = 4, 0.002, 200


def main():
    import tweeker_raytracer_amd as twk
    L = twk._lib
    layer_counts = [int(a) for a in sys.argv[1:]] or [L.TWK_CASCADE_LAYERS]
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    i = app.info
    camera = lambda frame: twk.camera_frustum(tuple(i.center), i.phi + STEP * frame, i.theta, i.fov, i.distance, RES[0] / RES[1])
    dev = twk.Device(ordinal=0, miss=i.miss)
    app.initDevice(dev)
    dev.enableGeometry(True)
    hip = C.CDLL("libamdhip64.so")
    pixels = RES[0] * RES[1]
    shape = (RES[1], RES[0])
    peak = dev.streamPeakGBps(1 << 30, 10)
    print(f"C2 {RES[0]}x{RES[1]}, two frames of {SPP} spp {STEP} of a turn apart; twk_temporal_accumulate_cascade, explicit form, {CALLS} calls per window, the smallest of 5 windows; "
          f"stream peak {peak:.0f} GB/s (twk_stream_peak_gbps, 1 GiB x 10).\n")
    print("| layers | us per call | compulsory bytes (32 + 48 K per pixel) | floor us | us / floor | share of pixels with history |")
    print("|---|---|---|---|---|---|")

    def allocate(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p

    for K in layer_counts:
        cascade = L.Cascade(K, L.TWK_CASCADE_START, L.TWK_CASCADE_BASE)
        dev.enableCascade(True, cascade)
        layer_bytes, plane = pixels * K * 16, pixels * 16
        history, history_geometry, out = allocate(layer_bytes), allocate(plane), allocate(layer_bytes)

        def frame(index):
            dev.updateCamera(0, camera(index))
            dev.setSampleOffset(index * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            dev.synchronizeStream()

        frame(0)
        assert hip.hipMemcpy(history, C.c_void_p(dev.cascadeDevicePointer()[0]), C.c_size_t(layer_bytes), 3) == 0
        assert hip.hipMemcpy(history_geometry, C.c_void_p(dev.geometryDevicePointer()[0]), C.c_size_t(plane), 3) == 0
        frame(1)
        layers, geometry = dev.cascadeDevicePointer()[0], dev.geometryDevicePointer()[0]
        call = lambda: dev.temporalAccumulateCascade(None, cascade, layers, geometry, history.value, history_geometry.value, camera(0), shape, out.value)

        def window():
            dev.synchronizeStream()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            dev.synchronizeStream()
            return (time.perf_counter() - t0) * 1e6 / CALLS

        for _ in range(10):
            call()
        us = min(window() for _ in range(5))
        merged = np.empty((pixels, 4), np.float32)  # layer 0
        assert hip.hipMemcpy(merged.ctypes.data_as(C.c_void_p), out, C.c_size_t(plane), 2) == 0
        share = float((merged[:, 3] > SPP).mean())
        nbytes = pixels * (32 + 48 * K)
        floor = nbytes / (peak * 1e9) * 1e6
        print(f"| {K} | {us:.1f} | {nbytes / 1e6:.0f} MB | {floor:.1f} | {us / floor:.2f} | {share:.3f} |")
        for p in (history, history_geometry, out):
            hip.hipFree(p)
    dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
