#!/usr/bin/env python3
"""Cost of twk_temporal_accumulate_rectified on a 1920x1080 Cornell frame (C2, GPU box), beside twk_temporal_accumulate on the same
buffers and the floor of its compulsory bytes.

Two frames of 4 spp a small orbit step apart: the first frame's colour (widened), moments and geometry AOV are copied aside as the
history, the second frame's are the handle's own. Timed: a window of N asynchronous explicit-form calls between two
synchronisations, divided by N, the smallest of 5 windows after a warm-up (the form of tools/temporal_cascade_time.py) — the plain
merge, then the rectified one (BOTH of its launches) at every radius. The floors, at the stream-copy rate twk_stream_peak_gbps
reports in the same process, P = the bytes of a pixel of the output format (16 or 8):
  plain      P + 32 read of the frame, 48 of the history in aggregate (every history pixel is gathered by about one pixel's four
             taps, which share it with their neighbours' through the cache), P + 32 written                   = 112 + 2 P
  launch 1   the same reads, 32 written (the two scratch streams)                                                = 112 + P
  launch 2   P + 16 of the frame and 32 of the scratch read (the halo's re-reads are its neighbours' own lines), P + 32 + 4 written
                                                                                                                  = 84 + 2 P
The split between the two launches is not visible from the host: run the tool under `rocprofv3 --kernel-trace --stats` for it.
With TWK_LIB pointing at builds with -DTWK_RECTIFY_RUNTIME_FROM=1 (every radius a run-time value) and =5 (every radius a template
parameter; tools/ab_variant.sh) the same table gives the two sides of the A/B that csrc/temporal_rectify_kernels.hip's default rests on.
usage (GPU box): python tools/temporal_rectify_time.py [half] > table.md"""
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
    half = "half" in sys.argv[1:]
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    i = app.info
    camera = lambda frame: twk.camera_frustum(tuple(i.center), i.phi + STEP * frame, i.theta, i.fov, i.distance, RES[0] / RES[1])
    dev = twk.Device(ordinal=0, miss=i.miss)
    app.initDevice(dev)
    if half:
        dev.setOutputFormat(1)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    hip = C.CDLL("libamdhip64.so")
    pixels = RES[0] * RES[1]
    shape = (RES[1], RES[0])
    P = 8 if half else 16
    peak = dev.streamPeakGBps(1 << 30, 10)
    print(f"C2 {RES[0]}x{RES[1]}, {'RGBA16F' if half else 'RGBA32F'}, two frames of {SPP} spp {STEP} of a turn apart; explicit forms, {CALLS} calls per window, the smallest of 5 "
          f"windows; stream peak {peak:.0f} GB/s (twk_stream_peak_gbps, 1 GiB x 10); library {os.path.basename(L.LIB_PATH)}.\n")

    def allocate(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p

    def frame(index):
        dev.updateCamera(0, camera(index))
        dev.setSampleOffset(index * SPP)
        for it in range(SPP):
            dev.render(it)
        dev.renderGeometry()
        dev.synchronizeStream()

    plane = pixels * 16
    frame(0)
    first = dev.getOutputBufferHost()  # widened: the history's colour is f32 in both formats
    h_colour, h_moments, h_geometry = allocate(plane), allocate(plane), allocate(plane)
    assert hip.hipMemcpy(h_colour, first.ctypes.data_as(C.c_void_p), C.c_size_t(plane), 1) == 0
    assert hip.hipMemcpy(h_moments, C.c_void_p(dev.momentsDevicePointer()[0]), C.c_size_t(plane), 3) == 0
    assert hip.hipMemcpy(h_geometry, C.c_void_p(dev.geometryDevicePointer()[0]), C.c_size_t(plane), 3) == 0
    frame(1)
    current = L.TemporalFrame(dev.outputDevicePointer()[0], dev.momentsDevicePointer()[0], dev.geometryDevicePointer()[0], camera(1))
    history = L.TemporalFrame(h_colour.value, h_moments.value, h_geometry.value, camera(0))
    outs = [allocate(pixels * P), allocate(plane), allocate(plane), allocate(pixels * 4)]
    o = [p.value for p in outs]
    tp = L.Temporal(maxHistory=32, positionTolerance=0.01)

    def timed(call):
        def window():
            dev.synchronizeStream()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            dev.synchronizeStream()
            return (time.perf_counter() - t0) * 1e6 / CALLS
        for _ in range(10):
            call()
        return min(window() for _ in range(5))

    floor = lambda nbytes: nbytes * pixels / (peak * 1e9) * 1e6
    print("| call | us per call | compulsory bytes per pixel | floor us | us / floor | share of pixels with trust < 1 |")
    print("|---|---|---|---|---|---|")
    us = timed(lambda: dev.temporalAccumulate(tp, current, history, shape, o[0], o[1], o[2]))
    print(f"| twk_temporal_accumulate | {us:.1f} | {112 + 2 * P} | {floor(112 + 2 * P):.1f} | {us / floor(112 + 2 * P):.2f} | |")
    nbytes = (112 + P) + (84 + 2 * P)
    for radius in (1, 2, 3, 4):
        rp = L.TemporalRectify(radius=radius)
        us = timed(lambda: dev.temporalAccumulateRectified(tp, rp, current, history, shape, *o))
        trust = np.empty(pixels, np.float32)
        assert hip.hipMemcpy(trust.ctypes.data_as(C.c_void_p), outs[3], C.c_size_t(pixels * 4), 2) == 0
        print(f"| twk_temporal_accumulate_rectified, radius {radius} (both launches) | {us:.1f} | {nbytes} | {floor(nbytes):.1f} | {us / floor(nbytes):.2f} | {float((trust < 1).mean()):.4f} |")
    for p in outs + [h_colour, h_moments, h_geometry]:
        hip.hipFree(p)
    dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
