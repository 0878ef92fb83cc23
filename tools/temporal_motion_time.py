#!/usr/bin/env python3
"""Cost of the Moving builds of the temporal merges (csrc/temporal_motion_device.h) on a 1920x1080 Cornell frame (C2, GPU box), each
beside its parent build on the same buffers in the same run, and the cost of an instance-transform update.

Two frames of 4 spp a small orbit step apart: the first frame's colour (widened), moments, geometry AOV and cascade layers are copied
aside as the history, the second frame's are the handle's own. The table marks as `moved` the instances that cover about half of the
frame's hit pixels, with the IDENTITY as their matrix: the moved pixels read their record and run the transform, and then gather
exactly what the parent build gathers, so the difference of the two times is the cost of the motion alone. Timed: a window of N
asynchronous explicit-form calls between two synchronisations, divided by N, the smallest of 5 windows after a warm-up (the form of
tools/temporal_rectify_time.py), the parent and the Moving build alternating. The floor of the compulsory bytes is the parent's
(tools/temporal_rectify_time.py, tools/temporal_cascade_time.py) plus at most one 64-byte record per pixel, at the stream-copy rate
twk_stream_peak_gbps reports in the same process.

With TWK_LIB pointing at a build with -DTWK_MOTION_STAGED_RECORDS=64 (tools/ab_variant.sh: the table staged in LDS by every block)
the same table is the other side of the A/B that the macro's default in csrc/temporal_motion_device.h rests on.

`update`: instead, buildMilliseconds of twk_build and of a twk_update_instance_transform (the whole rebuild) on C2 and on the C2 room
with the spheres tessellated 1000 x 500 (2.0 M triangles), flattened and two-level.
usage (GPU box): python tools/temporal_motion_time.py [half] [update] > table.md"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (1920, 1080)
SPP, STEP, CALLS = 4, 0.002, 200
K = 6
SCENES = os.path.join(ROOT, "scenes")


def update_times(twk):
    system = open(os.path.join(SCENES, "system_rtigo3_cornell_box.txt")).read()
    scene = open(os.path.join(SCENES, "scene_rtigo3_cornell_box.txt")).read()
    print("| scene | policy | triangles | twk_build ms | twk_update_instance_transform ms (3 updates) |")
    print("|---|---|---|---|---|")
    for name, text in (("C2", scene), ("C2 room, spheres 1000 x 500", scene.replace("sphere 180 90", "sphere 1000 500"))):
        for policy, flatten in (("flattened (default)", None), ("two-level", (0, 0))):
            app = twk.Application(system_text=system, scene_text=text)
            app.setResolution(256, 256)
            dev = twk.Device(ordinal=0, miss=app.info.miss)
            app.initDevice(dev)
            if flatten is not None:
                dev.setFlattenPolicy(*flatten)
                dev.build()
            built = dev.buildInfo()
            sphere = max(range(app.info.numInstances), key=lambda i: len(app.geometry(app.instance(i)[0])[1]) if app.instance(i)[3] < 0 else -1)
            t = dev.instanceTransform(sphere)
            times = []
            for step in range(3):
                t[7] += np.float32(0.05)
                dev.updateInstanceTransform(sphere, t)
                times.append(dev.buildInfo()["buildMilliseconds"])
            print(f"| {name} | {policy} | {built['triangleSlots']} slots | {built['buildMilliseconds']:.1f} | {', '.join(f'{x:.1f}' for x in times)} |")
            dev.close()
            app.close()


def main():
    import tweeker_raytracer_amd as twk
    L = twk._lib
    if "update" in sys.argv[1:]:
        update_times(twk)
        return 0
    half = "half" in sys.argv[1:]
    app = twk.Application(os.path.join(SCENES, "system_rtigo3_cornell_box.txt"), os.path.join(SCENES, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    i = app.info
    camera = lambda frame: twk.camera_frustum(tuple(i.center), i.phi + STEP * frame, i.theta, i.fov, i.distance, RES[0] / RES[1])
    dev = twk.Device(ordinal=0, miss=i.miss)
    dev.enableCascade(True)
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
    h_colour, h_moments, h_geometry, h_layers = allocate(plane), allocate(plane), allocate(plane), allocate(K * plane)
    assert hip.hipMemcpy(h_colour, first.ctypes.data_as(C.c_void_p), C.c_size_t(plane), 1) == 0
    assert hip.hipMemcpy(h_moments, C.c_void_p(dev.momentsDevicePointer()[0]), C.c_size_t(plane), 3) == 0
    assert hip.hipMemcpy(h_geometry, C.c_void_p(dev.geometryDevicePointer()[0]), C.c_size_t(plane), 3) == 0
    assert hip.hipMemcpy(h_layers, C.c_void_p(dev.cascadeDevicePointer()[0]), C.c_size_t(K * plane), 3) == 0
    frame(1)
    # the instances that cover about half of the hit pixels, largest first
    inst = dev.readGeometry()[..., 3].view(np.uint32).reshape(-1)
    counts = np.bincount(inst, minlength=i.numInstances + 1)[1:]
    moved, covered = [], 0
    for k in np.argsort(-counts):
        if covered + counts[k] <= 0.55 * counts.sum():
            moved.append(int(k))
            covered += int(counts[k])
    table = (L.InstanceMotion * i.numInstances)()
    for k in range(i.numInstances):
        table[k].previousFromCurrent[0] = table[k].previousFromCurrent[5] = table[k].previousFromCurrent[10] = 1.0
        table[k].moved = int(k in moved)
    d_table = allocate(C.sizeof(table))
    assert hip.hipMemcpy(d_table, table, C.c_size_t(C.sizeof(table)), 1) == 0
    print(f"C2 {RES[0]}x{RES[1]}, {'RGBA16F' if half else 'RGBA32F'}, two frames of {SPP} spp {STEP} of a turn apart; explicit forms, {CALLS} calls per window, the smallest of 5 "
          f"windows; stream peak {peak:.0f} GB/s (twk_stream_peak_gbps, 1 GiB x 10); library {os.path.basename(L.LIB_PATH)}. Moved: instances {moved}, "
          f"{covered / pixels:.3f} of the pixels ({covered / max(1, counts.sum()):.3f} of the hits).\n")
    current = L.TemporalFrame(dev.outputDevicePointer()[0], dev.momentsDevicePointer()[0], dev.geometryDevicePointer()[0], camera(1))
    history = L.TemporalFrame(h_colour.value, h_moments.value, h_geometry.value, camera(0))
    outs = [allocate(pixels * P), allocate(plane), allocate(plane), allocate(pixels * 4), allocate(K * plane)]
    o = [p.value for p in outs]
    tp = L.Temporal(maxHistory=32, positionTolerance=0.01)
    rp = L.TemporalRectify()
    layers, geometry = dev.cascadeDevicePointer()[0], dev.geometryDevicePointer()[0]
    n = i.numInstances

    def window(call):
        dev.synchronizeStream()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        dev.synchronizeStream()
        return (time.perf_counter() - t0) * 1e6 / CALLS

    def timed_pair(parent, moving):
        for _ in range(10):
            parent()
            moving()
        a, b = [], []
        for _ in range(5):
            a.append(window(parent))
            b.append(window(moving))
        return min(a), min(b)

    def download(pointer, count, dtype):
        out = np.empty(count, dtype)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), pointer, C.c_size_t(out.nbytes), 2) == 0
        return out

    floor = lambda nbytes: nbytes * pixels / (peak * 1e9) * 1e6
    rows = [
        ("twk_temporal_accumulate", 112 + 2 * P, pixels * 4, 2,
         lambda: dev.temporalAccumulate(tp, current, history, shape, o[0], o[1], o[2]),
         lambda: dev.temporalAccumulateMoving(tp, None, current, history, d_table.value, n, shape, o[0], o[1], o[2], None)),
        ("twk_temporal_accumulate_rectified, radius 3 (both launches)", (112 + P) + (84 + 2 * P), pixels * 4, 2,
         lambda: dev.temporalAccumulateRectified(tp, rp, current, history, shape, o[0], o[1], o[2], o[3]),
         lambda: dev.temporalAccumulateMoving(tp, rp, current, history, d_table.value, n, shape, o[0], o[1], o[2], o[3])),
        (f"twk_temporal_accumulate_cascade, {K} layers", 16 + 16 + 48 * K, K * pixels * 4, 4,
         lambda: dev.temporalAccumulateCascade(tp, None, layers, geometry, h_layers.value, h_geometry.value, camera(0), shape, o[4]),
         lambda: dev.temporalAccumulateCascadeMoving(tp, None, layers, geometry, h_layers.value, h_geometry.value, camera(0), None, d_table.value, n, shape, o[4])),
        (f"twk_temporal_accumulate_cascade_trusted, {K} layers", 16 + 16 + 4 + 48 * K, K * pixels * 4, 4,
         lambda: dev.temporalAccumulateCascadeTrusted(tp, None, layers, geometry, h_layers.value, h_geometry.value, camera(0), o[3], shape, o[4]),
         lambda: dev.temporalAccumulateCascadeMoving(tp, None, layers, geometry, h_layers.value, h_geometry.value, camera(0), o[3], d_table.value, n, shape, o[4])),
    ]
    print("| call | parent us | Moving us | Moving - parent us | parent bytes per pixel | parent floor us | Moving floor us (+ 64 bytes per pixel at most) | same bytes out |")
    print("|---|---|---|---|---|---|---|---|")
    for name, nbytes, words, which, parent, moving in rows:
        parent()
        dev.synchronizeStream()
        want = download(outs[which], words, np.uint32)
        moving()
        dev.synchronizeStream()
        same = np.array_equal(download(outs[which], words, np.uint32), want)  # the identity moves nothing: the Moving build must write the parent's bytes
        a, b = timed_pair(parent, moving)
        print(f"| {name} | {a:.1f} | {b:.1f} | {b - a:+.1f} | {nbytes} | {floor(nbytes):.1f} | {floor(nbytes + 64):.1f} | {same} |")
    for p in outs + [h_colour, h_moments, h_geometry, h_layers, d_table]:
        hip.hipFree(p)
    dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
