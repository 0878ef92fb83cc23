#!/usr/bin/env python3
"""What twk_temporal_accumulate_rectified buys after a light edit, and what it costs without one (C2, GPU box).

C2 at 160x90, an orbit of 8 frames of 4 spp 0.004 of a turn apart through the own-buffer forms, Temporal(maxHistory=32,
positionTolerance=0.1). EDIT: twk_update_light halves the emission before frame 4. For the plain merge, for a twk_temporal_reset at
the edit, and for the rectified merge at gamma in {2, 3, 4} x radius in {2, 3} (minTaps at its default), the error of the merged colour after frames
4, 5 and 7 against 512 spp of the NEW lighting from that frame's camera. The unchanged-lighting cost stands beside each rectified
row: the same orbit WITHOUT the edit, its error after frame 7 against 512 spp of the old lighting, the plain merge's error there, and
the share of hit pixels whose trust was below 1 in that frame. The errors, over the pixels that hit something, with e = (L - Lref) /
(Lref + 0.01) of the luminance: the mean of |e|, and after a slash sqrt(mean(e^2)) — which a handful of fireflies in the history
decides on this scene (the cascade is there for them), so the first is the one to read. Beside the frame-4 errors of a rectified
row: the mean trust over hit pixels in that frame.
usage (GPU box): python tools/temporal_rectify_sweep.py > table.md"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (160, 90)
FRAMES, SPP, STEP, EDIT_AT, REFERENCE_SPP = 8, 4, 0.004, 4, 512
REPORT = (4, 5, 7)


def luminance(c):
    return 0.2126 * c[..., 0].astype(np.float64) + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def main():
    import tweeker_raytracer_amd as twk
    L = twk._lib
    scenes = os.path.join(ROOT, "scenes")
    app = twk.Application(os.path.join(scenes, "system_rtigo3_cornell_box.txt"), os.path.join(scenes, "scene_rtigo3_cornell_box.txt"))
    app.setResolution(*RES)
    i = app.info
    camera = lambda frame: twk.camera_frustum(tuple(i.center), i.phi + STEP * frame, i.theta, i.fov, i.distance, RES[0] / RES[1])
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)

    def light(scale):
        (l,) = app.lights
        for k in range(3):
            l.emission[k] = l.emission[k] * scale
        return l

    dev = twk.Device(ordinal=0, miss=i.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    dev.enableGeometry(True)

    def reference(frame, scale):
        dev.updateLight(0, light(scale))
        dev.updateCamera(0, camera(frame))
        dev.setSampleOffset(1 << 20)
        for it in range(REFERENCE_SPP):
            dev.render(it)
        dev.renderGeometry()
        return luminance(dev.getOutputBufferHost()), dev.readGeometry()[..., 3].view(np.uint32) != 0

    new = {f: reference(f, 0.5) for f in REPORT}
    old = reference(FRAMES - 1, 1.0)

    def error(colour, ref):
        lum, hit = ref
        e = ((luminance(colour) - lum) / (lum + 0.01))[hit]
        return f"{float(np.abs(e).mean()):.4f} / {float(np.sqrt((e ** 2).mean())):.3f}"

    def orbit(mode, rp, edit):
        """mode: 'plain', 'reset' or 'rectified'. Returns ({frame: error against the matching reference}, share of trust < 1 in the last frame)."""
        dev.temporalReset()
        dev.updateLight(0, light(1.0))
        errors, share = {}, None
        for f in range(FRAMES):
            dev.updateCamera(0, camera(f))
            if edit and f == EDIT_AT:
                dev.updateLight(0, light(0.5))
                if mode == "reset":
                    dev.temporalReset()
            dev.setSampleOffset(f * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometry()
            if mode == "rectified":
                dev.temporalAccumulateRectified(tp, rp)
            else:
                dev.temporalAccumulate(tp)
            if edit and f in REPORT:
                errors[f] = error(dev.readTemporal(), new[f])
                if mode == "rectified" and f == EDIT_AT:
                    errors[f] += f" (trust {float(dev.readTemporalTrust()[new[f][1]].mean()):.3f})"
            if not edit and f == FRAMES - 1:
                errors[f] = error(dev.readTemporal(), old)
                if mode == "rectified":
                    share = float((dev.readTemporalTrust()[old[1]] < 1).mean())
        return errors, share

    print(f"C2 {RES[0]}x{RES[1]}, {FRAMES} frames of {SPP} spp {STEP} of a turn apart, maxHistory 32, positionTolerance 0.1; the emission halved before frame {EDIT_AT}; "
          f"references {REFERENCE_SPP} spp. Relative luminance error over hit pixels: mean absolute / RMS.\n")
    print("| merge | after frame 4 | after frame 5 | after frame 7 | no edit: after frame 7 | no edit: share of trust < 1 |")
    print("|---|---|---|---|---|---|")
    for name, mode, rp in [("plain", "plain", None), ("twk_temporal_reset at the edit", "reset", None)] + \
                          [(f"rectified, gamma {g}, radius {r}", "rectified", L.TemporalRectify(radius=r, gamma=float(g))) for g in (2, 3, 4) for r in (2, 3)]:
        with_edit, _ = orbit(mode, rp, True)
        without, share = orbit(mode, rp, False)
        print(f"| {name} | " + " | ".join(with_edit[f] for f in REPORT) + f" | {without[FRAMES - 1]} | " + ("" if share is None else f"{share:.4f}") + " |")
    dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
