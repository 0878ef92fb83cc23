"""The rule of csrc/light_motion.h (twk_light_moved_host) restated in numpy, statement for statement: double where the header is double,
float32 where it is float, every sum in the header's order. A helper module, not a conftest; tests/test_light_motion_host.py (CPU) and
tests/test_gpu_emitter_motion.py use it.

A light definition is a numpy record of LIGHT (80 bytes, the layout of TwkLightDefinition)."""
import ctypes as C

import numpy as np

F, D = np.float32, np.float64
LIGHT = np.dtype([("type", np.int32), ("position", F, 3), ("vecU", F, 3), ("vecV", F, 3), ("normal", F, 3), ("area", F), ("emission", F, 3), ("unused", F, 3)])
assert LIGHT.itemsize == 80
PARALLELOGRAM = 1


def record(definition):
    """The LIGHT record of a ctypes LightDefinition (or of 80 bytes)."""
    raw = bytes(definition) if not isinstance(definition, (bytes, bytearray)) else bytes(definition)
    return np.frombuffer(raw, LIGHT)[0].copy()


def definition(twk, rec):
    """The ctypes LightDefinition of a LIGHT record."""
    out = twk.LightDefinition()
    C.memmove(C.byref(out), np.asarray(rec, LIGHT).tobytes(), 80)
    return out


def parallelogram(position, vecU, vecV, emission=(10.0, 10.0, 10.0)):
    """A LIGHT record as createLights makes one: normal and area from the float cross product."""
    rec = np.zeros((), LIGHT)
    rec["type"] = PARALLELOGRAM
    rec["position"], rec["vecU"], rec["vecV"], rec["emission"] = F(position), F(vecU), F(vecV), F(emission)
    n, area, normal = cross_area_normal(rec["vecU"], rec["vecV"])
    rec["area"], rec["normal"] = area, normal
    return rec


def cross_area_normal(u, v):
    """createLights' three statements on float32 vectors: n = cross(u, v), area = length(n), normal = n / area (n * (1 / area))."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], F)
    with np.errstate(all="ignore"):
        area = np.sqrt(F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        inverse = F(1.0) / area
        return n, area, np.array([n[0] * inverse, n[1] * inverse, n[2] * inverse], F)


def delta(anchor_transform, transform):
    """D = T_new . inv(T_anchor) in double, 3 x 4, with the header's cofactor inverse and summation order; None: a singular anchor."""
    a = np.asarray(anchor_transform, F).reshape(3, 4).astype(D)
    n = np.asarray(transform, F).reshape(3, 4).astype(D)
    (a00, a01, a02, t0), (a10, a11, a12, t1), (a20, a21, a22, t2) = a
    c00 = a11 * a22 - a12 * a21
    c01 = a12 * a20 - a10 * a22
    c02 = a10 * a21 - a11 * a20
    det = (a00 * c00 + a01 * c01) + a02 * c02
    if not np.isfinite(det) or det == 0.0:
        return None
    r = 1.0 / det
    inv = np.zeros((3, 4), D)
    inv[0, :3] = c00 * r, (a02 * a21 - a01 * a22) * r, (a01 * a12 - a02 * a11) * r
    inv[1, :3] = c01 * r, (a00 * a22 - a02 * a20) * r, (a02 * a10 - a00 * a12) * r
    inv[2, :3] = c02 * r, (a01 * a20 - a00 * a21) * r, (a00 * a11 - a01 * a10) * r
    for k in range(3):
        inv[k, 3] = -((inv[k, 0] * t0 + inv[k, 1] * t1) + inv[k, 2] * t2)
    d = np.zeros((3, 4), D)
    for k in range(3):
        for j in range(3):
            d[k, j] = (n[k, 0] * inv[0, j] + n[k, 1] * inv[1, j]) + n[k, 2] * inv[2, j]
        d[k, 3] = ((n[k, 0] * inv[0, 3] + n[k, 1] * inv[1, 3]) + n[k, 2] * inv[2, 3]) + n[k, 3]
    return d


def light_moved(anchor, anchor_transform, transform):
    """The moved LIGHT record, or None where the header refuses."""
    anchor = np.asarray(anchor, LIGHT)
    at, t = np.asarray(anchor_transform, F).reshape(12), np.asarray(transform, F).reshape(12)
    if int(anchor["type"]) != PARALLELOGRAM or not (np.isfinite(at).all() and np.isfinite(t).all()):
        return None
    with np.errstate(all="ignore"):
        d = delta(at, t)
        if d is None:
            return None
        if at.tobytes() == t.tobytes():
            return anchor.copy()
        out = anchor.copy()
        p, u, v = (anchor[name].astype(D) for name in ("position", "vecU", "vecV"))
        for k in range(3):
            out["position"][k] = F(((d[k, 0] * p[0] + d[k, 1] * p[1]) + d[k, 2] * p[2]) + d[k, 3])
            out["vecU"][k] = F((d[k, 0] * u[0] + d[k, 1] * u[1]) + d[k, 2] * u[2])
            out["vecV"][k] = F((d[k, 0] * v[0] + d[k, 1] * v[1]) + d[k, 2] * v[2])
        _, area, normal = cross_area_normal(out["vecU"], out["vecV"])
        if not np.isfinite(area) or area == 0.0:
            return None
        e00 = d[1, 1] * d[2, 2] - d[1, 2] * d[2, 1]
        e01 = d[1, 2] * d[2, 0] - d[1, 0] * d[2, 2]
        e02 = d[1, 0] * d[2, 1] - d[1, 1] * d[2, 0]
        if (d[0, 0] * e00 + d[0, 1] * e01) + d[0, 2] * e02 < 0.0:
            normal = -normal
        out["area"], out["normal"] = area, normal
        if not all(np.isfinite(out[name]).all() for name in ("position", "vecU", "vecV", "normal")):
            return None
        return out
