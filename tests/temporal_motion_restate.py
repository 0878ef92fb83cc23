"""Instance motion in the temporal merges (csrc/temporal_motion_device.h) restated: twk_instance_motion in float64 scalars in the
written operation order, and the step of a Moving build, g -> g', statement by statement in numpy float32. The merges themselves are
not restated again: a Moving build is the existing merge with g' in place of g in the projection and in the taps' position test, and
g'.w = g.w, so the restatements of temporal_restate, temporal_rectify_restate and temporal_cascade_restate are CALLED with the moved
geometry — where g' is not finite they find the pixel no candidate, which is "no history" as the definition says. No test in here:
tests/test_temporal_motion_host.py (CPU) and tests/test_gpu_temporal_motion.py / tests/test_gpu_instance_update.py use it."""
import numpy as np

import temporal_cascade_restate
import temporal_rectify_restate
import temporal_restate
from temporal_restate import F, U32, _finite3

RECORD = np.dtype([("previousFromCurrent", F, (12,)), ("moved", U32), ("reserved", U32, (3,))])  # TwkInstanceMotion, 64 bytes
assert RECORD.itemsize == 64


def instance_motion(previous, current):
    """twk_instance_motion: one RECORD (a 0-d structured array) from two row-major 3 x 4 float32 matrices, or None where the call
    refuses. Python floats are IEEE doubles; every product and sum below is one rounded operation, in the header's order."""
    p32, c32 = np.ascontiguousarray(previous, F).reshape(12), np.ascontiguousarray(current, F).reshape(12)
    if not (np.isfinite(p32).all() and np.isfinite(c32).all()):
        return None
    a00, a01, a02, t0, a10, a11, a12, t1, a20, a21, a22, t2 = (float(v) for v in c32)
    c00 = a11 * a22 - a12 * a21
    c01 = a12 * a20 - a10 * a22
    c02 = a10 * a21 - a11 * a20
    det = (a00 * c00 + a01 * c01) + a02 * c02
    if not np.isfinite(det) or det == 0.0:
        return None
    out = np.zeros((), RECORD)
    if p32.tobytes() == c32.tobytes():
        out["previousFromCurrent"][[0, 5, 10]] = 1.0
        return out
    r = 1.0 / det
    inv = [[c00 * r, (a02 * a21 - a01 * a22) * r, (a01 * a12 - a02 * a11) * r],
           [c01 * r, (a00 * a22 - a02 * a20) * r, (a02 * a10 - a00 * a12) * r],
           [c02 * r, (a01 * a20 - a00 * a21) * r, (a00 * a11 - a01 * a10) * r]]
    for k in range(3):
        inv[k].append(-((inv[k][0] * t0 + inv[k][1] * t1) + inv[k][2] * t2))
    with np.errstate(over="ignore"):
        for k in range(3):
            p0, p1, p2, p3 = (float(v) for v in p32[4 * k:4 * k + 4])
            for j in range(3):
                out["previousFromCurrent"][4 * k + j] = F((p0 * inv[0][j] + p1 * inv[1][j]) + p2 * inv[2][j])
            out["previousFromCurrent"][4 * k + 3] = F(((p0 * inv[0][3] + p1 * inv[1][3]) + p2 * inv[2][3]) + p3)
    out["moved"] = 1
    return out


def as_table(records):
    """A RECORD array [n] from ctypes InstanceMotion records, RECORD scalars or a RECORD array; None stays None."""
    if records is None:
        return None
    if isinstance(records, np.ndarray) and records.dtype == RECORD:
        return np.ascontiguousarray(records).reshape(-1)
    return np.array([np.frombuffer(bytes(r), RECORD)[0] if not isinstance(r, np.ndarray) else r[()] for r in records], RECORD).reshape(-1)


def moved_geometry(g, table):
    """temporalMove over g [..., 4] float32: g' where the pixel is a hit with finite g.xyz whose instance has a record that says
    `moved`, g (its bits) elsewhere; g'.w = g.w everywhere. g'.k = ((X[k][0] g.x + X[k][1] g.y) + X[k][2] g.z) + X[k][3] in float32."""
    g = np.ascontiguousarray(g, F)
    table = as_table(table)
    if table is None or table.shape[0] == 0:
        return g.copy()
    bits = g[..., 3].view(U32)
    i = bits - U32(1)  # (a miss wraps to 2^32 - 1: beyond every table)
    listed = (bits != 0) & (i < U32(table.shape[0]))
    rec = table[np.where(listed, i, 0).astype(np.int64)]
    moves = listed & _finite3(g) & (rec["moved"] != 0)
    X = rec["previousFromCurrent"]
    out = g.copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            gk = ((X[..., 4 * k] * g[..., 0] + X[..., 4 * k + 1] * g[..., 1]) + X[..., 4 * k + 2] * g[..., 2]) + X[..., 4 * k + 3]
            assert gk.dtype == F
            out[..., k] = np.where(moves, gk, g[..., k])
    return out


def restate_temporal_moving(cur, mc, g, history, cam, max_history, tolerance, table, info=None):
    """twk_temporal_accumulate_moving, rp NULL: temporal_restate.restate_temporal with the moved geometry."""
    return temporal_restate.restate_temporal(cur, mc, moved_geometry(g, table) if history is not None else g, history, cam, max_history, tolerance, info)


def expect_temporal_moving(colour_raw, moments, geometry, history, cam, max_history, tolerance, table):
    """The three outputs of the plain merge as the device writes them: (colourOut in colour_raw's format, historyOut f32, momentsOut f32, took)."""
    colour, merged_moments, took = restate_temporal_moving(colour_raw.astype(F), moments, geometry, history, cam, max_history, tolerance, table)
    with np.errstate(over="ignore"):
        narrow = colour.astype(colour_raw.dtype)
    narrow[~took] = colour_raw[~took]
    return narrow, colour, merged_moments, took


def expect_rectify_moving(colour_raw, moments, geometry, history, cam, max_history, tolerance, radius, min_taps, gamma, table, info=None):
    """twk_temporal_accumulate_moving with rp: temporal_rectify_restate.expect_rectify with the moved geometry (launch 2 reads only the
    bits of g.w, which the move keeps)."""
    g = moved_geometry(geometry, table) if history is not None else geometry
    return temporal_rectify_restate.expect_rectify(colour_raw, moments, g, history, cam, max_history, tolerance, radius, min_taps, gamma, info)


def restate_cascade_moving(layers, g, history, cam, max_history, tolerance, table, trust=None, info=None):
    """twk_temporal_accumulate_cascade_moving: temporal_cascade_restate's merge with the moved geometry. Returns (merged layers, took)."""
    return temporal_cascade_restate.restate_temporal_cascade(layers, moved_geometry(g, table) if history is not None else g, history, cam, max_history, tolerance, info, None, trust)


# ---- frames and tables -------------------------------------------------------------------------------------------------------------
def four_instances(g):
    """The geometry with instance words spanning 1..4: temporal_restate's synthetic wall has instances 1 (x < 0) and 2; the upper half of
    the picture becomes 3 and 4, in the frame and (by the same world height) in the history."""
    g = g.copy()
    bits = g[..., 3].view(U32)
    upper = (bits != 0) & (g[..., 1] > F(0.0))
    g[..., 3] = np.where(upper, bits + U32(2), bits).astype(U32).view(F)
    return g


def motion_table():
    """The table of the tests, for instance words 1..4: record 0 unmoved; record 1 a translation; record 2 a NaN matrix that says
    `moved` (its pixels pass through); record 3 a rotation with a non-uniform scale. The tests pass it with numMotion = 3 — instance
    4 then lies beyond the table and behaves as unmoved, whatever record 3 says — and with numMotion = 4. The motions stay in the
    plane of temporal_restate's wall but for a step of 0.01 - 0.02 off it, a fraction of the tolerance (0.18 at the wall), so that a
    moved pixel finds the wall's history at the place it is carried to."""
    identity = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    shifted = identity.copy()
    shifted[[3, 7, 11]] = (0.13, -0.07, 0.02)
    a = np.radians(4.0)
    turned = np.array([1.02 * np.cos(a), -0.97 * np.sin(a), 0, 0.03, 1.02 * np.sin(a), 0.97 * np.cos(a), 0, -0.02, 0, 0, 1.01, 0.01], F)
    table = np.zeros(4, RECORD)
    table[0] = instance_motion(identity, identity)
    table[1] = instance_motion(identity, shifted)
    table[2]["previousFromCurrent"][:] = np.nan
    table[2]["moved"] = 1
    table[3] = instance_motion(identity, turned)
    assert table[0]["moved"] == 0 and table[1]["moved"] == 1 and table[3]["moved"] == 1
    return table


def moving_frames(width, height, seed=0):
    """temporal_rectify_restate.rectify_frames (every branch of the plain and the rectified merge) on four instances, and the table:
    (current, history, cam, maxHistory, tolerance, table)."""
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance = temporal_rectify_restate.rectify_frames(width, height, seed)
    return (cur, mc, four_instances(g)), (hc, hm, four_instances(hg)), cam, max_history, tolerance, motion_table()


def moving_layers(width, height, K, seed=0):
    """temporal_cascade_restate.synthetic_layers on four instances: (layers, geometry, (history layers, history geometry), cam,
    maxHistory, tolerance, table)."""
    Lc, g, (Hl, hg), cam, max_history, tolerance, _ = temporal_cascade_restate.synthetic_layers(width, height, K, seed)
    return Lc, four_instances(g), (Hl, four_instances(hg)), cam, max_history, tolerance, motion_table()
