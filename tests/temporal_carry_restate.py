"""csrc/temporal_carry_device.h restated in numpy, statement for statement: the previous-position plane of
twk_render_geometry_motion / twk_previous_positions_host. What tests/test_temporal_carry_host.py and tests/test_gpu_temporal_carry.py
share. A helper module, not a conftest. Every float32 operation below is one rounded operation, in the header's order."""
import numpy as np

from temporal_motion_restate import RECORD, as_table
from temporal_restate import F, U32

CARRY = np.dtype([("previousObjectToWorld", F, (12,)), ("deformed", U32), ("positionBase", U32), ("indexBase", U32), ("reserved", U32)])  # TwkInstanceCarry
assert CARRY.itemsize == 64


def as_carry(records):
    """A CARRY array [n] from ctypes InstanceCarry records or a CARRY array; None stays None."""
    if records is None:
        return None
    if isinstance(records, np.ndarray) and records.dtype == CARRY:
        return np.ascontiguousarray(records).reshape(-1)
    return np.array([np.frombuffer(bytes(r), CARRY)[0] for r in records], CARRY).reshape(-1)


def to_ctypes(array, kind):
    """A ctypes array of `kind` (L.InstanceMotion / L.InstanceCarry) with the bytes of a RECORD / CARRY array."""
    return (kind * array.shape[0]).from_buffer_copy(np.ascontiguousarray(array).tobytes())


def _affine(M, x, y, z, k):
    out = ((M[..., 4 * k] * x + M[..., 4 * k + 1] * y) + M[..., 4 * k + 2] * z) + M[..., 4 * k + 3]
    assert out.dtype == F
    return out


def previous_positions(hits, instance, primitive, geometry, indices, positions, motion, carry):
    """The plane [n, 4] float32. hits [n, 3] (t, beta, gamma); instance, primitive [n] int32 (instance < 0: a miss); geometry [n, 4]
    the geometry AOV; indices uint32; positions [m, 4]; motion: RECORD table or None; carry: CARRY table or None."""
    hits = np.ascontiguousarray(hits, F).reshape(-1, 3)
    instance = np.ascontiguousarray(instance, np.int32).reshape(-1)
    primitive = np.ascontiguousarray(primitive, np.int32).reshape(-1)
    g = np.ascontiguousarray(geometry, F).reshape(-1, 4)
    indices = np.ascontiguousarray(indices, U32).reshape(-1)
    positions = np.ascontiguousarray(positions, F).reshape(-1, 4)
    motion, carry = as_table(motion), as_carry(carry)
    n = hits.shape[0]
    hit = instance >= 0
    out = np.zeros((n, 4), F)
    out[hit] = g[hit]  # g' = g (its bits), and g.w in every case
    with np.errstate(all="ignore"):
        # temporalMove: the instance word is g.w's, as the function reads it
        if motion is not None and motion.shape[0] > 0:
            i = g[:, 3].view(U32) - U32(1)
            listed = hit & (i < U32(motion.shape[0]))
            rec = motion[np.where(listed, i, 0).astype(np.int64)]
            moves = listed & (rec["moved"] != 0)
            X = rec["previousFromCurrent"]
            for k in range(3):
                out[:, k] = np.where(moves, _affine(X, g[:, 0], g[:, 1], g[:, 2], k), out[:, k])
        # a deformed geometry: the barycentrics on the previous vertices, through Mp
        if carry is not None and carry.shape[0] > 0:
            listed = hit & (instance < carry.shape[0])
            rec = carry[np.where(listed, instance, 0).astype(np.int64)]
            deformed = listed & (rec["deformed"] != 0)
            q = np.where(deformed, primitive, 0).astype(np.int64)
            first = np.where(deformed, rec["indexBase"].astype(np.int64) + 3 * q, 0)
            base = np.where(deformed, rec["positionBase"].astype(np.int64), 0)
            have = indices.size > 0 and positions.shape[0] > 0
            if have and deformed.any():
                v = [positions[np.where(deformed, base + indices[np.minimum(first + j, indices.size - 1)].astype(np.int64), 0)] for j in range(3)]
                beta, gamma = hits[:, 1], hits[:, 2]
                a = (F(1.0) - beta) - gamma
                o = [(a * v[0][:, k] + beta * v[1][:, k]) + gamma * v[2][:, k] for k in range(3)]
                assert all(c.dtype == F for c in o)
                Mp = rec["previousObjectToWorld"]
                for k in range(3):
                    out[:, k] = np.where(deformed, _affine(Mp, o[0], o[1], o[2], k), out[:, k])
    out[~hit] = 0
    return out



# ---- the Carried builds of the merges: temporalCarry composed with the existing restatements --------------------------------------
import temporal_cascade_restate  # noqa: E402
import temporal_motion_restate  # noqa: E402
import temporal_rectify_restate  # noqa: E402
import temporal_restate  # noqa: E402
from temporal_restate import _finite3  # noqa: E402


def carried_geometry(g, plane):
    """temporalCarry over g, plane [..., 4] float32, as the geometry the existing restatements gather with: where the pixel passes the
    candidate's test on g (a hit, g.xyz finite) the plane's element if its instance word has g's bits and its xyz is finite, else a
    miss (zero words: no history); g (its bits) where the pixel is no candidate anyway. Every other term of the candidate test is the
    restatements' own."""
    g, plane = np.ascontiguousarray(g, F), np.ascontiguousarray(plane, F)
    candidate = (g[..., 3].view(U32) != 0) & _finite3(g)
    ok = candidate & (plane[..., 3].view(U32) == g[..., 3].view(U32)) & _finite3(plane)
    out = g.copy()
    out[candidate & ~ok] = 0
    out[ok] = plane[ok]
    return out


def restate_temporal_carried(cur, mc, g, history, cam, max_history, tolerance, plane, info=None):
    """twk_temporal_accumulate_carried, rp NULL: temporal_restate.restate_temporal with the carried geometry."""
    return temporal_restate.restate_temporal(cur, mc, carried_geometry(g, plane) if history is not None else g, history, cam, max_history, tolerance, info)


def expect_temporal_carried(colour_raw, moments, geometry, history, cam, max_history, tolerance, plane):
    """The plain merge's three outputs as the device writes them: temporal_motion_restate.expect_temporal_moving's, by way of a table
    that moves nothing, on the carried geometry."""
    g = carried_geometry(geometry, plane) if history is not None else geometry
    return temporal_motion_restate.expect_temporal_moving(colour_raw, moments, g, history, cam, max_history, tolerance, None)


def expect_rectify_carried(colour_raw, moments, geometry, history, cam, max_history, tolerance, radius, min_taps, gamma, plane, info=None):
    """twk_temporal_accumulate_carried with rp: temporal_rectify_restate.expect_rectify with the carried geometry (launch 2 keys a pixel
    by its instance word only where it took history, and there the plane's word is g's)."""
    g = carried_geometry(geometry, plane) if history is not None else geometry
    return temporal_rectify_restate.expect_rectify(colour_raw, moments, g, history, cam, max_history, tolerance, radius, min_taps, gamma, info)


def restate_cascade_carried(layers, g, history, cam, max_history, tolerance, plane, trust=None, info=None):
    """twk_temporal_accumulate_cascade_carried: temporal_cascade_restate's merge with the carried geometry. Returns (merged layers, took)."""
    return temporal_cascade_restate.restate_temporal_cascade(layers, carried_geometry(g, plane) if history is not None else g, history, cam, max_history, tolerance, info, None, trust)


def seeded_plane(g, table, seed=0):
    """A plane for the frames of temporal_motion_restate.moving_frames / moving_layers: the rigid motion of `table` everywhere, a seeded
    displacement of up to 0.05 on the pixels of instance word 1 (a deformation), and — in the picture's lower right part — elements whose instance word names
    another instance, elements that are not finite, and elements with a zero word on a hit."""
    rng = np.random.default_rng(seed + 17)
    plane = temporal_motion_restate.moved_geometry(g, table)
    word = g[..., 3].view(U32)
    bend = rng.uniform(-0.05, 0.05, g.shape[:-1] + (3,)).astype(F)
    plane[..., :3] = np.where((word == 1)[..., None], plane[..., :3] + bend, plane[..., :3])
    pick = rng.uniform(size=word.shape)
    hit = word != 0
    w = plane[..., 3].view(U32)
    w[hit & (pick < 0.05)] += U32(1)          # a w mismatch
    w[hit & (pick > 0.97)] = 0                # the plane says miss where the frame hits
    plane[hit & (pick > 0.05) & (pick < 0.09), 1] = np.nan
    plane[hit & (pick > 0.09) & (pick < 0.11), 2] = np.inf
    return plane
