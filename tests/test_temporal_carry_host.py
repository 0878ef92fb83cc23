"""CPU: the previous-position plane (csrc/temporal_carry_device.h) — twk_previous_positions_host, the header compiled for the host,
against tests/temporal_carry_restate.py bit for bit on seeded inputs that hold a miss, an unmoved instance, a moved one, a deformed
one, a deformed instance that has also moved, an instance beyond both tables and a previous vertex that is not finite; that a plane
without deformation has temporalMove's bits (tests/temporal_motion_restate.py moved_geometry); the refusals; and the same host code
under the address and undefined-behaviour sanitizers, in a stand-alone program. No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from temporal_carry_restate import CARRY, previous_positions, to_ctypes
from temporal_motion_restate import RECORD, instance_motion, moved_geometry
from temporal_restate import F, U32

SIZES = [(37, 23), (64, 4)]


def _matrix(rng):
    m = np.concatenate([np.eye(3) + 0.3 * rng.normal(size=(3, 3)), rng.uniform(-2.0, 2.0, (3, 1))], axis=1)
    return m.astype(F).reshape(12)


def carry_case(width, height, seed=0):
    """Two geometries (20 vertices / 30 triangles, 9 / 11), five instances — 0 still, 1 moved, 2 deformed, 3 deformed and moved,
    4 beyond both tables (which have four records) — and one pixel per element of a width x height picture."""
    rng = np.random.default_rng(seed + 100 * width + height)
    n = width * height
    vertices, triangles = (20, 9), (30, 11)
    indices = np.concatenate([rng.integers(0, v, 3 * t) for v, t in zip(vertices, triangles)]).astype(U32)
    index_base = (0, 3 * triangles[0])
    positions = np.zeros((sum(vertices), 4), F)
    positions[:, :3] = rng.uniform(-1.0, 1.0, (sum(vertices), 3))
    positions[5, 1] = np.nan  # a previous vertex that is not finite: g' is not, and is written as it is
    position_base = (0, vertices[0])
    instance_geometry = (0, 1, 0, 1, 0)
    previous, current = [_matrix(rng) for _ in range(5)], [_matrix(rng) for _ in range(5)]
    motion, carry = np.zeros(4, RECORD), np.zeros(4, CARRY)
    for i in range(4):
        if i in (0, 2):
            current[i] = previous[i]
        motion[i] = instance_motion(previous[i], current[i])
        assert int(motion[i]["moved"]) == int(i in (1, 3))
        g = instance_geometry[i]
        carry[i] = (previous[i], int(i in (2, 3)), position_base[g], index_base[g], 0)
    instance = rng.integers(-1, 5, n).astype(np.int32)
    primitive = np.array([rng.integers(0, triangles[instance_geometry[i]]) if i >= 0 else -1 for i in instance], np.int32)
    beta = rng.uniform(0.0, 1.0, n)
    gamma = rng.uniform(0.0, 1.0, n) * (1.0 - beta)
    hits = np.stack([rng.uniform(0.5, 4.0, n), beta, gamma], axis=1).astype(F)
    geometry = np.zeros((n, 4), F)
    geometry[:, :3] = rng.uniform(-3.0, 3.0, (n, 3))
    geometry[:, 3] = (instance + 1).astype(U32).view(F)
    geometry[instance < 0] = 0
    return hits, instance, primitive, geometry, indices, positions, motion, carry


def _host(twk, case, motion=True, carry=True):
    L = twk._lib
    hits, instance, primitive, geometry, indices, positions, m, c = case
    return twk.previous_positions_host(hits, instance, primitive, geometry, indices, positions, to_ctypes(m, L.InstanceMotion) if motion else None,
                                       to_ctypes(c, L.InstanceCarry) if carry else None)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_host_form_equals_the_restatement(twk, size):
    case = carry_case(*size)
    hits, instance, primitive, geometry, indices, positions, motion, carry = case
    got = _host(twk, case)
    want = previous_positions(*case)
    assert np.array_equal(got.view(U32), want.view(U32))
    # what the case holds
    assert not got[instance < 0].any(), "a miss is zero words"
    assert np.array_equal(got[:, 3].view(U32), geometry[:, 3].view(U32)), "the instance word is the geometry AOV's"
    same = np.all(got[:, :3].view(U32) == geometry[:, :3].view(U32), axis=1)
    assert same[(instance == 0) | (instance == 4)].all(), "a still instance, and one beyond the tables: g' = g, its bits"
    for i in (1, 2, 3):
        assert not same[instance == i].any(), f"instance {i}: g' is elsewhere"
    assert np.isnan(got[:, :3]).any() and not np.isnan(got[instance < 2]).any(), "the previous vertex that is not finite shows, on deformed instances only"
    # the deformed instance that has also moved takes the previous vertices through Mp, whatever its motion record says
    still = motion.copy()
    still["moved"][3] = 0
    other = twk.previous_positions_host(hits, instance, primitive, geometry, indices, positions, to_ctypes(still, twk._lib.InstanceMotion), to_ctypes(carry, twk._lib.InstanceCarry))
    assert np.array_equal(other.view(U32), got.view(U32))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_without_deformation_the_plane_is_the_moved_geometry(twk, size):
    """No carry table, and one that says nothing is deformed: g' = temporalMove's, the bits of temporal_motion_restate.moved_geometry;
    without either table g' = g."""
    case = carry_case(*size)
    hits, instance, primitive, geometry, indices, positions, motion, carry = case
    want = moved_geometry(geometry, motion)
    assert np.array_equal(_host(twk, case, carry=False).view(U32), want.view(U32))
    none = carry.copy()
    none["deformed"] = 0
    got = twk.previous_positions_host(hits, instance, primitive, geometry, [], [], to_ctypes(motion, twk._lib.InstanceMotion), to_ctypes(none, twk._lib.InstanceCarry))
    assert np.array_equal(got.view(U32), want.view(U32))
    assert np.array_equal(_host(twk, case, motion=False, carry=False).view(U32), geometry.view(U32))


def test_refusals(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE
    case = carry_case(8, 4)
    hits, instance, primitive, geometry, indices, positions, motion, carry = case
    m, c = to_ctypes(motion, L.InstanceMotion), to_ctypes(carry, L.InstanceCarry)

    def refused(f, *words):
        with pytest.raises(twk.TwkError) as e:
            f()
        assert e.value.code == VALUE and "twk_previous_positions_host" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    deformed = np.nonzero(instance >= 2)[0]
    deformed = deformed[instance[deformed] <= 3]
    assert deformed.size > 0
    refused(lambda: twk.previous_positions_host(hits, instance, primitive, geometry, indices[:3], positions, m, c), "numIndices")
    refused(lambda: twk.previous_positions_host(hits, instance, primitive, geometry, indices, positions[:1], m, c), "numPositions")
    bad = primitive.copy()
    bad[deformed[0]] = -1
    refused(lambda: twk.previous_positions_host(hits, instance, bad, geometry, indices, positions, m, c), f"pixel {deformed[0]}")
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    out = np.zeros((hits.shape[0], 4), F)
    args = lambda: [hits.ctypes.data_as(fp), instance.ctypes.data_as(ip), primitive.ctypes.data_as(ip), geometry.ctypes.data_as(fp), C.c_size_t(hits.shape[0]),
                    indices.ctypes.data_as(C.POINTER(C.c_uint)), C.c_size_t(indices.size), positions.ctypes.data_as(fp), C.c_size_t(positions.shape[0]), m, len(m), c, len(c),
                    out.ctypes.data_as(fp)]
    assert L.lib.twk_previous_positions_host(*args()) == L.TWK_SUCCESS
    for k, word in ((0, "NULL"), (1, "NULL"), (2, "NULL"), (3, "NULL"), (13, "NULL"), (5, "count"), (7, "count"), (9, "count"), (11, "count")):
        a = args()
        a[k] = None
        assert L.lib.twk_previous_positions_host(*a) == VALUE and word in L.lib.twk_last_error().decode(), (k, L.lib.twk_last_error().decode())
    for k, value in ((4, C.c_size_t(0)), (10, -1), (12, -2)):
        a = args()
        a[k] = value
        assert L.lib.twk_previous_positions_host(*a) == VALUE, k


def test_the_host_form_runs_clean_under_the_sanitizers(twk, tmp_path):
    """The 37 x 23 case through the stand-alone program (tests/temporal_carry_host.cpp): it exits 0 with nothing on stderr, and what it
    computed has the restatement's bits."""
    out = str(tmp_path / "temporal_carry_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"),
                    "-o", out, os.path.join(ROOT, "tests", "temporal_carry_host.cpp")], check=True)
    case_values = carry_case(37, 23)
    hits, instance, primitive, geometry, indices, positions, motion, carry = case_values
    case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.array([hits.shape[0], indices.size, positions.shape[0], motion.shape[0], carry.shape[0]], np.int32).tobytes())
        for a in (hits, instance, primitive, geometry, indices, positions, motion, carry):
            f.write(np.ascontiguousarray(a).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([out, case, result], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    got = np.fromfile(result, F).reshape(-1, 4)
    assert np.array_equal(got.view(U32), previous_positions(*case_values).view(U32))


# ---- the Carried builds of the merges: the host forms against the restatement -----------------------------------------------------
from temporal_carry_restate import carried_geometry, expect_rectify_carried, restate_cascade_carried, restate_temporal_carried, seeded_plane  # noqa: E402
from temporal_motion_restate import moving_frames, moving_layers  # noqa: E402
from test_temporal_motion_host import host_cascade_moving, host_moving  # noqa: E402
from test_temporal_rectify_host import _camera, _same  # noqa: E402

RECTIFY = (3, 8, 3.0)
K = 6


def host_carried(twk, rectify, cur, mc, g, history, cam, max_history, tolerance, plane, expect=0, trust_out=None):
    """twk_temporal_carried_host on numpy arrays: (colour, moments, trust) — trust None for the plain merge — or the refusal's code."""
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = cur.shape[:2]
    colour, moments, trust = np.full((height, width, 4), -7, F), np.full((height, width, 4), -7, F), np.full((height, width), -7, F)
    tp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance)
    rp = None if rectify is None else L.TemporalRectify(*rectify)
    hc, hm, hg = (None, None, None) if history is None else history
    give_trust = (rectify is not None) if trust_out is None else trust_out
    rc = L.lib.twk_temporal_carried_host(C.byref(tp), None if rp is None else C.byref(rp), fp(cur), fp(mc), fp(g), fp(hc), fp(hm), fp(hg),
                                         None if history is None else C.byref(_camera(twk, cam)), fp(plane), int(width), int(height), fp(colour), fp(moments),
                                         fp(trust) if give_trust else None)
    assert rc == expect, L.lib.twk_last_error().decode()
    return (colour, moments, trust if rectify is not None else None) if rc == 0 else rc


def host_cascade_carried(twk, layers, g, history, cam, max_history, tolerance, trust, plane, expect=0):
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = g.shape[:2]
    out = np.full(layers.shape, -7, F)
    tp, cp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.Cascade(layers.shape[0], 1.0, 8.0)
    hl, hgeo = (None, None) if history is None else history
    rc = L.lib.twk_temporal_cascade_carried_host(C.byref(tp), C.byref(cp), fp(layers), fp(g), fp(hl), fp(hgeo), None if history is None else C.byref(_camera(twk, cam)), fp(trust),
                                                 fp(plane), int(width), int(height), fp(out))
    assert rc == expect, L.lib.twk_last_error().decode()
    return out if rc == 0 else rc


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_carried_host_merges_equal_the_restatement(twk, size):
    """The plain and the rectified merge and the cascade's merge, plain and trusted, on a seeded plane with a deformation, rigid motion,
    w mismatches, elements that are not finite and misses; with the identity plane the bytes of the existing host forms; with the
    rigid-only plane the bytes of the *_moving host forms with the table."""
    width, height = size
    (cur, mc, g), history, cam, max_history, tolerance, table = moving_frames(width, height)
    plane = seeded_plane(g, table)
    word = g[..., 3].view(U32)
    took = {}
    expect = restate_temporal_carried(cur, mc, g, history, cam, max_history, tolerance, plane, took)
    colour, moments, _ = host_carried(twk, None, cur, mc, g, history, cam, max_history, tolerance, plane)
    _same(colour, expect[0], "plain: colour")
    _same(moments, expect[1], "plain: moments")
    carried = carried_geometry(g, plane)
    dropped = (word != 0) & (carried[..., 3].view(U32) == 0)
    assert dropped.sum() > 10 and not expect[2][dropped].any(), "a w mismatch, a plane element that is not finite, a plane miss: no history"
    assert expect[2][word == 1].sum() > 10, "the deformed instance takes history through the plane"
    r_narrow, _, r_moments, r_trust, r_merged = expect_rectify_carried(cur, mc, g, history, cam, max_history, tolerance, *RECTIFY, plane)
    got = host_carried(twk, RECTIFY, cur, mc, g, history, cam, max_history, tolerance, plane)
    assert r_merged.sum() > 10
    _same(got[0], r_narrow, "rectified: colour")
    _same(got[1], r_moments, "rectified: moments")
    _same(got[2], r_trust, "rectified: trust")
    # the identity plane (every element has the bits of g): the existing host forms; no plane: the same
    for rectify in (None, RECTIFY):
        want = host_moving(twk, rectify, cur, mc, g, history, cam, max_history, tolerance, None, 0)
        for given in (g, None):
            got = host_carried(twk, rectify, cur, mc, g, history, cam, max_history, tolerance, given)
            for a, b, what in zip(got, want, ("colour", "moments", "trust")):
                if a is not None:
                    _same(a, b, f"identity plane, {what}")
        # the rigid-only plane: the moving host form with the table
        rigid = moved_geometry(g, table)
        want = host_moving(twk, rectify, cur, mc, g, history, cam, max_history, tolerance, table, len(table))
        got = host_carried(twk, rectify, cur, mc, g, history, cam, max_history, tolerance, rigid)
        for a, b, what in zip(got, want, ("colour", "moments", "trust")):
            if a is not None:
                _same(a, b, f"rigid-only plane, {what}")
    # without a history every pixel passes through, whatever the plane says
    got = host_carried(twk, None, cur, mc, g, None, None, max_history, tolerance, plane)
    _same(got[0], cur, "no history: colour")
    # the cascade's layers
    Lc, gl, (Hl, hg), cam, max_history, tolerance, table = moving_layers(width, height, K)
    plane = seeded_plane(gl, table)
    trust = np.random.default_rng(5).uniform(0.0, 1.0, (height, width)).astype(F)
    for t in (None, trust):
        want, _ = restate_cascade_carried(Lc, gl, (Hl, hg), cam, max_history, tolerance, plane, t)
        _same(host_cascade_carried(twk, Lc, gl, (Hl, hg), cam, max_history, tolerance, t, plane), want, "cascade" + (" trusted" if t is not None else ""))
        _same(host_cascade_carried(twk, Lc, gl, (Hl, hg), cam, max_history, tolerance, t, gl), host_cascade_moving(twk, Lc, gl, (Hl, hg), cam, max_history, tolerance, t, None, 0), "cascade, identity plane")
        _same(host_cascade_carried(twk, Lc, gl, (Hl, hg), cam, max_history, tolerance, t, moved_geometry(gl, table)),
              host_cascade_moving(twk, Lc, gl, (Hl, hg), cam, max_history, tolerance, t, table, len(table)), "cascade, rigid-only plane")


def test_the_carried_host_forms_refuse_what_the_device_forms_refuse(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE
    (cur, mc, g), history, cam, max_history, tolerance, table = moving_frames(8, 4)
    assert host_carried(twk, None, cur, mc, g, history, cam, max_history, tolerance, g, expect=VALUE, trust_out=True) == VALUE  # a trustOut without rp
    assert "twk_temporal_carried_host" in L.lib.twk_last_error().decode() and "trustOut" in L.lib.twk_last_error().decode()
    assert host_carried(twk, None, cur, mc, g, (history[0], None, history[2]), cam, max_history, tolerance, g, expect=VALUE) == VALUE
    assert host_carried(twk, None, cur, mc, g, history, cam, 0, tolerance, g, expect=VALUE) == VALUE      # maxHistory < 1
    assert host_carried(twk, None, cur, mc, g, history, cam, max_history, -1.0, g, expect=VALUE) == VALUE   # tolerance < 0
    assert host_carried(twk, (9, 8, 3.0), cur, mc, g, history, cam, max_history, tolerance, g, expect=VALUE) == VALUE  # radius
    assert host_carried(twk, None, cur, None, g, history, cam, max_history, tolerance, g, expect=VALUE) == VALUE
    Lc, gl, (Hl, hg), cam, max_history, tolerance, table = moving_layers(8, 4, K)
    assert host_cascade_carried(twk, Lc, gl, (Hl, None), cam, max_history, tolerance, None, gl, expect=VALUE) == VALUE
    assert "twk_temporal_cascade_carried_host" in L.lib.twk_last_error().decode()
    assert host_cascade_carried(twk, Lc, gl, (Hl, hg), cam, 0, tolerance, None, gl, expect=VALUE) == VALUE  # maxHistory < 1
    # the device forms refuse a NULL handle before any HIP call, under their own names
    for call, args in (("twk_temporal_accumulate_carried", (None,) * 6 + (0, 0) + (None,) * 4), ("twk_temporal_accumulate_cascade_carried", (None,) * 10 + (0, 0, None))):
        assert getattr(L.lib, call)(*args) == VALUE and call in L.lib.twk_last_error().decode(), call
    for method in ("temporalAccumulateCarried", "temporalAccumulateCascadeCarried", "updateGeometryVertices", "renderGeometryMotion", "readPreviousPositions", "previousPositionsDevicePointer"):
        assert callable(getattr(twk.Device, method))
    assert L.lib.twk_abi_version() == 9


def test_the_carried_host_merges_run_clean_under_the_sanitizers(twk, tmp_path):
    """The 37 x 23 case with the seeded plane through a stand-alone program (tests/temporal_carry_merge_host.cpp): the Carried builds of
    the plain and the rectified merge and of the cascade's merge, plain and trusted — the code twk_temporal_carried_host and
    twk_temporal_cascade_carried_host run — under the address and undefined-behaviour sanitizers. It exits 0 with nothing on stderr,
    and what it computed has the restatement's bits. (As in tests/test_temporal_motion_host.py the frames' geometry serves the layers
    too.) Nothing is loaded into Python under a sanitizer."""
    width, height, radius, min_taps, gamma = 37, 23, 3, 8, 3.0
    out = str(tmp_path / "temporal_carry_merge_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"),
                    "-o", out, os.path.join(ROOT, "tests", "temporal_carry_merge_host.cpp")], check=True)
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance, table = moving_frames(width, height)
    Lc, _, (Hl, _), _, _, _, _ = moving_layers(width, height, K)
    plane = seeded_plane(g, table)
    trust = np.random.default_rng(5).uniform(0.0, 1.0, (height, width)).astype(F)
    case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.array([width, height, K, max_history, radius, min_taps], np.int32).tobytes())
        f.write(np.array([tolerance, gamma, 1.0, 8.0], F).tobytes())
        for a in (cam, cur, mc, g, hc, hm, hg, Lc, Hl, trust, plane):
            f.write(np.ascontiguousarray(a, F).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([out, case, result], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    n = width * height
    sizes = [4 * n, 4 * n, 4 * n, 4 * n, n, 4 * n * K, 4 * n * K]
    floats = np.fromfile(result, F)
    assert floats.size == sum(sizes)
    p_colour, p_moments, r_colour, r_moments, r_trust, layers, trusted = np.split(floats, np.cumsum(sizes)[:-1])
    expect = restate_temporal_carried(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, plane)
    _same(p_colour.reshape(height, width, 4), expect[0], "plain colour")
    _same(p_moments.reshape(height, width, 4), expect[1], "plain moments")
    assert expect[2].sum() > 10
    narrow, _, moments, e_trust, merged = expect_rectify_carried(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, radius, min_taps, gamma, plane)
    _same(r_colour.reshape(height, width, 4), narrow, "rectified colour")
    _same(r_moments.reshape(height, width, 4), moments, "rectified moments")
    _same(r_trust.reshape(height, width), e_trust, "rectified trust")
    assert merged.sum() > 10
    want, took = restate_cascade_carried(Lc, g, (Hl, hg), cam, max_history, tolerance, plane)
    _same(layers.reshape(Lc.shape), want, "cascade")
    assert took.sum() > 10
    _same(trusted.reshape(Lc.shape), restate_cascade_carried(Lc, g, (Hl, hg), cam, max_history, tolerance, plane, trust)[0], "trusted cascade")
