"""CPU: instance motion in the temporal merges (csrc/temporal_motion_device.h) — twk_instance_motion against its float64 restatement
bit for bit; the host-only forms twk_temporal_moving_host and twk_temporal_cascade_moving_host, the same headers compiled for the
host, against tests/temporal_motion_restate.py bit for bit; that without a table (or with one that says nothing moved) every output
has the bytes of the existing host forms; the refusals; and the same host code under the address and undefined-behaviour sanitizers,
in a stand-alone program. No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from temporal_motion_restate import (RECORD, expect_rectify_moving, instance_motion, motion_table, moved_geometry, moving_frames, moving_layers,
                                     restate_cascade_moving, restate_temporal_moving)
from temporal_restate import F, U32, restate_temporal
from test_temporal_cascade_host import host_merge
from test_temporal_rectify_host import _bits, _camera, _same, host_merge_trusted, host_rectify

SIZES = [(37, 23), (64, 4)]
K = 6


def _table_pointer(table, L):
    return None if table is None else np.ascontiguousarray(table).ctypes.data_as(C.POINTER(L.InstanceMotion))


def host_moving(twk, rectify, cur, mc, g, history, cam, max_history, tolerance, table, num_motion, expect=0, trust_out=None):
    """twk_temporal_moving_host on numpy arrays: (colour, moments, trust) — trust None for the plain merge (rectify None) — or the
    refusal's code when one is expected. rectify: (radius, minTaps, gamma) or None. trust_out: whether a trustOut is passed (None: with
    the rectified merge only)."""
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = cur.shape[:2]
    colour, moments, trust = np.full((height, width, 4), -7, F), np.full((height, width, 4), -7, F), np.full((height, width), -7, F)
    tp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance)
    rp = None if rectify is None else L.TemporalRectify(*rectify)
    hc, hm, hg = (None, None, None) if history is None else history
    give_trust = (rectify is not None) if trust_out is None else trust_out
    rc = L.lib.twk_temporal_moving_host(C.byref(tp), None if rp is None else C.byref(rp), fp(cur), fp(mc), fp(g), fp(hc), fp(hm), fp(hg),
                                        None if history is None else C.byref(_camera(twk, cam)), _table_pointer(table, L), int(num_motion), int(width), int(height),
                                        fp(colour), fp(moments), fp(trust) if give_trust else None)
    assert rc == expect, L.lib.twk_last_error().decode()
    return (colour, moments, trust if rectify is not None else None) if rc == 0 else rc


def host_cascade_moving(twk, layers, g, history, cam, max_history, tolerance, trust, table, num_motion, expect=0):
    L = twk._lib
    fp = lambda a: None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    height, width = g.shape[:2]
    out = np.full(layers.shape, -7, F)
    tp, cp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.Cascade(layers.shape[0], 1.0, 8.0)
    hl, hgeo = (None, None) if history is None else history
    rc = L.lib.twk_temporal_cascade_moving_host(C.byref(tp), C.byref(cp), fp(layers), fp(g), fp(hl), fp(hgeo), None if history is None else C.byref(_camera(twk, cam)), fp(trust),
                                                _table_pointer(table, L), int(num_motion), int(width), int(height), fp(out))
    assert rc == expect, L.lib.twk_last_error().decode()
    return out if rc == 0 else rc


def test_the_new_calls_exist_and_refuse_a_null_handle(twk):
    """Every new symbol is in the binding; the device calls refuse a NULL handle with TWK_ERROR_INVALID_VALUE and their own name,
    before any HIP call (this machine has no GPU to call)."""
    L = twk._lib
    for name in ("twk_instance_motion", "twk_update_instance_transform", "twk_get_instance_transform", "twk_temporal_accumulate_moving", "twk_temporal_accumulate_cascade_moving",
                 "twk_temporal_moving_host", "twk_temporal_cascade_moving_host", "twk_read_temporal_motion", "twk_app_get_temporal_motion"):
        assert name in L.SYMBOLS and getattr(L.lib, name) is not None
    for method in ("updateInstanceTransform", "instanceTransform", "temporalAccumulateMoving", "temporalAccumulateCascadeMoving", "readTemporalMotion"):
        assert callable(getattr(twk.Device, method))
    assert callable(twk.instance_motion) and C.sizeof(L.InstanceMotion) == 64 == RECORD.itemsize and twk.InstanceMotion is L.InstanceMotion
    identity = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    count = C.c_int(0)
    for call, args in (("twk_update_instance_transform", (None, 0, identity)), ("twk_get_instance_transform", (None, 0, identity)),
                       ("twk_temporal_accumulate_moving", (None,) * 6 + (0, 0, 0) + (None,) * 4), ("twk_temporal_accumulate_cascade_moving", (None,) * 10 + (0, 0, 0, None)),
                       ("twk_read_temporal_motion", (None, None, C.c_size_t(0), C.byref(count))), ("twk_app_get_temporal_motion", (None, None, None))):
        assert getattr(L.lib, call)(*args) == L.TWK_ERROR_INVALID_VALUE, call
        assert call in L.lib.twk_last_error().decode(), call
    assert L.lib.twk_abi_version() == 9


def _random_pairs(rng, count):
    """`count` pairs of affine 3 x 4 matrices: translations, rotations, non-uniform scales, shears, mixtures, and bit-equal pairs."""
    def rotation():
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    def matrix(kind):
        a, t = np.eye(3), rng.uniform(-20.0, 20.0, 3)
        if kind in ("rotation", "mixed"):
            a = rotation() @ a
        if kind in ("scale", "mixed"):
            a = a @ np.diag(rng.uniform(0.05, 30.0, 3) * rng.choice([-1.0, 1.0], 3))
        if kind == "mixed":
            a = a + rng.normal(0.0, 0.2, (3, 3))
        return np.concatenate([a, t[:, None]], axis=1).astype(F).reshape(12)

    kinds = ("translation", "rotation", "scale", "mixed", "equal")
    pairs = []
    for i in range(count):
        kind = kinds[i % len(kinds)]
        current = matrix(kind)
        pairs.append((current.copy() if kind == "equal" else matrix(kind), current))
    return pairs


def test_instance_motion_equals_its_restatement_bit_for_bit(twk):
    rng = np.random.default_rng(23)
    pairs = _random_pairs(rng, 250)
    moved = 0
    for previous, current in pairs:
        expect = instance_motion(previous, current)
        assert expect is not None
        got = np.frombuffer(bytes(twk.instance_motion(previous, current)), RECORD)[0]
        assert got.tobytes() == expect.tobytes(), (previous, current, got, expect)
        moved += int(got["moved"])
        if got["moved"]:  # X carries a point of the instance now to where it was: X . current = previous, to rounding
            to4 = lambda m: np.vstack([np.asarray(m, np.float64).reshape(3, 4), [0, 0, 0, 1]])
            assert np.allclose((to4(got["previousFromCurrent"]) @ to4(current))[:3], to4(previous)[:3], rtol=1e-4, atol=1e-4 * np.abs(previous).max())
        else:
            assert got["previousFromCurrent"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and not got["reserved"].any()
    assert moved == 200 and len(pairs) - moved == 50
    # -0.0 against +0.0 is a pair that differs in a word: moved, with X the identity to rounding
    a = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    b = a.copy()
    b[1] = -0.0
    assert twk.instance_motion(a, b).moved == 1 and twk.instance_motion(a, a).moved == 0


def test_instance_motion_refusals(twk):
    L = twk._lib
    identity = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = L.InstanceMotion()
    for args in ((None, fp(identity), C.byref(out)), (fp(identity), None, C.byref(out)), (fp(identity), fp(identity), None)):
        assert L.lib.twk_instance_motion(*args) == L.TWK_ERROR_INVALID_VALUE and "twk_instance_motion" in L.lib.twk_last_error().decode()
    flat = identity.copy()
    flat[10] = 0.0  # a singular current: refused, also when previous is bit-equal to it
    twice = identity.copy()
    twice[4:8] = twice[0:4]
    for previous, current in ((identity, flat), (flat, flat), (identity, twice)):
        with pytest.raises(twk.TwkError) as e:
            twk.instance_motion(previous, current)
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "determinant" in str(e.value)
        assert instance_motion(previous, current) is None
    twk.instance_motion(flat, identity)  # a singular PREVIOUS is no obstacle: only current is inverted
    for bad in (np.nan, np.inf, -np.inf):
        for word in (0, 3, 11):
            broken = identity.copy()
            broken[word] = bad
            for previous, current in ((broken, identity), (identity, broken)):
                with pytest.raises(twk.TwkError):
                    twk.instance_motion(previous, current)
                assert instance_motion(previous, current) is None


def test_the_table_of_the_tests_does_what_it_is_for():
    """Checks the test's inputs, by the restatement alone: with the table more pixels of the translated instance take history than
    without it or the same number, the results differ at many pixels, the NaN record's pixels all pass through, and with numMotion = 3
    instance 4 behaves as unmoved."""
    (cur, mc, g), history, cam, max_history, tolerance, table = moving_frames(37, 23)
    inst = g[..., 3].view(U32)
    assert set(np.unique(inst)) == {0, 1, 2, 3, 4}
    none = restate_temporal(cur, mc, g, history, cam, max_history, tolerance)
    three = restate_temporal_moving(cur, mc, g, history, cam, max_history, tolerance, table[:3])
    four = restate_temporal_moving(cur, mc, g, history, cam, max_history, tolerance, table)
    assert none[2][inst == 3].sum() > 20 and three[2][inst == 3].sum() == 0, "a NaN matrix: no history"
    assert three[2][inst == 2].sum() > 30 and (_bits(three[0]) != _bits(none[0])).any(axis=-1)[inst == 2].sum() > 30, "the translation changes what instance 2 merges"
    assert np.array_equal(_bits(three[0])[inst == 4], _bits(none[0])[inst == 4]) and np.array_equal(_bits(three[0])[inst == 1], _bits(none[0])[inst == 1])
    assert four[2][inst == 4].sum() > 20 and (_bits(four[0]) != _bits(none[0])).any(axis=-1)[inst == 4].sum() > 20, "the rotation changes what instance 4 merges"
    moved = moved_geometry(g, table)
    assert np.array_equal(moved[..., 3].view(U32), inst) and np.array_equal(_bits(moved)[inst <= 1], _bits(g)[inst <= 1])


@pytest.mark.parametrize("num_motion", [3, 4])
@pytest.mark.parametrize("width,height", SIZES)
def test_the_host_forms_equal_the_restatement_bit_for_bit(twk, width, height, num_motion):
    """37x23: partial tiles of the rectified merge's second launch; 64x4: one row of tiles, a picture flatter than the window."""
    (cur, mc, g), history, cam, max_history, tolerance, table = moving_frames(width, height)
    what = f"{width}x{height}, numMotion {num_motion}"
    colour, moments, took = restate_temporal_moving(cur, mc, g, history, cam, max_history, tolerance, table[:num_motion])
    got = host_moving(twk, None, cur, mc, g, history, cam, max_history, tolerance, table, num_motion)
    _same(got[0], colour, what + ", plain colour")
    _same(got[1], moments, what + ", plain moments")
    assert took.sum() > 10 and np.array_equal(_bits(got[0])[~took], _bits(cur)[~took])
    for radius, min_taps in ((1, 4), (3, 8)):
        narrow, colour, moments, trust, merged = expect_rectify_moving(cur, mc, g, history, cam, max_history, tolerance, radius, min_taps, 3.0, table[:num_motion])
        got = host_moving(twk, (radius, min_taps, 3.0), cur, mc, g, history, cam, max_history, tolerance, table, num_motion)
        _same(got[0], narrow, what + f", rectified radius {radius} colour")
        _same(got[1], moments, what + f", rectified radius {radius} moments")
        _same(got[2], trust, what + f", rectified radius {radius} trust")
        assert merged.sum() > 10
    Lc, gl, hist, cam, max_history, tolerance, table = moving_layers(width, height, K)
    expect, took = restate_cascade_moving(Lc, gl, hist, cam, max_history, tolerance, table[:num_motion])
    _same(host_cascade_moving(twk, Lc, gl, hist, cam, max_history, tolerance, None, table, num_motion), expect, what + ", cascade")
    assert took.sum() > 10
    trust = np.random.default_rng(5).uniform(0.0, 1.0, (height, width)).astype(F)
    expect, _ = restate_cascade_moving(Lc, gl, hist, cam, max_history, tolerance, table[:num_motion], trust)
    _same(host_cascade_moving(twk, Lc, gl, hist, cam, max_history, tolerance, trust, table, num_motion), expect, what + ", trusted cascade")


@pytest.mark.parametrize("width,height", SIZES)
def test_without_motion_every_output_has_the_bytes_of_the_existing_host_forms(twk, width, height):
    """motion NULL, numMotion 0, and a table whose every record says moved = 0 (with matrices that would move everything if they
    were read)."""
    (cur, mc, g), history, cam, max_history, tolerance, table = moving_frames(width, height)
    still = table.copy()
    still["moved"] = 0
    existing = host_rectify(twk, cur, mc, g, history, cam, max_history, tolerance, 3, 8, 3.0)
    plain = restate_temporal(cur, mc, g, history, cam, max_history, tolerance)
    Lc, gl, hist, cam_l, mh, tol, _ = moving_layers(width, height, K)
    trust = np.random.default_rng(6).uniform(0.0, 1.0, (height, width)).astype(F)
    layers, trusted = host_merge(twk, Lc, gl, hist, cam_l, mh, tol, K), host_merge_trusted(twk, Lc, gl, hist, cam_l, mh, tol, K, trust)
    for what, tb, n in (("motion NULL", None, 4), ("numMotion 0", table, 0), ("every record unmoved", still, 4)):
        got = host_moving(twk, (3, 8, 3.0), cur, mc, g, history, cam, max_history, tolerance, tb, n)
        for a, b, name in zip(got, existing, ("colour", "moments", "trust")):
            _same(a, b, f"{what}: rectified {name}")
        got = host_moving(twk, None, cur, mc, g, history, cam, max_history, tolerance, tb, n)
        _same(got[0], plain[0], f"{what}: plain colour")
        _same(got[1], plain[1], f"{what}: plain moments")
        _same(host_cascade_moving(twk, Lc, gl, hist, cam_l, mh, tol, None, tb, n), layers, f"{what}: cascade")
        _same(host_cascade_moving(twk, Lc, gl, hist, cam_l, mh, tol, trust, tb, n), trusted, f"{what}: trusted cascade")
    # no history: everything passes through, table or not
    got = host_moving(twk, None, cur, mc, g, None, cam, max_history, tolerance, table, 4)
    _same(got[0], cur, "no history: colour")
    _same(got[1], mc, "no history: moments")


def test_the_host_forms_refuse_what_the_device_forms_refuse(twk):
    L = twk._lib
    bad = L.TWK_ERROR_INVALID_VALUE
    (cur, mc, g), history, cam, max_history, tolerance, table = moving_frames(9, 7)
    assert host_moving(twk, None, cur, mc, g, history, cam, max_history, tolerance, table, -1, expect=bad) == bad and "twk_temporal_moving_host" in L.lib.twk_last_error().decode()
    assert host_moving(twk, None, cur, mc, g, history, cam, max_history, tolerance, table, 3, expect=bad, trust_out=True) == bad, "a trustOut with the plain merge"
    assert host_moving(twk, None, cur, mc, g, history, cam, 0, tolerance, table, 3, expect=bad) == bad
    assert host_moving(twk, (5, 8, 3.0), cur, mc, g, history, cam, max_history, tolerance, table, 3, expect=bad) == bad
    assert host_moving(twk, None, cur, mc, g, (history[0], None, history[2]), cam, max_history, tolerance, table, 3, expect=bad) == bad
    assert host_moving(twk, None, cur, mc, g, history, np.zeros(12, F), max_history, tolerance, table, 3, expect=bad) == bad
    Lc, gl, hist, cam_l, mh, tol, _ = moving_layers(9, 7, K)
    assert host_cascade_moving(twk, Lc, gl, hist, cam_l, mh, tol, None, table, -1, expect=bad) == bad and "twk_temporal_cascade_moving_host" in L.lib.twk_last_error().decode()
    assert host_cascade_moving(twk, Lc, gl, hist, cam_l, 0, tol, None, table, 3, expect=bad) == bad


def test_description_key_of_the_moving_instance(twk):
    from conftest import scene_path
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    scene = open(scene_path("scene_rtigo3_cornell_box.txt")).read()

    def description(text):
        app = twk.Application(system_text=text, scene_text=scene)
        try:
            return app.temporalMotion, app.systemDescription()
        finally:
            app.close()

    off, off_text = description(base)
    assert off == (-1, (0.0, 0.0, 0.0)) and "temporalInstanceStep" not in off_text, "no key by default, nothing written back"
    on, on_text = description(base + "\ntemporalAccumulation 1\ntemporalInstanceStep 6 0.25 0 -0.5\n")
    assert on == (6, (0.25, 0.0, -0.5)) and "temporalInstanceStep 6 0.25 0 -0.5\n" in on_text
    assert description(on_text) == (on, on_text), "what is written back parses to the same"
    got, text = description(base + "\ntemporalInstanceStep -1 0 0 0\n")  # an id the update would refuse drops the line
    assert got == (-1, (0.0, 0.0, 0.0)) and "temporalInstanceStep" not in text
    with pytest.raises(twk.TwkError):  # words that are no numbers are a parse error, as for every numeric key
        description(base + "\ntemporalInstanceStep 2 left 0 0\n")


# ---- the same host code under the sanitizers, in a stand-alone program ----------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("temporal_motion") / "temporal_motion_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    # the flags of the host builds of the kernel headers (no contraction: every expression rounds as written), plus the sanitizers
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"),
           "-o", out, os.path.join(ROOT, "tests", "temporal_motion_host.cpp")]
    subprocess.run(cmd, check=True)
    return out


def test_the_host_forms_run_clean_under_the_sanitizers(sanitized_program, tmp_path):
    """The 37x23 case with numMotion = 3 through the stand-alone program: the plain and the rectified merge, the cascade's merge
    plain and trusted, and twk_instance_motion's body on pairs that include refusals. It exits 0 with nothing on stderr, and what it
    computed has the restatement's bits."""
    width, height, radius, min_taps, gamma = 37, 23, 3, 8, 3.0
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance, table = moving_frames(width, height)
    Lc, _, (Hl, _), _, _, _, _ = moving_layers(width, height, K)  # (the program takes one geometry: the frames' serves the layers too)
    trust = np.random.default_rng(5).uniform(0.0, 1.0, (height, width)).astype(F)
    pairs = _random_pairs(np.random.default_rng(29), 40)
    singular = np.zeros(12, F)
    pairs += [(pairs[0][0], singular), (np.full(12, np.nan, F), pairs[0][1])]
    case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.array([width, height, K, 3, max_history, radius, min_taps, len(pairs)], np.int32).tobytes())
        f.write(np.array([tolerance, gamma, 1.0, 8.0], F).tobytes())
        for a in (cam, cur, mc, g, hc, hm, hg, Lc, Hl, trust):
            f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.ascontiguousarray(table[:3]).tobytes())
        f.write(np.stack([p for p, _ in pairs]).astype(F).tobytes())
        f.write(np.stack([c for _, c in pairs]).astype(F).tobytes())
    # (the leak check stops the process with a tracer of its own, which a sandbox may forbid: off, the address checks are what is asked for)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([sanitized_program, case, result], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    raw = np.fromfile(result, np.uint8)
    n = width * height
    sizes = [4 * n, 4 * n, 4 * n, 4 * n, n, 4 * n * K, 4 * n * K]
    floats = np.frombuffer(raw[: 4 * sum(sizes)].tobytes(), F)
    parts = np.split(floats, np.cumsum(sizes)[:-1])
    rest = raw[4 * sum(sizes):]
    records = np.frombuffer(rest[: 64 * len(pairs)].tobytes(), RECORD)
    refused = np.frombuffer(rest[64 * len(pairs):].tobytes(), np.int32)
    assert refused.shape == (len(pairs),) and refused.tolist() == [0] * 40 + [1, 1]
    for (previous, current), record in zip(pairs[:40], records):
        assert record.tobytes() == instance_motion(previous, current).tobytes()
    colour, moments, _ = restate_temporal_moving(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, table[:3])
    _same(parts[0].reshape(height, width, 4), colour, "plain colour")
    _same(parts[1].reshape(height, width, 4), moments, "plain moments")
    narrow, _, moments, trust_out, _ = expect_rectify_moving(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, radius, min_taps, gamma, table[:3])
    _same(parts[2].reshape(height, width, 4), narrow, "rectified colour")
    _same(parts[3].reshape(height, width, 4), moments, "rectified moments")
    _same(parts[4].reshape(height, width), trust_out, "rectified trust")
    _same(parts[5].reshape(K, height, width, 4), restate_cascade_moving(Lc, g, (Hl, hg), cam, max_history, tolerance, table[:3])[0], "cascade")
    _same(parts[6].reshape(K, height, width, 4), restate_cascade_moving(Lc, g, (Hl, hg), cam, max_history, tolerance, table[:3], trust)[0], "trusted cascade")
