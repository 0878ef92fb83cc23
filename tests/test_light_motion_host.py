"""CPU: the rule that moves a light with its emitter (csrc/light_motion.h, twk_light_moved_host) against its numpy restatement
(tests/light_motion_restate.py) and a float64 numpy.linalg computation, its refusals, the same code under the sanitizers in a
stand-alone program, and the moved-light cases of tests/emitter_motion_cases.py through the ORACLE: what direct_light's statistic does
with the right light and with each slip is known here, on a CPU, before a GPU is touched (tests/test_gpu_emitter_direct_light.py runs
the same cases on the HIP path; device and oracle agree bit for bit).

Measured on the oracle (the rows this file prints; profiles/r33_emitter_motion.md holds them):
  reshape, right light            R 0.954 / 0.936 / 2.136 (light / sum / off), accepted on every image
  mirror, right light             R 1.516 / 1.458 / 0.977, accepted on every image
  area x 1.02 control             rejected on every image, R 6.2 .. 657
  unmoved rectangle as reference  rejected on every image, R >= 722
  stale area (reshape)            rejected on "light" and "sum", R 2 512 and 2 660; "off" reads no area
  un-negated normal (mirror)      "light" is black (bias -1); rejected on "light" and "sum" (bias -0.996); "off" reads no normal"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import direct_light as D
import emitter_motion_cases as E
import light_motion_restate as R
from conftest import ROOT

F = np.float32


# ---- seeded transform pairs ---------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _transform(rng, kind):
    """Row-major 3 x 4 float32 [12]: a rotation, with unequal scales, a shear or a mirror by `kind`, and a translation up to 1e4."""
    m = _rotation(rng)
    if kind in ("scale", "shear", "mirror"):
        m = m @ np.diag(np.exp(rng.uniform(-1.5, 1.5, 3)))
    if kind == "shear":
        s = np.eye(3)
        s[0, 1], s[0, 2], s[1, 2] = rng.uniform(-1.0, 1.0, 3)
        m = m @ s
    if kind == "mirror":
        m = m @ np.diag([1.0, -1.0, 1.0]) if rng.integers(2) else np.diag([-1.0, 1.0, 1.0]) @ m
    t = rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(-1.0, 4.0)
    return np.concatenate([m, t.reshape(3, 1)], axis=1).astype(F).reshape(12)


KINDS = ("rotation", "scale", "shear", "mirror")


def seeded_pairs(count=1000, seed=33):
    """[(anchor LIGHT record, anchor transform, transform, kinds)]: each of the two transforms of a pair is of a kind of its own."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        light = R.parallelogram(rng.uniform(-3.0, 3.0, 3), rng.uniform(-2.0, 2.0, 3), rng.uniform(-2.0, 2.0, 3), rng.uniform(0.5, 20.0, 3))
        light["unused"] = rng.uniform(-1.0, 1.0, 3)  # copied, whatever it holds
        kinds = (KINDS[k % 4], KINDS[(k // 4) % 4])
        out.append((light, _transform(rng, kinds[0]), _transform(rng, kinds[1]), kinds))
    return out


PAIRS = seeded_pairs()


def moved_host(twk, light, anchor_transform, transform):
    return R.record(twk.light_moved_host(R.definition(twk, light), anchor_transform, transform))


def test_host_form_equals_the_restatement_bit_for_bit(twk):
    mirrors = 0
    for light, a, t, kinds in PAIRS:
        got, want = moved_host(twk, light, a, t), R.light_moved(light, a, t)
        assert want is not None and got.tobytes() == want.tobytes(), (kinds, got, want)
        d = R.delta(a, t)
        mirrors += np.linalg.det(d[:, :3]) < 0.0
    assert 300 < mirrors < 700, "mirrors on either side of the pair: about half of the pairs flip the handedness"


def test_the_anchor_transform_returns_the_anchor(twk):
    for light, a, _, _ in PAIRS[:50]:
        light = light.copy()
        light["area"], light["normal"] = 7.0, (0.5, 0.25, -3.0)  # not what the rule would derive: the 80 bytes come back as they are
        assert moved_host(twk, light, a, a.copy()).tobytes() == light.tobytes()
    # ... its own BITS: -0.0 for 0.0 in the translation is another transform, and the rule derives
    light, a = PAIRS[0][0], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    b = a.copy()
    b[3] = -0.0
    got = moved_host(twk, light, a, b)
    assert got.tobytes() == R.light_moved(light, a, b).tobytes() and got["position"].tolist() == light["position"].tolist()


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)


def test_moved_vectors_lie_within_one_ulp_of_float64_linalg(twk):
    """position, vecU, vecV against numpy.linalg in float64. The rule's D differs from linalg's by the roundings of a double 3 x 4
    inverse and product, relative 1e-15 times the condition of the anchor matrix (at most e^3 here) and, in the position, times the
    cancellation of translations up to 1e4 against each other: far below the half ulp of the one rounding to float32, so 1 ulp of
    the result holds with room (a result next to a rounding boundary may round the other way, which is 1 ulp and no more). area
    and normal are the reference's three statements on those floats, exactly."""
    worst = 0.0
    for light, a, t, _ in PAIRS:
        got = moved_host(twk, light, a, t)
        A, T = (np.concatenate([np.asarray(m, F).reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]]) for m in (a, t))
        d = T @ np.linalg.inv(A)
        for name in ("position", "vecU", "vecV"):
            want = d[:3, :3] @ light[name].astype(np.float64) + (d[:3, 3] if name == "position" else 0.0)
            err = np.abs(got[name].astype(np.float64) - want) / _ulp(got[name])
            worst = max(worst, float(err.max()))
            assert (err <= 1.0).all(), (name, got[name], want)
        n, area, normal = R.cross_area_normal(got["vecU"], got["vecV"])
        sign = -1.0 if np.linalg.det(d[:3, :3]) < 0.0 else 1.0
        assert got["area"] == area and got["normal"].tobytes() == (F(sign) * normal).tobytes()
        assert got["type"] == 1 and got["emission"].tobytes() == light["emission"].tobytes() and got["unused"].tobytes() == light["unused"].tobytes()
        # the lit side: the anchor's normal through the inverse transpose of D, which is what the emitter's hit shader does
        carried = np.linalg.inv(d[:3, :3]).T @ light["normal"].astype(np.float64)
        assert float(got["normal"].astype(np.float64) @ carried) > 0.0
    print(f"\nlight motion: position / vecU / vecV at most {worst:.3f} ulp from float64 linalg over {len(PAIRS)} pairs")


def test_host_form_refusals(twk):
    from tweeker_raytracer_amd import _lib as L
    light, a, t, _ = PAIRS[1]
    good = R.definition(twk, light)
    fp = lambda m: np.ascontiguousarray(m, F).ctypes.data_as(C.POINTER(C.c_float))
    out = twk.LightDefinition()
    before = bytes(out)

    def refused(anchor, at, tt, text):
        rc = L.lib.twk_light_moved_host(C.byref(anchor) if anchor is not None else None, fp(at) if at is not None else None, fp(tt) if tt is not None else None, C.byref(out))
        message = L.lib.twk_last_error().decode()
        assert rc == L.TWK_ERROR_INVALID_VALUE and message.startswith("twk_light_moved_host: ") and text in message, message
        assert bytes(out) == before, "a refused call leaves `out` as it was"

    refused(None, a, t, "NULL argument")
    refused(good, None, t, "NULL argument")
    refused(good, a, None, "NULL argument")
    assert L.lib.twk_light_moved_host(C.byref(good), fp(a), fp(t), None) == L.TWK_ERROR_INVALID_VALUE
    environment = R.definition(twk, light)
    environment.type = 0
    refused(environment, a, t, "not a TWK_LIGHT_PARALLELOGRAM")
    for bad in (np.nan, np.inf):
        broken = t.copy()
        broken[7] = bad
        refused(good, a, broken, "not finite")
        refused(good, broken, t, "not finite")
    refused(good, np.zeros(12, F), t, "determinant is zero")
    flat = a.copy().reshape(3, 4)
    flat[2, :3] = flat[1, :3]  # two equal rows: singular
    refused(good, flat.reshape(12), t, "determinant is zero")
    refused(good, a, np.zeros(12, F), "degenerate")            # the new matrix collapses the light to a point: area 0
    huge = (np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F) * F(3e38))
    refused(good, np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F) * F(0.01), huge, "degenerate")  # components beyond float32: not finite
    for light, at, tt in ((light, np.zeros(12, F), t), (light, a, np.zeros(12, F))):
        assert R.light_moved(light, at, tt) is None, "the restatement refuses what the header refuses"
    # out may be anchor
    same = R.definition(twk, light)
    assert L.lib.twk_light_moved_host(C.byref(same), fp(a), fp(t), C.byref(same)) == L.TWK_SUCCESS
    assert bytes(same) == R.light_moved(light, a, t).tobytes()


def test_host_form_makes_no_device_of_itself(twk):
    """Pure CPU: it answers on a machine without a GPU (this test runs there) and through a NULL-free, handle-free signature."""
    moved = twk.light_moved_host(E.base_case().scene.lights[0], E.IDENTITY, E.MOVES["reshape"][0])
    E.check_definition_is_the_rectangle(moved, E.MOVES["reshape"][1])
    moved = twk.light_moved_host(E.base_case().scene.lights[0], E.IDENTITY, E.MOVES["mirror"][0])
    E.check_definition_is_the_rectangle(moved, E.MOVES["mirror"][1])
    assert R.record(moved)["vecU"].tolist() == [-2.0, 0.0, 0.0], "the mirror turns vecU, and the normal stays down all the same"


def test_description_key_of_the_moving_emitters(twk):
    """`movingEmitters 1` is parsed and written back by twk_app_system_description (where rtigo3_hip reads it); 0 and the default write
    nothing; a word that is no number is a parse error, as for every numeric key."""
    from conftest import scene_path
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    scene = open(scene_path("scene_rtigo3_cornell_box.txt")).read()

    def description(text):
        app = twk.Application(system_text=text, scene_text=scene)
        try:
            return app.systemDescription()
        finally:
            app.close()

    assert "movingEmitters" not in description(base) and "movingEmitters" not in description(base + "\nmovingEmitters 0\n")
    on = description(base + "\nmovingEmitters 1\n")
    assert "movingEmitters 1\n" in on and description(on) == on, "what is written back parses to the same"
    assert "movingEmitters" not in description(base + "\nmovingEmitters 2\n"), "a value that is neither 0 nor 1 keeps the default"
    with pytest.raises(twk.TwkError):
        description(base + "\nmovingEmitters yes\n")


# ---- the same code under the sanitizers, in a stand-alone program ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("light_motion") / "light_motion_host")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "light_motion_host.cpp")]
    subprocess.run(cmd, check=True)
    return out


def test_the_rule_runs_clean_under_the_sanitizers(sanitized_program, tmp_path):
    """200 of the seeded pairs, the anchor's own transform, and the refusals through the stand-alone program: it exits 0 with nothing
    on stderr, and what it computed has the restatement's bits."""
    cases = [(l, a, t) for l, a, t, _ in PAIRS[:200]]
    cases += [(l, a, a.copy()) for l, a, _, _ in PAIRS[:8]]
    light = PAIRS[0][0]
    other = light.copy()
    other["type"] = 0
    refusals = [(other, PAIRS[0][1], PAIRS[0][2]), (light, np.zeros(12, F), PAIRS[0][2]), (light, PAIRS[0][1], np.zeros(12, F)), (light, np.full(12, np.nan, F), PAIRS[0][2])]
    cases += refusals
    case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes())
        f.write(b"".join(np.asarray(l, R.LIGHT).tobytes() for l, _, _ in cases))
        f.write(np.stack([a for _, a, _ in cases]).astype(F).tobytes())
        f.write(np.stack([t for _, _, t in cases]).astype(F).tobytes())
    # (the leak check stops the process with a tracer of its own, which a sandbox may forbid: off, the address checks are what is asked for)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([sanitized_program, case, result], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    raw = np.fromfile(result, np.uint8)
    moved = np.frombuffer(raw[: 80 * len(cases)].tobytes(), R.LIGHT)
    refused = np.frombuffer(raw[80 * len(cases):].tobytes(), np.int32)
    assert refused.tolist() == [0] * (len(cases) - len(refusals)) + [1] * len(refusals)
    for (l, a, t), got in zip(cases[: len(cases) - len(refusals)], moved):
        assert got.tobytes() == R.light_moved(l, a, t).tobytes()
    assert not raw[80 * (len(cases) - len(refusals)): 80 * len(cases)].any(), "a refused entry is left untouched"


# ---- the moved light through the oracle: direct_light's statistic on the right light and on each slip ------------------------------
CASE = E.base_case()
_runs = {}


def oracle_halves(orc, move, image, slip=None):
    """two_halves of one image of P1 with its light moved, on an oracle fed the FRESH scene: the instance under the move's transform
    and the definition twk_light_moved_host derives (slip: one of emitter_motion_cases.slipped's wrong ones instead)."""
    key = (move, image, slip)
    if key not in _runs:
        light = E.moved_definition(CASE, move)
        if slip:
            light = E.slipped(light, slip, CASE)
        ref = orc.Oracle(miss=CASE.scene.miss, nee=CASE.nee(image))
        D.feed(ref, E.fresh_scene(CASE, move, light), CASE.state(image))
        ref.setShaderVariant(CASE.variant)
        _runs[key] = D.render_halves(lambda it: ref.render(it, threads=8), ref.getOutputBufferHost, CASE.n[image])
        ref.close()
    return _runs[key]


MOVE_IMAGES = [(move, image) for move in E.MOVES for image in D.IMAGES]


@pytest.mark.parametrize("move,image", MOVE_IMAGES)
def test_oracle_moved_light_equals_the_moved_rectangles_reference(orc, move, image):
    E.check_definition_is_the_rectangle(E.moved_definition(CASE, move), E.MOVES[move][1])
    halves = oracle_halves(orc, move, image)
    R_, bias, sigma = D.statistic(halves, E.reference_case(CASE, E.MOVES[move][1]).reference(image))
    print("\n" + D.row(f"P1 {move}", image, CASE.n[image], R_, bias, sigma))
    assert D.BIAS_SIGMAS * sigma <= D.BIAS_POWER
    assert R_ <= D.R_BOUND, "block means differ from the closed form by more than their noise"
    assert abs(bias) <= D.BIAS_SIGMAS * sigma


@pytest.mark.parametrize("move,image", MOVE_IMAGES)
def test_oracle_moved_light_rejects_a_wrong_reference(orc, move, image):
    """The two controls on the reference: the moved rectangle 2 % larger, and the rectangle where it was before the move."""
    halves = oracle_halves(orc, move, image)
    for name, reference in (("area x 1.02", E.reference_case(CASE, E.MOVES[move][1]).reference(image, ("area", 1.02))),
                            ("unmoved rectangle", CASE.reference(image))):
        R_, bias, sigma = D.statistic(halves, reference)
        print("\n" + D.row(f"P1 {move}", image, CASE.n[image], R_, bias, sigma, f"  control: {name}"))
        assert not D.accepted(R_, bias, sigma), name


SLIPS = (("reshape", "stale area"), ("mirror", "un-negated normal"))


@pytest.mark.parametrize("move,slip", SLIPS)
def test_oracle_rejects_each_slip_of_the_rule(orc, move, slip):
    """A definition with the anchor's area after a reshape, or with cross(vecU, vecV) un-negated after a mirror, is rejected on
    "light" and "sum". "off", the brute-force image, reads neither area nor normal (the emitter's hit reads the emission alone there), so it
    cannot tell the slips from the right light and is not asserted on."""
    reference = E.reference_case(CASE, E.MOVES[move][1])
    for image in ("light", "sum"):
        halves = oracle_halves(orc, move, image, slip)
        with np.errstate(divide="ignore"):  # a black image has no noise: R is infinite, which is a rejection
            R_, bias, sigma = D.statistic(halves, reference.reference(image))
        print("\n" + D.row(f"P1 {move}", image, CASE.n[image], R_, bias, sigma, f"  slip: {slip}"))
        assert not D.accepted(R_, bias, sigma), (slip, image)
        if slip == "un-negated normal" and image == "light":
            assert halves[2][..., :3].max() == 0.0, "a light whose normal points away from the receiver samples nothing"
