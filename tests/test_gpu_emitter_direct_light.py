"""-m gpu: the moved light is the RIGHT light. Case P1 of tests/direct_light.py (LIGHT_1 = Rect(-1, 3.5, -2, 2, 2)) is built, emitter
motion is switched on, and the light's instance is moved with twk_update_instance_transform; the three images are then held against
Case.reference of the rectangle the move produces, with direct_light's own statistic and bounds (R <= R_BOUND, |bias| <= 4 sigma,
4 sigma <= 0.01) at P1's iteration counts, 256 / 256 / 1024. Both moves of tests/emitter_motion_cases.py keep the light axis-parallel
and lit side down, so the closed forms apply as they are:
  reshape  [0.75,0,0,0.5, 0,1,0,-0.5, 0,0,1.25,0.25]  ->  Rect(-0.25, 3.0, -2.25, 1.5, 2.5)
  mirror   [-1,0,0,0.75, 0,1,0,0.25, 0,0,1,0.5]       ->  Rect(-0.25, 3.75, -1.5, 2.0, 2.0)
The controls: the moved rectangle 2 % larger and the unmoved rectangle as references, rejected on every image; and the two slips a
wrong rule would make — the anchor's area kept after the reshape, cross(vecU, vecV) un-negated after the mirror — handed as
definitions to a fresh handle (never made by a switch in the product) and rejected on "light" and "sum" ("off", the brute-force image,
reads neither area nor normal). tests/test_light_motion_host.py runs the same on the oracle, on a CPU; device and oracle agree bit
for bit, so the rows printed here repeat that file's (profiles/r33_emitter_motion.md holds both columns)."""
import numpy as np
import pytest

import direct_light as D
import emitter_motion_cases as E
import shading_fuzz as FZ

pytestmark = pytest.mark.gpu

CASE = E.base_case()
_runs = {}


def device_halves(twk, move, image, slip=None):
    """(two_halves of one image, the image after its first 2 iterations), rendered once per session. slip None: P1 built as it is and
    its light MOVED by the update call; else a fresh handle given the moved scene with the slipped definition."""
    key = (move, image, slip)
    if key not in _runs:
        dev = twk.Device(ordinal=0, miss=CASE.scene.miss)
        try:
            if slip is None:
                D.feed(dev, CASE.scene, CASE.state(image))
                dev.enableEmitterMotion()
                dev.updateInstanceTransform(E.LIGHT_INSTANCE, E.MOVES[move][0])
                assert bytes(dev.getLight(E.LIGHT_ID)) == bytes(E.moved_definition(CASE, move))
            else:
                D.feed(dev, E.fresh_scene(CASE, move, E.slipped(E.moved_definition(CASE, move), slip, CASE)), CASE.state(image))
            dev.setShaderVariant(CASE.variant)
            dev.setNextEventEstimation(CASE.nee(image))
            snapshot = {}
            halves = D.render_halves(dev.render, dev.getOutputBufferHost, CASE.n[image], snapshot)
        finally:
            dev.close()
        _runs[key] = (halves, snapshot["two"])
    return _runs[key]


MOVE_IMAGES = [(move, image) for move in E.MOVES for image in D.IMAGES]


@pytest.mark.parametrize("move,image", MOVE_IMAGES)
def test_first_two_iterations_equal_the_oracle_fed_the_fresh_scene(twk, orc, move, image):
    _, got = device_halves(twk, move, image)
    _, want, _ = FZ.render_oracle(orc, E.fresh_scene(CASE, move, E.moved_definition(CASE, move)), CASE.state(image), 2, CASE.variant, CASE.nee(image))
    bad = FZ.mismatch(got, want)
    assert bad is None, f"{move} {image}: {bad}"
    assert np.isfinite(want).all() and want[..., :3].max() > 0.0


@pytest.mark.parametrize("move,image", MOVE_IMAGES)
def test_moved_light_equals_the_moved_rectangles_reference(twk, move, image):
    E.check_definition_is_the_rectangle(E.moved_definition(CASE, move), E.MOVES[move][1])
    halves, _ = device_halves(twk, move, image)
    R, bias, sigma = D.statistic(halves, E.reference_case(CASE, E.MOVES[move][1]).reference(image))
    print("\n" + D.row(f"P1 {move}", image, CASE.n[image], R, bias, sigma))
    assert D.BIAS_SIGMAS * sigma <= D.BIAS_POWER
    assert R <= D.R_BOUND, "block means differ from the closed form by more than their noise"
    assert abs(bias) <= D.BIAS_SIGMAS * sigma


@pytest.mark.parametrize("move,image", MOVE_IMAGES)
def test_a_wrong_reference_is_rejected(twk, move, image):
    halves, _ = device_halves(twk, move, image)
    for name, reference in (("area x 1.02", E.reference_case(CASE, E.MOVES[move][1]).reference(image, ("area", 1.02))),
                            ("unmoved rectangle", CASE.reference(image))):
        R, bias, sigma = D.statistic(halves, reference)
        print("\n" + D.row(f"P1 {move}", image, CASE.n[image], R, bias, sigma, f"  control: {name}"))
        assert not D.accepted(R, bias, sigma), name


@pytest.mark.parametrize("move,slip", (("reshape", "stale area"), ("mirror", "un-negated normal")))
def test_each_slip_of_the_rule_is_rejected(twk, move, slip):
    reference = E.reference_case(CASE, E.MOVES[move][1])
    for image in ("light", "sum"):
        halves, _ = device_halves(twk, move, image, slip)
        with np.errstate(divide="ignore"):  # a black image has no noise: R is infinite, which is a rejection
            R, bias, sigma = D.statistic(halves, reference.reference(image))
        print("\n" + D.row(f"P1 {move}", image, CASE.n[image], R, bias, sigma, f"  slip: {slip}"))
        assert not D.accepted(R, bias, sigma), (slip, image)
        if slip == "un-negated normal" and image == "light":
            assert halves[2][..., :3].max() == 0.0, "a light whose normal points away from the receiver samples nothing"
