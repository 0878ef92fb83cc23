"""What tests/test_light_motion_host.py (the oracle, on a CPU) and tests/test_gpu_emitter_direct_light.py (the HIP path) share: case
P1 of tests/direct_light.py with its light moved. A helper module, not a conftest.

P1's light is LIGHT_1 = Rect(-1, 3.5, -2, 2, 2), instance 1 of the scene (instance 0 is the receiver), light 0, under the identity.
Both moves keep it axis-parallel and lit side down, so direct_light's closed forms apply as they are to the rectangle the move makes.
The scenes, references, statistic and bounds are direct_light's own."""
import copy

import numpy as np

import direct_light as D
import tweeker_raytracer_amd as twk
from light_motion_restate import definition, record

LIGHT_INSTANCE, LIGHT_ID = 1, 0
# name: (transform, the rectangle it makes of LIGHT_1)
MOVES = {
    "reshape": (np.array([0.75, 0, 0, 0.5, 0, 1, 0, -0.5, 0, 0, 1.25, 0.25], np.float32), D.Rect(-0.25, 3.0, -2.25, 1.5, 2.5)),
    "mirror": (np.array([-1, 0, 0, 0.75, 0, 1, 0, 0.25, 0, 0, 1, 0.5], np.float32), D.Rect(-0.25, 3.75, -1.5, 2.0, 2.0)),
}
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def base_case():
    return D.make_cases()["P1"]


def moved_definition(case, move):
    """The light's definition after `move`: twk_light_moved_host on P1's own definition and the identity it was built under."""
    return twk.light_moved_host(case.scene.lights[LIGHT_ID], IDENTITY, MOVES[move][0])


def slipped(light, slip, case):
    """A definition with one of the two slips a wrong rule would make: "stale area" keeps the anchor's area, "un-negated normal" is
    cross(vecU, vecV) / area without the mirror's sign. Handed to a fresh handle or oracle, never made by a switch in the product."""
    rec = record(light)
    if slip == "stale area":
        rec["area"] = record(case.scene.lights[LIGHT_ID])["area"]
    elif slip == "un-negated normal":
        rec["normal"] = -rec["normal"]
    else:
        raise ValueError(slip)
    return definition(twk, rec)


def fresh_scene(case, move, light):
    """P1's scene as a fresh handle is given it after the move: the light's instance under the move's transform, `light` the definition."""
    s = copy.copy(case.scene)
    s.lights = [light]
    s.instances = list(case.scene.instances)
    g, _, m, l = s.instances[LIGHT_INSTANCE]
    assert l == LIGHT_ID
    s.instances[LIGHT_INSTANCE] = (g, MOVES[move][0].copy(), m, l)
    return s


def reference_case(case, rect):
    """P1 with `rect` where LIGHT_1 is: what Case.reference is asked for the moved light (and, with LIGHT_1 itself, for the control)."""
    c = copy.copy(case)
    c.lights = [("rect", rect, case.lights[LIGHT_ID][2])]
    c._points = None
    return c


def check_definition_is_the_rectangle(light, rect):
    """The derived definition spans `rect`, lit side down, exactly: the moves are exact in float."""
    rec = record(light)
    corners = np.array([rec["position"], rec["position"] + rec["vecU"], rec["position"] + rec["vecV"], rec["position"] + rec["vecU"] + rec["vecV"]], np.float64)
    assert corners[:, 0].min() == rect.x0 and corners[:, 0].max() == rect.x0 + rect.sx
    assert corners[:, 2].min() == rect.z0 and corners[:, 2].max() == rect.z0 + rect.sz
    assert (corners[:, 1] == rect.y).all()
    assert rec["normal"].tolist() == [0.0, -1.0, 0.0] and float(rec["area"]) == rect.area
