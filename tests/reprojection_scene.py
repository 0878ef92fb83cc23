"""What tests/test_reprojection_host.py (CPU) and tests/test_gpu_reprojection.py share: the scene of tests/reprojection_reference.py as
the library takes it — the cameras (tests/temporal_restate.py look_at: a camera builder, it does not touch the formulas under test),
and the surfaces as meshes of a shading_fuzz.Scene, which feeds a Device and an Oracle alike — the world of a scenario as the
reference sees it, computed once, and the judging of a merge against it. A helper module, not a conftest. The reference traces the
unit squares and the patch from the same float32 vertices and transforms that are handed over here."""
import functools
import types

import numpy as np

import reprojection_reference as R
from reprojection_reference import HEIGHT, U, WIDTH
from temporal_restate import look_at

F, U32, D = np.float32, np.uint32, np.float64
K_AOV = 16        # G's constant: four times the largest ratio measured against the oracle (3.22), rounded up to a power of two
LAYERS = 3
RECTIFY = (3, 8, 3.0)
SCENARIOS = {"static": (False, False), "moved": (True, False), "deformed": (True, True)}
PLACES = [False, True]
place_id = lambda far: "far" if far else "near"

FLATTEN = {"flattened": (4, 2), "two-level": (0, 0)}  # the default policy (include/tweeker_hip.h TWK_FLATTEN_*) and every instance entered


def cameras(far=False):
    """(current, history) as 12 float32 words: the current camera looks from (0.5, 0.4, 4.0) at the origin, the history camera from
    (-0.4, 0.2, 4.2) at (0.1, 0, 0); far: both translated by R.FAR with the scene."""
    offset = R.FAR if far else np.zeros(3)
    aspect = R.WIDTH / R.HEIGHT
    return (look_at(np.array((0.5, 0.4, 4.0)) + offset, np.array((0.0, 0.0, 0.0)) + offset, R.FOV, aspect),
            look_at(np.array((-0.4, 0.2, 4.2)) + offset, np.array((0.1, 0.0, 0.0)) + offset, R.FOV, aspect))


def attributes(vertices):
    """Vertex records [n, 12] (position, tangent, normal, texcoord) of object-space positions on or near z = 0."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    a = np.zeros((v.shape[0], 12), F)
    a[:, 0:3], a[:, 3], a[:, 8], a[:, 9:11] = v, 1.0, 1.0, v[:, 0:2]
    return a


SQUARE = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F), np.array([0, 1, 2, 2, 3, 0], np.uint32))  # twk.mesh_parallelogram's layout


def mesh(surface):
    """(attributes [n, 12], indices) of a reference surface."""
    if surface.kind == "square":
        return attributes(SQUARE[0]), SQUARE[1].copy()
    return attributes(surface.vertices), np.ascontiguousarray(surface.triangles, np.uint32).reshape(-1)


def camera_definition(twk, words):
    """A CameraDefinition of 12 float32 words (P, U, V, W)."""
    c = twk.CameraDefinition()
    for k in range(3):
        c.P[k], c.U[k], c.V[k], c.W[k] = (float(words[3 * j + k]) for j in range(4))
    return c


def fuzz_scene(surfaces, camera_words, flatten, area_light=False, far=False):
    """A shading_fuzz.Scene of the surfaces — one geometry and one instance each, in order — with one diffuse material under the
    constant white environment, and its state at R.WIDTH x R.HEIGHT. area_light: a black environment and a square light of edge 1
    above both views instead (one more instance, after the surfaces; far: translated by R.FAR with the scene) — under the constant environment most of the wall has no noise."""
    from shading_fuzz import Scene, default_state, environment_light, material, parallelogram_light, transform
    import tweeker_raytracer_amd as twk
    s = Scene()
    s.miss, s.flatten = 1, FLATTEN[flatten] if isinstance(flatten, str) else flatten
    s.camera = camera_definition(twk, camera_words)
    s.lights = [environment_light()]
    s.materials = [material(0, albedo=(0.7, 0.7, 0.7))]
    for i, surface in enumerate(surfaces):
        a, idx = mesh(surface)
        s.geometries.append((a, idx))
        s.instances.append((i, surface.transform.copy(), 0, -1))
    if area_light:
        offset = R.FAR if far else np.zeros(3)
        light = parallelogram_light(np.array((-1.0, 2.6, 1.5)) + offset, 1.0, (20.0, 20.0, 20.0))
        s.miss, s.lights = 0, [light]
        s.materials.append(material(1, albedo=(0.0, 0.0, 0.0), thinwalled=1))
        s.geometries.append(tuple(np.ascontiguousarray(a) for a in twk.mesh_parallelogram(list(light.position), list(light.vecU), list(light.vecV), list(light.normal))))
        s.instances.append((len(surfaces), transform(), 1, 0))
    state = default_state(s, pathLengths=(2, 4))
    state.resolution[0], state.resolution[1] = R.WIDTH, R.HEIGHT
    return s, state


# ---- the world of a scenario ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(far, scenario):
    """Everything the reference says about a scenario, computed once and left unchanged: the cameras, the surfaces now and as of the
    history's frame, the hits of both views, the float32 AOVs, the float64 previous positions, the expected lookup and B."""
    moved, deformed = SCENARIOS[scenario]
    w = types.SimpleNamespace(far=far, scenario=scenario)
    w.words_now, w.words_then = cameras(far)
    w.now, w.then = R.Camera(w.words_now), R.Camera(w.words_then)
    w.surfaces, w.previous = R.scene(far, moved, deformed), R.scene(far)
    w.hits = R.trace(w.surfaces, *w.now.rays(WIDTH, HEIGHT))
    w.history_hits = R.trace(w.previous, *w.then.rays(WIDTH, HEIGHT))
    w.g, w.hg = R.aov(w.hits), R.aov(w.history_hits)
    w.gp = R.previous_positions(w.hits, w.surfaces, w.previous)
    w.lookup = R.expected_lookup(w.gp, w.hits.instance, w.then, w.history_hits.instance)
    w.B = R.bound_B(w.gp, w.then, w.lookup, WIDTH, HEIGHT)
    return w


def motion_table(twk, w):
    """The table of twk_instance_motion's records for the scenario, as a RECORD array."""
    from temporal_motion_restate import RECORD
    return np.array([np.frombuffer(bytes(twk.instance_motion(then.transform, now.transform)), RECORD)[0] for now, then in zip(w.surfaces, w.previous)], RECORD)


# ---- judging a merge -----------------------------------------------------------------------------------------------------------------
def judge(w, position_rgb, count, outputs_and_inputs, lookup=None, B=None, constant=1.0, keep=None):
    """What a merge did against what the reference expects. position_rgb [H, W, >= 3]: the merged code; count [H, W]: the merged
    sample count (above the frame's 1 where history was taken); outputs_and_inputs: pairs that must have equal bits where no history
    was taken. Returns a namespace: took_wrong (pixels), passed_wrong, ratio [H, W] = the position error / B on the `full` pixels (NaN
    elsewhere), constant_error (largest |z / constant - 1| on them), and ok. keep [H, W]: the pixels the position and the took checks
    look at (the GPU tests leave their exclusion out of both); None: every pixel."""
    lookup = w.lookup if lookup is None else lookup
    B = w.B if B is None else B
    taken = count > F(1.0)
    out = types.SimpleNamespace(taken=taken)
    keep = np.ones(taken.shape, bool) if keep is None else keep
    out.took_wrong = int(((taken != lookup.took) & keep).sum())
    untouched = np.ones(taken.shape, bool)
    for got, given in outputs_and_inputs:
        assert got.dtype == given.dtype and got.shape == given.shape
        bits = U32 if got.dtype == F else np.uint16
        same = np.ascontiguousarray(got).view(bits) == np.ascontiguousarray(given).view(bits)
        untouched &= same.all(axis=-1) if got.ndim == 3 else same.all(axis=(0, -1))  # [H, W, 4], or the cascade's [K, H, W, 4]
    out.passed_wrong = int((~taken & ~untouched).sum())
    x, y, z = R.decode(position_rgb)
    full = lookup.full & taken & keep
    error = np.maximum(np.abs(x - lookup.fx), np.abs(y - lookup.fy))
    out.full = full
    out.ratio = np.where(full, error / B, np.nan)
    out.error = np.where(full, error, np.nan)
    out.constant_error = float(np.abs(z[full] / constant - 1.0).max()) if full.any() else 0.0
    out.worst = float(np.nanmax(out.ratio)) if full.any() else 0.0
    out.ok = out.took_wrong == 0 and out.passed_wrong == 0 and out.worst <= 1.0 and out.constant_error <= 4 * U
    return out


def report(what, w, verdict):
    print(f"{what}, {place_id(w.far)}, {w.scenario}: full {int(verdict.full.sum())}, largest error {np.nanmax(verdict.error):.3e} px, largest error / B {verdict.worst:.4f}, "
          f"took wrong {verdict.took_wrong}, passed through wrong {verdict.passed_wrong}, constant off by {verdict.constant_error / U:.2f} u")


def plane_bound(w, K=K_AOV):
    """G for the previous-position plane: the AOV's term, and the same term for the previous vertices and the previous matrix."""
    largest = np.array([np.abs(s.transform).max() for s in w.previous])[np.maximum(w.hits.instance, 0)]
    return R.bound_G(K, w.now.P, w.hits.position, w.hits.cos, extra=np.abs(w.gp).max(axis=-1) + largest)
