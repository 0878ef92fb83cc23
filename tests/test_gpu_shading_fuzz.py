"""-m gpu: materials and pass state fuzzed through every build of shadeKernel, device against oracle bit for bit.

Scenes and states come from tests/shading_fuzz.py (seeded; the oracle alone is checked on them in tests/test_shading_fuzz_host.py).
  * Build matrix: ENV x TEX x {slim, full} x three table bands = 24 scenes, each rendered by the device in five modes (default,
    TWK_SHADE_SORT=0, TWK_SHADE_SORT=2, statistics, time view) and once by the oracle. Every image equals the oracle's; the union of
    the builds twk_debug_shade_builds reports must be every launcher slot the library holds, minus UNREACHABLE (empty today).
  * Branch coverage: the statistics runs must have lanes in every shading phase named in PHASES.
  * State sweep: 24 seeds, each a whole drawn state (path lengths, lens shader, samplesSqrt, epsilon, shader variant, NEE, output
    format, launch batch) on a mid-size scene; image and both AOVs equal the oracle's in the drawn format.
  * Range ends: roughness 0 and ior at the GUI's ends; where the oracle is NaN the device is NaN, everything else bit for bit.
  * The two analytic anchors of the host test, on the device.
A mismatch message names the seed, the feature tuple, the mode, the count of differing pixels and the first one (x, y): that pixel
goes into tools/debug_pixel_mismatch.py or Oracle.debugPath.
"""
import os

import numpy as np
import pytest

import shading_fuzz as F
from test_shading_fuzz_host import MATRIX, check_slab, matrix_scene

pytestmark = pytest.mark.gpu

MODES = ("default", "sort0", "sort2", "stats", "timeview")
ITERATIONS = 2
MATRIX_PATH_LENGTHS = (2, 16)  # 16 bounces: through the six nested spheres and out again

# Launcher slots that hold a build but that no state of launchShade (shade_kernels.hip) can select, index -> reason. Every flag is
# free there: ENV and TEX follow the scene, PRIMARY the launch's depth, SLIM the stream layout; MEASURE excludes SORT, SORT needs
# LDS_TABLES, and the slots that break those two rules are null (shadeLauncher). So nothing is unreachable, and a build added to the
# dispatcher must be launched by this file or argued into this list.
UNREACHABLE = {}

# TwkLaunchStats::shadePhaseLanes indices (include/tweeker_hip.h TWK_SHADE_PHASE_*)
PHASES = {"PATH": 0, "VOLUME_FETCH": 1, "MISS": 2, "HIT_RECORD": 3, "TANGENT": 4, "LIGHT_HIT": 6, "BSDF_DIFFUSE": 7, "BSDF_MIRROR": 8,
          "BSDF_GLASS": 9, "BSDF_GGX": 10, "BSDF_GGX_GLASS": 11, "NEE_SAMPLE": 12, "NEE_EVAL": 13, "VOLUME_PUSH": 16}
PHASE_TEXCOORD = 5


def render_device(twk, scene, state, iterations, mode="default", variant=0, nee=True, half=False, aov=False, batch=None):
    """-> dict(image, aovs, builds, stats, layout). The TWK_SHADE_SORT modes set the variable the device reads when it is created."""
    saved = os.environ.get("TWK_SHADE_SORT")
    if mode in ("sort0", "sort2"):
        os.environ["TWK_SHADE_SORT"] = mode[-1]
    try:
        dev = twk.Device(ordinal=0, miss=scene.miss)
    finally:
        if mode in ("sort0", "sort2"):
            if saved is None:
                del os.environ["TWK_SHADE_SORT"]
            else:
                os.environ["TWK_SHADE_SORT"] = saved
    try:
        F.feed(dev, scene, state)
        dev.setShaderVariant(variant)
        dev.setNextEventEstimation(nee)
        dev.enableAov(aov)
        if half:
            dev.setOutputFormat(1)
        if batch is not None:
            dev.setLaunchBatch(batch)
        if mode == "stats":
            dev.statsEnable(True)
        if mode == "timeview":
            dev.setTimeView(True)
        layout = dev.streamLayout()
        dev.debugShadeBuilds(reset=True)
        for it in range(iterations):
            dev.render(it)
        dev.synchronizeStream()
        out = {"image": dev.getOutputBufferHost().copy(), "aovs": [dev.readAov(0).copy(), dev.readAov(1).copy()] if aov else None,
               "builds": dev.debugShadeBuilds(), "stats": dev.statsGet() if mode == "stats" else None, "layout": layout}
    finally:
        dev.close()
    return out


_matrix_cache = {}


def run_matrix_scene(twk, orc, key):
    """Renders one matrix scene in every mode (once per session) and compares each image with the oracle's.
    -> (builds launched, shadePhaseLanes of the statistics run)."""
    if key in _matrix_cache:
        return _matrix_cache[key]
    scene = matrix_scene(*key)
    state = F.default_state(scene, MATRIX_PATH_LENGTHS)
    _, want, _ = F.render_oracle(orc, scene, state, ITERATIONS)
    builds, lanes = set(), None
    for mode in MODES:
        got = render_device(twk, scene, state, ITERATIONS, mode)
        assert got["layout"] == scene.predicted_layout, (scene.features, got["layout"])
        # the table band shows in the LDS_TABLES flag (bit 3) of the builds: small always, large never, mid in the plain builds only
        lds = {bool(b & 8) for b in got["builds"]}
        expect_lds = {"small": {True}, "large": {False}, "mid": {mode not in ("stats", "timeview")}}[scene.band]
        assert lds == expect_lds, (scene.features, mode, sorted(got["builds"]))
        image, reference = (got["image"][..., :3], want[..., :3]) if mode == "timeview" else (got["image"], want)  # alpha is the path time there
        bad = F.mismatch(image, reference)
        assert bad is None, f"seed {scene.seed}, features {scene.features}, mode {mode}: {bad}"
        builds |= got["builds"]
        if mode == "stats":
            lanes = got["stats"]["shadePhaseLanes"]
    _matrix_cache[key] = (builds, lanes)
    return _matrix_cache[key]


@pytest.mark.parametrize("env,tex,full,band", MATRIX)
def test_matrix_scene_equals_the_oracle_in_every_mode(twk, orc, env, tex, full, band):
    builds, lanes = run_matrix_scene(twk, orc, (env, tex, full, band))
    for b in builds:  # the flags the scene fixes
        assert bool(b & 1) == env and bool(b & 2) == tex and bool(b & 64) == (not full), (twk.shade_build_name(b), (env, tex, full, band))
    for name, index in PHASES.items():
        assert lanes[index] > 0, f"features {(env, tex, full, band)}: no lane ever ran phase {name}"
    if tex:
        assert lanes[PHASE_TEXCOORD] > 0, f"features {(env, tex, full, band)}: no lane ever ran phase TEXCOORD"


def launched_over(twk, orc, keys):
    launched = set()
    for key in keys:
        launched |= run_matrix_scene(twk, orc, key)[0]
    return launched


def check_every_build_was_launched(twk, launched):
    have = twk.shade_build_slots()
    assert set(UNREACHABLE) <= have
    missing = have - set(UNREACHABLE) - launched
    assert not missing, f"{len(missing)} builds of shadeKernel were never launched: {sorted(twk.shade_build_name(b) for b in missing)}"
    assert launched <= have
    assert not (launched & set(UNREACHABLE)), "a build listed as unreachable was launched"


def test_every_build_the_library_holds_was_launched(twk, orc):
    """The union over the whole matrix (scenes already rendered by the tests above are not rendered again). Dropping one axis of
    the matrix, for example the large band, makes this fail: tried once, see the pull request."""
    check_every_build_was_launched(twk, launched_over(twk, orc, MATRIX))


def compare_case(twk, orc, scene, state, iterations, what, variant=0, nee=True, half=False, batch=None, nan_positions_only=False):
    _, image, aovs = F.render_oracle(orc, scene, state, iterations, variant, nee, half, aov=True)
    got = render_device(twk, scene, state, iterations, "default", variant, nee, half, aov=True, batch=batch)
    assert got["layout"] == scene.predicted_layout
    for name, g, w in (("image", got["image"], image), ("albedo AOV", got["aovs"][0], aovs[0]), ("normal AOV", got["aovs"][1], aovs[1])):
        bad = F.mismatch(g, w, nan_positions_only)
        assert bad is None, f"{what}, features {scene.features}, mode default, {name}: {bad}"
    return image


@pytest.mark.parametrize("seed", F.SWEEP_SEEDS)
def test_state_sweep_equals_the_oracle(twk, orc, seed):
    case = F.draw_case(seed)
    scene = F.case_scene(case)
    iterations = case["samplesSqrt"] ** 2
    compare_case(twk, orc, scene, F.case_state(case, scene), iterations, f"seed {seed}, case {case}", case["variant"], case["nee"], case["half"],
                 batch=iterations if case["batchAll"] else 1)


def test_range_ends_agree_where_the_oracle_is_a_number(twk, orc):
    scene = F.make_scene(4242, 1, True, True, "mid", range_ends=True)
    image = compare_case(twk, orc, scene, F.default_state(scene, (2, 6)), 4, "seed 4242, range ends", nan_positions_only=True)
    assert np.isnan(image).any(axis=2).mean() <= 0.05


def test_invisible_glass_on_the_device(twk):
    scene, state = F.invisible_glass_scene()
    got = render_device(twk, scene, state, 2)["image"]
    bad = F.mismatch(got, np.ones_like(got))
    assert bad is None, f"invisible glass: {bad}"


def test_beer_lambert_slab_on_the_device(twk):
    scene, state = F.slab_scene()
    check_slab(render_device(twk, scene, state, 1)["image"], scene.camera)
