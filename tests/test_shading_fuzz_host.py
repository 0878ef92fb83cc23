"""CPU: the shading fuzz generator (tests/shading_fuzz.py) and what it promises, on the oracle alone.
  * the same seed gives byte-equal arrays;
  * its slim / full and table-band predictions use the byte sizes and budgets the product's sources state;
  * the oracle renders every generated scene finite (NaN-capped in the range-ends case) and not black, reaches both clamps of the
    volume stack in the nested spheres, and the 24 sweep seeds draw every value of every state axis;
  * the two analytic anchors (invisible glass, Beer-Lambert slab) hold on the oracle; tests/test_gpu_shading_fuzz.py repeats them on the device.
"""
import itertools
import os
import re

import numpy as np
import pytest

import shading_fuzz as F
from conftest import ROOT

MATRIX = list(itertools.product((False, True), (False, True), (False, True), F.BANDS))  # ENV x TEX x full x band = 24


def matrix_scene(env, tex, full, band):
    # scenes without the spherical environment alternate between the black and the constant white miss program
    miss = 2 if env else (1 if (tex != full) else 0)
    seed = 100 + MATRIX.index((env, tex, full, band))
    return F.make_scene(seed, miss, tex, full, band)


def test_same_seed_gives_byte_equal_arrays():
    for args in ((5, 2, True, True, "mid"), (6, 0, False, False, "large")):
        assert F.make_scene(*args).arrays() == F.make_scene(*args).arrays()
    assert F.make_scene(5, 2, True, True, "mid").arrays() != F.make_scene(7, 2, True, True, "mid").arrays()
    assert F.draw_case(1003) == F.draw_case(1003)
    a, b = F.make_scene(5, 1, False, False, "small", range_ends=True), F.make_scene(5, 1, False, False, "small", range_ends=True)
    assert a.arrays() == b.arrays()


def test_predictions_use_the_products_byte_sizes(twk):
    csrc = os.path.join(ROOT, "tweeker_raytracer_amd", "csrc")
    api = open(os.path.join(csrc, "device_handle.h")).read()
    shade = open(os.path.join(csrc, "shade_kernels.hip")).read()
    assert int(re.search(r"static_assert\(sizeof\(DevInstance\) == (\d+)", api).group(1)) == F.INSTANCE_BYTES
    assert int(re.search(r"static_assert\(sizeof\(DevMaterial\) == (\d+)", api).group(1)) == F.MATERIAL_BYTES
    assert "static_assert(sizeof(DevLight) == sizeof(TwkLightDefinition)" in api
    import ctypes
    assert ctypes.sizeof(twk.LightDefinition) == F.LIGHT_BYTES
    assert int(re.search(r"#define TWK_SHADE_SORT_TABLE_BYTES (\d+)", shade).group(1)) == F.SORT_TABLE_BYTES
    assert int(re.search(r"#define TWK_SHADE_TABLE_BYTES (\d+)", shade).group(1)) == F.TABLE_BYTES
    for env, tex, full, band in MATRIX:
        s = matrix_scene(env, tex, full, band)
        assert s.predicted_band == band, (s.features, s.table_bytes)
        assert s.predicted_layout == ("full" if full else "slim"), s.features
        assert (s.miss == 2) == env
    for seed in F.SWEEP_SEEDS:
        case = F.draw_case(seed)
        s = F.case_scene(case)
        assert s.predicted_band == "mid" and s.predicted_layout == ("full" if case["full"] else "slim")


def test_every_scene_holds_the_material_space():
    s = matrix_scene(True, True, True, "small")
    fuzz = s.materials[F.M_FUZZ0:F.M_FUZZ0 + F.NUM_FUZZ]
    assert {(m.indexBSDF, m.thinwalled) for m in fuzz} == set(itertools.product(range(5), (0, 1)))
    rough = np.array([[m.roughness[0], m.roughness[1]] for m in fuzz])
    assert rough.min() >= np.float32(0.001) and rough.max() == 1.0 and [float(np.float32(0.001)), 1.0] in rough.tolist()  # 1000 : 1
    iors = [m.ior for m in fuzz]
    assert 1.0 in iors and min(iors) >= 0.5 and max(iors) <= 3.0 and min(iors) < 1.0
    assert {m.absorptionScale for m in fuzz} == set(F.ABSORPTION_SCALES)
    assert any(m.useAlbedoTexture and m.indexBSDF != 0 for m in fuzz)
    assert any(m.useCutoutTexture and m.indexBSDF == 2 for m in s.materials)
    assert sum(1 for l in s.lights if l.type == 1) == 3 and len({(l.area, l.emission[0]) for l in s.lights if l.type == 1}) == 3
    ends = F.make_scene(1, 1, False, False, "small", range_ends=True).materials[F.M_FUZZ0:F.M_FUZZ0 + F.NUM_FUZZ]
    assert any(m.roughness[0] == 0.0 and m.roughness[1] == 0.0 for m in ends) and any(m.roughness[0] == 0.0 and m.roughness[1] > 0.0 for m in ends)
    assert {0.0, 10.0} <= {m.ior for m in ends}  # the ends of the GUI's ior range (Application.cpp:956)


def test_sweep_seeds_draw_every_value_of_every_axis():
    cases = [F.draw_case(seed) for seed in F.SWEEP_SEEDS]
    assert len(cases) >= 24
    want = {"miss": {0, 1, 2}, "tex": {False, True}, "full": {False, True}, "lensShader": {0, 1, 2}, "samplesSqrt": {1, 2, 3},
            "epsilonFactor": set(F.EPSILON_FACTORS), "variant": {0, 1}, "nee": {False, True}, "half": {False, True}, "batchAll": {False, True}}
    for key, values in want.items():
        assert {c[key] for c in cases} == values, key
    assert {c["pathLengths"][0] for c in cases} == set(F.PATH_MIN) and {c["pathLengths"][1] for c in cases} == set(F.PATH_MAX)


@pytest.mark.parametrize("env,tex,full,band", MATRIX)
def test_oracle_renders_every_matrix_scene(orc, env, tex, full, band):
    s = matrix_scene(env, tex, full, band)
    ref, img, _ = F.render_oracle(orc, s, F.default_state(s, (2, 16)), 2)
    assert np.isfinite(img).all(), s.features
    assert (img[..., :3].max(axis=2) > 0).mean() > 0.2, s.features
    push, pop = ref.stackClamps()  # the six nested spheres overflow the four-entry volume stack, and the way out underflows it
    assert push > 0 and pop > 0, (s.features, push, pop)


@pytest.mark.parametrize("seed", F.SWEEP_SEEDS)
def test_oracle_renders_every_sweep_case(orc, seed):
    case = F.draw_case(seed)
    s = F.case_scene(case)
    n = case["samplesSqrt"] ** 2
    _, img, aovs = F.render_oracle(orc, s, F.case_state(case, s), n, case["variant"], case["nee"], case["half"], aov=True)
    assert np.isfinite(img).all() and all(np.isfinite(a).all() for a in aovs), case
    assert img[..., :3].max() > 0, case
    if case["half"]:
        assert np.array_equal(img, img.astype(np.float16).astype(np.float32))


def test_oracle_range_ends_stay_within_the_nan_cap(orc):
    s = F.make_scene(4242, 1, True, True, "mid", range_ends=True)
    _, img, _ = F.render_oracle(orc, s, F.default_state(s, (2, 6)), 4)
    assert np.isnan(img).any(axis=2).mean() <= 0.05
    assert (np.nan_to_num(img[..., :3]).max(axis=2) > 0).mean() > 0.2


def test_invisible_glass_on_the_oracle(orc):
    s, st = F.invisible_glass_scene()
    _, img, _ = F.render_oracle(orc, s, st, 2)
    assert np.array_equal(F.bits(img), F.bits(np.ones_like(img))), F.mismatch(img, np.ones_like(img))


def check_slab(img, camera):
    """Every pixel within the analytic interval of its footprint, widened by F.SLAB_TOLERANCE (derived there from the fp32 roundings
    along the chain and the oracle-exp bound of tests/test_oracle_math.py, not from a run)."""
    lo, hi = F.slab_expected_interval(camera)
    rgb = img[..., :3].astype(np.float64)
    excess = np.maximum(lo - rgb, rgb - hi)
    print(f"slab: largest distance outside the analytic interval {excess.max():.3e} (tolerance {F.SLAB_TOLERANCE:.3e}), interval width up to {(hi - lo).max():.3e}")
    y, x, c = (int(v) for v in np.unravel_index(np.argmax(excess), excess.shape))
    assert excess.max() <= F.SLAB_TOLERANCE, f"pixel x={x}, y={y}, channel {c}: {rgb[y, x, c]} outside [{lo[y, x, c]}, {hi[y, x, c]}]"
    assert np.all(img[..., 3] == 1.0)
    assert hi.max() < 0.9 and lo.min() > 0.2  # the slab absorbs visibly in every channel and nowhere to black


def test_beer_lambert_slab_on_the_oracle(orc):
    s, st = F.slab_scene()
    _, img, _ = F.render_oracle(orc, s, st, 1)
    check_slab(img, s.camera)


def test_shade_build_tap_without_a_gpu(twk):
    from tweeker_raytracer_amd import _lib
    slots = twk.shade_build_slots()
    assert slots and slots <= set(range(128))
    assert twk.shade_build_name(0) == "plain" and twk.shade_build_name(1 | 8 | 32) == "ENV|LDS_TABLES|SORT"
    import ctypes
    mask = (ctypes.c_uint64 * 2)()
    assert _lib.lib.twk_debug_shade_builds(None, mask, 1) == _lib.TWK_ERROR_INVALID_VALUE
    assert "twk_debug_shade_builds" in _lib.lib.twk_last_error().decode()
    assert _lib.lib.twk_debug_shade_build_slots(None) == _lib.TWK_ERROR_INVALID_VALUE
