"""Direct lighting against closed-form irradiance on the ORACLE (tests/direct_light.py holds scenes, references and the statistic;
tests/test_gpu_direct_light.py runs the same cases on the HIP path). Not marked gpu: what the acceptance thresholds do on every
case is known here, on a CPU, before a GPU is touched - device and oracle agree bit for bit, so the statistic a GPU test sees is
the one this file sees at the same iteration count.
  * the float64 references against themselves: Lambert's formula against a 512 x 512 quadrature, the hemisphere's light half
    against its closed form, the constant map's true radiance rho * c, the stored R bounds against the simulation that made them;
  * every case and image through the oracle: R <= R_BOUND, |bias| <= 4 sigma, and 4 sigma <= 0.01 so that the test has power;
  * every negative control rejected: a reference wrong by little (a light 2 % larger, an occluder missing, numLights dropped, the
    map shifted or mirrored, envIntegral 2 % off) must fail the statistic the right reference passes."""
import math

import numpy as np
import pytest

import direct_light as D

CASES = D.make_cases()
_runs = {}


def oracle_halves(orc, case, image):
    """two_halves of one image of one case, rendered once per session."""
    key = (case.id, image)
    if key not in _runs:
        ref = orc.Oracle(miss=case.scene.miss, nee=case.nee(image))
        D.feed(ref, case.scene, case.state(image))
        ref.setShaderVariant(case.variant)
        _runs[key] = D.render_halves(lambda it: ref.render(it, threads=8), ref.getOutputBufferHost, case.n[image])
        ref.close()
    return _runs[key]


def test_r_bounds_are_what_the_simulation_gives():
    assert D.R_BOUND == round(D.null_quantile(D.GRID[0] * D.GRID[1]), 3)
    assert D.R_BOUND_GGX == round(D.null_quantile(D.GGX_BLOCKS ** 2), 3)


@pytest.mark.parametrize("case_id", [c for c in CASES if CASES[c].rects or CASES[c].occluders])
def test_lamberts_formula_equals_its_quadrature(case_id):
    """At the corner and centre pixels (their centres), per rectangle of the scene, to 1e-6 relative."""
    case = CASES[case_id]
    points = case.points.mean(axis=2)
    for y, x in ((0, 0), (0, D.WIDTH - 1), (D.HEIGHT - 1, 0), (D.HEIGHT - 1, D.WIDTH - 1), (D.HEIGHT // 2, D.WIDTH // 2)):
        for rect in case.rects + list(case.occluders):
            closed = float(D.lambert(points[y, x][None, :], case.receiver.normal, rect.vertices())[0])
            numeric = D.midpoint_form_factor(points[y, x], case.receiver.normal, rect)
            assert abs(closed - numeric) <= 1e-6 * numeric, (case_id, x, y, closed, numeric)


def test_clipped_light_equals_its_quadrature():
    """P1c: Lambert's formula over the visible part of the light against a quadrature that tests every cell's segment to the
    receiver point against the occluder. The cells cut by the shadow's edge bound the difference: 4 * 512 cells of 512^2."""
    case = CASES["P1c"]
    light, occluder = case.rects[0], case.occluders[0]
    points = case.points.mean(axis=2)
    cells = 512
    x = light.x0 + (np.arange(cells) + 0.5) / cells * light.sx
    z = light.z0 + (np.arange(cells) + 0.5) / cells * light.sz
    partly = 0
    for y_, x_ in ((0, 0), (0, D.WIDTH - 1), (D.HEIGHT - 1, 0), (D.HEIGHT - 1, D.WIDTH - 1), (D.HEIGHT // 2, D.WIDTH // 2)):
        p = points[y_, x_]
        d = np.stack(np.broadcast_arrays(x[:, None] - p[0], light.y - p[1], z[None, :] - p[2]), -1)
        s = (occluder.y - p[1]) / d[..., 1]
        ox, oz = p[0] + s * d[..., 0], p[2] + s * d[..., 2]
        seen = ~((ox > occluder.x0) & (ox < occluder.x0 + occluder.sx) & (oz > occluder.z0) & (oz < occluder.z0 + occluder.sz))
        r2 = (d * d).sum(-1)
        term = (d @ case.receiver.normal) * d[..., 1] / (r2 * r2) * light.area / cells ** 2
        numeric = float((term * seen).sum())
        closed = float(D.form_factor(p[None, :], case.receiver.normal, light, [occluder])[0])
        assert abs(closed - numeric) <= 4 * cells * float(term.max()), (x_, y_, closed, numeric)
        partly += 0.0 < closed < float(D.lambert(p[None, :], case.receiver.normal, light.vertices())[0])
    assert partly > 0, "the occluder hides a part of the light from a part of the frame"


def test_hemisphere_light_half_closed_form():
    c, w = np.polynomial.legendre.leggauss(64)
    c, w = 0.5 * (c + 1.0), 0.5 * w
    numeric = 2.0 * math.pi * float((D.power(D.P_SPHERE, c / math.pi) * c * w).sum())
    assert abs(numeric - D.HEMISPHERE_LIGHT_HALF) <= 1e-12


def test_constant_map_is_rho_times_its_colour():
    """E2: the true radiance is exactly rho * c; the quadrature of the NEE-off reference says so to 1e-5."""
    got = CASES["E2"].reference("off")[0, 0]
    assert np.allclose(got, np.array(D.RHO) * np.array((0.5, 1.0, 2.0)), rtol=1e-5, atol=0.0)


def test_importance_table_is_the_oracles(orc):
    """The float64 restatement of the CDF build against the tables the oracle itself builds (float32): the probability of every
    texel and envIntegral."""
    tex = D.lobe_map()
    ref = orc.Oracle(miss=2)
    ref.initTexture(2, tex)
    cdf_u, cdf_v, integral = ref.envTables(tex.shape[1], tex.shape[0])
    ref.close()
    cdf_u = cdf_u.reshape(tex.shape[0], tex.shape[1] + 1).astype(np.float64)
    probability = np.diff(cdf_u, axis=1) * np.diff(cdf_v.astype(np.float64))[:, None]
    want, want_integral = D.importance(tex.astype(np.float64))
    assert np.allclose(probability, want, rtol=0.0, atol=1e-5 * want.max())
    assert abs(integral - want_integral) <= 1e-5 * want_integral


def test_the_map_has_one_lobe_off_every_axis():
    tex = D.lobe_map().astype(np.float64)
    assert 45.0 < tex[..., 0].max() / tex[..., 0].min() <= 50.0
    phi, theta = (D.LOBE_U - 0.37) * 2 * math.pi, D.LOBE_V * math.pi
    direction = np.array([-math.sin(phi) * math.sin(theta), -math.cos(theta), math.cos(phi) * math.sin(theta)])
    assert (np.abs(direction) > 0.2).all() and direction[1] > 0.0


IMAGE_PARAMS = [(c.id, image) for c in CASES.values() if not c.ggx for image in c.images]


@pytest.mark.parametrize("case_id,image", IMAGE_PARAMS)
def test_oracle_image_equals_its_reference(orc, case_id, image):
    case = CASES[case_id]
    halves = oracle_halves(orc, case, image)
    R, bias, sigma = D.statistic(halves, case.reference(image))
    gap = f"  discretisation of miss 2 {case.discretisation():+.5f}" if case.miss == 2 else ""
    print("\n" + D.row(case_id, image, case.n[image], R, bias, sigma, gap))
    if (case_id, image) in D.EXACT:  # no variance: compared with the exact value, see direct_light.exact_bound
        dropped, worst = D.check_exact(halves[2], D.EXACT[(case_id, image)], 2 * case.n[image])
        print(f"direct-light {case_id} {image}: every sample is the same number; {dropped} samples dropped, worst pixel {worst:.3e} of bound {D.exact_bound(2 * case.n[image]):.3e}")
        return
    assert D.BIAS_SIGMAS * sigma <= D.BIAS_POWER, "too few samples for the bias bound to mean anything: raise this case's n"
    assert R <= D.R_BOUND, "block means differ from the closed form by more than their noise"
    assert abs(bias) <= D.BIAS_SIGMAS * sigma


CONTROL_PARAMS = [(case_id, name, image) for case_id, controls in D.CONTROLS.items() for name, _, images in controls for image in images]


@pytest.mark.parametrize("case_id,name,image", CONTROL_PARAMS)
def test_negative_control_is_rejected(orc, case_id, name, image):
    case = CASES[case_id]
    control = next(c for n, c, _ in D.CONTROLS[case_id] if n == name)
    R, bias, sigma = D.statistic(oracle_halves(orc, case, image), case.reference(image, control))
    print("\n" + D.row(case_id, image, case.n[image], R, bias, sigma, f"  control: {name}"))
    assert not D.accepted(R, bias, sigma), "a reference that is wrong by little passes: too few samples or too coarse blocks"


def test_oracle_ggx_receiver_nee_on_and_off_agree(orc):
    """G1: no closed form; the two estimators must agree within their noise - once the light half is given back what the
    reference takes from it. The reference samples a light only where the BSDF sampler returned a direction
    (direct_light.ggx_sample_success), so NEE on is (P * light half + BSDF half) and NEE off (light half + BSDF half). The
    (1, 1) image is P * light half, hence  sum + (1 - P) / P * light  estimates what NEE off does. Measured on the oracle:
    uncorrected, NEE on is 7.5 % below NEE off at this view (P is 0.79 to 0.94 over the frame); corrected, see the row printed."""
    case = CASES["G1"]
    light, both, off = (oracle_halves(orc, case, image) for image in ("light", "sum", "off"))
    R, bias, sigma = D.ggx_statistic(both, off)
    print("\n" + D.row("G1", "raw", f"{case.n['sum']}/{case.n['off']}", R, bias, sigma, "  NEE on / off as rendered: the reference's dropped light samples"))
    P = case.ggx_success()
    print(f"direct-light G1: BSDF sample succeeds with probability {P.min():.4f} .. {P.max():.4f}, mean {P.mean():.4f}")
    k = ((1.0 - P) / P)[..., None]
    on = tuple(b[..., :3] + k * l[..., :3] for b, l in zip(both, light))
    R, bias, sigma = D.ggx_statistic(on, off)
    print(D.row("G1", "on/off", f"{case.n['sum']}/{case.n['off']}", R, bias, sigma))
    assert off[2][..., :3].max() > 0.5, "the brute-force image found the light"
    assert D.BIAS_SIGMAS * sigma <= D.BIAS_POWER
    assert R <= D.R_BOUND_GGX
    assert abs(bias) <= D.BIAS_SIGMAS * sigma
