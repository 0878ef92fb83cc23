"""-m gpu: direct lighting against closed-form irradiance on the HIP path. The cases, the float64 references and the statistic are
those of tests/direct_light.py, at the iteration counts tests/test_direct_light_host.py runs on the oracle; the bounds are the same
(R <= R_BOUND, |bias| <= 4 sigma, 4 sigma <= 0.01). Device and oracle agree bit for bit, so the figures printed here should repeat
the host test's digit for digit (profiles/r17_direct_light.md holds both columns).

In addition every image's first 2 iterations are compared with the oracle's bit for bit: the scenes have what no other parity test
has - a receiver scaled differently per axis, an occluder behind a light, two area lights, `miss 2` with pathLengths (1, 1)."""
import numpy as np
import pytest

import direct_light as D
import shading_fuzz as F

pytestmark = pytest.mark.gpu

CASES = D.make_cases()
IMAGE_PARAMS = [(c.id, image) for c in CASES.values() for image in c.images]
_runs = {}


def device_halves(twk, case, image):
    """(two_halves of one image of one case, the image after its first 2 iterations), rendered once per session."""
    key = (case.id, image)
    if key not in _runs:
        dev = twk.Device(ordinal=0, miss=case.scene.miss)
        try:
            D.feed(dev, case.scene, case.state(image))
            dev.setShaderVariant(case.variant)
            dev.setNextEventEstimation(case.nee(image))
            assert dev.streamLayout() == case.scene.predicted_layout
            snapshot = {}
            halves = D.render_halves(dev.render, dev.getOutputBufferHost, case.n[image], snapshot)
        finally:
            dev.close()
        _runs[key] = (halves, snapshot["two"])
    return _runs[key]


@pytest.mark.parametrize("case_id,image", IMAGE_PARAMS)
def test_first_two_iterations_equal_the_oracle(twk, orc, case_id, image):
    case = CASES[case_id]
    _, got = device_halves(twk, case, image)
    _, want, _ = F.render_oracle(orc, case.scene, case.state(image), 2, case.variant, case.nee(image))
    bad = F.mismatch(got, want)
    assert bad is None, f"{case_id} {image}: {bad}"
    assert np.isfinite(want).all() and want[..., :3].max() > 0.0


@pytest.mark.parametrize("case_id,image", [p for p in IMAGE_PARAMS if not CASES[p[0]].ggx])
def test_device_image_equals_its_reference(twk, case_id, image):
    case = CASES[case_id]
    halves, _ = device_halves(twk, case, image)
    R, bias, sigma = D.statistic(halves, case.reference(image))
    print("\n" + D.row(case_id, image, case.n[image], R, bias, sigma))
    if (case_id, image) in D.EXACT:  # no variance: compared with the exact value, see direct_light.exact_bound
        dropped, worst = D.check_exact(halves[2], D.EXACT[(case_id, image)], 2 * case.n[image])
        print(f"direct-light {case_id} {image}: every sample is the same number; {dropped} samples dropped, worst pixel {worst:.3e} of bound {D.exact_bound(2 * case.n[image]):.3e}")
        return
    assert D.BIAS_SIGMAS * sigma <= D.BIAS_POWER
    assert R <= D.R_BOUND, "block means differ from the closed form by more than their noise"
    assert abs(bias) <= D.BIAS_SIGMAS * sigma


def test_device_ggx_receiver_nee_on_and_off_agree(twk):
    """G1 as tests/test_direct_light_host.py states it: sum + (1 - P) / P * light against NEE off, P the probability that the
    reference's GGX sampler returns a direction. This puts evalBsdf's GGX branch and its pdf through the MIS weights on the device."""
    case = CASES["G1"]
    light, both, off = (device_halves(twk, case, image)[0] for image in ("light", "sum", "off"))
    R, bias, sigma = D.ggx_statistic(both, off)
    print("\n" + D.row("G1", "raw", f"{case.n['sum']}/{case.n['off']}", R, bias, sigma))
    P = case.ggx_success()
    k = ((1.0 - P) / P)[..., None]
    on = tuple(b[..., :3] + k * l[..., :3] for b, l in zip(both, light))
    R, bias, sigma = D.ggx_statistic(on, off)
    print(D.row("G1", "on/off", f"{case.n['sum']}/{case.n['off']}", R, bias, sigma))
    assert off[2][..., :3].max() > 0.5, "the brute-force image found the light"
    assert D.BIAS_SIGMAS * sigma <= D.BIAS_POWER
    assert R <= D.R_BOUND_GGX
    assert abs(bias) <= D.BIAS_SIGMAS * sigma
