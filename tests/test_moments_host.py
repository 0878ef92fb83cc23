"""The luminance moments of the integrator's samples (twk_enable_moments) and the mode of the denoiser they feed
(twk_denoise_variance_sampled), where they need no GPU: the new entry points refuse a NULL handle before any HIP call, the system
description's keys `denoiserSampledVariance` and `denoiserMinSamples` are read, reported and written back only when they differ
from off / the default, and the f32 Welford recurrence that csrc/shade_device.h foldSamples states is accurate.

`fold_mean` and `welford` below are that header's per-sample fold again in numpy float32, statement for statement;
tests/test_gpu_moments.py feeds them the device's own samples and compares bits."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

F = np.float32
U = 2.0 ** -24  # unit roundoff of f32, round to nearest


def luminance(rgb):
    """device_math.h luminance3, in its order."""
    return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def kept_radiance(sample, debug_exceptions):
    """(radiance [..., 3], keep [...]) of raw samples [..., 4] as foldSamples takes them: w == 0 is no sample; NaN samples are
    dropped, or every sample is kept with its false colour (NaN red, inf green, negative blue) under debugExceptions."""
    s = np.ascontiguousarray(sample, F)
    rgb = s[..., :3].copy()
    nan = np.isnan(rgb).any(axis=-1)
    keep = ~nan
    if debug_exceptions:
        inf = ~nan & np.isinf(rgb).any(axis=-1)
        neg = ~nan & ~inf & (rgb < 0).any(axis=-1)
        rgb[nan], rgb[inf], rgb[neg] = (F(1000000.0), 0, 0), (0, F(1000000.0), 0), (0, 0, F(1000000.0))
        keep = np.ones_like(nan)
    return rgb, keep & (s[..., 3] != 0)


def fold_mean(samples, first_iteration, dst, debug_exceptions=False):
    """foldSamples' running mean over samples [S, ..., 4] (iterations first_iteration ...), on dst [..., 4] f32; returns the new dst."""
    dst = np.array(dst, F)
    with np.errstate(all="ignore"):
        for s, sample in enumerate(samples):
            rgb, keep = kept_radiance(sample, debug_exceptions)
            iteration = first_iteration + s
            if iteration > 0:
                t = F(1.0) / F(iteration + 1)
                rgb = dst[..., :3] + t * (rgb - dst[..., :3])  # lerp(dst, radiance, t) = a + t * (b - a)
            new = np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,), F)], axis=-1).astype(F)
            dst = np.where(keep[..., None], new, dst)
    return dst


def welford(samples, first_iteration, triple, debug_exceptions=False):
    """foldSamples' MOMENTS fold over samples [S, ..., 4] on triple [..., 4] = (mean, M2, n, 0); returns the new triple."""
    m = np.array(triple, F)
    with np.errstate(all="ignore"):
        for s, sample in enumerate(samples):
            rgb, keep = kept_radiance(sample, debug_exceptions)
            l = luminance(rgb)
            mean, m2, n = (m[..., 0], m[..., 1], m[..., 2]) if first_iteration + s > 0 else (np.zeros_like(l),) * 3
            n1 = n + F(1.0)
            d = l - mean
            mean1 = mean + d / n1
            m21 = m2 + d * (l - mean1)
            new = np.stack([mean1, m21, n1, m[..., 3]], axis=-1).astype(F)
            m = np.where(keep[..., None], new, m)
    assert m.dtype == F
    return m


@pytest.mark.parametrize("name,args", [
    ("twk_enable_moments", (1,)),
    ("twk_read_moments", (None, 0)),
    ("twk_get_moments_device_pointer", (None, None)),
    ("twk_debug_read_path_radiance", (None, 0)),
    ("twk_denoise_variance_sampled", (None, None, 4, None, None, None, None, 0, 0, None)),
    ("twk_app_get_denoiser_sampled", (None, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    rc = getattr(L.lib, name)(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_abi_version_and_default_min_samples(twk):
    import os
    import re
    from conftest import ROOT
    L = twk._lib
    header = open(os.path.join(ROOT, "include", "tweeker_hip.h")).read()
    assert "#define TWK_ABI_VERSION 9" in header and L.lib.twk_abi_version() == 9
    assert int(re.search(r"#define TWK_DENOISER_MIN_SAMPLES (\d+)", header).group(1)) == L.TWK_DENOISER_MIN_SAMPLES >= 2


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        return app.denoiserSampled, app.systemDescription()
    finally:
        app.close()


def test_sampled_keys_of_the_system_description(twk):
    """The description text already carries the denoiser* keys (tests/test_denoise_variance_host.py), so the new ones round-trip
    through it, written only when they differ from off / the default: older texts keep their text."""
    default = twk._lib.TWK_DENOISER_MIN_SAMPLES
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    off, text = _description(twk, base)
    assert off == (False, default)
    assert "denoiserSampledVariance" not in text and "denoiserMinSamples" not in text
    assert _description(twk, text) == (off, text)
    assert _description(twk, base + f"\ndenoiserSampledVariance 0\ndenoiserMinSamples {default}\n") == (off, text)
    older = _description(twk, base + "\ndenoiser 3\ndenoiserVariance 1\ndenoiserFirefly 2.5\n")[1]
    assert "denoiserSampledVariance" not in older and "denoiserMinSamples" not in older and _description(twk, older)[1] == older

    on, on_text = _description(twk, base + "\ndenoiser 3\ndenoiserSampledVariance 1\n")
    assert on == (True, default)
    assert on_text.replace("denoiserSampledVariance 1\n", "").replace("denoiser 3\n", "") == text
    assert _description(twk, on_text) == (on, on_text)

    custom, custom_text = _description(twk, base + "\ndenoiser 3\ndenoiserSampledVariance 1\ndenoiserMinSamples 16\n")
    assert custom == (True, 16)
    for line in ("denoiserSampledVariance 1\n", "denoiserMinSamples 16\n"):
        assert custom_text.count(line) == 1
    assert _description(twk, custom_text) == (custom, custom_text)
    # the switch is 0 or 1; a count twk_denoise_variance_sampled would refuse drops the line, the previous value stays
    assert _description(twk, base + "\ndenoiserSampledVariance 7\n")[0][0] is False
    assert _description(twk, base + "\ndenoiserMinSamples 8\ndenoiserMinSamples 1\n")[0] == (False, 8)
    assert _description(twk, base + "\ndenoiserMinSamples 0\n")[0] == (False, default)
    # a setting kept beside a switch that is off
    kept, kept_text = _description(twk, base + "\ndenoiserMinSamples 2\n")
    assert kept == (False, 2) and "denoiserMinSamples 2\n" in kept_text and "denoiserSampledVariance" not in kept_text


def test_min_samples_below_two_is_refused_before_any_device_call(twk):
    L = twk._lib
    dn, dv = L.Denoiser(), L.DenoiserVariance()
    handle = C.c_void_p(1)  # never dereferenced: the count is checked first
    for n in (1, 0, -3):
        rc = L.lib.twk_denoise_variance_sampled(handle, C.byref(dn), C.byref(dv), n, None, None, None, None, 0, 0, None)
        assert rc == L.TWK_ERROR_INVALID_VALUE and "minSamples" in L.lib.twk_last_error().decode()


@pytest.mark.parametrize("n", [2, 7, 64])
@pytest.mark.parametrize("data", ["uniform", "offset", "fireflies"])
def test_f32_welford_against_a_float64_two_pass(n, data):
    """welford() against mean and sum of squared deviations computed in float64 in two passes over the same f32 luminances
    (error ~2^-53 relative: nothing beside f32's). The bound, from the roundings of the recurrence, u = 2^-24, R = max |l|:

    mean. One step computes fl(mean + fl(fl(l - mean) / n)). Two roundings on the increment, |l - mean| <= 2R: <= 2u 2R / j at
    step j; one on the sum: <= u R. An error e of the mean before step j is carried as e (1 - 1/j), so a local error of step j
    reaches the end scaled by j / n:  |mean - exact| <= sum_j (j / n) (4 u R / j + u R) = u R (4 + (n + 1) / 2) =: D.

    M2. The exact recurrence adds T_j = (l - mean_{j-1}) (l - mean_j). The computed term uses means that are off by <= D each
    (factors of size <= 2R: <= 2R D + 2R D), and rounds both differences and the product (3 u |T_j| <= 12 u R^2); the n
    additions of non-negative terms round by at most u M2 each. So
        |M2 - exact| <= n (4 R D + 12 u R^2) + n u M2,
    to first order in u; the factor 1.01 covers the terms of order u^2 (n u <= 4e-6). Nothing here was fitted to the result."""
    rng = np.random.default_rng(n * 31 + len(data))
    pixels = 4096
    if data == "uniform":
        rgb = rng.uniform(0.0, 1.0, (n, pixels, 3))
    elif data == "offset":  # ill-conditioned: mean 100, deviation 0.01
        rgb = 100.0 + rng.normal(0.0, 0.01, (n, pixels, 1)) * np.ones(3)
    else:
        rgb = rng.gamma(2.0, 0.5, (n, pixels, 3))
        rgb[rng.random((n, pixels)) < 0.05] *= 1000.0
    samples = np.ones((n, pixels, 4), F)
    samples[..., :3] = rgb.astype(F)
    got = welford(samples, 0, np.zeros((pixels, 4), F)).astype(np.float64)
    l = luminance(samples[..., :3]).astype(np.float64)  # the f32 luminances the recurrence sees
    mean = l.mean(axis=0)
    m2 = ((l - mean) ** 2).sum(axis=0)
    R = np.abs(l).max(axis=0)
    D = U * R * (4 + (n + 1) / 2)
    bound = n * (4 * R * D + 12 * U * R * R) + n * U * m2
    assert (got[:, 2] == n).all() and (got[:, 3] == 0).all()
    assert (np.abs(got[:, 0] - mean) <= 1.01 * D).all()
    err = np.abs(got[:, 1] - m2)
    with np.errstate(invalid="ignore"):  # two samples that coincide: error 0, bound 0
        print(f"\n{data}, n = {n}: max |M2 - exact| / bound = {np.nanmax(err / bound):.3f}, max relative error of M2 {np.nanmax(err / m2):.3e}")
    assert (err <= 1.01 * bound).all()
    assert (got[:, 1] >= 0).all()  # |d / n| <= |d| and rounding is monotone: l - mean' never has the other sign of d
    if data == "uniform":
        assert np.median(bound / m2) < 1e-3  # the bound says something where the data are well conditioned (a pixel whose samples nearly coincide has M2 near 0)


def test_restated_fold_rules():
    """The restatement's own rules on a hand-made pixel row: w == 0 is no sample, NaN is dropped or false-coloured, iteration 0
    starts afresh, a batch equals its iterations one by one."""
    nan, inf = float("nan"), float("inf")
    samples = np.array([[[1, 1, 1, 1], [nan, 0, 0, 1], [2, 2, 2, 0], [inf, 0, 0, 1], [-1, 0, 0, 1]],
                        [[3, 3, 3, 1], [1, 1, 1, 1], [2, 2, 2, 0], [1, 1, 1, 1], [1, 1, 1, 1]]], F)
    stale = np.full((5, 4), 7.0, F)
    m = welford(samples, 0, stale)
    # pixel 1: its NaN sample of iteration 0 is dropped, so nothing started afresh there: the stale n = 7 went on to 8
    assert m[:, 2].tolist() == [2, 8, 7, 2, 2] and (m[:, 3] == 7).all()
    assert np.array_equal(m[2], stale[2])                  # never a sample: untouched
    assert abs(float(m[0, 0]) - 2.0) < 1e-6 and abs(float(m[0, 1]) - 2.0) < 1e-5  # l = 1, 3: mean 2, M2 = 1 + 1
    assert not np.isfinite(m[3, :2]).any()                 # an infinite sample is kept and makes the triple not finite
    one_by_one = welford(samples[1:], 1, welford(samples[:1], 0, stale))
    assert np.array_equal(m.view(np.uint32), one_by_one.view(np.uint32))
    dbg = welford(samples, 0, stale, debug_exceptions=True)
    assert dbg[:, 2].tolist() == [2, 2, 7, 2, 2]           # every sample counts, in its false colour
    red, green, blue = (float(luminance(np.array(c, F))) for c in ((1e6, 0, 0), (0, 1e6, 0), (0, 0, 1e6)))
    one = float(luminance(np.ones(3, F)))
    for pixel, colour in ((1, red), (3, green), (4, blue)):
        assert abs(float(dbg[pixel, 0]) - (colour + one) / 2) <= 1e-6 * colour
    mean = fold_mean(samples, 0, stale)
    assert mean[0].tolist() == [2.0, 2.0, 2.0, 1.0] and mean[1].tolist() == [4.0, 4.0, 4.0, 1.0] and mean[2].tolist() == [7.0] * 4
