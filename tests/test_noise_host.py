"""The noise estimate (twk_estimate_noise, csrc/noise_device.h) where it needs no GPU: the new entry points refuse a NULL handle
before any HIP call, the host-only helpers (merge, mean, quantile) equal tests/noise_restate.py, the estimator estimates what it
claims to on data of a known distribution, and the system description's `targetNoise*` keys are read, reported, dropped when
invalid and written back only when they differ from off / the defaults."""
import ctypes as C

import numpy as np
import pytest

import noise_restate as nr
from conftest import scene_path
from test_moments_host import welford

F = np.float32


@pytest.mark.parametrize("name,args", [
    ("twk_estimate_noise", (None, None, 0, None)),
    ("twk_read_noise", (None,)),
    ("twk_app_get_target_noise", (None, None, None, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    rc = getattr(L.lib, name)(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_parameters_are_refused_before_any_device_call(twk):
    L = twk._lib
    handle = C.c_void_p(1)  # never dereferenced: the parameters are checked first
    for bad in (L.Noise(minSamples=1), L.Noise(minSamples=0), L.Noise(darkFloor=0.0), L.Noise(darkFloor=-1.0),
                L.Noise(darkFloor=float("inf")), L.Noise(darkFloor=float("nan"))):
        assert L.lib.twk_estimate_noise(handle, C.byref(bad), None, C.c_size_t(0), None) == L.TWK_ERROR_INVALID_VALUE
        assert "twk_estimate_noise" in L.lib.twk_last_error().decode()
    moments = C.c_void_p(4096)
    for n in (0, (1 << 31) + 1):  # explicit moments: 1 .. 2^31 elements
        assert L.lib.twk_estimate_noise(handle, None, moments, C.c_size_t(n), None) == L.TWK_ERROR_INVALID_VALUE
    assert L.lib.twk_estimate_noise(handle, None, None, C.c_size_t(5), None) == L.TWK_ERROR_INVALID_VALUE  # a count without a buffer


def test_defaults(twk):
    L = twk._lib
    np_ = L.Noise(minSamples=99, darkFloor=7.0)
    L.check(L.lib.twk_noise_defaults(C.byref(np_)))
    assert np_.minSamples == L.TWK_DENOISER_MIN_SAMPLES == 4 and F(np_.darkFloor) == F(0.01) == F(L.TWK_NOISE_DARK_FLOOR)
    assert L.lib.twk_noise_defaults(None) == L.TWK_ERROR_INVALID_VALUE and "twk_noise_defaults" in L.lib.twk_last_error().decode()
    fresh = L.Noise()
    assert (fresh.minSamples, F(fresh.darkFloor)) == (np_.minSamples, F(np_.darkFloor))
    assert C.sizeof(L.NoiseSummary) == 4 * 8 + 2 * 4 + 256 * 4 and C.sizeof(L.Noise) == 8


def _random_summary(L, rng, valid_matches=True):
    """A summary as a device could produce it (valid = the histogram's sum), or with arbitrary words."""
    s = L.NoiseSummary()
    hist = rng.integers(0, 1 << 20, 256, dtype=np.uint64) * (rng.random(256) < rng.uniform(0.02, 1.0))
    for b in range(256):
        s.bins[b] = int(hist[b])
    s.valid = int(hist.sum()) if valid_matches else int(rng.integers(1, 1 << 40))
    s.unknown, s.empty = int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 30))
    s.sumFixed = int(rng.integers(0, 1 << 62))
    s.maxErrorBits = int(rng.integers(0, 0x7f800000))
    return s


def test_host_helpers_equal_the_restatement(twk):
    L = twk._lib
    rng = np.random.default_rng(7)
    qs = [1.0, 0.95, 0.5, 0.25, 1e-3, float(np.nextafter(F(0), F(1))), float(np.nextafter(F(1), F(0))), 2.0 ** -24, 1.0 / 3.0]
    for trial in range(40):
        a, b = _random_summary(L, rng, trial % 4 != 3), _random_summary(L, rng)
        da, db = nr.as_dict(a), nr.as_dict(b)
        if da["valid"]:
            assert F(a.mean) == nr.mean(da)
            for q in qs + list(rng.random(4)):
                assert F(a.quantile(q)) == nr.quantile(da, q), (trial, q)
        assert a.merge(b) is a
        assert nr.same(nr.as_dict(a), nr.merge(da, db))
    # the ceiling is exact where a product in double is not: 2^-52 x (2^53 + 1) = 2 + 2^-52 needs 3 elements, a double says 2
    s = L.NoiseSummary()
    s.valid, s.bins[0], s.bins[1] = (1 << 53) + 1, 2, 1
    assert F(s.quantile(2.0 ** -52)) == nr.quantile(nr.as_dict(s), 2.0 ** -52) == nr.bin_upper_edge(1)
    assert F(s.quantile(2.0 ** -53)) == nr.quantile(nr.as_dict(s), 2.0 ** -53) == nr.bin_upper_edge(0)
    assert F(s.quantile(1.0)) == nr.quantile(nr.as_dict(s), 1.0) == nr.bin_upper_edge(255)  # never reached: the last edge


def test_bad_quantiles_and_empty_summaries_are_refused(twk):
    L = twk._lib
    s = _random_summary(L, np.random.default_rng(3))
    for q in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        with pytest.raises(twk.TwkError) as e:
            s.quantile(q)
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_noise_quantile" in str(e.value)
    empty = L.NoiseSummary()
    empty.unknown, empty.empty = 5, 9
    for call in (lambda: empty.quantile(0.5), lambda: empty.mean):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == L.TWK_ERROR_INVALID_STATE
    assert empty.maxError == 0.0 and not empty.histogram.any()
    out = C.c_float(0)
    assert L.lib.twk_noise_quantile(None, C.c_float(0.5), C.byref(out)) == L.TWK_ERROR_INVALID_VALUE
    assert L.lib.twk_noise_mean(None, C.byref(out)) == L.TWK_ERROR_INVALID_VALUE
    assert L.lib.twk_noise_merge(None, C.byref(empty)) == L.TWK_ERROR_INVALID_VALUE
    assert L.lib.twk_noise_merge(C.byref(empty), None) == L.TWK_ERROR_INVALID_VALUE


def test_restated_classes_and_bins():
    """The restatement's own rules on hand-made triples: the order of the tests, the bin of a power of two, both clamps."""
    nan, inf = float("nan"), float("inf")
    m = np.array([[1, 1, 0, 0], [nan, 1, 0, 0], [1, 1, -0.0, 0],        # n == 0 comes first: empty whatever else holds
                  [1, 1, 3, 0], [1, 1, nan, 0], [nan, 1, 8, 0], [1, inf, 8, 0], [1, 1, inf, 0], [1, -1, 8, 0], [-1, 1, 8, 0], [1, 1, -4, 0],
                  [1, 0, 4, 0], [0.99, 12, 4, 0], [0, 0, 4, 0], [0.99, -0.0, 4, 0]], F)
    cls, e = nr.classify(m)
    assert cls.tolist() == [nr.EMPTY] * 3 + [nr.UNKNOWN] * 8 + [nr.VALID] * 4
    assert e[11] == 0 and e[12] == F(1.0) and e[13] == 0 and e[14].view(np.uint32) == 0   # sqrt(12 / 12) / (0.99 + 0.01)
    assert nr.classify(m, min_samples=3)[0][3] == nr.VALID
    octaves = np.array([2.0 ** k for k in range(-20, 21)], F)
    assert nr.bins(octaves).tolist() == [min(255, max(0, 8 * (k + 16))) for k in range(-20, 21)]
    assert nr.bins(np.array([1.0, 1.124, 1.125, 1.9999], F)).tolist() == [128, 128, 129, 135]
    assert nr.fixed(np.array([0, 2.0 ** -21, 2.0 ** -20, 1.5, 65536, 1e9], F)).tolist() == [0, 0, 1, 3 << 19, 1 << 36, 1 << 36]
    assert nr.bin_upper_edge(128) == F(1.125) and nr.bin_upper_edge(255) == F(2.0 ** 16) and nr.bin_upper_edge(0) == F(2.0 ** -16 * 1.125)
    s, emap = nr.summary(m)
    assert (s["valid"], s["unknown"], s["empty"]) == (4, 8, 3) and s["histogram"][0] == 3 and s["histogram"][128] == 1
    assert s["sumFixed"] == 1 << 20 and s["maxErrorBits"] == 0x3f800000
    assert emap.tolist() == [-2.0] * 3 + [-1.0] * 8 + [0.0, 1.0, 0.0, 0.0]


def test_the_estimator_estimates_the_relative_standard_error():
    """4096 pixels of 64 exponential samples with mean 1: the standard deviation is 1, so the standard error of a pixel's mean is
    1 / sqrt(64) and e = that / (mean + 0.01), about 1 / (8 x 1.01). The sample standard deviation of an exponential is biased low
    at 64 samples (1.8 % low in a numpy check when the bound was set; 5.5 % at 16 samples): within 5 %. And the quantile the
    histogram gives is the upper edge of the bin that holds the true one: in (Q, 9/8 Q]."""
    rng = np.random.default_rng(1)
    lum = rng.exponential(1.0, (64, 4096)).astype(F)
    samples = np.ones((64, 4096, 4), F)
    samples[..., :3] = lum[..., None]  # grey: the luminance is the value, up to the rounding of the weights' sum
    moments = welford(samples, 0, np.zeros((4096, 4), F))
    assert (moments[:, 2] == 64).all()
    s, _ = nr.summary(moments)
    assert s["valid"] == 4096 and s["unknown"] == 0 and s["empty"] == 0
    cls, e = nr.classify(moments)
    expected = 1.0 / (np.sqrt(64.0) * 1.01)
    got = float(nr.mean(s))
    print(f"\nmean e {got:.6f}, expected {expected:.6f}: {100 * (got / expected - 1):+.2f} %")
    assert abs(got - float(e.astype(np.float64).mean())) < 2.0 ** -20  # the fixed point rounds each e by at most 2^-21
    assert abs(got / expected - 1) < 0.05
    Q = float(np.quantile(e, 0.95))
    edge = float(nr.quantile(s, 0.95))
    print(f"0.95 quantile: edge {edge:.6f}, true {Q:.6f}")
    assert Q < edge <= 9 / 8 * Q


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        return app.targetNoise, app.systemDescription()
    finally:
        app.close()


def test_target_noise_keys_of_the_system_description(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    defaults = (False, 0.0, F(0.95), 16)
    strip = lambda t: (t[0], F(t[1]), F(t[2]), t[3])
    off, text = _description(twk, base)
    assert strip(off) == defaults
    assert "targetNoise" not in text
    assert _description(twk, text) == (off, text)  # a description without the keys writes back the text it wrote before
    assert _description(twk, base + "\ntargetNoise 0\ntargetNoiseQuantile 0.95\ntargetNoiseInterval 16\n") == (off, text)
    older = _description(twk, base + "\ndenoiser 3\ndenoiserSampledVariance 1\ndenoiserMinSamples 16\n")[1]
    assert "targetNoise" not in older and _description(twk, older)[1] == older

    on, on_text = _description(twk, base + "\ntargetNoise 0.125\n")
    assert strip(on) == (True, F(0.125), F(0.95), 16)
    assert on_text.replace("targetNoise 0.125\n", "") == text
    assert _description(twk, on_text) == (on, on_text)

    custom, custom_text = _description(twk, base + "\ntargetNoise 0.0625\ntargetNoiseQuantile 0.5\ntargetNoiseInterval 4\n")
    assert strip(custom) == (True, F(0.0625), F(0.5), 4)
    for line in ("targetNoise 0.0625\n", "targetNoiseQuantile 0.5\n", "targetNoiseInterval 4\n"):
        assert custom_text.count(line) == 1
    assert _description(twk, custom_text) == (custom, custom_text)
    # a value the calls would refuse drops the line, the previous value stays
    assert strip(_description(twk, base + "\ntargetNoise 0.25\ntargetNoise -1\n")[0]) == (True, F(0.25), F(0.95), 16)
    assert strip(_description(twk, base + "\ntargetNoise 1e39\n")[0]) == defaults  # not finite as a float
    assert strip(_description(twk, base + "\ntargetNoiseQuantile 0\n")[0]) == defaults
    assert strip(_description(twk, base + "\ntargetNoiseQuantile 0.5\ntargetNoiseQuantile 1.5\n")[0]) == (False, 0.0, F(0.5), 16)
    assert strip(_description(twk, base + "\ntargetNoiseQuantile 1\n")[0]) == (False, 0.0, F(1.0), 16)
    assert strip(_description(twk, base + "\ntargetNoiseInterval 0\n")[0]) == defaults
    assert strip(_description(twk, base + "\ntargetNoiseInterval 8\ntargetNoiseInterval -2\n")[0]) == (False, 0.0, F(0.95), 8)
    # settings kept beside a target that is off
    kept, kept_text = _description(twk, base + "\ntargetNoiseInterval 32\n")
    assert strip(kept) == (False, 0.0, F(0.95), 32) and "targetNoiseInterval 32\n" in kept_text and "targetNoise " not in kept_text
