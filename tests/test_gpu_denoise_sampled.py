"""-m gpu: twk_denoise_variance_sampled — the variance-guided mode of the a-trous filter with the MEASURED variance of a pixel's
mean (from the luminance moments the accumulate kernels fold, twk_enable_moments) in place of the spatial estimate wherever the
pixel has seen at least minSamples samples; SVGF's fallback rule (Schied et al. 2017, section 4.2) the other way round.

csrc/denoise_device.h defines it operation by operation. `restate_sampled` is tests/test_gpu_denoise_variance.py restate_variance
with the one step the SAMPLED moments pass adds, in numpy float32: the device result must equal it in every bit, alpha included,
in both output formats. (tools/denoise_sampled_sweep.py runs the same restatement on the oracle's renders; it needs no GPU.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_app, scene_path
from test_gpu_denoise import BUILDS, CASES, H5, _assert_same_bits, _bits, _choose_build, _dist2, _errors, _exp, _finite3, _own_buffers
from test_gpu_denoise_variance import B3, EPSILON, RADIUS, _lum, _small_device, _sqrt, _taps, _upload, restate_variance
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
HALF = 1


def restate_sampled(beauty, albedo, normal, moments, min_samples, dn, dv, exp, sqrt, info=None):
    """restate_variance with the sampled variance (csrc/denoise_device.h, "the sampled variance"). moments: float32 [H, W, 4] =
    (mean, M2, n, .). Same returns; info (a dict) receives the masks `sampled` (pixels whose variance is the measured one) and
    `clamped` (pixels the firefly clamp scaled)."""
    b = np.ascontiguousarray(beauty, F)
    if dn.iterations == 0 or dn.blendFactor == 1.0:
        return b.copy(), np.ones(b.shape[:2], bool)
    kind, demod = dn.inputKind, bool(dn.demodulateAlbedo)
    inv_normal = F(1.0) / (F(dn.sigmaNormal) * F(dn.sigmaNormal)) if kind >= 2 else F(0)
    inv_albedo = F(1.0) / (F(dn.sigmaAlbedo) * F(dn.sigmaAlbedo)) if kind >= 1 else F(0)
    blend, firefly, sigma_l = F(dn.blendFactor), F(dv.fireflyThreshold), F(dv.sigmaLuminance)
    height, width = b.shape[:2]
    sq = lambda v: sqrt(np.ascontiguousarray(v, F)).reshape(v.shape)
    with np.errstate(all="ignore"):
        # prepare
        c = b.copy()
        guides_finite = np.ones(b.shape[:2], bool)
        if kind >= 2:
            guides_finite &= _finite3(normal)
        if kind >= 1:
            guides_finite &= _finite3(albedo)
        if demod:
            d = np.fmax(albedo[..., :3].astype(F), F(0.01))
            c[..., :3] = b[..., :3] / d
        # moments pass: the spatial estimate and the clamp, as in restate_variance
        lum, fin = _lum(c), _finite3(c)
        s0, s1, s2 = (np.zeros((height, width), F) for _ in range(3))
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                pq = _taps(height, width, dx, dy, 1)
                if (dx == 0 and dy == 0) or pq is None:
                    continue
                P, Q = pq
                ok = fin[Q]
                g = np.ones(ok.shape, F)
                if kind >= 1:
                    t = _dist2(albedo[P], albedo[Q]) * inv_albedo
                    if kind >= 2:
                        t = _dist2(normal[P], normal[Q]) * inv_normal + t
                    ok = ok & (t <= F(87.0))
                    g = exp(np.where(ok, -t, F(0)).astype(F)).reshape(t.shape)
                lq = lum[Q]
                s0[P] = s0[P] + np.where(ok, g, F(0))
                s1[P] = s1[P] + np.where(ok, g * lq, F(0))
                s2[P] = s2[P] + np.where(ok, g * (lq * lq), F(0))
        reaches = fin & np.isfinite(lum) & guides_finite  # the pixels that get past the early (cp.xyz, 0)
        estimated = reaches & (s0 > 0)
        m1, m2 = s1 / s0, s2 / s0
        var = np.fmax(m2 - m1 * m1, F(0))
        out = np.concatenate([c[..., :3], np.where(estimated, var, F(0))[..., None]], axis=-1).astype(F)
        f = np.ones((height, width), F)
        clamp = np.zeros((height, width), bool)
        if firefly > 0:
            limit = m1 + firefly * sq(var)
            clamp = estimated & (lum > limit) & (limit > 0)
            f = np.where(clamp, limit / lum, F(1.0)).astype(F)
            out[clamp, :3] = (c[..., :3] * f[..., None])[clamp]
        # ... and the measured variance of the pixel's mean where the pixel has seen enough samples
        mean, big_m2, n = (np.ascontiguousarray(moments[..., k], F) for k in range(3))
        sampled = reaches & (n >= F(min_samples)) & np.isfinite(mean) & np.isfinite(big_m2) & np.isfinite(n) & (mean > 0)
        v = big_m2 / ((n - F(1.0)) * n)
        if demod:
            rho = lum / mean  # lum: of the demodulated colour before the clamp
            v = v * (rho * rho)
        v = v * (f * f)
        out[sampled, 3] = v[sampled]
        if info is not None:
            info["sampled"], info["clamped"] = sampled, clamp
        c = out
        # levels, as in restate_variance
        for level in range(dn.iterations):
            s = 1 << level
            lum, fin = _lum(c), _finite3(c)
            fin_v = fin & np.isfinite(c[..., 3])
            vs, bs = np.zeros((height, width), F), np.zeros((height, width), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    pq = _taps(height, width, dx, dy, s)
                    if pq is None:
                        continue
                    P, Q = pq
                    k = B3[dy + 1] * B3[dx + 1]
                    vs[P] = vs[P] + np.where(fin_v[Q], k * c[Q][..., 3], F(0))
                    bs[P] = bs[P] + np.where(fin_v[Q], k, F(0))
            vbar = np.where(bs > 0, vs / bs, F(0)).astype(F)
            inv_l = F(1.0) / (sigma_l * sq(vbar) + EPSILON)
            total = np.zeros((height, width, 3), F)
            wsum, vsum = np.zeros((height, width), F), np.zeros((height, width), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _taps(height, width, dx, dy, s)
                    if pq is None:
                        continue
                    P, Q = pq
                    cq = c[Q]
                    t = np.abs(lum[P] - lum[Q]) * inv_l[P]
                    if kind >= 2:
                        t = t + _dist2(normal[P], normal[Q]) * inv_normal
                    if kind >= 1:
                        t = t + _dist2(albedo[P], albedo[Q]) * inv_albedo
                    ok = fin[Q] & (t <= F(87.0))
                    e = exp(np.where(ok, -t, F(0)).astype(F)).reshape(t.shape)
                    w = np.where(ok, (H5[dy + 2] * H5[dx + 2]) * e, F(0))
                    total[P] = total[P] + np.where(ok[..., None], w[..., None] * cq[..., :3], F(0))
                    wsum[P] = wsum[P] + w
                    vsum[P] = vsum[P] + np.where(ok, (w * w) * cq[..., 3], F(0))
            nxt = c.copy()
            centre = fin & guides_finite & np.isfinite(lum)
            nxt[centre, :3] = (total / wsum[..., None])[centre]
            nxt[centre, 3] = (vsum / (wsum * wsum))[centre]
            c = nxt
        # finish
        r = c[..., :3] * d if demod else c[..., :3]
        o = b.copy()
        through = ~(_finite3(b) & guides_finite & np.isfinite(r).all(axis=-1))
        o[~through, :3] = (r + blend * (b[..., :3] - r))[~through]
    assert o.dtype == F
    return o, through


def _expect_sampled(beauty_raw, albedo_raw, normal_raw, moments, min_samples, dn, dv, orc, info=None):
    widen = lambda a: None if a is None else a.astype(F)
    o, through = restate_sampled(widen(beauty_raw), widen(albedo_raw), widen(normal_raw), moments, min_samples, dn, dv, _exp(orc), _sqrt(orc), info)
    if beauty_raw.dtype == np.float16:
        with np.errstate(over="ignore"):
            o = o.astype(np.float16)
        o[through] = beauty_raw[through]
    return o


def _rendered(twk, spp, half=False, res=(61, 37), moments=True):
    """C2 with Optix7Gui's closest-hit rule, AOVs and moments on."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    dev.enableAov(True)
    if moments:
        dev.enableMoments(True)
    if half:
        dev.setOutputFormat(HALF)
    for it in range(spp):
        dev.render(it)
    return dev


@BUILDS
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_render_equals_the_restatement_bit_for_bit(twk, orc, half, lds_max_step, monkeypatch):
    """C2 at 61x37, 6 spp, the handle's own buffers and its own moments: every inputKind x 1 / 3 / 5 levels x demodulation off / on
    with the default border between the level builds (three of them with every level direct, every level staged), minSamples 2 and
    6 (every pixel on the measured side) and 7 (every pixel on the fallback side: twk_denoise_variance's bits)."""
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    spp = 6
    dev = _rendered(twk, spp, half=half)
    beauty, albedo, normal = _own_buffers(dev, half)
    moments = dev.readMoments()
    assert (moments[..., 2] == spp).all()
    cases = CASES if lds_max_step is None else [(2, 5, 1), (1, 3, 0), (0, 3, 0)]
    dv = L.DenoiserVariance()
    for kind, iterations, demod in cases:
        dn = L.Denoiser(inputKind=kind, iterations=iterations, demodulateAlbedo=demod)
        guides = (albedo if kind >= 1 else None, normal if kind >= 2 else None)
        for min_samples in ((2, 7) if (kind, iterations) == (2, 3) else (spp,)):
            info = {}
            dev.denoise(dn, variance=dv, minSamples=min_samples)
            got = dev.readDenoised(raw=True)
            expect = _expect_sampled(beauty, *guides, moments, min_samples, dn, dv, orc, info)
            _assert_same_bits(got, expect, f"kind {kind}, {iterations} levels, demodulate {demod}, minSamples {min_samples}")
            assert (got[..., 3] == 1).all()
            # (a black pixel has mean 0 and stays on the fallback side)
            assert (info["sampled"].mean() > 0.5) if min_samples <= spp else not info["sampled"].any()
        if (kind, iterations) == (2, 3):
            # minSamples 7 was the last: the fallback side everywhere is twk_denoise_variance, and the measured side is not
            dev.denoise(dn, variance=dv)
            spatial = dev.readDenoised(raw=True)
            _assert_same_bits(got, spatial, "every pixel on the fallback side against twk_denoise_variance")
            dev.denoise(dn, variance=dv, moments=True)  # the default minSamples
            assert L.TWK_DENOISER_MIN_SAMPLES <= spp and not np.array_equal(_bits(dev.readDenoised(raw=True)), _bits(spatial))
    after = _own_buffers(dev, half) + (dev.readMoments(),)
    for a, b, name in zip(after, (beauty, albedo, normal, moments), ("beauty", "albedo", "normal", "moments")):
        _assert_same_bits(a, b, f"input {name} after twk_denoise_variance_sampled")
    dev.close()


MIN_SAMPLES = 5


def _synthetic_frame(width, height):
    """Noise over flat guides with fireflies (pixels the clamp scales), and moments that reach both sides of the rule: n = 1,
    minSamples - 1, minSamples and more; mean 0 and below; inf and NaN in each of the three words."""
    rng = np.random.default_rng(width * 1000 + height)
    beauty = rng.gamma(2.0, 0.5, (height, width, 4)).astype(F)
    beauty[rng.random((height, width)) < 0.05, :3] *= F(200.0)
    albedo = np.ones((height, width, 4), F)
    albedo[..., :3] = rng.uniform(0.3, 0.4, (height, width, 3)).astype(F)
    normal = np.zeros((height, width, 4), F)
    normal[..., :3] = (0.0, 0.6, 0.8)
    normal[:, width // 2:, :3] = (0.6, 0.0, 0.8)
    moments = np.zeros((height, width, 4), F)
    moments[..., 0] = _lum(beauty) * rng.uniform(0.8, 1.25, (height, width)).astype(F)
    moments[..., 1] = rng.gamma(2.0, 0.5, (height, width)).astype(F)
    moments[..., 2] = rng.choice(np.array([1, MIN_SAMPLES - 1, MIN_SAMPLES, MIN_SAMPLES + 3, 64], F), (height, width))
    moments[..., 3] = rng.uniform(-1.0, 1.0, (height, width)).astype(F)  # the fourth word is not read
    if width * height == 1:
        moments[..., 2] = MIN_SAMPLES
    flat = moments.reshape(-1, 4)
    if len(flat) >= 15:  # special values, each at a pixel of its own that has enough samples otherwise
        special = rng.choice(len(flat), 15 if len(flat) < 200 else 60, replace=False)
        values = [(0, 0.0), (0, -0.5), (0, np.inf), (0, np.nan), (1, np.inf), (1, np.nan), (2, np.inf), (2, np.nan), (0, -np.inf), (1, 0.0), (2, 1.0), (2, MIN_SAMPLES - 1), (2, MIN_SAMPLES), (1, 3.0e38), (0, 1.0e-30)]
        for i, pixel in enumerate(special):
            flat[pixel, 2] = MIN_SAMPLES + 3
            word, value = values[i % len(values)]
            flat[pixel, word] = value
    return beauty, albedo, normal, moments


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("width,height", [(1, 1), (5, 3), (61, 37)])
def test_explicit_buffers_and_synthetic_moments(twk, orc, width, height, half):
    """Explicit buffers at 1x1 (no window tap: the spatial side has no variance, the measured side has), 5x3 (narrower than the
    halo of the moments pass) and 61x37 (no multiple of the 32x8 tile), in both formats: every inputKind, demodulation off and
    on, clamp on and off. At 61x37 the moments must have reached both sides of the rule, through every reason, and a clamped pixel."""
    L = twk._lib
    beauty, albedo, normal, moments = _synthetic_frame(width, height)
    if half:
        with np.errstate(over="ignore"):
            beauty, albedo, normal = (a.astype(np.float16) for a in (beauty, albedo, normal))
    shape = (height, width)
    dev = _small_device(twk, half)
    buffers = _upload(twk, (beauty, albedo, normal, moments))
    out = _DeviceBuffer(twk, beauty.nbytes)
    pointers = [b.ptr.value for b in buffers]
    for kind, iterations, demod, firefly in ((2, 5, 1, 3.0), (2, 3, 0, 3.0), (1, 1, 1, 1.0), (0, 3, 0, 3.0), (2, 2, 1, 0.0)):
        dn, dv = L.Denoiser(inputKind=kind, iterations=iterations, demodulateAlbedo=demod), L.DenoiserVariance(fireflyThreshold=firefly)
        info = {}
        expect = _expect_sampled(beauty, albedo if kind >= 1 else None, normal if kind >= 2 else None, moments, MIN_SAMPLES, dn, dv, orc, info)
        dev.denoise(dn, *pointers[:3], shape=shape, variance=dv, moments=pointers[3], minSamples=MIN_SAMPLES)
        got = dev.readDenoised(raw=True, shape=shape)
        what = f"{width}x{height}, kind {kind}, {iterations} levels, demodulate {demod}, firefly {firefly}"
        _assert_same_bits(got, expect, what)
        _assert_same_bits(got[..., 3], beauty[..., 3], "alpha")
        dev.denoise(dn, *pointers[:3], shape=shape, denoised=out.ptr.value, variance=dv, moments=pointers[3], minSamples=MIN_SAMPLES)
        dev.synchronizeStream()
        _assert_same_bits(out.download(beauty.shape, beauty.dtype), expect, what + ", the caller's buffer")
        if (width, height) == (61, 37):
            m, s = moments, info["sampled"]
            enough = m[..., 2] >= MIN_SAMPLES
            assert s.sum() > 500 and (~s).sum() > 500
            assert not s[m[..., 2] == MIN_SAMPLES - 1].any() and not s[m[..., 2] == 1].any() and (m[..., 2] == 1).any() and (m[..., 2] == MIN_SAMPLES - 1).any()
            assert s[(m[..., 2] == MIN_SAMPLES) & np.isfinite(m[..., :2]).all(axis=-1) & (m[..., 0] > 0)].all() and ((m[..., 2] == MIN_SAMPLES) & s).any()
            for word in range(3):
                for bad in (np.isinf(m[..., word]), np.isnan(m[..., word])):
                    assert bad.any() and not s[bad].any()
            assert (enough & (m[..., 0] == 0)).any() and not s[m[..., 0] <= 0].any()
            if firefly > 0:
                assert (info["clamped"] & s).any() and (info["clamped"] & ~s).any(), "a pixel the clamp scales, on either side of the rule"
            dev.denoise(dn, *pointers[:3], shape=shape, variance=dv)
            assert not np.array_equal(_bits(dev.readDenoised(raw=True, shape=shape)), _bits(got)), "the measured variance changed nothing"
        elif (width, height) == (1, 1):
            assert info["sampled"].all()
    # every pixel on the fallback side: twk_denoise_variance's bits, and the restatement is restate_variance's
    dn, dv = L.Denoiser(iterations=4), L.DenoiserVariance()
    few = moments.copy()
    few[..., 2] = np.minimum(few[..., 2], MIN_SAMPLES - 1)
    buffers[3].upload(few)
    dev.denoise(dn, *pointers[:3], shape=shape, variance=dv, moments=pointers[3], minSamples=MIN_SAMPLES)
    got = dev.readDenoised(raw=True, shape=shape)
    dev.denoise(dn, *pointers[:3], shape=shape, variance=dv)
    _assert_same_bits(got, dev.readDenoised(raw=True, shape=shape), "fallback side everywhere against twk_denoise_variance")
    widen = lambda a: a.astype(F)
    a = restate_sampled(widen(beauty), widen(albedo), widen(normal), few, MIN_SAMPLES, dn, dv, _exp(orc), _sqrt(orc))[0]
    b = restate_variance(widen(beauty), widen(albedo), widen(normal), dn, dv, _exp(orc), _sqrt(orc))[0]
    _assert_same_bits(a, b, "restate_sampled on the fallback side against restate_variance")
    for buf, arr in zip(buffers, (beauty, albedo, normal, few)):
        _assert_same_bits(buf.download(arr.shape, arr.dtype), arr, "input after twk_denoise_variance_sampled")
    for buf in buffers + [out]:
        buf.free()
    dev.close()


def test_refusals(twk):
    L = twk._lib
    INVALID_VALUE, INVALID_STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, call):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and "twk_denoise_variance_sampled" in str(e.value), str(e.value)

    dev = _rendered(twk, 2, moments=False)
    refused(INVALID_STATE, lambda: dev.denoise(minSamples=2))                     # no moments enabled
    dev.enableMoments(True)
    for it in range(2):
        dev.render(it)
    dev.denoise(minSamples=2)
    for n in (1, 0, -1):
        refused(INVALID_VALUE, lambda: dev.denoise(minSamples=n))
    refused(INVALID_VALUE, lambda: dev.denoise(L.Denoiser(iterations=9), minSamples=2))           # twk_denoise's own refusals, under the new name
    refused(INVALID_VALUE, lambda: dev.denoise(variance=L.DenoiserVariance(sigmaLuminance=0.0), minSamples=2))
    beauty, nbytes = dev.outputDevicePointer()
    moments, mbytes = dev.momentsDevicePointer()
    assert mbytes == 61 * 37 * 16
    rgb = L.Denoiser(inputKind=0)
    refused(INVALID_VALUE, lambda: dev.denoise(rgb, beauty, shape=(37, 61), minSamples=2))          # an explicit beauty without moments
    refused(INVALID_VALUE, lambda: dev.denoise(rgb, moments=moments, minSamples=2))               # moments without a beauty
    refused(INVALID_VALUE, lambda: dev.denoise(rgb, beauty, shape=(37, 61), moments=moments, denoised=moments, minSamples=2))  # the output overlaps the moments
    refused(INVALID_VALUE, lambda: dev.denoise(rgb, beauty, shape=(37, 61), moments=moments, denoised=moments + mbytes - 16, minSamples=2))
    refused(INVALID_VALUE, lambda: dev.denoise(rgb, beauty, shape=(37, 61), moments=moments, denoised=beauty, minSamples=2))
    dev.denoise(rgb, beauty, shape=(37, 61), moments=moments, minSamples=2)
    explicit = dev.readDenoised(raw=True, shape=(37, 61))
    dev.denoise(rgb, minSamples=2)
    _assert_same_bits(dev.readDenoised(raw=True), explicit, "the handle's own buffers passed explicitly")
    dev.close()
    # a packed tile buffer is no picture
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (61, 37))
    tile = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tile, distribution=1)
    tile.enableMoments(True)
    tile.render(0)
    refused(INVALID_STATE, lambda: tile.denoise(rgb, minSamples=2))
    tile.close()


def test_command_line_with_denoiser_sampled_variance(twk, tmp_path):
    """rtigo3_hip -m 1 with `denoiserSampledVariance 1` beside `denoiser 3`: the screenshot is twk_tonemap of the mode's result, byte
    for byte, and not the picture of the same run with `denoiserVariance 1` in its place."""
    from test_gpu_screenshot import _run_cli
    system, png = _run_cli(tmp_path, 0, extra="denoiser 3\ndenoiserSampledVariance 1\ndenoiserMinSamples 3\ndenoiserFirefly 2.5\n")
    app = twk.Application(system, scene_path("scene_rtigo3_cornell_box.txt"))
    on, dn = app.denoiser
    _, dv = app.denoiserVariance
    son, min_samples = app.denoiserSampled
    assert on and dn.inputKind == 2 and son and min_samples == 3 and dv.fireflyThreshold == 2.5
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)  # enables the AOVs and the moments
    for it in range(4):
        dev.render(it)
    assert (dev.readMoments()[..., 2] == 4).all()
    dev.denoise(dn, variance=dv, minSamples=min_samples)
    ptr, _ = dev.denoisedDevicePointer()
    expect = dev.tonemap(app.tonemapper, ptr, shape=(64, 96))
    assert png.shape == (64, 96, 3) and np.array_equal(png, expect[::-1])
    dev.close()
    (tmp_path / "spatial").mkdir()
    _, png_spatial = _run_cli(tmp_path / "spatial", 0, extra="denoiser 3\ndenoiserVariance 1\ndenoiserFirefly 2.5\n")
    assert not np.array_equal(png, png_spatial)


def test_it_denoises_better(twk):
    """C2 at 160x90 against the renderer's own 512 spp, every filter at its defaults, in the two measures of
    test_gpu_denoise.test_it_denoises. The inequalities are the CPU sweep's own (tools/denoise_sampled_sweep.py through the
    restatement, profiles/r09_denoise_sampled.md), which the device computes too where the bit tests above hold; no margins:
      4 spp   unfiltered 0.285 / 0.886, twk_denoise_variance 0.193 / 0.317 (0.19329), sampled 0.193 / 0.283 (0.19310)
      16 spp  unfiltered 0.134 / 0.460, twk_denoise_variance 0.103 / 0.250,           sampled 0.094 / 0.202
    (64 spp, in the sweep only: 0.064 / 0.220, 0.070 / 0.222, 0.050 / 0.157.) Strictly below the unfiltered input at 16 spp, and
    strictly below twk_denoise_variance at 4 and at 16 spp, where the sweep showed it."""
    L = twk._lib
    reference = _rendered(twk, 512, res=(160, 90), moments=False)
    r = reference.getOutputBufferHost()
    reference.close()
    for spp in (4, 16):
        dev = _rendered(twk, spp, res=(160, 90))
        noisy = dev.getOutputBufferHost()
        dev.denoise(variance=L.DenoiserVariance())
        spatial = dev.readDenoised()
        dev.denoise(variance=L.DenoiserVariance(), moments=True)
        sampled = dev.readDenoised()
        dev.close()
        e_noisy, e_spatial, e_sampled = _errors(noisy, r), _errors(spatial, r), _errors(sampled, r)
        print(f"\n{spp} spp, relative RMSE / per-pixel relative RMSE against 512 spp: unfiltered {e_noisy[0]:.5f} / {e_noisy[1]:.5f}, "
              f"twk_denoise_variance {e_spatial[0]:.5f} / {e_spatial[1]:.5f}, twk_denoise_variance_sampled {e_sampled[0]:.5f} / {e_sampled[1]:.5f}")
        if spp == 16:
            assert e_sampled[0] < e_noisy[0] and e_sampled[1] < e_noisy[1]
        assert e_sampled[0] < e_spatial[0]
        assert e_sampled[1] < e_spatial[1]
