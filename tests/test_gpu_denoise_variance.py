"""-m gpu: twk_denoise_variance, the variance-guided, firefly-clamping mode of the a-trous filter (the spatial-variance path of
Schied et al. 2017, SVGF sections 4.2 and 4.4): a moments pass estimates a per-pixel luminance variance from the picture itself and
clamps fireflies against it, and the levels scale their colour edge-stop by it.

The mode is defined operation by operation in csrc/denoise_device.h. `restate_variance` below is that definition again in numpy
float32, statement for statement, with the exp and sqrt of the CPU oracle (orc.oracle_math(2, .) / (6, .)): the device result must
equal it in every bit, alpha included, in both output formats. (tools/denoise_variance_sweep.py runs the same restatement on the
oracle's renders to choose the defaults; it needs no GPU.)
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_app, scene_path
from test_gpu_denoise import BUILDS, CASES, H5, _assert_same_bits, _bits, _choose_build, _cornell, _dist2, _errors, _exp, _expect, _finite3, _own_buffers, _synthetic
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

HALF = 1
F = np.float32
RADIUS = 3               # TWK_DENOISE_MOMENTS_RADIUS
EPSILON = F(1e-3)        # TWK_DENOISE_LUMINANCE_EPSILON
B3 = np.array([1 / 4, 1 / 2, 1 / 4], F)  # the 3 x 3 binomial; every product of two is exact


def _lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _taps(height, width, dx, dy, s):
    """Slices (P, Q) of the pixels p whose tap q = p + (dx s, dy s) lies inside the picture; None when there is none."""
    y0, y1 = max(0, -dy * s), min(height, height - dy * s)
    x0, x1 = max(0, -dx * s), min(width, width - dx * s)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))


def restate_variance(beauty, albedo, normal, dn, dv, exp, sqrt):
    """The variance-guided mode of csrc/denoise_device.h in numpy float32. beauty / albedo / normal: float32 [H, W, 4] (halves
    widened); returns (float32 [H, W, 4] before the final narrowing, mask of the pixels that pass through with the input's bits)."""
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
        guides_finite = np.ones(b.shape[:2], bool)  # of the guides in use, at the centre
        if kind >= 2:
            guides_finite &= _finite3(normal)
        if kind >= 1:
            guides_finite &= _finite3(albedo)
        if demod:
            d = np.fmax(albedo[..., :3].astype(F), F(0.01))
            c[..., :3] = b[..., :3] / d
        # moments
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
                    ok = ok & (t <= F(87.0))  # a NaN t compares false
                    g = exp(np.where(ok, -t, F(0)).astype(F)).reshape(t.shape)
                lq = lum[Q]
                s0[P] = s0[P] + np.where(ok, g, F(0))  # adding +0 leaves the sums as they are
                s1[P] = s1[P] + np.where(ok, g * lq, F(0))
                s2[P] = s2[P] + np.where(ok, g * (lq * lq), F(0))
        estimated = fin & np.isfinite(lum) & guides_finite & (s0 > 0)
        m1, m2 = s1 / s0, s2 / s0
        var = np.fmax(m2 - m1 * m1, F(0))  # fmaxf: a NaN difference gives 0
        moments = np.concatenate([c[..., :3], np.where(estimated, var, F(0))[..., None]], axis=-1).astype(F)
        if firefly > 0:
            limit = m1 + firefly * sq(var)
            clamp = estimated & (lum > limit) & (limit > 0)
            f = limit / lum
            moments[clamp, :3] = (c[..., :3] * f[..., None])[clamp]
        c = moments
        # levels
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
            out = c.copy()
            centre = fin & guides_finite & np.isfinite(lum)
            out[centre, :3] = (total / wsum[..., None])[centre]
            out[centre, 3] = (vsum / (wsum * wsum))[centre]
            c = out
        # finish
        r = c[..., :3] * d if demod else c[..., :3]
        o = b.copy()
        through = ~(_finite3(b) & guides_finite & np.isfinite(r).all(axis=-1))
        o[~through, :3] = (r + blend * (b[..., :3] - r))[~through]
    assert o.dtype == F
    return o, through


def _sqrt(orc):
    return lambda x: orc.oracle_math(6, x)


def _expect_variance(beauty_raw, albedo_raw, normal_raw, dn, dv, orc):
    """restate_variance fed the raw buffers, narrowed like the device (cf. test_gpu_denoise._expect)."""
    o, through = restate_variance(beauty_raw.astype(F), None if albedo_raw is None else albedo_raw.astype(F), None if normal_raw is None else normal_raw.astype(F),
                                  dn, dv, _exp(orc), _sqrt(orc))
    if beauty_raw.dtype == np.float16:
        with np.errstate(over="ignore"):
            o = o.astype(np.float16)
        o[through] = beauty_raw[through]
    return o


# clamp on (the default k) in every case of test_gpu_denoise.CASES; clamp off (k = 0) with each inputKind, each count of levels and demodulation off / on
VARIANCE_CASES = [case + (None,) for case in CASES] + [(2, 3, 1, 0.0), (1, 1, 0, 0.0), (0, 5, 0, 0.0)]


def _variance(L, firefly):
    return L.DenoiserVariance() if firefly is None else L.DenoiserVariance(fireflyThreshold=firefly)


@BUILDS
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_render_equals_the_restatement_bit_for_bit(twk, orc, half, lds_max_step, monkeypatch):
    """C2 at 160x90, 4 spp, the handle's own buffers: the three inputKinds x 1 / 3 / 5 levels x demodulation off / on with the
    clamp on, and the clamp off with every inputKind, with the default choice of level builds and every level on either build;
    the inputs are unchanged afterwards, and a second call returns the same bits."""
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    dev = _cornell(twk, 4, half=half)
    beauty, albedo, normal = _own_buffers(dev, half)
    for kind, iterations, demod, firefly in VARIANCE_CASES:
        dn, dv = L.Denoiser(inputKind=kind, iterations=iterations, demodulateAlbedo=demod), _variance(L, firefly)
        dev.denoise(dn, variance=dv)
        got = dev.readDenoised(raw=True)
        expect = _expect_variance(beauty, albedo if kind >= 1 else None, normal if kind >= 2 else None, dn, dv, orc)
        _assert_same_bits(got, expect, f"kind {kind}, {iterations} levels, demodulate {demod}, firefly {firefly}")
        assert (got[..., 3] == 1).all()
        if kind == 2 and iterations == 3 and firefly is None:
            plain = _expect(beauty, albedo, normal, dn, _exp(orc))
            assert not np.array_equal(_bits(got), _bits(plain)), "the mode computes what twk_denoise computes"
            dev.denoise(dn, variance=dv)
            _assert_same_bits(dev.readDenoised(raw=True), got, "second call")
    after = _own_buffers(dev, half)
    for a, b, name in zip(after, (beauty, albedo, normal), ("beauty", "albedo", "normal")):
        _assert_same_bits(a, b, f"input {name} after twk_denoise_variance")
    dev.close()


def _small_device(twk, half=False):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    if half:
        dev.setOutputFormat(HALF)
    return dev


def _upload(twk, arrays):
    buffers = [_DeviceBuffer(twk, a.nbytes) for a in arrays]
    for buf, a in zip(buffers, arrays):
        buf.upload(a)
    return buffers


@BUILDS
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_explicit_buffers_with_inf_nan_and_null_albedo(twk, orc, half, lds_max_step, monkeypatch):
    """The synthetic 64x48 frame of test_gpu_denoise (inf, NaN, null albedo, non-finite guides) through explicit buffers."""
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    dev = _small_device(twk, half)
    arrays = _synthetic(half)
    beauty, albedo, normal = arrays
    shape = beauty.shape[:2]
    buffers = _upload(twk, arrays)
    out = _DeviceBuffer(twk, beauty.nbytes)
    pointers = [b.ptr.value for b in buffers]
    for kind, iterations, demod, firefly in ((2, 4, 1, None), (2, 2, 0, 1.0), (1, 3, 1, None), (0, 3, 0, None), (2, 5, 1, 0.0)):
        dn, dv = L.Denoiser(inputKind=kind, iterations=iterations, demodulateAlbedo=demod), _variance(L, firefly)
        expect = _expect_variance(beauty, albedo if kind >= 1 else None, normal if kind >= 2 else None, dn, dv, orc)
        dev.denoise(dn, *pointers, shape=shape, denoised=out.ptr.value, variance=dv)
        dev.synchronizeStream()
        _assert_same_bits(out.download(beauty.shape, beauty.dtype), expect, f"explicit buffers, kind {kind}, {iterations} levels, demodulate {demod}, firefly {firefly}")
        dev.denoise(dn, *pointers, shape=shape, variance=dv)
        got = dev.readDenoised(raw=True, shape=shape)
        _assert_same_bits(got, expect, "internal buffer")
        _assert_same_bits(got[..., 3], beauty[..., 3], "alpha")
    bad = ~_finite3(beauty.astype(F))
    assert bad.sum() >= 14 and np.array_equal(_bits(got)[bad], _bits(beauty)[bad])
    assert np.isfinite(got.astype(F)[~bad]).all()
    for buf, a in zip(buffers, arrays):
        _assert_same_bits(buf.download(a.shape, a.dtype), a, "input after twk_denoise_variance")
    for buf in buffers + [out]:
        buf.free()
    dev.close()


@pytest.mark.parametrize("width,height", [(1, 1), (5, 3), (61, 37)])
def test_smallest_shapes(twk, orc, width, height):
    """1x1: every window tap falls outside the picture (no variance, no clamp, the level's only tap is the centre); 5x3: narrower than
    the halo of the moments pass; 61x37: no multiple of the 32x8 tile and narrower than the reach 2 x 16 of step 16 (5 levels)."""
    L = twk._lib
    rng = np.random.default_rng(width * 1000 + height)
    beauty = rng.gamma(2.0, 0.5, (height, width, 4)).astype(F)
    beauty[rng.random((height, width)) < 0.05, :3] *= F(200.0)
    albedo = np.ones((height, width, 4), F)
    albedo[..., :3] = rng.uniform(0.3, 0.4, (height, width, 3)).astype(F)
    normal = np.zeros((height, width, 4), F)
    normal[..., :3] = (0.0, 0.6, 0.8)
    normal[:, width // 2:, :3] = (0.6, 0.0, 0.8)
    dev = _small_device(twk)
    buffers = _upload(twk, (beauty, albedo, normal))
    pointers = [b.ptr.value for b in buffers]
    for kind, iterations in ((2, 5), (0, 3), (1, 1)):
        dn, dv = L.Denoiser(inputKind=kind, iterations=iterations), L.DenoiserVariance()
        dev.denoise(dn, *pointers, shape=(height, width), variance=dv)
        got = dev.readDenoised(raw=True, shape=(height, width))
        expect = _expect_variance(beauty, albedo if kind >= 1 else None, normal if kind >= 2 else None, dn, dv, orc)
        _assert_same_bits(got, expect, f"{width}x{height}, kind {kind}, {iterations} levels")
    if (width, height) == (1, 1):
        # a single pixel: nothing to estimate from, and sum w c / sum w of one tap is c again up to the rounding of d * (c / d)
        assert np.allclose(got[..., :3], beauty[..., :3], rtol=3e-7, atol=0)
    for buf in buffers:
        buf.free()
    dev.close()


def _flat_field(amplitude, fireflies=()):
    """64x48, grey 0.5 + uniform noise of +-amplitude (the same in r, g, b), alpha 1, flat guides (albedo 1, normal +z)."""
    h, w = 48, 64
    rng = np.random.default_rng(2017)
    beauty = np.ones((h, w, 4), F)
    beauty[..., :3] = (F(0.5) + rng.uniform(-amplitude, amplitude, (h, w)).astype(F))[..., None]
    for y, x in fireflies:
        beauty[y, x, :3] = 1000.0
    albedo = np.ones((h, w, 4), F)
    normal = np.zeros((h, w, 4), F)
    normal[..., 2] = 1.0
    return beauty, albedo, normal


def test_fireflies_are_clamped(twk):
    """A flat field 0.5 +- A (A = 0.01) with six isolated pixels of 1000, more than 2R + 1 = 7 apart and off the border.

    twk_denoise keeps them: the assertion below, so that the case cannot pass for a trivial reason.
    The bound for the new mode, fireflyThreshold k: every field value lies in [0.5 - A, 0.5 + A]. The window of a firefly p holds
    no other firefly and leaves p out, so its m1 lies in that interval and its variance is at most A^2 (Popoviciu: a variable on an
    interval of length 2A has variance <= A^2), hence limit <= 0.5 + A + k A, and p is scaled to luminance limit: r = g = b
    <= 0.5 + (1 + k) A. A field pixel is either left alone or scaled down to its own limit, and limit >= m1, a weighted mean of
    window values that are all >= 0.5 - A (a firefly in the window only raises it): it stays >= 0.5 - A. So after the
    moments pass every pixel lies in [0.5 - A, 0.5 + (1 + k) A], and every level replaces a pixel by a convex combination (weights
    >= 0, normalised) of such pixels, which stays inside. Albedo 1 makes demodulation the identity. Rounding: luminance weights
    that sum to 1 within 2^-23, the f32 sums and quotients of at most 48 terms: 1e-4 absolute is generous at values of 0.5."""
    L = twk._lib
    A = 0.01
    fireflies = ((8, 9), (8, 40), (20, 25), (30, 50), (39, 12), (40, 33))
    for i, (y0, x0) in enumerate(fireflies):
        for y1, x1 in fireflies[i + 1:]:
            assert max(abs(y0 - y1), abs(x0 - x1)) > 2 * RADIUS + 1
    beauty, albedo, normal = _flat_field(A, fireflies)
    dev = _small_device(twk)
    buffers = _upload(twk, (beauty, albedo, normal))
    pointers = [b.ptr.value for b in buffers]
    dev.denoise(L.Denoiser(), *pointers, shape=beauty.shape[:2])
    plain = dev.readDenoised(shape=beauty.shape[:2])
    kept = min(plain[y, x, :3].min() for y, x in fireflies)
    print(f"\ntwk_denoise keeps the fireflies at >= {kept:.1f}")
    assert kept > 100.0
    for k in (L.DenoiserVariance().fireflyThreshold, 1.0):
        dev.denoise(L.Denoiser(), *pointers, shape=beauty.shape[:2], variance=L.DenoiserVariance(fireflyThreshold=k))
        got = dev.readDenoised(shape=beauty.shape[:2])[..., :3].astype(np.float64)
        lo, hi = 0.5 - A - 1e-4, 0.5 + (1 + k) * A + 1e-4
        print(f"k = {k}: output in [{got.min():.5f}, {got.max():.5f}], bound [{lo:.5f}, {hi:.5f}]")
        assert lo <= got.min() and got.max() <= hi
    for buf in buffers:
        buf.free()
    dev.close()


def test_a_constant_picture_comes_back(twk):
    """No noise: variance 0, every tap's t is 0 and its weight h h exp(0) = h h exactly; the output is fl(sum w c) / fl(sum w) of 25
    (fewer at the border) terms. With c constant, every partial sum of the w c and of the w carries a relative error of at most
    (n - 1) u after n terms, each product w c one more u, the quotient one more: <= (24 + 1 + 24 + 1) u = 50 u per level, u = 2^-24,
    and 5 levels compound to <= 250 u (1 + o(1)) < 1.5e-5 relative. Demodulation by albedo 1 is exact."""
    L = twk._lib
    h, w = 48, 64
    beauty = np.ones((h, w, 4), F)
    beauty[..., :3] = (0.3, 0.7, 0.123456)
    albedo = np.ones((h, w, 4), F)
    normal = np.zeros((h, w, 4), F)
    normal[..., 2] = 1.0
    dev = _small_device(twk)
    buffers = _upload(twk, (beauty, albedo, normal))
    dev.denoise(L.Denoiser(iterations=5), *[b.ptr.value for b in buffers], shape=(h, w), variance=L.DenoiserVariance())
    got = dev.readDenoised(shape=(h, w))
    rel = np.abs(got[..., :3].astype(np.float64) / beauty[..., :3].astype(np.float64) - 1.0).max()
    print(f"\nconstant picture: max relative deviation {rel:.3e} (bound {250 * 2.0 ** -24:.3e})")
    assert rel <= 250 * 2.0 ** -24
    _assert_same_bits(got[..., 3], beauty[..., 3], "alpha")
    for buf in buffers:
        buf.free()
    dev.close()


def test_edges_hold(twk):
    """The two-halves input of test_gpu_denoise.test_edges_hold (normal +x / -x, colour 0 / 1, sigmaNormal 0.1, 5 levels): within 1e-3
    of its own side's colour in the variance-guided mode too."""
    L = twk._lib
    h, w = 64, 96
    beauty = np.zeros((h, w, 4), F)
    beauty[:, w // 2:, :3] = 1.0
    beauty[..., 3] = 1.0
    normal = np.zeros((h, w, 4), F)
    normal[:, :w // 2, 0] = 1.0
    normal[:, w // 2:, 0] = -1.0
    albedo = np.full((h, w, 4), 0.5, F)
    dev = _small_device(twk)
    buffers = _upload(twk, (beauty, albedo, normal))
    for demod in (0, 1):
        dev.denoise(L.Denoiser(iterations=5, sigmaNormal=0.1, demodulateAlbedo=demod), *[b.ptr.value for b in buffers], shape=(h, w), variance=L.DenoiserVariance())
        got = dev.readDenoised(shape=(h, w))
        err = np.abs(got[..., :3] - beauty[..., :3]).max()
        print(f"\nedges hold (demodulate {demod}): max |output - own side's colour| {err:.3e}")
        assert err <= 1e-3
    for buf in buffers:
        buf.free()
    dev.close()


def test_it_denoises_better(twk):
    """C2 at 160x90, 4 spp against the renderer's own 512 spp: the mode at its defaults is strictly below default twk_denoise on the
    same input in both measures of test_gpu_denoise.test_it_denoises.
    Values of the CPU sweep through the restatement (profiles/r08_denoise_variance.md), which the device computes too
    where the bit tests above hold: unfiltered 4 spp 0.285 / 0.886, twk_denoise 0.216 / 0.549, twk_denoise_variance 0.193 / 0.317."""
    L = twk._lib
    reference = _cornell(twk, 512, aov=False)
    r = reference.getOutputBufferHost()
    reference.close()
    dev = _cornell(twk, 4)
    noisy = dev.getOutputBufferHost()
    dev.denoise()
    plain = dev.readDenoised()
    dev.denoise(variance=L.DenoiserVariance())
    guided = dev.readDenoised()
    dev.close()
    e_noisy, e_plain, e_guided = _errors(noisy, r), _errors(plain, r), _errors(guided, r)
    print(f"\nrelative RMSE / per-pixel relative RMSE against 512 spp: unfiltered 4 spp {e_noisy[0]:.3f} / {e_noisy[1]:.3f}, "
          f"twk_denoise (defaults) {e_plain[0]:.3f} / {e_plain[1]:.3f}, twk_denoise_variance (defaults) {e_guided[0]:.3f} / {e_guided[1]:.3f}")
    assert e_guided[0] < e_plain[0]
    assert e_guided[1] < e_plain[1]


def test_refusals_and_identities(twk, orc):
    L = twk._lib
    dev = _cornell(twk, 4)
    beauty, albedo, normal = _own_buffers(dev, False)
    nan, inf = float("nan"), float("inf")
    for bad in (L.DenoiserVariance(fireflyThreshold=-1.0), L.DenoiserVariance(fireflyThreshold=nan), L.DenoiserVariance(fireflyThreshold=inf),
                L.DenoiserVariance(sigmaLuminance=0.0), L.DenoiserVariance(sigmaLuminance=-2.0), L.DenoiserVariance(sigmaLuminance=nan), L.DenoiserVariance(sigmaLuminance=inf)):
        with pytest.raises(twk.TwkError) as e:
            dev.denoise(variance=bad)
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_denoise_variance" in str(e.value), str(e.value)
    # twk_denoise's own refusals hold, under the new call's name; sigmaColor is ignored
    with pytest.raises(twk.TwkError) as e:
        dev.denoise(L.Denoiser(iterations=9), variance=L.DenoiserVariance())
    assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_denoise_variance" in str(e.value)
    L.lib.twk_denoise_variance.restype = C.c_int
    assert L.lib.twk_denoise_variance(dev.handle, None, None, None, None, None, 0, 0, None) == L.TWK_ERROR_INVALID_VALUE
    dev.denoise(L.Denoiser(sigmaColor=0.0), variance=L.DenoiserVariance())
    ignored = dev.readDenoised(raw=True)
    dev.denoise(variance=L.DenoiserVariance())
    _assert_same_bits(dev.readDenoised(raw=True), ignored, "sigmaColor is ignored")
    # the copies
    dev.denoise(L.Denoiser(iterations=0), variance=L.DenoiserVariance())
    _assert_same_bits(dev.readDenoised(raw=True), beauty, "iterations 0")
    dev.denoise(L.Denoiser(blendFactor=1.0), variance=L.DenoiserVariance())
    _assert_same_bits(dev.readDenoised(raw=True), beauty, "blendFactor 1")
    # twk_denoise afterwards computes what it always did
    dev.denoise(variance=L.DenoiserVariance())
    dn = L.Denoiser()
    dev.denoise(dn)
    _assert_same_bits(dev.readDenoised(raw=True), _expect(beauty, albedo, normal, dn, _exp(orc)), "twk_denoise after twk_denoise_variance")
    dev.close()


def test_command_line_with_denoiser_variance(twk, tmp_path):
    """rtigo3_hip -m 1 with `denoiserVariance 1` beside `denoiser 3`: the screenshot is twk_tonemap of the mode's result, byte for
    byte, and not the picture of the same run without the key."""
    from test_gpu_screenshot import _run_cli
    system, png = _run_cli(tmp_path, 0, extra="denoiser 3\ndenoiserVariance 1\ndenoiserFirefly 2.5\n")
    app = twk.Application(system, scene_path("scene_rtigo3_cornell_box.txt"))
    on, dn = app.denoiser
    von, dv = app.denoiserVariance
    assert on and dn.inputKind == 2 and von and dv.fireflyThreshold == 2.5
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    for it in range(4):
        dev.render(it)
    dev.denoise(dn, variance=dv)
    ptr, _ = dev.denoisedDevicePointer()
    expect = dev.tonemap(app.tonemapper, ptr, shape=(64, 96))
    assert png.shape == (64, 96, 3) and np.array_equal(png, expect[::-1])
    dev.close()
    (tmp_path / "without").mkdir()
    _, png_without = _run_cli(tmp_path / "without", 0, extra="denoiser 3\n")
    assert not np.array_equal(png, png_without)
