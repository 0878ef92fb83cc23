"""-m gpu: twk_denoise, the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; a classical filter, no network) that stands
where Optix7Gui calls optixDenoiserInvoke (apps/Optix7Gui/src/Application.cpp:942-1001), guided by the albedo and normal AOVs.

The filter is defined operation by operation in csrc/denoise_device.h. `_restate` below is that definition again in numpy float32,
statement for statement, with the Cephes exp of the CPU oracle (orc.oracle_math(2, .), pinned bit for bit against the device's
by the math tests): the device result must equal it in every bit, alpha included, in both output formats.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_app, scene_path
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

HALF = 1
F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)  # B3 spline; every product of two is exact


def _finite3(c):
    return np.isfinite(c[..., :3]).all(axis=-1)


def _dist2(a, b):
    e = a[..., :3] - b[..., :3]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def _restate(beauty, albedo, normal, dn, exp):
    """csrc/denoise_device.h in numpy float32. beauty / albedo / normal: float32 [H, W, 4] (halves widened); returns (float32
    [H, W, 4] before the final narrowing, mask of the pixels that pass through with the input's bits)."""
    b = np.ascontiguousarray(beauty, F)
    if dn.iterations == 0 or dn.blendFactor == 1.0:
        return b.copy(), np.ones(b.shape[:2], bool)
    kind, demod = dn.inputKind, bool(dn.demodulateAlbedo)
    inv_color = F(1.0) / (F(dn.sigmaColor) * F(dn.sigmaColor))
    inv_normal = F(1.0) / (F(dn.sigmaNormal) * F(dn.sigmaNormal)) if kind >= 2 else F(0)
    inv_albedo = F(1.0) / (F(dn.sigmaAlbedo) * F(dn.sigmaAlbedo)) if kind >= 1 else F(0)
    blend = F(dn.blendFactor)
    height, width = b.shape[:2]
    with np.errstate(all="ignore"):
        # prepare
        c = b.copy()
        guides_finite = np.ones(b.shape[:2], bool)  # of the guides in use, at the centre
        if kind >= 2:
            guides_finite &= _finite3(normal)
        if kind >= 1:
            guides_finite &= _finite3(albedo)
        if demod:
            d = np.fmax(albedo[..., :3].astype(F), F(0.01))  # fmaxf: a NaN component gives 0.01
            c[..., :3] = b[..., :3] / d
        # levels
        for level in range(dn.iterations):
            s = 1 << level
            total = np.zeros((height, width, 3), F)
            wsum = np.zeros((height, width), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    # pixels p whose tap q = p + (dx s, dy s) lies inside the picture
                    y0, y1 = max(0, -dy * s), min(height, height - dy * s)
                    x0, x1 = max(0, -dx * s), min(width, width - dx * s)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    cq = c[Q]
                    t = _dist2(c[P], cq) * inv_color
                    if kind >= 2:
                        t = t + _dist2(normal[P], normal[Q]) * inv_normal
                    if kind >= 1:
                        t = t + _dist2(albedo[P], albedo[Q]) * inv_albedo
                    ok = _finite3(cq) & (t <= F(87.0))  # a NaN t compares false
                    e = exp(np.where(ok, -t, F(0)).astype(F)).reshape(t.shape)
                    w = np.where(ok, (H5[dy + 2] * H5[dx + 2]) * e, F(0))  # weight 0: adding +0 leaves the sums as they are
                    total[P] = total[P] + np.where(ok[..., None], w[..., None] * cq[..., :3], F(0))
                    wsum[P] = wsum[P] + w
            out = c.copy()
            centre = _finite3(c) & guides_finite  # a centre whose colour or guide is not finite passes through
            out[centre, :3] = (total / wsum[..., None])[centre]
            c = out
        # finish
        r = c[..., :3] * d if demod else c[..., :3]
        o = b.copy()
        through = ~(_finite3(b) & guides_finite & np.isfinite(r).all(axis=-1))  # r not finite: the demodulated colour overflowed
        o[~through, :3] = (r + blend * (b[..., :3] - r))[~through]
    assert o.dtype == F
    return o, through


def _exp(orc):
    return lambda x: orc.oracle_math(2, x)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _assert_same_bits(got, expect, what):
    assert got.shape == expect.shape and got.dtype == expect.dtype, what
    diff = _bits(got) != _bits(expect)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} values differ in their bits, first at {np.argwhere(diff)[:4].tolist()}, max |diff| {np.nanmax(np.abs(got.astype(np.float64) - expect.astype(np.float64)))}"


def _expect(beauty_raw, albedo_raw, normal_raw, dn, exp):
    """The restatement fed the raw buffers (float32, or float16 widened), narrowed like the device: astype(float16) rounds to
    nearest even; a pixel that passes through keeps the input's bits."""
    o, through = _restate(beauty_raw.astype(F), None if albedo_raw is None else albedo_raw.astype(F), None if normal_raw is None else normal_raw.astype(F), dn, exp)
    if beauty_raw.dtype == np.float16:
        with np.errstate(over="ignore"):
            o = o.astype(np.float16)
        o[through] = beauty_raw[through]
    return o


def _cornell(twk, spp, half=False, res=(160, 90), aov=True):
    """C2 (Cornell box, full BSDF set) with Optix7Gui's closest-hit rule, AOVs on."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.setShaderVariant(1)
    if aov:
        dev.enableAov(True)
    if half:
        dev.setOutputFormat(HALF)
    for it in range(spp):
        dev.render(it)
    return dev


def _own_buffers(dev, half):
    if half:
        return dev.getOutputBufferHalf(), dev.readAov(0, raw=True), dev.readAov(1, raw=True)
    return dev.getOutputBufferHost(), dev.readAov(0), dev.readAov(1)


CASES = [(kind, iterations, demod) for kind in (0, 1, 2) for iterations in (1, 3, 5) for demod in ((0, 1) if kind else (0,))]

# The level kernel has two builds, LDS-staged and direct-load, chosen per level by its step (staged up to step 4 by default).
# TWK_DENOISE_LDS_MAX_STEP, read when the handle is created, moves the border: 0 = every level direct, 128 = every level staged.
BUILDS = pytest.mark.parametrize("lds_max_step", [None, "0", "128"], ids=["default", "direct", "staged"])


def _choose_build(monkeypatch, lds_max_step):
    if lds_max_step is None:
        monkeypatch.delenv("TWK_DENOISE_LDS_MAX_STEP", raising=False)
    else:
        monkeypatch.setenv("TWK_DENOISE_LDS_MAX_STEP", lds_max_step)



@BUILDS
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_render_equals_the_restatement_bit_for_bit(twk, orc, half, lds_max_step, monkeypatch):
    """All three inputKinds x 1 / 3 / 5 levels x demodulation off / on, on the handle's own buffers, with the default choice of
    level builds (steps 1 - 4 staged in LDS, step 16 direct) and with every level on either build; the inputs are unchanged after
    the calls, and a second call returns the same bits."""
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    dev = _cornell(twk, 4, half=half)
    beauty, albedo, normal = _own_buffers(dev, half)
    assert np.isfinite(beauty.astype(F)).all() and beauty[..., :3].max() > 0.5
    for kind, iterations, demod in CASES:
        dn = L.Denoiser(inputKind=kind, iterations=iterations, demodulateAlbedo=demod)
        dev.denoise(dn)
        got = dev.readDenoised(raw=True)
        expect = _expect(beauty, albedo if kind >= 1 else None, normal if kind >= 2 else None, dn, _exp(orc))
        _assert_same_bits(got, expect, f"kind {kind}, {iterations} levels, demodulate {demod}")
        assert (got[..., 3] == 1).all()
        if kind == 2 and iterations == 3:
            assert not np.array_equal(_bits(got), _bits(beauty)), "the filter changed nothing"
            _assert_same_bits(dev.readDenoised(), got.astype(F), "twk_read_denoised widens exactly")
            ptr, nbytes = dev.denoisedDevicePointer()
            assert ptr and nbytes == got.nbytes
            dev.denoise(dn)
            _assert_same_bits(dev.readDenoised(raw=True), got, "second call")
    after = _own_buffers(dev, half)
    for a, b, name in zip(after, (beauty, albedo, normal), ("beauty", "albedo", "normal")):
        _assert_same_bits(a, b, f"input {name} after twk_denoise")
    dev.close()


def _synthetic(half):
    """A frame with noise over three flat regions, inf / NaN / -inf colours (alone, in a cluster, on the border), albedo of
    exactly 0, negative colours and a non-trivial alpha."""
    rng = np.random.default_rng(20100625)
    h, w = 48, 64
    beauty = rng.gamma(2.0, 0.5, (h, w, 4)).astype(F)
    beauty[:, 40:, :3] *= F(4.0)
    beauty[..., 3] = rng.uniform(0.25, 1.0, (h, w)).astype(F)
    albedo = np.zeros((h, w, 4), F)
    albedo[..., :3] = rng.uniform(0.2, 0.9, 3).astype(F)
    albedo[:, 20:40, :3] = rng.uniform(0.0, 1.0, (h, 20, 3)).astype(F)
    albedo[..., 3] = 1
    albedo[10:14, 10:14, :3] = 0.0  # exactly 0: demodulated by the clamp 0.01
    albedo[30, 5, 1] = 0.0
    normal = np.zeros((h, w, 4), F)
    n = rng.normal(size=(h, w, 3))
    n[:, :32] = (0.0, 0.6, 0.8)
    normal[..., :3] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    normal[40:, :, :3] = 0.0  # a miss: null normal
    beauty[5, 5, 0] = np.inf
    beauty[5, 6, 1] = np.nan
    beauty[6, 5, 2] = -np.inf
    beauty[20:23, 50:53, :3] = np.nan
    beauty[0, 0, :3] = np.inf
    beauty[h - 1, w - 1, 0] = np.nan
    beauty[25, 25, :3] = (-0.5, -0.25, 0.0)
    # guides that are not finite: such a centre passes through, such a tap weighs 0
    albedo[15, 44, 0] = np.nan
    normal[16, 45, 1] = np.inf
    normal[2, 2, :3] = np.nan
    if not half:
        beauty[17, 46, :3] = 3.0e38  # finite, but 3e38 / 0.01 is not: passes through
        albedo[17, 46, :3] = 0.0
    if half:
        return beauty.astype(np.float16), albedo.astype(np.float16), normal.astype(np.float16)
    return beauty, albedo, normal


@BUILDS
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_explicit_buffers_with_inf_nan_and_null_albedo(twk, orc, half, lds_max_step, monkeypatch):
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    if half:
        dev.setOutputFormat(HALF)
    arrays = _synthetic(half)
    shape = arrays[0].shape[:2]
    buffers = [_DeviceBuffer(twk, a.nbytes) for a in arrays]
    for buf, a in zip(buffers, arrays):
        buf.upload(a)
    out = _DeviceBuffer(twk, arrays[0].nbytes)
    beauty, albedo, normal = arrays
    for kind, iterations, demod in ((2, 4, 1), (2, 2, 0), (1, 3, 1), (0, 3, 0)):
        dn = L.Denoiser(inputKind=kind, iterations=iterations, demodulateAlbedo=demod, sigmaColor=1.5)
        expect = _expect(beauty, albedo if kind >= 1 else None, normal if kind >= 2 else None, dn, _exp(orc))
        # into a buffer of the caller ...
        dev.denoise(dn, buffers[0].ptr.value, buffers[1].ptr.value, buffers[2].ptr.value, shape=shape, denoised=out.ptr.value)
        dev.synchronizeStream()
        got = out.download(beauty.shape, beauty.dtype)
        _assert_same_bits(got, expect, f"explicit buffers, kind {kind}, {iterations} levels, demodulate {demod}")
        # ... and into the internal one
        dev.denoise(dn, buffers[0].ptr.value, buffers[1].ptr.value, buffers[2].ptr.value, shape=shape)
        _assert_same_bits(dev.readDenoised(raw=True, shape=shape), expect, "internal buffer")
    bad = ~_finite3(beauty.astype(F))
    assert bad.sum() >= 14 and np.array_equal(_bits(got)[bad], _bits(beauty)[bad])
    # (the last case is unguided: the non-finite guides play no part in it; the guided cases above covered them)
    dn = L.Denoiser(sigmaColor=1.5)
    dev.denoise(dn, buffers[0].ptr.value, buffers[1].ptr.value, buffers[2].ptr.value, shape=shape)
    guided = dev.readDenoised(raw=True, shape=shape)
    for y, x in ((15, 44), (16, 45), (2, 2)) + (() if half else ((17, 46),)):
        assert np.array_equal(_bits(guided)[y, x], _bits(beauty)[y, x]), (y, x)
    assert np.isfinite(guided[15, 45].astype(F)).all() and np.isfinite(guided.astype(F)[~bad]).all()
    # a neighbour of a non-finite pixel is filtered from its finite taps
    assert np.isfinite(got[5, 7].astype(F)).all() and np.isfinite(got[19, 51].astype(F)).all()
    for buf, a in zip(buffers, arrays):
        _assert_same_bits(buf.download(a.shape, a.dtype), a, "input after twk_denoise")
    for buf in buffers + [out]:
        buf.free()
    dev.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_identities(twk, orc, half):
    """iterations 0 and blendFactor 1 return the input's bits; blendFactor 0.5 is the restated lerp."""
    L = twk._lib
    dev = _cornell(twk, 4, half=half)
    beauty, albedo, normal = _own_buffers(dev, half)
    dev.denoise(L.Denoiser(iterations=0))
    _assert_same_bits(dev.readDenoised(raw=True), beauty, "iterations 0")
    dev.denoise(L.Denoiser(blendFactor=1.0))
    _assert_same_bits(dev.readDenoised(raw=True), beauty, "blendFactor 1")
    dn = L.Denoiser(blendFactor=0.5)
    dev.denoise(dn)
    half_way = dev.readDenoised(raw=True)
    _assert_same_bits(half_way, _expect(beauty, albedo, normal, dn, _exp(orc)), "blendFactor 0.5")
    dev.denoise(L.Denoiser())
    full = dev.readDenoised()
    # the lerp lies between its ends (to rounding)
    lo, hi = np.minimum(full, beauty.astype(F)), np.maximum(full, beauty.astype(F))
    tol = 2.0 ** (-9 if half else -20) * np.maximum(1.0, hi)
    assert ((half_way.astype(F) >= lo - tol) & (half_way.astype(F) <= hi + tol)).all()
    dev.close()


def test_edges_hold(twk):
    """Two halves that differ in normal (+x / -x) and colour (0 / 1), no noise, sigmaNormal 0.1, 5 levels: with the normals 2
    apart the cross-edge weight is exp(-400), 0 in f32, so every pixel stays within 1e-3 of its own side's colour."""
    L = twk._lib
    h, w = 64, 96
    beauty = np.zeros((h, w, 4), F)
    beauty[:, w // 2:, :3] = 1.0
    beauty[..., 3] = 1.0
    normal = np.zeros((h, w, 4), F)
    normal[:, :w // 2, 0] = 1.0
    normal[:, w // 2:, 0] = -1.0
    albedo = np.full((h, w, 4), 0.5, F)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    buffers = [_DeviceBuffer(twk, a.nbytes) for a in (beauty, albedo, normal)]
    for buf, a in zip(buffers, (beauty, albedo, normal)):
        buf.upload(a)
    for demod in (0, 1):
        dev.denoise(L.Denoiser(iterations=5, sigmaNormal=0.1, demodulateAlbedo=demod), *[b.ptr.value for b in buffers], shape=(h, w))
        got = dev.readDenoised(shape=(h, w))
        err = np.abs(got[..., :3] - beauty[..., :3]).max()
        print(f"\nedges hold (demodulate {demod}): max |output - own side's colour| {err:.3e}")
        assert err <= 1e-3
    for buf in buffers:
        buf.free()
    dev.close()


def _errors(x, r):
    x, r = x[..., :3].astype(np.float64), r[..., :3].astype(np.float64)
    return np.sqrt(((x - r) ** 2).sum() / (r ** 2).sum()), np.sqrt(np.mean((x - r) ** 2 / (r ** 2 + 0.01)))


def test_it_denoises(twk):
    """C2 at 160x90, 4 spp, filtered with the defaults, against the renderer's own 512 spp image: lower error than the unfiltered
    4 spp image in relative RMSE ||x - r|| / ||r|| and in per-pixel relative RMSE sqrt(mean((x - r)^2 / (r^2 + 0.01))).
    Values seen on the MI355X: unfiltered 4 spp 0.285 / 0.886, filtered 0.216 / 0.549, unfiltered 16 spp 0.134 / 0.460."""
    reference = _cornell(twk, 512, aov=False)
    r = reference.getOutputBufferHost()
    reference.close()
    dev = _cornell(twk, 4)
    noisy = dev.getOutputBufferHost()
    dev.denoise()
    filtered = dev.readDenoised()
    for it in range(4, 16):
        dev.render(it)
    spp16 = dev.getOutputBufferHost()
    dev.close()
    e_noisy, e_filtered, e_16 = _errors(noisy, r), _errors(filtered, r), _errors(spp16, r)
    print(f"\nrelative RMSE / per-pixel relative RMSE against 512 spp: unfiltered 4 spp {e_noisy[0]:.3f} / {e_noisy[1]:.3f}, "
          f"filtered (defaults) {e_filtered[0]:.3f} / {e_filtered[1]:.3f}, unfiltered 16 spp {e_16[0]:.3f} / {e_16[1]:.3f}")
    assert e_filtered[0] < e_noisy[0]
    assert e_filtered[1] < e_noisy[1]


def test_refusals(twk):
    L = twk._lib
    INVALID_VALUE, INVALID_STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, call):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and "twk_" in str(e.value), str(e.value)
        return str(e.value)

    # the read and pointer calls before any denoise
    dev = _cornell(twk, 2, aov=False)
    assert "twk_read_denoised" in refused(INVALID_STATE, dev.readDenoised)
    assert "twk_read_denoised_raw" in refused(INVALID_STATE, lambda: dev.readDenoised(raw=True))
    assert "twk_get_denoised_device_pointer" in refused(INVALID_STATE, dev.denoisedDevicePointer)
    # AOVs off with a guided kind; the unguided kind runs
    assert "twk_denoise" in refused(INVALID_STATE, dev.denoise)
    assert "twk_denoise" in refused(INVALID_STATE, lambda: dev.denoise(L.Denoiser(inputKind=1)))
    dev.denoise(L.Denoiser(inputKind=0))
    assert dev.readDenoised().shape == (90, 160, 4)
    # parameters
    for bad in (L.Denoiser(iterations=9), L.Denoiser(iterations=-1), L.Denoiser(sigmaColor=0.0), L.Denoiser(sigmaNormal=-1.0), L.Denoiser(sigmaAlbedo=0.0),
                L.Denoiser(sigmaColor=1e-30), L.Denoiser(blendFactor=2.0), L.Denoiser(blendFactor=-0.1), L.Denoiser(blendFactor=float("nan")),
                L.Denoiser(inputKind=3), L.Denoiser(inputKind=0, demodulateAlbedo=1)):
        refused(INVALID_VALUE, lambda: dev.denoise(bad))
    L.lib.twk_denoise.restype = C.c_int
    assert L.lib.twk_denoise(dev.handle, None, None, None, None, 0, 0, None) == INVALID_VALUE
    # the output aliasing an input: the handle's own buffer, and explicit ones
    own, nbytes = dev.outputDevicePointer()
    refused(INVALID_VALUE, lambda: dev.denoise(L.Denoiser(inputKind=0), denoised=own))
    buf = _DeviceBuffer(twk, 64 * 64 * 16 * 2)
    first, second = buf.ptr.value, buf.ptr.value + 64 * 64 * 16
    refused(INVALID_VALUE, lambda: dev.denoise(L.Denoiser(inputKind=0), first, shape=(64, 64), denoised=first))
    refused(INVALID_VALUE, lambda: dev.denoise(L.Denoiser(inputKind=1), first, second, shape=(64, 64), denoised=second))
    refused(INVALID_VALUE, lambda: dev.denoise(L.Denoiser(inputKind=0), first, shape=(64, 64), denoised=first + 16))  # overlapping
    refused(INVALID_VALUE, lambda: dev.denoise(L.Denoiser(inputKind=2), first, second, shape=(64, 64)))  # no normal buffer
    dev.denoise(L.Denoiser(inputKind=0), first, shape=(64, 64), denoised=second)  # side by side: accepted
    dev.synchronizeStream()
    buf.free()
    # after a format switch the denoised picture of the old format is gone
    dev.setOutputFormat(HALF)
    refused(INVALID_STATE, dev.readDenoised)
    dev.close()

    # a tiled handle's own buffer is not a picture
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (160, 90))
    tiled = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tiled, distribution=1)
    tiled.enableAov(True)
    tiled.render(0)
    assert "tile" in refused(INVALID_STATE, tiled.denoise)
    tiled.close()


def test_command_line_with_denoiser_3(twk, tmp_path):
    """rtigo3_hip -m 1 with `denoiser 3`: the screenshot is twk_tonemap of twk_get_denoised_device_pointer, byte for byte, and it is
    not the picture of the same run without the key."""
    from test_gpu_screenshot import _run_cli
    system, png = _run_cli(tmp_path, 0, extra="denoiser 3\ndenoiserIterations 4\n")
    app = twk.Application(system, scene_path("scene_rtigo3_cornell_box.txt"))
    on, dn = app.denoiser
    assert on and dn.inputKind == 2 and dn.iterations == 4
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)  # enables the AOVs: the key asks for a guided kind
    for it in range(4):
        dev.render(it)
    dev.denoise(dn)
    ptr, _ = dev.denoisedDevicePointer()
    expect = dev.tonemap(app.tonemapper, ptr, shape=(64, 96))
    assert png.shape == (64, 96, 3) and np.array_equal(png, expect[::-1])
    plain = dev.tonemap(app.tonemapper)
    assert not np.array_equal(png, plain[::-1])
    dev.close()
    (tmp_path / "plain").mkdir()
    _, png_plain = _run_cli(tmp_path / "plain", 0)
    assert np.array_equal(png_plain, plain[::-1])


def test_command_line_with_several_devices(twk, tmp_path):
    """Three handles sharing the GPU: `denoiser 1` (no guides) filters the assembled frame, in each of the three buffer strategies, and
    gives the single-device picture; a guided kind is refused before anything is rendered (no frame rate line)."""
    import re
    import subprocess
    from test_gpu_screenshot import _run_cli
    from test_screenshot_files import CLI
    (tmp_path / "single").mkdir()
    _, single = _run_cli(tmp_path / "single", 0, extra="denoiser 1\n")
    (tmp_path / "plain").mkdir()
    _, plain = _run_cli(tmp_path / "plain", 0)
    assert not np.array_equal(single, plain)
    for strategy in (3, 1, 2):
        _, png = _run_cli(tmp_path, strategy, env={"TWK_CLI_VIRTUAL_DEVICES": "3"}, extra="denoiser 1\n")
        assert np.array_equal(png, single), f"strategy {strategy}"
    system = tmp_path / "system_refused.txt"
    text = re.sub(r"(?m)^strategy .*$", "strategy 3", open(scene_path("system_rtigo3_cornell_box.txt")).read())
    system.write_text(text + "\nresolution 96 64\ndenoiser 3\n")
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path("scene_rtigo3_cornell_box.txt"), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120, env={**__import__("os").environ, "TWK_CLI_VIRTUAL_DEVICES": "3"})
    assert r.returncode != 0 and "denoiser 3" in r.stderr and "fps" not in r.stdout
