"""-m gpu: twk_denoise_geometry, the geometry guide of the a-trous denoiser (plane and instance stops from the geometry AOV), in the
three modes of the filter. The device result equals tests/denoise_geometry_restate.py (csrc/denoise_device.h in numpy float32) and
the host form twk_denoise_geometry_host in every bit, in both output formats, with every level on the direct-load and on the
LDS-staged build, also at the smallest shapes, where most taps lie outside the picture; with a geometry of misses only its bytes are those of the three existing calls; on the Cornell box the own-buffer
form equals the explicit form; a stale geometry is refused."""
import numpy as np
import pytest

from conftest import load_app
from denoise_geometry_restate import CAMERA, instance_bits, restate, step_scene, synthetic, world_positions
from test_denoise_geometry_host import MODES, _exp, _mode, _sqrt, host
from test_gpu_denoise import BUILDS, _choose_build, _restate
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
HALF = 1
SHAPES = [(19, 37), (21, 70)]


def _device(twk, half=False, res=(32, 32)):
    """A fresh handle; the output format is chosen after initDevice, which sets the description's."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    if half:
        dev.setOutputFormat(HALF)
    return app, dev


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _same(got, expect, what):
    assert got.shape == expect.shape and got.dtype == expect.dtype, what
    diff = _bits(got) != _bits(expect)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} values differ in their bits, first at {np.argwhere(diff)[:4].tolist()}"


def _narrow(o, through, beauty_raw):
    """The device's narrowing of a float32 result: round to nearest even once; a pixel that passes through keeps the input's bits."""
    if beauty_raw.dtype == np.float16:
        with np.errstate(over="ignore"):
            o = o.astype(np.float16)
        o[through] = beauty_raw[through]
    return o


class _Uploaded:
    def __init__(self, twk, arrays):
        self.buffers = [_DeviceBuffer(twk, a.nbytes) for a in arrays]
        for buf, a in zip(self.buffers, arrays):
            buf.upload(a)
        self.pointers = [b.ptr.value for b in self.buffers]

    def free(self):
        for b in self.buffers:
            b.free()


@BUILDS
@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_device_equals_restatement_and_host_form(twk, orc, half, lds_max_step, monkeypatch):
    """The synthetic pictures of the host test (37x19 and 70x21, 5 levels, all three modes, demodulation on / off, instanceStop
    off / on) through explicit buffers: the restatement's bits; in RGBA32F also the host form's."""
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    app, dev = _device(twk, half)
    for shape in SHAPES:
        beauty, albedo, normal, moments, geometry = synthetic(*shape)
        if half:
            beauty, albedo, normal = (a.astype(np.float16) for a in (beauty, albedo, normal))
        up = _Uploaded(twk, (beauty, albedo, normal, moments, geometry))
        pb, pa, pn, pm, pg = up.pointers
        wide = [a.astype(F) for a in (beauty, albedo, normal)]
        for mode in MODES:
            dv, use_moments, min_samples = _mode(L, mode)
            for demod, stop, sigma in ((1, 0, 0.01), (0, 1, 0.03)):
                dn = L.Denoiser(iterations=5, demodulateAlbedo=demod, sigmaColor=1.5)
                dg = L.DenoiserGeometry(sigmaPosition=sigma, instanceStop=stop)
                dev.denoise(dn, pb, pa, pn, shape=shape, variance=dv, moments=pm if use_moments else None, minSamples=min_samples if use_moments else None,
                            geometry=dg, geometryBuffer=pg, camera=CAMERA)
                got = dev.readDenoised(raw=True, shape=shape)
                o, through = restate(*wide, geometry, CAMERA, dn, dg, _exp(orc), _sqrt(orc), dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
                what = f"{shape}, {mode}, demodulate {demod}, instanceStop {stop}"
                _same(got, _narrow(o, through, beauty), what)
                if not half:
                    rc, on_host = host(L, dn, dg, beauty, albedo, normal, geometry, dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
                    assert rc == 0
                    _same(got, on_host, what + ", host form")
        for buf, a in zip(up.buffers, (beauty, albedo, normal, moments, geometry)):
            _same(buf.download(a.shape, a.dtype), a, "input after twk_denoise_geometry")
        up.free()
    dev.close()
    app.close()


BORDER_SHAPES = [(1, 1), (3, 5), (37, 61)]  # (height, width)
_border_cache = {}


def _border_case(L, orc, shape):
    """Inputs and the three restatements of one border shape, computed once and shared by both builds: noise over two depths and two
    instances, with one column of misses (the middle one; the single pixel of 1x1 is a hit)."""
    if shape not in _border_cache:
        h, w = shape
        rng = np.random.default_rng(1000 * w + h)
        beauty = rng.gamma(2.0, 0.5, (h, w, 4)).astype(F)
        albedo = np.ones((h, w, 4), F)
        albedo[..., :3] = rng.uniform(0.3, 0.4, (h, w, 3)).astype(F)
        normal = np.zeros((h, w, 4), F)
        normal[..., 2] = 1.0
        normal[..., :2] = rng.normal(0.0, 0.05, (h, w, 2)).astype(F)
        depth = np.full((h, w), 3.0)
        depth[:, (w * 3) // 4:] = 3.2
        ids = np.ones((h, w), np.uint32)
        ids[h // 2:, : w // 4] = 2
        geometry = np.zeros((h, w, 4), F)
        geometry[..., :3] = world_positions(h, w, depth)
        if w > 1:
            ids[:, w // 2] = 0
            geometry[:, w // 2, :3] = 0.0
            normal[:, w // 2, :3] = 0.0
        geometry[..., 3] = instance_bits(ids)
        dn, dg, dv = L.Denoiser(iterations=5, sigmaColor=1.5), L.DenoiserGeometry(sigmaPosition=0.05), L.DenoiserVariance()
        expect = {"plain": _restate(beauty, albedo, normal, dn, _exp(orc))[0]}
        for mode, variance in (("geometry", None), ("geometry, variance", dv)):
            expect[mode] = restate(beauty, albedo, normal, geometry, CAMERA, dn, dg, _exp(orc), _sqrt(orc), dv=variance)[0]
        _border_cache[shape] = ((beauty, albedo, normal, geometry), (dn, dg, dv), expect)
    return _border_cache[shape]


@pytest.mark.parametrize("lds_max_step", ["0", "128"], ids=["direct", "staged"])
def test_the_border_on_either_build(twk, orc, lds_max_step, monkeypatch):
    """Where a tap lies outside the picture is the one thing the two builds of the level tell differently (a bounds test; a NaN
    colour staged in LDS). 1x1: every tap but the centre is outside; 5x3: narrower than the halo of either pass; 61x37: no multiple
    of the 32x8 tile and narrower than the reach 2 x 16 of step 16. 5 levels, RGBA32F, explicit buffers, every level on the direct
    and on the staged build: twk_denoise equals test_gpu_denoise._restate, twk_denoise_geometry plain and variance-guided equal
    denoise_geometry_restate.restate, in every bit."""
    L = twk._lib
    _choose_build(monkeypatch, lds_max_step)
    app, dev = _device(twk)
    for shape in BORDER_SHAPES:
        arrays, (dn, dg, dv), expect = _border_case(L, orc, shape)
        hits = arrays[3][..., 3].view(np.uint32) != 0
        assert hits.any() and (shape == (1, 1) or (~hits).all(axis=0).sum() == 1)
        up = _Uploaded(twk, arrays)
        pb, pa, pn, pg = up.pointers
        for mode in expect:
            if mode == "plain":
                dev.denoise(dn, pb, pa, pn, shape=shape)
            else:
                dev.denoise(dn, pb, pa, pn, shape=shape, variance=dv if "variance" in mode else None, geometry=dg, geometryBuffer=pg, camera=CAMERA)
            _same(dev.readDenoised(raw=True, shape=shape), expect[mode], f"{shape[1]}x{shape[0]}, {mode}, TWK_DENOISE_LDS_MAX_STEP {lds_max_step}")
        up.free()
    dev.close()
    app.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_step_scene_and_all_miss_anchor(twk, half):
    """On the device: the step scene comes out exactly 1 and exactly 0; and with a geometry of misses only the bytes are those of
    twk_denoise, twk_denoise_variance and twk_denoise_variance_sampled on the same buffers (default choice of level builds, 5 levels)."""
    L = twk._lib
    app, dev = _device(twk, half)
    kind = np.float16 if half else F
    beauty, albedo, normal, geometry = step_scene()
    shape = beauty.shape[:2]
    up = _Uploaded(twk, (beauty.astype(kind), albedo.astype(kind), normal.astype(kind), geometry))
    dn = L.Denoiser(iterations=4, sigmaColor=100.0)
    dev.denoise(dn, *up.pointers[:3], shape=shape)
    plain = dev.readDenoised(shape=shape)
    assert ((plain[..., :3] > 0) & (plain[..., :3] < 1)).any()
    for dv in (None, L.DenoiserVariance()):
        dev.denoise(dn, *up.pointers[:3], shape=shape, variance=dv, geometry=L.DenoiserGeometry(sigmaPosition=0.01), geometryBuffer=up.pointers[3], camera=CAMERA)
        assert np.array_equal(dev.readDenoised(shape=shape), beauty)
    up.free()

    beauty, albedo, normal, moments, _ = synthetic(19, 37)
    shape = beauty.shape[:2]
    up = _Uploaded(twk, (beauty.astype(kind), albedo.astype(kind), normal.astype(kind), moments, np.zeros_like(moments)))
    pb, pa, pn, pm, pg = up.pointers
    dn = L.Denoiser(iterations=5, sigmaColor=1.5)
    for mode in MODES:
        dv, use_moments, min_samples = _mode(L, mode)
        older = dict(variance=dv, moments=pm if use_moments else None, minSamples=min_samples if use_moments else None)
        dev.denoise(dn, pb, pa, pn, shape=shape, **older)
        expect = dev.readDenoised(raw=True, shape=shape)
        dev.denoise(dn, pb, pa, pn, shape=shape, geometry=L.DenoiserGeometry(instanceStop=1), geometryBuffer=pg, camera=CAMERA, **older)
        _same(dev.readDenoised(raw=True, shape=shape), expect, f"all-miss geometry, {mode}")
    up.free()
    dev.close()
    app.close()


def test_own_buffers_equal_the_explicit_form_and_a_stale_geometry_is_refused(twk):
    """The Cornell box at 64x48, 4 spp: the own-buffer form (the handle's accumulation, AOVs, moments, geometry AOV and camera 0)
    equals the explicit form fed the handle's own pointers (copies of the AOVs, which have no pointer getter) in all three modes, and
    differs from the unguided call. Then the refusals of the own-buffer form."""
    L = twk._lib
    STATE, VALUE = L.TWK_ERROR_INVALID_STATE, L.TWK_ERROR_INVALID_VALUE
    app, dev = _device(twk, res=(64, 48))
    shape = (48, 64)
    dev.setShaderVariant(1)
    dev.enableAov(True)
    dev.enableMoments(True)

    def refused(code, call, *words):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and "twk_denoise_geometry" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    for it in range(4):
        dev.render(it)
    dg = L.DenoiserGeometry()
    refused(STATE, lambda: dev.denoise(geometry=dg), "twk_enable_geometry")
    dev.enableGeometry(True)
    refused(STATE, lambda: dev.denoise(geometry=dg), "twk_render_geometry")
    dev.renderGeometry()
    geometry = dev.readGeometry()
    hits = geometry[..., 3].view(np.uint32) != 0
    assert 0.5 < hits.mean() < 1.0, "the view holds the box and some background: hits and misses both take part"
    guides = _Uploaded(twk, (dev.readAov(0), dev.readAov(1)))
    out_ptr, _ = dev.outputDevicePointer()
    moments_ptr, _ = dev.momentsDevicePointer()
    geometry_ptr, _ = dev.geometryDevicePointer()
    for mode in MODES:
        dv, use_moments, min_samples = _mode(L, mode)
        dev.denoise(variance=dv, minSamples=min_samples if use_moments else None, geometry=dg)
        own = dev.readDenoised(raw=True)
        dev.denoise(None, out_ptr, *guides.pointers, shape=shape, variance=dv, moments=moments_ptr if use_moments else None, minSamples=min_samples if use_moments else None,
                    geometry=dg, geometryBuffer=geometry_ptr, camera=app.cameras[0])
        _same(dev.readDenoised(raw=True, shape=shape), own, f"explicit form, {mode}")
        dev.denoise(variance=dv, minSamples=min_samples if use_moments else None)
        assert not np.array_equal(_bits(dev.readDenoised(raw=True)), _bits(own)), f"{mode}: the guide changes the picture"
        assert np.isfinite(own).all()
    # the parameters and the explicit form's buffers
    refused(VALUE, lambda: dev.denoise(L.Denoiser(inputKind=1), geometry=dg), "inputKind")
    refused(VALUE, lambda: dev.denoise(L.Denoiser(inputKind=0), geometry=dg), "inputKind")
    for sigma in (0.0, -1.0, 1e30, float("nan")):
        refused(VALUE, lambda: dev.denoise(geometry=L.DenoiserGeometry(sigmaPosition=sigma)), "sigmaPosition")
    refused(VALUE, lambda: dev.denoise(None, out_ptr, *guides.pointers, shape=shape, geometry=dg), "geometry")
    refused(VALUE, lambda: dev.denoise(None, out_ptr, *guides.pointers, shape=shape, geometry=dg, geometryBuffer=geometry_ptr, denoised=geometry_ptr), "overlaps")
    refused(VALUE, lambda: dev.denoise(geometry=dg, geometryBuffer=geometry_ptr), "beauty")
    # the camera moved after the trace: the geometry is of the old view
    moved = twk.camera_frustum(tuple(app.info.center), app.info.phi + 0.01, app.info.theta, app.info.fov, app.info.distance, 64 / 48)
    dev.updateCamera(0, moved)
    refused(STATE, lambda: dev.denoise(geometry=dg), "older than the camera")
    dev.renderGeometry()
    dev.denoise(geometry=dg)
    guides.free()
    dev.close()
    # a packed tile buffer is not a picture
    tiled = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tiled, distribution=1)
    tiled.enableAov(True)
    tiled.enableGeometry(True)
    tiled.render(0)
    tiled.renderGeometryTile()
    refused(STATE, lambda: tiled.denoise(geometry=dg), "tile")
    tiled.close()
    app.close()
