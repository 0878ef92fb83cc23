"""-m gpu: the resolve of the firefly cascade (twk_cascade_resolve, csrc/cascade_kernels.hip) against the numpy restatement
tests/cascade_restate.py, bit for bit, on the handle's own layers and on explicit buffers, in both output formats; the resolved
picture as the explicit beauty of twk_denoise_variance_sampled; and the two conditions that chose the default kappa, on the device."""
import ctypes as C

import numpy as np
import pytest

import cascade_restate as restate
from test_gpu_denoise import _assert_same_bits, _cornell, _errors
from test_gpu_denoise_sampled import _expect_sampled
from test_gpu_denoise_variance import _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_moments import ITERATIONS, RES, _app, _device, _passes, _same
from test_moments_host import F

pytestmark = pytest.mark.gpu

WIDE = (4, 0.01, 2.0)  # every layer and the clamp in use on C2 (tests/test_gpu_cascade.py)
ALL_ONE = 1e-30        # a kappa so small that every weight whose layer has energy is 1


def _narrow(a, half):
    if not half:
        return a
    with np.errstate(over="ignore"):
        return a.astype(np.float16)


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("params", [None, WIDE], ids=["defaults", "narrow"])
def test_own_buffer_and_explicit_resolve_equal_the_restatement_bit_for_bit(twk, params, half):
    L = twk._lib
    cascade = L.Cascade() if params is None else L.Cascade(*params)
    b = restate.thresholds(cascade.layers, cascade.start, cascade.base)
    dev = _device(twk, _app(twk), half=half)
    with pytest.raises(twk.TwkError) as e:
        dev.cascadeResolve()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_enable_cascade" in str(e.value)
    dev.enableCascade(True, cascade)
    with pytest.raises(twk.TwkError) as e:
        dev.readResolved()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_read_resolved" in str(e.value)
    _passes(dev, ITERATIONS)
    layers = dev.readCascade()
    pixels = RES[0] * RES[1]
    mine = _DeviceBuffer(twk, pixels * (8 if half else 16))
    copy = _DeviceBuffer(twk, layers.nbytes)
    copy.upload(layers)
    for kappa in (L.TWK_CASCADE_KAPPA, ALL_ONE):
        expect = restate.resolve(layers, b, kappa)
        if kappa == ALL_ONE:
            total = layers[0, ..., :3].copy()
            for j in range(1, len(b)):
                total = total + layers[j, ..., :3]
            _same(expect[..., :3], total / layers[0, ..., 3:], "every weight 1: the plain quotient")
        else:
            assert not np.array_equal(expect, restate.resolve(layers, b, ALL_ONE)), "the default kappa changes nothing on this frame"
        expect = _narrow(expect, half)
        dev.cascadeResolve(resolve=L.CascadeResolve(kappa))
        got = dev.readResolved()
        assert got.dtype == F and (got[..., 3] == 1).all()
        _same(got, expect.astype(F), f"own-buffer resolve at kappa {kappa}")
        # the device pointer holds the picture in the output format, narrowed once
        ptr, nbytes = dev.resolvedDevicePointer()
        assert ptr and nbytes == mine.nbytes
        raw = np.empty(expect.shape, expect.dtype)
        assert mine.hip.hipMemcpy(raw.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
        _assert_same_bits(raw, expect, "the resolved buffer behind the pointer")
        # explicit form, on a copy of the layers, into the caller's buffer: the same bits, and the input is not written
        dev.cascadeResolve(cascade, L.CascadeResolve(kappa), layers=copy.ptr.value, shape=(RES[1], RES[0]), resolved=mine.ptr.value)
        dev.synchronizeStream()
        _assert_same_bits(mine.download(expect.shape, expect.dtype), expect, f"explicit resolve at kappa {kappa}")
        _same(copy.download(layers.shape, F), layers, "the explicit form's input afterwards")
    _same(dev.readCascade(), layers, "the handle's layers after the resolves")
    # refusals of the call itself
    shape = (RES[1], RES[0])
    for kw, word in ((dict(layers=copy.ptr.value), "without a size"), (dict(shape=shape), "without layers"), (dict(resolved=mine.ptr.value), "without layers"),
                     (dict(params=cascade, layers=copy.ptr.value, shape=shape, resolved=copy.ptr.value + 16), "overlaps"),
                     (dict(params=L.Cascade(5, 1.0, 8.0)), "differs"), (dict(resolve=L.CascadeResolve(0.0)), "kappa"), (dict(params=L.Cascade(1, 1.0, 8.0)), "layers")):
        with pytest.raises(twk.TwkError) as e:
            dev.cascadeResolve(**kw)
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_cascade_resolve" in str(e.value) and word in str(e.value), (kw, str(e.value))
    mine.free()
    copy.free()
    dev.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_the_resolved_picture_as_the_beauty_of_the_sampled_denoiser(twk, orc, half):
    """twk_get_resolved_device_pointer feeds the explicit `beauty` of twk_denoise_variance_sampled unchanged; the guides and the
    moments are the frame's own (uploaded copies: the explicit form takes every input)."""
    L = twk._lib
    dev = _device(twk, _app(twk), half=half, aov=True)
    dev.setShaderVariant(1)
    dev.enableCascade(True)
    _passes(dev, ITERATIONS)
    dev.cascadeResolve()
    resolved = _narrow(restate.resolve(dev.readCascade(), restate.thresholds(), L.TWK_CASCADE_KAPPA), half)
    albedo, normal = dev.readAov(0, raw=True), dev.readAov(1, raw=True)
    moments = dev.readMoments()
    buffers = _upload(twk, (albedo, normal, moments))
    ptr, _ = dev.resolvedDevicePointer()
    dn, dv = L.Denoiser(), L.DenoiserVariance()
    dev.denoise(dn, ptr, buffers[0].ptr.value, buffers[1].ptr.value, shape=(RES[1], RES[0]), variance=dv, moments=buffers[2].ptr.value, minSamples=4)
    got = dev.readDenoised(raw=True, shape=(RES[1], RES[0]))
    _assert_same_bits(got, _expect_sampled(resolved, albedo, normal, moments, 4, dn, dv, orc), "twk_denoise_variance_sampled over the resolved picture")
    # and the tonemapper takes the pointer as it takes any picture in the output format
    ldr = dev.tonemap(rgbaDevicePointer=ptr, shape=(RES[1], RES[0]), half=half)
    up = _upload(twk, (resolved,))[0]
    assert np.array_equal(ldr, dev.tonemap(rgbaDevicePointer=up.ptr.value, shape=(RES[1], RES[0]), half=half))
    for buffer in buffers + [up]:
        buffer.free()
    dev.close()


def test_the_resolve_is_better_where_samples_are_few_and_no_worse_where_they_are_many(twk):
    """The two conditions that chose the default kappa (tools/cascade_sweep.py, profiles/r15_cascade.md), on the device: C2 at
    160x90, Optix7Gui rule, against 256 spp of the same device. At 16 spp the resolved picture's per-pixel relative RMSE is strictly
    below the plain picture's; at 64 spp its relative RMSE is not above the plain picture's. The reference's 256 samples are seeded
    as iterations 64 .. 319 (twk_set_sample_offset), so that it shares no sample with either frame: against a reference that holds
    the frame's own samples the plain mean's error would be understated by what they share, and the resolve's bias would not."""
    reference = _cornell(twk, 0, aov=False)
    reference.setSampleOffset(64)
    for it in range(256):
        reference.render(it)
    r256 = reference.getOutputBufferHost()
    reference.close()
    dev = _cornell(twk, 0, aov=False)
    dev.enableCascade(True)
    figures = {}
    done = 0
    for spp in (16, 64):
        for it in range(done, spp):
            dev.render(it)
        done = spp
        dev.cascadeResolve()
        figures[spp] = (dev.getOutputBufferHost(), dev.readResolved())
    dev.close()
    e = {spp: (_errors(p, r256), _errors(r, r256)) for spp, (p, r) in figures.items()}
    print("\nrelative RMSE / per-pixel relative RMSE against 256 spp: " + "; ".join(
        f"{spp} spp plain {a[0]:.4f} / {a[1]:.4f}, resolved {b[0]:.4f} / {b[1]:.4f}" for spp, (a, b) in e.items()))
    assert e[16][1][1] < e[16][0][1], "per-pixel relative RMSE at 16 spp"
    assert e[64][1][0] <= e[64][0][0], "relative RMSE at 64 spp"
