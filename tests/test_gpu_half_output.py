"""-m gpu: the RGBA16F output format (twk_set_output_format TWK_OUTPUT_HALF4 ≙ Optix7Gui's USE_FP32_OUTPUT 0,
apps/Optix7Gui/shaders/app_config.h:57-59; the fold of raygeneration.cu:267-317 with half_common.h:36-80).

The half fold is pinned bit for bit by a reference that does not use the kernel under test: the float path, fed the previous
half mean widened through an output buffer of the test's own, does one lerp in f32; numpy rounds it to half (correctly rounded,
to nearest even, subnormals kept, overflow to inf). Half rounding compounds once per iteration, so a batched pass that folds out
of order, or rounds once per pass instead of once per sample, shows at once.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_app, scene_path
from test_gpu_scenes import _intro07

pytestmark = pytest.mark.gpu

HALF = 1
H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


def _hip(twk):
    # the HIP runtime the library links, resolved through its own handle (see test_gpu_parity.py)
    return twk._lib.lib


def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same_half(got, expect, what):
    """Bit equality of every half; where both are NaN, positions only (payloads are not specified)."""
    got, expect = np.asarray(got, np.float16), np.asarray(expect, np.float16)
    assert got.shape == expect.shape
    gn, en = np.isnan(got), np.isnan(expect)
    assert np.array_equal(gn, en), f"{what}: NaN positions differ ({(gn != en).sum()} values)"
    diff = (got.view(np.uint16) != expect.view(np.uint16)) & ~gn
    assert not diff.any(), f"{what}: {diff.sum()} halves differ, first at {np.argwhere(diff)[:4].tolist()}"


class _DeviceBuffer:
    def __init__(self, twk, nbytes):
        self.hip, self.nbytes, self.ptr = _hip(twk), nbytes, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(nbytes)) == 0

    def upload(self, array):
        array = np.ascontiguousarray(array)
        assert array.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.ptr, array.ctypes.data_as(C.c_void_p), C.c_size_t(array.nbytes), H2D) == 0

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), D2H) == 0
        return out

    def free(self):
        assert self.hip.hipFree(self.ptr) == 0


def _cornell(twk, res):
    return load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res), None, ()


def _device(twk, scene, half, aov=False, batch=None, debug=False, emission=None, index=0, count=1):
    app, material_edit, textures = scene
    dev = twk.Device(ordinal=0, index=index, count=count, miss=app.info.miss)
    for slot, img in textures:
        dev.initTexture(slot, img)
    app.initDevice(dev, distribution=1 if count > 1 else None)
    if material_edit:
        mats = app.materials
        material_edit(mats)
        dev.initMaterials(mats)
    if emission is not None:
        lights = app.lights
        for l in lights:
            l.emission[0], l.emission[1], l.emission[2] = emission
        dev.initLights(lights)
    dev.setDebugExceptions(debug)
    if aov:
        dev.enableAov(True)
    if half:
        dev.setOutputFormat(HALF)
    if batch is not None:
        dev.setLaunchBatch(batch)
    return dev


def _fold_reference(twk, make, iterations):
    """h[k] for k < iterations from the float path: batch 1, the output in a buffer of the test's own, refilled with
    float32(h[k-1]) before iteration k; the launch leaves lerp(float(h[k-1]), r_k, t_k) (or h[k-1], for a dropped sample)."""
    dev = make(half=False, batch=1)
    h, w = dev.state.resolution[1], dev.launchWidth
    buf = _DeviceBuffer(twk, h * w * 16)
    dev.setOutputDevicePointer(buf.ptr.value, buf.nbytes)
    prev = np.zeros((h, w, 4), np.float16)  # the half buffers start zeroed
    means = []
    for k in range(iterations):
        buf.upload(prev.astype(np.float32))
        dev.render(k)
        with np.errstate(over="ignore"):  # what exceeds 65504 rounds to inf, as on the device
            prev = dev.getOutputBufferHost().astype(np.float16)
        means.append(prev)
    dev.setOutputDevicePointer(0, 0)
    dev.close()
    buf.free()
    return means


def _check_fold(twk, make, iterations):
    means = _fold_reference(twk, make, iterations)
    dev = make(half=True)
    for k in range(iterations):
        dev.render(k)
        _assert_same_half(dev.getOutputBufferHalf(), means[k], f"iteration {k}")
    last = dev.getOutputBufferHalf()
    dev.close()
    return last


def test_half_fold_equals_the_float_lerp_rounded_per_iteration(twk):
    """C3 (intro_07: albedo texture, cutout opacity, spherical environment + area light; AOVs on) at 128x72, 64 iterations."""
    scene = _intro07(twk, (128, 72))
    last = _check_fold(twk, lambda **kw: _device(twk, scene, aov=True, **kw), 64)
    assert np.isfinite(last).all() and last[..., :3].max() > 0.5 and (last[..., 3] == 1).all()


def test_batched_equals_single_launches(twk):
    """Half mode: one 64-sample pass and 64 one-sample passes give the same output and AOV halves."""
    scene = _intro07(twk, (128, 72))
    batched = _device(twk, scene, half=True, aov=True, batch=64)
    single = _device(twk, scene, half=True, aov=True, batch=1)
    for it in range(64):
        batched.render(it)
        single.render(it)
    b, s = batched.getOutputBufferHalf(), single.getOutputBufferHalf()
    assert b.dtype == np.float16 and b.shape == (72, 128, 4)
    assert np.array_equal(b.view(np.uint16), s.view(np.uint16))
    for which in (0, 1):
        assert np.array_equal(batched.readAov(which, raw=True).view(np.uint16), single.readAov(which, raw=True).view(np.uint16))
    batched.close()
    single.close()


def test_iteration_zero_is_the_float_buffer_rounded(twk):
    """After iteration 0 the half output and AOVs are np.float16 of the float-mode buffers; twk_read_output / twk_read_aov
    of the half buffers are their exact widening."""
    scene = _intro07(twk, (128, 72))
    devs = [_device(twk, scene, half=half, aov=True) for half in (False, True)]
    for d in devs:
        d.render(0)
    fl, hf = devs
    assert hf.outputFormat == HALF and fl.outputFormat == 0
    _assert_same_half(hf.getOutputBufferHalf(), fl.getOutputBufferHost().astype(np.float16), "output")
    assert np.array_equal(_f32_bits(hf.getOutputBufferHost()), _f32_bits(hf.getOutputBufferHalf().astype(np.float32)))
    for which in (0, 1):
        _assert_same_half(hf.readAov(which, raw=True), fl.readAov(which).astype(np.float16), f"aov {which}")
        assert np.array_equal(_f32_bits(hf.readAov(which)), _f32_bits(hf.readAov(which, raw=True).astype(np.float32)))
        assert fl.readAov(which, raw=True).dtype == np.float32
    for d in devs:
        d.close()


def test_aovs_after_64_iterations(twk):
    """Albedo within the bound of compounded half rounding. With h_k = fl16(lerp(h_{k-1}, a_k, t_k)), t_k = 1/(k+1), the error
    against the exact running mean obeys e_k = (1 - t_k) e_{k-1} + d_k, |d_k| <= 1/2 ulp; unrolled,
    e_n = sum_k d_k (k+1)/(n+1), so |e_n| <= (n+2)/2 * 1/2 ulp = (n+2) * 2^-13 for values <= 1 (ulp 2^-11 in [1/2, 1)).
    n = 63 here: 65 * 2^-13 ~ 7.9e-3 (+1e-5 for the float path's own f32 rounding). Normals: unit length to half precision
    (three components each within 2^-11 relative) wherever they are not null."""
    scene = _intro07(twk, (128, 72))
    devs = [_device(twk, scene, half=half, aov=True) for half in (False, True)]
    for d in devs:
        for it in range(64):
            d.render(it)
    fl, hf = devs
    albedo_f, albedo_h = fl.readAov(0), hf.readAov(0, raw=True).astype(np.float32)
    bound = 65 * 2.0 ** -13 + 1e-5
    err = np.abs(albedo_h[..., :3] - albedo_f[..., :3])
    print(f"\nhalf albedo after 64 iterations: max |error| {err.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound and (albedo_h[..., 3] == 1).all()
    normal = hf.readAov(1, raw=True).astype(np.float32)
    n = np.linalg.norm(normal[..., :3], axis=2)
    hit = n > 0
    assert hit.mean() > 0.5 and np.abs(n[hit] - 1.0).max() <= 2e-3 and (normal[..., 3] == 0).all()
    for d in devs:
        d.close()


@pytest.mark.parametrize("emission,debug", [
    ((-10.0, -10.0, -10.0), True), ((-10.0, -10.0, -10.0), False),
    ((float("inf"),) * 3, True), ((float("inf"),) * 3, False),
    ((1.0e6,) * 3, False),
], ids=["negative-debug", "negative", "infinite-debug", "infinite", "overflow"])
def test_overflow_and_debug_exceptions_fold(twk, emission, debug):
    """The lights of test_debug_exceptions_false_colours (negative, infinite emission), with the debug filter on and off, and a
    finite emission whose samples pass 65504: the fold matches the reference of the first test in every case, including
    pixels that round to inf (a 1e6 false colour, an overflowing sample) and become NaN at the next lerp, as in Optix7Gui."""
    scene = _cornell(twk, (128, 72))
    last = _check_fold(twk, lambda **kw: _device(twk, scene, debug=debug, emission=emission, **kw), 8)
    if debug or emission[0] == 1.0e6:
        assert np.isinf(last[..., :3]).any() or np.isnan(last[..., :3]).any()


def test_time_view_in_half_mode(twk):
    scene = _cornell(twk, (160, 90))
    images = []
    for timed in (False, True):
        dev = _device(twk, scene, half=True)
        dev.setTimeView(timed)
        for it in range(4):
            dev.render(it)
        images.append(dev.getOutputBufferHalf())
        dev.close()
    plain, timed = images
    assert np.array_equal(plain[..., :3].view(np.uint16), timed[..., :3].view(np.uint16))
    alpha = timed[..., 3]
    assert np.isfinite(alpha).all() and (alpha > 0).all() and (plain[..., 3] == 1).all()


def _single_half(twk, scene, iterations):
    dev = _device(twk, scene, half=True)
    for it in range(iterations):
        dev.render(it)
    img = dev.getOutputBufferHalf()
    dev.close()
    return img


def _composited_half(twk, scene, n, iterations):
    """N handles, distribution 1, half packed tiles gathered into one block and assembled by twk_compositor_half.
    Returns (the handle that composited, the frame's device buffer)."""
    handles = [_device(twk, scene, half=True, index=i, count=n) for i in range(n)]
    for it in range(iterations):
        for d in handles:
            d.render(it)
    tiles = np.stack([d.getOutputBufferHalf() for d in handles])
    for d in handles[1:]:
        d.close()
    res = scene[0].state.resolution
    block = _DeviceBuffer(twk, tiles.nbytes)
    block.upload(tiles)
    frame = _DeviceBuffer(twk, res[0] * res[1] * 8)
    handles[0].compositor(block.ptr.value, frame.ptr.value, half=True)
    handles[0].synchronizeStream()
    block.free()
    return handles[0], frame


@pytest.mark.parametrize("n", [2, 3])
def test_tiled_half_compositor_equals_single_device(twk, n):
    res = (200, 120)  # not a multiple of 8 * N: the last tile column is partly outside the image
    scene = _cornell(twk, res)
    single = _single_half(twk, scene, 3)
    dev, frame = _composited_half(twk, scene, n, 3)
    got = frame.download((res[1], res[0], 4), np.float16)
    assert np.array_equal(got.view(np.uint16), single.view(np.uint16)), f"composited half frame of {n} handles differs"
    dev.close()
    frame.free()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_shared_frame_on_pinned_host_memory(twk, half):
    """twk_set_shared_frame on hipHostMalloc(Mapped | Portable) memory (≙ DeviceMultiGPUZeroCopy.cpp:106-118): N = 2, 3 handles
    write their pixels straight into the host frame; each format equals its single-device image bit for bit."""
    hip = _hip(twk)
    res = (200, 120)
    scene = _cornell(twk, res)
    px = 8 if half else 16
    dtype, view = (np.float16, np.uint16) if half else (np.float32, np.uint32)
    single = _device(twk, scene, half=half)
    for it in range(3):
        single.render(it)
    full = single.getOutputBufferHalf() if half else single.getOutputBufferHost()
    single.close()
    for n in (2, 3):
        nbytes = res[0] * res[1] * px
        host, mapped = C.c_void_p(), C.c_void_p()
        assert hip.hipHostMalloc(C.byref(host), C.c_size_t(nbytes), C.c_uint(0x2 | 0x1)) == 0  # hipHostMallocMapped | Portable
        assert hip.hipHostGetDevicePointer(C.byref(mapped), host, C.c_uint(0)) == 0
        C.memset(host, 0, nbytes)
        handles = []
        for i in range(n):
            d = _device(twk, scene, half=half, index=i, count=n)
            d.setSharedFrame(mapped.value, nbytes)
            handles.append(d)
        for it in range(3):
            for d in handles:
                d.render(it)
        for d in handles:
            d.synchronizeStream()
        frame = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint8)), shape=(nbytes,)).view(dtype).reshape(res[1], res[0], 4).copy()
        assert np.array_equal(frame.view(view), full.view(view)), f"pinned shared frame of {n} handles differs ({'half' if half else 'float'})"
        read = handles[0].getOutputBufferHalf() if half else handles[0].getOutputBufferHost()
        assert np.array_equal(read.view(view), full.view(view))
        for d in handles:
            d.close()
        assert hip.hipHostFree(host) == 0


def test_tonemap_of_half_buffers(twk):
    """twk_tonemap of the handle's half buffer and twk_tonemap_half of a composited half frame give the bytes twk_tonemap
    gives for the widened float copy uploaded as RGBA32F."""
    res = (200, 120)
    scene = _cornell(twk, res)
    app = scene[0]
    tm = app.tonemapper
    tm.gamma, tm.saturation, tm.crushBlacks = 2.2, 1.2, 0.2
    dev = _device(twk, scene, half=True)
    for it in range(3):
        dev.render(it)
    widened = dev.getOutputBufferHost()
    fbuf = _DeviceBuffer(twk, widened.nbytes)
    fbuf.upload(widened)
    expect = dev.tonemap(tm, fbuf.ptr.value, shape=widened.shape[:2])
    assert np.array_equal(dev.tonemap(tm), expect)
    dev.close()
    fbuf.free()

    comp, frame = _composited_half(twk, scene, 2, 3)
    img = frame.download((res[1], res[0], 4), np.float16)
    fbuf = _DeviceBuffer(twk, img.size * 4)
    fbuf.upload(img.astype(np.float32))
    expect = comp.tonemap(tm, fbuf.ptr.value, shape=img.shape[:2])
    got = comp.tonemap(tm, frame.ptr.value, shape=img.shape[:2], half=True)
    assert np.array_equal(got, expect) and got.max() > 0
    comp.close()
    frame.free()
    fbuf.free()


def test_format_switch(twk):
    """The reported buffer size halves; an external buffer too small for RGBA32F is refused on the switch back; switching back
    to float gives the float image bit for bit; setting the current format again is a no-op."""
    scene = _cornell(twk, (96, 64))
    dev = _device(twk, scene, half=False)
    for it in range(3):
        dev.render(it)
    float_image = dev.getOutputBufferHost()
    _, nbytes = dev.outputDevicePointer()
    assert nbytes == 96 * 64 * 16
    dev.setOutputFormat(HALF)
    dev.setOutputFormat(HALF)  # no-op
    _, half_bytes = dev.outputDevicePointer()
    assert half_bytes * 2 == nbytes and dev.outputFormat == HALF
    assert not dev.getOutputBufferHost().any()  # reallocated, zeroed
    for it in range(3):
        dev.render(it)
    assert np.isfinite(dev.getOutputBufferHalf()).all()
    small = _DeviceBuffer(twk, half_bytes)
    dev.setOutputDevicePointer(small.ptr.value, half_bytes)
    with pytest.raises(twk.TwkError) as e:
        dev.setOutputFormat(0)
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_STATE and "twk_set_output_format" in str(e.value)
    assert dev.outputFormat == HALF
    with pytest.raises(twk.TwkError) as e:
        dev.setOutputFormat(2)
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_VALUE
    dev.setOutputDevicePointer(0, 0)
    dev.setOutputFormat(0)
    with pytest.raises(twk.TwkError) as e:
        dev.setOutputDevicePointer(small.ptr.value, half_bytes)  # 8 bytes per pixel: too small for RGBA32F
    assert e.value.code == twk._lib.TWK_ERROR_INVALID_VALUE
    small.free()
    for it in range(3):
        dev.render(it)
    assert np.array_equal(_f32_bits(dev.getOutputBufferHost()), _f32_bits(float_image))
    dev.close()


def test_command_line_with_output_format_1(twk, tmp_path):
    """rtigo3_hip with `outputFormat 1` runs its benchmark and writes the PNG of the tonemapped half image."""
    from test_gpu_screenshot import _run_cli
    _, png = _run_cli(tmp_path, 0, extra="outputFormat 1\n")
    assert png.shape == (64, 96, 3) and png.max() > 0
    system = tmp_path / "system_0.txt"
    app = twk.Application(str(system), scene_path("scene_rtigo3_cornell_box.txt"))
    assert app.outputFormat == HALF
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    assert dev.outputFormat == HALF
    for it in range(4):
        dev.render(it)
    assert np.array_equal(dev.tonemap(app.tonemapper)[::-1], png)
    dev.close()
