"""-m gpu: twk_temporal_accumulate — the last frame's colour and luminance moments reprojected through the previous camera and merged
with this frame's samples by sample count (the temporal half of SVGF, Schied et al. 2017, section 4.1).

csrc/temporal_device.h defines it operation by operation; tests/temporal_restate.py restates it in numpy float32: the device's three
outputs must equal the restatement in every bit, in both output formats, on frames that reach every branch of the definition."""
import numpy as np
import pytest

from conftest import load_app
from temporal_restate import F, U32, camera_array, restate_temporal, synthetic_frames
from test_gpu_denoise import _errors
from test_gpu_denoise_sampled import _rendered
from test_gpu_denoise_variance import _small_device, _upload
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

HALF = 1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _same(got, expect, what):
    assert got.shape == expect.shape and got.dtype == expect.dtype, what
    diff = _bits(got) != _bits(expect)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} words differ, first at {np.argwhere(diff)[:4].tolist()}"


def _camera(twk, cam12):
    c = twk.CameraDefinition()
    for k in range(3):
        c.P[k], c.U[k], c.V[k], c.W[k] = (float(cam12[3 * j + k]) for j in range(4))
    return c


def _expect(colour_raw, moments, geometry, history, cam, max_history, tolerance, info=None):
    """The three outputs as the device writes them: (colourOut in the format of colour_raw, historyOut f32, momentsOut f32)."""
    colour, merged_moments, took = restate_temporal(colour_raw.astype(F), moments, geometry, history, cam, max_history, tolerance, info)
    narrow = colour
    if colour_raw.dtype == np.float16:
        with np.errstate(over="ignore"):
            narrow = colour.astype(np.float16)
    narrow[~took] = colour_raw[~took]
    return narrow, colour, merged_moments, took


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("width,height", [(37, 23), (64, 4)])
def test_explicit_buffers_equal_the_restatement_bit_for_bit(twk, width, height, half):
    """37x23 (no multiple of a wave or a block, five blocks) and 64x4 (one block, a picture four rows high: most reprojections leave
    it), in both formats. Every branch of the definition is counted and none is empty."""
    L = twk._lib
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance = synthetic_frames(width, height)
    if half:
        with np.errstate(over="ignore"):
            cur = cur.astype(np.float16)
    shape = (height, width)
    dev = _small_device(twk, half)
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg))
    outs = [_DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, hc.nbytes), _DeviceBuffer(twk, hm.nbytes)]
    p = [b.ptr.value for b in buffers]
    o = [b.ptr.value for b in outs]
    current, history = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    tp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance)
    info = {}
    colour, kept, moments, took = _expect(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, info)
    for branch in ("miss", "id_mismatch", "outside", "behind", "position", "current_not_finite", "current_n_below_1", "history_not_finite",
                   "capped", "uncapped", "one_tap", "four_taps", "took", "no_tap"):
        assert info[branch] > 0 or (branch == "no_tap" and height == 4), (branch, info)
    dev.temporalAccumulate(tp, current, history, shape, *o)
    dev.synchronizeStream()
    what = f"{width}x{height}, {'rgba16f' if half else 'rgba32f'}"
    got = [outs[0].download(cur.shape, cur.dtype), outs[1].download(hc.shape, F), outs[2].download(hm.shape, F)]
    _same(got[0], colour, what + ", colourOut")
    _same(got[1], kept, what + ", historyOut")
    _same(got[2], moments, what + ", momentsOut")
    # a pixel without history returns the input's bits, NaN payloads and the unread fourth word of the moments included
    assert (~took).sum() > 50
    assert np.array_equal(_bits(got[0])[~took], _bits(cur)[~took]) and np.array_equal(_bits(got[1])[~took], _bits(cur.astype(F))[~took])
    assert np.array_equal(_bits(got[2])[~took], _bits(mc)[~took])
    assert np.array_equal(_bits(got[1][..., 3]), _bits(cur.astype(F)[..., 3])), "alpha is the frame's"
    # each output alone (the others NULL) is the same; no history: the frame passes through
    for k in range(3):
        fresh = _DeviceBuffer(twk, outs[k].nbytes)
        only = [None, None, None]
        only[k] = fresh.ptr.value
        dev.temporalAccumulate(tp, current, history, shape, *only)
        dev.synchronizeStream()
        _same(fresh.download(got[k].shape, got[k].dtype), got[k], what + f", output {k} alone")
        fresh.free()
    dev.temporalAccumulate(tp, current, None, shape, *o)
    dev.synchronizeStream()
    _same(outs[0].download(cur.shape, cur.dtype), cur, what + ", no history: colourOut")
    _same(outs[1].download(hc.shape, F), cur.astype(F), what + ", no history: historyOut")
    _same(outs[2].download(hm.shape, F), mc, what + ", no history: momentsOut")
    # the defaults are what NULL parameters mean
    dev.temporalAccumulate(L.Temporal(), current, history, shape, *o)
    dev.synchronizeStream()
    with_defaults = outs[1].download(hc.shape, F)
    assert L.lib.twk_temporal_accumulate(dev.handle, None, L.C.byref(current), L.C.byref(history), width, height, *(L.C.c_void_p(x) for x in o)) == 0
    dev.synchronizeStream()
    _same(outs[1].download(hc.shape, F), with_defaults, "NULL parameters against twk_temporal_defaults")
    for buf, arr in zip(buffers, (cur, mc, g, hc, hm, hg)):
        _same(buf.download(arr.shape, arr.dtype), arr, "an input after twk_temporal_accumulate")
    for buf in buffers + outs:
        buf.free()
    dev.close()


def _moved(twk, app, dphi):
    """The application's camera a step of dphi (a fraction of the full turn) along its orbit."""
    i = app.info
    return twk.camera_frustum(tuple(i.center), i.phi + dphi, i.theta, i.fov, i.distance, i.resolution[0] / i.resolution[1])


def _frame(dev, offset, spp):
    dev.setSampleOffset(offset)
    for it in range(spp):
        dev.render(it)
    dev.renderGeometry()


def test_refusals(twk):
    L = twk._lib
    INVALID_VALUE, INVALID_STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, call):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and "twk_temporal_accumulate" in str(e.value), str(e.value)

    width, height = 37, 23
    (cur, mc, g), (hc, hm, hg), cam, _, _ = synthetic_frames(width, height)
    shape = (height, width)
    dev = _small_device(twk)
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg))
    out = _DeviceBuffer(twk, cur.nbytes)
    p = [b.ptr.value for b in buffers]
    current, history = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    dev.temporalAccumulate(None, current, history, shape, out.ptr.value)
    for k in range(6):  # an output that overlaps an input, at its start and at its last pixel
        refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, history, shape, p[k]))
        refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, history, shape, None, p[k] + cur.nbytes - 16))
        refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, history, shape, None, None, p[k] - cur.nbytes + 16))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, history, shape, out.ptr.value, out.ptr.value))  # two outputs overlap
    for bad in ([0] * 12, list(cam[:9]) + list(cam[3:6]), list(cam[:3]) + [float("nan")] * 9, list(cam[:9]) + [float("inf"), 0, 0]):  # a degenerate camera
        frame = L.TemporalFrame(p[3], p[4], p[5], _camera(twk, np.array(bad, F)))
        refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, frame, shape, out.ptr.value))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, L.TemporalFrame(p[0], None, p[2]), history, shape, out.ptr.value))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, L.TemporalFrame(p[3], p[4], None, _camera(twk, cam)), shape, out.ptr.value))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, current, history, (0, width), out.ptr.value))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, None, history))                       # a history without a frame
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(None, None, None, None, out.ptr.value))     # an output in the own-buffer form
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(L.Temporal(maxHistory=0), current, history, shape, out.ptr.value))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(L.Temporal(positionTolerance=-0.1), current, history, shape, out.ptr.value))
    refused(INVALID_VALUE, lambda: dev.temporalAccumulate(L.Temporal(positionTolerance=float("nan")), current, history, shape, out.ptr.value))
    for buf in buffers + [out]:
        buf.free()
    # the own-buffer form needs moments, a geometry AOV, and one rendered since the camera last changed
    refused(INVALID_STATE, lambda: dev.temporalAccumulate())
    dev.enableMoments(True)
    dev.render(0)
    refused(INVALID_STATE, lambda: dev.temporalAccumulate())            # no geometry
    dev.enableGeometry(True)
    refused(INVALID_STATE, lambda: dev.temporalAccumulate())            # not rendered
    dev.renderGeometry()
    dev.temporalAccumulate()
    dev.enableMoments(False)
    refused(INVALID_STATE, lambda: dev.temporalAccumulate())            # no moments
    dev.enableMoments(True)
    dev.render(0)
    dev.temporalAccumulate()
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    dev.updateCamera(0, _moved(twk, app, 0.01))
    refused(INVALID_STATE, lambda: dev.temporalAccumulate())            # the geometry is older than the camera
    dev.renderGeometry()
    dev.temporalAccumulate()
    dev.temporalReset()
    with pytest.raises(twk.TwkError) as e:
        dev.readTemporal()                                               # nothing kept
    assert e.value.code == INVALID_STATE and "twk_read_temporal" in str(e.value)
    dev.close()
    tile = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tile, distribution=1)
    tile.enableMoments(True)
    tile.enableGeometry(True)
    tile.render(0)
    refused(INVALID_STATE, lambda: tile.temporalAccumulate())           # a packed tile buffer
    tile.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_own_buffers_equal_the_explicit_form(twk, half):
    """C2 at 61x37, two frames of 4 spp a small orbit step apart: the first call has no history and copies the frame through; the
    second equals the explicit form fed the same buffers, and the restatement; after twk_temporal_reset the next call passes through."""
    L = twk._lib
    res, spp = (61, 37), 4
    shape = (res[1], res[0])
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    dev = _rendered(twk, 0, half=half, res=res)
    dev.enableGeometry(True)
    raw = lambda: dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()
    _frame(dev, 0, spp)
    first = (raw(), dev.readMoments(), dev.readGeometry())
    dev.temporalAccumulate(tp)
    _same(dev.readTemporal(), first[0].astype(F), "the first call copies the frame through")
    _same(dev.readTemporalMoments(), first[1], "... and its moments")
    assert (first[1][..., 2] == spp).all()
    cam0, cam1 = app.cameras[0], _moved(twk, app, 0.004)
    dev.updateCamera(0, cam1)
    _frame(dev, spp, spp)
    second = (raw(), dev.readMoments(), dev.readGeometry())
    dev.temporalAccumulate(tp)
    own_colour, own_moments = dev.readTemporal(), dev.readTemporalMoments()
    colour_ptr, colour_bytes, moments_ptr, moments_bytes = dev.temporalDevicePointers()
    assert colour_bytes == second[0].nbytes and moments_bytes == second[1].nbytes
    info = {}
    colour, kept, moments, took = _expect(*second, (first[0].astype(F), first[1], first[2]), camera_array(cam0), 32, 0.1, info)
    assert took.mean() > 0.5, info
    _same(own_colour, colour.astype(F), "own buffers against the restatement, colour")
    _same(own_moments, moments, "own buffers against the restatement, moments")
    # the explicit form on the handle's own current buffers and an uploaded history
    history_buffers = _upload(twk, (first[0].astype(F), first[1], first[2]))
    outs = [_DeviceBuffer(twk, second[0].nbytes), _DeviceBuffer(twk, second[1].nbytes), _DeviceBuffer(twk, second[1].nbytes)]
    current = L.TemporalFrame(dev.outputDevicePointer()[0], dev.momentsDevicePointer()[0], dev.geometryDevicePointer()[0], cam1)
    history = L.TemporalFrame(*(b.ptr.value for b in history_buffers), cam0)
    dev.temporalAccumulate(tp, current, history, shape, *(b.ptr.value for b in outs))
    dev.synchronizeStream()
    _same(outs[0].download(second[0].shape, second[0].dtype), colour, "explicit form, colourOut")
    _same(outs[0].download(second[0].shape, second[0].dtype).astype(F), own_colour, "explicit form against the own-buffer form")
    _same(outs[1].download(second[1].shape, F), kept, "explicit form, historyOut")
    _same(outs[2].download(second[1].shape, F), own_moments, "explicit form, momentsOut")
    # the result feeds the filter: the merged colour as beauty, the merged moments beside it
    dev.denoise(beauty=colour_ptr, albedo=None, normal=None, params=L.Denoiser(inputKind=0), shape=shape, moments=moments_ptr, minSamples=4)
    assert np.isfinite(dev.readDenoised(shape=shape)).all()
    # a third frame from the same camera merges with what the second call kept: n grows to the cap's side of 3 x spp
    _frame(dev, 2 * spp, spp)
    dev.temporalAccumulate(tp)
    third = dev.readTemporalMoments()
    expect3 = _expect(raw(), dev.readMoments(), dev.readGeometry(), (kept, moments, second[2]), camera_array(cam1), 32, 0.1)
    _same(third, expect3[2], "the third frame merges with the kept history")
    assert third[..., 2].max() > 2 * spp + 1 and third[..., 2].max() < 3 * spp + 0.001
    dev.temporalReset()
    with pytest.raises(twk.TwkError):
        dev.readTemporal()
    dev.temporalAccumulate(tp)
    _same(dev.readTemporal(), raw().astype(F), "after twk_temporal_reset the next call is a pass-through")
    _same(dev.readTemporalMoments(), dev.readMoments(), "... moments too")
    for buf in history_buffers + outs:
        buf.free()
    dev.close()


def test_it_accumulates_better(twk):
    """C2 at 96x54, two cameras a small orbit step apart, 4 spp each with sample offsets 0 and 4, against 256 spp from the second
    camera. On the pixels that took history the merged colour is strictly closer (relative RMSE) than the 4 spp frame, and
    Device.denoise(minSamples=4) on the merged colour and moments is strictly closer than the same call on the unmerged frame.
    The tolerance: a pixel of a 54-row picture at fov 60 is 2 tan(30 deg) / 54 = 0.021 of the distance wide on a surface that faces the
    camera, so the default (0.01, chosen at 1080 rows) would refuse every neighbouring tap; 0.1 is five such pixels."""
    L = twk._lib
    res, spp = (96, 54), 4
    shape = (res[1], res[0])
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    cam0, cam1 = app.cameras[0], _moved(twk, app, 0.004)
    reference = _rendered(twk, 0, res=res, moments=False)
    reference.updateCamera(0, cam1)
    for it in range(256):
        reference.render(it)
    r = reference.getOutputBufferHost()
    reference.close()
    dev = _rendered(twk, 0, res=res)
    dev.enableGeometry(True)
    _frame(dev, 0, spp)
    first = (dev.getOutputBufferHost(), dev.readMoments(), dev.readGeometry())
    dev.temporalAccumulate(tp)
    dev.updateCamera(0, cam1)
    _frame(dev, spp, spp)
    noisy, noisy_moments, geometry = dev.getOutputBufferHost(), dev.readMoments(), dev.readGeometry()
    dev.denoise(minSamples=4)
    filtered_alone = dev.readDenoised()
    dev.temporalAccumulate(tp)
    merged = dev.readTemporal()
    colour_ptr, _, moments_ptr, _ = dev.temporalDevicePointers()
    albedo, normal = _DeviceBuffer(twk, noisy.nbytes), _DeviceBuffer(twk, noisy.nbytes)
    albedo.upload(dev.readAov(0))
    normal.upload(dev.readAov(1))
    dev.denoise(beauty=colour_ptr, albedo=albedo.ptr.value, normal=normal.ptr.value, shape=shape, moments=moments_ptr, minSamples=4)
    filtered_merged = dev.readDenoised(shape=shape)
    info = {}
    _, _, took = restate_temporal(noisy, noisy_moments, geometry, first, camera_array(cam0), 32, 0.1, info)
    took_device = dev.readTemporalMoments()[..., 2] > noisy_moments[..., 2]
    assert int(took_device.sum()) == info["took"] and np.array_equal(took_device, took), "the share of pixels with history"
    share = took.mean()
    on = lambda img: _errors(img[took][None], r[took][None])[0]
    e_noisy, e_merged, e_alone, e_both = on(noisy), on(merged), on(filtered_alone), on(filtered_merged)
    print(f"\n{share:.3f} of the pixels took history; relative RMSE there against 256 spp: 4 spp {e_noisy:.4f}, merged {e_merged:.4f}, "
          f"4 spp filtered {e_alone:.4f}, merged and filtered {e_both:.4f}")
    assert share > 0.5
    assert e_merged < e_noisy
    assert e_both < e_alone
    albedo.free()
    normal.free()
    dev.close()
