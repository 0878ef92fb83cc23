"""-m gpu: twk_temporal_accumulate_rectified — the temporal merge with a per-pixel trust in its reprojected history
(csrc/temporal_rectify_device.h), against the numpy float32 restatement tests/temporal_rectify_restate.py: the device's four outputs
equal it in every bit, in both output formats, at sizes that leave partial tiles, put the halo over every border, span several tiles
and are smaller than one; a test that never runs gives the bytes of twk_temporal_accumulate; and the own-buffer form notices a light
that twk_update_light has halved."""
import numpy as np
import pytest

from conftest import load_app
from temporal_rectify_restate import BRANCHES, expect_rectify, rectify_frames
from temporal_restate import F, camera_array
from test_gpu_denoise_sampled import _rendered
from test_gpu_denoise_variance import _small_device, _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_temporal import _camera, _frame, _moved, _same

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (70, 20), (8, 8), (1, 1)]


def _run(twk, dev, tp, rp, arrays, history=True):
    """The explicit form on uploaded frames: (colourOut, historyOut, momentsOut, trustOut) downloaded."""
    L = twk._lib
    cur, mc, g, hc, hm, hg, cam = arrays
    height, width = mc.shape[:2]
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg))
    outs = [_DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, hc.nbytes), _DeviceBuffer(twk, hm.nbytes), _DeviceBuffer(twk, width * height * 4)]
    p = [b.ptr.value for b in buffers]
    current = L.TemporalFrame(p[0], p[1], p[2])
    hist = L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam)) if history else None
    dev.temporalAccumulateRectified(tp, rp, current, hist, (height, width), *(b.ptr.value for b in outs))
    dev.synchronizeStream()
    got = (outs[0].download(cur.shape, cur.dtype), outs[1].download(hc.shape, F), outs[2].download(hm.shape, F), outs[3].download((height, width), F))
    for buf, arr in zip(buffers, (cur, mc, g, hc, hm, hg)):
        _same(buf.download(arr.shape, arr.dtype), arr, "an input after twk_temporal_accumulate_rectified")
    for buf in buffers + outs:
        buf.free()
    return got


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
@pytest.mark.parametrize("width,height", SIZES)
def test_explicit_buffers_equal_the_restatement_bit_for_bit(twk, width, height, half):
    """Radii 1, 3 and 4 on one device per size and format; minTaps as tests/test_temporal_rectify_host.py chooses it, so that every
    branch of the test is reached at the two larger sizes."""
    L = twk._lib
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance = rectify_frames(width, height)
    if half:
        with np.errstate(over="ignore"):
            cur = cur.astype(np.float16)
    dev = _small_device(twk, half)
    tp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance)
    for radius, min_taps in ((1, 4), (3, 20), (4, 30)):
        info = {}
        expect = expect_rectify(cur, mc, g, (hc, hm, hg), cam, max_history, tolerance, radius, min_taps, 3.0, info)
        if width * height > 500:
            for branch in BRANCHES:
                assert info[branch] > 0, (branch, info)
        got = _run(twk, dev, tp, L.TemporalRectify(radius, min_taps, 3.0), (cur, mc, g, hc, hm, hg, cam))
        what = f"{width}x{height}, {'rgba16f' if half else 'rgba32f'}, radius {radius}"
        for k, name in enumerate(("colourOut", "historyOut", "momentsOut", "trustOut")):
            _same(got[k], expect[k], f"{what}, {name}")
    # no history: the frame passes through and nothing was tested
    got = _run(twk, dev, tp, None, (cur, mc, g, hc, hm, hg, cam), history=False)
    _same(got[0], cur, "no history: colourOut")
    _same(got[1], cur.astype(F), "no history: historyOut")
    _same(got[2], mc, "no history: momentsOut")
    assert (got[3] == 1).all()
    dev.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_a_test_that_never_runs_gives_the_bytes_of_the_plain_merge(twk, half):
    """minTaps = 50 at radius 3 (a window has 49 taps): colourOut, historyOut and momentsOut are those of twk_temporal_accumulate ON
    THE DEVICE, the trust is 1 everywhere."""
    L = twk._lib
    width, height = 37, 23
    (cur, mc, g), (hc, hm, hg), cam, max_history, tolerance = rectify_frames(width, height)
    if half:
        with np.errstate(over="ignore"):
            cur = cur.astype(np.float16)
    dev = _small_device(twk, half)
    tp = L.Temporal(maxHistory=max_history, positionTolerance=tolerance)
    got = _run(twk, dev, tp, L.TemporalRectify(3, 50, 3.0), (cur, mc, g, hc, hm, hg, cam))
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg))
    outs = [_DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, hc.nbytes), _DeviceBuffer(twk, hm.nbytes)]
    p = [b.ptr.value for b in buffers]
    dev.temporalAccumulate(tp, L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam)), (height, width), *(b.ptr.value for b in outs))
    dev.synchronizeStream()
    plain = (outs[0].download(cur.shape, cur.dtype), outs[1].download(hc.shape, F), outs[2].download(hm.shape, F))
    for k, name in enumerate(("colourOut", "historyOut", "momentsOut")):
        _same(got[k], plain[k], name + " against twk_temporal_accumulate")
    assert (plain[2][..., 2] > mc[..., 2]).sum() > 100, "the plain merge took history"
    assert (got[3] == 1).all()
    for buf in buffers + outs:
        buf.free()
    dev.close()


def test_refusals(twk):
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, call, *words):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and "twk_temporal_accumulate_rectified" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    width, height = 37, 23
    (cur, mc, g), (hc, hm, hg), cam, _, _ = rectify_frames(width, height)
    shape = (height, width)
    dev = _small_device(twk)
    buffers = _upload(twk, (cur, mc, g, hc, hm, hg))
    out, trust = _DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, width * height * 4)
    p = [b.ptr.value for b in buffers]
    current, history = L.TemporalFrame(p[0], p[1], p[2]), L.TemporalFrame(p[3], p[4], p[5], _camera(twk, cam))
    merge = lambda rp=None, tp=None, c=current, h=history, s=shape, outs=(out.ptr.value, None, None, trust.ptr.value): dev.temporalAccumulateRectified(tp, rp, c, h, s, *outs)
    merge()
    for rp, word in ((L.TemporalRectify(radius=0), "radius"), (L.TemporalRectify(radius=5), "radius"), (L.TemporalRectify(minTaps=1), "minTaps"),
                     (L.TemporalRectify(gamma=-1.0), "gamma"), (L.TemporalRectify(gamma=float("nan")), "gamma"), (L.TemporalRectify(gamma=float("inf")), "gamma")):
        refused(VALUE, lambda: merge(rp), word)
    refused(VALUE, lambda: merge(tp=L.Temporal(maxHistory=0)), "maxHistory")
    refused(VALUE, lambda: merge(tp=L.Temporal(positionTolerance=-0.1)), "positionTolerance")
    for k in range(6):  # the trust overlaps an input; an output overlaps an input
        refused(VALUE, lambda: merge(outs=(None, None, None, p[k])), "overlaps")
        refused(VALUE, lambda: merge(outs=(p[k], None, None, None)), "overlaps")
    refused(VALUE, lambda: merge(outs=(out.ptr.value, None, None, out.ptr.value + 16)), "two outputs overlap")
    refused(VALUE, lambda: merge(h=L.TemporalFrame(p[3], p[4], p[5], _camera(twk, np.zeros(12, F)))), "degenerate")
    refused(VALUE, lambda: merge(c=L.TemporalFrame(p[0], None, p[2])), "NULL")
    refused(VALUE, lambda: merge(h=L.TemporalFrame(p[3], p[4], None, _camera(twk, cam))), "NULL")
    refused(VALUE, lambda: merge(s=(0, width)), "width and height")
    refused(VALUE, lambda: dev.temporalAccumulateRectified(None, None, None, history))                                    # a history without a frame
    refused(VALUE, lambda: dev.temporalAccumulateRectified(None, None, None, None, None, None, None, None, trust.ptr.value))  # a trust output in the own-buffer form
    for buf in buffers + [out, trust]:
        buf.free()
    # the own-buffer form: the refusals of twk_temporal_accumulate's, and the trust plane's readers
    refused(STATE, lambda: dev.temporalAccumulateRectified(), "twk_enable_moments")
    dev.enableMoments(True)
    dev.render(0)
    refused(STATE, lambda: dev.temporalAccumulateRectified(), "twk_enable_geometry")
    dev.enableGeometry(True)
    refused(STATE, lambda: dev.temporalAccumulateRectified(), "twk_render_geometry")
    dev.renderGeometry()
    with pytest.raises(twk.TwkError) as e:
        dev.readTemporalTrust()
    assert e.value.code == STATE and "twk_read_temporal_trust" in str(e.value)
    dev.temporalAccumulateRectified()
    assert (dev.readTemporalTrust() == 1).all() and dev.temporalTrustDevicePointer()[1] == 32 * 32 * 4
    dev.temporalAccumulate()  # a plain merge on the same history: the trust plane is an earlier frame's
    with pytest.raises(twk.TwkError) as e:
        dev.temporalTrustDevicePointer()
    assert e.value.code == STATE and "twk_get_temporal_trust_device_pointer" in str(e.value)
    dev.temporalAccumulateRectified()
    dev.temporalReset()
    with pytest.raises(twk.TwkError):
        dev.readTemporalTrust()
    dev.close()
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (32, 32))
    tile = twk.Device(ordinal=0, index=0, count=2, miss=app.info.miss)
    app.initDevice(tile, distribution=1)
    tile.enableMoments(True)
    tile.enableGeometry(True)
    tile.render(0)
    refused(STATE, lambda: tile.temporalAccumulateRectified(), "packed tile")
    tile.close()


def _orbit(twk, halve, half=False):
    """C2 at 61x37 (the smallest Cornell frame the temporal tests use), three frames of 4 spp 0.004 of a turn apart through the
    own-buffer form; halve: twk_update_light halves the emission before the third. After every frame the handle's merged colour,
    moments and trust equal the restatement of the inputs read back — the frame's buffers, and as history what the merge before kept
    (its f32 historyOut, which the RGBA16F result does not show: the restatement's, once the frame before has been found equal).
    Returns (the third frame's geometry, its trust)."""
    L = twk._lib
    res, spp = (61, 37), 4
    tp, rp = L.Temporal(maxHistory=32, positionTolerance=0.1), L.TemporalRectify()
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    dev = _rendered(twk, 0, half=half, res=res)
    dev.enableGeometry(True)
    raw = lambda: dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()
    cameras = [app.cameras[0], _moved(twk, app, 0.004), _moved(twk, app, 0.008)]
    kept = None
    for f in range(3):
        dev.updateCamera(0, cameras[f])
        if f == 2 and halve:
            (light,) = app.lights
            for k in range(3):
                light.emission[k] = light.emission[k] * 0.5
            dev.updateLight(0, light)
        _frame(dev, f * spp, spp)
        colour_raw, mc, g = raw(), dev.readMoments(), dev.readGeometry()
        dev.temporalAccumulateRectified(tp, rp)
        expect = expect_rectify(colour_raw, mc, g, kept, camera_array(cameras[f - 1]) if f else None, 32, 0.1, rp.radius, rp.minTaps, rp.gamma)
        what = f"frame {f}, emission {'halved' if halve else 'unchanged'}"
        _same(dev.readTemporal(), expect[0].astype(F), what + ": colour")
        _same(dev.readTemporalMoments(), expect[2], what + ": moments")
        trust = dev.readTemporalTrust()
        _same(trust, expect[3], what + ": trust")
        if not half:
            _same(expect[1], dev.readTemporal(), what + ": in RGBA32F the history kept is the colour read back")
        assert expect[4].any() == (f > 0)
        kept = (expect[1], expect[2], g)
    dev.close()
    return g, trust


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_own_buffers_notice_a_halved_light(twk, half):
    """Three frames, each merge equal to the restatement in colour, moments and trust; and the mean trust of the third merge over the
    pixels that hit something is lower with the emission halved before it than in the same run without the update."""
    means = {}
    for halve in (False, True):
        g, trust = _orbit(twk, halve, half)
        hit = g[..., 3].view(np.uint32) != 0
        assert hit.mean() > 0.5
        means[halve] = float(trust[hit].mean())
    print(f"\nmean trust over hit pixels: lighting unchanged {means[False]:.4f}, emission halved {means[True]:.4f}")
    assert means[True] < means[False]
