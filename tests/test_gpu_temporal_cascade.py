"""-m gpu: the firefly cascade's layers through the temporal merge — twk_temporal_accumulate_cascade (explicit buffers) and
twk_temporal_enable_cascade (the handle's own layers, merged by the own-buffer twk_temporal_accumulate).

csrc/temporal_cascade_device.h defines it operation by operation; tests/temporal_cascade_restate.py restates it in numpy float32:
the device's merged layers must equal the restatement in every bit. The own-buffer form must equal the explicit form driven by
hand and leave the colour and moments of twk_temporal_accumulate what they are; and on a moving camera the resolve of the merged
layers must beat both the resolve of one frame's layers and the merged plain colour."""
import numpy as np
import pytest

import cascade_restate
from conftest import load_app
from temporal_cascade_restate import BRANCHES, F, U32, restate_temporal_cascade, synthetic_layers
from temporal_restate import camera_array
from test_gpu_denoise import _cornell, _errors
from test_gpu_denoise_sampled import _rendered
from test_gpu_denoise_variance import _small_device, _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_temporal import _camera, _frame, _moved

pytestmark = pytest.mark.gpu


def _same(got, expect, what):
    assert got.shape == expect.shape and got.dtype == expect.dtype == F, what
    diff = got.view(U32) != expect.view(U32)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} words differ, first at {np.argwhere(diff)[:4].tolist()}"


@pytest.mark.parametrize("K", [2, 6, 8])
@pytest.mark.parametrize("width,height", [(37, 23), (64, 4)])
def test_explicit_buffers_equal_the_restatement_bit_for_bit(twk, width, height, K):
    """The existing temporal tests' shapes — 37x23 (no multiple of a wave or a block, four blocks) and 64x4 (one block, rows shorter
    than a block: most reprojections leave the picture) — with 2 layers (the two the kernel keeps in registers and nothing between),
    6 (the default) and 8 (every predicated layer in use). At 37x23 every branch of the definition is counted and none is empty."""
    L = twk._lib
    Lc, g, (Hl, hg), cam, max_history, tolerance, _ = synthetic_layers(width, height, K)
    info = {}
    expect, took = restate_temporal_cascade(Lc, g, (Hl, hg), cam, max_history, tolerance, info)
    if (width, height) == (37, 23):
        for branch in BRANCHES:
            assert info[branch] > 0, (branch, info)
    assert took.sum() > 20 and (~took).sum() > 20
    dev = _small_device(twk)
    buffers = _upload(twk, (Lc, g, Hl, hg))
    out = _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    tp, cp, camera = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.Cascade(K, 1.0, 8.0), _camera(twk, cam)
    shape = (height, width)
    what = f"{width}x{height}, {K} layers"
    dev.temporalAccumulateCascade(tp, cp, p[0], p[1], p[2], p[3], camera, shape, out.ptr.value)
    dev.synchronizeStream()
    got = out.download(Lc.shape, F)
    _same(got, expect, what)
    # a pixel without history returns the input's bits, NaN payloads and the unused .w of the inner layers included
    assert np.array_equal(got.view(U32)[:, ~took], Lc.view(U32)[:, ~took])
    # no history: every pixel passes through; the history's geometry and camera are not looked at
    dev.temporalAccumulateCascade(tp, cp, p[0], p[1], None, None, None, shape, out.ptr.value)
    dev.synchronizeStream()
    _same(out.download(Lc.shape, F), Lc, what + ", no history")
    if K == L.TWK_CASCADE_LAYERS:  # the defaults are what NULL parameters mean
        dev.temporalAccumulateCascade(L.Temporal(), L.Cascade(), p[0], p[1], p[2], p[3], camera, shape, out.ptr.value)
        dev.synchronizeStream()
        with_defaults = out.download(Lc.shape, F)
        _same(with_defaults, restate_temporal_cascade(Lc, g, (Hl, hg), cam, L.TWK_TEMPORAL_MAX_HISTORY, L.Temporal().positionTolerance)[0], what + ", the defaults")
        dev.temporalAccumulateCascade(None, None, p[0], p[1], p[2], p[3], camera, shape, out.ptr.value)
        dev.synchronizeStream()
        _same(out.download(Lc.shape, F), with_defaults, what + ", NULL parameters")
    for buf, arr in zip(buffers, (Lc, g, Hl, hg)):
        _same(buf.download(arr.shape, F), arr, "an input after twk_temporal_accumulate_cascade")
    for buf in buffers + [out]:
        buf.free()
    dev.close()


def test_refusals(twk):
    L = twk._lib
    INVALID_VALUE, INVALID_STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, call, name="twk_temporal_accumulate_cascade"):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == code and name in str(e.value), str(e.value)

    width, height, K = 37, 23, 6
    Lc, g, (Hl, hg), cam, _, _, _ = synthetic_layers(width, height, K)
    shape = (height, width)
    dev = _small_device(twk)
    buffers = _upload(twk, (Lc, g, Hl, hg))
    out = _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    o = out.ptr.value
    camera = _camera(twk, cam)
    merge = lambda tp=None, cp=None, a=p[0], b=p[1], c=p[2], d=p[3], e=camera, s=shape, out_=o: dev.temporalAccumulateCascade(tp, cp, a, b, c, d, e, s, out_)
    merge()
    refused(INVALID_VALUE, lambda: merge(a=None))
    refused(INVALID_VALUE, lambda: merge(b=None))
    refused(INVALID_VALUE, lambda: merge(out_=None))
    refused(INVALID_VALUE, lambda: merge(d=None))   # history layers without their geometry
    refused(INVALID_VALUE, lambda: merge(e=None))   # ... without their camera
    for k, nbytes in zip(range(4), (Lc.nbytes, g.nbytes, Hl.nbytes, hg.nbytes)):  # the output overlaps an input, at its start and at its last pixel
        refused(INVALID_VALUE, lambda: merge(out_=p[k]))
        refused(INVALID_VALUE, lambda: merge(out_=p[k] + nbytes - 16))
        refused(INVALID_VALUE, lambda: merge(out_=p[k] - Lc.nbytes + 16))
    for cp in (L.Cascade(1, 1.0, 8.0), L.Cascade(9, 1.0, 8.0), L.Cascade(6, 0.0, 8.0), L.Cascade(6, float("inf"), 8.0), L.Cascade(6, 1.0, 1.0),
               L.Cascade(6, 1.0, float("nan")), L.Cascade(8, 1e30, 1e3)):  # the TwkCascade parameter rules
        refused(INVALID_VALUE, lambda: merge(cp=cp))
    refused(INVALID_VALUE, lambda: merge(tp=L.Temporal(maxHistory=0)))
    refused(INVALID_VALUE, lambda: merge(tp=L.Temporal(positionTolerance=-0.1)))
    refused(INVALID_VALUE, lambda: merge(tp=L.Temporal(positionTolerance=float("nan"))))
    for bad in ([0] * 12, list(cam[:3]) + [1, 0, 0, 0, 1, 0, 2, 0, 0], list(cam[:3]) + [float("nan")] * 9, list(cam[:9]) + [float("inf"), 0, 0]):  # a degenerate camera
        refused(INVALID_VALUE, lambda: merge(e=_camera(twk, np.array(bad, F))))
    refused(INVALID_VALUE, lambda: merge(s=(0, width)))
    refused(INVALID_VALUE, lambda: merge(s=(height, 0)))
    refused(INVALID_VALUE, lambda: merge(s=(1 << 14, 1 << 15)))  # above 2^28 pixels: refused before anything is launched
    for buf in buffers + [out]:
        buf.free()
    # the switch needs the cascade; the own-buffer twk_temporal_accumulate with the switch on needs it too
    refused(INVALID_STATE, lambda: dev.enableTemporalCascade(True), "twk_temporal_enable_cascade")
    refused(INVALID_STATE, lambda: dev.readTemporalCascade(), "twk_read_temporal_cascade")
    refused(INVALID_STATE, lambda: dev.temporalCascadeDevicePointer(), "twk_get_temporal_cascade_device_pointer")
    dev.enableCascade(True)
    dev.enableTemporalCascade(True)
    refused(INVALID_STATE, lambda: dev.temporalAccumulate(), "twk_temporal_accumulate")   # the existing refusals stay: no moments
    dev.enableMoments(True)
    dev.enableGeometry(True)
    dev.render(0)
    refused(INVALID_STATE, lambda: dev.temporalAccumulate(), "twk_temporal_accumulate")   # the geometry is not rendered
    dev.renderGeometry()
    dev.temporalAccumulate()
    assert dev.readTemporalCascade().shape == (6, 32, 32, 4)
    dev.enableCascade(False)
    refused(INVALID_STATE, lambda: dev.readTemporalCascade(), "twk_read_temporal_cascade")  # dropped with the cascade
    refused(INVALID_STATE, lambda: dev.temporalAccumulate(), "twk_temporal_accumulate")    # the switch is on, the cascade is off
    dev.enableTemporalCascade(False)
    dev.temporalAccumulate()                                                                # off: as ever
    refused(INVALID_STATE, lambda: dev.readTemporalCascade(), "twk_read_temporal_cascade")
    dev.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_own_buffers_equal_the_explicit_form_and_leave_colour_and_moments_alone(twk, half):
    """C2 at 61x37, three frames of 4 spp a small orbit step apart, in both output formats of the handle (the layers are f32 in
    both). The first call has no history of layers and copies the frame's through; the second and third equal the explicit form
    driven by hand on the handle's own current layers and geometry with the previous call's output, geometry and camera as history,
    and the restatement. A second handle runs the same frames with the switch off: its merged colour and moments are the same bytes.
    After twk_temporal_reset, and after twk_enable_cascade with new parameters, the next call passes the frame's layers through."""
    L = twk._lib
    res, spp = (61, 37), 4
    shape = (res[1], res[0])
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    cams = [app.cameras[0], _moved(twk, app, 0.004), _moved(twk, app, 0.008)]
    dev, plain = (_rendered(twk, 0, half=half, res=res) for _ in range(2))
    for d in (dev, plain):
        d.enableGeometry(True)
    dev.enableCascade(True)
    dev.enableTemporalCascade(True)
    previous, took_any = None, 0
    for frame, cam in enumerate(cams):
        for d in (dev, plain):
            d.updateCamera(0, cam)
            _frame(d, frame * spp, spp)
        layers, g = dev.readCascade(), dev.readGeometry()
        assert (layers[0, ..., 3] == spp).all()
        dev.temporalAccumulate(tp)
        plain.temporalAccumulate(tp)
        own = dev.readTemporalCascade()
        ptr, nbytes = dev.temporalCascadeDevicePointer()
        assert ptr and nbytes == layers.nbytes
        assert np.array_equal(dev.readTemporal().view(U32), plain.readTemporal().view(U32)), f"frame {frame}: the merged colour with the switch on"
        assert np.array_equal(dev.readTemporalMoments().view(U32), plain.readTemporalMoments().view(U32)), f"frame {frame}: the merged moments with the switch on"
        _same(dev.readCascade(), layers, "the handle's own layers after the merge")
        if previous is None:
            _same(own, layers, "the first call copies the frame's layers through")
        else:
            hl, hg, hcam = previous
            expect, took = restate_temporal_cascade(layers, g, (hl, hg), camera_array(hcam), 32, 0.1)
            took_any += int(took.sum())
            assert took.mean() > 0.5
            _same(own, expect, f"frame {frame}: own buffers against the restatement")
            history = _upload(twk, (hl, hg))
            out = _DeviceBuffer(twk, layers.nbytes)
            dev.temporalAccumulateCascade(tp, None, dev.cascadeDevicePointer()[0], dev.geometryDevicePointer()[0], history[0].ptr.value, history[1].ptr.value, hcam, shape, out.ptr.value)
            dev.synchronizeStream()
            _same(out.download(layers.shape, F), own, f"frame {frame}: the explicit form driven by hand against the own-buffer form")
            for buf in history + [out]:
                buf.free()
        previous = (own, g, cam)
    assert own[0, ..., 3].max() > 2 * spp + 1 and own[0, ..., 3].max() < 3 * spp + 0.001, "n grows with the frames, below 3 x spp"
    # the merged layers feed the resolve's explicit form as they are
    resolved = _DeviceBuffer(twk, res[0] * res[1] * (8 if half else 16))
    dev.cascadeResolve(L.Cascade(), L.CascadeResolve(), layers=ptr, shape=shape, resolved=resolved.ptr.value)
    dev.synchronizeStream()
    expect = cascade_restate.resolve(own, cascade_restate.thresholds(), L.TWK_CASCADE_KAPPA)
    got = resolved.download(expect.shape, np.float16 if half else F)
    with np.errstate(over="ignore"):
        assert np.array_equal(got, expect.astype(got.dtype)), "twk_cascade_resolve on the merged layers"
    resolved.free()
    # a reset drops the layers with the rest of the history; the next call passes the frame's through
    dev.temporalReset()
    with pytest.raises(twk.TwkError) as e:
        dev.readTemporalCascade()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE
    dev.temporalAccumulate(tp)
    _same(dev.readTemporalCascade(), dev.readCascade(), "after twk_temporal_reset the next call is a pass-through")
    # new cascade parameters drop them too (the temporal history of colour and moments stays)
    dev.enableCascade(True, L.Cascade(4, 0.5, 4.0))
    with pytest.raises(twk.TwkError) as e:
        dev.readTemporalCascade()
    assert e.value.code == L.TWK_ERROR_INVALID_STATE
    _frame(dev, 3 * spp, spp)
    dev.temporalAccumulate(tp)
    assert dev.readTemporalMoments()[..., 2].max() > spp, "the colour and moments still had their history"
    _same(dev.readTemporalCascade(), dev.readCascade(), "after new cascade parameters the next call is a pass-through")
    assert dev.readTemporalCascade().shape[0] == 4
    dev.close()
    plain.close()


def test_the_resolve_of_the_merged_layers_beats_one_frames_resolve_and_the_merged_plain_colour(twk):
    """C2 at 160x90, Optix7Gui rule, the orbit of tools/temporal_cascade_sweep.py: 8 frames 0.002 of a turn apart, 4 spp each with
    the sample offset advancing by 4, maxHistory 32, positionTolerance 0.1 (the tolerance of tests/test_gpu_temporal.py at this
    size), against 512 spp from the last camera seeded as iterations 32 .. 543 (no sample shared with the orbit). In per-pixel
    relative RMSE the resolve of the merged layers must be strictly below both the resolve of the last frame's own layers and the
    merged plain colour. kappa is the default, 32: the CPU sweep (profiles/r18_temporal_cascade.md) has the condition hold at 8, 16
    and 32 and widest at 32 — 0.280 against 0.358 and 0.377."""
    L = twk._lib
    res, frames, spp, step = (160, 90), 8, 4, 0.002
    shape = (res[1], res[0])
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    reference = _cornell(twk, 0, aov=False)
    reference.updateCamera(0, _moved(twk, app, step * (frames - 1)))
    reference.setSampleOffset(frames * spp)
    for it in range(512):
        reference.render(it)
    r = reference.getOutputBufferHost()
    reference.close()
    dev = _rendered(twk, 0, res=res)
    dev.enableGeometry(True)
    dev.enableCascade(True)
    dev.enableTemporalCascade(True)
    for frame in range(frames):
        dev.updateCamera(0, _moved(twk, app, step * frame))
        _frame(dev, frame * spp, spp)
        dev.temporalAccumulate(tp)
    dev.cascadeResolve()
    own = dev.readResolved()
    merged_plain = dev.readTemporal()
    ptr, _ = dev.temporalCascadeDevicePointer()
    out = _DeviceBuffer(twk, r.nbytes)
    dev.cascadeResolve(L.Cascade(), L.CascadeResolve(), layers=ptr, shape=shape, resolved=out.ptr.value)
    dev.synchronizeStream()
    merged = out.download(r.shape, F)
    n = dev.readTemporalCascade()[0, ..., 3]
    out.free()
    dev.close()
    e_own, e_plain, e_merged = _errors(own, r), _errors(merged_plain, r), _errors(merged, r)
    print(f"\nrelative RMSE / per-pixel relative RMSE against 512 spp, kappa {L.TWK_CASCADE_KAPPA:g}: resolve of the last frame's own layers {e_own[0]:.4f} / {e_own[1]:.4f}, "
          f"merged plain colour {e_plain[0]:.4f} / {e_plain[1]:.4f}, resolve of the merged layers {e_merged[0]:.4f} / {e_merged[1]:.4f}; mean merged n {n.mean():.1f}")
    assert e_merged[1] < e_own[1], "against the resolve of the last frame's own layers"
    assert e_merged[1] < e_plain[1], "against the merged plain colour"
