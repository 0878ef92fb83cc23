"""-m gpu: the trusted build of the cascade's temporal merge — twk_temporal_accumulate_cascade_trusted against the host form
twk_temporal_cascade_trusted_host (the same header compiled for the host; tests/test_temporal_rectify_host.py holds it against the
numpy restatement) bit for bit, and the own-buffer form: with twk_temporal_enable_cascade(1), twk_temporal_accumulate_rectified
merges the handle's layers with the trust it has just written."""
import numpy as np
import pytest

from conftest import load_app
from temporal_cascade_restate import F, U32, synthetic_layers
from temporal_rectify_restate import restate_temporal_cascade_trusted
from temporal_restate import camera_array
from test_gpu_denoise_sampled import _rendered
from test_gpu_denoise_variance import _small_device, _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_temporal import _camera, _frame, _moved
from test_gpu_temporal_cascade import _same
from test_temporal_cascade_host import host_merge
from test_temporal_rectify_host import host_merge_trusted

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [2, 6, 8])
@pytest.mark.parametrize("width,height", [(37, 23), (64, 4)])
def test_the_device_equals_the_host_form_bit_for_bit(twk, width, height, K):
    """The shapes and layer counts of test_gpu_temporal_cascade, a random trust in [0, 1] with exact zeros and ones in it; then trust
    all 1, which must give the bytes of twk_temporal_accumulate_cascade on the device."""
    L = twk._lib
    Lc, g, (Hl, hg), cam, max_history, tolerance, _ = synthetic_layers(width, height, K)
    rng = np.random.default_rng(17 + K)
    trust = rng.uniform(0.0, 1.0, (height, width)).astype(F)
    trust[rng.uniform(size=trust.shape) < 0.1] = 0
    trust[rng.uniform(size=trust.shape) < 0.1] = 1
    expect = host_merge_trusted(twk, Lc, g, (Hl, hg), cam, max_history, tolerance, K, trust)
    assert not np.array_equal(expect.view(U32), host_merge(twk, Lc, g, (Hl, hg), cam, max_history, tolerance, K).view(U32))
    dev = _small_device(twk)
    ones = np.ones((height, width), F)
    buffers = _upload(twk, (Lc, g, Hl, hg, trust, ones))
    out, plain = _DeviceBuffer(twk, Lc.nbytes), _DeviceBuffer(twk, Lc.nbytes)
    p = [b.ptr.value for b in buffers]
    tp, cp, camera = L.Temporal(maxHistory=max_history, positionTolerance=tolerance), L.Cascade(K, 1.0, 8.0), _camera(twk, cam)
    shape = (height, width)
    what = f"{width}x{height}, {K} layers"
    dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], p[2], p[3], camera, p[4], shape, out.ptr.value)
    dev.synchronizeStream()
    _same(out.download(Lc.shape, F), expect, what)
    dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], p[2], p[3], camera, p[5], shape, out.ptr.value)
    dev.temporalAccumulateCascade(tp, cp, p[0], p[1], p[2], p[3], camera, shape, plain.ptr.value)
    dev.synchronizeStream()
    _same(out.download(Lc.shape, F), plain.download(Lc.shape, F), what + ", trust 1 against twk_temporal_accumulate_cascade")
    # no history: every pixel passes through, the trust is not read
    dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], None, None, None, p[4], shape, out.ptr.value)
    dev.synchronizeStream()
    _same(out.download(Lc.shape, F), Lc, what + ", no history")
    for call in (lambda: dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], p[2], p[3], camera, None, shape, out.ptr.value),        # no trust
                 lambda: dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], p[2], p[3], camera, out.ptr.value + 64, shape, out.ptr.value),  # the output overlaps it
                 lambda: dev.temporalAccumulateCascadeTrusted(tp, cp, p[0], p[1], p[2], p[3], camera, p[4], shape, p[2])):
        with pytest.raises(twk.TwkError) as e:
            call()
        assert e.value.code == L.TWK_ERROR_INVALID_VALUE and "twk_temporal_accumulate_cascade_trusted" in str(e.value)
    for buf in buffers + [out, plain]:
        buf.free()
    dev.close()


def test_own_buffers_merge_the_layers_with_the_trust(twk):
    """C2 at 61x37, three frames of 4 spp, the emission halved by twk_update_light before the third; cascade and its temporal merge
    on, the merge is twk_temporal_accumulate_rectified. After every frame the merged layers equal the restatement of the trusted
    build fed the handle's own layers and geometry, the layers the merge before kept, and the trust read back; in the third frame
    that trust is below 1 somewhere, so the layers differ from what the plain merge of the same inputs gives."""
    L = twk._lib
    res, spp = (61, 37), 4
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", res)
    cams = [app.cameras[0], _moved(twk, app, 0.004), _moved(twk, app, 0.008)]
    dev = _rendered(twk, 0, res=res)
    dev.enableGeometry(True)
    dev.enableCascade(True)
    dev.enableTemporalCascade(True)
    previous = None
    for frame, cam in enumerate(cams):
        dev.updateCamera(0, cam)
        if frame == 2:
            (light,) = app.lights
            for k in range(3):
                light.emission[k] = light.emission[k] * 0.5
            dev.updateLight(0, light)
        _frame(dev, frame * spp, spp)
        layers, g = dev.readCascade(), dev.readGeometry()
        dev.temporalAccumulateRectified(tp)
        own, trust = dev.readTemporalCascade(), dev.readTemporalTrust()
        if previous is None:
            _same(own, layers, "the first call copies the frame's layers through")
            assert (trust == 1).all()
        else:
            hl, hg, hcam = previous
            expect, took, _ = restate_temporal_cascade_trusted(layers, g, (hl, hg), camera_array(hcam), 32, 0.1, trust)
            assert took.mean() > 0.5
            _same(own, expect, f"frame {frame}: own layers against the restatement with the trust read back")
            if frame == 2:
                plain = restate_temporal_cascade_trusted(layers, g, (hl, hg), camera_array(hcam), 32, 0.1, np.ones_like(trust))[0]
                assert (trust[took] < 1).any() and not np.array_equal(own.view(U32), plain.view(U32))
        previous = (own, g, cam)
    dev.close()
