"""-m gpu: a wavefront pass cut into 1, 2, 3 and 4 lanes (TWK_PASS_LANES; device_pass.hip laneParams). Every path stream of a
lane starts at an offset of its own kind (device_types.h TWK_PATH_STREAMS: by queue record or by path); a stream that is
forgotten there, or given the wrong kind, makes two lanes write over each other. So the image of a pass is the same bit for
bit for every lane count, and the one-lane image is the oracle's.
Scenes are the smallest at which every one of four lanes keeps the 4 096 paths below which chooseLanes drops a lane:
  * C2 160x90x3 = 43 200 paths: shares of 11 264 / 11 264 / 11 264 / 9 408 (a ragged last lane), slim layout;
  * the same under TWK_SLIM_STREAMS=0: the hitInstance and shadowPixel offsets on a flattened scene;
  * C4 instances 128x72x3 = 27 648 paths: 7 168 / 7 168 / 7 168 / 6 144, two-level, full layout;
  * C3 with cutout opacity 160x90x3: no packed queue, so rayPixel and raySeedFlags are live;
  * C2 with the denoiser AOVs on: the pathAlbedo / pathNormal offsets.
Several iterations as ONE deferred pass, as in test_gpu_stream_layout.py."""
import functools

import numpy as np
import pytest

from test_gpu_stream_layout import ITERATIONS, _bits, _c2, _c3, _c4_instances, _oracle

pytestmark = pytest.mark.gpu

LANES = (1, 2, 3, 4)


def _render(twk, monkeypatch, lanes, app, edit, textures, aov=False):
    monkeypatch.setenv("TWK_PASS_LANES", str(lanes))  # read when the handle is created
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    for slot, img in textures:
        dev.initTexture(slot, img)
    app.initDevice(dev)
    if edit:
        mats = app.materials
        edit(mats)
        dev.initMaterials(mats)
    if aov:
        dev.enableAov(True)
    for it in range(ITERATIONS):
        dev.render(it)
    dev.synchronizeStream()
    out = [dev.getOutputBufferHost().copy()] + ([dev.readAov(0).copy(), dev.readAov(1).copy()] if aov else [])
    dev.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle_image(twk, orc, scene):
    image = _oracle(orc, *scene(twk))
    image.setflags(write=False)
    return image


@pytest.mark.parametrize("scene,slim", [(_c2, True), (_c2, False), (_c4_instances, True), (_c3, True)],
                         ids=["C2", "C2_full_layout", "C4_instances", "C3_cutout"])
def test_image_does_not_depend_on_the_lane_count(twk, orc, monkeypatch, scene, slim):
    if not slim:
        monkeypatch.setenv("TWK_SLIM_STREAMS", "0")
    app, edit, textures = scene(twk)
    images = {lanes: _render(twk, monkeypatch, lanes, app, edit, textures)[0] for lanes in LANES}
    one = images[1]
    assert np.isfinite(one).all() and one[..., :3].max() > 0.5
    for lanes in LANES[1:]:
        mism = (_bits(images[lanes]) != _bits(one)).any(axis=2).sum()
        assert mism == 0, f"{lanes} lanes: {mism} pixels differ from one lane, max |diff| {np.abs(images[lanes] - one).max()}"
    cpu = _oracle_image(twk, orc, scene)
    mism = (_bits(one) != _bits(cpu)).any(axis=2).sum()
    assert mism == 0, f"one lane: {mism} pixels differ from the oracle, max |diff| {np.abs(one - cpu).max()}"


def test_aovs_do_not_depend_on_the_lane_count(twk, monkeypatch):
    app, edit, textures = _c2(twk)
    one = _render(twk, monkeypatch, 1, app, edit, textures, aov=True)
    four = _render(twk, monkeypatch, 4, app, edit, textures, aov=True)
    for name, a, b in zip(("image", "albedo", "normal"), four, one):
        assert np.isfinite(b).all() and np.abs(b[..., :3]).max() > 0.0, name
        mism = (_bits(a) != _bits(b)).any(axis=2).sum()
        assert mism == 0, f"{name}: {mism} pixels of four lanes differ from one lane"
