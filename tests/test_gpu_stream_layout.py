"""-m gpu: the slim path streams (device_types.h LaunchParams::slimSlotBits). A scene whose instances are all flattened and
that has no cutout opacity runs without the hitInstance and shadowPixel streams: the instance of a hit rides in the hit
record's slot word, the launch index of a shadow ray in its pending record. Every other scene keeps the full layout.
  * C2 (Cornell box), C3 (intro_07 with cutout opacity) and C4 instances (two-level) are bit-identical to the oracle;
  * Device.streamLayout() (twk_get_stream_layout) says which layout a pass over the scene runs: C2 slim, the other two full;
  * TWK_SLIM_STREAMS=0 puts C2 on the full layout, with the same image bit for bit;
  * the four forms of a record (csrc/path_queue.h: TWK_PACKED_QUEUE x TWK_SLIM_STREAMS) render the same image bit for bit, the
    measurement builds of the time view included.
Several iterations as ONE deferred pass, and deep enough for shadow rays and continuation rays of every bounce."""
import numpy as np
import pytest

from conftest import load_app
from procedural import albedo_checker, cutout_slots, environment_hdr

pytestmark = pytest.mark.gpu

ITERATIONS = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _c2(twk):
    return load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (160, 90)), None, ()


def _c3(twk):
    app = load_app(twk, "system_intro_07.txt", "scene_intro_07.txt", (160, 90))

    def edit(mats):  # material 0 is the area light's, then file order: 1 floor, 4 cutout (tests/test_gpu_scenes.py _intro07)
        mats[1].useAlbedoTexture = 1
        mats[4].useCutoutTexture = 1

    return app, edit, ((0, albedo_checker()), (1, cutout_slots()), (2, environment_hdr()))


def _c4_instances(twk):
    return load_app(twk, "system_rtigo3_instances.txt", "scene_rtigo3_instances.txt", (128, 72)), None, ()


def _gpu(twk, app, edit, textures):
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    for slot, img in textures:
        dev.initTexture(slot, img)
    app.initDevice(dev)
    if edit:
        mats = app.materials
        edit(mats)
        dev.initMaterials(mats)
    layout = dev.streamLayout()
    for it in range(ITERATIONS):
        dev.render(it)
    dev.synchronizeStream()
    image = dev.getOutputBufferHost().copy()
    assert dev.streamLayout() == layout
    info = dev.buildInfo()
    dev.close()
    return image, layout, info


def _oracle(orc, app, edit, textures):
    ref = orc.Oracle(miss=app.info.miss)
    for slot, img in textures:
        ref.initTexture(slot, img)
    ref.loadApplication(app)
    if edit:
        mats = app.materials
        edit(mats)
        ref.initMaterials(mats)
    for it in range(ITERATIONS):
        ref.render(it)
    return ref.getOutputBufferHost()


@pytest.mark.parametrize("scene,want", [(_c2, "slim"), (_c3, "full"), (_c4_instances, "full")], ids=["C2", "C3_cutout", "C4_instances"])
def test_layout_by_scene_and_image_equals_the_oracle(twk, orc, scene, want):
    app, edit, textures = scene(twk)
    gpu, layout, info = _gpu(twk, app, edit, textures)
    assert layout == want, (layout, info)
    if want == "slim":
        assert info["flattenedInstances"] == info["instances"]
    cpu = _oracle(orc, app, edit, textures)
    assert np.isfinite(cpu).all() and cpu[..., :3].max() > 0.5
    mism = (_bits(gpu) != _bits(cpu)).any(axis=2).sum()
    assert mism == 0, f"{mism} pixels differ, max |diff| {np.abs(gpu - cpu).max()}"


def test_off_switch_keeps_the_full_layout_and_the_image(twk, orc, monkeypatch):
    app, edit, textures = _c2(twk)
    slim, layout, _ = _gpu(twk, app, edit, textures)
    assert layout == "slim"
    monkeypatch.setenv("TWK_SLIM_STREAMS", "0")
    full, layout0, _ = _gpu(twk, app, edit, textures)
    monkeypatch.delenv("TWK_SLIM_STREAMS")
    assert layout0 == "full"
    assert np.array_equal(_bits(full), _bits(slim)), f"{(_bits(full) != _bits(slim)).any(axis=2).sum()} pixels differ"
    cpu = _oracle(orc, app, edit, textures)
    assert np.array_equal(_bits(slim), _bits(cpu))


def test_statistics_and_time_view_builds_run_the_slim_layout(twk):
    """The measurement builds (twk_stats_enable, twk_set_time_view) find a shadow ray's path through the pending record too: the
    same image, every ray counted, and a time word for every path."""
    app, edit, textures = _c2(twk)
    plain, layout, _ = _gpu(twk, app, edit, textures)
    assert layout == "slim"
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.statsEnable(True)
    dev.setTimeView(True)
    for it in range(ITERATIONS):
        dev.render(it)
    dev.synchronizeStream()
    stats = dev.statsGet()
    dev.close()
    assert stats["shadowRays"] > 0 and stats["radianceRays"] >= ITERATIONS * 160 * 90
    # the same pass without the time view (its alpha is the path time): the counting builds change no colour
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.statsEnable(True)
    for it in range(ITERATIONS):
        dev.render(it)
    dev.synchronizeStream()
    counted = dev.getOutputBufferHost().copy()
    dev.close()
    assert np.array_equal(_bits(counted), _bits(plain))


def _cornell_forms(twk, monkeypatch, timeView):
    """The Cornell scene at 64 x 48, four iterations as one pass (paths up to ten segments long), once per form of the records:
    {(packed, slim): image}. The switches are read when the handle is created."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (64, 48))
    assert app.state.pathLengths[1] >= 4
    images = {}
    for packed in (1, 0):
        for slim in (1, 0):
            monkeypatch.setenv("TWK_PACKED_QUEUE", str(packed))
            monkeypatch.setenv("TWK_SLIM_STREAMS", str(slim))
            dev = twk.Device(ordinal=0, miss=app.info.miss)
            app.initDevice(dev)
            dev.setLaunchBatch(4)
            dev.setTimeView(timeView)
            assert dev.streamLayout() == ("slim" if slim else "full")
            for it in range(4):
                dev.render(it)
            dev.synchronizeStream()
            images[(packed, slim)] = dev.getOutputBufferHost().copy()
            dev.close()
    return images


def test_every_form_of_a_record_renders_the_same_image(twk, monkeypatch):
    """Full and packed closest-hit records x full and slim hit and shadow records: no test turned TWK_PACKED_QUEUE off before, so
    the full continuation record of a cutout-free scene was unpinned. With the time view on, the COUNT builds of the trace
    kernels find a ray's launch index in the packed word, rayPixel, shadowPending.w or shadowPixel: same colour, a time for
    every path."""
    plain = _cornell_forms(twk, monkeypatch, False)
    want = plain[(1, 1)]
    assert np.isfinite(want).all() and want[..., :3].max() > 0.5 and np.all(want[..., 3] == 1.0)
    for form, image in plain.items():
        assert np.array_equal(_bits(image), _bits(want)), f"(packed, slim) = {form}: {(_bits(image) != _bits(want)).any(axis=2).sum()} pixels differ"
    timed = _cornell_forms(twk, monkeypatch, True)
    for form, image in timed.items():
        assert np.array_equal(_bits(image[..., :3]), _bits(want[..., :3])), f"time view, (packed, slim) = {form}"
        alpha = image[..., 3]
        assert np.isfinite(alpha).all() and (alpha > 0.0).all(), f"time view, (packed, slim) = {form}"
