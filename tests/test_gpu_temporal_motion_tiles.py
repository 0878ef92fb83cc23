"""-m gpu: an object that moves in the moving-camera loop on a frame tiled over several handles. The orbit of
tests/test_gpu_temporal_tiles.py (the Cornell box at 61x37 with 8x8 tiles, three frames of 2 spp, 0.004 of a turn apart, maxHistory 32,
positionTolerance 0.1, the cascade and its temporal merge on) with the mirror sphere stepped between the frames by
twk_update_instance_transform on every handle: after EVERY frame the primary's merged colour, moments and layers equal one handle's,
byte for byte, on 2 and on 3 handles sharing this GPU; a source handle that was not updated is refused; and rtigo3_hip with
`temporalInstanceStep` on three handles writes the one-device screenshot."""
import os
import re
import subprocess

import numpy as np
import pytest

import lifecycle as lc
from conftest import load_app, scene_path
from test_gpu_temporal_cli import FRAMES as CLI_FRAMES, ORBIT, SCENE, SYSTEM, THREE, _run
from test_gpu_temporal_tiles import FRAMES, HEIGHT, MERGED, SPP, TILE, WIDTH, _assert_same, _camera, _close, _device, _merged, _render, _tiled, _tp
from test_screenshot_files import CLI

pytestmark = pytest.mark.gpu

SPHERE, LIGHT = 6, 0      # the mirror sphere; the area light's instance
STEP = (0.0, 0.3, 0.25)   # per frame: up and towards the camera, clear of the glass sphere


def _step(devs, frame):
    """Before every frame after the first: the sphere one step further, on every handle."""
    if frame == 0:
        return
    for d in devs:
        t = d.instanceTransform(SPHERE)
        t[[3, 7, 11]] += np.array(STEP, np.float32)
        d.updateInstanceTransform(SPHERE, t)


@pytest.fixture(scope="module")
def single(twk):
    """[the merged buffers after each frame] of ONE handle running the own-buffer loop with the sphere stepped; computed once."""
    shape = lc.Shape(WIDTH, HEIGHT, TILE, 1)
    app = lc.make_app(twk, load_app, shape)
    dev = _device(twk, app, shape)
    dev.enableTemporalCascade(True)
    frames = []
    for f in range(FRAMES):
        _step([dev], f)
        dev.updateCamera(0, _camera(twk, app, f))
        dev.setSampleOffset(f * SPP)
        for it in range(SPP):
            dev.render(it)
        dev.renderGeometry()
        dev.temporalAccumulate(_tp(twk))
        frames.append(_merged(dev))
        table = dev.readTemporalMotion()
        assert [r.moved for r in table] == ([] if f == 0 else [int(i == SPHERE) for i in range(app.info.numInstances)])
        sphere = dev.readGeometry()[..., 3].view(np.uint32) == SPHERE + 1
        took = dev.readTemporalMoments()[..., 2] > dev.readMoments()[..., 2]
        assert sphere.sum() > 40 and ((took & sphere).sum() > 0.5 * sphere.sum() if f > 0 else not took.any()), (f, sphere.sum(), (took & sphere).sum())
    dev.close()
    app.close()
    return frames


@pytest.mark.parametrize("n", [2, 3])
def test_the_loop_with_a_moving_sphere_on_tiles_equals_one_device(twk, single, n):
    app, devs = _tiled(twk, n, False)
    primary = devs[0]
    for f in range(FRAMES):
        _step(devs, f)
        _render(devs, _camera(twk, app, f), f)
        primary.assembleWithGeometry(devs, MERGED)
        primary.temporalAccumulateAssembled(_tp(twk))
        _assert_same(_merged(primary), single[f], f"{n} handles, frame {f}")
        assert len(primary.readTemporalMotion()) == (0 if f == 0 else app.info.numInstances)
    _close(app, devs)


def test_a_source_that_was_not_updated_is_refused(twk, single):
    L = twk._lib
    app, devs = _tiled(twk, 2, False)
    primary = devs[0]
    _render(devs, _camera(twk, app, 0), 0)
    primary.assembleWithGeometry(devs, MERGED)
    primary.temporalAccumulateAssembled(_tp(twk))
    _step(devs[:1], 1)  # the primary alone
    _render(devs, _camera(twk, app, 1), 1)
    with pytest.raises(twk.TwkError) as e:
        primary.assembleWithGeometry(devs, MERGED)
    assert e.value.code == L.TWK_ERROR_INVALID_STATE and "twk_assemble_devices_with_geometry" in str(e.value), str(e.value)
    for word in (f"instance {SPHERE}", "index 1", "twk_update_instance_transform"):
        assert word in str(e.value), str(e.value)
    _step(devs[1:], 1)  # ... and once the other handle has caught up the loop goes on, with the history it had
    _render(devs, _camera(twk, app, 1), 1)
    primary.assembleWithGeometry(devs, MERGED)
    primary.temporalAccumulateAssembled(_tp(twk))
    _assert_same(_merged(primary), single[1], "frame 1, after the refused attempt")
    _close(app, devs)


def test_the_command_line_on_three_devices_writes_the_one_device_screenshot(tmp_path):
    orbit = ORBIT.format(frames=CLI_FRAMES)
    moving = orbit + f"temporalInstanceStep {SPHERE} {STEP[0]} {STEP[1]} {STEP[2]}\n"
    _, one = _run(tmp_path, "one", 0, moving, 4 * CLI_FRAMES)
    _, three = _run(tmp_path, "three", 3, moving + "tileAssembly 1\n", 4 * CLI_FRAMES, env=THREE)
    differ = (three != one).any(-1)
    assert one.shape == (64, 96, 3) and not differ.any(), f"{differ.sum()} of {differ.size} pixels differ between three handles and one"
    _, still = _run(tmp_path, "still", 0, orbit, 4 * CLI_FRAMES)
    assert not np.array_equal(still, one), "the sphere has moved: another picture than the orbit around the scene at rest"


@pytest.mark.parametrize("extra,words", [
    (f"temporalInstanceStep {SPHERE} 0 0.1 0\n", ("temporalInstanceStep", "temporalAccumulation 1")),
    (ORBIT.format(frames=2) + f"temporalInstanceStep {LIGHT} 0 0.1 0\n", ("temporalInstanceStep", "light")),
    (ORBIT.format(frames=2) + "temporalInstanceStep 99 0 0.1 0\n", ("temporalInstanceStep", "instance 99")),
], ids=["no-loop", "light", "beyond-the-scene"])
def test_the_key_is_refused_where_it_cannot_apply(tmp_path, extra, words):
    system = tmp_path / "system.txt"
    system.write_text(open(scene_path(SYSTEM)).read() + "\n" + extra)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert r.returncode != 0
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
    for word in words:
        assert word in r.stderr, r.stderr
    assert re.search(r"ERROR: .*temporalInstanceStep", r.stderr)
