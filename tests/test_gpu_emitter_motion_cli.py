"""-m gpu: rtigo3_hip -m 1 with `movingEmitters 1` — tests/test_gpu_temporal_cli.py's orbit (96x64, 4 spp a frame) of two frames with
`temporalInstanceStep` on the instance that carries the light. The run writes, byte for byte, the screenshot a Python loop making the
same calls produces (twk_enable_emitter_motion before the loop, twk_update_instance_transform on the light before the second frame);
that screenshot differs from the orbit with the light at rest; the key is written back by twk_app_system_description; and without the
key the command line refuses the light's instance with the text it always had."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_temporal_cli import ORBIT, SCENE, SYSTEM, _run
from test_screenshot_files import CLI

pytestmark = pytest.mark.gpu

FRAMES, LIGHT = 2, 0
STEP = (0.2, -0.1, 0.15)
MOVING = ORBIT.format(frames=FRAMES) + f"temporalInstanceStep {LIGHT} {STEP[0]} {STEP[1]} {STEP[2]}\n"


def _python_loop(twk, system):
    """The command line's loop through the Python binding on one device: the tonemapped merged colour, top row first, and the light's
    definitions before and after."""
    app = twk.Application(system, scene_path(SCENE))
    text = app.systemDescription()
    assert "movingEmitters 1\n" in text and f"temporalInstanceStep {LIGHT} " in text, "both keys are written back"
    on, tp, frames, step = app.temporal
    assert on and frames == FRAMES
    i = app.info
    spp = i.samplesSqrt * i.samplesSqrt
    light = app.instance(LIGHT)[3]
    assert light >= 0, "the instance carries the light"
    dev = twk.Device(ordinal=0, miss=i.miss)
    app.initDevice(dev)
    dev.enableEmitterMotion()
    before = bytes(dev.getLight(light))
    for f in range(frames):
        if f > 0:
            t = dev.instanceTransform(LIGHT)
            t[[3, 7, 11]] += np.array(STEP, np.float32)
            dev.updateInstanceTransform(LIGHT, t)
        dev.updateCamera(0, twk.camera_frustum(tuple(i.center), i.phi + f * step, i.theta, i.fov, i.distance, i.resolution[0] / i.resolution[1]))
        dev.setSampleOffset(f * spp)
        for it in range(spp):
            dev.render(it)
        dev.renderGeometry()
        dev.temporalAccumulate(tp)
    assert [r.moved for r in dev.readTemporalMotion()] == [int(k == LIGHT) for k in range(i.numInstances)]
    after = dev.getLight(light)
    picture = dev.tonemap(app.tonemapper, rgbaDevicePointer=dev.temporalDevicePointers()[0], shape=(i.resolution[1], i.resolution[0]))
    dev.close()
    app.close()
    return picture[::-1], before, after


def test_the_command_line_moves_the_light_as_the_python_loop_does(twk, tmp_path):
    system, shot = _run(tmp_path, "moving", 0, MOVING + "movingEmitters 1\n", 4 * FRAMES)
    picture, before, after = _python_loop(twk, system)
    assert shot.shape == (64, 96, 3) and np.array_equal(picture, shot), "the command line runs the library's loop"
    assert bytes(after) != before
    assert [after.position[k] - np.frombuffer(before, np.float32)[1 + k] for k in range(3)] == pytest.approx(STEP, abs=1e-6), "the definition went along"
    _, still = _run(tmp_path, "still", 0, ORBIT.format(frames=FRAMES), 4 * FRAMES)
    assert not np.array_equal(still, shot), "the light has moved: another picture than the orbit around the scene at rest"


@pytest.mark.parametrize("extra", ["", "movingEmitters 0\n"], ids=["no-key", "key-off"])
def test_without_the_key_the_lights_instance_is_refused_as_before(tmp_path, extra):
    system = tmp_path / "system.txt"
    system.write_text(open(scene_path(SYSTEM)).read() + "\n" + MOVING + extra)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert r.returncode != 0
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
    assert "ERROR: temporalInstanceStep names an instance that carries a light: moving emitters is not supported" in r.stderr, r.stderr
    assert re.search(r"ERROR: .*temporalInstanceStep", r.stderr)
