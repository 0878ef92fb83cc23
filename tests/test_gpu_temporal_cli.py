"""-m gpu: rtigo3_hip -m 1 with `temporalAccumulation 1` — the moving-camera loop from the command line, 96x64, an orbit of three
frames of 4 spp (samplesSqrt 2), 0.004 of a turn apart, positionTolerance 0.1, with two key sets: plain, and the sampled-variance
denoiser (denoiser 3) on the resolve of the firefly cascade. Three handles sharing this GPU (strategy 3, tileAssembly 1) write,
byte for byte, the screenshot one device writes; that screenshot differs from the run with one frame and from the run without the
key; for the plain key set it equals the tonemapped readTemporal() of the same loop driven through Python. Every refusal of the
key is checked by its text, before any device is created."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_screenshot_files import CLI, read_png_rgb8

pytestmark = pytest.mark.gpu

SYSTEM, SCENE = "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt"
FRAMES = 3
ORBIT = "temporalAccumulation 1\ntemporalFrames {frames}\ntemporalOrbitStep 0.004\ntemporalPositionTolerance 0.1\n"
KEY_SETS = {"plain": "", "denoised-cascade": "denoiser 3\ndenoiserSampledVariance 1\nfireflyCascade 1\n"}
THREE = {"TWK_CLI_VIRTUAL_DEVICES": "3"}


def _run(tmp_path, tag, strategy, extra, iterations, env=None):
    """One run at 96x64, samplesSqrt 2; returns (the system file, the screenshot uint8 [64, 96, 3], top row first)."""
    folder = tmp_path / tag
    folder.mkdir()
    system = folder / "system.txt"
    text = open(scene_path(SYSTEM)).read()
    text = re.sub(r"(?m)^resolution .*$", "resolution 96 64", text)
    text = re.sub(r"(?m)^samplesSqrt .*$", "samplesSqrt 2", text)
    text = re.sub(r"(?m)^strategy .*$", f"strategy {strategy}", text)
    text += f"\nprefixScreenshot {folder}/shot\ngamma 2.2\ncolorBalance 1.0 0.95 0.9\nburnHighlights 0.8\ncrushBlacks 0.2\nsaturation 1.2\nbrightness 0.8\n" + extra
    system.write_text(text)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(folder), capture_output=True, text=True, timeout=300,
                       env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert re.fullmatch(rf"{iterations} / (\d+\.\d{{3}}) = (\d+\.\d{{3}}) fps", lines[0]), lines[0]  # frames x samplesSqrt² iterations
    assert re.fullmatch(rf"{re.escape(str(folder))}/shot_4spp_\d{{7}}_\d{{6}}_000\.png", lines[1]), lines[1]
    return str(system), read_png_rgb8(lines[1])


def _python_loop(twk, system):
    """The loop of the plain key set through the Python binding on one device: the tonemapped merged colour, top row first."""
    app = twk.Application(system, scene_path(SCENE))
    on, tp, frames, step = app.temporal
    assert on and frames == FRAMES
    i = app.info
    spp = i.samplesSqrt * i.samplesSqrt
    dev = twk.Device(ordinal=0, miss=i.miss)
    app.initDevice(dev)
    for f in range(frames):
        dev.updateCamera(0, twk.camera_frustum(tuple(i.center), i.phi + f * step, i.theta, i.fov, i.distance, i.resolution[0] / i.resolution[1]))
        dev.setSampleOffset(f * spp)
        for it in range(spp):
            dev.render(it)
        dev.renderGeometry()
        dev.temporalAccumulate(tp)
    merged = dev.readTemporal()
    assert (dev.readTemporalMoments()[..., 2] > spp).mean() > 0.5, "most pixels hold more samples than one frame's"
    picture = dev.tonemap(app.tonemapper, rgbaDevicePointer=dev.temporalDevicePointers()[0], shape=(i.resolution[1], i.resolution[0]))
    assert np.isfinite(merged).all()
    dev.close()
    app.close()
    return picture[::-1]


@pytest.mark.parametrize("keys", list(KEY_SETS), ids=list(KEY_SETS))
def test_three_devices_write_the_one_device_screenshot(twk, tmp_path, keys):
    orbit = KEY_SETS[keys] + ORBIT.format(frames=FRAMES)
    system, one = _run(tmp_path, "one", 0, orbit, 4 * FRAMES)
    _, three = _run(tmp_path, "three", 3, orbit + "tileAssembly 1\n", 4 * FRAMES, env=THREE)
    assert one.shape == three.shape == (64, 96, 3)
    differ = (three != one).any(-1)
    assert not differ.any(), f"{differ.sum()} of {differ.size} pixels differ, columns {np.unique(np.nonzero(differ)[1])[:40]}"
    _, single_frame = _run(tmp_path, "frames1", 0, KEY_SETS[keys] + ORBIT.format(frames=1), 4)
    assert not np.array_equal(single_frame, one), "the orbit's last frame holds history: another picture than one frame"
    _, without = _run(tmp_path, "off", 0, KEY_SETS[keys], 4)
    assert not np.array_equal(without, one), "without the key the loop renders the camera at rest"
    if keys == "plain":
        assert np.array_equal(_python_loop(twk, system), one), "the command line runs the library's loop"


def _refused_run(tmp_path, strategy, extra, env=None):
    system = tmp_path / "system.txt"
    text = open(scene_path(SYSTEM)).read()
    text = re.sub(r"(?m)^strategy .*$", f"strategy {strategy}", text)
    system.write_text(text + "\n" + ORBIT.format(frames=FRAMES) + extra)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120,
                       env={**os.environ, **(env or {})})
    assert r.returncode != 0
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
    return r.stderr


@pytest.mark.parametrize("strategy,extra,env,words", [
    (0, "targetNoise 0.05\n", None, ("temporalAccumulation", "targetNoise")),
    (0, "targetNoise 0.05\nadaptiveSampling 1\n", None, ("temporalAccumulation", "adaptiveSampling")),
    (0, "lensShader 1\n", None, ("temporalAccumulation", "lensShader")),
    (1, "", THREE, ("temporalAccumulation", "strategy 1 or 2", "shared frame")),
    (2, "", THREE, ("temporalAccumulation", "strategy 1 or 2", "shared frame")),
    (3, "", THREE, ("temporalAccumulation", "tileAssembly 1")),
    (3, "tileAssembly 0\n", THREE, ("temporalAccumulation", "tileAssembly 1")),
], ids=["target-noise", "adaptive", "lens", "strategy-1", "strategy-2", "no-assembly", "assembly-off"])
def test_the_key_is_refused_where_the_loop_cannot_run(tmp_path, strategy, extra, env, words):
    err = _refused_run(tmp_path, strategy, extra, env)
    for w in words:
        assert w in err, err
