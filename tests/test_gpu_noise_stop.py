"""-m gpu: the stopping rule of rtigo3_hip -m 1 ("targetNoise" in the system description): the run ends at the first check, every
"targetNoiseInterval" iterations, at which the quantile of the merged noise summaries is at most the target; the lines it prints
and the file it names carry the iterations rendered, and the picture is the picture of that many plain iterations, byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_app, scene_path
from test_screenshot_files import CLI, read_png_rgb8

pytestmark = pytest.mark.gpu

RES = (160, 90)
SCENE = "scene_rtigo3_cornell_box.txt"
INTERVAL, SAMPLES_SQRT, QUANTILE = 16, 8, 0.95


@pytest.fixture(scope="module")
def predicted(twk):
    """(target, K, the tonemapped picture of K plain iterations as the file stores it). The target comes from the data: the 0.95
    quantile after 32 iterations, so a run that checks every 16 stops at 32 at the latest; K is what the same loop does in Python."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", SCENE, RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    quantiles = {}
    for it in range(32):
        dev.render(it)
        if (it + 1) % INTERVAL == 0:
            quantiles[it + 1] = dev.estimateNoise().quantile(QUANTILE)
    dev.close()
    target = quantiles[32]
    K = min(k for k, q in quantiles.items() if q <= target)
    print(f"\n0.95 quantile edges {quantiles}: target {target!r}, the loop stops at {K}")
    assert K < SAMPLES_SQRT ** 2
    plain = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(plain)
    for it in range(K):
        plain.render(it)
    picture = plain.tonemap(app.tonemapper)[::-1]  # the file stores the top row first
    plain.close()
    return target, K, picture


def _run(tmp_path, strategy, target, env=None):
    text = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    text = re.sub(r"(?m)^resolution .*$", f"resolution {RES[0]} {RES[1]}", text)
    text = re.sub(r"(?m)^samplesSqrt .*$", f"samplesSqrt {SAMPLES_SQRT}", text)
    text = re.sub(r"(?m)^strategy .*$", f"strategy {strategy}", text)
    text += f"\nprefixScreenshot {tmp_path}/stop{strategy}\ntargetNoise {float(np.float32(target))!r}\ntargetNoiseInterval {INTERVAL}\n"
    system = tmp_path / f"system_stop{strategy}.txt"
    system.write_text(text)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300, env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stdout + r.stderr
    return str(system), r.stdout.strip().splitlines()


def _check(twk, tmp_path, strategy, predicted, env=None):
    target, K, picture = predicted
    system, lines = _run(tmp_path, strategy, target, env)
    app = twk.Application(system, scene_path(SCENE))
    on, t, q, interval = app.targetNoise
    assert on and np.float32(t) == np.float32(target) and np.float32(q) == np.float32(QUANTILE) and interval == INTERVAL  # the file said what was meant
    assert len(lines) == 3, lines
    assert re.fullmatch(rf"{K} / (\d+\.\d{{3}}) = (\d+\.\d{{3}}) fps", lines[0]), lines[0]
    assert re.match(rf"noise: {K} spp, mean \S+, \S+ quantile at most \S+, target \S+$", lines[1]), lines[1]
    assert re.fullmatch(rf"{re.escape(str(tmp_path))}/stop{strategy}_{K}spp_\d{{7}}_\d{{6}}_000\.png", lines[2]), lines[2]
    png = read_png_rgb8(lines[2])
    assert png.shape == (RES[1], RES[0], 3) and png.max() > 100
    assert np.array_equal(png, picture), f"{(png != picture).any(-1).sum()} pixels differ from {K} plain iterations"


def test_one_device_stops_at_the_predicted_iteration(twk, tmp_path, predicted):
    _check(twk, tmp_path, 0, predicted)


def test_two_virtual_devices_stop_at_the_same_iteration(twk, tmp_path, predicted):
    """Strategy 3 over two handles that share the GPU: each estimates its own packed tile buffer, the host merges; the merged
    summary is the single device's, so the run stops at the same K with the same picture."""
    _check(twk, tmp_path, 3, predicted, env={"TWK_CLI_VIRTUAL_DEVICES": "2"})


def test_a_target_never_met_renders_every_sample(twk, tmp_path):
    """A target of 2^-16 (no bin's upper edge lies below it, unless every pixel is noise-free) leaves the loop at samplesSqrt²; and
    a count that is no multiple of the interval still prints the frame's figures."""
    text = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    text = re.sub(r"(?m)^resolution .*$", "resolution 96 64", text)
    text = re.sub(r"(?m)^samplesSqrt .*$", "samplesSqrt 3", text)
    text += f"\nprefixScreenshot {tmp_path}/never\ntargetNoise {2.0 ** -16!r}\ntargetNoiseInterval 4\n"
    system = tmp_path / "system_never.txt"
    system.write_text(text)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("9 / ") and lines[1].startswith("noise: 9 spp, mean ") and "/never_9spp_" in lines[2]
