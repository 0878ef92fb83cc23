"""-m gpu: rtigo3_hip -m 1 with `fireflyCascade 1`: the screenshot is the tonemapped RESOLVED picture, alone and as the beauty of
the sampled-variance denoiser, byte for byte what the Python path computes; with two devices the key is refused before one is created."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_denoise_variance import _upload
from test_gpu_screenshot import CLI, _run_cli

pytestmark = pytest.mark.gpu

KEYS = "fireflyCascade 1\nfireflyCascadeLayers 4\nfireflyCascadeStart 0.05\nfireflyCascadeBase 3\nfireflyCascadeKappa 8\n"


def _python_path(twk, system, denoise):
    app = twk.Application(system, scene_path("scene_rtigo3_cornell_box.txt"))
    on, cascade, resolve = app.fireflyCascade
    assert on and (cascade.layers, cascade.start, cascade.base, resolve.kappa) == (4, np.float32(0.05), 3.0, 8.0)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)  # enables the cascade (and AOVs and moments where the denoiser keys ask)
    for it in range(4):
        dev.render(it)
    assert (dev.readCascade()[0, ..., 3] == 4).all()
    plain = dev.tonemap(app.tonemapper)
    dev.cascadeResolve(cascade, resolve)
    ptr, _ = dev.resolvedDevicePointer()
    buffers = []
    if denoise:
        on, dn = app.denoiser
        _, dv = app.denoiserVariance
        son, min_samples = app.denoiserSampled
        assert on and son and dn.inputKind == 2
        buffers = _upload(twk, (dev.readAov(0, raw=True), dev.readAov(1, raw=True)))
        moments, _ = dev.momentsDevicePointer()
        dev.denoise(dn, ptr, buffers[0].ptr.value, buffers[1].ptr.value, shape=(64, 96), variance=dv, moments=moments, minSamples=min_samples)
        ptr, _ = dev.denoisedDevicePointer()
    expect = dev.tonemap(app.tonemapper, ptr, shape=(64, 96))
    for buffer in buffers:
        buffer.free()
    dev.close()
    app.close()
    return expect[::-1], plain[::-1]  # the file stores the top row first


@pytest.mark.parametrize("denoise", [False, True], ids=["resolved", "resolved-denoised"])
def test_command_line_writes_the_resolved_picture(twk, tmp_path, denoise):
    extra = KEYS + ("denoiser 3\ndenoiserSampledVariance 1\ndenoiserMinSamples 3\n" if denoise else "")
    system, png = _run_cli(tmp_path, 0, extra=extra)  # (checks the frame-rate line, which is what it is without the key)
    expect, plain = _python_path(twk, system, denoise)
    assert png.shape == (64, 96, 3) and np.array_equal(png, expect)
    assert not np.array_equal(png, plain), "the resolve changed nothing at these thresholds"
    (tmp_path / "off").mkdir()
    _, png_off = _run_cli(tmp_path / "off", 0, extra=extra.replace("fireflyCascade 1", "fireflyCascade 0"))
    assert not np.array_equal(png, png_off)
    if not denoise:
        assert np.array_equal(png_off, plain), "without the key the screenshot is the plain picture"


def test_command_line_refuses_the_cascade_on_two_devices(tmp_path):
    system = tmp_path / "system.txt"
    text = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    text = re.sub(r"(?m)^strategy .*$", "strategy 3", text)
    system.write_text(text + "\n" + KEYS)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path("scene_rtigo3_cornell_box.txt"), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120, env={**os.environ, "TWK_CLI_VIRTUAL_DEVICES": "2"})
    assert r.returncode == 1 and "fireflyCascade" in r.stderr and "ONE device" in r.stderr
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
