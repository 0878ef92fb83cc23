"""-m gpu: rtigo3_hip -m 1 with `denoiserGeometry 1` beside `denoiser 3`, at 96x64 and 4 spp: the screenshot is the one the same
chain driven through Python writes (trace the geometry once, twk_denoise_geometry on the handle's own buffers, tonemap), it is not
the picture without the key, and three handles sharing this GPU (strategy 3, tileAssembly 1) write it byte for byte. With the key,
what the geometry AOV refuses is refused before any device is created."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_screenshot import _run_cli
from test_screenshot_files import CLI

pytestmark = pytest.mark.gpu

SCENE = "scene_rtigo3_cornell_box.txt"
THREE = {"TWK_CLI_VIRTUAL_DEVICES": "3"}
KEYS = "denoiser 3\ndenoiserVariance 1\ndenoiserGeometry 1\ndenoiserSigmaPosition 0.02\ndenoiserInstanceStop 1\n"


def _folder(tmp_path, name):
    folder = tmp_path / name
    folder.mkdir()
    return folder


def test_the_screenshot_is_the_python_chain_on_one_device_and_on_three(twk, tmp_path):
    system, one = _run_cli(_folder(tmp_path, "one"), 0, extra=KEYS)
    app = twk.Application(system, scene_path(SCENE))
    on, dn = app.denoiser
    variance_on, dv = app.denoiserVariance
    geometry_on, dg = app.denoiserGeometry
    assert on and variance_on and geometry_on and dn.inputKind == 2 and (dg.sigmaPosition, dg.instanceStop) == (np.float32(0.02), 1)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)  # enables the AOVs and the geometry AOV: the keys ask for them
    for it in range(4):
        dev.render(it)
    dev.renderGeometry()
    dev.denoise(dn, variance=dv, geometry=dg)
    expect = dev.tonemap(app.tonemapper, dev.denoisedDevicePointer()[0], shape=(64, 96))
    assert one.shape == (64, 96, 3) and np.array_equal(one, expect[::-1])
    dev.denoise(dn, variance=dv)
    unguided = dev.tonemap(app.tonemapper, dev.denoisedDevicePointer()[0], shape=(64, 96))
    assert not np.array_equal(one, unguided[::-1]), "the key changes the picture"
    dev.close()
    app.close()
    _, three = _run_cli(_folder(tmp_path, "three"), 3, env=THREE, extra=KEYS + "tileAssembly 1\n")
    differ = (three != one).any(-1)
    assert not differ.any(), f"{differ.sum()} of {differ.size} pixels differ"


@pytest.mark.parametrize("strategy,extra,env,words", [
    (0, "lensShader 1\n", None, ("denoiserGeometry", "lensShader")),
    (3, "", THREE, ("denoiserGeometry", "tileAssembly 1")),
    (1, "tileAssembly 0\n", THREE, ("denoiserGeometry", "tileAssembly 1")),
], ids=["lens", "no-assembly", "shared-frame"])
def test_the_key_is_refused_where_the_geometry_aov_is(tmp_path, strategy, extra, env, words):
    system = tmp_path / "system.txt"
    text = re.sub(r"(?m)^strategy .*$", f"strategy {strategy}", open(scene_path("system_rtigo3_cornell_box.txt")).read())
    system.write_text(text + "\nresolution 96 64\n" + KEYS + extra)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120,
                       env={**os.environ, **(env or {})})
    assert r.returncode != 0
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
    for w in words:
        assert w in r.stderr, r.stderr
