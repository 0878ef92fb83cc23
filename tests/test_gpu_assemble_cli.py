"""-m gpu: rtigo3_hip -m 1 with `tileAssembly 1`: three handles sharing this GPU (strategy 3) assemble the planes the description's
post steps need and write, byte for byte, the screenshot one device writes for the same keys; strategy 1 with the key is refused
before any device is created; without the key the three refusals of a several-device run are what they were."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_cascade_stop import KEYS
from test_gpu_screenshot import CLI, _run_cli

pytestmark = pytest.mark.gpu

SAMPLED = "denoiser 3\ndenoiserSampledVariance 1\ndenoiserMinSamples 3\n"
KEY_SETS = {"guided": "denoiser 3\n", "sampled": SAMPLED, "cascade": KEYS, "cascade-sampled": KEYS + SAMPLED}
THREE = {"TWK_CLI_VIRTUAL_DEVICES": "3"}


@pytest.mark.parametrize("keys", list(KEY_SETS), ids=list(KEY_SETS))
def test_three_devices_write_the_one_device_screenshot(tmp_path, keys):
    """96x64, 4 spp (_run_cli also checks the frame-rate line of both runs)."""
    (tmp_path / "one").mkdir()
    _, one = _run_cli(tmp_path / "one", 0, extra=KEY_SETS[keys])
    _, three = _run_cli(tmp_path, 3, env=THREE, extra=KEY_SETS[keys] + "tileAssembly 1\n")
    assert three.shape == (64, 96, 3)
    differ = (three != one).any(-1)
    assert not differ.any(), f"{differ.sum()} of {differ.size} pixels differ, columns {np.unique(np.nonzero(differ)[1])[:40]}"
    if keys == "guided":  # the key alone changes nothing on one device, and the plain picture is another one
        (tmp_path / "key").mkdir()
        (tmp_path / "plain").mkdir()
        assert np.array_equal(_run_cli(tmp_path / "key", 0, extra=KEY_SETS[keys] + "tileAssembly 1\n")[1], one)
        assert not np.array_equal(_run_cli(tmp_path / "plain", 3, env=THREE, extra="tileAssembly 1\n")[1], one)


def _refused_run(tmp_path, strategy, extra):
    system = tmp_path / "system.txt"
    text = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    text = re.sub(r"(?m)^strategy .*$", f"strategy {strategy}", text)
    system.write_text(text + "\n" + extra)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path("scene_rtigo3_cornell_box.txt"), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120, env={**os.environ, **THREE})
    assert r.returncode != 0
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
    return r.stderr


@pytest.mark.parametrize("strategy", [1, 2])
def test_shared_frame_strategies_refuse_the_key(tmp_path, strategy):
    err = _refused_run(tmp_path, strategy, "denoiser 3\ntileAssembly 1\n")
    assert "tileAssembly" in err and "shared frame" in err


@pytest.mark.parametrize("extra,words", [("denoiser 3\n", ("denoiser 3", "ONE device")), (SAMPLED, ("denoiserSampledVariance", "ONE device")),
                                         (KEYS, ("fireflyCascade", "ONE device"))], ids=["guided", "sampled", "cascade"])
def test_without_the_key_the_old_refusals_stand(tmp_path, extra, words):
    for off in ("", "tileAssembly 0\n"):
        err = _refused_run(tmp_path, 3, extra + off)
        for w in words:
            assert w in err, err
        assert "not assembled" in err or "assembled frame" in err
