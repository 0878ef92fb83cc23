"""-m gpu: rtigo3_hip -m 1 with `temporalRectify 1` beside `temporalAccumulation 1` — the orbit of tests/test_gpu_temporal_cli.py
(96x64, three frames of 4 spp, 0.004 of a turn apart, positionTolerance 0.1) merged by twk_temporal_accumulate_rectified. The orbit
runs with the key, on one device and on three handles sharing this GPU, which write the same bytes; with `temporalRectifyMinTaps 50`
(a test that never runs) the screenshot equals the one written without the key; the keys are read back by Application.temporalRectify;
and any of the four keys without `temporalAccumulation 1` is refused, by name, before a device is created."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_temporal_cli import FRAMES, ORBIT, SCENE, SYSTEM, THREE, _run
from test_screenshot_files import CLI

pytestmark = pytest.mark.gpu


def test_the_orbit_runs_with_the_key(twk, tmp_path):
    orbit = ORBIT.format(frames=FRAMES)
    _, plain = _run(tmp_path, "plain", 0, orbit, 4 * FRAMES)
    system, rectified = _run(tmp_path, "rectified", 0, orbit + "temporalRectify 1\n", 4 * FRAMES)
    assert rectified.shape == plain.shape == (64, 96, 3) and rectified.any()
    _, never = _run(tmp_path, "never", 0, orbit + "temporalRectify 1\ntemporalRectifyMinTaps 50\n", 4 * FRAMES)
    assert np.array_equal(never, plain), "a test that never runs writes the screenshot of the plain merge"
    _, three = _run(tmp_path, "three", 3, orbit + "temporalRectify 1\ntileAssembly 1\n", 4 * FRAMES, env=THREE)
    differ = (three != rectified).any(-1)
    assert not differ.any(), f"{differ.sum()} of {differ.size} pixels differ between three handles and one"
    # gamma 0: every mean difference counts as bias, the history is discounted nearly everywhere: another picture than the plain merge
    _, eager = _run(tmp_path, "eager", 0, orbit + "temporalRectify 1\ntemporalRectifyGamma 0\ntemporalRectifyRadius 2\n", 4 * FRAMES)
    assert not np.array_equal(eager, plain)
    app = twk.Application(system, scene_path(SCENE))
    on, rp, keys = app.temporalRectify
    assert on and keys == 1 and (rp.radius, rp.minTaps, rp.gamma) == (3, 8, 3.0)
    written = app.systemDescription()
    assert "temporalRectify 1" in written and "temporalRectifyGamma" not in written, "the keys are written back only when they differ from the defaults"
    app.close()


@pytest.mark.parametrize("key", ["temporalRectify 1", "temporalRectify 0", "temporalRectifyGamma 2", "temporalRectifyRadius 2", "temporalRectifyMinTaps 12"])
def test_a_key_without_the_loop_is_refused(tmp_path, key):
    system = tmp_path / "system.txt"
    system.write_text(open(scene_path(SYSTEM)).read() + "\n" + key + "\n")
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert r.returncode != 0
    assert "INFO:" not in r.stderr and not r.stdout.strip(), "refused before any device is created or anything is rendered"
    for word in ("temporalRectify", "temporalRectifyGamma", "temporalRectifyRadius", "temporalRectifyMinTaps", "temporalAccumulation 1"):
        assert word in r.stderr, r.stderr
    assert re.search(r"ERROR: .*temporalRectify", r.stderr)
