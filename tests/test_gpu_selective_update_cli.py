"""-m gpu: rtigo3_hip -m 1 with `selectiveUpdate 1` — the moving-object loop from the command line on the Cornell box at 61x37, three
frames of 4 spp, the mirror sphere (instance 6) stepped before every frame after the first. With the key the loop's updates are
selective — the loop says so per update on stderr, from twk_get_update_info — and it writes, byte for byte, the screenshot it writes
without the key. The description writer hands the key back only when it is on."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_screenshot_files import CLI, read_png_rgb8

SYSTEM, SCENE = "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt"
LOOP = "temporalAccumulation 1\ntemporalFrames 3\ntemporalPositionTolerance 0.1\ntemporalInstanceStep 6 0.0 0.2 0.15\n"


def _system(folder, extra):
    text = open(scene_path(SYSTEM)).read()
    text = re.sub(r"(?m)^resolution .*$", "resolution 61 37", text)
    text = re.sub(r"(?m)^samplesSqrt .*$", "samplesSqrt 2", text)
    system = folder / "system.txt"
    system.write_text(text + f"\nprefixScreenshot {folder}/shot\n" + extra)
    return system


def _run(tmp_path, tag, extra):
    folder = tmp_path / tag
    folder.mkdir()
    system = _system(folder, extra)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(folder), capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert re.fullmatch(r"12 / (\d+\.\d{3}) = (\d+\.\d{3}) fps", lines[0]), lines[0]
    return read_png_rgb8(lines[1]), r.stderr


@pytest.mark.gpu
def test_the_key_changes_no_pixel_of_the_moving_object_loop(tmp_path):
    full, full_log = _run(tmp_path, "full", LOOP)
    selective, selective_log = _run(tmp_path, "selective", LOOP + "selectiveUpdate 1\n")
    # the loop says per update which path ran (twk_get_update_info): two updates in three frames, of the sphere's tree alone with the key
    assert len(re.findall(r"INFO: frame \d+, device 0: instance 6 moved by a full update, ", full_log)) == 2 and "selective update" not in full_log, full_log
    assert len(re.findall(r"INFO: frame \d+, device 0: instance 6 moved by a selective update, 1 tree\(s\) rebuilt, ", selective_log)) == 2 and "full update" not in selective_log, selective_log
    assert full.shape == selective.shape == (37, 61, 3)
    differ = (full != selective).any(-1)
    assert not differ.any(), f"{differ.sum()} of {differ.size} pixels differ"
    at_rest, rest_log = _run(tmp_path, "rest", LOOP.replace("temporalInstanceStep 6 0.0 0.2 0.15\n", "") + "selectiveUpdate 1\n")
    assert "moved by" not in rest_log
    assert not np.array_equal(at_rest, selective), "the object moves in the loop"


def test_the_key_is_parsed_and_written_back_only_when_on(twk, tmp_path):
    for extra, expect in (("", False), ("selectiveUpdate 0\n", False), ("selectiveUpdate 1\n", True), ("selectiveUpdate 1\nselectiveUpdate 7\n", True)):
        folder = tmp_path / f"case{len(os.listdir(tmp_path))}"
        folder.mkdir()
        app = twk.Application(str(_system(folder, extra)), scene_path(SCENE))
        assert app.selectiveUpdate is expect, extra
        written = app.systemDescription()
        assert ("selectiveUpdate 1" in written) is expect and ("selectiveUpdate" in written) is expect, extra
        app.close()
    L = twk._lib
    assert L.lib.twk_app_get_selective_update(None, None) == L.TWK_ERROR_INVALID_VALUE and "twk_app_get_selective_update" in L.lib.twk_last_error().decode()
