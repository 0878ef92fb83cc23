"""-m gpu: the adaptive loop of rtigo3_hip -m 1 ("targetNoise" with "adaptiveSampling 1" in the system description): uniform
iterations up to the first check, then rounds of select + "targetNoiseInterval" samples on the selected pixels. The run ends, prints
the samples per pixel and the active share, spends no more than samplesSqrt² x pixels samples, and does what the same loop does
through the Python calls, whose final quantile is recomputed from the read-back moments by tests/noise_restate.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import noise_restate as nr
from conftest import load_app, scene_path
from test_screenshot_files import CLI

pytestmark = pytest.mark.gpu

F = np.float32
RES = (96, 64)
SCENE = "scene_rtigo3_cornell_box.txt"
INTERVAL, SAMPLES_SQRT, QUANTILE = 8, 8, 0.95
PIXELS = RES[0] * RES[1]
BUDGET = SAMPLES_SQRT ** 2 * PIXELS


def _replay(twk, target, cap=4096):
    """INTEGRATION.md "The adaptive loop" on one device through the Python calls: what the command line is expected to do."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", SCENE, RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    dev.enableAdaptive(True)
    ap = twk.Adaptive(targetNoise=target, maxSamples=cap)
    for it in range(INTERVAL):
        dev.render(it)
    spent, active, end = INTERVAL * PIXELS, PIXELS, "target met"
    summary = dev.estimateNoise()
    adaptive = not (summary.valid > 0 and summary.quantile(QUANTILE) <= target)
    while adaptive:
        active = dev.adaptiveSelect(ap)
        if active == 0:
            end = "nothing selected"
            break
        samples = min(INTERVAL, (BUDGET - spent) // active)
        if samples == 0:
            end = "budget spent"
            break
        dev.renderAdaptive(samples)
        spent += active * samples
        summary = dev.estimateNoise()
        if summary.valid > 0 and summary.quantile(QUANTILE) <= target:
            break
    restated, _ = nr.summary(dev.readMoments().reshape(-1, 4))
    assert nr.same(nr.as_dict(summary), restated)  # the last check saw the frame as it was left
    out = {"adaptive": adaptive, "spent": spent, "active": active, "end": end, "quantile": float(nr.quantile(restated, QUANTILE)), "mean": float(nr.mean(restated)),
           "largest": int(dev.readSampleCounts().max()), "spp": -(-spent // PIXELS)}
    dev.close()
    return out


@pytest.fixture(scope="module")
def target(twk):
    """From the data: the 0.95 quantile edge a uniform render has after 24 iterations. The first check, at 8, is above it; the
    adaptive rounds reach it well inside the budget of 64 samples per pixel."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", SCENE, RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    edges = {}
    for it in range(24):
        dev.render(it)
        if it + 1 in (INTERVAL, 24):
            edges[it + 1] = dev.estimateNoise().quantile(QUANTILE)
    dev.close()
    assert edges[24] < edges[INTERVAL]
    return float(F(edges[24]))


def _run(tmp_path, name, target, extra="", env=None):
    text = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    text = re.sub(r"(?m)^resolution .*$", f"resolution {RES[0]} {RES[1]}", text)
    text = re.sub(r"(?m)^samplesSqrt .*$", f"samplesSqrt {SAMPLES_SQRT}", text)
    text = re.sub(r"(?m)^strategy .*$", f"strategy {3 if env else 0}", text)
    text += f"\nprefixScreenshot {tmp_path}/{name}\ntargetNoise {float(F(target))!r}\ntargetNoiseInterval {INTERVAL}\nadaptiveSampling 1\n{extra}"
    system = tmp_path / f"system_{name}.txt"
    system.write_text(text)
    r = subprocess.run([CLI, "-s", str(system), "-d", scene_path(SCENE), "-m", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120, env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


LINE = re.compile(r"noise: (\d+) spp, mean (\S+), (\S+) quantile at most (\S+), target (\S+), adaptive: mean (\S+) spp, max (\d+) spp, "
                  r"last active share (\S+), samples (\d+) of (\d+), ended: (target met|nothing selected|budget spent)$")


def _check(tmp_path, name, lines, want, target):
    print("\n" + "\n".join(lines[:2]), "\nreplay:", want)
    assert len(lines) == 3, lines
    m = LINE.match(lines[1])
    assert m, lines[1]
    spp, mean, q, edge, t, mean_spp, largest, share, spent, budget, end = m.groups()
    assert want["adaptive"]  # the case is one in which the first check does not meet the target
    assert int(budget) == BUDGET and int(spent) <= BUDGET  # no more than the uniform budget
    assert (int(spent), end, int(largest), int(spp)) == (want["spent"], want["end"], want["largest"], want["spp"])
    assert float(mean_spp) == float(f"{want['spent'] / PIXELS:.6g}") and float(share) == float(f"{want['active'] / PIXELS:.6g}")
    assert float(edge) == float(f"{want['quantile']:.6g}") and float(mean) == float(f"{want['mean']:.6g}") and float(t) == float(f"{F(target):.6g}")
    assert (end == "target met") == (want["quantile"] <= target)  # met, or one of the two other ends held
    assert re.fullmatch(rf"{int(spp)} / (\d+\.\d{{3}}) = (\d+\.\d{{3}}) fps", lines[0]), lines[0]
    assert re.fullmatch(rf"{re.escape(str(tmp_path))}/{name}_{int(spp)}spp_\d{{7}}_\d{{6}}_000\.png", lines[2]) and os.path.getsize(lines[2]) > 1000, lines[2]
    return end


def test_the_adaptive_loop_meets_the_target_inside_the_budget(twk, tmp_path, target):
    want = _replay(twk, target)
    assert _check(tmp_path, "met", _run(tmp_path, "met", target), want, target) == "target met"
    assert want["spent"] < 24 * PIXELS  # fewer samples than the uniform render that defined the target
    # two virtual devices, each selecting on its own packed tile buffer: the same pixels, the same samples, the same end
    assert _check(tmp_path, "met2", _run(tmp_path, "met2", target, env={"TWK_CLI_VIRTUAL_DEVICES": "2"}), want, target) == "target met"


def test_the_other_two_ends(twk, tmp_path):
    tiny = 2.0 ** -16  # no bin's upper edge lies below it: never met
    assert _check(tmp_path, "cap", _run(tmp_path, "cap", tiny, "adaptiveMaxSamples 20\n"), _replay(twk, tiny, cap=20), tiny) == "nothing selected"
    assert _check(tmp_path, "budget", _run(tmp_path, "budget", tiny), _replay(twk, tiny), tiny) == "budget spent"
