"""-m gpu: the planned adaptive loop of rtigo3_hip -m 1 ("adaptiveBudget 1" beside "adaptiveSampling 1" and a "targetNoise"), with the
description, the printed line and the checks of tests/test_gpu_adaptive_stop.py: uniform iterations up to the first check, then one
twk_adaptive_plan + one twk_launch_adaptive_planned per interval. The run meets its target before the uniform budget, the samples it
prints are the sum of the per-pixel sample counts of the same loop through the Python calls, two virtual devices that each plan
their own packed tile buffer do the same, and with "adaptiveBudget 0" the run is byte for byte the run without the key."""
import numpy as np
import pytest

import noise_restate as nr
from conftest import load_app
from test_gpu_adaptive_stop import BUDGET, INTERVAL, PIXELS, QUANTILE, RES, SCENE, _check, _run, target  # noqa: F401  (target: the fixture)

pytestmark = pytest.mark.gpu


def _replay(twk, target, plan=None):
    """INTEGRATION.md "The adaptive loop", the planned form, on one device through the Python calls: what the command line is
    expected to do."""
    app = load_app(twk, "system_rtigo3_cornell_box.txt", SCENE, RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    dev.enableAdaptive(True)
    ap = twk.Adaptive(targetNoise=target)
    plan = plan or twk.AdaptivePlan()
    for it in range(INTERVAL):
        dev.render(it)
    spent, active, end, rounds = INTERVAL * PIXELS, PIXELS, "target met", 0
    summary = dev.estimateNoise()
    adaptive = not (summary.valid > 0 and summary.quantile(QUANTILE) <= target)
    while adaptive:
        active, paths = dev.adaptivePlan(ap, plan)
        if active and paths > BUDGET - spent:  # more than is left: every selected pixel the same share of the rest
            each = min((BUDGET - spent) // active, plan.maxBatch)
            active, paths = dev.adaptivePlan(ap, twk.AdaptivePlan(minBatch=each, maxBatch=each)) if each else (active, 0)
        if active == 0:
            end = "nothing selected"
            break
        if paths == 0 or paths > BUDGET - spent:
            end = "budget spent"
            break
        dev.renderPlanned()
        spent += paths
        rounds += 1
        summary = dev.estimateNoise()
        if summary.valid > 0 and summary.quantile(QUANTILE) <= target:
            break
    restated, _ = nr.summary(dev.readMoments().reshape(-1, 4))
    assert nr.same(nr.as_dict(summary), restated)  # the last check saw the frame as it was left
    counts = dev.readSampleCounts()
    assert int(counts.astype(np.int64).sum()) == spent  # the samples the loop counts are the samples the pixels hold
    out = {"adaptive": adaptive, "spent": spent, "active": active, "end": end, "quantile": float(nr.quantile(restated, QUANTILE)), "mean": float(nr.mean(restated)),
           "largest": int(counts.max()), "spp": -(-spent // PIXELS), "rounds": rounds, "distinct": int(np.unique(counts).size)}
    dev.close()
    return out


def test_the_planned_loop_meets_the_target_inside_the_budget(twk, tmp_path, target):
    want = _replay(twk, target)
    print("\nplanned replay:", want)
    assert _check(tmp_path, "plan", _run(tmp_path, "plan", target, "adaptiveBudget 1\n"), want, target) == "target met"
    assert want["spent"] < BUDGET and want["rounds"] >= 1 and want["distinct"] >= 3  # before the uniform budget, by passes whose pixels got different numbers
    # two virtual devices, each planning its own packed tile buffer: the same pixels, the same samples, the same end
    assert _check(tmp_path, "plan2", _run(tmp_path, "plan2", target, "adaptiveBudget 1\n", env={"TWK_CLI_VIRTUAL_DEVICES": "2"}), want, target) == "target met"
    # other batches are other plans
    small = _replay(twk, target, twk.AdaptivePlan(minBatch=1, maxBatch=5))
    assert _check(tmp_path, "plan5", _run(tmp_path, "plan5", target, "adaptiveBudget 1\nadaptiveMinBatch 1\nadaptiveMaxBatch 5\n"), small, target) in ("target met", "budget spent", "nothing selected")


def test_the_key_off_is_the_run_without_the_key(tmp_path, target):
    absent = _run(tmp_path, "absent", target)
    off = _run(tmp_path, "off", target, "adaptiveBudget 0\nadaptiveMinBatch 2\nadaptiveMaxBatch 9\n")
    assert len(absent) == len(off) == 3 and absent[1] == off[1]  # the same samples, the same figures
    assert open(absent[2], "rb").read() == open(off[2], "rb").read()  # and the same screenshot, byte for byte
