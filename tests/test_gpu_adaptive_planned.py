"""-m gpu: the planned adaptive pass (twk_adaptive_plan + twk_launch_adaptive_planned) against the library's own uniform render, with
the scenes, formats and helpers of tests/test_gpu_adaptive.py. The invariant is that test's: after uniform launches 0 .. K-1 and any
planned passes, a launch index whose sample count is c holds in colour, both AOVs and moments exactly the bits it holds after
twk_launch(0 .. c-1) on a fresh handle. The schedule: four uniform iterations, then three rounds of plan + planned pass with
minBatch 1, maxBatch 7; the target of a round is the median of that round's valid errors. Every round's plan equals
tests/adaptive_plan_restate.py, holds at least three distinct budgets (what makes the pass a planned one and not a fixed batch),
and advances every count by exactly its budget."""
import numpy as np
import pytest

import adaptive_plan_restate as apr
import noise_restate as nr
from test_gpu_adaptive import NAMES, SCENES, UNIFORM, _assemble, _assert_invariant, _device, _read, _refused, _uniform

pytestmark = pytest.mark.gpu

ROUNDS, MIN_BATCH, MAX_BATCH = 3, 1, 7


def _schedule(twk, dev, cap=4096, targets=None):
    """Four uniform iterations, three rounds of plan + renderPlanned; checks each round's plan against the restatement, the spread
    of its budgets and the counts' advance. Returns (targets, budgets of every round [N], counts after the last round, per round how
    many budgets the cap clipped)."""
    for it in range(UNIFORM):
        dev.render(it)
    pl = twk.AdaptivePlan(minBatch=MIN_BATCH, maxBatch=MAX_BATCH)
    used, rounds, clipped = [], [], []
    for r in range(ROUNDS):
        m = dev.readMoments().reshape(-1, 4)
        counts = dev.readSampleCounts().reshape(-1)
        if r == 0:
            assert (counts == UNIFORM).all()
        cls, e = nr.classify(m)
        target = float(np.median(e[cls == nr.VALID])) if targets is None else targets[r]
        ap = twk.Adaptive(targetNoise=target, maxSamples=cap)
        num_active, num_paths = dev.adaptivePlan(ap, pl)
        active, offsets = dev.readPlan()
        w_active, w_offsets, w_paths = apr.plan(m, counts, **apr.parameters(ap, pl))
        assert (num_active, num_paths) == (w_active.size, w_paths) and np.array_equal(active, w_active) and np.array_equal(offsets, w_offsets), f"round {r}"
        b = apr.budgets(m, counts, **apr.parameters(ap, pl)).astype(np.int64)
        distinct = np.unique(b[b > 0])
        print(f"round {r}: target {target:.4f}, {num_active} entries, {num_paths} paths, budgets {dict(zip(*[x.tolist() for x in np.unique(b, return_counts=True)]))}")
        if targets is None:  # the condition the schedule rests on
            assert distinct.size >= 3, f"round {r}: the budgets take the values {distinct.tolist()} only"
            assert (b == 0).any() and ((b == 0) & (cls == nr.VALID)).any()
        dev.renderPlanned()
        after = dev.readSampleCounts().reshape(-1)
        assert np.array_equal(after.astype(np.int64) - counts, b), f"round {r}: every count advances by its budget"
        free = apr.budgets(m, counts, **{**apr.parameters(ap, pl), "max_samples": 1 << 30}).astype(np.int64)  # what the same plan gives without the cap
        assert (b <= free).all() and np.array_equal(b, np.minimum(free, np.maximum(cap - counts.astype(np.int64), 0)))
        used.append(target)
        rounds.append(b)
        clipped.append(int((b < free).sum()))
    return used, rounds, dev.readSampleCounts(), clipped


@pytest.mark.parametrize("scene,half,cap", [("cornell", False, 4096), ("cornell", True, 4096), ("fuzz", False, 4096), ("fuzz", True, 4096), ("cornell", False, 10)])
def test_a_pixel_with_count_c_holds_the_bits_of_c_uniform_launches(twk, scene, half, cap):
    dev = _device(twk, scene, half)
    targets, rounds, counts, clipped = _schedule(twk, dev, cap)
    got = _read(dev, half)
    if cap == 10:  # the cap clips some budgets: a pixel that would pass it gets the room that is left, and is left out once there
        flat = counts.reshape(-1)
        assert flat.max() == 10 and (flat <= 10).all()
        before_last = UNIFORM + rounds[0] + rounds[1]
        assert sum(clipped) > 0 and (before_last >= 10).any() and not rounds[2][before_last >= 10].any()
    else:
        assert sum(clipped) == 0
    distinct = _assert_invariant(twk, scene, half, got, counts)
    print(f"{scene} half={half} cap={cap}: targets {[round(t, 4) for t in targets]}, counts {distinct.tolist()}")
    assert distinct.size >= 4 and distinct.min() == UNIFORM  # many histories in one picture, one of them purely uniform
    dev.close()


@pytest.mark.parametrize("scene", SCENES)
def test_two_tiled_handles_equal_one(twk, scene):
    single = _device(twk, scene, False)
    targets, _, counts, _ = _schedule(twk, single)
    whole = _read(single, False) + [counts[..., None]]
    tile = (single.state.tileSize[0], single.state.tileSize[1])
    single.close()
    parts = []
    for index in range(2):
        dev = _device(twk, scene, False, index=index, count=2)
        _, _, c, _ = _schedule(twk, dev, targets=targets)
        parts.append(_read(dev, False) + [c[..., None]])
        dev.close()
    for name, x, y in zip(NAMES + ("counts",), _assemble(twk, parts, tile), whole):
        assert np.array_equal(x, y), name


def test_sample_offset_gives_the_bits_of_a_uniform_render_with_it(twk):
    dev = _device(twk, "cornell", False, offset=7)
    _, _, counts, _ = _schedule(twk, dev)
    got = _read(dev, False)
    dev.close()
    _assert_invariant(twk, "cornell", False, got, counts, offset=7)


def test_launch_rules_of_a_plan(twk):
    L = twk._lib
    dev = _device(twk, "cornell", False)
    _refused(twk, lambda: dev.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_launch_adaptive_planned", "twk_adaptive_plan")  # before any plan
    _refused(twk, lambda: dev.readPlan(), L.TWK_ERROR_INVALID_STATE, "twk_read_plan")
    for it in range(UNIFORM):
        dev.render(it)
    pl = twk.AdaptivePlan(minBatch=MIN_BATCH, maxBatch=MAX_BATCH)
    fine = twk.Adaptive(targetNoise=1e-6)
    n, paths = dev.adaptivePlan(fine, pl)
    assert n > 0 and paths >= n
    dev.render(UNIFORM)  # still uniform: allowed, and it drops the plan
    _refused(twk, lambda: dev.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_plan")
    # a plan leaves the select's list what it is, a select drops the plan
    listed = dev.adaptiveSelect(fine)
    first = dev.readActive()
    n, paths = dev.adaptivePlan(twk.Adaptive(targetNoise=0.2), pl)
    assert 0 < n < listed and np.array_equal(dev.readActive(), first)
    dev.adaptiveSelect(fine)
    _refused(twk, lambda: dev.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_plan")
    # a plan is rendered once
    n, paths = dev.adaptivePlan(fine, pl)
    active, offsets = dev.readPlan()
    assert active.size == n and offsets[-1] == paths
    dev.renderPlanned()
    counts = dev.readSampleCounts().copy()
    _refused(twk, lambda: dev.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_launch_adaptive_planned", "twk_adaptive_plan")
    _refused(twk, lambda: dev.readPlan(), L.TWK_ERROR_INVALID_STATE, "twk_read_plan")
    assert np.array_equal(dev.readSampleCounts(), counts)
    # the picture holds adaptive samples: only a restart at 0 is a uniform launch
    _refused(twk, lambda: dev.render(5), L.TWK_ERROR_INVALID_STATE, "twk_launch", "iteration 0")
    dev.adaptivePlan(fine, pl)
    dev.renderPlanned()  # the refused launch has dropped nothing that a new plan does not bring back
    dev.render(0)  # restarts a uniform frame
    _refused(twk, lambda: dev.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_plan")
    dev.render(1)
    dev.render(2)
    got = _read(dev, False)
    for name, g, w in zip(NAMES, got, _uniform(twk, "cornell", False, [3])[3]):
        assert np.array_equal(g, w), name
    # what drops a list drops a plan
    for name, change in (("state", lambda d: d.setState(d.state)), ("format", lambda d: d.setOutputFormat(L.TWK_OUTPUT_HALF4)), ("build", lambda d: d.build()),
                         ("switch", lambda d: (d.enableAdaptive(False), d.enableAdaptive(True)))):
        dev.render(0)
        assert dev.adaptivePlan(fine, pl)[0] > 0
        change(dev)
        _refused(twk, lambda: dev.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_launch_adaptive_planned")
        _refused(twk, lambda: dev.readPlan(), L.TWK_ERROR_INVALID_STATE, "twk_read_plan")
    dev.close()
    plain = _device(twk, "cornell", False, adaptive=False)
    _refused(twk, lambda: plain.adaptivePlan(), L.TWK_ERROR_INVALID_STATE, "twk_enable_adaptive")
    _refused(twk, lambda: plain.renderPlanned(), L.TWK_ERROR_INVALID_STATE, "twk_enable_adaptive")
    plain.close()
