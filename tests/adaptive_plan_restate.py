"""csrc/adaptive_plan_device.h again in numpy float32, statement for statement: the sample budget a planned adaptive pass gives each
element of a stream of luminance moments and sample counts, and the plan, the ascending list of the elements with a budget beside
the exclusive prefix sum of their budgets. Who is in the plan is adaptive_restate.selected, the classification noise_restate.classify.
tests/test_adaptive_plan_host.py holds twk_adaptive_plan_host to it and tests/test_gpu_adaptive_plan.py the kernels."""
import numpy as np

import adaptive_restate as ar
import noise_restate as nr

F = np.float32


def budgets(moments, counts, min_batch=4, max_batch=64, target_noise=0.05, min_samples=4, dark_floor=0.01, max_samples=4096):
    """uint32 [N] of moments float32 [N, 4] = (mean, M2, n, .) and counts uint32 [N]; the steps in the order of adaptiveBudget."""
    m = np.ascontiguousarray(moments, F).reshape(-1, 4)
    counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
    chosen = ar.selected(m, counts, target_noise=target_noise, min_samples=min_samples, dark_floor=dark_floor, max_samples=max_samples)
    cls, e = nr.classify(m, min_samples, dark_floor)
    n = m[:, 2]
    with np.errstate(all="ignore"):
        r = e / F(target_noise)
        q = r * r
        need = n * q
        extra = need - n
        assert extra.dtype == F
        top = ~(extra < F(max_batch))                                           # the negated comparison: inf and NaN land here
        rounded = np.ceil(np.where(top, F(0.0), extra)).astype(np.int64)        # (uint32) ceilf(extra), of a value in [0, maxBatch)
    b = np.where(top, np.int64(max_batch), rounded)
    b = np.maximum(b, np.int64(min_batch))                                      # 3. VALID: the prediction, at least minBatch
    b = np.where(cls == nr.UNKNOWN, np.int64(min_batch), b)                     # 2. UNKNOWN: minBatch
    left = np.int64(max_samples) - counts.astype(np.int64)
    b = np.minimum(b, left)                                                     # 4. the room maxSamples leaves
    b = np.where(chosen, b, 0)                                                  # 1. not selected: 0
    assert (b[chosen] >= 1).all() and (b <= max_batch).all()
    return b.astype(np.uint32)


def plan(moments, counts, **parameters):
    """(active uint32 [numActive], pathOffset uint32 [numActive + 1], numPaths int): the elements with a budget, ascending, the
    exclusive prefix sum of their budgets with the total as its last word (the low 32 bits, as the C arrays hold it), and the total."""
    b = budgets(moments, counts, **parameters)
    active = np.flatnonzero(b > 0).astype(np.uint32)
    offsets = np.zeros(active.size + 1, np.uint64)
    np.cumsum(b[active], dtype=np.uint64, out=offsets[1:])
    return active, (offsets & np.uint64(0xFFFFFFFF)).astype(np.uint32), int(offsets[-1])


def parameters(ap, pl):
    """The keyword arguments of budgets() for a tweeker_raytracer_amd Adaptive and AdaptivePlan."""
    return {"min_batch": pl.minBatch, "max_batch": pl.maxBatch, **ar.parameters(ap)}
