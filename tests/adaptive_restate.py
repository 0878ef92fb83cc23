"""csrc/adaptive_device.h again in numpy float32, statement for statement: which elements of a stream of luminance moments and
sample counts an adaptive pass samples, and the active list, their indices in ascending order. The classification it starts from
is noise_restate.classify. tests/test_adaptive_host.py holds twk_adaptive_select_host to it and tests/test_gpu_adaptive_select.py
the kernels."""
import numpy as np

import noise_restate as nr

F = np.float32


def selected(moments, counts, target_noise=0.05, min_samples=4, dark_floor=0.01, max_samples=4096):
    """bool [N] of moments float32 [N, 4] = (mean, M2, n, .) and counts uint32 [N]; the tests in the order of adaptiveSelected."""
    cls, e = nr.classify(moments, min_samples, dark_floor)
    counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
    out = np.zeros(cls.shape, bool)
    decided = np.zeros(cls.shape, bool)
    empty = cls == nr.EMPTY                               # 1. EMPTY: not selected
    decided |= empty
    capped = ~decided & (counts >= np.uint32(max_samples))  # 2. the count has reached maxSamples: not selected
    decided |= capped
    unknown = ~decided & (cls == nr.UNKNOWN)              # 3. UNKNOWN: selected
    out |= unknown
    decided |= unknown
    valid = ~decided                                      # 4. VALID: selected exactly when e > targetNoise
    out |= valid & (e > F(target_noise))
    return out


def active_list(moments, counts, **parameters):
    """uint32 [numActive]: the selected indices, ascending."""
    return np.flatnonzero(selected(moments, counts, **parameters)).astype(np.uint32)


def parameters(ap):
    """The keyword arguments of selected() for a tweeker_raytracer_amd Adaptive."""
    return {"target_noise": F(ap.targetNoise), "min_samples": ap.minSamples, "dark_floor": F(ap.darkFloor), "max_samples": ap.maxSamples}


def mixed_moments(rng, n, target_noise=0.05, min_samples=4, dark_floor=0.01):
    """float32 [n, 4] that mixes every class: n == 0 and -0, n < minSamples, NaN and inf in each component, negative M2 and mean,
    a M2 of -0, e far from, next to and exactly equal to the target, and ordinary triples on both sides of it."""
    m = np.zeros((n, 4), F)
    m[:, 0] = rng.uniform(0.0, 2.0, n)
    m[:, 2] = rng.integers(min_samples, 64, n)
    e_wanted = (F(target_noise) * rng.choice([0.25, 0.5, 0.999, 1.0, 1.001, 2.0, 4.0], n)).astype(F)
    # M2 that gives about e_wanted: e = sqrt(M2 / ((n - 1) n)) / (mean + floor)
    m[:, 1] = (e_wanted * (m[:, 0] + F(dark_floor))) ** 2 * (m[:, 2] - 1) * m[:, 2]
    m[:, 3] = rng.uniform(-1, 1, n)
    kind = rng.integers(0, 20, n)
    m[kind == 0, 2] = 0.0
    m[kind == 1, 2] = -0.0
    m[kind == 2, 2] = rng.integers(1, min_samples, (kind == 2).sum())
    for k, (column, value) in enumerate([(0, np.nan), (1, np.nan), (2, np.nan), (0, np.inf), (1, np.inf), (2, np.inf), (0, -np.inf)]):
        m[kind == 3 + k, column] = value
    m[kind == 10, 1] *= -1
    m[kind == 11, 0] *= -1
    m[kind == 12, 1] = -0.0
    # e exactly equal to the target: mean + floor = 1 in float32 arithmetic, n = 4, M2 = 12 t^2 with t a power of two -> s = t
    exact = kind == 13
    m[exact, 0] = F(1.0) - F(dark_floor)
    m[exact, 2] = 4.0
    m[exact, 1] = F(12.0) * F(target_noise) * F(target_noise)
    return m
