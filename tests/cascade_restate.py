"""The firefly cascade of csrc/cascade_device.h again in numpy float32, statement for statement: the threshold table, the fold of
kept samples into the layers and the resolve. Every operation is one float32 operation, rounded once, in the header's order; the
tests compare words. No test in here: tests/test_cascade_host.py and the tests/test_gpu_cascade*.py use it."""
import numpy as np

from test_moments_host import F, kept_radiance, luminance

MAX_LAYERS = 8


def thresholds(layers=6, start=1.0, base=8.0):
    """b[0] = start, b[j + 1] = b[j] * base by repeated float32 multiplication (cascadeConstants)."""
    b = [F(start)]
    for _ in range(1, int(layers)):
        b.append(F(b[-1] * F(base)))
    return np.array(b, F)


def fold(samples, first_iteration, layers, b, debug_exceptions=False, branches=None):
    """cascadeFoldSample over samples [S, ..., 4] (iterations first_iteration ...) on layers [K, ..., 4]; returns the new layers.
    branches: a dict that receives how many kept samples took each branch."""
    K = len(b)
    L = np.array(layers, F)
    assert L.shape[0] == K and 2 <= K <= MAX_LAYERS
    count = {"below_start": 0, "at_threshold": 0, "interior": 0, "clamp": 0, "rejected": 0, "weight_zero_interior": 0}
    with np.errstate(all="ignore"):
        for s, sample in enumerate(samples):
            rgb, keep = kept_radiance(sample, debug_exceptions)
            sums = L[..., :3].copy()
            n = L[0, ..., 3].copy()
            rejected = L[K - 1, ..., 3].copy()
            if first_iteration + s == 0:
                sums[...] = 0
                n[...] = 0
                rejected[...] = 0
            n = n + F(1.0)
            finite = np.isfinite(rgb).all(axis=-1)
            rejected = np.where(finite, rejected, rejected + F(1.0))
            l = luminance(rgb)
            j = np.zeros(l.shape, np.int64)
            for i in range(1, K - 1):
                j = np.where(b[i] <= l, i, j)
            lo, hi = b[j], b[j + 1]
            q = lo / hi
            interior = (lo / l - q) / (F(1.0) - q)
            below, inside = l <= lo, (l > lo) & (l < hi)
            w_lo = np.where(below, F(1.0), np.where(inside, interior, F(0.0))).astype(F)
            w_hi = np.where(below, F(0.0), np.where(inside, F(1.0) - w_lo, hi / l)).astype(F)
            for i in range(K):
                w = np.where(i == j, w_lo, np.where(i == j + 1, w_hi, F(0.0))).astype(F)
                add = finite & (w != 0)
                sums[i] = np.where(add[..., None], sums[i] + w[..., None] * rgb, sums[i])
            new = np.zeros_like(L)
            new[..., :3] = sums
            new[0, ..., 3] = n
            new[K - 1, ..., 3] = rejected
            L = np.where(keep[None, ..., None], new, L)
            kept = keep & finite
            count["rejected"] += int((keep & ~finite).sum())
            count["below_start"] += int((kept & (l < b[0])).sum())
            count["at_threshold"] += int((kept & (l == lo)).sum())
            count["interior"] += int((kept & inside).sum())
            count["clamp"] += int((kept & ~below & ~inside).sum())
            count["weight_zero_interior"] += int((kept & inside & ((w_lo == 0) | (w_hi == 0))).sum())
    if branches is not None:
        for key, value in count.items():
            branches[key] = branches.get(key, 0) + value
    assert L.dtype == F
    return L


def resolve(layers, b, kappa, fallback=None):
    """cascadeResolvePixel over layers [K, H, W, 4]: float32 [H, W, 4], not narrowed. fallback: a list that receives the mask of
    the pixels that took the plain quotient."""
    L = np.ascontiguousarray(layers, F)
    K, H, W = L.shape[:3]
    assert K == len(b)
    kappa = F(kappa)
    with np.errstate(all="ignore"):
        lam = luminance(L[..., :3])
        n = L[0, ..., 3]
        acc = L[0, ..., :3].copy()
        total = L[0, ..., :3].copy()
        plain = np.zeros((H, W), bool)
        for j in range(1, K):
            a = lam[j - 1] + lam[j]
            if j < K - 1:
                a = a + lam[j + 1]
            S = np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
                    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
                    S[yd, xd] = S[yd, xd] + a[ys, xs]
            c = S / b[j]
            plain |= ~np.isfinite(c)
            t = c / kappa
            w = np.where(t < F(1.0), t, F(1.0)).astype(F)
            acc = acc + w[..., None] * L[j, ..., :3]
            total = total + L[j, ..., :3]
        rgb = np.where(plain[..., None], total / n[..., None], acc / n[..., None])
        out = np.concatenate([rgb, np.ones((H, W, 1), F)], axis=-1).astype(F)
        out[(n == 0) | ~np.isfinite(n)] = 0
    if fallback is not None:
        fallback.append(plain & ~((n == 0) | ~np.isfinite(n)))
    return out
