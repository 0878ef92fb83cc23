"""csrc/noise_device.h again in numpy float32, statement for statement: the class of every element of a stream of luminance
moments, the relative standard error e of a valid one, its histogram bin and fixed-point value, the summary, the merge of two
summaries and the quantile edge. tests/test_noise_host.py holds the C helpers to it and tests/test_gpu_noise.py the kernel."""
from fractions import Fraction

import numpy as np

F = np.float32
VALID, UNKNOWN, EMPTY = 0, 1, 2
BIN_BASE = (127 - 16) << 3


def classify(moments, min_samples=4, dark_floor=0.01):
    """(class int32 [N], e float32 [N]; e is 0 where the class is not VALID) of moments float32 [N, 4] = (mean, M2, n, .)."""
    m = np.ascontiguousarray(moments, F).reshape(-1, 4)
    mean, m2, n = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        empty = n == F(0.0)
        finite = np.isfinite(mean) & np.isfinite(m2) & np.isfinite(n)
        unknown = ~empty & (~finite | (n < F(min_samples)) | (m2 < F(0.0)) | (mean < F(0.0)))
        candidate = ~empty & ~unknown
        d = (n - F(1.0)) * n
        v = m2 / d
        s = np.sqrt(v)
        e = s / (mean + F(dark_floor))
        assert e.dtype == F
        e = (e.view(np.uint32) & np.uint32(0x7fffffff)).view(F)  # a M2 of -0 gives e = -0: the sign bit is cleared
        bad = candidate & ~np.isfinite(e)
    cls = np.where(empty, EMPTY, np.where(unknown | bad, UNKNOWN, VALID)).astype(np.int32)
    return cls, np.where(cls == VALID, e, F(0.0)).astype(F)


def bins(e):
    return np.clip((e.view(np.uint32) >> np.uint32(20)).astype(np.int64) - BIN_BASE, 0, 255)


def fixed(e):
    return np.rint(np.minimum(e, F(65536.0)) * F(1048576.0)).astype(np.uint64)


def error_map(cls, e):
    return np.where(cls == VALID, e, np.where(cls == UNKNOWN, F(-1.0), F(-2.0))).astype(F)


def summary(moments, min_samples=4, dark_floor=0.01):
    """The summary as a dict of Python ints and a uint32 [256] histogram, and the error map float32 [N]."""
    cls, e = classify(moments, min_samples, dark_floor)
    ev = e[cls == VALID]
    out = {"valid": int((cls == VALID).sum()), "unknown": int((cls == UNKNOWN).sum()), "empty": int((cls == EMPTY).sum()),
           "sumFixed": int(fixed(ev).sum(dtype=np.uint64)) if ev.size else 0,
           "maxErrorBits": int(ev.view(np.uint32).max()) if ev.size else 0,
           "histogram": np.bincount(bins(ev), minlength=256).astype(np.uint32)}
    return out, error_map(cls, e)


def merge(a, b):
    return {"valid": a["valid"] + b["valid"], "unknown": a["unknown"] + b["unknown"], "empty": a["empty"] + b["empty"],
            "sumFixed": (a["sumFixed"] + b["sumFixed"]) % (1 << 64), "maxErrorBits": max(a["maxErrorBits"], b["maxErrorBits"]),
            "histogram": (a["histogram"].astype(np.uint64) + b["histogram"]).astype(np.uint32)}


def mean(s):
    """sumFixed / 2^20 / valid in double, narrowed once."""
    return F(np.float64(s["sumFixed"]) / np.float64(1048576.0) / np.float64(s["valid"]))


def bin_upper_edge(b):
    return np.array([(b + 1 + BIN_BASE) << 20], np.uint32).view(F)[0]


def quantile(s, q):
    """The upper edge of the first bin at which the cumulative count reaches ceil(q valid), q a float32 in (0, 1]; the ceiling is
    taken of the exact product (a float32 is a rational)."""
    exact = Fraction(float(F(q))) * s["valid"]
    need = -((-exact.numerator) // exact.denominator)
    seen = 0
    for b in range(256):
        seen += int(s["histogram"][b])
        if seen >= need:
            return bin_upper_edge(b)
    return bin_upper_edge(255)


def as_dict(c_summary):
    """A tweeker_raytracer_amd NoiseSummary in the form summary() returns."""
    return {"valid": int(c_summary.valid), "unknown": int(c_summary.unknown), "empty": int(c_summary.empty), "sumFixed": int(c_summary.sumFixed),
            "maxErrorBits": int(c_summary.maxErrorBits), "histogram": c_summary.histogram}


def same(a, b):
    return all(a[k] == b[k] for k in ("valid", "unknown", "empty", "sumFixed", "maxErrorBits")) and np.array_equal(a["histogram"], b["histogram"])
