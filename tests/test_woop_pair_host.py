"""CPU: woopIntersectPair (trace_device.h: the two halves of a quad in one test) against two woopIntersect calls, through the host
compilation of the very header the kernels compile — t, beta, gamma and the verdict of BOTH triangles, bit for bit, hit or miss.
Random quads and rays, random small-integer ones (exact zeros everywhere), and constructed cases on quads with small-integer
coordinates: rays through each vertex, through points of the shared diagonal and of each outer edge, rays in the quad's plane
along the diagonal and the edges (det = 0), and a sphere's pole quad (two vertices coincide: one triangle is degenerate). The
constructed set must reach the double-precision fallback for T0 alone, for T1 alone and for both."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def pair_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("woop_pair") / "libwoop_pair_host.so")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    # the flags of the oracle's host build of the kernel headers (no contraction: every expression rounds as written)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
           "-I" + hip_inc, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"),
           "-o", out, os.path.join(ROOT, "tests", "woop_pair_host.cpp")]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.woop_pair_cases.restype = None
    lib.woop_pair_cases.argtypes = [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _run(lib, rays, quads):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
    quads = np.ascontiguousarray(quads, np.float32).reshape(-1, 12)
    n = rays.shape[0]
    assert quads.shape[0] == n
    single = np.zeros((n, 8), np.float32)
    pair = np.zeros((n, 8), np.float32)
    fallback = np.zeros((n, 2), np.int32)
    lib.woop_pair_cases(rays.ctypes.data, quads.ctypes.data, n, single.ctypes.data, pair.ctypes.data, fallback.ctypes.data)
    return single, pair, fallback


def _assert_same(single, pair, what):
    a, b = single.view(np.uint32), pair.view(np.uint32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.shape[0]} cases differ, first {bad[0]}: single {single[bad[0]]} pair {pair[bad[0]]}"


def test_random_quads_and_rays(pair_lib):
    rng = np.random.default_rng(1913)
    n = 4096
    quads = rng.uniform(-1.0, 1.0, (n, 4, 3)).astype(np.float32)
    # half of them nearly planar quads, as meshes have them
    quads[: n // 2, 3] = quads[: n // 2, 0] + (quads[: n // 2, 2] - quads[: n // 2, 1]) + rng.normal(0.0, 1e-3, (n // 2, 3)).astype(np.float32)
    o = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    wgt = rng.dirichlet(np.ones(4), n).astype(np.float32)
    target = (quads * wgt[:, :, None]).sum(axis=1)
    target[::4] += rng.normal(0.0, 0.7, (target[::4].shape)).astype(np.float32)  # a quarter aimed beside the quad
    d = (target - o).astype(np.float32)
    d[1::8] = -d[1::8]  # behind the origin
    tmin = np.where(rng.random(n) < 0.5, 0.0, 1e-4).astype(np.float32)
    single, pair, _ = _run(pair_lib, np.concatenate([o, d, tmin[:, None]], 1), quads)
    assert 0.2 < single[:, 3].mean() + single[:, 7].mean() < 1.0  # hits and misses are both well represented
    _assert_same(single, pair, "random")


def test_random_small_integer_quads_and_rays(pair_lib):
    rng = np.random.default_rng(7)
    n = 4096
    quads = rng.integers(-3, 4, (n, 4, 3)).astype(np.float32)
    o = rng.integers(-4, 5, (n, 3)).astype(np.float32)
    d = rng.integers(-2, 3, (n, 3)).astype(np.float32)
    d[(d == 0).all(axis=1)] = (0.0, 0.0, 1.0)
    single, pair, fallback = _run(pair_lib, np.concatenate([o, d, np.zeros((n, 1), np.float32)], 1), quads)
    assert fallback.any(axis=1).sum() > 400  # the inputs do what they are for: hundreds of cases take a fallback
    _assert_same(single, pair, "small integers")


def _constructed():
    """(rays [n, 7], quads [n, 12], labels)"""
    cases = []

    def add(label, quad, origin, direction, tmin=0.0):
        cases.append((label, np.asarray(quad, np.float32).reshape(12), np.asarray(list(origin) + list(direction) + [tmin], np.float32)))

    skew = [(1, 2, 0), (7, 3, 0), (8, 9, 1), (2, 7, 1)]    # no two edges parallel to an axis, not planar
    flat = [(0, 0, 0), (4, 0, 0), (4, 4, 0), (0, 4, 0)]    # a mesh's quad: planar, axis-aligned
    pole = [(0, 0, 0), (4, 0, 0), (2, 3, 1), (2, 3, 1)]    # ul == ur: T1 = (p2, p3, p0) is degenerate
    pole0 = [(2, 3, 1), (2, 3, 1), (4, 0, 0), (0, 0, 0)]   # ll == lr: T0 is degenerate
    directions = [(0, 0, -1), (1, 2, -4), (-1, 1, -2), (2, -1, -4), (0, 0, 1)]
    for name, quad in (("skew", skew), ("flat", flat), ("pole", pole), ("pole0", pole0)):
        q = np.asarray(quad, np.float64)
        points = {"p0": q[0], "p1": q[1], "p2": q[2], "p3": q[3],
                  "diagonal 1/2": (q[0] + q[2]) / 2, "diagonal 1/4": q[0] + (q[2] - q[0]) / 4,
                  "edge p0p1": (q[0] + q[1]) / 2, "edge p1p2": (q[1] + q[2]) / 2, "edge p2p3": (q[2] + q[3]) / 2, "edge p3p0": (q[3] + q[0]) / 2,
                  "inside T0": (2 * q[0] + 3 * q[1] + 3 * q[2]) / 8, "inside T1": (3 * q[2] + 3 * q[3] + 2 * q[0]) / 8,
                  "outside": q[1] + (q[1] - q[3])}
        for what, point in points.items():
            for d in directions:
                d = np.asarray(d, np.float64)
                add(f"{name}: through {what} along {tuple(d)}", quad, point - 4 * d, d)   # small integers and quarters: exact in float
                add(f"{name}: through {what} along {tuple(d)}, behind", quad, point + 4 * d, d)
        # in the quad's plane (flat, pole: planar), along the diagonal and along each outer edge: det = 0
        for a, b, what in ((0, 2, "diagonal"), (0, 1, "edge p0p1"), (1, 2, "edge p1p2"), (2, 3, "edge p2p3"), (3, 0, "edge p3p0")):
            along = q[b] - q[a]
            if not along.any():
                continue
            add(f"{name}: along {what}", quad, q[a] - along, along)
            add(f"{name}: along {what}, reversed", quad, q[b] + along, -along)
    # in the flat quad's plane, across it
    add("flat: in plane, across", flat, (-2, 1, 0), (4, 1, 0))
    add("flat: in plane, across, other axis", flat, (1, -2, 0), (1, 4, 0))
    labels = [c[0] for c in cases]
    return np.stack([c[2] for c in cases]), np.stack([c[1] for c in cases]), labels


def test_constructed_cases_reach_every_fallback_combination(pair_lib):
    rays, quads, labels = _constructed()
    single, pair, fallback = _run(pair_lib, rays, quads)
    both = fallback[:, 0] & fallback[:, 1]
    only0 = fallback[:, 0] & ~fallback[:, 1] & 1
    only1 = ~fallback[:, 0] & fallback[:, 1] & 1
    none = ((fallback[:, 0] | fallback[:, 1]) == 0)
    # counted on this set before it was committed: the fallback for T0 alone, for T1 alone, for both, and for neither
    assert only0.sum() >= 20 and only1.sum() >= 20 and both.sum() >= 40 and none.sum() >= 40, (only0.sum(), only1.sum(), both.sum(), none.sum())
    a, b = single.view(np.uint32), pair.view(np.uint32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, [(labels[i], single[i].tolist(), pair[i].tolist()) for i in bad[:5]]
    # the set holds accepted hits on either triangle and on both at once (a ray through the diagonal), and in-plane rays (det = 0: never a hit)
    assert single[:, 3].sum() >= 20 and single[:, 7].sum() >= 20 and (single[:, 3] * single[:, 7]).sum() >= 4
    in_plane = [i for i, l in enumerate(labels) if ("flat: along" in l or "flat: in plane" in l)]
    assert len(in_plane) >= 10 and not single[in_plane][:, [3, 7]].any()
