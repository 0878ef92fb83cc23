"""The inputs of tests/test_bvh_audit_host.py and tests/test_gpu_bvh_audit.py: meshes as data, seeded. A helper module, not a conftest.

A mesh is (attributes [v, 12], indices [3 t]) in a unit cube about the origin unless its name says otherwise; a case is a list of
meshes that one scene holds side by side, every mesh referenced by one instance whose transform is selective_scenes.rotated (a
rotation with a non-uniform scale) to a place of its own."""
import functools
import os
import re

import numpy as np

import selective_scenes as S

F32 = np.float32
# build primitives per geometry: the single-leaf node, the flatten threshold and the direct-leaf rule (1 .. 5), SAH_SMALL and its
# neighbours (7, 8, 9), the bin count (16, 17), a wave and a block (63 .. 65, 255 .. 257), several blocks and one odd (1023, 1025),
# and one size with several large levels (4097)
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
ODD = (9, 65, 257)
DISTRIBUTION_SIZES = (257, 1025)
WELL_BEHAVED = ("uniform", "sphere", "clusters")
DEGENERATE = ("identical", "line", "plane", "sixteenths", "far", "spanning", "zero-area")
EVERYTHING_FLAT = (1 << 20, 1 << 20)


def attributes(vertices, rng):
    """TriangleAttributes from positions: a random unit tangent and normal and a random texcoord per vertex, so that a shading record
    that holds another vertex's shows."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    a = np.zeros((v.shape[0], 12), F32)
    a[:, 0:3] = v
    for first in (3, 6):
        d = rng.normal(0.0, 1.0, (v.shape[0], 3))
        a[:, first:first + 3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    a[:, 9:11] = rng.uniform(0.0, 1.0, (v.shape[0], 2))
    return a


def soup(centres, rng, size=0.05, shape=None):
    """One triangle per centre, no shared vertices, no pairs. shape [3, 3]: every triangle is that one, translated."""
    c = np.asarray(centres, np.float64).reshape(-1, 1, 3)
    tri = rng.normal(0.0, size, (c.shape[0], 3, 3)) if shape is None else np.broadcast_to(np.asarray(shape, np.float64), (c.shape[0], 3, 3))
    return attributes((c + tri).reshape(-1, 3), rng), np.arange(3 * c.shape[0], dtype=np.uint32)


def quads(centres, rng, size=0.05, extra=()):
    """One quad per centre as the triangles (a, b, c), (c, d, a): all pairs. extra: "broken" adds a quad whose second triangle is
    wound (d, a, c) and does not pair, "trailing" one more triangle at the end."""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    vertices, indices = [], []

    def quad(at, second):
        u, w = rng.normal(0.0, size, 3), rng.normal(0.0, size, 3)
        b = len(vertices)
        vertices.extend([at, at + u, at + u + w, at + w])
        indices.extend([b, b + 1, b + 2] + [b + k for k in second])

    for k in range(c.shape[0]):
        if "broken" in extra and k == c.shape[0] // 2:
            quad(rng.uniform(-0.5, 0.5, 3), (3, 0, 2))
        quad(c[k], (2, 3, 0))
    if "trailing" in extra:
        b = len(vertices)
        vertices.extend(rng.uniform(-0.5, 0.5, 3) + rng.normal(0.0, size, (3, 3)))
        indices.extend([b, b + 1, b + 2])
    return attributes(np.array(vertices), rng), np.array(indices, np.uint32)


def sized(n, kind, rng):
    """A mesh of n build primitives: "soup", "quads", or "odd" (a quad mesh with one quad that does not pair and one trailing triangle)."""
    if kind == "soup":
        return soup(rng.uniform(-0.5, 0.5, (n, 3)), rng)
    if kind == "quads":
        return quads(rng.uniform(-0.5, 0.5, (n, 3)), rng)
    return quads(rng.uniform(-0.5, 0.5, (n - 3, 3)), rng, extra=("broken", "trailing"))  # n - 3 pairs + 2 triangles of the broken quad + 1


def quad_sphere(tess, rng):
    """A latitude / longitude sphere of radius 0.5 as tess x tess quads, as twk_mesh_sphere emits them: all pairs, the pole quads with two
    coinciding vertices."""
    u, v = np.meshgrid(np.arange(tess + 1) * (2.0 * np.pi / tess), np.arange(tess + 1) * (np.pi / tess))
    p = 0.5 * np.stack([np.sin(v) * np.cos(u), np.cos(v), np.sin(v) * np.sin(u)], -1).reshape(-1, 3)
    j, i = np.meshgrid(np.arange(tess), np.arange(tess))
    a = (i * (tess + 1) + j).reshape(-1)
    b, c, d = a + 1, a + tess + 2, a + tess + 1
    return attributes(p, rng), np.stack([a, b, c, c, d, a], 1).reshape(-1).astype(np.uint32)


def distribution(name, n, rng):
    tiny = np.array([[0.0, 0.0, 0.0], [2.0 ** -6, 0.0, 0.0], [0.0, 2.0 ** -6, 2.0 ** -6]]) - np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -7])  # its box is centred exactly
    if name == "uniform":
        return soup(rng.uniform(-0.5, 0.5, (n, 3)), rng)
    if name == "sphere":
        return quad_sphere({257: 16, 1025: 32}[n], rng)
    if name == "clusters":  # two unit clusters 1e4 apart: the Morton grid puts each cluster into very few cells
        return soup(rng.uniform(-0.5, 0.5, (n, 3)) + np.where(np.arange(n)[:, None] % 2 == 0, -5.0e3, 5.0e3) * np.array([1.0, 0.0, 0.0]), rng)
    if name == "identical":
        return soup(np.zeros((n, 3)), rng, shape=rng.normal(0.0, 0.2, (3, 3)))
    if name == "line":  # centroids on a line parallel to x, no centroid extent on y and z: multiples of 2^-10 are exact
        return soup(np.stack([rng.integers(-512, 512, n) / 1024.0, np.zeros(n), np.zeros(n)], 1), rng, shape=tiny)
    if name == "plane":
        return soup(np.stack([rng.integers(-512, 512, n) / 1024.0, rng.integers(-512, 512, n) / 1024.0, np.zeros(n)], 1), rng, shape=tiny)
    if name == "sixteenths":  # centroids exactly on the sixteenths of their range [-1/2, 1/2], the ends included
        cells = rng.integers(0, 17, (n, 3))
        cells[0], cells[1] = 0, 16
        return soup(cells / 16.0 - 0.5, rng, shape=tiny)
    if name == "far":
        return soup(rng.uniform(-0.5, 0.5, (n, 3)) + np.array([1.0e6, -1.0e6, 1.0e6]), rng)
    if name == "spanning":  # one triangle that spans the whole cloud among tiny ones
        a, i = soup(rng.uniform(-0.5, 0.5, (n, 3)), rng, size=0.005)
        a[3 * (n // 2):3 * (n // 2) + 3, 0:3] = [[-0.5, -0.5, -0.5], [0.5, 0.5, -0.5], [0.0, 0.5, 0.5]]
        return a, i
    if name == "zero-area":  # every fourth triangle has no area: three collinear points, or a repeated vertex
        a, i = soup(rng.uniform(-0.5, 0.5, (n, 3)), rng)
        v = a[:, 0:3].reshape(n, 3, 3)
        v[0::8, 2] = 0.5 * (v[0::8, 0] + v[0::8, 1])
        v[4::8, 1] = v[4::8, 0]
        return a, i
    raise KeyError(name)


def forced_middle():
    """57 thin triangles in planes x = 17^k, k = -28 .. 28, with the same y and z (extent 2^-20 each): every centroid extent is zero
    but x's, and with ratio 17 the largest centroid falls alone into bin 15 and all others into bin 0, so each SAH level can only peel
    one primitive off — until the level loop halves the ranges by position from level 40 on (bvh_sah.hip buildSahTopology)."""
    x = np.array([17.0 ** k for k in range(-28, 29)]).astype(F32).astype(np.float64)
    e = 2.0 ** -20
    v = np.stack([np.stack([x, np.zeros(57), np.zeros(57)], 1), np.stack([x, np.full(57, e), np.zeros(57)], 1), np.stack([x, np.zeros(57), np.full(57, e)], 1)], 1)
    return attributes(v.reshape(-1, 3), np.random.default_rng(57)), np.arange(171, dtype=np.uint32)


def boxes_of(mesh):
    """The build-primitive boxes [n, 2, 3] (float32) of a mesh in object space, and the triangles of each primitive."""
    from bvh_reference import build_primitives
    a, i = mesh
    pos = np.asarray(a, F32)[np.asarray(i).reshape(-1, 3), 0:3]
    first, pair = build_primitives(i)
    lo, hi = pos.min(1), pos.max(1)
    nxt = np.minimum(first + 1, lo.shape[0] - 1)
    return np.stack([np.where(pair[:, None], np.minimum(lo[first], lo[nxt]), lo[first]), np.where(pair[:, None], np.maximum(hi[first], hi[nxt]), hi[first])], 1), np.where(pair, 2, 1)


def cases():
    """{name: [mesh names]} and the meshes {name: mesh}: what one scene holds."""
    rng = np.random.default_rng(2027)
    meshes, out = {}, {}
    for kind in ("soup", "quads"):
        for n in SIZES:
            meshes[f"{kind}-{n}"] = sized(n, kind, rng)
        out[f"sizes-{kind}"] = [f"{kind}-{n}" for n in SIZES]
    for n in ODD:
        meshes[f"odd-{n}"] = sized(n, "odd", rng)
    out["sizes-quads"] += [f"odd-{n}" for n in ODD]
    for n in DISTRIBUTION_SIZES:
        for name in WELL_BEHAVED + DEGENERATE:
            meshes[f"{name}-{n}"] = distribution(name, n, rng)
        out[f"distributions-{n}"] = [f"{name}-{n}" for name in WELL_BEHAVED + DEGENERATE]
    return out, meshes


def place(k):
    """The transform of the k-th mesh of a scene: 3 apart on a grid of 8 columns."""
    return S.rotated((3.0 * (k % 8), 3.0 * (k // 8), 0.0))


def stack_height():
    """The deepest tree twk_build accepts (csrc/device_scene.hip checkDepth): TWK_TRACE_STACK_LDS + TWK_TRACE_STACK_SPILL - 2, read from
    csrc/device_types.h."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tweeker_raytracer_amd", "csrc", "device_types.h")).read()
    return sum(int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) for name in ("TWK_TRACE_STACK_LDS", "TWK_TRACE_STACK_SPILL")) - 2


@functools.lru_cache(maxsize=None)
def reference_costs():
    """Per well-behaved mesh: inner + leaf cost (one node visit = one triangle test) of the float64 binned SAH, the float32 binned SAH
    and the float64 median split over the mesh's build primitives in object space."""
    import bvh_reference as R
    _, meshes = cases()
    out = {}
    for n in DISTRIBUTION_SIZES:
        for name in WELL_BEHAVED:
            boxes, triangles = boxes_of(meshes[f"{name}-{n}"])
            trees = (R.binned_sah(boxes, np.float64), R.binned_sah(boxes, F32), R.median_split(boxes))
            out[f"{name}-{n}"] = tuple(sum(R.sah_terms(tree, boxes, triangles)) for tree in trees)
    return out


def quality_margin():
    """How far the device's binned SAH may cost more than the float64 reference's: three times the largest |ratio - 1| between the
    float32 and the float64 run of the reference on the same meshes, and not less than 1 % (profiles/r27_bvh_audit.md)."""
    return max(0.01, 3.0 * max(abs(c32 / c64 - 1.0) for c64, c32, _ in reference_costs().values()))
