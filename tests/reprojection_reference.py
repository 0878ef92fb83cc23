"""A float64 world for the reprojection chain: where was this pixel's surface point in the previous frame, and which history pixels
does the temporal merge read for it? Everything here is written from the geometry — a pinhole camera given by its float32 words
(P, U, V, W) widened to double, parallelograms and triangle meshes under 3 x 4 transforms — with numpy.linalg.solve and
numpy.linalg.inv. It imports no restatement module and shares no formula with csrc/: no cross products in the projection, no
adjugate in the instance motion. A helper module, not a conftest; tests/test_reprojection_host.py (CPU) and
tests/test_gpu_reprojection.py use it.

The lookup is observed through a coded history: bilinear interpolation reproduces an affine function, so a history whose colour is its
own pixel coordinate hands back the position the merge looked up (coded_history / decode)."""
import collections

import numpy as np

F = np.float32
U32 = np.uint32
D = np.float64

U = 2.0 ** -24                      # the unit roundoff of float32
WIDTH, HEIGHT, FOV = 61, 37, 50.0
FAR = np.array([1000.0, -333.0, 2000.0])
WALL, CARD, PATCH = 0, 1, 2
MAX_HISTORY, TOLERANCE = 1.0e6, 0.2  # no cap; a tolerance of 0.2 x the distance (about 0.8) accepts every tap of the same surface
EDGE = 0.02                         # the exclusion's distance to an edge, in the surface's own parameters
NEAR_INTEGER = 1.0e-3               # the exclusion's distance of fx, fy to an integer


# ---- the camera ----------------------------------------------------------------------------------------------------------------------
class Camera:
    """A pinhole camera from 12 float32 words (P, U, V, W): the pixel (i, j) of a width x height picture looks along
    U ndcX + V ndcY + W with ndc = (i + 0.5) / N * 2 - 1. centre and swap are the negative controls: pixel centres taken at
    i + centre, and U and V exchanged."""

    def __init__(self, words, centre=0.5, swap=False):
        w = np.asarray(np.asarray(words, F).reshape(12), D)
        self.words = np.asarray(words, F).reshape(12).copy()
        self.P, self.U, self.V, self.W = w[0:3], w[3:6], w[6:9], w[9:12]
        if swap:
            self.U, self.V = self.V, self.U
        self.centre = float(centre)

    def rays(self, width, height):
        """(origin [3], directions [H, W, 3]) of the pixel centres; the directions are not normalised."""
        ndcx = (np.arange(width, dtype=D) + self.centre) / width * 2.0 - 1.0
        ndcy = (np.arange(height, dtype=D) + self.centre) / height * 2.0 - 1.0
        d = self.U[None, None, :] * ndcx[None, :, None] + self.V[None, None, :] * ndcy[:, None, None] + self.W[None, None, :]
        return self.P.copy(), d

    def project(self, g, width, height):
        """(fx, fy, s2) of world points g [..., 3]: [U V W] s = g - P, fx = (s0 / s2 + 1) / 2 * width - centre. s2 > 0: in front."""
        g = np.asarray(g, D)
        basis = np.stack([self.U, self.V, self.W], axis=1)
        s = np.linalg.solve(basis, (g - self.P).reshape(-1, 3).T).T.reshape(g.shape)
        with np.errstate(all="ignore"):
            fx = (s[..., 0] / s[..., 2] + 1.0) / 2.0 * width - self.centre
            fy = (s[..., 1] / s[..., 2] + 1.0) / 2.0 * height - self.centre
        return fx, fy, s[..., 2]

    def pixel_width(self, s2, width):
        """The world-space width of a pixel at the depth s2 (in units of W): the picture is 2 |U| s2 wide there."""
        return 2.0 * np.linalg.norm(self.U) * s2 / width


# ---- surfaces ------------------------------------------------------------------------------------------------------------------------
def to4(transform):
    """4 x 4 float64 of a row-major 3 x 4 matrix given as float32 words."""
    return np.vstack([np.asarray(np.asarray(transform, F).reshape(3, 4), D), [0.0, 0.0, 0.0, 1.0]])


def apply(matrix4, points):
    points = np.asarray(points, D)
    return points @ matrix4[:3, :3].T + matrix4[:3, 3]


class Surface:
    """A unit square (kind "square": the parallelogram origin (0, 0, 0), edges x and y) or a triangle mesh (kind "mesh": vertices
    float32 [n, 3], triangles [m, 3]) in object space, under a float32 3 x 4 transform. World space is the transform applied in double."""

    def __init__(self, kind, transform, vertices=None, triangles=None):
        self.kind = kind
        self.transform = np.asarray(transform, F).reshape(12).copy()
        self.vertices = None if vertices is None else np.asarray(vertices, F).reshape(-1, 3).copy()
        self.triangles = None if triangles is None else np.asarray(triangles, np.int64).reshape(-1, 3).copy()

    @property
    def matrix(self):
        return to4(self.transform)

    def world_vertices(self):
        return apply(self.matrix, self.vertices)


Hits = collections.namedtuple("Hits", "position instance t edge cos triangle barycentrics")


def _solve_columns(a, b, c, rhs):
    """x of [a b c] x = rhs for stacks [..., 3] of columns, by numpy.linalg.solve; singular systems give NaN."""
    a, b, c = np.broadcast_arrays(a, b, c)
    m = np.stack([a, b, c], axis=-1)
    shape = np.broadcast_shapes(m.shape[:-2], rhs.shape[:-1])
    m = np.broadcast_to(m, shape + (3, 3)).reshape(-1, 3, 3)
    r = np.broadcast_to(rhs, shape + (3,)).reshape(-1, 3, 1)
    good = np.abs(np.linalg.det(m)) > 1e-300
    x = np.full((m.shape[0], 3), np.nan)
    x[good] = np.linalg.solve(m[good], r[good])[..., 0]
    return x.reshape(shape + (3,))


def trace(surfaces, origin, directions):
    """The nearest hit of every ray among the surfaces: Hits of world position [.., 3], instance (-1: a miss), t in units of the
    direction as given, edge (the hit's distance to the nearest edge in the surface's own parameters: min(a, 1 - a, b, 1 - b) of a
    square, the smallest barycentric of a triangle), |cos| between ray and normal, and for a mesh the triangle and its barycentrics
    (b0, b1, b2) by a double-precision Moeller-Trumbore."""
    origin, d = np.asarray(origin, D), np.asarray(directions, D)
    shape = d.shape[:-1]
    best_t = np.full(shape, np.inf)
    instance, triangle = np.full(shape, -1, np.int64), np.full(shape, -1, np.int64)
    edge, cos = np.zeros(shape), np.zeros(shape)
    bary = np.zeros(shape + (3,))
    length = np.linalg.norm(d, axis=-1)

    def consider(i, o, e1, e2, is_triangle, index):
        nonlocal best_t
        x = _solve_columns(e1, e2, -d, origin - o)  # o + a e1 + b e2 = origin + t d
        a, b, t = x[..., 0], x[..., 1], x[..., 2]
        with np.errstate(invalid="ignore"):
            inside = (a >= 0) & (b >= 0) & ((a + b <= 1) if is_triangle else ((a <= 1) & (b <= 1))) & (t > 0) & (t < best_t)
        n = np.cross(e1, e2)
        c = np.abs(d @ n) / (np.linalg.norm(n) * length)
        e = np.minimum(np.minimum(a, b), 1 - a - b) if is_triangle else np.minimum(np.minimum(a, 1 - a), np.minimum(b, 1 - b))
        best_t = np.where(inside, t, best_t)
        instance[inside], triangle[inside] = i, index
        edge[inside], cos[inside] = e[inside], c[inside]
        bary[inside] = np.stack([1 - a - b, a, b], axis=-1)[inside]

    for i, s in enumerate(surfaces):
        m = s.matrix
        if s.kind == "square":
            consider(i, apply(m, (0, 0, 0)), m[:3, 0].copy(), m[:3, 1].copy(), False, -1)
        else:
            w = s.world_vertices()
            for k, (i0, i1, i2) in enumerate(s.triangles):
                consider(i, w[i0], w[i1] - w[i0], w[i2] - w[i0], True, k)
    hit = instance >= 0
    position = np.where(hit[..., None], origin + np.where(hit, best_t, 0.0)[..., None] * d, 0.0)
    return Hits(position, instance, np.where(hit, best_t, 0.0), edge, cos, triangle, bary)


def aov(hits):
    """The geometry AOV of the hits as the device writes it: float32 (world position, bits of instance + 1), zero words for a miss."""
    g = np.zeros(hits.instance.shape + (4,), F)
    g[..., :3] = hits.position.astype(F)
    g[..., 3] = (hits.instance + 1).astype(U32).view(F)
    g[hits.instance < 0] = 0
    return g


# ---- motion --------------------------------------------------------------------------------------------------------------------------
def instance_motion(previous, current):
    """X = M_prev inv(M_cur) on 4 x 4 doubles: carries a world point of the instance now to where it was."""
    return to4(previous) @ np.linalg.inv(to4(current))


def previous_positions(hits, current, previous, invert=False, rotate=0):
    """g' [..., 3] for the hits of a trace of `current` (surfaces), with `previous` the same instances as of the history's frame: a
    mesh whose vertices changed gives M_prev sum b_i v_i_prev with the barycentrics of the hit on the current vertices; an instance whose
    transform changed gives X g; every other pixel g. invert and rotate are the negative controls: X inverted, and the barycentrics
    rotated by `rotate` vertices."""
    out = hits.position.copy()
    for i, (now, then) in enumerate(zip(current, previous)):
        on = hits.instance == i
        if not on.any():
            continue
        if now.kind == "mesh" and not np.array_equal(now.vertices, then.vertices):
            v = np.asarray(then.vertices, D)[now.triangles[hits.triangle[on]]]          # [n, 3 vertices, 3]
            b = np.roll(hits.barycentrics[on], rotate, axis=-1)
            out[on] = apply(then.matrix, (b[..., None] * v).sum(axis=-2))
        elif not np.array_equal(now.transform.view(U32), then.transform.view(U32)):
            x = instance_motion(then.transform, now.transform)
            out[on] = apply(np.linalg.inv(x) if invert else x, hits.position[on])
    return out


# ---- what the merge is expected to do ---------------------------------------------------------------------------------------------
Lookup = collections.namedtuple("Lookup", "fx fy s2 took full taps")


def expected_lookup(previous_position, instance, camera, history_instance):
    """For current pixels with previous positions g' [H, W, 3] and instance ids [H, W] (-1: a miss): (fx, fy) through the history
    camera; the four taps floor(fx) + {0, 1}, floor(fy) + {0, 1}; a tap counts when it lies inside the picture and the history's
    instance id there equals the pixel's. took = any tap counts, full = all four; taps = [(qy, qx, counts)] in the order dy outer."""
    height, width = instance.shape
    fx, fy, s2 = camera.project(previous_position, width, height)
    hit = (instance >= 0) & (s2 > 0) & np.isfinite(fx) & np.isfinite(fy)
    x0 = np.where(hit, np.floor(np.where(hit, fx, 0.0)), 0).astype(np.int64)
    y0 = np.where(hit, np.floor(np.where(hit, fy, 0.0)), 0).astype(np.int64)
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = x0 + dx, y0 + dy
            inpic = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
            qyc, qxc = np.clip(qy, 0, height - 1), np.clip(qx, 0, width - 1)
            taps.append((qyc, qxc, hit & inpic & (history_instance[qyc, qxc] == instance)))
    counted = np.stack([t[2] for t in taps])
    return Lookup(fx, fy, s2, counted.any(axis=0), counted.all(axis=0), taps)


def exclusion(hits, history_hits, lookup):
    """The GPU tests' exclusion: the current hit within EDGE of an edge, one of the four history taps within EDGE of one, or fx / fy
    within NEAR_INTEGER of an integer. A condition, not a tolerance."""
    out = hits.edge < EDGE
    for qy, qx, _ in lookup.taps:
        out |= (history_hits.edge[qy, qx] < EDGE) & (history_hits.instance[qy, qx] >= 0)
    with np.errstate(invalid="ignore"):
        for f in (lookup.fx, lookup.fy):
            out |= np.abs(f - np.round(f)) < NEAR_INTEGER
    return out & (hits.instance >= 0)


# ---- the coded history ---------------------------------------------------------------------------------------------------------------
def coded_history(width, height):
    """(history colour, history moments, frame colour, frame moments), float32 [H, W, 4]: the history's colour is (qx, qy, 1, 1) with
    n = 3 samples, the frame is black with n = 1. The merged history is then (fx, fy, 1) x 3/4."""
    hc, hm = np.zeros((height, width, 4), F), np.zeros((height, width, 4), F)
    hc[..., 0], hc[..., 1] = np.arange(width, dtype=F)[None, :], np.arange(height, dtype=F)[:, None]
    hc[..., 2:] = 1.0
    hm[..., 2] = 3.0
    cur, mc = np.zeros((height, width, 4), F), np.zeros((height, width, 4), F)
    cur[..., 3] = 1.0
    mc[..., 2] = 1.0
    return hc, hm, cur, mc


def coded_layers(width, height, layers):
    """(history layers, frame layers), float32 [K, H, W, 4], for the cascade's merges: layer 0 of the history holds the code with a
    count of 3, every other sum is zero; the frame's layers are zero with a count of 1."""
    hl, cl = np.zeros((layers, height, width, 4), F), np.zeros((layers, height, width, 4), F)
    hl[0, ..., 0], hl[0, ..., 1] = np.arange(width, dtype=F)[None, :], np.arange(height, dtype=F)[:, None]
    hl[0, ..., 2], hl[0, ..., 3] = 1.0, 3.0
    cl[0, ..., 3] = 1.0
    return hl, cl


def decode(rgb):
    """(x, y, z) of a merged colour [..., >= 3]: the looked-up position (x, y) = rgb.xy / rgb.z — the normalisation cancels — and the
    constant channel z = rgb.z, which is 3/4 after a plain merge and 1 in the cascade's layer 0."""
    rgb = np.asarray(rgb, D)
    with np.errstate(all="ignore"):
        return rgb[..., 0] / rgb[..., 2], rgb[..., 1] / rgb[..., 2], rgb[..., 2]


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def bound_B(previous_position, camera, lookup, width, height):
    """B, the lookup position bound in pixels: 8 u (|g'|inf + |P'|inf) / s + 8 u max(W, H), s the world-space width of a history
    pixel at the depth of g'."""
    s = camera.pixel_width(np.where(lookup.s2 > 0, lookup.s2, np.nan), width)
    return 8.0 * U * (np.abs(previous_position).max(axis=-1) + np.abs(camera.P).max()) / s + 8.0 * U * max(width, height)


def bound_G(K, origin, position, cos, extra=0.0):
    """G, the world-position bound: K u (|P|inf + |g|inf + extra) / |cos|. extra: the same term for the previous vertices and matrix."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return K * U * (np.abs(origin).max() + np.abs(position).max(axis=-1) + extra) / cos


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
def _rotation(axis, degrees):
    a = np.asarray(axis, D) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    return np.eye(3) + np.sin(r) * k + (1 - np.cos(r)) * (k @ k)


def _transform(linear, translation, far):
    t = np.asarray(translation, D) + (FAR if far else 0.0)
    return np.concatenate([np.asarray(linear, D), t.reshape(3, 1)], axis=1).astype(F).reshape(12)


PATCH_TRIANGLES = np.array([[3 * j + i, 3 * j + i + 1, 3 * (j + 1) + i + 1, 3 * j + i, 3 * (j + 1) + i + 1, 3 * (j + 1) + i]
                            for j in range(2) for i in range(2)], np.int64).reshape(-1, 3)  # two per cell, sharing the diagonal


def patch_vertices(deformed=False):
    """The patch's 3 x 3 vertices on z = 0 of [0, 1]^2 in object space; deformed: each displaced by a seeded offset of up to 0.1."""
    v = np.array([[i / 2.0, j / 2.0, 0.0] for j in range(3) for i in range(3)], D)
    if deformed:
        v = v + np.random.default_rng(30).uniform(-0.1, 0.1, v.shape)
    return v.astype(F)


def scene(far=False, card_moved=False, patch_deformed=False):
    """[wall, card, patch]. The wall: origin (-4, -3, 0), edges (8, 0, 0) and (0, 6, 0). The card: origin (-0.6, -0.5, 1.0), edges
    (1.1, 0.1, 0.2) and (-0.1, 0.9, 0.1), a unit square under a sheared transform; moved: turned 20 degrees about (1, 2, 0.5) through
    its origin, its first edge scaled by 1.15, shifted by (0.15, -0.1, 0.2). The patch: 3 x 3 vertices, 8 triangles, under a rotated,
    non-uniformly scaled transform, to the right of the card. far: everything translated by FAR."""
    wall = Surface("square", _transform(np.diag([8.0, 6.0, 1.0]), (-4.0, -3.0, 0.0), far))
    linear = np.array([[1.1, -0.1, 0.1], [0.1, 0.9, -0.2], [0.2, 0.1, 1.0]])
    origin = np.array([-0.6, -0.5, 1.0])
    if card_moved:
        linear = _rotation((1.0, 2.0, 0.5), 20.0) @ (linear @ np.diag([1.15, 1.0, 1.0]))
        origin = origin + (0.15, -0.1, 0.2)
    card = Surface("square", _transform(linear, origin, far))
    turn = _rotation((0.0, 0.0, 1.0), 25.0) @ _rotation((1.0, 0.0, 0.0), 20.0) @ np.diag([1.0, 1.2, 1.3])
    patch = Surface("mesh", _transform(turn, (1.4, -0.75, 0.8), far), patch_vertices(patch_deformed), PATCH_TRIANGLES)
    return [wall, card, patch]
