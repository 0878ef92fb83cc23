"""The exact reference of the triangle test: ray-triangle geometry in rational arithmetic, the case classes, the bounds.

No GPU and no product code. tests/test_triangle_exact_host.py (host build of trace_device.h, the oracle's brute force) and
tests/test_gpu_triangle_exact.py (the HIP kernels) hold their hit records against what this module computes.

REFERENCE. Every float32 is a rational number, so the geometry a kernel's input words describe can be computed without error. With
A = p0 - o, B = p1 - o, C = p2 - o the edge functions are the scalar triple products

    U = d . (C x B)    V = d . (A x C)    W = d . (B x A)        det = U + V + W

and the ray o + t d meets the plane of the triangle at t = A . (C x B) / det, at the point (U p0 + V p1 + W p2) / det: beta = V / det
and gamma = W / det are the weights of p1 and p2, alpha = U / det that of p0. All of it is evaluated in Python integers (the inputs
scaled by a power of two) and `fractions.Fraction`: no float, no shear, no permutation of axes, no line of woopIntersect.

CONDITIONING. kappa = L^2 max|d_i| / |det| with L the largest |component| of p_k - o over the three vertices and det exact.

BOUND. |t_dev - t| / t, |beta_dev - beta| and |gamma_dev - gamma| are at most K u kappa, u = 2^-24. The roundings of woopIntersect
as it is written (trace_device.h), to first order in u, every one taken at its worst and all of them adding up:
  * p - o: one rounding of a number of at most L: u L per permuted coordinate (Akx, Aky, Akz).
  * the shear Ax = Akx - Sx Akz, |Sx| <= 1 (d[kz] is the largest component), |Ax| <= 2 L: u L from Akx; 3 u L in the product (the
    correctly rounded quotient Sx, the rounded Akz, the product's own rounding); 2 u L for the difference: 6 u L per sheared
    coordinate.
  * an edge function U' = Cx By - Cy Bx (U' = U / d[kz]: the shear has determinant one and maps d onto the z axis): each product is
    at most 4 L^2, carries 2 * (2 L)(6 u L) = 24 u L^2 from its operands and 4 u L^2 of its own; the difference of at most 8 L^2
    adds 8 u L^2: 64 u L^2 per edge function. (The double-precision branch only lowers the last two terms.)
  * det' = (U' + V') + W': 3 * 64 u L^2 from the operands, 16 u L^2 and 24 u L^2 for the two sums: 232 u L^2, that is
    232 u kappa relative to det' = det / d[kz].
  * beta = V' * (1 / det'): the reciprocal is correctly rounded and the product rounds once, 2 u |beta|; together
    |beta_dev - beta| <= (64 + 232 |beta|) u kappa + 2 u |beta|. On a hit |beta| <= 1, and kappa >= 1 / 24 because |det'| <= 24 L^2,
    so 2 u <= 48 u kappa: 344 u kappa. gamma alike.
  * t = (U' Az + V' Bz + W' Cz) / det' with Az = Sz Akz (three roundings, |Az| <= L / |d[kz]|): the numerator collects
    3 * 64 u L^3 / |d[kz]| from the edge functions and, on a hit where |U'|, |V'|, |W'| <= |det'|, 3 * 4 u L |det'| / |d[kz]| from
    the products and two sums of at most 3 L |det'| / |d[kz]|, 6 u of them. Relative to t det' this is rho (192 kappa + 18) u with
    rho = L / (t max|d_i|), the distance of the farthest vertex over that of the hit, both along the dominant axis; with det's 232
    and the two final roundings: |t_dev - t| / t <= (192 rho + 232) u kappa + (18 rho + 2) u. rho is at least one; the classes below
    (origins about as far from a triangle as it is wide) reach rho = 2. The sum of worst cases for t therefore goes past 512 u kappa
    once rho exceeds about 1.2, and for t the bound stands as the issue states it, not as a theorem; `rho` is printed with the ratios
    for that reason, and the measured errors of t stay below 6 u kappa.
K is the next power of two above the 344 of beta and gamma: K = 512. It is NOT tightened to what any implementation achieves (the
largest measured ratios are a few times u kappa, recorded in profiles/r35_triangle_exact.md).

VERDICT. A triangle whose exact alpha, beta, gamma all exceed K u kappa, with t (1 - K u kappa) > tmin and t (1 + K u kappa) < tmax,
MUST be reported; one with a coordinate below -K u kappa, or t on the wrong side of tmin or tmax by that factor, MUST NOT be; a
triangle of zero area (two equal vertices: U' is exactly zero and W' = -V' exactly, so det' = 0) must never be. Anything in
between asserts nothing on its own. With K u kappa >= 1 nothing is decided.

WATERTIGHTNESS. An aimed case is KEPT when (1) the exact ray meets the closed union of its fan or pair at t > 0 in a triangle whose
unshared edges are all further than |det| / 100 away (their edge functions exceed |det| / 100), and (2) every triangle of the group
that has any area has the same exact sign of det: a spoke seen edge-on is a silhouette, and a ray through it may rightly miss. On a
kept case some triangle must be reported and its t is the exact entry t within the bound.

YARDSTICK. `moller_trumbore` is the textbook float32 test in numpy, measured against the same exact values.

CASES. `case_set(name)` returns one of the seeded classes (MAKERS) with its exact reference, each class one scene of 100 fans (or pairs) on a 5 x 5 x 5 grid with 20 rays per group:
twelve aimed at the centre and at 1/4, 1/2, 3/4 of a spoke (of the shared edge, for a pair) from origins on either side, five aimed
well inside a triangle, three beside the group. The fan's normal is near the x, y, z axis in turn, so every axis is the dominant one, and
the rays from the far side have d[kz] < 0; every other group is wound the other way round about its normal, so the sheared
triangles of the test come in both orientations (the origin's side alone does not change it: det and d[kz] change sign together). Outside the random classes each triangle's vertex order is rotated by its index, so every
edge function meets a shared edge; the random classes keep the plain order (centre, r_i, r_i+1), on which the float32 yardstick
slips more often (every triangle then subtracts the same vertex from the origin and the errors of two neighbours have less in common).
"""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24
K = 512
EDGE_MARGIN = 0.01     # kept: unshared edge functions exceed |det| / 100
PREFILTER = 2.0 * K * U32  # a triangle with edge functions of both signs beyond this x L^2 max|d| cannot be reported: not evaluated exactly
TMAX = 1e27
STATUS_NO, STATUS_MAYBE, STATUS_SURE = 0, 1, 2
IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def attributes(vertices):
    """Vertex attributes [v, 12] as addGeometry takes them: the position, and a tangent and a normal nobody reads here."""
    a = np.zeros((len(vertices), 12), F32)
    a[:, 0:3] = vertices
    a[:, 3] = 1.0
    a[:, 8] = 1.0
    return a


# ---------------------------------------------------------------------------------------------------------------- exact geometry

def _scale(values):
    """s such that x 2^s is an integer for every float32 value x of `values`."""
    s = 0
    for x in values:
        if x != 0.0:
            s = max(s, 24 - math.frexp(x)[1])
    return s


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


ROW = np.dtype([("ray", np.int64), ("tri", np.int64), ("sign", np.int64), ("alpha", np.float64), ("beta", np.float64), ("gamma", np.float64),
                ("t", np.float64), ("kappa", np.float64), ("rho", np.float64), ("zero", np.bool_, 3), ("inside", np.bool_)])


def exact_ray(o, d, tris):
    """Exact records of the ray (o, d) against tris [m, 3, 3] (all float32 values): a list of tuples
    (sign of det, alpha, beta, gamma, t as Fractions or None, kappa, rho, (U == 0, V == 0, W == 0), inside the closed triangle at t > 0)."""
    o = [float(x) for x in o]
    d = [float(x) for x in d]
    flat = [float(x) for x in np.asarray(tris, F32).reshape(-1)]
    sp, sd = _scale(o + flat), _scale(d)
    oi = [int(math.ldexp(x, sp)) for x in o]
    di = [int(math.ldexp(x, sd)) for x in d]
    dmax = max(abs(x) for x in di)
    out = []
    for k in range(len(flat) // 9):
        P = [[int(math.ldexp(flat[9 * k + 3 * v + c], sp)) - oi[c] for c in range(3)] for v in range(3)]
        A, B, C = P
        CB = _cross(C, B)
        Ue, Ve, We = _dot(di, CB), _dot(di, _cross(A, C)), _dot(di, _cross(B, A))
        det = Ue + Ve + We
        L = max(abs(x) for row in P for x in row)
        zero = (Ue == 0, Ve == 0, We == 0)
        if det == 0:
            out.append((0, None, None, None, None, math.inf, math.inf, zero, False))
            continue
        s = 1 if det > 0 else -1
        a, b, g = Fraction(Ue, det), Fraction(Ve, det), Fraction(We, det)
        t = Fraction(_dot(A, CB) << sd, det << sp)
        kappa = float(Fraction(L * L * dmax, abs(det)))
        rho = float(Fraction(L << sd, dmax << sp) / t) if t > 0 else math.inf
        out.append((s, a, b, g, t, kappa, rho, zero, a >= 0 and b >= 0 and g >= 0 and t > 0))
    return out


class Reference:
    """The exact records of every (ray, candidate triangle) of a case set: `rows` (ROW, sorted by ray) and `span` [n, 2], the rows of
    each ray. The candidates of a ray are the triangles of its own group and every other triangle of the scene that a float64
    evaluation does not rule out by the stated margin PREFILTER."""
    def __init__(self, cs):
        tris64 = cs.tris.astype(np.float64)
        rows, span = [], np.zeros((cs.rays.shape[0], 2), np.int64)
        for r in range(cs.rays.shape[0]):
            o, d = cs.rays[r, 0:3], cs.rays[r, 4:7]
            P = tris64 - o.astype(np.float64)
            A, B, C = P[:, 0], P[:, 1], P[:, 2]
            d64 = d.astype(np.float64)
            E = np.stack([np.cross(C, B) @ d64, np.cross(A, C) @ d64, np.cross(B, A) @ d64], 1)
            m = PREFILTER * np.abs(P).max(axis=(1, 2)) ** 2 * np.abs(d64).max()
            ruled_out = (E.min(axis=1) < -m) & (E.max(axis=1) > m)
            own = np.zeros(len(tris64), bool)
            g = cs.ray_group[r]
            own[cs.group_first[g]:cs.group_first[g] + cs.group_count[g]] = True
            cand = np.nonzero(own | ~ruled_out)[0]
            span[r] = (len(rows), len(rows) + len(cand))
            for k, rec in zip(cand, exact_ray(o, d, cs.tris[cand])):
                s, a, b, g_, t, kappa, rho, zero, inside = rec
                rows.append((r, k, s, *(float(x) if x is not None else math.nan for x in (a, b, g_, t)), kappa, rho, zero, inside))
        self.rows = np.array(rows, ROW)
        self.span = span
        self.bound = K * U32 * self.rows["kappa"]
        self.own = cs.tri_group[self.rows["tri"]] == cs.ray_group[self.rows["ray"]]

    def status(self, cs):
        """STATUS_SURE / STATUS_MAYBE / STATUS_NO of every row under its ray's tmin and tmax (module docstring: VERDICT)."""
        r, b = self.rows, self.bound
        tmin, tmax = cs.rays[r["ray"], 3].astype(np.float64), cs.rays[r["ray"], 7].astype(np.float64)
        with np.errstate(invalid="ignore"):
            m = np.minimum(np.minimum(r["alpha"], r["beta"]), r["gamma"])
            decided = b < 1.0
            sure = decided & (m > b) & (r["t"] * (1 - b) > tmin) & (r["t"] * (1 + b) < tmax)
            no = decided & ((m < -b) | (r["t"] <= 0) | (r["t"] * (1 + b) <= tmin) | (r["t"] * (1 - b) >= tmax))
        no |= cs.zero_area[r["tri"]]
        return np.where(sure, STATUS_SURE, np.where(no, STATUS_NO, STATUS_MAYBE))

    def kept(self, cs):
        """(kept [n] bool, entry t [n]) of the watertightness rule (module docstring). Only aimed rays can be kept."""
        n = cs.rays.shape[0]
        kept, entry = np.zeros(n, bool), np.full(n, np.nan)
        for i in range(n):
            if not cs.aimed[i]:
                continue
            rows = self.rows[self.span[i, 0]:self.span[i, 1]]
            own = rows[cs.tri_group[rows["tri"]] == cs.ray_group[i]]
            area = own[~cs.zero_area[own["tri"]]]
            if not ((area["sign"] == area["sign"][0]).all() and area["sign"][0] != 0):
                continue
            inside = area[area["inside"]]
            if not len(inside):
                continue
            t0 = inside["t"].min()
            first = inside[inside["t"] == t0]
            coords = np.stack([first["alpha"], first["beta"], first["gamma"]], 1)
            if (coords[cs.unshared[first["tri"]]] > EDGE_MARGIN).all():
                kept[i] = True
                # the entry into the scene: another group in front of this one counts too
                entry[i] = rows[rows["inside"]]["t"].min()
        return kept, entry


# ---------------------------------------------------------------------------------------------------- checks of hit records

def errors(ref_rows, tbg):
    """(|t_dev - t| / t, |beta_dev - beta|, |gamma_dev - gamma|) [n, 3] of records tbg [n, 3] against exact rows."""
    tbg = np.asarray(tbg, np.float64)
    return np.stack([np.abs(tbg[:, 0] - ref_rows["t"]) / ref_rows["t"], np.abs(tbg[:, 1] - ref_rows["beta"]), np.abs(tbg[:, 2] - ref_rows["gamma"])], 1)


def check_per_triangle(cs, ref, hit, tbg, what):
    """A triangle test's own verdicts and values: hit [rows] bool and tbg [rows, 3] for ref.rows, each (ray, triangle) tested on its
    own under the ray's tmin and `t < tmax`. Returns (failures, the largest error / bound over the reported hits, per t / beta / gamma)."""
    status = ref.status(cs)
    hit = np.asarray(hit, bool)
    fails = []
    for i in np.nonzero((status == STATUS_SURE) & ~hit)[0][:5]:
        fails.append(f"{what}: ray {ref.rows['ray'][i]} triangle {ref.rows['tri'][i]} lies {ref.rows[i]} inside by more than the bound and is not reported")
    for i in np.nonzero((status == STATUS_NO) & hit)[0][:5]:
        fails.append(f"{what}: ray {ref.rows['ray'][i]} triangle {ref.rows['tri'][i]} is reported, exact {ref.rows[i]}")
    sel = hit & np.isfinite(ref.bound) & (ref.rows["sign"] != 0)
    ratio = errors(ref.rows[sel], tbg[sel]) / ref.bound[sel, None]
    for i in np.nonzero((ratio > 1.0).any(axis=1))[0][:5]:
        fails.append(f"{what}: ray {ref.rows[sel]['ray'][i]} triangle {ref.rows[sel]['tri'][i]}: errors / bound {ratio[i]} of {tbg[sel][i]} against {ref.rows[sel][i]}")
    return fails, (ratio.max(axis=0) if len(ratio) else np.zeros(3)), sel


def check_traversal(cs, ref, tri, tbg, any_hit, what, values=True):
    """A traversal's answers over the whole scene: tri [n] the reported triangle (index into cs.tris, -1 for none; for an occlusion
    flag alone pass -2 for `occluded`) and tbg [n, 3]. Closest hit: the reported triangle may be reported, its values are within its
    bound, and no triangle that must be reported lies in front of it beyond both bounds (on a tie in exact t either is right). Any
    hit: a triangle that must be reported means occluded, and an occluded ray has one that may be. Returns (failures, largest ratios)."""
    status = ref.status(cs)
    fails, worst = [], np.zeros(3)
    tbg = np.asarray(tbg, np.float64)
    for i in range(cs.rays.shape[0]):
        a, b = ref.span[i]
        rows, st, bd = ref.rows[a:b], status[a:b], ref.bound[a:b]
        sure = st == STATUS_SURE
        if tri[i] == -1:
            if sure.any():
                fails.append(f"{what}: ray {i} reports nothing, triangle {rows['tri'][sure][0]} must be: {rows[sure][0]}")
            continue
        if tri[i] == -2:
            if not (st != STATUS_NO).any():
                fails.append(f"{what}: ray {i} is occluded and no triangle may be reported")
            continue
        j = np.nonzero(rows["tri"] == tri[i])[0]
        if not len(j) or st[j[0]] == STATUS_NO:
            fails.append(f"{what}: ray {i} reports triangle {tri[i]}, which must not be" + (f": {rows[j[0]]}" if len(j) else " (ruled out by the float64 margin)"))
            continue
        j = j[0]
        if values and np.isfinite(bd[j]) and rows["sign"][j] != 0:
            ratio = errors(rows[j:j + 1], tbg[i:i + 1])[0] / bd[j]
            worst = np.maximum(worst, ratio)
            if (ratio > 1.0).any():
                fails.append(f"{what}: ray {i} triangle {tri[i]}: errors / bound {ratio} of {tbg[i]} against {rows[j]}")
            if not any_hit and sure.any():
                nearest = (rows["t"][sure] * (1 + bd[sure])).min()
                if tbg[i, 0] > nearest:
                    fails.append(f"{what}: ray {i} reports t {tbg[i, 0]} of triangle {tri[i]} behind a triangle that must be reported at t <= {nearest}")
    return fails, worst


def check_watertight(cs, ref, kept, entry, tri, t, what):
    """On every kept case something is reported, and its t is the exact entry t within the bound of the reported triangle."""
    fails, worst = [], 0.0
    for i in np.nonzero(kept)[0]:
        if tri[i] < 0:
            fails.append(f"{what}: kept ray {i} slips through its group (entry t {entry[i]})")
            continue
        a, b = ref.span[i]
        j = np.nonzero(ref.rows["tri"][a:b] == tri[i])[0]
        if not len(j):
            fails.append(f"{what}: kept ray {i} reports triangle {tri[i]}, ruled out by the float64 margin")
            continue
        ratio = abs(float(t[i]) - entry[i]) / entry[i] / ref.bound[a + j[0]]
        worst = max(worst, ratio)
        if ratio > 1.0:
            fails.append(f"{what}: kept ray {i}: t {t[i]} of triangle {tri[i]} against the entry t {entry[i]}: {ratio} bounds")
    return fails, worst


# ------------------------------------------------------------------------------------------------------ the float32 yardstick

def moller_trumbore(o, d, tris, tmin, tmax):
    """The textbook float32 Moeller-Trumbore test, row by row: o, d [n, 3], tris [n, 3, 3], tmin, tmax [n] -> (hit [n], t / beta / gamma [n, 3]).
    Every operation is a float32 numpy operation. A reference to measure against, not code under test."""
    o, d, tris = np.asarray(o, F32), np.asarray(d, F32), np.asarray(tris, F32)

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    def dot(a, b):
        return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
        p = cross(d, e2)
        det = dot(e1, p)
        inv = F32(1.0) / det
        s = o - tris[:, 0]
        u = dot(s, p) * inv
        q = cross(s, e1)
        v = dot(d, q) * inv
        t = dot(e2, q) * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= F32(1.0)) & (t > np.asarray(tmin, F32)) & (t < np.asarray(tmax, F32))
    assert t.dtype == F32 and u.dtype == F32
    return hit, np.stack([t, u, v], 1)


def quantiles(err):
    """(median, 99.9 % quantile) of each column of err [n, 3]."""
    return np.quantile(err, 0.5, axis=0), np.quantile(err, 0.999, axis=0)


# ---------------------------------------------------------------------------------------------------------------- the cases

class CaseSet:
    """One class = one scene. tris [T, 3, 3] float32 (world space), tri_group [T], unshared [T, 3] (which of U, V, W belong to an edge
    no neighbour shares), zero_area [T], group_first / group_count [G], vertices [V, 3] and indices [T, 3] of the one mesh,
    rays [n, 8] = o, tmin, d, tmax, ray_group [n], aimed [n] (the rays the watertightness rule speaks about)."""
    def __init__(self, name):
        self.name = name
        self.dyadic = False
        self._v, self._i, self._tg, self._un, self._za, self._rays, self._rg, self._aim = [], [], [], [], [], [], [], []
        self.group_first, self.group_count = [], []
        self._nv = 0

    def add_group(self, vertices, triangles, unshared, zero_area):
        g = len(self.group_first)
        self.group_first.append(len(self._i))
        self.group_count.append(len(triangles))
        for tri, un, za in zip(triangles, unshared, zero_area):
            self._i.append([self._nv + k for k in tri])
            self._un.append(un)
            self._za.append(za)
            self._tg.append(g)
        self._v.extend(np.asarray(vertices, np.float64))
        self._nv += len(vertices)
        return g

    def add_ray(self, g, o, d, aimed, tmin=0.0, tmax=TMAX):
        self._rays.append([o[0], o[1], o[2], tmin, d[0], d[1], d[2], tmax])
        self._rg.append(g)
        self._aim.append(aimed)

    def finish(self):
        self.vertices = np.asarray(self._v, np.float64).astype(F32)
        self.indices = np.asarray(self._i, np.int64)
        self.tris = self.vertices[self.indices]
        self.tri_group, self.unshared, self.zero_area = np.asarray(self._tg), np.asarray(self._un, bool), np.asarray(self._za, bool)
        self.group_first, self.group_count = np.asarray(self.group_first), np.asarray(self.group_count)
        self.rays = np.asarray(self._rays, np.float64).astype(F32)
        self.ray_group, self.aimed = np.asarray(self._rg), np.asarray(self._aim, bool)
        return self


GRID, SPACING, GROUPS = 5, 16.0, 100


def _unit(v):
    return v / np.linalg.norm(v)


def _frame(rng, axis, tilt=0.35):
    n = np.zeros(3)
    n[axis] = 1.0
    n = _unit(n + tilt * rng.uniform(-1, 1, 3))
    other = np.zeros(3)
    other[(axis + 1) % 3] = 1.0
    e1 = _unit(np.cross(n, other))
    return n, e1, np.cross(n, e1)


def _rotate(tri, un, k):
    k %= 3
    return tri[k:] + tri[:k], un[k:] + un[:k]


def _fan_group(cs, rng, centre, frame, m, aspect, noise, degenerate, quantum, rotate, mirror):
    """A closed fan of m triangles around `centre`; returns (group, centre, rim [m, 3]) with the coordinates as the mesh holds them."""
    n, e1, e2 = frame
    ang = (np.arange(m) + rng.uniform(-0.2, 0.2, m)) * (2 * np.pi / m) + rng.uniform(0, 2 * np.pi)
    if mirror:
        ang = ang[::-1]
    ln = rng.uniform(0.5, 2.0, m)
    rim = centre + ln[:, None] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2 / aspect) + (noise / aspect) * rng.uniform(-1, 1, m)[:, None] * n
    verts = np.concatenate([[centre], rim])
    if quantum:
        verts = np.round(verts / quantum) * quantum
    verts = verts.astype(F32).astype(np.float64)
    tris, uns, zas = [], [], []
    for i in range(m):
        tri, un = _rotate([0, 1 + i, 1 + (i + 1) % m], [True, False, False], i if rotate else 0)   # (centre, r_i, r_i+1): U belongs to the rim edge
        tris.append(tri), uns.append(un), zas.append(False)
    if degenerate:
        # one rim point twice, as two vertices of the mesh: (centre, r_j, r_j) has no area and lies along a spoke
        j = int(rng.integers(0, m))
        verts = np.concatenate([verts, verts[1 + j:2 + j]])
        tri, un = _rotate([0, 1 + j, len(verts) - 1], [False, False, False], j if rotate else 0)
        tris.insert(j, tri), uns.insert(j, un), zas.insert(j, True)
    g = cs.add_group(verts, tris, uns, zas)
    return g, verts[0], verts[1:1 + m]


def _pair_group(cs, rng, centre, frame, order, noise, quantum, mirror):
    n, e1, e2 = frame
    sx, sy = np.array([-1, 1, 1, -1.0]) * (-1.0 if mirror else 1.0), np.array([-1, -1, 1, 1.0])
    p = centre + (sx * rng.uniform(0.5, 2.0, 4))[:, None] * e1 + (sy * rng.uniform(0.5, 2.0, 4))[:, None] * e2 + noise * rng.uniform(-1, 1, 4)[:, None] * n
    if quantum:
        p = np.round(p / quantum) * quantum
    p = p.astype(F32).astype(np.float64)
    tris = ([0, 1, 2], [2, 3, 0]) if order == 0 else (([0, 1, 2], [0, 2, 3]) if order == 1 else ([1, 2, 0], [3, 0, 2]))
    # U belongs to the edge (second, third vertex), V to (third, first), W to (first, second); the shared edge is p0 p2
    uns = [[{t[1], t[2]} != {0, 2}, {t[2], t[0]} != {0, 2}, {t[0], t[1]} != {0, 2}] for t in tris]
    return cs.add_group(p, tris, uns, [False, False]), p


def _targets_fan(c, rim, j):
    m = len(rim)
    i = (j // 4) % m
    if j < 12:
        return c + (0.0, 0.25, 0.5, 0.75)[j % 4] * (rim[i] - c), True
    if j < 17:
        a, b = ((0.3, 0.3), (0.5, 0.2), (0.2, 0.6), (0.1, 0.1), (0.45, 0.45))[j - 12]
        return c + a * (rim[(i + j) % m] - c) + b * (rim[(i + j + 1) % m] - c), True
    return c + 1.5 * (rim[(i + j) % m] - c) + 0.5 * (rim[(i + j + 1) % m] - c), False


def _targets_pair(p, j):
    if j < 12:
        return p[0] + (0.25, 0.5, 0.75)[j % 3] * (p[2] - p[0]), True
    if j < 16:
        k = 1 if j % 2 else 3
        return 0.25 * p[0] + 0.5 * p[k] + 0.25 * p[2], True
    if j < 18:
        return p[0] + 0.5 * (p[2] - p[0]), True
    return p[1] + 0.75 * (p[1] - p[3]), False


def _make(name, seed, kind="fan", aspect_max=1.0, noise=0.3, degenerate=False, dyadic=False, graze=False, translate=0.0, scale_d=False, rotate=True):
    rng = np.random.default_rng(seed)
    cs = CaseSet(name)
    cs.dyadic = dyadic
    quantum = 0.5 if dyadic else 0.0   # halves: the quarter points of a spoke are multiples of 2^-3 as well
    for g in range(GROUPS):
        cell = np.array([g % GRID, (g // GRID) % GRID, g // (GRID * GRID)], np.float64)
        offset = (cell - (GRID - 1) / 2) * SPACING + translate
        axis = g % 3
        frame = _frame(rng, (axis + 1) % 3 if graze else axis)
        n, e1, e2 = frame
        centre = offset + rng.uniform(-2, 2, 3)
        aspect = 10.0 ** rng.uniform(1.0, math.log10(aspect_max)) if aspect_max > 1.0 else 1.0
        if kind == "fan":
            grp, c, rim = _fan_group(cs, rng, centre, frame, 3 + g % 5, aspect, noise, degenerate, quantum, rotate, (g // 3) % 2 == 1)
        else:
            grp, p = _pair_group(cs, rng, centre, frame, g % 3, noise, quantum, (g // 3) % 2 == 1)
        for j in range(20):
            target, aimed = _targets_fan(c, rim, j) if kind == "fan" else _targets_pair(p, j)
            side = 1.0 if (j // 4 + j % 2 + g) % 2 == 0 else -1.0
            if dyadic:
                w = np.zeros(3)
                w[axis] = float(rng.choice([2.0, 4.0]))
                w[(axis + 1) % 3], w[(axis + 2) % 3] = rng.integers(-4, 5, 2) / 8.0
                w *= side
                d = w * float(rng.choice([0.5, 1.0, 2.0, 4.0]))
            else:
                if graze:
                    theta = np.radians(rng.uniform(0.3, 0.9))
                    along = _unit(e2 + 0.3 * rng.uniform(-1, 1) * e1)   # e2 is near the axis after the frame's normal
                    w = side * rng.uniform(2.0, 4.0) * (np.sin(theta) * n + np.cos(theta) * along)
                else:
                    w = side * (rng.uniform(2.0, 4.0) * n + 0.3 * (rng.uniform(-1, 1) * e1 + rng.uniform(-1, 1) * e2 / aspect))
                d = w * (rng.uniform(0.1, 10.0) if scale_d else 1.0)
            o = (target - w).astype(F32).astype(np.float64)
            if not dyadic:
                # aimed from the origin as it was rounded, and as well as float32 allows: of sixteen lengths of the direction the one
                # whose rounded components pass closest to the target (a ray that misses the edge by more than a float32 test's own
                # error tells nothing about that test)
                v = target - o
                cands = [(v * (np.linalg.norm(d) / np.linalg.norm(w)) * (1 + k / 64)).astype(F32).astype(np.float64) for k in range(16)]
                d = min(cands, key=lambda c: np.linalg.norm(np.cross(v, c)) / np.linalg.norm(c))
            cs.add_ray(grp, o, d, aimed)
    return cs.finish()


def _extent(seed):
    """Rays of a random scene aimed well inside a triangle, four of each: closest-hit rays with tmin = t (1 -+ delta), any-hit rays
    with tmax = t (1 -+ delta), t the exact distance of the triangle aimed at and delta twice its bound."""
    base = _make("extent", seed, scale_d=True, rotate=False)
    cs = CaseSet("extent")
    cs.vertices, cs.indices, cs.tris = base.vertices, base.indices, base.tris
    cs.tri_group, cs.unshared, cs.zero_area, cs.group_first, cs.group_count = base.tri_group, base.unshared, base.zero_area, base.group_first, base.group_count
    rays, groups = [], []
    for g in range(GROUPS):
        first, m = base.group_first[g], base.group_count[g]
        src = base.rays[base.ray_group == g]
        for j in range(5):
            tri = base.tris[first + j % m].astype(np.float64)
            o = src[j * 3, 0:3].astype(np.float64)
            target = tri.mean(axis=0)
            d = ((target - o) * (0.3 + 0.4 * j)).astype(F32)
            rec = exact_ray(o, d, base.tris[first + j % m:first + j % m + 1])[0]
            if rec[0] == 0 or not rec[8]:
                continue
            delta = 2.0 * K * U32 * rec[5]
            t = float(rec[4])
            for tmin, tmax in ((t * (1 - delta), TMAX), (t * (1 + delta), TMAX), (0.0, t * (1 - delta)), (0.0, t * (1 + delta))):
                rays.append([*o, tmin, *d, tmax])
                groups.append(g)
    cs.rays = np.asarray(rays, np.float64).astype(F32)
    cs.ray_group, cs.aimed = np.asarray(groups), np.zeros(len(rays), bool)
    return cs


WATERTIGHT_CLASSES = ("fan", "pair", "needle", "degenerate", "grazing", "dyadic", "dyadic pair", "random", "random+1e3", "random+1e5")
RANDOM_CLASSES = ("random", "random+1e3", "random+1e5")
MAKERS = {
    "fan": lambda: _make("fan", 101),
    "pair": lambda: _make("pair", 102, kind="pair"),
    "needle": lambda: _make("needle", 103, aspect_max=1e4),
    "degenerate": lambda: _make("degenerate", 104, degenerate=True),
    "grazing": lambda: _make("grazing", 105, noise=0.001, graze=True),
    "dyadic": lambda: _make("dyadic", 106, dyadic=True),
    "dyadic pair": lambda: _make("dyadic pair", 107, kind="pair", dyadic=True),
    "random": lambda: _make("random", 108, scale_d=True, rotate=False),
    "random+1e3": lambda: _make("random+1e3", 108, scale_d=True, translate=1e3, rotate=False),
    "random+1e5": lambda: _make("random+1e5", 108, scale_d=True, translate=1e5, rotate=False),
    "extent": lambda: _extent(109),
}
_CACHE = {}


def case_set(name):
    """(CaseSet, Reference) of a class, computed once per process."""
    if name not in _CACHE:
        cs = MAKERS[name]()
        _CACHE[name] = (cs, Reference(cs))
    return _CACHE[name]


def own_rows(cs, ref):
    """(rows of ref that pair a ray with a triangle of its own group, the rays' o, d, tmin, tmax and the triangles, row by row)."""
    rows = ref.rows[ref.own]
    rays = cs.rays[rows["ray"]]
    return ref.own, rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], cs.tris[rows["tri"]]


# --------------------------------------------------------------------------------------- exact transforms for entered instances

def exact_transforms(dyadic):
    """Four object-to-world transforms [12] that are exact on the coordinates of any class: quarter turns and power-of-two scales,
    and for the dyadic class integer translations as well."""
    t = [(3.0, -5.0, 7.0), (-6.0, 2.0, 1.0), (4.0, 4.0, -3.0), (-1.0, 8.0, 5.0)] if dyadic else [(0.0, 0.0, 0.0)] * 4
    return [np.array(m, F32) for m in (
        [0, -1, 0, t[0][0], 1, 0, 0, t[0][1], 0, 0, 1, t[0][2]],        # quarter turn about z
        [2, 0, 0, t[1][0], 0, 2, 0, t[1][1], 0, 0, 2, t[1][2]],         # scale 2
        [0.5, 0, 0, t[2][0], 0, 0, -0.5, t[2][1], 0, 0.5, 0, t[2][2]],  # quarter turn about x, scale 1/2
        [0, 0, 4, t[3][0], 4, 0, 0, t[3][1], 0, 4, 0, t[3][2]])]        # the cyclic shift of the axes (two quarter turns), scale 4


def split_into_instances(cs):
    """The scene as four geometries under exact_transforms: [(object-space vertices [v, 3] float32, indices [t, 3], transform [12],
    world triangle of each primitive [t])]. Geometry k holds the groups g with g % 10 in its share (1, 2, 3 and 4 tenths), so the
    geometries differ in size and a flatten policy by triangle count flattens the two small ones. The object-space vertices
    transform back to the world-space ones exactly (asserted)."""
    share = [0, 1, 1, 2, 2, 2, 3, 3, 3, 3]
    out = []
    for k, m in enumerate(exact_transforms(cs.dyadic)):
        tri_ids = np.nonzero(np.asarray(share)[cs.tri_group % 10] == k)[0]
        used, local = np.unique(cs.indices[tri_ids], return_inverse=True)
        M, T = m.reshape(3, 4)[:, :3].astype(np.float64), m.reshape(3, 4)[:, 3].astype(np.float64)
        inverse = M.T / (M[0] @ M[0])   # M = s P with a signed permutation P: the inverse is P^T / s, exactly
        obj = (inverse @ (cs.vertices[used].astype(np.float64) - T).T).T
        obj32 = obj.astype(F32)
        back = (M @ obj32.astype(np.float64).T).T + T
        assert np.array_equal(obj32.astype(np.float64), obj) and np.array_equal(back.astype(F32), cs.vertices[used]) and np.array_equal(back, cs.vertices[used].astype(np.float64))
        out.append((obj32, local.reshape(-1, 3).astype(np.uint32), m, tri_ids))
    return out
