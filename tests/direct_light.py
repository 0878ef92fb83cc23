"""Direct lighting against closed-form irradiance, light by light: scenes, float64 references and the statistic shared by
tests/test_direct_light_host.py (the oracle on a CPU; the only file that asserts the acceptance thresholds' outcomes before a GPU
is touched) and tests/test_gpu_direct_light.py (the HIP path). Everything goes through the calls Device and Oracle share, like
the slab anchor of tests/shading_fuzz.py; nothing here reads a sampler from inside.

The estimator.  With pathLengths (2, 2) a path is: primary hit, the light sample with its MIS weight, one BSDF-sampled segment,
the light-hit or miss branch with its MIS weight, end (Russian roulette starts at depth 2). With (1, 1) only the light-sampling
half is left. So a case has three IMAGES, each with a reference of its own:
  "light"  NEE on, (1, 1):  integral of q * w(p_rep, p_b) / p_rep * f * L * cos, w(a, b) = a^2 / (a^2 + b^2), p_b = cos / pi,
                            q the density the sampler draws from and p_rep the pdf it reports
  "sum"    NEE on, (2, 2):  rho / pi * E, E the irradiance (for `miss 2` the expectation of the reference's own estimator, whose
                            q and p_rep differ: sphere_environment_terms)
  "off"    NEE off, (2, 2): rho / pi * E, always the true integral
E is Lambert's polygon formula per light, minus what an occluder hides, averaged over a 4 x 4 sub-grid of the pixel's jitter
square (the camera model slab_expected_interval documents).

The statistic (statistic): block means over a 6 x 4 grid, R = sum (mean - reference)^2 / sum s^2 with s^2 from the two halves of
the run, and the relative bias of the image mean with its sigma. Bounds: R_BOUND, the 1 - 1e-4 quantile of R's null distribution
(null_quantile, which depends on the block count only), |bias| <= 4 sigma, and 4 sigma <= 0.01 for power.
sigma of the image mean: the difference of the two halves' image means is one number, and a sigma estimated from one number has
one degree of freedom - |bias| / sigma would then be Cauchy-like and exceed 4 in 16 % of correct runs. The image mean is the mean
of the block means, so its variance is pooled from the blocks' half differences instead (24 degrees of freedom)."""
import math

import numpy as np

import tweeker_raytracer_amd as twk
from shading_fuzz import HEIGHT, WIDTH, Scene, default_state, environment_light, feed, material, parallelogram_light, transform  # noqa: F401
from test_nee_switch import agreement, block_means, two_halves  # noqa: F401

RHO = (0.8, 0.5, 0.3)
IMAGES = ("light", "sum", "off")
SETTINGS = {"light": ((1, 1), True), "sum": ((2, 2), True), "off": ((2, 2), False)}  # image -> (pathLengths, NEE)
SUB = 4                      # sub-grid of the jitter square per axis
GRID = (6, 4)                # blocks across, down: 10 x 9 pixels each, the remainder cropped as block_means does
GGX_ROUGHNESS = (0.3, 0.15)
GGX_BLOCKS = 4               # G1 goes through test_nee_switch.agreement, whose grid is square
DENOMINATOR_EPSILON = 1.0e-6
M_LIGHT, M_RECEIVER, M_BLACK = 0, 1, 2


# ---- the statistic ------------------------------------------------------------------------------------------------------
def null_quantile(blocks, draws=100000, seed=17, q=1.0 - 1.0e-4):
    """The q quantile of R = sum mean_b^2 / sum s_b^2 when the two halves of every block are independent unit Gaussians around
    the reference: mean_b = (h1 + h2) / 2 and s_b^2 = (h1 - h2)^2 / 4 have the same variance and are independent. The three
    channels of a block share their paths, so they add no degrees of freedom: `blocks` is the count of independent terms."""
    rng = np.random.default_rng(seed)
    h1, h2 = rng.standard_normal((draws, blocks)), rng.standard_normal((draws, blocks))
    return float(np.quantile((((h1 + h2) / 2.0) ** 2).sum(axis=1) / (((h1 - h2) ** 2) / 4.0).sum(axis=1), q))


R_BOUND = 4.980       # round(null_quantile(GRID[0] * GRID[1]), 3)
R_BOUND_GGX = 7.138   # round(null_quantile(GGX_BLOCKS ** 2), 3)
BIAS_SIGMAS, BIAS_POWER = 4.0, 0.01


def grid_means(img, grid=GRID):
    """[down, across, 3] block means; each block is one call of block_means on its own crop."""
    gx, gy = grid
    bh, bw = img.shape[0] // gy, img.shape[1] // gx
    return np.array([[block_means(img[j * bh:(j + 1) * bh, i * bw:(i + 1) * bw], 1)[0, 0] for i in range(gx)] for j in range(gy)])


def pooled_sigma(first, second, grid):
    """Sigma of the mean of the block means (channels averaged), from the blocks' half differences."""
    d = (grid_means(first, grid) - grid_means(second, grid)).mean(axis=2)
    return math.sqrt(float((d ** 2 / 4.0).sum())) / d.size


def statistic(halves, reference):
    """halves = two_halves(...) = (first, second, whole); reference [H, W, 3] float64 -> (R, bias, sigma_bias)."""
    first, second, whole = halves
    m, r = grid_means(whole), grid_means(reference)
    s2 = (grid_means(first) - grid_means(second)) ** 2 / 4.0
    R = float(((m - r) ** 2).sum() / s2.sum())
    return R, float((m.mean() - r.mean()) / r.mean()), pooled_sigma(first, second, GRID) / float(r.mean())


def accepted(R, bias, sigma, bound=R_BOUND):
    return R <= bound and abs(bias) <= BIAS_SIGMAS * sigma


def ggx_statistic(on, off):
    """G1: (R of test_nee_switch.agreement, its relative bias of the image mean, that bias's sigma pooled from both runs).
    on, off = (first half, second half, whole) each."""
    R, _, _, _, bias = agreement(on, off, GGX_BLOCKS)
    grid = (GGX_BLOCKS, GGX_BLOCKS)
    sigma = math.hypot(pooled_sigma(on[0], on[1], grid), pooled_sigma(off[0], off[1], grid)) / float(on[2][..., :3].mean())
    return R, bias, sigma


def exact_bound(iterations):
    """An image whose every sample is the same number (E2 with NEE off: cosine sampling under a constant map has no variance) has
    no noise for the statistic to measure against. Its pixels are compared with rho * c itself instead, relative bound: u = 2^-24
    per fold of the running mean dst + t (x - dst) (x - dst and its product with t are far below dst, so the sum's rounding is
    the step's error) plus 16 u for the sample itself (four bilinear weights and products, the albedo, the throughput)."""
    return (iterations + 16) * 2.0 ** -24


# A sample of such an image can still be DROPPED whole: its BSDF ray leaves within a slope z of the horizon and either rounds out
# of the hemisphere (bxdf_diffuse.cu:72-76) or, from a hit point rounded below the plane, meets the receiver again beyond
# sceneEpsilon. The hit point o + t d (t and coordinates below 8) is within 3 * 8 * u = 1.5e-6 of the plane, and a ray of slope z
# is back at the plane after 1.5e-6 / z, which is beyond sceneEpsilon = 5e-5 for z < 0.03; cosine sampling puts z^2 = 9e-4 of its
# samples there and half the hit points are below. So a pixel is rho * c * (1 - j / iterations) for a whole j, and over the frame
# no more than DROPPED of all samples are dropped.
DROPPED = 4.5e-4
EXACT = {("E2", "off"): np.array(RHO) * np.array((0.5, 1.0, 2.0))}


def check_exact(whole, value, iterations):
    """-> (samples dropped over the frame, worst relative distance of a pixel from value * (1 - j / iterations)); asserts both."""
    ratio = whole[..., :3].astype(np.float64) / value
    j = np.round((1.0 - ratio.mean(axis=2)) * iterations)
    worst = float(np.abs(ratio - (1.0 - j / iterations)[..., None]).max())
    assert (j >= 0).all() and j.sum() <= DROPPED * iterations * j.size, (j.sum(), "samples dropped")
    assert worst <= exact_bound(iterations), (worst, exact_bound(iterations))
    return int(j.sum()), worst


def row(case_id, image, n, R, bias, sigma, extra=""):
    return f"direct-light {case_id:<12} {image:<5} n {n:<5} R {R:7.3f}  bias {bias:+.5f}  sigma_bias {sigma:.5f}{extra}"


# ---- geometry in float64 ------------------------------------------------------------------------------------------------
class Rect:
    """An axis-parallel rectangle in a plane y = const: x in [x0, x0 + sx], z in [z0, z0 + sz]. Lights are lit side down."""

    def __init__(self, x0, y, z0, sx, sz):
        self.x0, self.y, self.z0, self.sx, self.sz = (float(np.float32(v)) for v in (x0, y, z0, sx, sz))

    @property
    def area(self):
        return self.sx * self.sz

    def vertices(self):
        x0, x1, z0, z1, y = self.x0, self.x0 + self.sx, self.z0, self.z0 + self.sz, self.y
        return np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], np.float64)

    def scaled_area(self, factor):
        """The same centre, `factor` times the area."""
        k = math.sqrt(factor)
        r = Rect(0, self.y, 0, 0, 0)
        r.sx, r.sz = self.sx * k, self.sz * k
        r.x0, r.z0 = self.x0 + 0.5 * (self.sx - r.sx), self.z0 + 0.5 * (self.sz - r.sz)
        return r

    def mesh(self):
        return twk.mesh_parallelogram([self.x0, self.y, self.z0], [self.sx, 0.0, 0.0], [0.0, 0.0, self.sz], [0.0, -1.0, 0.0])


def stretch(scale, translate, angle_x):
    """shading_fuzz.transform extended: rotation about x, THEN a scale per world axis, then the translation. Scaling after the
    rotation matters: the plane's normal then turns with the scale, and only the inverse transpose gets it right."""
    r = np.asarray(transform(1.0, (0.0, 0.0, 0.0), angle_x), np.float64).reshape(3, 4)[:, :3]
    m = np.diag(np.asarray(scale, np.float64)) @ r
    return np.concatenate([m, np.asarray(translate, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(12)


class Receiver:
    """twk.mesh_plane(1, 1, 1), the square [-1, 1]^2 of the plane y = 0, under a row-major 3 x 4 transform."""

    def __init__(self, t):
        m = np.asarray(t, np.float32).astype(np.float64).reshape(3, 4)
        at = lambda x, z: m[:, :3] @ np.array([x, 0.0, z]) + m[:, 3]
        self.corner, self.eu, self.ev = at(-1, -1), at(1, -1) - at(-1, -1), at(-1, 1) - at(-1, -1)
        n = np.linalg.inv(m[:, :3]).T @ np.array([0.0, 1.0, 0.0])
        self.normal = n / np.linalg.norm(n)
        assert abs(self.normal @ self.eu) < 1e-9 and abs(self.normal @ self.ev) < 1e-9 and abs(self.eu @ self.ev) < 1e-9


def primary_points(camera, receiver, others):
    """[HEIGHT, WIDTH, SUB * SUB, 3]: where the primary rays through the sub-grid of every pixel's jitter square meet the
    receiver. Asserts that every one of them does, inside the receiver's edges, and before any rectangle of `others`."""
    P, U, V, W = (np.array(list(v), np.float64) for v in (camera.P, camera.U, camera.V, camera.W))
    sub = (np.arange(SUB) + 0.5) / SUB
    nx = ((np.arange(WIDTH)[:, None] + sub[None, :]) / WIDTH * 2.0 - 1.0).reshape(-1)     # [WIDTH * SUB]
    ny = ((np.arange(HEIGHT)[:, None] + sub[None, :]) / HEIGHT * 2.0 - 1.0).reshape(-1)
    n = receiver.normal
    assert n @ (P - receiver.corner) > 0.0, "the camera is on the receiver's lit side"

    def meet(nx, ny):
        d = U[None, None, :] * nx[None, :, None] + V[None, None, :] * ny[:, None, None] + W[None, None, :]
        # the camera is below every other rectangle and no ray rises: nothing but the receiver can be met first
        assert (d[..., 1] < 0.0).all() and all(r.y > P[1] for r in others), "nothing is in front of the receiver"
        t = (n @ (receiver.corner - P)) / (d @ n)
        assert (t > 0.0).all(), "every primary ray meets the receiver's plane"
        hit = P + t[..., None] * d
        a = ((hit - receiver.corner) @ receiver.eu) / (receiver.eu @ receiver.eu)
        b = ((hit - receiver.corner) @ receiver.ev) / (receiver.ev @ receiver.ev)
        assert a.min() > 0.0 and a.max() < 1.0 and b.min() > 0.0 and b.max() < 1.0, "every primary ray hits the receiver"
        return hit

    # the frame's corner rays: the rays of a frame meet a plane in the convex hull of where its corner rays do
    meet(np.array([-1.0, 1.0]), np.array([-1.0, 1.0]))
    hit = meet(nx, ny)
    hit = hit.reshape(HEIGHT, SUB, WIDTH, SUB, 3).transpose(0, 2, 1, 3, 4).reshape(HEIGHT, WIDTH, SUB * SUB, 3)
    return hit


def lambert(points, normal, vertices):
    """Lambert's formula with Le = 1: 1/2 sum_k acos(u_k . u_k+1) n . (u_k x u_k+1) / |u_k x u_k+1|, u_k the unit vectors from
    the point to the vertices. points [N, 3]; vertices [4, 3] or [N, 4, 3]. A polygon of no area gives 0. Asserts that the polygon
    is wholly above the point's horizon."""
    v = np.broadcast_to(vertices, (points.shape[0], 4, 3)) - points[:, None, :]
    height = v @ normal
    u = v / np.linalg.norm(v, axis=2, keepdims=True)
    total = np.zeros(points.shape[0])
    for k in range(4):
        a, b = u[:, k], u[:, (k + 1) % 4]
        c = np.cross(a, b)
        length = np.linalg.norm(c, axis=1)
        safe = np.where(length > 0.0, length, 1.0)
        total += np.where(length > 0.0, np.arccos(np.clip((a * b).sum(axis=1), -1.0, 1.0)) * (c @ normal) / safe, 0.0)
    total = np.abs(0.5 * total)
    assert (height[total > 0.0] > 0.0).all(), "the polygon is wholly above the receiver's horizon"
    return total


def quad_vertices(x0, x1, z0, z1, y):
    """[N, 4, 3] from per-point bounds; an empty intersection (x1 <= x0 or z1 <= z0) collapses to a point."""
    x1, z1 = np.maximum(x1, x0), np.maximum(z1, z0)
    empty = (x1 <= x0) | (z1 <= z0)
    x1, z1 = np.where(empty, x0, x1), np.where(empty, z0, z1)
    yy = np.full_like(x0, y)
    return np.stack([np.stack([x0, yy, z0], 1), np.stack([x1, yy, z0], 1), np.stack([x1, yy, z1], 1), np.stack([x0, yy, z1], 1)], 1)


def hidden(points, normal, rect, occluder):
    """Lambert's sum over the part of `rect` that `occluder` (a rectangle between the points and rect's plane) hides: the
    occluder's shadow volume from each point meets rect's plane in a rectangle, and two axis-parallel rectangles meet in one."""
    assert (points[:, 1] < occluder.y).all() and occluder.y < rect.y
    s = (rect.y - points[:, 1]) / (occluder.y - points[:, 1])
    px0, px1 = points[:, 0] + s * (occluder.x0 - points[:, 0]), points[:, 0] + s * (occluder.x0 + occluder.sx - points[:, 0])
    pz0, pz1 = points[:, 2] + s * (occluder.z0 - points[:, 2]), points[:, 2] + s * (occluder.z0 + occluder.sz - points[:, 2])
    x0, x1 = np.maximum(px0, rect.x0), np.minimum(px1, rect.x0 + rect.sx)
    z0, z1 = np.maximum(pz0, rect.z0), np.minimum(pz1, rect.z0 + rect.sz)
    return lambert(points, normal, quad_vertices(x0, x1, z0, z1, rect.y))


def form_factor(points, normal, rect, occluders=()):
    """Integral of cos over the solid angle of the visible part of rect. At most one occluder may hide a part of it."""
    f = lambert(points, normal, rect.vertices())
    parts = [hidden(points, normal, rect, o) for o in occluders if o.y < rect.y]
    if parts:
        assert (np.count_nonzero(np.array(parts) > 0.0, axis=0) <= 1).all(), "shadows of two occluders do not overlap on a light"
        f = f - np.sum(parts, axis=0)
    return f


def midpoint_form_factor(point, normal, rect, cells=512):
    """The check of lambert(): midpoint quadrature of cos cos_l / r^2 over the rectangle."""
    x = rect.x0 + (np.arange(cells) + 0.5) / cells * rect.sx
    z = rect.z0 + (np.arange(cells) + 0.5) / cells * rect.sz
    d = np.stack(np.broadcast_arrays(x[:, None] - point[0], rect.y - point[1], z[None, :] - point[2]), -1)
    r2 = (d * d).sum(-1)
    return float((np.maximum(d @ normal, 0.0) * np.maximum(d[..., 1], 0.0) / (r2 * r2)).sum() * rect.area / cells ** 2)


_GL = np.polynomial.legendre.leggauss(16)


def over_rect(points, normal, rect, integrand, chunk=4096):
    """Gauss-Legendre (16 x 16) over rect of integrand(cos, p_area) * cos * cos_l / r^2 per point, p_area = r^2 / (A cos_l) the
    parallelogram sampler's pdf over solid angle (light_sample.cu:156-177). Directions the sampler rejects
    (cos_l <= DENOMINATOR_EPSILON) and directions below the horizon contribute nothing."""
    gx, gw = 0.5 * (_GL[0] + 1.0), 0.5 * _GL[1]
    x, z = rect.x0 + gx * rect.sx, rect.z0 + gx * rect.sz
    w = (gw[:, None] * gw[None, :]).reshape(-1) * rect.area
    nodes = np.stack([np.repeat(x, 16), np.full(256, rect.y), np.tile(z, 16)], 1)
    out = np.empty(points.shape[0])
    for lo in range(0, points.shape[0], chunk):
        d = nodes[None, :, :] - points[lo:lo + chunk, None, :]
        r2 = (d * d).sum(-1)
        r = np.sqrt(r2)
        cos, cos_l = (d @ normal) / r, d[..., 1] / r
        ok = (cos > 0.0) & (cos_l > DENOMINATOR_EPSILON)
        cos_l = np.where(ok, cos_l, 1.0)
        out[lo:lo + chunk] = (np.where(ok, integrand(cos, r2 / (rect.area * cos_l)) * cos * cos_l / r2, 0.0) * w).sum(axis=1)
    return out


def power(a, b):
    return a * a / (a * a + b * b)


P_SPHERE = 0.25 / math.pi  # the constant environment's pdf (light_sample.cu:40-65)
# integral over the hemisphere of w(1 / 4 pi, cos / pi) cos = 2 pi * integral_0^1 c / (1 + 16 c^2) dc
HEMISPHERE_LIGHT_HALF = math.pi * math.log(17.0) / 16.0


# ---- the GGX receiver ---------------------------------------------------------------------------------------------------
def ggx_sample_success(wo, roughness, cells=(256, 64)):
    """Probability that bxdf_ggx_smith.cu's sampler (:96-106, :169-222) returns a direction, per outgoing direction wo [N, 3] in
    the tangent frame (z the normal): the half vector is drawn from D cos by stretching an isotropic draw, the reflection of wo
    about it must leave the surface, and wo . wm must be positive. Midpoint rule over the unit square, fine along u1 (across
    which the outcome flips), coarse along u2 (along which the flip point moves smoothly).
    It matters because the reference sets FLAG_DIFFUSE at the sampler's END (:221) and closesthit.cu:253 samples a light only
    with that flag: a failed BSDF sample drops the light sample of the same vertex, so with NEE on the light half is scaled by
    this probability. NEE off has no such term."""
    ax, ay = roughness
    u1, u2 = (np.arange(cells[0]) + 0.5) / cells[0], (np.arange(cells[1]) + 0.5) / cells[1]
    theta = np.arctan(ay * np.sqrt(u1) / np.sqrt(1.0 - u1))[:, None]
    phi = (2.0 * math.pi * u2)[None, :]
    wm = np.stack(np.broadcast_arrays(np.cos(phi) * np.sin(theta) * ax / ay, np.sin(phi) * np.sin(theta), np.cos(theta)), -1).reshape(-1, 3)
    wm /= np.linalg.norm(wm, axis=1, keepdims=True)
    out = np.empty(wo.shape[0])
    for lo in range(0, wo.shape[0], 256):
        w = wo[lo:lo + 256]
        dot = w @ wm.T                                              # [n, cells]
        wi_z = 2.0 * dot * wm[None, :, 2] - w[:, 2:3]
        out[lo:lo + 256] = ((wi_z > 0.0) & (dot > 0.0) & (w[:, 2:3] > 0.0) & (wm[None, :, 2] > DENOMINATOR_EPSILON)).mean(axis=1)
    return out


# ---- the spherical environment ------------------------------------------------------------------------------------------
def bilinear(tex, u, v):
    """tex2D as the oracle states it (normalized coordinates, u wraps, v clamps) in float64: tex [H, W, C], u [M], v [N] -> [N, M, C]."""
    H, W = tex.shape[:2]
    xb, yb = (u - np.floor(u)) * W - 0.5, np.clip(v, 0.0, 1.0) * H - 0.5
    xf, yf = np.floor(xb), np.floor(yb)
    a, b = (xb - xf)[None, :, None], (yb - yf)[:, None, None]
    i0, i1 = xf.astype(int) % W, (xf.astype(int) + 1) % W
    j0, j1 = np.clip(yf.astype(int), 0, H - 1), np.clip(yf.astype(int) + 1, 0, H - 1)
    return ((1 - a) * (1 - b) * tex[j0][:, i0] + a * (1 - b) * tex[j0][:, i1] + (1 - a) * b * tex[j1][:, i0] + a * b * tex[j1][:, i1])


def importance(tex):
    """src/Texture.cpp:1499-1645 as oracle/orc_render.cpp cites it: (probability of each texel [H, W], envIntegral). The function
    sampled is the 3 x 3 Gaussian-filtered intensity (x wraps, y clamps) times the row's sin(theta); the integral is of the
    unfiltered intensity."""
    H, W = tex.shape[:2]
    i = tex[..., :3].astype(np.float64).sum(axis=2)
    up, down = np.concatenate([i[:1], i[:-1]]), np.concatenate([i[1:], i[-1:]])
    side = lambda a: np.roll(a, 1, axis=1) + np.roll(a, -1, axis=1)
    g = (i * 0.619347 + (up + down + side(i)) * 0.0838195 + (side(up) + side(down)) * 0.0113437) / 3.0
    sin_row = np.sin(math.pi * (np.arange(H) + 0.5) / H)[:, None]
    func = g * sin_row
    return func / func.sum(), float((i / 3.0 * sin_row).sum() * 2.0 * math.pi * math.pi / (W * H))


def sphere_environment_terms(tex, rotation, normal, sub, integral_scale=1.0):
    """A Lambert receiver of albedo 1 under the spherical environment alone, nothing occluding: (true radiance, the light half's
    expectation, the expectation of light half + BSDF half), each [3], by midpoint quadrature on sub x sub cells per texel.
    The sampler draws a texel with importance()'s probability and a point uniformly in it (light_sample.cu:67-153), so
    q du dv = P_texel W H du dv, while it reports p_rep = intensity(bilinear lookup) / envIntegral: the two differ, and the
    estimator's expectation is not the true integral. integral_scale multiplies envIntegral (a negative control)."""
    tex = np.asarray(tex, np.float64)
    H, W = tex.shape[:2]
    assert sub >= 8
    u, v = (np.arange(W * sub) + 0.5) / (W * sub), (np.arange(H * sub) + 0.5) / (H * sub)
    L = bilinear(tex[..., :3], u, v)
    phi, theta = (u - rotation) * 2.0 * math.pi, v * math.pi
    sin_t = np.sin(theta)[:, None]
    direction = np.stack([-np.sin(phi)[None, :] * sin_t, np.broadcast_to(-np.cos(theta)[:, None], (v.size, u.size)), np.cos(phi)[None, :] * sin_t], -1)
    cos = np.maximum(direction @ normal, 0.0)[..., None]
    dudv = 1.0 / (u.size * v.size)
    domega = 2.0 * math.pi * math.pi * sin_t[..., None] * dudv
    true = (L * cos * domega).sum(axis=(0, 1)) / math.pi
    probability, integral = importance(tex)
    q = np.repeat(np.repeat(probability, sub, axis=0), sub, axis=1)[..., None] * (W * H)
    p_rep = L.sum(axis=2, keepdims=True) / 3.0 / (integral * integral_scale)
    lit = (cos > 0.0) & (p_rep > 0.0)
    w_light = np.where(lit, power(p_rep, cos / math.pi), 0.0)
    light = (np.where(lit, q * w_light / np.where(lit, p_rep, 1.0), 0.0) * L * cos * dudv).sum(axis=(0, 1)) / math.pi
    bsdf = (np.where(cos > 0.0, 1.0 - np.where(p_rep > 0.0, power(p_rep, cos / math.pi), 0.0), 0.0) * L * cos * domega).sum(axis=(0, 1)) / math.pi
    return true, light, light + bsdf


def constant_map(width=128, height=64, colour=(0.5, 1.0, 2.0)):
    return np.broadcast_to(np.array(list(colour) + [1.0], np.float32), (height, width, 4)).copy()


LOBE_U, LOBE_V, LOBE_KAPPA, LOBE_FLOOR, LOBE_PEAK, LOBE_TINT = 0.57, 0.70, 8.0, 0.1, 5.0, (1.0, 0.8, 0.6)


def lobe_map(width=64, height=32):
    """One smooth bright lobe, floor + (peak - floor) exp(kappa (cos gamma - 1)) about the direction of (LOBE_U, LOBE_V), on a dim
    floor; evaluated in float64 at the texel centres. The lobe is off every axis and 72 degrees of azimuth from the tilt."""
    u, v = (np.arange(width) + 0.5) / width, (np.arange(height) + 0.5) / height
    angle = lambda uu, vv: np.stack(np.broadcast_arrays(-np.sin(2 * math.pi * uu) * np.sin(math.pi * vv), -np.cos(math.pi * vv),
                                                        np.cos(2 * math.pi * uu) * np.sin(math.pi * vv)), -1)
    cos_gamma = angle(u[None, :], v[:, None]) @ angle(np.float64(LOBE_U), np.float64(LOBE_V))
    bump = np.exp(LOBE_KAPPA * (cos_gamma - 1.0))[..., None]
    rgb = LOBE_FLOOR + (LOBE_PEAK - LOBE_FLOOR) * bump * np.array(LOBE_TINT)
    return np.concatenate([rgb, np.ones((height, width, 1))], axis=2).astype(np.float32)


# ---- cases --------------------------------------------------------------------------------------------------------------
PLANE = stretch((9.0, 1.0, 9.0), (0.0, 0.0, -1.0), 0.0)
TILTED = stretch((9.0, 4.0, 8.0), (0.0, 0.3, -1.0), 0.5)   # about 15 degrees, rising away from the camera
LIGHT_1 = (Rect(-1.0, 3.5, -2.0, 2.0, 2.0), (10.0, 8.0, 6.0))
LIGHT_2A = (Rect(-2.5, 3.0, -2.5, 1.5, 1.5), (10.0, 8.0, 6.0))
LIGHT_2B = (Rect(0.75, 4.0, -1.25, 1.0, 1.0), (6.0, 12.0, 18.0))
ABOVE_LIGHT_1 = Rect(-1.5, 3.75, -2.5, 3.0, 3.0)
BELOW_LIGHT_1 = Rect(-0.25, 2.875, -2.25, 1.5, 1.25)
OVERHEAD = Rect(-1.5, 3.5, -2.5, 3.0, 2.5)


class Case:
    """One scene with its float64 description. lights: [("rect", Rect, emission) | ("constant",) | ("sphere", map)] in light order."""

    def __init__(self, case_id, lights, miss, tilted=False, occluders=(), rotation=0.0, variant=0, ggx=False, n=None):
        self.id, self.lights, self.miss, self.tilted, self.occluders, self.variant, self.ggx = case_id, lights, miss, tilted, tuple(occluders), variant, ggx
        self.n = {"light": 256, "sum": 256, "off": 256}
        self.n.update(n or {})
        self.images = ("sum", "off") if case_id in ("P1b", "P1c") else IMAGES
        t = TILTED if tilted else PLANE
        self.receiver = Receiver(t)
        s = Scene()
        s.miss, s.env_rotation = miss, float(np.float32(rotation))
        self.rotation = s.env_rotation
        if tilted:
            s.flatten = (0, 0)  # the receiver stays an instance: its normal goes through worldToObject
        s.camera = twk.camera_frustum((0.0, 0.0, -1.0), 0.75, 0.72, 40.0, 4.0, WIDTH / HEIGHT)
        s.materials = [material(1, albedo=(0.0, 0.0, 0.0), thinwalled=1),
                       material(3, albedo=(0.9, 0.9, 0.9), roughness=GGX_ROUGHNESS) if ggx else material(0, albedo=RHO),
                       material(0, albedo=(0.0, 0.0, 0.0))]
        geometry = lambda mesh: (s.geometries.append((np.ascontiguousarray(mesh[0], np.float32), np.ascontiguousarray(mesh[1], np.uint32))), len(s.geometries) - 1)[1]
        s.instances.append((geometry(twk.mesh_plane(1, 1, 1)), t, M_RECEIVER, -1))
        for k, light in enumerate(lights):
            if light[0] == "rect":
                r, emission = light[1], light[2]
                assert r.sx == r.sz
                l = parallelogram_light((r.x0, r.y, r.z0), r.sx, emission)
                assert float(l.area) == float(np.float32(r.area))
                s.lights.append(l)
                s.instances.append((geometry(twk.mesh_parallelogram(list(l.position), list(l.vecU), list(l.vecV), list(l.normal))), transform(), M_LIGHT, k))
            else:
                assert k == 0
                s.lights.append(environment_light())
                if light[0] == "sphere":
                    s.textures.append((2, light[1]))
        for r in self.occluders:
            s.instances.append((geometry(r.mesh()), transform(), M_BLACK, -1))
        self.scene = s
        self._points = None

    def state(self, image):
        return default_state(self.scene, SETTINGS[image][0], samplesSqrt=1, lensShader=0)

    def nee(self, image):
        return SETTINGS[image][1]

    @property
    def rects(self):
        return [l[1] for l in self.lights if l[0] == "rect"]

    @property
    def points(self):
        if self._points is None:
            self._points = primary_points(self.scene.camera, self.receiver, self.rects + list(self.occluders))
        return self._points

    # -- references: [HEIGHT, WIDTH, 3] float64 --
    def _over_pixels(self, per_point):
        """per_point([N, 3] points) -> [N] or [N, 3]; averaged over the sub-grid."""
        p = self.points.reshape(-1, 3)
        return np.asarray(per_point(p)).reshape(HEIGHT, WIDTH, SUB * SUB, -1).mean(axis=2)

    def reference(self, image, control=None):
        """control: None, or one of the negative controls - ("area", 1.02), ("no_occluder",), ("no_num_lights",),
        ("shift", texels), ("mirror",), ("integral", 1.02) - applied to this reference, never to what is rendered."""
        control = control or ("none",)
        rho, normal = np.array(RHO), self.receiver.normal
        grow = (lambda r: r.scaled_area(control[1])) if control[0] == "area" else (lambda r: r)
        occluders = () if control[0] == "no_occluder" else self.occluders
        count = len(self.lights)
        if self.lights[0][0] == "sphere":
            assert count == 1 and not self.occluders
            tex = np.asarray(self.lights[0][1], np.float64)
            if control[0] == "shift":
                tex = np.roll(tex, control[1], axis=1)
            if control[0] == "mirror":
                tex = tex[:, ::-1]
            true, light, both = sphere_environment_terms(tex, self.rotation, normal, 8 * 128 // tex.shape[1], control[1] if control[0] == "integral" else 1.0)
            value = {"light": light, "sum": both, "off": true}[image] * rho
            return np.broadcast_to(value, (HEIGHT, WIDTH, 3)).copy()

        def irradiance(p):
            """The true integral: Lambert's formula per rectangle, the constant environment where no rectangle is."""
            total, covered = np.zeros((p.shape[0], 3)), np.zeros(p.shape[0])
            for light in self.lights:
                if light[0] == "rect":
                    total += form_factor(p, normal, grow(light[1]), occluders)[:, None] * np.array(light[2])
                    for other in self.rects:  # a lower light is an occluder too: the scenes keep it out of the way
                        assert other.y >= light[1].y or not hidden(p, normal, grow(light[1]), other).any(), "no light hides another"
                    covered += lambert(p, normal, grow(light[1]).vertices())
            if self.lights[0][0] == "constant":
                for o in occluders:
                    covered += lambert(p, normal, o.vertices())
                total += (math.pi - covered)[:, None]
            return total

        def light_half(p):
            total = np.zeros((p.shape[0], 3))
            for light in self.lights:
                if light[0] == "rect":
                    assert not occluders
                    r = grow(light[1])
                    total += over_rect(p, normal, r, lambda cos, pdf: power(pdf, cos / math.pi))[:, None] * np.array(light[2])
            if self.lights[0][0] == "constant":
                env = np.full(p.shape[0], HEMISPHERE_LIGHT_HALF)
                for r in [grow(l[1]) for l in self.lights if l[0] == "rect"] + list(occluders):
                    env -= over_rect(p, normal, r, lambda cos, pdf: power(P_SPHERE, cos / math.pi))
                total += env[:, None]
            return total

        if image == "off" or (image == "sum" and control[0] != "no_num_lights"):
            return self._over_pixels(irradiance) * rho / math.pi
        half = self._over_pixels(light_half) * rho / math.pi
        if control[0] == "no_num_lights":  # the estimator without its numLights factor: the light half is 1 / numLights of it
            if image == "light":
                return half / count
            return self._over_pixels(irradiance) * rho / math.pi - half * (1.0 - 1.0 / count)
        return half

    def ggx_success(self):
        """[HEIGHT, WIDTH] ggx_sample_success at the pixels' centres. The plane's tangent is x and its normal y; the sign of the
        bitangent does not matter, the distribution is even in it."""
        assert self.ggx and not self.tilted
        P = np.array(list(self.scene.camera.P), np.float64)
        wo = P[None, :] - self.points.mean(axis=2).reshape(-1, 3)
        wo /= np.linalg.norm(wo, axis=1, keepdims=True)
        local = np.stack([wo[:, 0], -wo[:, 2], wo[:, 1]], 1)
        return ggx_sample_success(local, GGX_ROUGHNESS).reshape(HEIGHT, WIDTH)

    def discretisation(self):
        """`miss 2` only: (expectation of the reference's estimator - true integral) / true integral, over the channels' sum."""
        true, _, both = sphere_environment_terms(np.asarray(self.lights[0][1], np.float64), self.rotation, self.receiver.normal, 8 * 128 // self.lights[0][1].shape[1])
        return float(((both - true) * np.array(RHO)).sum() / (true * np.array(RHO)).sum())


def make_cases():
    p1 = [("rect",) + LIGHT_1]
    cases = [
        Case("P1", p1, 0, n={"off": 1024}),
        Case("P1-optix7gui", p1, 0, variant=1, n={"off": 1024}),
        Case("P1-tilted", p1, 0, tilted=True, n={"off": 1024}),
        Case("P1b", p1, 0, occluders=[ABOVE_LIGHT_1], n={"off": 1024}),
        Case("P1c", p1, 0, occluders=[BELOW_LIGHT_1], n={"off": 1536}),
        Case("P2", [("rect",) + LIGHT_2A, ("rect",) + LIGHT_2B], 0, n={"off": 1536}),
        Case("P3", [("constant",)] + p1, 1),
        Case("E1", [("constant",)], 1, tilted=True, occluders=[OVERHEAD]),
        Case("E2", [("sphere", constant_map())], 2, rotation=0.3),
        Case("E3", [("sphere", lobe_map())], 2, rotation=0.37),
        Case("E3-tilted", [("sphere", lobe_map())], 2, tilted=True, rotation=0.37),
        Case("G1", p1, 0, ggx=True, n={"light": 512, "sum": 512, "off": 4096}),
    ]
    return {c.id: c for c in cases}


# negative controls: case -> [(name, control, images it changes the reference of)]
CONTROLS = {
    "P1": [("area x 1.02", ("area", 1.02), IMAGES)],
    "P1-optix7gui": [("area x 1.02", ("area", 1.02), IMAGES)],
    "P1-tilted": [("area x 1.02", ("area", 1.02), IMAGES)],
    "P1b": [("area x 1.02", ("area", 1.02), ("sum", "off"))],
    "P1c": [("area x 1.02", ("area", 1.02), ("sum", "off")), ("occluder removed", ("no_occluder",), ("sum", "off"))],
    "P2": [("area x 1.02", ("area", 1.02), IMAGES), ("numLights dropped", ("no_num_lights",), ("light", "sum"))],
    "P3": [("area x 1.02", ("area", 1.02), IMAGES), ("numLights dropped", ("no_num_lights",), ("light", "sum"))],
    "E1": [("occluder removed", ("no_occluder",), IMAGES)],
    "E2": [("envIntegral x 1.02", ("integral", 1.02), ("light", "sum"))],
    "E3-tilted": [("map shifted two texels in u", ("shift", 2), IMAGES), ("map mirrored in u", ("mirror",), IMAGES)],
}


def render_halves(render_one, read, n, snapshot=None):
    """two_halves of one image on a Device or an Oracle that feed() has filled: render_one(iteration), read() -> image.
    snapshot: a dict that receives the image after the first 2 iterations under "two"."""
    def render(it):
        render_one(it)
        if snapshot is not None and it == 1:
            snapshot["two"] = read().copy()
    return two_halves(render, read, n)
