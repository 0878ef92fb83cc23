"""The geometry guide of the a-trous denoiser (twk_denoise_geometry; csrc/denoise_device.h, "the geometry guide") restated statement
for statement in numpy float32, for all three modes of the filter: plain (dv None), variance-guided (dv) and sampled variance (dv,
moments and min_samples). It imports nothing from the library: exp and sqrt are handed in (the tests pass the CPU oracle's, which the
math tests pin bit for bit against the device's). Also the synthetic pictures the host and the GPU tests share."""
import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)  # B3 spline; every product of two is exact
B3 = np.array([1 / 4, 1 / 2, 1 / 4], F)
RADIUS = 3         # TWK_DENOISE_MOMENTS_RADIUS
EPSILON = F(1e-3)  # TWK_DENOISE_LUMINANCE_EPSILON
CUT = F(87.0)


def finite3(c):
    return np.isfinite(c[..., :3]).all(axis=-1)


def dist2(a, b):
    e = a[..., :3] - b[..., :3]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def taps(height, width, dx, dy, s):
    """Slices (P, Q) of the pixels p whose tap q = p + (dx s, dy s) lies inside the picture; None when there is none."""
    y0, y1 = max(0, -dy * s), min(height, height - dy * s)
    x0, x1 = max(0, -dx * s), min(width, width - dx * s)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))


def normalize(v):
    """device_math.h normalize: invLen = 1 / sqrtf(dot(v, v)) with dot = x x + y y + z z left to right; v * invLen."""
    v = np.asarray(v, F)
    inv = F(1.0) / np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
    return (v * inv).astype(F)


class Centre:
    """What the centre of every pixel keeps for its taps, and which centres pass through."""

    def __init__(self, geometry, normal, camera, dg):
        cam = np.asarray(camera, F).reshape(12)
        P, Un, Vn, Wn = cam[0:3], normalize(cam[3:6]), normalize(cam[6:9]), normalize(cam[9:12])
        self.inv_position = F(1.0) / (F(dg.sigmaPosition) * F(dg.sigmaPosition))
        self.instance_stop = bool(dg.instanceStop)
        self.g = np.ascontiguousarray(geometry, F)
        self.bits = self.g[..., 3].copy().view(np.uint32)
        self.hit = self.bits != 0
        vx, vy, vz = self.g[..., 0] - P[0], self.g[..., 1] - P[1], self.g[..., 2] - P[2]
        vv = dot3(vx, vy, vz, vx, vy, vz)
        self.n = [(Un[k] * normal[..., 0] + Vn[k] * normal[..., 1]) - Wn[k] * normal[..., 2] for k in range(3)]
        self.inv_g = self.inv_position / vv
        ok = finite3(self.g) & np.isfinite(vv) & (vv != 0) & np.isfinite(self.inv_g)
        for k in range(3):
            ok &= np.isfinite(self.n[k])
        self.ok = ~self.hit | ok  # a miss centre has no plane term and is filtered

    def tap(self, P, Q, t):
        """(t with the tap's term added, mask of the taps the guide lets through)."""
        hp, hq = self.hit[P], self.hit[Q]
        allowed = hp == hq  # hit and miss never mix
        if self.instance_stop:
            allowed = allowed & (~hp | (self.bits[P] == self.bits[Q]))
        gp, gq = self.g[P], self.g[Q]
        d = dot3(gq[..., 0] - gp[..., 0], gq[..., 1] - gp[..., 1], gq[..., 2] - gp[..., 2], self.n[0][P], self.n[1][P], self.n[2][P])
        return np.where(hp & hq, t + (d * d) * self.inv_g[P], t).astype(F), allowed


def restate(beauty, albedo, normal, geometry, camera, dn, dg, exp, sqrt, dv=None, moments=None, min_samples=0):
    """beauty / albedo / normal: float32 [H, W, 4] (halves widened); geometry: float32 [H, W, 4]; camera: 12 floats P, U, V, W;
    dn / dg / dv: anything with the fields of TwkDenoiser / TwkDenoiserGeometry / TwkDenoiserVariance. Returns (float32 [H, W, 4]
    before the final narrowing, mask of the pixels whose output is the input's bits)."""
    b = np.ascontiguousarray(beauty, F)
    assert dn.inputKind == 2
    if dn.iterations == 0 or dn.blendFactor == 1.0:
        return b.copy(), np.ones(b.shape[:2], bool)
    demod = bool(dn.demodulateAlbedo)
    inv_color = F(1.0) / (F(dn.sigmaColor) * F(dn.sigmaColor))
    inv_normal = F(1.0) / (F(dn.sigmaNormal) * F(dn.sigmaNormal))
    inv_albedo = F(1.0) / (F(dn.sigmaAlbedo) * F(dn.sigmaAlbedo))
    blend = F(dn.blendFactor)
    height, width = b.shape[:2]
    sq = lambda v: sqrt(np.ascontiguousarray(v, F)).reshape(v.shape)
    ex = lambda ok, t: exp(np.ascontiguousarray(np.where(ok, -t, F(0)), F)).reshape(t.shape)
    with np.errstate(all="ignore"):
        # prepare
        c = b.copy()
        guides_finite = finite3(normal) & finite3(albedo)
        if demod:
            d = np.fmax(albedo[..., :3].astype(F), F(0.01))  # fmaxf: a NaN component gives 0.01
            c[..., :3] = b[..., :3] / d
        centre = Centre(geometry, normal, camera, dg)
        through_levels = guides_finite & centre.ok  # the centres the passes filter, their colour permitting
        if dv is not None:
            firefly, sigma_l = F(dv.fireflyThreshold), F(dv.sigmaLuminance)
            # moments pass
            l, fin = lum(c), finite3(c)
            s0, s1, s2 = (np.zeros((height, width), F) for _ in range(3))
            for dy in range(-RADIUS, RADIUS + 1):
                for dx in range(-RADIUS, RADIUS + 1):
                    pq = taps(height, width, dx, dy, 1)
                    if (dx == 0 and dy == 0) or pq is None:
                        continue
                    P, Q = pq
                    t = dist2(albedo[P], albedo[Q]) * inv_albedo
                    t = dist2(normal[P], normal[Q]) * inv_normal + t
                    t, allowed = centre.tap(P, Q, t)
                    ok = fin[Q] & allowed & (t <= CUT)  # a NaN t compares false
                    g = ex(ok, t)
                    lq = l[Q]
                    s0[P] = s0[P] + np.where(ok, g, F(0))  # adding +0 leaves the sums as they are
                    s1[P] = s1[P] + np.where(ok, g * lq, F(0))
                    s2[P] = s2[P] + np.where(ok, g * (lq * lq), F(0))
            reaches = fin & np.isfinite(l) & through_levels
            estimated = reaches & (s0 > 0)
            m1, m2 = s1 / s0, s2 / s0
            var = np.fmax(m2 - m1 * m1, F(0))  # fmaxf: a NaN difference gives 0
            out = np.concatenate([c[..., :3], np.where(estimated, var, F(0))[..., None]], axis=-1).astype(F)
            f = np.ones((height, width), F)
            if firefly > 0:
                limit = m1 + firefly * sq(var)
                clamp = estimated & (l > limit) & (limit > 0)
                f = np.where(clamp, limit / l, F(1.0)).astype(F)
                out[clamp, :3] = (c[..., :3] * f[..., None])[clamp]
            if moments is not None:
                mean, big_m2, n = (np.ascontiguousarray(moments[..., k], F) for k in range(3))
                sampled = reaches & (n >= F(min_samples)) & np.isfinite(mean) & np.isfinite(big_m2) & np.isfinite(n) & (mean > 0)
                v = big_m2 / ((n - F(1.0)) * n)
                if demod:
                    rho = l / mean  # l: of the demodulated colour before the clamp
                    v = v * (rho * rho)
                v = v * (f * f)
                out[sampled, 3] = v[sampled]
            c = out
        # levels
        for level in range(dn.iterations):
            s = 1 << level
            l, fin = lum(c), finite3(c)
            if dv is not None:
                fin_v = fin & np.isfinite(c[..., 3])
                vs, bs = np.zeros((height, width), F), np.zeros((height, width), F)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        pq = taps(height, width, dx, dy, s)
                        if pq is None:
                            continue
                        P, Q = pq
                        k = B3[dy + 1] * B3[dx + 1]
                        vs[P] = vs[P] + np.where(fin_v[Q], k * c[Q][..., 3], F(0))
                        bs[P] = bs[P] + np.where(fin_v[Q], k, F(0))
                vbar = np.where(bs > 0, vs / bs, F(0)).astype(F)
                inv_l = F(1.0) / (sigma_l * sq(vbar) + EPSILON)
            total = np.zeros((height, width, 3), F)
            wsum, vsum = np.zeros((height, width), F), np.zeros((height, width), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = taps(height, width, dx, dy, s)
                    if pq is None:
                        continue
                    P, Q = pq
                    cq = c[Q]
                    if dv is not None:
                        t = np.abs(l[P] - l[Q]) * inv_l[P]
                    else:
                        t = dist2(c[P], cq) * inv_color
                    t = t + dist2(normal[P], normal[Q]) * inv_normal
                    t = t + dist2(albedo[P], albedo[Q]) * inv_albedo
                    t, allowed = centre.tap(P, Q, t)
                    ok = fin[Q] & allowed & (t <= CUT)
                    w = np.where(ok, (H5[dy + 2] * H5[dx + 2]) * ex(ok, t), F(0))
                    total[P] = total[P] + np.where(ok[..., None], w[..., None] * cq[..., :3], F(0))
                    wsum[P] = wsum[P] + w
                    vsum[P] = vsum[P] + np.where(ok, (w * w) * cq[..., 3], F(0))
            nxt = c.copy()
            filtered = fin & through_levels
            if dv is not None:
                filtered &= np.isfinite(l)
                nxt[filtered, 3] = (vsum / (wsum * wsum))[filtered]
            nxt[filtered, :3] = (total / wsum[..., None])[filtered]
            c = nxt
        # finish (it does not read the geometry)
        r = c[..., :3] * d if demod else c[..., :3]
        o = b.copy()
        through = ~(finite3(b) & guides_finite & np.isfinite(r).all(axis=-1))
        o[~through, :3] = (r + blend * (b[..., :3] - r))[~through]
    assert o.dtype == F
    return o, through


# ---- the pictures of the tests --------------------------------------------------------------------------------------------------
CAMERA = np.array([0.5, 1.0, 4.0, 1.6, 0.0, 0.0, 0.0, 0.9, 0.0, 0.0, 0.0, -2.0], F)  # P, U, V, W: looks down -z


def instance_bits(ids):
    return np.asarray(ids, np.uint32).view(F)


def world_positions(height, width, depth, camera=CAMERA):
    """World positions of the pinhole rays of `camera` through the pixel centres where they meet the plane z = P.z - depth
    (depth: [H, W]); the surfaces face the camera, so their normal AOV is (0, 0, 1)."""
    cam = np.asarray(camera, np.float64)
    P, U, V, W = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    ndc_x = ((np.arange(width) + 0.5) / width * 2 - 1)[None, :, None]
    ndc_y = ((np.arange(height) + 0.5) / height * 2 - 1)[:, None, None]
    direction = U * ndc_x + V * ndc_y + W
    s = np.asarray(depth, np.float64)[..., None] / -direction[..., 2:3]
    return (P + direction * s).astype(F)


def synthetic(height, width, seed=20170728):
    """beauty, albedo, normal, moments, geometry (float32 [H, W, 4]) with: two parallel planes at different depths with equal
    albedo and normal (left / right of 45 % of the width); a region of misses (the top rows); two instances on the near plane;
    noise; NaN and inf in the colour, each guide, the moments and the geometry; a pixel at the camera position (vv == 0)."""
    rng = np.random.default_rng(seed)
    h, w = height, width
    beauty = rng.gamma(2.0, 0.5, (h, w, 4)).astype(F)
    beauty[..., 3] = rng.uniform(0.25, 1.0, (h, w)).astype(F)
    albedo = np.zeros((h, w, 4), F)
    albedo[..., :3] = (0.75, 0.75, 0.75)
    albedo[h // 2:, : w // 4, :3] = rng.uniform(0.1, 0.9, (h - h // 2, w // 4, 3)).astype(F)
    normal = np.zeros((h, w, 4), F)
    normal[..., 2] = 1.0
    tilt = rng.normal(0.0, 0.05, (h, w, 2)).astype(F)  # shading normals that waver a little, not renormalised
    normal[..., :2] = tilt
    edge = (w * 45) // 100
    depth = np.full((h, w), 3.0)
    depth[:, edge:] = 4.5
    geometry = np.zeros((h, w, 4), F)
    geometry[..., :3] = world_positions(h, w, depth)
    ids = np.full((h, w), 1, np.uint32)
    ids[:, edge:] = 2
    ids[h // 3:, : edge // 2] = 3  # a second instance on the near plane
    miss = np.zeros((h, w), bool)
    miss[:3, :] = True
    miss[3, w // 2:] = True
    ids[miss] = 0
    geometry[miss, :3] = 0.0
    normal[miss, :3] = 0.0
    albedo[miss, :3] = 0.0
    beauty[miss, :3] = rng.uniform(0.0, 0.2, (int(miss.sum()), 3)).astype(F)
    geometry[..., 3] = instance_bits(ids)
    moments = np.zeros((h, w, 4), F)
    l = lum(beauty)
    moments[..., 0] = l
    moments[..., 2] = rng.integers(1, 9, (h, w)).astype(F)  # some below, some at or above minSamples
    moments[..., 1] = (rng.uniform(0.0, 0.5, (h, w)) * l * l * moments[..., 2]).astype(F)
    # what is not finite: in the colour ...
    beauty[5, 5, 0] = np.inf
    beauty[6, 7, 1] = np.nan
    beauty[h - 1, w - 1, :3] = np.nan
    beauty[0, 0, 2] = -np.inf
    # ... in each guide ...
    albedo[8, 11, 0] = np.nan
    normal[9, 13, 1] = np.inf
    normal[10, 3, :3] = np.nan
    # ... in the moments ...
    moments[7, 9, 0] = np.nan
    moments[7, 10, 1] = np.inf
    moments[11, 4, 2] = np.nan
    moments[12, 5, 0] = 0.0
    # ... and in the geometry: a hit with a NaN position, one with an inf position, a miss with a NaN position (ignored)
    geometry[12, 15, 0] = np.nan
    geometry[13, 16, 2] = np.inf
    geometry[1, 2, 1] = np.nan
    # a hit at the camera position itself: vv == 0
    geometry[14, 8, :3] = CAMERA[:3]
    # a hit so close to the camera that invPosition / vv overflows
    geometry[15, 9, :3] = CAMERA[:3] + np.array([1e-20, 0, 0], F)
    # a finite normal so large that the world-space normal overflows
    normal[16, 6, :3] = (3e38, 3e38, -3e38)
    return beauty, albedo, normal, moments, geometry


def step_scene(height=24, width=40, instances=False):
    """The reason for the guide: the left half at colour exactly 1, the right half exactly 0, identical albedo and normal. Either
    the halves lie on two parallel planes (near / far) of one instance, or (instances) on one plane as two instances."""
    h, w = height, width
    beauty = np.zeros((h, w, 4), F)
    beauty[:, : w // 2, :3] = 1.0
    beauty[..., 3] = 1.0
    albedo = np.zeros((h, w, 4), F)
    albedo[..., :3] = 0.5
    normal = np.zeros((h, w, 4), F)
    normal[..., 2] = 1.0
    depth = np.full((h, w), 3.0)
    ids = np.ones((h, w), np.uint32)
    if instances:
        ids[:, w // 2:] = 2
    else:
        depth[:, w // 2:] = 4.5
    geometry = np.zeros((h, w, 4), F)
    geometry[..., :3] = world_positions(h, w, depth)
    geometry[..., 3] = instance_bits(ids)
    return beauty, albedo, normal, geometry
