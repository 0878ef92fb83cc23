"""The temporal merge of csrc/temporal_device.h restated statement for statement in numpy float32 (no GPU needed), the centre
rays of the geometry AOV, and the synthetic frames the tests feed both sides. The projection, the footprint's taps, the gather and
the capped history are written here once: tests/temporal_rectify_restate.py and tests/temporal_cascade_restate.py call them. Shared by tests/test_temporal_host.py (CPU) and
tests/test_gpu_temporal.py / tests/test_gpu_geometry.py (which compare the device's bits with it)."""
import numpy as np

F = np.float32
U32 = np.uint32


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _finite3(a):
    return np.isfinite(a[..., 0]) & np.isfinite(a[..., 1]) & np.isfinite(a[..., 2])


def camera_array(cam):
    """12 float32 (P, U, V, W) of a CameraDefinition, or of anything array-like."""
    if hasattr(cam, "P"):
        return np.array(list(cam.P) + list(cam.U) + list(cam.V) + list(cam.W), F)
    return np.ascontiguousarray(cam, F).reshape(12)


def camera_constants(cam):
    """temporalCamera: P', A = cross(V', W'), B = cross(W', U'), C = cross(U', V'), D = dot(U', A), every operation in float32."""
    c = camera_array(cam)
    Ux, Uy, Uz, Vx, Vy, Vz, Wx, Wy, Wz = (c[i] for i in range(3, 12))
    with np.errstate(all="ignore"):
        A = (Vy * Wz - Vz * Wy, Vz * Wx - Vx * Wz, Vx * Wy - Vy * Wx)
        B = (Wy * Uz - Wz * Uy, Wz * Ux - Wx * Uz, Wx * Uy - Wy * Ux)
        C = (Uy * Vz - Uz * Vy, Uz * Vx - Ux * Vz, Ux * Vy - Uy * Vx)
        D = _dot3(Ux, Uy, Uz, *A)
    assert all(isinstance(v, F) for v in A + B + C + (D,))
    return (c[0], c[1], c[2]), A, B, C, D


def centre_rays(cam, width, height):
    """centreRay for every pixel: primaryRay's pinhole branch with sampleX = sampleY = 0.5f. Returns (origin [3], directions [H, W, 3])."""
    c = camera_array(cam)
    P, U, V, W = c[0:3], c[3:6], c[6:9], c[9:12]
    px = np.arange(width, dtype=F)[None, :].repeat(height, 0)
    py = np.arange(height, dtype=F)[:, None].repeat(width, 1)
    ndcx = ((px + F(0.5)) / F(width)) * F(2.0) - F(1.0)
    ndcy = ((py + F(0.5)) / F(height)) * F(2.0) - F(1.0)
    d = [(U[k] * ndcx + V[k] * ndcy) + W[k] for k in range(3)]  # U * ndcX + V * ndcY + W
    inv = F(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])  # normalize: 1 / sqrtf(dot), then the product
    out = np.stack([d[0] * inv, d[1] * inv, d[2] * inv], axis=-1)
    assert out.dtype == F
    return P, out


def project(g, cam, width, height):
    """temporalProject over g [..., 4]: (fx, fy, vv, front, inside), every operation in float32."""
    (P0, P1, P2), A, B, C, D = camera_constants(cam)
    with np.errstate(all="ignore"):
        vx, vy, vz = g[..., 0] - P0, g[..., 1] - P1, g[..., 2] - P2
        a, b, c = _dot3(vx, vy, vz, *A), _dot3(vx, vy, vz, *B), _dot3(vx, vy, vz, *C)
        vv = _dot3(vx, vy, vz, vx, vy, vz)
        front = c * D > F(0.0)
        fx = ((a / c + F(1.0)) * F(0.5)) * F(width) - F(0.5)
        fy = ((b / c + F(1.0)) * F(0.5)) * F(height) - F(0.5)
        inside = (fx >= F(-1.0)) & (fx < F(width)) & (fy >= F(-1.0)) & (fy < F(height))
    assert fx.dtype == F and fy.dtype == F and vv.dtype == F
    return fx, fy, vv, front, inside


def footprint_taps(g, hg, fx, fy, vv, ok, tolerance):
    """The four taps of the footprint of (fx, fy) in the definition's order, dy = 0, 1 outer and dx = 0, 1 inner, for the pixels
    `ok` (candidates that project into the previous view). Per tap: (w, q, inpic, same, near) — the bilinear weight, the history
    pixel q = (qy, qx) as an index clipped into the picture, and the masks every merge shares: q inside the picture, the history's
    geometry hg[q] with the instance bits of g, and within the tolerance of g (temporalTapGeometry)."""
    height, width = g.shape[:2]
    gw = g[..., 3].view(U32)
    with np.errstate(all="ignore"):
        tol2 = F(tolerance) * F(tolerance)
        fx0, fy0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - fx0, fy - fy0
        x0, y0 = np.where(ok, fx0, F(0)).astype(np.int64), np.where(ok, fy0, F(0)).astype(np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            with np.errstate(all="ignore"):
                qx, qy = x0 + dx, y0 + dy
                inpic = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                q = (np.clip(qy, 0, height - 1), np.clip(qx, 0, width - 1))
                hgq = hg[q]
                same = hgq[..., 3].view(U32) == gw
                ex, ey, ez = hgq[..., 0] - g[..., 0], hgq[..., 1] - g[..., 1], hgq[..., 2] - g[..., 2]
                near = (ex * ex + ey * ey) + ez * ez <= tol2 * vv
                w = (tx if dx else F(1.0) - tx) * (ty if dy else F(1.0) - ty)
            yield w, q, inpic, same, near


def gather(cur, mc, g, history, cam, tolerance):
    """temporalGather on float32 [H, W, 4] arrays, history = (colour, moments, geometry): the candidates, the projection and the
    four taps. Returns (sums, took, counts) — sums = (sx, sy, sz, smean, sM2, sn, ws), took = ws > 0, and one count per branch."""
    hc, hm, hg = (np.ascontiguousarray(a, F) for a in history)
    height, width = cur.shape[:2]
    with np.errstate(all="ignore"):
        hit = g[..., 3].view(U32) != 0
        finite = _finite3(g) & _finite3(cur) & _finite3(mc)
        cand = hit & finite & ~(mc[..., 2] < F(1.0))
        fx, fy, vv, front, inside = project(g, cam, width, height)
        ok = cand & front & inside
        sx, sy, sz, smean, sm2, sn, ws = (np.zeros((height, width), F) for _ in range(7))
        taps = np.zeros((height, width), np.int64)
        counts = dict(outside=0, id_mismatch=0, position=0, history_not_finite=0, history_n_below_1=0)
        for w, q, inpic, same, near in footprint_taps(g, hg, fx, fy, vv, ok, tolerance):
            hcq, hmq = hc[q], hm[q]
            fin = _finite3(hcq) & _finite3(hmq)
            enough = hmq[..., 2] >= F(1.0)
            counted = ok & inpic & same & near & fin & enough
            sx = np.where(counted, sx + w * hcq[..., 0], sx)
            sy = np.where(counted, sy + w * hcq[..., 1], sy)
            sz = np.where(counted, sz + w * hcq[..., 2], sz)
            smean = np.where(counted, smean + w * hmq[..., 0], smean)
            sm2 = np.where(counted, sm2 + w * hmq[..., 1], sm2)
            sn = np.where(counted, sn + w * hmq[..., 2], sn)
            ws = np.where(counted, ws + w, ws)
            taps += counted
            counts["outside"] += int((ok & ~inpic).sum())
            counts["id_mismatch"] += int((ok & inpic & ~same).sum())
            counts["position"] += int((ok & inpic & same & ~near).sum())
            counts["history_not_finite"] += int((ok & inpic & same & near & ~fin).sum())
            counts["history_n_below_1"] += int((ok & inpic & same & near & fin & ~enough).sum())
        took = ws > F(0.0)
    counts.update(miss=int((~hit).sum()), current_not_finite=int((hit & ~finite).sum()), current_n_below_1=int((hit & finite & ~cand).sum()),
                  behind=int((cand & ~front).sum()), off_screen=int((cand & front & ~inside).sum()), no_tap=int((ok & ~took).sum()),
                  one_tap=int((took & (taps == 1)).sum()), four_taps=int((took & (taps == 4)).sum()), took=int(took.sum()))
    return (sx, sy, sz, smean, sm2, sn, ws), took, counts


def capped_history(sums, max_history):
    """temporalHistory: the six quotients by ws and the cap. Returns (hx, hy, hz, hmean, hM2, hn, capped), meaningful where ws > 0."""
    sx, sy, sz, smean, sm2, sn, ws = sums
    max_h = F(max_history)
    with np.errstate(all="ignore"):
        hx, hy, hz, hmean, hm2, hn = sx / ws, sy / ws, sz / ws, smean / ws, sm2 / ws, sn / ws
        capped = hn > max_h
        hm2 = np.where(capped, hm2 * (max_h / hn), hm2)
        hn = np.where(capped, max_h, hn)
    return hx, hy, hz, hmean, hm2, hn, capped


def restate_temporal(cur, mc, g, history, cam, max_history, tolerance, info=None):
    """twk_temporal_accumulate on float32 [H, W, 4] arrays: cur = the current colour WIDENED, mc its moments, g its geometry;
    history = (colour, moments, geometry) or None; cam = the history's camera. Returns (colour f32, moments f32, took) — took: the
    pixels that merged history; the others pass through (the caller keeps the input's bits there). info (a dict) receives one
    count per branch of the definition."""
    cur, mc, g = (np.ascontiguousarray(a, F) for a in (cur, mc, g))
    colour, moments = cur.copy(), mc.copy()
    if history is None:
        return colour, moments, np.zeros(cur.shape[:2], bool)
    sums, took, counts = gather(cur, mc, g, history, cam, tolerance)
    hx, hy, hz, hmean, hm2, hn, capped = capped_history(sums, max_history)
    with np.errstate(all="ignore"):
        n = hn + mc[..., 2]
        r = mc[..., 2] / n
        merged = np.stack([hx + (cur[..., 0] - hx) * r, hy + (cur[..., 1] - hy) * r, hz + (cur[..., 2] - hz) * r, cur[..., 3]], axis=-1)
        d = mc[..., 0] - hmean
        merged_m = np.stack([hmean + d * r, (hm2 + mc[..., 1]) + (d * d) * (hn * r), n, np.zeros_like(n)], axis=-1)
    assert merged.dtype == F and merged_m.dtype == F
    colour[took] = merged[took]
    moments[took] = merged_m[took]
    if info is not None:
        info.update(counts)
        info.update(capped=int((took & capped).sum()), uncapped=int((took & ~capped).sum()))
    return colour, moments, took


# ---- synthetic frames -------------------------------------------------------------------------------------------------------------
def look_at(eye, target, fov_deg, aspect):
    """A pinhole camera as 12 float32 (P, U, V, W): W towards the target, U right, V up, |U| = aspect |V| = aspect tan(fov / 2) |W|."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    w = target - eye
    u = np.cross(w, (0.0, 1.0, 0.0))
    v = np.cross(u, w)
    half = np.linalg.norm(w) * np.tan(np.radians(fov_deg) / 2)
    u, v = u / np.linalg.norm(u) * half * aspect, v / np.linalg.norm(v) * half
    return np.concatenate([eye, u, v, w]).astype(F)


def _plane_geometry(cam, width, height, top):
    """Geometry AOV of a synthetic world as the camera sees it: the wall z = 0, which is instance 1 for x < 0 and instance 2 beyond
    (an id edge), with a slab 0.4 in front of it for 0.3 < x < 0.8 that has the wall's instance (a depth step within one id:
    position rejects), and nothing above y = top (misses)."""
    P, d = centre_rays(cam, width, height)
    P, d = P.astype(np.float64), d.astype(np.float64)
    t_wall = (0.0 - P[2]) / d[..., 2]
    t_slab = (0.4 - P[2]) / d[..., 2]
    slab_x = P[0] + t_slab * d[..., 0]
    on_slab = (slab_x > 0.3) & (slab_x < 0.8)
    t = np.where(on_slab, t_slab, t_wall)
    pos = P[None, None, :] + t[..., None] * d
    g = np.zeros((height, width, 4), F)
    g[..., :3] = pos.astype(F)
    inst = np.where(pos[..., 0] < 0.0, 1, 2).astype(U32)
    hit = (pos[..., 1] <= top) & (t > 0)
    g[..., 3] = np.where(hit, inst, 0).astype(U32).view(F)
    g[~hit, :3] = 0
    return g


def synthetic_frames(width, height, seed=0):
    """(current = (colour, moments, geometry), history = (colour, moments, geometry), history camera, maxHistory, tolerance) with
    every branch of the definition in it; all float32 [H, W, 4]. The two cameras look at the wall of _plane_geometry from the front,
    a small step apart, with a field of view that makes a pixel 0.1 wide on the wall: the tolerance, 0.06 x the distance of 3, is
    0.18 there — more than a pixel's diagonal, less than the slab's step of 0.4."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    aspect = width / height
    fov = 2.0 * np.degrees(np.arctan(0.05 * height / 3.0))
    cam_prev = look_at((-0.25, 0.03, 3.0), (0.0, 0.0, 0.0), fov, aspect)
    cam_now = look_at((0.2, 0.01, 2.9), (0.05, 0.0, 0.0), fov, aspect)
    top = 0.03 * height
    g, hg = _plane_geometry(cam_now, width, height, top), _plane_geometry(cam_prev, width, height, top)

    def frame(n_choices):
        c = rng.gamma(2.0, 0.5, (height, width, 4)).astype(F)
        c[..., 3] = rng.uniform(0.0, 1.0, (height, width)).astype(F)
        m = np.zeros((height, width, 4), F)
        m[..., 0] = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]) * rng.uniform(0.8, 1.25, (height, width)).astype(F)
        m[..., 1] = rng.gamma(2.0, 0.5, (height, width)).astype(F)
        m[..., 2] = rng.choice(np.array(n_choices, F), (height, width))
        m[..., 3] = rng.uniform(-1.0, 1.0, (height, width)).astype(F)  # the fourth word is not read
        return c, m

    cur, mc = frame([1, 4, 4, 4, 8])
    hc, hm = frame([1, 3, 12, 40, 100.5])  # with maxHistory 32: below and above the cap
    flat = lambda a: a.reshape(-1, 4)
    pixels = rng.permutation(width * height)
    special = iter(pixels)
    bad = [np.inf, -np.inf, np.nan]
    for array in (cur, mc, hc, hm):  # inf and NaN in each word of colour, moments and the history's
        for word in range(3):
            for value in bad:
                flat(array)[next(special), word] = value
    for value in (0.0, 0.5, -1.0):  # n < 1 in the frame and in the history
        flat(mc)[next(special), 2] = value
        flat(hm)[next(special), 2] = value
        flat(hm)[next(special), 2] = value
    for _ in range(4):  # surface points behind the previous camera, and one in its plane
        flat(g)[next(special), :3] = (cam_prev[0:3] - cam_prev[9:12] * F(rng.uniform(0.1, 2.0))).astype(F)
    flat(g)[next(special), :3] = cam_prev[0:3]
    for value in bad:  # a position that is not finite, in the frame and in the history
        flat(g)[next(special), 1] = value
        flat(hg)[next(special), 0] = value
    return (cur, mc, g), (hc, hm, hg), cam_prev, 32, 0.06
