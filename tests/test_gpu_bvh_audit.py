"""-m gpu: every tree twk_build emits, read back (twk_debug_read_acceleration, twk_debug_snapshot_scene) and audited on the host in
float64 by tests/bvh_audit.py — partition, pairs, boxes in both directions, the wide nodes as a cut of the binary tree, their
quantisation in both directions, the two top-of-tree caches, the height and the SAH terms of TwkBuildInfo, the shading records.

One scene per case (bvh_audit_scenes.cases): many geometries side by side, so that one twk_build yields many trees — 19 sizes from 1
to 4097 build primitives as triangle soups and as quad meshes (all pairs; three with a quad that does not pair and a trailing
triangle), and ten distributions at 257 and 1025 primitives. Every case under both build qualities and under two policies: every
geometry entered through one rotated, non-uniformly scaled instance, and every instance flattened (world-space trees, direct-leaf
instances, pair leaves). Then 2000 rays aimed at the geometry through twk_trace_rays and twk_debug_trace_queue against the oracle's
brute force. Also: the selective-update suite's twelve boxes (8-wide root) with and without entered spheres, the two scene files
of test_quantised_boxes_contain_everything_below_them, the forced-middle levels of the SAH level loop, TWK_TOP_CACHE=0, and the
quality relations on the well-behaved meshes. tests/test_bvh_audit_host.py shows on the CPU that the audit passes on reference
trees and catches what it claims to catch. Numbers: profiles/r27_bvh_audit.md."""
import time

import numpy as np
import pytest

import bvh_audit as A
import bvh_audit_scenes as M
import scene_snapshot as snapshot
import selective_scenes as S
from conftest import load_app, scene_path

pytestmark = pytest.mark.gpu

CASES, MESHES = M.cases()
QUALITIES = pytest.mark.parametrize("quality", [1, 0], ids=["sah", "lbvh"])
POLICIES = pytest.mark.parametrize("policy", [(0, 0), M.EVERYTHING_FLAT], ids=["entered", "flattened"])
RAYS = 2000
_results = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _renderers(twk, orc, geometries, instances, policy, quality, oracle=True):
    """A device (and an oracle) on the scene; one diffuse material, one light, a camera nobody looks through."""
    st = twk.DeviceState()
    st.resolution[0], st.resolution[1] = 48, 32
    st.tileSize[0], st.tileSize[1] = 8, 8
    st.pathLengths[0], st.pathLengths[1] = 1, 2
    st.distribution, st.samplesSqrt, st.lensShader = 0, 1, 0
    st.epsilonFactor, st.envRotation, st.clockFactor = 500.0, 0.0, 1000.0
    cam = twk.camera_frustum((0.0, 0.0, 0.0), 0.75, 0.5, 50.0, 6.0, 1.5)
    light = twk.LightDefinition()
    light.type, light.area = 0, 12.566371
    light.emission[0] = light.emission[1] = light.emission[2] = 1.0
    m = twk.MaterialGUI()
    m.indexBSDF = 0
    m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.7
    m.absorptionColor[0] = m.absorptionColor[1] = m.absorptionColor[2] = 1.0
    m.absorptionScale, m.ior, m.thinwalled, m.useAlbedoTexture, m.useCutoutTexture = 0.0, 1.5, 0, 0, 0
    m.roughness[0] = m.roughness[1] = 0.1
    out = []
    for k in range(2 if oracle else 1):
        r = twk.Device(ordinal=0, miss=1) if k == 0 else orc.Oracle(miss=1)
        r.setState(st)
        r.initCameras([cam])
        r.initLights([light])
        r.initMaterials([m])
        if k == 0:
            r.setBuildQuality(quality)
        r.setFlattenPolicy(*policy)
        for a, i in geometries:
            r.addGeometry(a, i)
        for g, t in instances:
            r.addInstance(g, t, 0)
        r.build()
        out.append(r)
    return out


def _aimed_rays(geometries, instances, n, seed):
    """Rays from around the scene at points of its triangles (three in four), the rest beside them."""
    rng = np.random.default_rng(seed)
    targets = []
    for g, t in instances:
        a, i = geometries[g]
        tri = np.asarray(a, np.float64)[np.asarray(i).reshape(-1, 3)][:, :, 0:3]
        pick = rng.integers(0, tri.shape[0], max(1, n // len(instances) + 1))
        w = rng.dirichlet(np.ones(3), pick.size)
        p = (tri[pick] * w[:, :, None]).sum(1)
        m = np.asarray(t, np.float64).reshape(3, 4)
        targets.append(p @ m[:, :3].T + m[:, 3])
    targets = np.concatenate(targets)[rng.permutation(sum(t.shape[0] for t in targets))[:n]]
    scale = np.maximum(1.0, np.abs(targets).max(1, keepdims=True) * 1e-3)
    targets[::4] += rng.normal(0.0, 0.3, targets[::4].shape) * scale[::4]
    d = rng.normal(0.0, 1.0, targets.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = targets - d * rng.uniform(2.0, 6.0, (targets.shape[0], 1)) * scale
    return np.concatenate([o, np.full((n, 1), 1e-4), d, np.full((n, 1), 1e27)], 1).astype(np.float32)


def _trace_against_oracle(dev, ref, rays, slot_primitive, brute=True):
    """twk_trace_rays and twk_debug_trace_queue against the oracle (its brute force, or its own tree where brute force over a scene
    file would take minutes), bit for bit. Returns (wrong, zero_sign): every difference by name — and, apart from those, the rays
    whose ONLY difference is the sign of a zero in t / beta / gamma (+0 against -0), which test_rays_agree_in_the_sign_of_a_zero
    holds on its own."""
    ref.setTraceMode(not brute)
    o_tbg, o_ids = ref.traceRays(rays)
    hit = o_ids[:, 0] >= 0
    assert hit.mean() > 0.3, hit.mean()
    shadow = rays.copy()
    shadow[:, 7] = np.random.default_rng(9).uniform(1.0, 8.0, rays.shape[0]).astype(np.float32)  # ends before, at and beyond the target
    _, s_ids = ref.traceRays(shadow, anyHit=True)
    wrong, zero_sign = [], []

    def name(what, bad, rows, got, want):
        k = bad[0]
        return (f"{what}: {bad.size} of {len(rows)} rays differ, in instances {sorted(set(o_ids[rows[bad], 0].tolist()))[:8]}; first ray {rows[k]} "
                f"(instance {o_ids[rows[k], 0]}, primitive {o_ids[rows[k], 1]}): {np.asarray(got)[k]} against {np.asarray(want)[k]}")

    def same(what, got, want, rows):
        got, want = np.asarray(got).reshape(len(rows), -1), np.asarray(want).reshape(len(rows), -1)
        if got.dtype.kind != "f":
            differs, only_zero = got != want, np.zeros(got.shape, bool)
        else:
            differs = _bits(got) != _bits(want)
            only_zero = differs & (got == 0.0) & (want == 0.0)  # the same value, the other zero
        bad = np.nonzero((differs & ~only_zero).any(1))[0]
        zero = np.nonzero(only_zero.any(1) & ~(differs & ~only_zero).any(1))[0]
        if bad.size:
            wrong.append(name(what, bad, rows, got, want))
        if zero.size:
            zero_sign.append(name(what + ", the sign of a zero only", zero, rows, got, want))

    every, hits = np.arange(rays.shape[0]), np.nonzero(hit)[0]
    g_tbg, g_ids = dev.traceRays(rays)
    same("twk_trace_rays ids", g_ids, o_ids, every)
    same("twk_trace_rays t / beta / gamma", g_tbg[hit], o_tbg[hit], hits)
    same("twk_trace_rays occlusion", dev.traceRays(shadow, anyHit=True)[1][:, 0], s_ids[:, 0], every)
    rec, inst, occ = dev.debugTraceQueue(rays, shadow)
    same("twk_debug_trace_queue instances", inst, o_ids[:, 0], every)
    same("twk_debug_trace_queue primitives", slot_primitive[np.clip(rec[hit, 3].view(np.int32), 0, slot_primitive.size - 1)], o_ids[hit, 1], hits)
    same("twk_debug_trace_queue t / beta / gamma", rec[hit, :3], o_tbg[hit], hits)
    same("twk_debug_trace_queue occlusion", occ, s_ids[:, 0], every)
    return wrong, zero_sign


def _audited(twk, orc, key, geometries, instances, policy, quality, rays=True, top_cache=True):
    """Builds, reads back, audits, traces, closes — once per key; returns what the audit measured, and under "rays" / "zeroSign" what
    _trace_against_oracle found (an AuditError or a build error is raised to whoever asks first and nothing is kept)."""
    if key in _results:
        return _results[key]
    t0 = time.perf_counter()
    made = _renderers(twk, orc, geometries, instances, policy, quality, oracle=rays)
    dev = made[0]
    try:
        t1 = time.perf_counter()
        rb = snapshot.readback(twk, orc, dev)
        t2 = time.perf_counter()
        out = A.audit(A.Scene(geometries, instances, policy, quality, top_cache), rb)
        t3 = time.perf_counter()
        wrong, zero_sign = _trace_against_oracle(dev, made[1], _aimed_rays(geometries, instances, RAYS, 5), rb.slots.view(np.int32)[:, 3]) if rays else ([], [])
        t4 = time.perf_counter()
    finally:
        dev.close()
    out["build"], out["info"], out["rays"], out["zeroSign"] = rb.build, rb.info, wrong, zero_sign
    print(f"{key}: build {1e3 * (t1 - t0):.0f} ms (twk_build {rb.build['buildMilliseconds']:.1f}), read-back {1e3 * (t2 - t1):.0f}, audit {1e3 * (t3 - t2):.0f}, rays {1e3 * (t4 - t3):.0f}; "
          f"{len(out['trees'])} trees, {rb.build['nodes']} nodes, depth {rb.build['maxTraversalDepth']}, root2 {rb.info['root2']}")
    _results[key] = out
    return out


def _case(twk, orc, case, quality, policy):
    geometries = [MESHES[n] for n in CASES[case]]
    instances = [(k, M.place(k)) for k in range(len(geometries))]
    return _audited(twk, orc, (case, quality, policy), geometries, instances, policy, quality)


@POLICIES
@QUALITIES
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_tree_of_the_build_passes_the_audit(twk, orc, case, quality, policy):
    out = _case(twk, orc, case, quality, policy)
    assert len(out["trees"]) == len(CASES[case]) and out["sahDefined"]
    if policy == M.EVERYTHING_FLAT and "quads" in case:
        assert out["build"]["pairLeaves"] > 0


@POLICIES
@QUALITIES
@pytest.mark.parametrize("case", sorted(CASES))
def test_rays_walk_the_audited_trees(twk, orc, case, quality, policy):
    """2000 rays aimed at the geometry through twk_trace_rays (closest and any hit) and twk_debug_trace_queue, against the oracle's
    brute force, bit for bit: ids, t, beta, gamma, occlusion. The kernels walk the audited trees correctly at these sizes too. (The
    sign of a zero coordinate is the next test's.)"""
    out = _case(twk, orc, case, quality, policy)
    assert not out["rays"], "\n".join(out["rays"])


SIGNED_ZERO = ("finding: one ray of 2000 hits triangle 653 of the `far` mesh (coordinates about 1e6, entered through a rotated instance) exactly on an edge, and its "
               "gamma is +0 on the device and -0 in the oracle, in twk_trace_rays and twk_debug_trace_queue alike and under both qualities; every other word of "
               "every ray agrees (test_rays_walk_the_audited_trees). Read from csrc/trace_device.h woopSetup: the device leaves out the exchange of kx and ky for "
               "d[kz] < 0 because every edge function is then the exact negation — which holds for every value but zero (x - x is +0 either way round), so a "
               "vanishing W times the reciprocal of a determinant of the other sign gives the other zero. The trees are not involved. Not fixed here: the fix "
               "belongs to the traversal kernel's triangle test and needs its own measurement")


def _zero_sign_cases():
    for case in sorted(CASES):
        for quality, q in ((1, "sah"), (0, "lbvh")):
            for policy, p in (((0, 0), "entered"), (M.EVERYTHING_FLAT, "flattened")):
                known = case == "distributions-1025" and policy == (0, 0)
                marks = [pytest.mark.xfail(strict=True, raises=ZeroSignDiffers, reason=SIGNED_ZERO)] if known else []
                yield pytest.param(case, quality, policy, id=f"{case}-{q}-{p}", marks=marks)


class ZeroSignDiffers(AssertionError):
    """Raised by the one assertion of test_rays_agree_in_the_sign_of_a_zero, so that its strict xfail expects nothing else."""


@pytest.mark.parametrize("case,quality,policy", list(_zero_sign_cases()))
def test_rays_agree_in_the_sign_of_a_zero(twk, orc, case, quality, policy):
    """Of the same rays: no hit record differs from the oracle's in the sign of a zero t, beta or gamma alone."""
    out = _case(twk, orc, case, quality, policy)
    if out["zeroSign"]:
        raise ZeroSignDiffers("\n".join(out["zeroSign"]))


def test_quality_relations_on_the_well_behaved_meshes(twk, orc):
    """In object space (every geometry entered), where the device builds over the very boxes the reference builds over: the SAH
    tree's inner + leaf cost, recomputed in float64 from the read-back tree, is at most the float64 median split's, at most the
    device's own LBVH tree's, and within the margin of the float64 binned SAH's — three times what float32 against float64 moves
    the reference itself, at least 1 % (bvh_audit_scenes.quality_margin; the code under test has no part in it)."""
    margin = M.quality_margin()
    for n in M.DISTRIBUTION_SIZES:
        case = f"distributions-{n}"
        sah, lbvh = (_case(twk, orc, case, quality, (0, 0)) for quality in (1, 0))
        for name in M.WELL_BEHAVED:
            k = CASES[case].index(f"{name}-{n}")
            c_sah, c_lbvh = (sum(out["trees"][f"geometry {k}"]["sah"]) for out in (sah, lbvh))
            c64, c32, median = M.reference_costs()[f"{name}-{n}"]
            print(f"{name}-{n}: device SAH {c_sah:.4f}, device LBVH {c_lbvh:.4f}, reference binned SAH {c64:.4f} (device / reference {c_sah / c64:.6f}), median split {median:.4f}")
            assert c_sah <= median, f"{name}-{n}: the SAH tree costs {c_sah}, the median split {median}"
            assert c_sah <= c_lbvh, f"{name}-{n}: the SAH tree costs {c_sah}, the LBVH tree {c_lbvh}"
            assert c_sah <= (1.0 + margin) * c64, f"{name}-{n}: the SAH tree costs {c_sah}, the reference's {c64}: more than {margin:.2%} above"


@QUALITIES
def test_forced_middle_levels(twk, orc, quality):
    """57 thin triangles at x = 17^k: the SAH level loop peels one primitive per level and halves the ranges from level 40 on
    (test_bvh_audit_host shows the three pre-conditions on the reference). Audit only, no rays: the coordinates lie outside the range
    the traversal's short divisions are proven for. Flattened through the identity: the tree is the scene and is built over the very
    boxes of the pre-conditions (through a rotation two box extents are about 1e33 and the half-areas of the sweep overflow float32:
    no plane compares cheaper than infinity and every level is cut in the middle — measured: depth 18)."""
    geometries, instances = [M.forced_middle()], [(0, S.affine(1.0, (0.0, 0.0, 0.0)))]
    out = _audited(twk, orc, ("forced-middle", quality), geometries, instances, M.EVERYTHING_FLAT, quality, rays=False)
    assert not out["sahDefined"], "the padded root box's float32 half-area overflows: TwkBuildInfo's terms of this tree are not numbers to compare"
    if quality == 1:
        assert 41 <= out["build"]["maxTraversalDepth"] <= M.stack_height()


@pytest.mark.xfail(strict=True, raises=A.AuditError, reason="finding: padBox's diagonal sqrtf(dx*dx + dy*dy + dz*dz) overflows float32 for a box wider than 1.8e19 "
                   "(sqrt of FLT_MAX) — here the world box of the one instance, 7e33 wide — so the top level's box of the instance is infinite and its "
                   "quantised copy is no box at all; far outside every supported scene, reported in profiles/r27_bvh_audit.md, not fixed")
def test_forced_middle_levels_entered(twk, orc):
    geometries, instances = [M.forced_middle()], [(0, M.place(0))]
    _audited(twk, orc, ("forced-middle-entered", 1), geometries, instances, (0, 0), 1, rays=False)


@pytest.fixture(scope="module")
def cornell(twk):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (33, 21))
    walls = [app.instance(i) for i in (0, 1, 3, 4)]  # light, floor, back wall, left wall: selective_scenes.WALLS
    geometries = [app.geometry(w[0]) for w in walls] + [twk.mesh_box(), twk.mesh_sphere(8, 4, 1.0, np.pi)]
    app.close()
    assert tuple(g[1].size // 3 for g in geometries) == S.TRIANGLES
    return geometries, [(g, w[1]) for g, w in zip(S.WALLS, walls)]


@QUALITIES
@pytest.mark.parametrize("spheres", [0, 3], ids=["many", "many-and-entered-spheres"])
def test_twelve_flattened_boxes_and_the_8_wide_root(twk, orc, cornell, quality, spheres):
    """selective_scenes' "many": four direct-leaf walls and twelve flattened boxes, enough top-level entries for the 8-wide root (with
    the SAH top level); and the same with three entered spheres: a mixed scene."""
    geometries, walls = cornell
    instances = walls + [(g, t) for g, t, _ in S.SCENES["many"][1]] + [(S.SPHERE, S.affine(0.35, at)) for at in S.SPHERE_AT[:spheres]]
    out = _audited(twk, orc, ("many", spheres, quality), geometries, instances, S.policy("many"), quality)
    assert not out["rays"] and not out["zeroSign"], "\n".join(out["rays"] + out["zeroSign"])
    assert out["sahDefined"] and out["build"]["directLeafInstances"] == 4 and out["info"]["twoLevel"] == int(spheres > 0)
    if quality == 1 and spheres == 0:
        assert out["info"]["root2"] >= 0, "the twelve boxes reach the 8-wide root"


@QUALITIES
@pytest.mark.parametrize("scene_file", ["scene_rtigo3_cornell_box.txt", "scene_rtigo3_instances.txt"])
def test_scene_files(twk, orc, scene_file, quality):
    """The two scene files of test_quantised_boxes_contain_everything_below_them under the default flatten policy: the audit, and the
    2000 rays against the oracle's own tree (brute force over these scenes' triangles would take minutes)."""
    system = "\n".join(["resolution 64 40", "tileSize 8 8", "samplesSqrt 1", "miss 0", "light 0", "pathLengths 1 1", "epsilonFactor 500",
                        "lensShader 0", "center 0 1 0", "camera 0.75 0.5 45 3.41"]) + "\n"
    app = twk.Application(system_text=system, scene_text=open(scene_path(scene_file)).read())
    geometries = [app.geometry(k) for k in range(app.info.numGeometries)]
    instances = [(g, t) for g, t, _, _ in app.instances]
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    dev.setBuildQuality(quality)
    app.initDevice(dev)
    try:
        rb = snapshot.readback(twk, orc, dev)
        start = time.perf_counter()
        out = A.audit(A.Scene(geometries, instances, (4, 2), quality), rb)  # TWK_FLATTEN_TRIANGLES, TWK_FLATTEN_REFERENCES
        audited = time.perf_counter()
        ref = orc.Oracle(miss=app.info.miss)
        ref.loadApplication(app)
        wrong, zero_sign = _trace_against_oracle(dev, ref, _aimed_rays(geometries, instances, RAYS, 5), rb.slots.view(np.int32)[:, 3], brute=False)
    finally:
        dev.close()
        app.close()
    print(f"{scene_file}: audit {1e3 * (audited - start):.0f} ms, rays {1e3 * (time.perf_counter() - audited):.0f}, {len(out['trees'])} trees, {rb.build['nodes']} nodes, "
          f"depth {rb.build['maxTraversalDepth']}")
    assert out["sahDefined"]
    assert not wrong and not zero_sign, "\n".join(wrong + zero_sign)


def test_without_the_top_cache_the_root_is_the_plain_root(twk, orc, monkeypatch):
    monkeypatch.setenv("TWK_TOP_CACHE", "0")
    geometries = [MESHES["quads-65"], MESHES["soup-17"]]
    instances = [(0, M.place(0)), (1, M.place(1))]
    out = _audited(twk, orc, ("no-top-cache",), geometries, instances, M.EVERYTHING_FLAT, 1, top_cache=False)
    assert out["sahDefined"] and out["info"]["root2"] < 0
    assert not out["rays"] and not out["zeroSign"], "\n".join(out["rays"] + out["zeroSign"])
