"""-m gpu: triangle pairs (device_types.h "triangle pairs"). The two halves of a quad are one primitive of the build and are tested
by the persistent traversal kernel as one four-vertex record. On small scenes — a single quad, a 2 x 2 plane, `sphere 8 4`, a
box, and a three-triangle mesh whose third triangle pairs with nothing — the persistent kernel (twk_debug_trace_queue) equals the
single-ray traversal over the binary nodes and the slots (twk_trace_rays) bit for bit, on random rays and on rays aimed at
vertices, edge midpoints and the quads' diagonals, closest hit and any hit; pairs on and pairs off (TWK_TRIANGLE_PAIRS=0) give
the same records; and the build reports the pairs it made. Images of the Cornell box and of a two-level scene are the oracle's
bit for bit with pairs on and off."""
import numpy as np
import pytest

from conftest import load_app

pytestmark = pytest.mark.gpu

IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _attrs(verts):
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    a = np.zeros((verts.shape[0], 12), np.float32)
    a[:, 0:3] = verts
    a[:, 3] = 1.0
    a[:, 8] = 1.0
    a[:, 9:11] = verts[:, 0:2]
    return a


def _state(twk):
    st = twk.DeviceState()
    st.resolution[0], st.resolution[1] = 16, 16
    st.tileSize[0], st.tileSize[1] = 8, 8
    st.pathLengths[0], st.pathLengths[1] = 1, 2
    st.distribution, st.samplesSqrt, st.lensShader = 0, 1, 0
    st.epsilonFactor, st.envRotation, st.clockFactor = 500.0, 0.0, 1000.0
    return st


def _material(twk):
    m = twk.MaterialGUI()
    m.indexBSDF = 0
    m.albedo[0], m.albedo[1], m.albedo[2] = 0.7, 0.6, 0.5
    m.absorptionColor[0] = m.absorptionColor[1] = m.absorptionColor[2] = 1.0
    m.absorptionScale, m.ior, m.thinwalled = 0.0, 1.5, 0
    m.useAlbedoTexture = m.useCutoutTexture = 0
    m.roughness[0] = m.roughness[1] = 0.1
    return m


FLOOR = [3, 0, 0, 0, 0, 1, 0, -1.5, 0, 0, 3, 0]   # a 6 x 6 quad below the mesh
TILTED = [1, 0.25, 0, 0.5, -0.25, 1, 0.5, 0.25, 0, -0.5, 1, -0.25]  # no vertex keeps a round coordinate


def _scenes(twk):
    """name -> (geometries, instances (geometry, transform), pair leaves the build must report)"""
    three = (_attrs([(0, 0, 0), (2, 0, 0.5), (2, 2, 0), (0, 2, 0.5), (3, 3, 1)]), np.array([0, 1, 2, 2, 3, 0, 2, 1, 4], np.uint32))
    odd_first = (_attrs([(0, 0, 0), (2, 0, 0.5), (2, 2, 0), (0, 2, 0.5), (3, 3, 1)]), np.array([2, 1, 4, 0, 1, 2, 2, 3, 0], np.uint32))
    plane1, plane2 = twk.mesh_plane(1, 1, 1), twk.mesh_plane(2, 2, 1)
    return {
        "single quad": ([plane1], [(0, TILTED)], 1),
        "plane 2x2": ([plane2], [(0, TILTED)], 4),
        "sphere 8 4": ([twk.mesh_sphere(8, 4, 1.0, np.pi), plane1], [(0, TILTED), (1, FLOOR)], 8 * 3 + 1),  # tessV = 4 rings: three bands of eight quads, the pole bands included
        "box": ([twk.mesh_box(), plane1], [(0, TILTED), (1, FLOOR)], 6 + 1),
        "three triangles": ([three], [(0, TILTED)], 1),
        # the matching couple is triangles 1, 2 — not 2k, 2k + 1: no pair
        "three triangles, couple at an odd primitive": ([odd_first], [(0, TILTED)], 0),
    }


def _device(twk, monkeypatch, geometries, instances, pairs):
    if pairs:
        monkeypatch.delenv("TWK_TRIANGLE_PAIRS", raising=False)
    else:
        monkeypatch.setenv("TWK_TRIANGLE_PAIRS", "0")
    dev = twk.Device(ordinal=0, miss=1)
    light = twk.LightDefinition()
    light.type = 0
    light.area = 12.566371
    light.emission[0] = light.emission[1] = light.emission[2] = 1.0
    dev.setState(_state(twk))
    dev.initCameras([twk.camera_frustum((0.0, 0.0, 0.0), 0.75, 0.5, 50.0, 6.0, 1.0)])
    dev.initLights([light])
    dev.initMaterials([_material(twk)])
    for a, i in geometries:
        dev.addGeometry(a, i)
    for g, t in instances:
        dev.addInstance(g, t, 0)
    dev.build()
    return dev


def _rays(tris):
    """[n, 8] rays for a scene whose world-space triangle slots are `tris` [m, 12]: 4 096 random ones, and from five origins one at
    every vertex, every edge midpoint and the midpoint of every quad diagonal candidate (the edge p0 p2 of a slot)."""
    rng = np.random.default_rng(58)
    v = tris.reshape(-1, 3, 4)[:, :, :3]
    lo, hi = v.reshape(-1, 3).min(axis=0) - 2.0, v.reshape(-1, 3).max(axis=0) + 2.0
    n = 4096
    o = rng.uniform(lo, hi, (n, 3))
    w = rng.dirichlet(np.ones(3), n)
    target = (v[rng.integers(0, v.shape[0], n)] * w[:, :, None]).sum(axis=1)
    target[::5] = rng.uniform(lo, hi, (target[::5].shape[0], 3))
    rays = [np.concatenate([o, target - o], 1)]
    points = np.concatenate([v.reshape(-1, 3), (v[:, 0] + v[:, 1]) / 2, (v[:, 1] + v[:, 2]) / 2, (v[:, 2] + v[:, 0]) / 2])
    for origin in ((0.3, 4.0, 0.2), (-3.0, 0.5, 2.5), (2.5, -4.0, -1.0), (0.1, 0.2, 6.0), (5.0, 0.4, 0.3)):
        oo = np.broadcast_to(np.asarray(origin), points.shape)
        rays.append(np.concatenate([oo, points - oo], 1))
    r = np.concatenate(rays).astype(np.float32)
    out = np.zeros((r.shape[0], 8), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = r[:, 0:3], 0.0, r[:, 3:6], 1e27
    return out


@pytest.mark.parametrize("name", ["single quad", "plane 2x2", "sphere 8 4", "box", "three triangles", "three triangles, couple at an odd primitive"])
def test_pair_leaves_against_the_single_ray_traversal(twk, monkeypatch, name):
    geometries, instances, expected_pairs = _scenes(twk)[name]
    records = []
    for pairs in (True, False):
        dev = _device(twk, monkeypatch, geometries, instances, pairs)
        info = dev.buildInfo()
        assert info["pairLeaves"] == (expected_pairs if pairs else 0) and info["pairTriangles"] == 2 * info["pairLeaves"], (name, pairs, info)
        assert info["flattenedInstances"] == info["instances"]  # the builds that test pair leaves: every instance flattened
        _, _, tris, _ = dev.readAcceleration()
        slot_primitive = tris[:, 3].view(np.int32)
        closest = _rays(tris) if not records else records[0][0]
        shadow = closest.copy()
        shadow[:, 7] = np.random.default_rng(3).uniform(0.3, 1.5, shadow.shape[0]).astype(np.float32)  # d is origin -> target: ends before, at and beyond it
        rec, inst, occ = dev.debugTraceQueue(closest, shadow)
        q_tbg, q_ids = dev.traceRays(closest)
        _, s_ids = dev.traceRays(shadow, anyHit=True)
        dev.close()
        hit = q_ids[:, 0] >= 0
        assert 0.2 < hit.mean() < 0.999, hit.mean()
        assert np.array_equal(inst, q_ids[:, 0]), f"{name}: {(inst != q_ids[:, 0]).sum()} instances differ"
        prim = slot_primitive[rec[hit, 3].view(np.int32)]
        assert np.array_equal(prim, q_ids[hit, 1]), f"{name}: {(prim != q_ids[hit, 1]).sum()} primitives differ"
        assert np.array_equal(_bits(rec[hit, :3]), _bits(q_tbg[hit])), f"{name}: t / beta / gamma differ"
        assert np.array_equal(occ, s_ids[:, 0]), f"{name}: {(occ != s_ids[:, 0]).sum()} occlusion flags differ"
        assert 0.02 < occ.mean() < 0.98
        records.append((closest, _bits(rec[:, :3])[hit], inst, prim, occ))
    on, off = records
    for k in range(1, 5):
        assert np.array_equal(on[k], off[k]), f"{name}: pairs on and off differ in {('t / beta / gamma', 'instance', 'primitive', 'occlusion')[k - 1]}"


_ORACLE_IMAGES = {}


def _oracle_image(orc, app, key, iterations):
    if key not in _ORACLE_IMAGES:
        ref = orc.Oracle(miss=app.info.miss)
        ref.loadApplication(app)
        for it in range(iterations):
            ref.render(it)
        _ORACLE_IMAGES[key] = ref.getOutputBufferHost()
    return _ORACLE_IMAGES[key]


@pytest.mark.parametrize("system,scene,resolution,two_level", [
    ("system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (96, 64), False),
    ("system_rtigo3_instances.txt", "scene_rtigo3_instances.txt", (48, 32), True),
])
def test_images_with_pairs_on_and_off_equal_the_oracle(twk, orc, monkeypatch, system, scene, resolution, two_level):
    iterations = 4
    app = load_app(twk, system, scene, resolution)
    cpu = _oracle_image(orc, app, scene, iterations)
    for pairs in ("1", "0"):
        monkeypatch.setenv("TWK_TRIANGLE_PAIRS", pairs)
        dev = twk.Device(ordinal=0, miss=app.info.miss)
        app.initDevice(dev)
        info = dev.buildInfo()
        assert (info["flattenedInstances"] < info["instances"]) == two_level
        assert (info["pairLeaves"] > 0) == (pairs == "1") and info["pairTriangles"] == 2 * info["pairLeaves"]
        if pairs == "1" and not two_level:
            assert info["pairTriangles"] == info["triangleSlots"]  # every mesh of the Cornell box is made of quads: all of it pairs
        for it in range(iterations):
            dev.render(it)
        dev.synchronizeStream()
        gpu = dev.getOutputBufferHost()
        dev.close()
        mism = (_bits(gpu) != _bits(cpu)).any(axis=2).sum()
        assert mism == 0, f"pairs {pairs}: {mism} of {resolution[0] * resolution[1]} pixels differ from the oracle"
