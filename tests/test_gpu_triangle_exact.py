"""-m gpu: the HIP triangle test against exact rational ray-triangle geometry (tests/triangle_exact.py). Every class of that module
is one scene of a hundred fans or pairs (a few hundred triangles), built once per module in three forms - triangle pairs on,
triangle pairs off (TWK_TRIANGLE_PAIRS=0), and as four instances under exact transforms of which two are flattened and two entered -
and traced through the three entry points: twk_trace_rays closest hit, twk_trace_rays any hit, and the persistent kernel with its
pair test (twk_debug_trace_queue). Each answer is held to the exact reference over ALL triangles of the scene: the reported
triangle may be reported and nothing that must be is missed or lies in front of it (on a tie in exact t any triangle of the tie is
right), t, beta and gamma are within K u kappa, the values are no worse than twice a float32 Moeller-Trumbore's on the random
classes, and no kept ray slips through a shared edge or vertex. The inputs are the words the kernels read: the world-space slots
of flattened instances are read back and compared, and the entered instances' inverse transforms are checked to be exact."""
import numpy as np
import pytest

import triangle_exact as X

pytestmark = pytest.mark.gpu

FORMS = ("pairs on", "pairs off", "flattened and entered")
_RUNS = {}


def _device(twk, monkeypatch, pairs):
    if pairs:
        monkeypatch.delenv("TWK_TRIANGLE_PAIRS", raising=False)
    else:
        monkeypatch.setenv("TWK_TRIANGLE_PAIRS", "0")
    st = twk.DeviceState()
    st.resolution[0], st.resolution[1] = 16, 16
    st.tileSize[0], st.tileSize[1] = 8, 8
    st.pathLengths[0], st.pathLengths[1] = 1, 2
    st.distribution, st.samplesSqrt, st.lensShader = 0, 1, 0
    st.epsilonFactor, st.envRotation, st.clockFactor = 500.0, 0.0, 1000.0
    light = twk.LightDefinition()
    light.type, light.area = 0, 12.566371
    light.emission[0] = light.emission[1] = light.emission[2] = 1.0
    m = twk.MaterialGUI()
    m.indexBSDF = 0
    m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.7
    m.absorptionColor[0] = m.absorptionColor[1] = m.absorptionColor[2] = 1.0
    m.absorptionScale, m.ior, m.thinwalled, m.useAlbedoTexture, m.useCutoutTexture = 0.0, 1.5, 0, 0, 0
    m.roughness[0] = m.roughness[1] = 0.1
    dev = twk.Device(ordinal=0, miss=1)
    dev.setState(st)
    dev.initCameras([twk.camera_frustum((0.0, 0.0, 0.0), 0.75, 0.5, 50.0, 6.0, 1.0)])
    dev.initLights([light])
    dev.initMaterials([m])
    return dev


def _run(twk, monkeypatch, name, form):
    """The three entry points' answers on a scene in a form, once per module: dict of (tri [n], tbg [n, 3]) per entry, and the build's info."""
    if (name, form) in _RUNS:
        return _RUNS[(name, form)]
    cs, _ = X.case_set(name)
    dev = _device(twk, monkeypatch, form != "pairs off")
    if form == "flattened and entered":
        parts = X.split_into_instances(cs)
        sizes = [len(p[3]) for p in parts]
        assert max(sizes[:2]) < min(sizes[2:])
        dev.setFlattenPolicy(max(sizes[:2]), 0)   # by triangle count alone: the two small geometries are flattened, the two large ones entered
        for k, (v, i, t, _) in enumerate(parts):
            dev.addGeometry(X.attributes(v), i)
            dev.addInstance(k, t, 0)
        table, transforms = [p[3] for p in parts], [p[2] for p in parts]
    else:
        dev.addGeometry(X.attributes(cs.vertices), cs.indices.astype(np.uint32))
        dev.addInstance(0, X.IDENT, 0)
        table, transforms = [np.arange(len(cs.tris))], [np.asarray(X.IDENT, np.float32)]
    dev.build()
    info = dev.buildInfo()
    _, _, slots, records = dev.readAcceleration()
    slot_primitive, slot_instance = slots[:, 3].view(np.int32), slots[:, 7].view(np.int32)
    tbg, ids = dev.traceRays(cs.rays)
    _, s_ids = dev.traceRays(cs.rays, anyHit=True)
    rec, inst, occ = dev.debugTraceQueue(cs.rays, cs.rays)
    dev.close()

    if form == "flattened and entered":
        assert info["instances"] == 4 and info["flattenedInstances"] == 2, info
        for k in (2, 3):   # entered: the ray is taken into object space by this matrix, which must be the exact inverse
            M = transforms[k].reshape(3, 4).astype(np.float64)
            inverse = M[:, :3].T / (M[0, :3] @ M[0, :3])
            expected = np.concatenate([inverse, -(inverse @ M[:, 3])[:, None]], 1).astype(np.float32)
            assert np.array_equal(records[k, 0:12].reshape(3, 4), expected), (name, k, records[k, 0:12], expected)
        world_instances = (0, 1)
    else:
        assert info["flattenedInstances"] == info["instances"] == 1, info
        world_instances = (0,)
    # the words the kernels read: the world-space slots of flattened instances are the float32 triangles the reference was given
    # (an object-space slot may carry any instance word: each world-space triangle must be found among the slots that name it)
    named = {}
    for s in range(info["triangleSlots"]):
        named.setdefault((int(slot_instance[s]), int(slot_primitive[s])), []).append(s)
    for k in world_instances:
        for prim, t in enumerate(table[k]):
            want = cs.tris[t]   # compared as numbers: the transform turns a -0 coordinate into +0, the same rational
            assert any(np.array_equal(slots[s].reshape(3, 4)[:, :3], want) for s in named.get((k, prim), ())), \
                f"{name}, {form}: no slot holds triangle {prim} of instance {k} as the reference was given it"

    def triangle(instance, primitive):
        out = np.full(len(instance), -1)
        for k, t in enumerate(table):
            sel = instance == k
            out[sel] = t[primitive[sel]]
        return out

    hit = inst >= 0
    q_prim = np.zeros(len(inst), np.int64)
    q_prim[hit] = slot_primitive[rec[hit, 3].view(np.int32)]
    out = {"closest hit": (triangle(ids[:, 0], ids[:, 1]), tbg),
           "any hit": (np.where(s_ids[:, 0] != 0, -2, -1), np.zeros((len(s_ids), 3), np.float32)),
           "persistent kernel": (triangle(inst, q_prim), rec[:, :3]),
           "persistent kernel, any hit": (np.where(occ != 0, -2, -1), np.zeros((len(occ), 3), np.float32)),
           "info": info}
    _RUNS[(name, form)] = out
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(X.MAKERS))
def test_verdict_and_values_against_the_exact_reference(twk, monkeypatch, name, form):
    cs, ref = X.case_set(name)
    run = _run(twk, monkeypatch, name, form)
    if name in ("pair", "dyadic pair") and form == "pairs on":
        assert run["info"]["pairLeaves"] > 0 and run["info"]["pairTriangles"] == 2 * run["info"]["pairLeaves"]
    fails = []
    for entry in ("closest hit", "persistent kernel"):
        tri, tbg = run[entry]
        f, worst = X.check_traversal(cs, ref, tri, tbg, False, f"{name}, {form}, {entry}")
        reported = (tri >= 0).mean()
        print(f"{name}, {form}, {entry}: reported {reported:.1%}; largest error / (K u kappa): t {worst[0]:.3g} beta {worst[1]:.3g} gamma {worst[2]:.3g} (in units of u kappa: {worst.max() * X.K:.3g})")
        assert 0.3 < reported < 0.99
        fails += f
    for entry in ("any hit", "persistent kernel, any hit"):
        tri, tbg = run[entry]
        f, _ = X.check_traversal(cs, ref, tri, tbg, True, f"{name}, {form}, {entry}", values=False)
        assert 0.3 < (tri == -2).mean() < 0.99
        fails += f
    assert not fails, "\n".join(fails[:10])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", X.WATERTIGHT_CLASSES)
def test_no_kept_ray_slips_through_a_shared_edge_or_vertex(twk, monkeypatch, name, form):
    cs, ref = X.case_set(name)
    run = _run(twk, monkeypatch, name, form)
    kept, entry_t = ref.kept(cs)
    assert kept.sum() >= 0.8 * cs.aimed.sum()
    fails = []
    for entry in ("closest hit", "persistent kernel"):
        tri, tbg = run[entry]
        f, worst = X.check_watertight(cs, ref, kept, entry_t, tri, tbg[:, 0], f"{name}, {form}, {entry}")
        print(f"{name}, {form}, {entry}: kept {int(kept.sum())}, slips {sum('slips' in x for x in f)}, largest |t - entry| / bound {worst:.3g}")
        fails += f
    for entry in ("any hit", "persistent kernel, any hit"):   # tmax is out of reach in these classes: a kept ray is occluded
        tri, _ = run[entry]
        fails += [f"{name}, {form}, {entry}: kept ray {i} is not occluded" for i in np.nonzero(kept & (tri != -2))[0]]
    assert not fails, "\n".join(fails[:10])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", X.RANDOM_CLASSES)
def test_values_are_no_worse_than_twice_moller_trumbore(twk, monkeypatch, name, form):
    """On the closest hits that a float32 Moeller-Trumbore accepts as well: the median and the 99.9 % quantile of the device's errors in
    t, beta and gamma are at most twice Moeller-Trumbore's."""
    cs, ref = X.case_set(name)
    run = _run(twk, monkeypatch, name, form)
    for entry in ("closest hit", "persistent kernel"):
        tri, tbg = run[entry]
        rows = np.full(len(tri), -1)
        for i in np.nonzero(tri >= 0)[0]:
            a, b = ref.span[i]
            j = np.nonzero(ref.rows["tri"][a:b] == tri[i])[0]
            if len(j):
                rows[i] = a + j[0]
        sel = np.nonzero(rows >= 0)[0]
        r = ref.rows[rows[sel]]
        mt_hit, mt = X.moller_trumbore(cs.rays[sel, 0:3], cs.rays[sel, 4:7], cs.tris[r["tri"]], cs.rays[sel, 3], cs.rays[sel, 7])
        both = mt_hit & (r["sign"] != 0)
        mine, theirs = X.errors(r[both], tbg[sel][both]), X.errors(r[both], mt[both])
        (m50, m999), (y50, y999) = X.quantiles(mine), X.quantiles(theirs)
        print(f"{name}, {form}, {entry}: {len(mine)} hits; median t / beta / gamma device {m50} Moeller-Trumbore {y50} ratio {m50 / y50}; "
              f"99.9 % device {m999} Moeller-Trumbore {y999} ratio {m999 / y999}")
        assert len(mine) >= 1000
        assert (m50 <= 2 * y50).all() and (m999 <= 2 * y999).all()
