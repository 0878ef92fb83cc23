"""-m gpu: vertex updates (twk_update_geometry_vertices). A handle whose geometry got new vertices — in full mode by a rebuild of
everything, in selective mode by a rebuild of what the new vertices change, a bottom-level tree included — must EQUAL a fresh handle
that was given the new vertices through twk_clear_scene ... twk_build: everything tests/test_gpu_selective_update.py compares
(acceleration read-back, scene arrays, build info except its time, every buffer a render leaves), byte for byte, no tolerance.

The scenes are tests/selective_scenes.py's flat, two-level, mixed and single at 33 x 21 and 2 spp, in SAH and LBVH quality. The
deformations are seeded float32 displacements of the sphere (geometry 5) and of the box (4), and the floor (1) with one corner
raised — still a pair by its indices."""
import numpy as np
import pytest

import lifecycle as lc
import selective_scenes as S
from vertex_update_scenes import deformed, with_geometry
from test_gpu_selective_update import QUALITIES, SPP, _assert_same, _device, _everything, _instances, _pictures, _step, app, parts  # noqa: F401  (app, parts: fixtures)

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ["flat", "two-level", "mixed", "single"]
MODES = pytest.mark.parametrize("selective", [True, False], ids=["selective", "full"])


def _geometries(name):
    """The geometries of the scene that a test deforms: the sphere, the box where it has one, the floor where it has walls."""
    used = set(S.instance_geometry(name))
    return [g for g in (S.SPHERE, S.BOX, S.FLOOR) if g in used]


@QUALITIES
@MODES
@pytest.mark.parametrize("name", SCENES)
def test_a_vertex_update_equals_a_fresh_build(twk, orc, app, parts, name, selective, quality):
    """Per deformed geometry of the scene: the updated handle against a fresh one, structure and pictures; updateInfo against the
    plan; the update back against the original build. Once per scene (the first geometry) also in RGBA16F."""
    instance_geometry = S.instance_geometry(name)
    dev = _device(twk, app, parts, name, quality, selective)
    before, _, build = _everything(twk, orc, dev)
    for k, geometry in enumerate(_geometries(name)):
        what = f"{name}, geometry {geometry}, {'selective' if selective else 'full'}"
        new = deformed(parts, geometry)
        dev.updateGeometryVertices(geometry, new)
        assert not dev.geometryDeformed(geometry), what + ": without a temporal history nothing is kept"
        u = dev.updateInfo()
        plan = twk.vertex_update_plan_host(instance_geometry, S.TRIANGLES, S.policy(name), [geometry])
        assert u["selective"] == int(selective) and u["instancesMoved"] == 0 and u["instanceRecordsUploaded"] == 0, what
        if selective:
            assert (u["treesRebuilt"], u["topLevelRebuilt"], u["nodesRequantised"], u["slotsRewritten"]) == \
                (plan["treesRebuilt"], plan["topLevelRebuilt"], plan["nodesRequantised"], plan["slotsRewritten"]), what
            assert u["treesRebuilt"] >= 1 and u["keptBytes"] > 0, what
        else:
            assert u["treesRebuilt"] == build["trees"] and u["keptBytes"] == 0 and u["slotsRewritten"] == build["triangleSlots"], what
        assert u["milliseconds"] > 0.0 and dev.buildInfo()["buildMilliseconds"] == u["milliseconds"], what
        got, _, _ = _everything(twk, orc, dev)
        fresh = _device(twk, app, with_geometry(parts, {geometry: new}), name, quality, False)
        want, _, _ = _everything(twk, orc, fresh)
        fresh.close()
        assert lc.first_difference(want["geometry"], before["geometry"]) is not None, what + ": the deformation shows"
        _assert_same(got, want, what + ": against a fresh handle")
        if k == 0:
            half_dev = _device(twk, app, parts, name, quality, selective, half=True)
            half_dev.updateGeometryVertices(geometry, new)
            half_fresh = _device(twk, app, with_geometry(parts, {geometry: new}), name, quality, False, half=True)
            _assert_same(_pictures(half_dev, True), _pictures(half_fresh, True), what + ": RGBA16F")
            half_dev.close()
            half_fresh.close()
        dev.updateGeometryVertices(geometry, parts[0][geometry][0])
        _assert_same(_everything(twk, orc, dev)[0], before, what + ": after the update back")
    dev.close()


@QUALITIES
@MODES
@pytest.mark.parametrize("name", SCENES)
def test_a_vertex_update_and_a_transform_update_in_both_orders(twk, orc, app, parts, name, selective, quality):
    """The sphere deformed and an instance of it moved, in both orders: each handle equals the fresh one with both."""
    instance = {"flat": 5, "two-level": 5, "mixed": 5, "single": 0}[name]
    moved = _step(_instances(name, parts)[instance][1], (0.05, 0.1, 0.05))
    new = deformed(parts, S.SPHERE, 1)
    fresh = _device(twk, app, with_geometry(parts, {S.SPHERE: new}), name, quality, False, {instance: moved})
    want = _everything(twk, orc, fresh)[0]
    fresh.close()
    for vertices_first in (True, False):
        dev = _device(twk, app, parts, name, quality, selective)
        for step in ((0, 1) if vertices_first else (1, 0)):
            if step == 0:
                dev.updateGeometryVertices(S.SPHERE, new)
            else:
                dev.updateInstanceTransform(instance, moved)
        assert dev.updateInfo()["instancesMoved"] == (0 if not vertices_first else 1)
        _assert_same(_everything(twk, orc, dev)[0], want, f"{name}: {'vertices, then transform' if vertices_first else 'transform, then vertices'}")
        dev.close()


@QUALITIES
@pytest.mark.parametrize("name", ["flat", "two-level"])
def test_refusals(twk, orc, app, parts, name, quality):
    """Each refusal leaves the handle byte-equal to before — acceleration read-back, scene arrays, build info, pictures — in both modes,
    and leaves no update record."""
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE

    def refused(code, f, *words):
        with pytest.raises(twk.TwkError) as e:
            f()
        assert e.value.code == code and "twk_update_geometry_vertices" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    sphere = np.array(parts[0][S.SPHERE][0], F).reshape(-1, 12)
    for selective in (True, False):
        dev = _device(twk, app, parts, name, quality, selective)
        before = _everything(twk, orc, dev)[0]
        refused(VALUE, lambda: dev.updateGeometryVertices(len(S.TRIANGLES), sphere), "bad geometry id")
        refused(VALUE, lambda: dev.updateGeometryVertices(-1, sphere), "bad geometry id")
        refused(VALUE, lambda: dev.updateGeometryVertices(S.SPHERE, sphere[:-1]), "vertices")
        refused(VALUE, lambda: dev.updateGeometryVertices(S.BOX, sphere), "vertices")
        for bad in (np.nan, np.inf):
            broken = sphere.copy()
            broken[3, 1] = bad
            refused(VALUE, lambda: dev.updateGeometryVertices(S.SPHERE, broken), "vertex 3", "finite")
        refused(VALUE, lambda: dev.updateGeometryVertices(S.LIGHT, parts[0][S.LIGHT][0]), "instance 0", "light")
        assert L.lib.twk_update_geometry_vertices(dev.handle, S.SPHERE, None, 0) == VALUE and "NULL attributes" in L.lib.twk_last_error().decode()
        with pytest.raises(twk.TwkError) as e:
            dev.updateInfo()
        assert e.value.code == STATE, "a refused update is no update"
        _assert_same(_everything(twk, orc, dev)[0], before, f"{name}: a refused vertex update changes nothing")
        dev.close()
    unbuilt = twk.Device(ordinal=0, miss=app.info.miss)
    refused(STATE, lambda: unbuilt.updateGeometryVertices(0, sphere), "twk_build")
    unbuilt.close()


@QUALITIES
def test_the_temporal_history_survives_a_vertex_update(twk, app, parts, quality):
    """One frame of the flat scene merged, the sphere deformed, a second frame merged: the own-buffer merge's colour and moments equal
    those of a twin handle in the other mode, byte for byte; and they differ from a handle that dropped its history (a build). The
    sphere is deformed between the update and the merge that swaps the history, and not after it."""
    L = twk._lib
    tp = L.Temporal(maxHistory=32, positionTolerance=0.1)
    new = deformed(parts, S.SPHERE, 2)
    results = []
    for selective, rebuild in ((True, False), (False, False), (False, True)):
        dev = _device(twk, app, parts, "flat", quality, selective)
        for frame in range(2):
            if frame:
                assert not dev.geometryDeformed(S.SPHERE)
                dev.updateGeometryVertices(S.SPHERE, new)
                assert dev.updateInfo()["selective"] == int(selective)
                assert dev.geometryDeformed(S.SPHERE) and not dev.geometryDeformed(S.BOX)
                dev.updateGeometryVertices(S.SPHERE, new)  # a second update keeps the oldest positions: still deformed
                assert dev.geometryDeformed(S.SPHERE)
                if rebuild:
                    dev.build()  # drops the history, and the previous positions with it
                    assert not dev.geometryDeformed(S.SPHERE)
            dev.setSampleOffset(frame * SPP)
            for it in range(SPP):
                dev.render(it)
            dev.renderGeometryMotion()  # the geometry AOV and, for the deformed sphere, the plane the merge then needs
            dev.temporalAccumulate(tp)
            assert not dev.geometryDeformed(S.SPHERE), "the merge swapped the history: previous := current"
        results.append({"colour": lc._words(dev.readTemporal()), "moments": lc._words(dev.readTemporalMoments())})
        dev.close()
    _assert_same(results[0], results[1], "the merge after a selective vertex update against the twin in full mode")
    assert lc.first_difference(results[1]["moments"], results[2]["moments"]) is not None, "the history was kept: a handle that dropped it merges nothing"
