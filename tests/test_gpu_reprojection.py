"""-m gpu: the reprojection chain on the device against float64 scene geometry (tests/reprojection_reference.py; the CPU half is
tests/test_reprojection_host.py, whose scenarios, bounds and judging are used here). The geometry AOV against the reference's trace;
the seven explicit merges looking a coded history up for AOVs the device made itself, read straight from its buffers; the
previous-position plane after each of the four vertex calls and a moved instance against the float64 g'; the own-buffer merge taking
history exactly where the reference has a tap; and three merged frames on a still camera counting as one long render.

Pixels in the exclusion (reprojection_reference.exclusion: the hit or one of its four history taps within 0.02 of an edge in the
surface's own parameters, or fx / fy within 1e-3 of an integer) are left out of the position and the took checks. It is a condition,
not a tolerance, and at most 15 % of a view's hit pixels may fall under it."""

import numpy as np
import pytest

import reprojection_reference as R
import reprojection_scene as S
from reprojection_reference import CARD, HEIGHT, PATCH, U, WALL, WIDTH
from shading_fuzz import feed
from test_gpu_denoise_variance import _small_device, _upload
from test_gpu_half_output import _DeviceBuffer
from test_gpu_vertex_source import _tensor, torch  # noqa: F401  (torch: a fixture)
from reprojection_scene import K_AOV, LAYERS, PLACES, RECTIFY, camera_definition as _camera, judge, motion_table, place_id, plane_bound, report, world

pytestmark = pytest.mark.gpu

F, U32, D = np.float32, np.uint32, np.float64
SPP = 4
FLATTENS = list(S.FLATTEN)
HOWS = ["updateGeometryVertices", "refitGeometryVertices", "updateGeometryVerticesDevice", "refitGeometryVerticesDevice"]


def _device(twk, surfaces, camera_words, flatten, selective=False, area_light=False, far=False):
    scene, state = S.fuzz_scene(surfaces, camera_words, flatten, area_light, far)
    dev = twk.Device(ordinal=0, miss=scene.miss)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    if selective:
        dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE)
    feed(dev, scene, state)
    assert (dev.buildInfo()["flattenedInstances"] > 0) == (flatten == "flattened")
    return dev


def _excluded(w):
    excluded = R.exclusion(w.hits, w.history_hits, w.lookup)
    hit = w.hits.instance >= 0
    assert excluded.sum() <= 0.15 * hit.sum(), "the exclusion's cap"
    return excluded


def _check_aov(what, got, hits, camera):
    """Instance words equal to the reference's outside the edge pixels, positions within G."""
    clear = hits.edge >= R.EDGE
    assert (~clear & (hits.instance >= 0)).sum() <= 0.15 * (hits.instance >= 0).sum()
    word = got[..., 3].view(U32).astype(np.int64) - 1
    wrong = (word != hits.instance) & clear
    assert not wrong.any(), f"{what}: instance words differ from the reference's at (y, x) {np.argwhere(wrong)[:8].tolist()} — a finding about traversal (tools/debug_pixel_mismatch.py)"
    same = word == hits.instance
    error = np.abs(got[..., :3].astype(D) - hits.position).max(axis=-1)
    G = R.bound_G(K_AOV, camera.P, hits.position, hits.cos)
    print(f"{what}: {int((~same).sum())} edge pixels differ in the instance; largest position error {error[same].max():.3e}, largest error / G {(error / G)[same].max():.4f}")
    assert (error[same] <= G[same]).all()
    assert not got[word < 0].any(), "a miss is zero words"
    return same


@pytest.mark.parametrize("flatten", FLATTENS)
@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_the_aov_against_geometry(twk, far, flatten):
    """twk_render_geometry in both views of the scene as the history saw it, and in the current view of the scene with the card moved
    and the patch deformed."""
    w = world(far, "deformed")
    dev = _device(twk, w.previous, w.words_then, flatten)
    dev.renderGeometry()
    _check_aov(f"{place_id(far)}, {flatten}, history view", dev.readGeometry(), w.history_hits, w.then)
    dev.updateCamera(0, _camera(twk, w.words_now))
    dev.renderGeometry()
    still = world(far, "static")
    _check_aov(f"{place_id(far)}, {flatten}, current view", dev.readGeometry(), still.hits, still.now)
    dev.close()
    dev = _device(twk, w.surfaces, w.words_now, flatten)
    dev.renderGeometry()
    _check_aov(f"{place_id(far)}, {flatten}, current view, card moved and patch deformed", dev.readGeometry(), w.hits, w.now)
    dev.close()


# ---- the history's frame, the updates, the current frame: one handle ---------------------------------------------------------------------
def _frame(dev, offset):
    dev.setSampleOffset(offset)
    for it in range(SPP):
        dev.render(it)


def _deform(twk, dev, how, vertices, torch_module):
    records = S.attributes(vertices)
    if how == "updateGeometryVertices":
        dev.updateGeometryVertices(PATCH, records)
    elif how == "refitGeometryVertices":
        dev.refitGeometryVertices(PATCH, records)
    else:
        source = _tensor(torch_module, np.ascontiguousarray(vertices, F))  # positions mode: float32 [n, 3]
        getattr(dev, how)(PATCH, source)
        torch_module.cuda.synchronize()


def _sequence(twk, w, flatten, how=None, torch_module=None, tp=None):
    """One handle through the scenario: a frame at the history's state and camera, merged (the history); then the scenario's updates —
    the patch deformed twice when it deforms (the oldest positions are the history's), the card moved when it moves — and the current
    camera; renderGeometryMotion. Returns (the handle, the history's AOV, the current AOV, the plane), the arrays downloaded."""
    moved, deformed = w.scenario != "static", w.scenario == "deformed"
    dev = _device(twk, w.previous, w.words_then, flatten, selective=how is not None and how != "updateGeometryVertices")
    _frame(dev, 0)
    dev.renderGeometry()
    hg = dev.readGeometry()
    dev.temporalAccumulate(tp if tp is not None else twk._lib.Temporal(maxHistory=32, positionTolerance=R.TOLERANCE))
    if deformed:
        between = (w.previous[PATCH].vertices.astype(D) + np.random.default_rng(31).uniform(-0.05, 0.05, (9, 3))).astype(F)
        _deform(twk, dev, how, between, torch_module)
        _deform(twk, dev, how, w.surfaces[PATCH].vertices, torch_module)
        assert dev.geometryDeformed(PATCH)
    if moved:
        dev.updateInstanceTransform(CARD, w.surfaces[CARD].transform)
    dev.updateCamera(0, _camera(twk, w.words_now))
    dev.renderGeometryMotion()
    dev.synchronizeStream()
    return dev, hg, dev.readGeometry(), dev.readPreviousPositions()


# ---- the kernels on device-made geometry ------------------------------------------------------------------------------------------
def _explicit(twk, merger, w, dev, hg, kernel, half):
    """One explicit merge of the coded history on `merger` (a handle in the output format under test): the current AOV and the plane
    straight from dev's buffers, the history's AOV uploaded as dev wrote it. Returns (verdict's inputs)."""
    L = twk._lib
    hc, hm, cur, mc = R.coded_history(WIDTH, HEIGHT)
    hl, cl = R.coded_layers(WIDTH, HEIGHT, LAYERS)
    if half:
        cur = cur.astype(np.float16)
    g_ptr, g_bytes = dev.geometryDevicePointer()
    assert g_bytes == WIDTH * HEIGHT * 16
    plane_ptr = dev.previousPositionsDevicePointer()[0] if "carried" in kernel else None
    table = motion_table(twk, w)
    shape = (HEIGHT, WIDTH)
    tp, cp, rp = L.Temporal(maxHistory=R.MAX_HISTORY, positionTolerance=R.TOLERANCE), L.Cascade(LAYERS, 1.0, 8.0), L.TemporalRectify(*RECTIFY)
    camera = _camera(twk, w.words_then)
    motion = _DeviceBuffer(twk, table.nbytes)
    motion.upload(table.view(np.uint8))
    if "cascade" in kernel:
        buffers = _upload(twk, (cl, hl, hg))
        out = _DeviceBuffer(twk, cl.nbytes)
        p = [b.ptr.value for b in buffers]
        if kernel == "cascade":
            merger.temporalAccumulateCascade(tp, cp, p[0], g_ptr, p[1], p[2], camera, shape, out.ptr.value)
        elif kernel == "cascade_moving":
            merger.temporalAccumulateCascadeMoving(tp, cp, p[0], g_ptr, p[1], p[2], camera, None, motion.ptr.value, len(table), shape, out.ptr.value)
        else:
            merger.temporalAccumulateCascadeCarried(tp, cp, p[0], g_ptr, p[1], p[2], camera, None, plane_ptr, shape, out.ptr.value)
        merger.synchronizeStream()
        layers = out.download(cl.shape, F)
        for b in buffers + [out, motion]:
            b.free()
        return dict(position_rgb=layers[0], count=layers[0, ..., 3], outputs_and_inputs=[(layers, cl)], constant=1.0)
    buffers = _upload(twk, (cur, mc, hc, hm, hg))
    outs = [_DeviceBuffer(twk, cur.nbytes), _DeviceBuffer(twk, hc.nbytes), _DeviceBuffer(twk, hm.nbytes), _DeviceBuffer(twk, WIDTH * HEIGHT * 4)]
    p, o = [b.ptr.value for b in buffers], [b.ptr.value for b in outs]
    current, history = L.TemporalFrame(p[0], p[1], g_ptr), L.TemporalFrame(p[2], p[3], p[4], camera)
    if kernel == "accumulate":
        merger.temporalAccumulate(tp, current, history, shape, *o[:3])
    elif kernel == "rectified":
        merger.temporalAccumulateRectified(tp, rp, current, history, shape, *o)
    elif kernel in ("moving", "moving_rectified"):
        merger.temporalAccumulateMoving(tp, rp if kernel == "moving_rectified" else None, current, history, motion.ptr.value, len(table), shape, o[0], o[1], o[2],
                                        o[3] if kernel == "moving_rectified" else None)
    else:
        assert kernel == "carried"
        merger.temporalAccumulateCarried(tp, None, current, history, plane_ptr, shape, o[0], o[1], o[2], None)
    merger.synchronizeStream()
    colour, merged, moments = outs[0].download(cur.shape, cur.dtype), outs[1].download(hc.shape, F), outs[2].download(hm.shape, F)
    for b in buffers + outs + [motion]:
        b.free()
    taken = moments[..., 2] > F(1.0)
    if half:  # colourOut is historyOut rounded once where history was taken, the input's bits elsewhere
        with np.errstate(over="ignore"):
            assert np.array_equal(colour.view(np.uint16)[taken], merged.astype(np.float16).view(np.uint16)[taken])
        assert np.array_equal(colour.view(np.uint16)[~taken], cur.view(np.uint16)[~taken])
    else:
        assert np.array_equal(colour.view(U32), merged.view(U32))
    return dict(position_rgb=merged, count=moments[..., 2], outputs_and_inputs=[(merged, cur.astype(F)), (moments, mc)], constant=0.75)


KERNELS = {"static": ("accumulate", "rectified", "cascade"), "moved": ("moving", "moving_rectified", "cascade_moving"), "deformed": ("carried", "cascade_carried")}


@pytest.mark.parametrize("flatten", FLATTENS)
@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_the_kernels_on_device_made_geometry(twk, far, flatten):
    """twk_temporal_accumulate, _rectified and _cascade on the static scene, _moving (plain and rectified) and _cascade_moving on the
    moved card with twk_instance_motion's table, _carried and _cascade_carried on the deformed patch with the plane the device made —
    in both output formats; the geometry is what twk_render_geometry and twk_render_geometry_motion left in the handle's buffers."""
    mergers = {False: _small_device(twk, False), True: _small_device(twk, True)}
    for scenario, kernels in KERNELS.items():
        w = world(far, scenario)
        keep = ~_excluded(w)
        dev, hg, g, plane = _sequence(twk, w, flatten, how="updateGeometryVertices")
        for kernel in kernels:
            for half, merger in mergers.items():
                verdict = judge(w, keep=keep, **_explicit(twk, merger, w, dev, hg, kernel, half))
                report(f"{kernel}, {'rgba16f' if half else 'rgba32f'}, {flatten}", w, verdict)
                assert verdict.ok, (kernel, half)
                assert verdict.full.sum() > 1400 and all((verdict.full & (w.hits.instance == i)).sum() >= 40 for i in (WALL, CARD, PATCH))
        dev.close()
    for merger in mergers.values():
        merger.close()


# ---- the previous-position plane and the own-buffer chain -------------------------------------------------------------------------
def _check_plane(what, w, g, plane):
    same = _check_aov(what + ", AOV", g, w.hits, w.now)
    error = np.abs(plane[..., :3].astype(D) - w.gp).max(axis=-1)
    G = plane_bound(w)
    for i, name in ((CARD, "card"), (PATCH, "patch")):
        on = same & (w.hits.instance == i)
        print(f"{what}, {name}: {int(on.sum())} pixels, largest |g' - g'64| {error[on].max():.3e}, largest error / G {(error / G)[on].max():.4f}")
        assert on.sum() >= 60 and (error[on] <= G[on]).all()
        assert (np.linalg.norm(plane[..., :3].astype(D) - g[..., :3], axis=-1)[on] > 1e-4).all(), "every pixel of it was elsewhere"
    assert np.array_equal(plane[..., 3].view(U32), g[..., 3].view(U32))
    elsewhere = (g[..., 3].view(U32) != CARD + 1) & (g[..., 3].view(U32) != PATCH + 1)
    assert elsewhere.sum() > 1500 and np.array_equal(plane.view(U32)[elsewhere], g.view(U32)[elsewhere]), "everywhere else the plane has the bits of g"


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("flatten", FLATTENS)
@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_the_previous_position_plane(twk, torch, far, flatten, how):  # noqa: F811
    """One frame at the history's state, merged; the patch deformed twice by `how` (a second deformation before the merge must still
    report the positions of the history's frame), the card moved: renderGeometryMotion's plane within G of the float64 g' on the
    patch and on the card, the bits of g everywhere else."""
    w = world(far, "deformed")
    dev, _, g, plane = _sequence(twk, w, flatten, how, torch)
    _check_plane(f"{how}, {place_id(far)}, {flatten}", w, g, plane)
    dev.close()


@pytest.mark.parametrize("scenario,how", [("deformed", how) for how in HOWS] + [("moved", None)], ids=HOWS + ["moved"])
@pytest.mark.parametrize("flatten", FLATTENS)
@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_the_own_buffer_chain(twk, torch, far, flatten, scenario, how):  # noqa: F811
    """The plane's test continued, after each of the four vertex calls, and once with the card moved alone: SPP samples at offset SPP,
    renderGeometryMotion, temporalAccumulate with positionTolerance 0.2. A pixel's merged count exceeds SPP exactly where the reference
    has a tap, outside the exclusion; the merge reports no motion table while the patch is deformed, and without the deformation the
    card's record has twk_instance_motion's bits."""
    L = twk._lib
    w = world(far, scenario)
    tp = L.Temporal(maxHistory=32, positionTolerance=R.TOLERANCE)
    dev, _, g, plane = _sequence(twk, w, flatten, how, torch, tp=tp)
    if scenario == "deformed":
        _check_plane(f"own-buffer chain, {how}, {place_id(far)}, {flatten}", w, g, plane)
    _frame(dev, SPP)
    dev.renderGeometryMotion()
    dev.temporalAccumulate(tp)
    count = dev.readTemporalMoments()[..., 2]
    keep = ~_excluded(w)
    took = count > F(SPP)
    wrong = (took != w.lookup.took) & keep
    print(f"own-buffer chain, {how or scenario}, {place_id(far)}, {flatten}: took {int(took.sum())}, the reference {int(w.lookup.took.sum())}, differing outside the exclusion {int(wrong.sum())}")
    assert not wrong.any(), np.argwhere(wrong)[:8].tolist()
    assert (np.abs(count[keep].astype(D) - np.where(took[keep], 2 * SPP, SPP)) <= 48 * U * 2 * SPP).all() and w.lookup.took[keep].sum() > 1500
    table = dev.readTemporalMotion()
    if scenario == "deformed":
        assert len(table) == 0 and not dev.geometryDeformed(PATCH)
    else:
        assert len(table) == len(w.surfaces)
        assert bytes(table[CARD]) == bytes(twk.instance_motion(w.previous[CARD].transform, w.surfaces[CARD].transform)) and table[CARD].moved == 1
        assert table[WALL].moved == 0 and table[PATCH].moved == 0
    dev.close()


# ---- counting on a still camera ----------------------------------------------------------------------------------------------------
def _window_max(a):
    """The largest value in each pixel's 3 x 3 window, [H, W]."""
    p = np.pad(a, 1, mode="edge")
    return np.max([p[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(3) for dx in range(3)], axis=0)


def _three_frames(twk, w, flatten, offsets):
    dev = _device(twk, w.surfaces, w.words_now, flatten, area_light=True, far=w.far)
    for offset in offsets:
        _frame(dev, offset)
        dev.renderGeometry()
        dev.temporalAccumulate()  # the defaults: maxHistory 32 is large enough for 12 samples
    out = dev.readTemporal(), dev.readTemporalMoments(), dev.readGeometry()
    dev.close()
    return out


@pytest.mark.parametrize("flatten", FLATTENS)
@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_three_merged_frames_count_as_one_long_render(twk, far, flatten):
    """F = 3 frames of 4 samples at sample offsets 0, 4 and 8 on a still camera, merged after each, against one handle that rendered
    iterations 0 to 11 (the same random numbers, by twk_set_sample_offset's contract). On every hit pixel n = 12 to 48 u; with M_p the
    largest magnitude of the quantity in the long render's 3 x 3 window (for M2: of the luminance mean) colour and mean agree within
    (16 F u + 2 B_p) M_p and M2 within (32 F u + 2 B_p) n M_p^2 — B_p, the lookup's
    position bound, is what a neighbour can leak through the bilinear weights. Control: with all three offsets 0 more than half of the
    non-emissive hit pixels violate the colour bound."""
    frames = 3
    w = world(far, "static")
    colour, moments, g = _three_frames(twk, w, flatten, (0, SPP, 2 * SPP))
    long = _device(twk, w.surfaces, w.words_now, flatten, area_light=True, far=w.far)
    for it in range(frames * SPP):
        long.render(it)
    want_colour, want_moments = long.getOutputBufferHost().astype(D), long.readMoments().astype(D)
    long.close()
    word = g[..., 3].view(U32)
    hit = word != 0
    surface = hit & (word <= len(w.surfaces))  # not the light's instance
    lookup = R.expected_lookup(w.hits.position, w.hits.instance, w.now, w.hits.instance)
    B = R.bound_B(w.hits.position, w.now, lookup, WIDTH, HEIGHT)
    assert np.isfinite(B).all() and lookup.took.all()
    n = frames * SPP
    assert hit.sum() > 2000 and (np.abs(moments[..., 2][hit].astype(D) - n) <= 48 * U * n).all(), "n = 12 on every hit pixel"
    assert (want_moments[..., 2][hit] == n).all()
    c_bound = (16 * frames * U + 2 * B) * _window_max(np.abs(want_colour[..., :3]).max(axis=-1))
    c_error = np.abs(colour[..., :3].astype(D) - want_colour[..., :3]).max(axis=-1)
    m_bound = (16 * frames * U + 2 * B) * _window_max(np.abs(want_moments[..., 0]))
    m_error = np.abs(moments[..., 0].astype(D) - want_moments[..., 0])
    v_bound = (32 * frames * U + 2 * B) * n * _window_max(np.abs(want_moments[..., 0])) ** 2
    v_error = np.abs(moments[..., 1].astype(D) - want_moments[..., 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, error, bound in (("colour", c_error, c_bound), ("mean", m_error, m_bound), ("M2", v_error, v_bound)):
            ratio = np.where(hit & (bound > 0), error / bound, 0.0)
            print(f"still camera, {place_id(far)}, {flatten}: {name}: largest error / bound {ratio.max():.4f}, pixels beyond {(hit & (error > bound)).sum()}")
    assert (c_error[hit] <= c_bound[hit]).all() and (m_error[hit] <= m_bound[hit]).all() and (v_error[hit] <= v_bound[hit]).all()
    assert (want_colour[..., :3][surface].max(axis=-1) > 0).mean() > 0.9, "the light reaches the surfaces"
    # control: the same random numbers in all three frames
    same_colour, _, _ = _three_frames(twk, w, flatten, (0, 0, 0))
    beyond = np.abs(same_colour[..., :3].astype(D) - want_colour[..., :3]).max(axis=-1) > c_bound
    print(f"control, offsets 0, 0, 0: {beyond[surface].mean():.1%} of the non-emissive hit pixels beyond the colour bound")
    assert beyond[surface].mean() > 0.5
