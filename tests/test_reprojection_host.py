"""CPU: the reprojection chain against float64 scene geometry (tests/reprojection_reference.py, which shares no formula with csrc/).
The host forms of the merges — twk_temporal_moving_host plain and rectified, twk_temporal_cascade_moving_host,
twk_temporal_carried_host, twk_temporal_cascade_carried_host — look a coded history up for the reference's geometry AOVs rounded to
float32; what they hand back is the position they looked up, which must lie within B of the reference's projection of the float64
previous position, and they must take history exactly where the reference says a tap of the same instance exists.
twk_instance_motion is held to the float64 M_prev inv(M_cur), twk_previous_positions_host to the float64 g'. Four negative controls —
slips applied to the REFERENCE — must each fail by at least 10 B on 90 % of the pixels they affect. No GPU needed."""
import types

import numpy as np
import pytest

import reprojection_reference as R
import reprojection_scene as S
from reprojection_reference import CARD, HEIGHT, PATCH, WALL, WIDTH
from reprojection_scene import K_AOV, LAYERS, PLACES, RECTIFY, SCENARIOS, judge, motion_table, place_id, plane_bound, report, world
from test_temporal_carry_host import host_carried, host_cascade_carried
from test_temporal_motion_host import host_cascade_moving, host_moving

F, U32, D = np.float32, np.uint32, np.float64


def plain_merge(twk, w, table=None, rectify=None, plane=None):
    """The plain (or rectified) merge of the coded history through twk_temporal_moving_host, or twk_temporal_carried_host with a plane."""
    hc, hm, cur, mc = R.coded_history(WIDTH, HEIGHT)
    if plane is not None:
        colour, moments, _ = host_carried(twk, rectify, cur, mc, w.g, (hc, hm, w.hg), w.words_then, R.MAX_HISTORY, R.TOLERANCE, plane)
    else:
        colour, moments, _ = host_moving(twk, rectify, cur, mc, w.g, (hc, hm, w.hg), w.words_then, R.MAX_HISTORY, R.TOLERANCE, table, 0 if table is None else len(table))
    return colour, moments, cur, mc


def judge_plain(w, merged, **more):
    colour, moments, cur, mc = merged
    return judge(w, colour, moments[..., 2], [(colour, cur), (moments, mc)], constant=0.75, **more)


def cascade_merge(twk, w, table=None, plane=None):
    hl, cl = R.coded_layers(WIDTH, HEIGHT, LAYERS)
    if plane is not None:
        out = host_cascade_carried(twk, cl, w.g, (hl, w.hg), w.words_then, R.MAX_HISTORY, R.TOLERANCE, None, plane)
    else:
        out = host_cascade_moving(twk, cl, w.g, (hl, w.hg), w.words_then, R.MAX_HISTORY, R.TOLERANCE, None, table, 0 if table is None else len(table))
    return out, cl


def judge_cascade(w, merged, **more):
    out, cl = merged
    return judge(w, out[0], out[0, ..., 3], [(out, cl)], constant=1.0, **more)


def control(w, merged, judge_merged, lookup, affected):
    """A negative control: `lookup` is the expectation of a reference with a slip in it. The merge must fail against it, and at least
    90 % of the affected pixels that are `full` by the true reference must lie at least 10 B off."""
    verdict = judge_merged(w, merged, lookup=lookup)
    assert not verdict.ok, "a reference with a slip in it is satisfied: the test shows nothing"
    x, y, _ = R.decode(merged[0][0] if merged[0].ndim == 4 else merged[0])
    pixels = w.lookup.full & affected & np.isfinite(lookup.fx) & np.isfinite(lookup.fy)
    off = np.maximum(np.abs(x - lookup.fx), np.abs(y - lookup.fy))[pixels] >= 10.0 * w.B[pixels]
    assert pixels.sum() >= 50 and off.mean() >= 0.9, f"only {off.mean():.2%} of {pixels.sum()} affected pixels lie 10 B off"
    return float(off.mean()), float(np.maximum(np.abs(x - lookup.fx), np.abs(y - lookup.fy))[pixels].min())


# ---- twk_instance_motion -------------------------------------------------------------------------------------------------------------
def _pairs():
    card_then, card_now = R.scene()[CARD].transform, R.scene(card_moved=True)[CARD].transform
    identity = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    turn = np.concatenate([R._rotation((0.3, -1.0, 0.5), 37.0), [[0.5], [-2.0], [1.5]]], axis=1).astype(F).reshape(12)
    scale = np.array([100, 0, 0, 1, 0, 1, 0, -2, 0, 0, 0.01, 3], F)
    mirror = np.array([-1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, -0.5], F)
    shift = identity.copy()
    shift[[3, 7, 11]] = (1.0e4, -1.0e4, 3333.0)
    return {"rotation": (identity, turn), "rotation to rotation": (turn, (R.to4(turn) @ R.to4(turn))[:3].astype(F).reshape(12)), "scale (100, 1, 0.01)": (turn, scale),
            "mirror": (turn, mirror), "translation 1e4": (turn, shift), "the scene's move": (card_then, card_now), "the scene's move, far": (R.scene(True)[CARD].transform, R.scene(True, True)[CARD].transform)}


@pytest.mark.parametrize("name", list(_pairs()))
def test_instance_motion_is_previous_times_the_inverse_of_current(twk, name):
    """Every element of X within 1 float32 ulp of the float64 M_prev inv(M_cur). The header computes in double and rounds once; with
    condition numbers of the 3 x 3 part up to 1e4 the double error stays far below half an ulp."""
    previous, current = _pairs()[name]
    record = twk.instance_motion(previous, current)
    assert record.moved == 1
    got = np.array(list(record.previousFromCurrent), D).reshape(3, 4)
    want = R.instance_motion(previous, current)[:3]
    ulp = np.spacing(np.abs(want).astype(F)).astype(D)
    worst = np.abs(got - want) / ulp
    print(f"{name}: condition {np.linalg.cond(R.to4(current)):.3g}, largest |X - X64| {worst.max():.3f} ulp")
    assert (worst <= 1.0).all(), (got, want)
    assert np.allclose(want @ R.to4(current), R.to4(previous)[:3], rtol=0, atol=1e-9 * np.abs(R.to4(previous)).max()), "the reference: X M_cur = M_prev"


def test_instance_motion_unmoved_and_singular(twk):
    for previous, current in _pairs().values():
        for m in (previous, current):
            assert twk.instance_motion(m, m.copy()).moved == 0, "bit-equal matrices: moved = 0"
    singular = np.array([1, 2, 3, 0, 2, 4, 6, 1, 0, 1, 0, 2], F)
    assert abs(np.linalg.det(R.to4(singular))) < 1e-12
    with pytest.raises(twk.TwkError):
        twk.instance_motion(_pairs()["rotation"][1], singular)


# ---- the merges ----------------------------------------------------------------------------------------------------------------------
def test_the_scene_is_what_the_checks_need():
    """Both views see the three instances without a miss; the patch overlaps neither the card nor the picture's edge in either view;
    the scenarios change what they say they change; and the exclusion the GPU tests use stays below its cap of 15 %."""
    for far in PLACES:
        for scenario in SCENARIOS:
            w = world(far, scenario)
            for hits in (w.hits, w.history_hits):
                assert (hits.instance >= 0).all() and all((hits.instance == i).sum() >= 60 for i in (WALL, CARD, PATCH))
                ys, xs = np.nonzero(hits.instance == PATCH)
                assert xs.min() > 0 and xs.max() < WIDTH - 1 and ys.min() > 0 and ys.max() < HEIGHT - 1
                near = np.zeros_like(hits.instance, bool)
                near[:, 1:] |= hits.instance[:, :-1] == CARD
                near[:, :-1] |= hits.instance[:, 1:] == CARD
                assert not (near & (hits.instance == PATCH)).any()
            excluded = R.exclusion(w.hits, w.history_hits, w.lookup)
            assert excluded.sum() <= 0.15 * (w.hits.instance >= 0).sum()
            assert w.lookup.full.sum() > 1500 and all((w.lookup.full & (w.hits.instance == i)).sum() >= 50 for i in (WALL, CARD, PATCH))
            moved = np.linalg.norm(w.gp - w.hits.position, axis=-1)
            assert (moved[w.hits.instance == WALL] == 0).all()
            assert (moved[w.hits.instance == CARD] > 0.05).all() == (scenario != "static") and (moved[w.hits.instance == PATCH] > 1e-4).all() == (scenario == "deformed")
    covered = world(False, "moved")
    was_card = np.stack([covered.history_hits.instance[qy, qx] == CARD for qy, qx, _ in covered.lookup.taps]).all(axis=0)
    assert (was_card & (covered.hits.instance == WALL)).sum() >= 5, "wall pixels that the card used to cover"


@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_static_scene_moved_camera(twk, far):
    """The plain merge without a table, the rectified merge, and the cascade's: the lookup on every full pixel within B, history taken
    exactly where the reference has a tap, every other pixel passed through."""
    w = world(far, "static")
    plain = plain_merge(twk, w)
    verdict = judge_plain(w, plain)
    report("plain", w, verdict)
    assert verdict.ok
    rectified = plain_merge(twk, w, rectify=RECTIFY)
    verdict_r = judge_plain(w, rectified)
    report("rectified", w, verdict_r)
    assert verdict_r.ok and np.array_equal(verdict_r.taken, verdict.taken)
    assert np.array_equal(rectified[0].view(U32)[verdict.taken], plain[0].view(U32)[verdict.taken]), "the rectified merge has the plain merge's position"
    cascade = cascade_merge(twk, w)
    verdict_c = judge_cascade(w, cascade)
    report("cascade", w, verdict_c)
    assert verdict_c.ok
    # negative controls: pixel centres taken at i, and U and V exchanged
    everywhere = np.ones((HEIGHT, WIDTH), bool)
    for name, camera in (("pixel centres at i", R.Camera(w.words_then, centre=0.0)), ("U and V exchanged", R.Camera(w.words_then, swap=True))):
        slipped = R.expected_lookup(w.gp, w.hits.instance, camera, w.history_hits.instance)
        share, least = control(w, plain, judge_plain, slipped, everywhere)
        print(f"control, {name}: {share:.1%} of the full pixels at least 10 B off, the least {least:.3f} px")
        control(w, cascade, judge_cascade, slipped, everywhere)


def test_a_point_behind_the_history_camera_and_a_miss_pass_through(twk):
    """The history camera turned round (every surface point has s2 <= 0) takes no history anywhere; and misses — a current camera that
    looks past the wall's edge — pass through with every pixel beyond the history's picture."""
    w = world(False, "static")
    hc, hm, cur, mc = R.coded_history(WIDTH, HEIGHT)
    away = w.words_then.copy()
    away[3:6], away[9:12] = -away[3:6], -away[9:12]
    assert (R.Camera(away).project(w.gp, WIDTH, HEIGHT)[2] < 0).all()
    colour, moments, _ = host_moving(twk, None, cur, mc, w.g, (hc, hm, w.hg), away, R.MAX_HISTORY, R.TOLERANCE, None, 0)
    assert np.array_equal(colour.view(U32), cur.view(U32)) and np.array_equal(moments.view(U32), mc.view(U32))
    from temporal_restate import look_at
    side = R.Camera(look_at((3.5, 0.4, 4.0), (3.6, 0.0, 0.0), R.FOV, WIDTH / HEIGHT))
    hits = R.trace(w.surfaces, *side.rays(WIDTH, HEIGHT))
    assert (hits.instance < 0).sum() > 100 and (hits.instance == WALL).sum() > 100
    lookup = R.expected_lookup(hits.position, hits.instance, w.then, w.history_hits.instance)
    colour, moments, _ = host_moving(twk, None, cur, mc, R.aov(hits), (hc, hm, w.hg), w.words_then, R.MAX_HISTORY, R.TOLERANCE, None, 0)
    seen = types.SimpleNamespace(lookup=lookup, B=R.bound_B(hits.position, w.then, lookup, WIDTH, HEIGHT), far=False, scenario="side view")
    verdict = judge(seen, colour, moments[..., 2], [(colour, cur), (moments, mc)], constant=0.75)
    report("plain", seen, verdict)
    assert verdict.ok and lookup.took.sum() > 100 and (~lookup.took & (hits.instance >= 0)).sum() > 20
    assert not verdict.taken[hits.instance < 0].any()


@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_moved_card(twk, far):
    """The card turned, stretched and shifted between the frames, with the table from twk_instance_motion: its pixels are looked up at
    X64 g projected, and the wall pixels the card used to cover take no history."""
    w = world(far, "moved")
    table = motion_table(twk, w)
    assert table["moved"].tolist() == [0, 1, 0]
    plain = plain_merge(twk, w, table)
    verdict = judge_plain(w, plain)
    report("plain", w, verdict)
    assert verdict.ok
    on_card = w.hits.instance == CARD
    assert (verdict.full & on_card).sum() >= 100
    was_card = np.stack([w.history_hits.instance[qy, qx] == CARD for qy, qx, _ in w.lookup.taps]).all(axis=0)
    assert not verdict.taken[was_card & (w.hits.instance == WALL)].any()
    rectified = plain_merge(twk, w, table, rectify=RECTIFY)
    verdict_r = judge_plain(w, rectified)
    report("rectified", w, verdict_r)
    assert verdict_r.ok and np.array_equal(rectified[0].view(U32)[verdict.taken], plain[0].view(U32)[verdict.taken])
    cascade = cascade_merge(twk, w, table)
    verdict_c = judge_cascade(w, cascade)
    report("cascade", w, verdict_c)
    assert verdict_c.ok
    # without the table the card's pixels are looked up where the card is now: the reference notices
    assert not judge_plain(w, plain_merge(twk, w)).ok
    # negative control: X inverted
    slipped = R.expected_lookup(R.previous_positions(w.hits, w.surfaces, w.previous, invert=True), w.hits.instance, w.then, w.history_hits.instance)
    share, least = control(w, plain, judge_plain, slipped, on_card)
    print(f"control, X inverted: {share:.1%} of the card's full pixels at least 10 B off, the least {least:.3f} px")
    control(w, cascade, judge_cascade, slipped, on_card)


def carry_inputs(twk, w):
    """What twk_previous_positions_host takes, restated from the reference's hits: (hits (t, beta, gamma), instance, primitive, g,
    indices, previous positions, motion, carry)."""
    from temporal_carry_restate import CARRY
    length = np.linalg.norm(w.now.rays(WIDTH, HEIGHT)[1], axis=-1)
    hits = np.stack([w.hits.t * length, w.hits.barycentrics[..., 1], w.hits.barycentrics[..., 2]], axis=-1).astype(F).reshape(-1, 3)
    primitive = w.hits.triangle.copy()
    for i, s in enumerate(w.surfaces):  # a square's two triangles are (0, 1, 2) and (2, 3, 0): the device reports one of them
        if s.kind == "square":
            primitive[w.hits.instance == i] = 0
    meshes = [S.mesh(s) for s in w.previous]
    index_base = np.concatenate([[0], np.cumsum([m[1].size for m in meshes])])
    indices = np.concatenate([m[1] for m in meshes]).astype(U32)
    positions, carry = [], np.zeros(len(w.surfaces), CARRY)
    for i, (now, then) in enumerate(zip(w.surfaces, w.previous)):
        deformed = now.kind == "mesh" and not np.array_equal(now.vertices, then.vertices)
        carry[i] = (then.transform, int(deformed), sum(p.shape[0] for p in positions) if deformed else 0, index_base[i], 0)
        if deformed:
            positions.append(np.concatenate([then.vertices, np.zeros((then.vertices.shape[0], 1), F)], axis=1))
    return hits, w.hits.instance.astype(np.int32).reshape(-1), primitive.astype(np.int32).reshape(-1), w.g.reshape(-1, 4), indices, np.concatenate(positions), motion_table(twk, w), carry


@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_deformed_patch_and_moved_card(twk, far):
    """twk_previous_positions_host on hits restated from the reference: its plane within G of the float64 g' = M_prev sum b_i v_i_prev
    (the patch) and X64 g (the card), and g's bits on the wall. Then the Carried merges with that plane: the same lookup checks."""
    from temporal_carry_restate import to_ctypes
    L = twk._lib
    w = world(far, "deformed")
    hits, instance, primitive, g, indices, positions, motion, carry = carry_inputs(twk, w)
    plane = twk.previous_positions_host(hits, instance, primitive, g, indices, positions, to_ctypes(motion, L.InstanceMotion), to_ctypes(carry, L.InstanceCarry))
    plane = plane.reshape(HEIGHT, WIDTH, 4)
    error = np.abs(plane[..., :3].astype(D) - w.gp).max(axis=-1)
    G = plane_bound(w)
    for i, name in ((CARD, "card"), (PATCH, "patch")):
        on = w.hits.instance == i
        print(f"plane, {place_id(far)}, {name}: largest |g' - g'64| {error[on].max():.3e}, largest error / G {(error / G)[on].max():.4f} (K = {K_AOV})")
    assert (error <= G).all()
    assert np.array_equal(plane[..., 3].view(U32), w.g[..., 3].view(U32))
    assert np.array_equal(plane.view(U32)[w.hits.instance == WALL], w.g.view(U32)[w.hits.instance == WALL]), "the wall has not moved: the bits of g"
    plain = plain_merge(twk, w, plane=plane)
    verdict = judge_plain(w, plain)
    report("carried", w, verdict)
    assert verdict.ok
    on_patch = w.hits.instance == PATCH
    assert (verdict.full & on_patch).sum() >= 50
    cascade = cascade_merge(twk, w, plane=plane)
    verdict_c = judge_cascade(w, cascade)
    report("cascade carried", w, verdict_c)
    assert verdict_c.ok
    # negative control: the deformation's barycentrics rotated by one vertex
    slipped = R.expected_lookup(R.previous_positions(w.hits, w.surfaces, w.previous, rotate=1), w.hits.instance, w.then, w.history_hits.instance)
    share, least = control(w, plain, judge_plain, slipped, on_patch)
    print(f"control, barycentrics rotated: {share:.1%} of the patch's full pixels at least 10 B off, the least {least:.3f} px")
    control(w, cascade, judge_cascade, slipped, on_patch)


# ---- K: the geometry AOV of the oracle, which is held bit-equal to the device, against the reference ---------------------------------
@pytest.mark.parametrize("flatten", list(S.FLATTEN))
@pytest.mark.parametrize("far", PLACES, ids=place_id)
def test_the_oracles_centre_ray_hits_lie_within_G(orc, far, flatten):
    """orc.Oracle.traceRays on the centre rays (tests/temporal_restate.py centre_rays, the rays the AOV traces) over the scene, in both
    views: outside the exclusion's edge pixels the instance is the reference's, and P + t d lies within G of the reference's position.
    The largest error / (u (|P|inf + |g|inf) / |cos|) over all cases, 3.22, is what K = 16 was taken from."""
    from shading_fuzz import feed
    from temporal_restate import centre_rays
    worst = 0.0
    for scenario in ("static", "deformed"):
        w = world(far, scenario)
        for words, surfaces, hits in ((w.words_now, w.surfaces, w.hits), (w.words_then, w.previous, w.history_hits)):
            scene, state = S.fuzz_scene(surfaces, words, flatten)
            oracle = orc.Oracle(miss=1)
            feed(oracle, scene, state)
            P, d = centre_rays(words, WIDTH, HEIGHT)
            rays = np.empty((HEIGHT, WIDTH, 8), F)
            rays[..., 0:3], rays[..., 3], rays[..., 4:7], rays[..., 7] = P, F(state.epsilonFactor * F(1.0e-7)), d, F(1.0e27)
            tbg, ids = oracle.traceRays(rays)
            oracle.close()
            t, instance = tbg[:, 0].reshape(HEIGHT, WIDTH), ids[:, 0].reshape(HEIGHT, WIDTH)
            g = np.stack([P[k] + t * d[..., k] for k in range(3)], axis=-1)
            clear = hits.edge >= R.EDGE
            assert np.array_equal(instance[clear], hits.instance[clear])
            same = instance == hits.instance
            ratio = np.abs(g.astype(D) - hits.position).max(axis=-1) / R.bound_G(1.0, R.Camera(words).P, hits.position, hits.cos)
            worst = max(worst, float(ratio[same].max()))
            assert (ratio[same] <= K_AOV).all()
    print(f"AOV, {place_id(far)}, {flatten}: largest error / (u (|P| + |g|) / |cos|) = {worst:.3f}, K = {K_AOV}")
    assert 4.0 * worst <= K_AOV
