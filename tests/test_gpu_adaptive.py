"""-m gpu: the adaptive pass (twk_adaptive_select + twk_launch_adaptive) against the library's own uniform render. The invariant:
after uniform launches 0 .. K-1 and any adaptive passes, a launch index whose sample count is c holds in colour, both AOVs and
moments exactly the bits it holds after twk_launch(0 .. c-1) on a fresh handle. Two scenes at 61 x 37 — the Cornell box (slim
streams, packed queue) and a shading-fuzz scene with albedo texture, cutout opacity and an HDR environment (full streams, unpacked
queue) — in RGBA32F and RGBA16F, AOVs on. The schedule: four uniform iterations, then three rounds of select + three samples; the
target of a round is the median of that round's valid errors, so about half of the valid pixels lie on each side."""
import numpy as np
import pytest

import adaptive_restate as ar
import noise_restate as nr
import shading_fuzz as sf
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
RES = (sf.WIDTH, sf.HEIGHT)
assert RES == (61, 37)
UNIFORM, ROUNDS, SAMPLES = 4, 3, 3
SCENES = ("cornell", "fuzz")


def _device(twk, scene, half, index=0, count=1, adaptive=True, offset=0):
    if scene == "cornell":
        app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", RES)
        dev = twk.Device(ordinal=0, index=index, count=count, miss=app.info.miss)
        app.initDevice(dev, distribution=1 if count > 1 else None)
    else:
        fuzz = sf.make_scene(77, miss=2, tex=True, full=True)
        state = sf.default_state(fuzz)
        state.distribution = 1 if count > 1 else 0
        dev = twk.Device(ordinal=0, index=index, count=count, miss=fuzz.miss)
        sf.feed(dev, fuzz, state)
    if half:
        dev.setOutputFormat(twk._lib.TWK_OUTPUT_HALF4)
    dev.enableAov(True)
    dev.enableMoments(True)
    if adaptive:
        dev.enableAdaptive(True)
    if offset:
        dev.setSampleOffset(offset)
    return dev


def _read(dev, half):
    """[colour, albedo, normal, moments] as the buffers hold them: float16 bits in half mode, float32 bits otherwise; moments f32."""
    word = np.uint16 if half else np.uint32
    colour = dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()
    return [colour.view(word), dev.readAov(0, raw=True).view(word), dev.readAov(1, raw=True).view(word), dev.readMoments().view(np.uint32)]


NAMES = ("colour", "albedo", "normal", "moments")
_uniform_cache = {}


def _uniform(twk, scene, half, counts, offset=0, index=0, count=1):
    """{c: buffers after twk_launch(0 .. c-1)} for every c asked for: one fresh handle per (scene, format, offset, tiling), read as
    it passes each c (a uniform render does not depend on how its iterations are grouped into passes; the existing tests hold that)."""
    key = (scene, half, offset, index, count)
    have = _uniform_cache.setdefault(key, {})
    need = sorted(set(int(c) for c in counts) - set(have))
    if need:
        dev = _device(twk, scene, half, index, count, adaptive=False, offset=offset)
        done = 0
        for c in need:
            for it in range(done, c):
                dev.render(it)
            done = max(done, c)
            have[c] = _read(dev, half)
        dev.close()
    return have


def _schedule(twk, dev, cap=4096, split=False, targets=None):
    """Four uniform iterations, three rounds of select + renderAdaptive(3) (split: three times renderAdaptive(1)); checks each
    round's list against the restatement and the counts' advance. Returns (targets, lists, counts after the last round)."""
    for it in range(UNIFORM):
        dev.render(it)
    used, lists = [], []
    for r in range(ROUNDS):
        m = dev.readMoments().reshape(-1, 4)
        counts = dev.readSampleCounts().reshape(-1)
        if r == 0:
            assert (counts == UNIFORM).all()
        cls, e = nr.classify(m)
        valid = cls == nr.VALID
        target = float(np.median(e[valid])) if targets is None else targets[r]
        ap = twk.Adaptive(targetNoise=target, maxSamples=cap)
        n = dev.adaptiveSelect(ap)
        active = dev.readActive()
        expect = ar.active_list(m, counts, **ar.parameters(ap))
        assert n == active.size == expect.size and np.array_equal(active, expect), f"round {r}"
        chosen = np.zeros(counts.size, bool)
        chosen[active] = True
        if targets is None:  # the condition the schedule rests on: valid pixels on both sides in every round
            assert (chosen & valid).any() and (~chosen & valid).any(), f"round {r}: {int((chosen & valid).sum())} of {int(valid.sum())} valid pixels selected"
        if split:
            for _ in range(SAMPLES):
                dev.renderAdaptive(1)
        else:
            dev.renderAdaptive(SAMPLES)
        after = dev.readSampleCounts().reshape(-1)
        assert np.array_equal(after.astype(np.int64) - counts, np.where(chosen, SAMPLES, 0)), f"round {r}: the counts advance by {SAMPLES} on the list only"
        used.append(target)
        lists.append(active)
    return used, lists, dev.readSampleCounts()


def _assert_invariant(twk, scene, half, got, counts, offset=0, index=0, count=1, skip=None):
    distinct = np.unique(counts if skip is None else counts[~skip])
    ref = _uniform(twk, scene, half, distinct, offset, index, count)
    for c in distinct:
        where = counts == c
        if skip is not None:
            where &= ~skip
        for name, g, w in zip(NAMES, got, ref[int(c)]):
            bad = np.nonzero((g[where] != w[where]).any(axis=-1))[0]
            assert bad.size == 0, f"{scene} half={half}: {name} differs from twk_launch(0..{int(c) - 1}) at {bad.size} of {int(where.sum())} pixels with count {int(c)}"
    return distinct


@pytest.mark.parametrize("scene,half,cap", [("cornell", False, 4096), ("cornell", True, 4096), ("fuzz", False, 4096), ("fuzz", True, 4096), ("cornell", False, 10)])
def test_a_pixel_with_count_c_holds_the_bits_of_c_uniform_launches(twk, scene, half, cap):
    dev = _device(twk, scene, half)
    info = dev.streamLayout()
    assert info == ("slim" if scene == "cornell" else "full")  # the two layouts of the path streams an adaptive pass runs on
    targets, lists, counts = _schedule(twk, dev, cap)
    got = _read(dev, half)
    if cap == 10:  # the cap cuts in during the third round: pixels selected twice are at 10 and stay out whatever their error
        m = dev.readMoments().reshape(-1, 4)
        assert (counts.reshape(-1) <= 4 + 2 * SAMPLES + SAMPLES).all()
        twice = np.intersect1d(lists[0], lists[1])
        assert twice.size > 0 and not np.isin(twice, lists[2]).any()
        assert (counts.reshape(-1)[twice] == 10).all()
    distinct = _assert_invariant(twk, scene, half, got, counts)
    print(f"\n{scene} half={half} cap={cap}: targets {[round(t, 4) for t in targets]}, active {[a.size for a in lists]}, counts {distinct.tolist()}, layout {info}")
    assert distinct.size >= 3 and distinct.min() == UNIFORM  # several histories in one picture, one of them purely uniform
    dev.close()


@pytest.mark.parametrize("scene,half", [("cornell", True), ("fuzz", False)])
def test_three_samples_at_once_equal_three_passes_of_one(twk, scene, half):
    one = _device(twk, scene, half)
    targets, lists, counts = _schedule(twk, one)
    a = _read(one, half)
    one.close()
    three = _device(twk, scene, half)
    _, lists3, counts3 = _schedule(twk, three, split=True, targets=targets)
    b = _read(three, half)
    three.close()
    assert all(np.array_equal(x, y) for x, y in zip(lists, lists3)) and np.array_equal(counts, counts3)
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), name


def _assemble(twk, parts, tile):
    """The pictures of two tiled handles' packed buffers put together on the host, as the compositor would."""
    full = [np.zeros((RES[1], RES[0]) + p.shape[2:], p.dtype) for p in parts[0]]
    seen = np.zeros((RES[1], RES[0]), int)
    for index, buffers in enumerate(parts):
        lw = buffers[0].shape[1]
        for ly in range(RES[1]):
            for lx in range(lw):
                px = twk.tile_column(lx, ly, tile, len(parts), index)
                if px < RES[0]:
                    seen[ly, px] += 1
                    for f, b in zip(full, buffers):
                        f[ly, px] = b[ly, lx]
    assert (seen == 1).all()
    return full


@pytest.mark.parametrize("scene", SCENES)
def test_two_tiled_handles_equal_one(twk, scene):
    single = _device(twk, scene, False)
    targets, _, counts = _schedule(twk, single)
    whole = _read(single, False) + [counts[..., None]]
    tile = (single.state.tileSize[0], single.state.tileSize[1])
    single.close()
    parts = []
    for index in range(2):
        dev = _device(twk, scene, False, index=index, count=2)
        _, _, c = _schedule(twk, dev, targets=targets)
        parts.append(_read(dev, False) + [c[..., None]])
        dev.close()
    for name, x, y in zip(NAMES + ("counts",), _assemble(twk, parts, tile), whole):
        assert np.array_equal(x, y), name


def test_sample_offset_gives_the_bits_of_a_uniform_render_with_it(twk):
    dev = _device(twk, "cornell", False, offset=7)
    _, _, counts = _schedule(twk, dev)
    got = _read(dev, False)
    dev.close()
    _assert_invariant(twk, "cornell", False, got, counts, offset=7)
    plain = _uniform(twk, "cornell", False, [UNIFORM + SAMPLES])[UNIFORM + SAMPLES]
    shifted = _uniform(twk, "cornell", False, [UNIFORM + SAMPLES], offset=7)[UNIFORM + SAMPLES]
    assert not np.array_equal(plain[0], shifted[0])  # and the offset is not a no-op


def test_enabled_without_an_adaptive_call_changes_no_byte(twk):
    for scene, half in (("cornell", True), ("fuzz", False)):
        dev = _device(twk, scene, half)
        for it in range(6):
            dev.render(it)
        got = _read(dev, half)
        assert (dev.readSampleCounts() == 6).all()
        dev.close()
        for name, g, w in zip(NAMES, got, _uniform(twk, scene, half, [6])[6]):
            assert np.array_equal(g, w), (scene, name)


def _refused(twk, call, code, *words):
    with pytest.raises(twk.TwkError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_launch_rules_after_an_adaptive_pass(twk):
    L = twk._lib
    dev = _device(twk, "cornell", False)
    _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_launch_adaptive")  # before any select
    for it in range(UNIFORM):
        dev.render(it)
    _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_select")
    for samples in (0, 65):
        _refused(twk, lambda: dev.renderAdaptive(samples), L.TWK_ERROR_INVALID_VALUE, "1..64")
    # an empty list is a successful no-op that changes nothing and leaves the picture uniform
    before = _read(dev, False)
    assert dev.adaptiveSelect(twk.Adaptive(targetNoise=1e30, minSamples=2)) == 0 and dev.readActive().size == 0
    dev.renderAdaptive(3)
    assert all(np.array_equal(x, y) for x, y in zip(before, _read(dev, False))) and (dev.readSampleCounts() == UNIFORM).all()
    dev.render(UNIFORM)  # still uniform: allowed, and it drops the list
    _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_select")
    n = dev.adaptiveSelect(twk.Adaptive(targetNoise=1e-6))
    assert n > 0 and (dev.readSampleCounts() == UNIFORM + 1).all()
    dev.renderAdaptive(2)
    _refused(twk, lambda: dev.render(5), L.TWK_ERROR_INVALID_STATE, "twk_launch", "iteration 0", "twk_launch_adaptive")
    dev.renderAdaptive(1)  # the refused launch has not dropped the list
    assert dev.readSampleCounts().max() == UNIFORM + 1 + 3
    dev.render(0)  # restarts a uniform frame
    _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_select")
    dev.adaptiveSelect(twk.Adaptive(targetNoise=1e-6))
    assert (dev.readSampleCounts() == 1).all()
    dev.render(1)
    dev.render(2)
    got = _read(dev, False)
    for name, g, w in zip(NAMES, got, _uniform(twk, "cornell", False, [3])[3]):
        assert np.array_equal(g, w), name  # the restarted frame is a uniform frame
    dev.close()


def test_state_refusals(twk):
    L = twk._lib
    plain = _device(twk, "cornell", False, adaptive=False)
    _refused(twk, lambda: plain.adaptiveSelect(), L.TWK_ERROR_INVALID_STATE, "twk_enable_adaptive")
    _refused(twk, lambda: plain.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE)
    _refused(twk, lambda: plain.readSampleCounts(), L.TWK_ERROR_INVALID_STATE)
    plain.enableMoments(False)
    _refused(twk, lambda: plain.enableAdaptive(True), L.TWK_ERROR_INVALID_STATE, "twk_enable_moments")
    plain.close()

    def selected():
        dev = _device(twk, "cornell", False)
        for it in range(UNIFORM):
            dev.render(it)
        assert dev.adaptiveSelect(twk.Adaptive(targetNoise=1e-6)) > 0
        return dev

    for name, switch in (("time view", lambda d: d.setTimeView(True)), ("capture", lambda d: d.debugCapture(True)), ("statistics", lambda d: d.statsEnable(True))):
        dev = selected()
        switch(dev)
        _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_launch_adaptive")
        dev.close()
    dev = selected()
    frame = _DeviceBuffer(twk, RES[0] * RES[1] * 16)
    dev.setSharedFrame(frame.ptr.value, frame.nbytes)
    _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "shared frame")
    dev.setSharedFrame(0, 0)
    _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_adaptive_select")  # the change of buffer dropped the list
    frame.free()
    dev.close()
    for name, change in (("state", lambda d: d.setState(d.state)), ("format", lambda d: d.setOutputFormat(L.TWK_OUTPUT_HALF4)), ("build", lambda d: d.build()),
                         ("switch", lambda d: (d.enableAdaptive(False), d.enableAdaptive(True)))):
        dev = selected()
        change(dev)
        _refused(twk, lambda: dev.renderAdaptive(1), L.TWK_ERROR_INVALID_STATE, "twk_launch_adaptive")
        _refused(twk, lambda: dev.readActive(), L.TWK_ERROR_INVALID_STATE, "twk_read_active")
        dev.close()
