"""-m gpu: a handle that lives through a second twk_set_state renders like a fresh one (tests/lifecycle.py: the transitions and the
schedule). Every comparison is np.array_equal on uint32 / uint16 words: there are no tolerances.
  2a  reused handle == fresh handle, key by key, for every transition of the table, in RGBA32F and RGBA16F; the tiled cases check
      their own sensitivity before the move and the padding after it; the one-handle cases are anchored to the CPU oracle
  2b  a twk_set_state that leaves the frame's geometry alone keeps the buffers (the device pointers do not change)
  2c  external output buffers and shared frames through a shrink and a grow, with guarded slack behind every allocation
  2d  three handles created, run through the schedule and destroyed in turn; a fourth renders what the first did"""
import numpy as np
import pytest

import lifecycle as lc
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

SLACK = 4096
PATTERN = 0xA5


def _problems(got, want):
    out = []
    for key in want:
        if key not in got:
            out.append(f"{key}: missing")
            continue
        diff = lc.first_difference(got[key], want[key])
        if diff:
            out.append(f"{key}: {diff}")
    return out


_ORACLE = {}


def _oracle(twk, orc, shape, index, count):
    """(output, albedo, normal) words of the CPU oracle after eight iterations at `shape`; computed once per shape."""
    key = (shape.width, shape.height, shape.tile, shape.distribution, index, count)
    if key not in _ORACLE:
        app = lc.make_app(twk, load_app, shape)
        ref = orc.Oracle(index=index, count=count, miss=app.info.miss)
        ref.loadApplication(app, state=lc.state_of(app, shape))
        ref.enableAov(True)
        for it in range(8):
            ref.render(it)
        _ORACLE[key] = tuple(np.ascontiguousarray(a, np.float32).view(np.uint32) for a in (ref.getOutputBufferHost(), ref.readAov(0), ref.readAov(1)))
        ref.close()
    return _ORACLE[key]


CASES = [pytest.param(t, fmt, id=f"{t.id}-{'rgba16f' if fmt == lc.HALF4 else 'rgba32f'}") for t in lc.TRANSITIONS for fmt in t.formats]


@pytest.mark.parametrize("t,fmt", CASES)
def test_reused_handle_equals_fresh_handle(twk, orc, t, fmt):
    half = fmt == lc.HALF4
    app_before, app_after = lc.make_app(twk, load_app, t.before), lc.make_app(twk, load_app, t.after)
    problems, non_empty = [], 0
    for index, count in t.handles:
        tiled_before, tiled_after = lc.is_tiled(t.before, count), lc.is_tiled(t.after, count)
        fresh = lc.new_device(twk, app_after, t.after, index, count, half)
        want = lc.snapshot(twk, fresh, app_after, tiled_after)
        fresh.close()
        for key in ("moments@start", "albedo@start", "normal@start", "geometry@start", "cascade@start"):
            assert not want[key].any(), f"a fresh handle's {key} is not zero"
        target = float(want["target"].view(np.float64)[0])

        dev = lc.new_device(twk, app_before, t.before, index, count, half and t.before.format is None)
        if t.before.format is not None:  # the format row: a picture in the first format, then the switch
            for it in range(2):
                dev.render(it)
            dev.setOutputFormat(t.before.format)
        soiled = lc.dirty(twk, dev, app_before, tiled_before, deep=t.before.deep)
        pad_after = lc.padding_mask(twk, t.after, index, count).reshape(-1)
        if tiled_after:
            # the case's own sensitivity: the elements that become padding hold a picture's words
            pad_before = lc.padding_mask(twk, t.before, index, count).reshape(-1)
            become = np.flatnonzero(pad_after)
            become = become[(become < pad_before.size)]
            become = become[~pad_before[become]]
            assert become.size >= min(24, int(pad_after.sum())), (become.size, int(pad_after.sum()))
            moments = soiled["moments@plan"].view(np.float32).reshape(-1, 4)
            output = soiled["output@plan"].reshape(-1, 4)
            assert (moments[become, 2] > 0).all() and (output[become, 3] != 0).all(), "the dirty handle holds nothing where the padding will be"

        lc.move(dev, app_after, t.after)
        if t.after.format is not None:
            dev.setOutputFormat(t.after.format)
        got = lc.snapshot(twk, dev, app_after, tiled_after, target=target)
        dev.close()
        who = f"handle {index}/{count}: "
        problems += [who + p for p in _problems(got, want)]

        if tiled_after:
            padding, elements = int(pad_after.sum()), pad_after.size
            valid, unknown, empty = (int(v) for v in got["noise"][:3])
            if empty != padding or valid + unknown != elements - padding:
                problems.append(who + f"noise summary: valid {valid} + unknown {unknown}, empty {empty}; the buffer has {elements - padding} picture elements and {padding} of padding")
            non_empty += valid + unknown
            for key in ("active", "plan.active"):
                listed = got[key][pad_after[got[key]]]
                if listed.size:
                    problems.append(who + f"{key}: {listed.size} entries are padding, first {int(listed[0])}")
            for key in ("output@8", "output@plan", "moments@8", "moments@plan"):
                words = got[key].reshape(pad_after.size, -1)[pad_after]
                if words.any():
                    problems.append(who + f"{key}: {int(words.any(axis=1).sum())} padding elements are not zero, first at element {int(np.flatnonzero(pad_after)[np.flatnonzero(words.any(axis=1))[0]])}")
            for key in ("cascade@8", "cascade@plan"):
                words = got[key].reshape(got[key].shape[0], pad_after.size, -1)[:, pad_after]
                if words.any():
                    problems.append(who + f"{key}: padding elements are not zero in {int(words.any(axis=(0, 2)).sum())} launch indices")

        if len(t.handles) == 1 and not half:
            # the anchor: reused == fresh would hold if both were wrong in the same way; the oracle does not share the handle's code
            for key, ref in zip(("output@8", "albedo@8", "normal@8"), _oracle(twk, orc, t.after, index, count)):
                diff = lc.first_difference(got[key], ref)
                if diff:
                    problems.append(who + f"{key} against the CPU oracle: {diff}")
    if len(t.handles) > 1 and non_empty != t.after.width * t.after.height:
        problems.append(f"the tiles' non-empty elements sum to {non_empty}, the picture has {t.after.width * t.after.height}")
    assert not problems, f"{t.id}: {len(problems)} differences\n  " + "\n  ".join(problems)


def _pointers(dev):
    return (dev.outputDevicePointer(), dev.momentsDevicePointer(), dev.cascadeDevicePointer(), dev.geometryDevicePointer())


def _picture(dev):
    return {"output": lc._output(dev), "albedo": lc._words(dev.readAov(0, raw=True)), "normal": lc._words(dev.readAov(1, raw=True)),
            "moments": lc._words(dev.readMoments()), "cascade": lc._words(dev.readCascade())}


def test_a_state_change_that_keeps_the_geometry_keeps_the_buffers(twk):
    """twk_set_state with only pathLengths changed, and again with an identical state, allocates and clears nothing: the device
    pointers keep their values (a GUI calls it on every slider move); the picture restarted at iteration 0 is a fresh handle's."""
    shape = lc.Shape(64, 37)
    app = lc.make_app(twk, load_app, shape)
    dev = lc.new_device(twk, app, shape)
    for it in range(4):
        dev.render(it)
    dev.renderGeometry()
    dev.synchronizeStream()
    before = _pointers(dev)
    assert all(p and n for p, n in before)
    st = lc.state_of(app, shape)
    assert st.pathLengths[1] != 5
    st.pathLengths[0], st.pathLengths[1] = 2, 5
    for _ in range(2):  # the changed state, then the identical one
        dev.setState(st)
        assert _pointers(dev) == before, "twk_set_state with the frame's geometry unchanged moved a buffer"
    for it in range(4):
        dev.render(it)
    got = _picture(dev)
    dev.close()

    fresh = lc.new_device(twk, app, shape)
    fresh.setState(st)
    for it in range(4):
        fresh.render(it)
    want = _picture(fresh)
    assert not _problems(got, want), _problems(got, want)

    # a move that changes the geometry may move the buffers; the getters answer for the new state
    after = lc.Shape(24, 16)
    lc.move(fresh, lc.make_app(twk, load_app, after), after)
    sizes = [n for _, n in _pointers(fresh)]
    assert sizes == [24 * 16 * 16, 24 * 16 * 16, 24 * 16 * 16 * twk._lib.TWK_CASCADE_LAYERS, 24 * 16 * 16]
    fresh.close()


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_a_destroyed_handle_leaves_nothing_to_the_next(twk, half):
    """Three handles with every feature on are created, run through the whole schedule and destroyed, one after the other in one
    process: twk_device_destroy frees every buffer the schedule made the handle allocate. A fourth, fresh handle's snapshot then
    equals the first's key by key, word by word: nothing of a destroyed handle reaches the next one."""
    shape = lc.Shape(24, 16)
    app = lc.make_app(twk, load_app, shape)
    shots = []
    for _ in range(4):
        dev = lc.new_device(twk, app, shape, half=half)
        shots.append(lc.snapshot(twk, dev, app, False))
        dev.close()
    assert set(shots[3]) == set(shots[0])
    problems = _problems(shots[3], shots[0])
    assert not problems, f"the fourth handle against the first: {len(problems)} differences\n  " + "\n  ".join(problems)


class _Guarded:
    """A device allocation SLACK bytes longer than asked, filled with a pattern: a write beyond an extent shows in the slack or in
    the bytes that should have stayed, as an assertion."""

    def __init__(self, twk, nbytes):
        self.nbytes = nbytes
        self.buffer = _DeviceBuffer(twk, nbytes + SLACK)
        self.buffer.upload(np.full(nbytes + SLACK, PATTERN, np.uint8))
        self.ptr = self.buffer.ptr.value

    def bytes(self):
        return self.buffer.download((self.nbytes + SLACK,), np.uint8)

    def check_slack(self, where):
        assert (self.bytes()[self.nbytes:] == PATTERN).all(), f"{where}: the slack behind the buffer was written"

    def free(self):
        self.buffer.free()


def _render4(devices):
    for it in range(4):
        for d in devices:
            d.render(it)
    for d in devices:
        d.synchronizeStream()


BIG, SMALL = lc.Shape(64, 37), lc.Shape(24, 16)


def _handles(twk, app, shape, count):
    shape = shape._replace(distribution=1 if count > 1 else 0)
    return shape, [lc.new_device(twk, app, shape, index, count) for index in range(count)]


@pytest.mark.parametrize("count", [1, 2], ids=["output-pointer", "shared-frame"])
def test_external_buffer_through_a_shrink(twk, count):
    """A caller's buffer that is large enough for the new state receives the picture at the new layout; what lies beyond the new
    extent, and the slack, are untouched; the picture is a fresh handle's with an external buffer of its own."""
    apps = {s: lc.make_app(twk, load_app, s) for s in (BIG, SMALL)}
    attach = (lambda d, g: d.setSharedFrame(g.ptr, g.nbytes)) if count > 1 else (lambda d, g: d.setOutputDevicePointer(g.ptr, g.nbytes))
    big, devices = _handles(twk, apps[BIG], BIG, count)
    ext = _Guarded(twk, BIG.width * BIG.height * 16)
    for d in devices:
        attach(d, ext)
    _render4(devices)
    ext.check_slack("at the first state")
    old = ext.bytes()
    assert (old[:ext.nbytes].view(np.uint32).reshape(-1, 4)[:, 3] == np.float32(1).view(np.uint32)).all()  # a whole picture
    small = SMALL._replace(distribution=big.distribution)
    for d in devices:
        lc.move(d, apps[SMALL], small)
        assert d.outputDevicePointer()[0] == ext.ptr, "an external buffer that is large enough was dropped"
    assert np.array_equal(ext.bytes(), old), "twk_set_state wrote to the caller's buffer"
    _render4(devices)
    ext.check_slack("after the shrink")
    new = ext.bytes()
    extent = SMALL.width * SMALL.height * 16 if count > 1 else devices[0].launchWidth * SMALL.height * 16
    assert np.array_equal(new[extent:], old[extent:]), "bytes beyond the new extent were written"
    read = [lc._output(d) for d in devices]
    for d in devices:
        d.close()

    _, devices = _handles(twk, apps[SMALL], SMALL, count)
    own = _Guarded(twk, ext.nbytes)
    for d in devices:
        attach(d, own)
    _render4(devices)
    own.check_slack("fresh handle")
    assert np.array_equal(new[:extent], own.bytes()[:extent]), "the picture in the external buffer differs from a fresh handle's"
    for d, r in zip(devices, read):
        assert np.array_equal(lc._output(d), r)
        d.close()
    ext.free()
    own.free()


@pytest.mark.parametrize("count", [1, 2], ids=["output-pointer", "shared-frame"])
def test_external_buffer_through_a_grow(twk, count):
    """A caller's buffer that is too small for the new state is let go: the handle renders into its internal buffer, the caller's
    allocation is not written again, twk_get_output_device_pointer no longer names it, and the picture is a fresh handle's."""
    apps = {s: lc.make_app(twk, load_app, s) for s in (BIG, SMALL)}
    small, devices = _handles(twk, apps[SMALL], SMALL, count)
    ext = _Guarded(twk, (SMALL.width if count > 1 else devices[0].launchWidth) * SMALL.height * 16)
    for d in devices:
        if count > 1:
            d.setSharedFrame(ext.ptr, ext.nbytes)
        else:
            d.setOutputDevicePointer(ext.ptr, ext.nbytes)
    _render4(devices)
    ext.check_slack("at the first state")
    old = ext.bytes()
    big = BIG._replace(distribution=small.distribution)
    for d in devices:
        lc.move(d, apps[BIG], big)
    _render4(devices)
    assert np.array_equal(ext.bytes(), old), "the caller's buffer, too small for the new state, was written again"
    for d in devices:
        pointer, nbytes = d.outputDevicePointer()
        assert pointer != ext.ptr and pointer and nbytes == d.launchWidth * BIG.height * 16
    got = [lc._output(d) for d in devices]
    for d in devices:
        d.close()
    ext.free()

    _, devices = _handles(twk, apps[BIG], BIG, count)
    _render4(devices)
    for d, g in zip(devices, got):
        assert g.shape == (BIG.height, d.launchWidth, 4)
        diff = lc.first_difference(g, lc._output(d))
        assert diff is None, diff
        d.close()
