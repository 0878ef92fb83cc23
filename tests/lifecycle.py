"""What tests/test_gpu_handle_lifecycle.py and tests/test_lifecycle_shapes_host.py share: the state transitions of a handle that
lives through a second twk_set_state, as data, and one fixed schedule over every per-launch-index buffer of a handle, whose byte-exact
results a reused handle and a fresh one are compared by. A helper module, not a conftest.

Left out of the schedule on a tiled handle (distribution 1, several devices), because the ABI refuses them for packed tile buffers:
  twk_render_geometry                     ("geometry")
  twk_cascade_resolve, own-buffer form     ("resolved")
  twk_denoise*, own-buffer form            ("denoised")
  twk_temporal_accumulate, own-buffer form ("temporal", "temporal_moments")
The read of the geometry buffer before the first pass is not refused and stays."""
from collections import namedtuple

import numpy as np

import noise_restate as nr

SYSTEM, SCENE = "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt"
TILED_LEFT_OUT = ("geometry", "resolved", "denoised", "temporal", "temporal_moments")
FLOAT4, HALF4 = 0, 1
DIRTY_OFFSET = 1000
DIRTY_TARGET = 0.05  # the adaptive target of the dirtying schedule (the default of twk_adaptive_defaults)

# One state of a transition. format: the output format to switch to before this state is set (None: the test's own, left alone);
# deep: a deferred pass of 16 iterations is part of the state's history (dirty only).
Shape = namedtuple("Shape", "width height tile distribution format deep", defaults=((8, 8), 0, None, False))
# handles: the (index, count) of every handle of the case. same_launch_width / same_elements: what the row claims of launchWidth and
# launchWidth x height before and after; padding: per handle, the elements outside the picture (before, after); formats: the output
# formats the case runs in.
Transition = namedtuple("Transition", "id handles before after same_launch_width same_elements padding formats")

ONE, TWO = ((0, 1),), ((0, 2), (1, 2))
BOTH = (FLOAT4, HALF4)
TRANSITIONS = (
    Transition("grow", ONE, Shape(24, 16), Shape(64, 37), False, False, ((0, 0),), BOTH),                # every buffer regrown
    Transition("shrink", ONE, Shape(64, 37), Shape(24, 16), False, False, ((0, 0),), BOTH),              # every buffer kept; stride changes
    Transition("reshape", ONE, Shape(64, 36), Shape(36, 64), False, True, ((0, 0),), BOTH),              # equal element count, other launchWidth
    Transition("tiles-pad", TWO, Shape(64, 37, (8, 8), 1), Shape(61, 37, (8, 8), 1), True, True, ((0, 48), (0, 63)), BOTH),
    Transition("tiles-tile", TWO, Shape(61, 37, (8, 8), 1), Shape(61, 37, (8, 16), 1), True, True, ((48, 48), (63, 63)), BOTH),
    Transition("tiles-shrink", TWO, Shape(128, 37, (8, 8), 1), Shape(61, 37, (8, 8), 1), False, False, ((0, 48), (0, 63)), BOTH),
    Transition("retile", ((1, 2),), Shape(61, 37, (8, 8), 0), Shape(61, 37, (8, 8), 1), False, False, ((0, 63),), BOTH),
    Transition("format", ONE, Shape(64, 37, format=HALF4), Shape(24, 16, format=FLOAT4), False, False, ((0, 0),), (FLOAT4,)),
    Transition("batch-history", ONE, Shape(64, 37, deep=True), Shape(24, 16), False, False, ((0, 0),), BOTH),
)
# tiles-tile: the elements that were picture with 8x8 tiles and are padding with 8x16 tiles, per handle
TILES_TILE_BECOME_PADDING = (24, 24)
BY_ID = {t.id: t for t in TRANSITIONS}


def is_tiled(shape, count):
    return bool(shape.distribution) and count > 1


def launch_width(twk, shape, count):
    return twk.launch_width(shape.width, shape.tile[0], count) if is_tiled(shape, count) else shape.width


def padding_mask(twk, shape, index, count):
    """bool [height, launchWidth]: the launch indices of handle `index` that map outside the picture (twk_tile_column)."""
    lw = launch_width(twk, shape, count)
    mask = np.zeros((shape.height, lw), bool)
    if is_tiled(shape, count):
        for y in range(shape.height):
            for x in range(lw):
                mask[y, x] = twk.tile_column(x, y, shape.tile, count, index) >= shape.width
    return mask


def make_app(twk, load_app, shape):
    """The Cornell box at the shape's resolution, with the shape's tile size in the state it hands out through state_of()."""
    return load_app(twk, SYSTEM, SCENE, (shape.width, shape.height))


def state_of(app, shape):
    st = app.state
    st.resolution[0], st.resolution[1] = shape.width, shape.height
    st.tileSize[0], st.tileSize[1] = shape.tile
    st.distribution = int(shape.distribution)
    return st


def new_device(twk, app, shape, index=0, count=1, half=False):
    """A handle with every feature on, enabled once before the first state, in `shape`."""
    dev = twk.Device(ordinal=0, index=index, count=count, miss=app.info.miss)
    dev.enableAov(True)
    dev.enableMoments(True)
    dev.enableGeometry(True)
    dev.enableAdaptive(True)
    dev.enableCascade(True)
    if half:
        dev.setOutputFormat(HALF4)
    app.initDevice(dev)
    dev.setState(state_of(app, shape))
    assert dev.launchWidth == launch_width(twk, shape, count)
    return dev


def move(dev, app_after, shape):
    """The viewer's resize: twk_set_state, then the camera of the new aspect. The scene is not rebuilt."""
    dev.setState(state_of(app_after, shape))
    dev.updateCamera(0, app_after.cameras[0])


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]).copy()


def _output(dev):
    return _words(dev.getOutputBufferHalf() if dev.outputFormat == HALF4 else dev.getOutputBufferHost())


def _summary(s):
    return np.concatenate([np.array([s.valid, s.unknown, s.empty, s.sumFixed, s.maxErrorBits], np.uint64), s.histogram.astype(np.uint64)])


def median_target(moments_words):
    """The median relative standard error of the valid elements of a moments buffer (uint32 words of readMoments)."""
    cls, e = nr.classify(moments_words.view(np.float32).reshape(-1, 4))
    assert (cls == nr.VALID).any()
    return float(np.median(e[cls == nr.VALID]))


def snapshot(twk, dev, app, tiled, target=None, offset=0):
    """The fixed schedule on a handle that is in its final state; returns {key: uint32 / uint16 / uint8 / uint64 words}, byte-exact.
    target: the adaptive select's and plan's targetNoise; None (the fresh handle) takes the median e of the handle's own valid
    elements after the eight uniform iterations, and hands it out as out["target"] for the other handle. offset: the sample offset
    the schedule runs under (dirty's)."""
    out = {}
    dev.setSampleOffset(offset)
    dev.setLaunchBatch(1)
    dev.reserveLaunchBatch(1)  # what twk_set_state leaves to the first use: the buffers of the state, zeroed on a fresh handle
    out["moments@start"] = _words(dev.readMoments())
    out["albedo@start"] = _words(dev.readAov(0, raw=True))
    out["normal@start"] = _words(dev.readAov(1, raw=True))
    out["geometry@start"] = _words(dev.readGeometry())
    out["cascade@start"] = _words(dev.readCascade())

    # part 1: four passes of one iteration, one deferred pass of four
    for it in range(4):
        dev.render(it)
    dev.synchronizeStream()
    dev.setLaunchBatch(4)
    for it in range(4, 8):
        dev.render(it)
    dev.synchronizeStream()
    dev.setLaunchBatch(1)
    out["output@8"] = _output(dev)
    out["albedo@8"] = _words(dev.readAov(0, raw=True))
    out["normal@8"] = _words(dev.readAov(1, raw=True))
    out["moments@8"] = _words(dev.readMoments())
    out["cascade@8"] = _words(dev.readCascade())

    # part 2
    if not tiled:
        dev.renderGeometry()
        out["geometry"] = _words(dev.readGeometry())
    out["noise"] = _summary(dev.estimateNoise())

    # part 3
    if target is None:
        target = median_target(out["moments@8"])
    out["target"] = np.array([target], np.float64).view(np.uint64)
    ap = twk.Adaptive(targetNoise=target)
    n = dev.adaptiveSelect(ap)
    out["active"] = dev.readActive()
    assert out["active"].size == n
    dev.renderAdaptive(2)
    out["counts@select"] = dev.readSampleCounts()
    n, paths = dev.adaptivePlan(ap)
    active, offsets = dev.readPlan()
    assert active.size == n and int(offsets[-1]) == paths
    out["plan.active"], out["plan.offsets"] = active, offsets
    dev.renderPlanned()
    out["output@plan"] = _output(dev)
    out["moments@plan"] = _words(dev.readMoments())
    out["counts@plan"] = dev.readSampleCounts()
    out["cascade@plan"] = _words(dev.readCascade())

    # part 4
    if not tiled:
        dev.cascadeResolve()
        out["resolved"] = _words(dev.readResolved())
        dev.denoise(twk.Denoiser(iterations=2), minSamples=4)
        out["denoised"] = _words(dev.readDenoised(raw=True))
    out["tonemap"] = dev.tonemap(app.tonemapper)
    if not tiled:
        dev.temporalAccumulate()
        out["temporal"] = _words(dev.readTemporal())
        out["temporal_moments"] = _words(dev.readTemporalMoments())
    return out


def dirty(twk, dev, app_before, tiled, deep=False):
    """The same schedule at the earlier state under another sample offset: every buffer then holds words that differ from what the
    final state produces at the same element. deep: a deferred pass of 16 iterations first, which grows the path streams to 16
    samples per launch index. Returns the dirty handle's snapshot."""
    if deep:
        dev.setSampleOffset(DIRTY_OFFSET)
        dev.setLaunchBatch(16)
        for it in range(16):
            dev.render(it)
        dev.synchronizeStream()
    # (a target of its own: at a wide "before" state most valid pixels are converged background and their median e is 0)
    out = snapshot(twk, dev, app_before, tiled, target=DIRTY_TARGET, offset=DIRTY_OFFSET)
    dev.setSampleOffset(0)
    return out


def first_difference(a, b):
    """None when the arrays are equal in shape and words, else a text that names the first differing element."""
    if a.shape != b.shape:
        return f"shape {a.shape} against {b.shape}"
    bad = np.argwhere(a != b)
    if bad.size == 0:
        return None
    at = tuple(int(i) for i in bad[0])
    return f"{bad.shape[0]} of {a.size} words differ, first at {at}: {int(a[at]):#x} against {int(b[at]):#x}"
