"""-m gpu: the geometry AOV of a tiled frame (twk_render_geometry_tile, twk_assemble_with_geometry,
twk_assemble_devices_with_geometry; csrc/temporal_device.h, csrc/assemble_device.h). Every comparison is byte equality.
  * every handle's tile share equals the single-device geometry gathered through twk.tile_column, zeros at the padding: 61x37 with
    8x8 tiles on 2 and 3 handles (launchWidth 32 and 24, 3 and 11 padding columns), 64x16 with 2x4 tiles on 2 (the element-wise path),
  * the assembly with geometry gives the single-device geometry, directly and staged, alone (planes=()) and beside all six planes,
    which then equal what assemble gives; the explicit form on blocks the test gathered,
  * on one device renderGeometryTile is renderGeometry,
  * every new refusal, and the life of the assembled geometry across a camera change and a resize."""
import ctypes as C

import numpy as np
import pytest

import lifecycle as lc
from conftest import load_app
from test_gpu_half_output import _DeviceBuffer

pytestmark = pytest.mark.gpu

PLANES = range(6)
OUTPUT, ALBEDO, NORMAL, MOMENTS, COUNTS, CASCADE = PLANES
CASES = [(61, 37, (8, 8), 2), (61, 37, (8, 8), 3), (64, 16, (2, 4), 2)]
IDS = ["61x37-2", "61x37-3", "64x16-elementwise-2"]


def _single_geometry(twk, width, height):
    shape = lc.Shape(width, height, (8, 8), 1)
    app = lc.make_app(twk, load_app, shape)
    dev = lc.new_device(twk, app, shape)
    dev.renderGeometry()
    words = lc._words(dev.readGeometry())
    dev.close()
    app.close()
    hit = words[..., 3] != 0
    assert hit.any() and words[hit][:, :3].any(), "centre rays hit the box (a wide frame sees the background beside it): the equalities are not of zeros"
    return words


@pytest.fixture(scope="module")
def single(twk):
    """{(width, height): uint32 [height, width, 4]}: the single-device geometry AOV of the Cornell box; computed once."""
    return {(w, h): _single_geometry(twk, w, h) for w, h in ((61, 37), (64, 16))}


def _handles(twk, width, height, tile, n, render=0):
    shape = lc.Shape(width, height, tile, 1)
    app = lc.make_app(twk, load_app, shape)
    devs = [lc.new_device(twk, app, shape, index=i, count=n) for i in range(n)]
    for d in devs:
        for it in range(render):
            d.render(it)
    return app, devs


def _close(app, devs):
    for d in devs:
        d.close()
    app.close()


def _gathered(twk, whole, tile, n, index, launch_width):
    """The tile share of handle `index`: whole[y, tile_column(lx, y)] per launch index, zeros at the padding."""
    height, width = whole.shape[:2]
    out = np.zeros((height, launch_width, 4), np.uint32)
    for y in range(height):
        for lx in range(launch_width):
            x = twk.tile_column(lx, y, tile, n, index)
            if x < width:
                out[y, lx] = whole[y, x]
    return out


def _same(got, want, what):
    diff = lc.first_difference(got, want)
    assert diff is None, f"{what}: {diff}"


@pytest.mark.parametrize("width,height,tile,n", CASES, ids=IDS)
def test_a_tile_share_is_the_single_device_geometry_gathered(twk, single, width, height, tile, n):
    app, devs = _handles(twk, width, height, tile, n)
    padding = 0
    for i, d in enumerate(devs):
        d.renderGeometryTile()
        want = _gathered(twk, single[(width, height)], tile, n, i, d.launchWidth)
        _same(lc._words(d.readGeometry()), want, f"handle {i} of {n}")
        padding += int(lc.padding_mask(twk, lc.Shape(width, height, tile, 1), i, n).sum())
    assert padding == n * devs[0].launchWidth * height - width * height
    assert padding > 0 or (width, height) == (64, 16)
    _close(app, devs)


@pytest.mark.parametrize("stage", [False, True], ids=["direct", "staged"])
@pytest.mark.parametrize("width,height,tile,n", CASES, ids=IDS)
def test_the_assembly_with_geometry_is_the_single_device_geometry(twk, single, width, height, tile, n, stage, monkeypatch):
    if stage:
        monkeypatch.setenv("TWK_ASSEMBLE_STAGE", "1")  # read when a handle is created
    app, devs = _handles(twk, width, height, tile, n, render=2)
    for d in devs:
        d.renderGeometryTile()
    primary, other = devs[0], devs[1]
    primary.assembleWithGeometry(devs[::-1], ())  # any order; the geometry alone
    _same(lc._words(primary.readAssembledGeometry()), single[(width, height)], "planes=()")
    ptr, nbytes = primary.assembledGeometryDevicePointer()
    assert ptr and nbytes == width * height * 16
    with pytest.raises(twk.TwkError):
        primary.readAssembled(OUTPUT)  # no plane was asked for
    # all six planes beside it, against assemble() on another primary: other buffers, the same bytes
    other.assemble(devs, PLANES)
    primary.assembleWithGeometry(devs, PLANES)
    for p in PLANES:
        _same(lc._words(primary.readAssembled(p)), lc._words(other.readAssembled(p)), f"plane {p}")
    assert lc._words(primary.readAssembled(OUTPUT)).any()
    _same(lc._words(primary.readAssembledGeometry()), single[(width, height)], "beside six planes")
    with pytest.raises(twk.TwkError):
        other.readAssembledGeometry()  # assemble() does not assemble the geometry
    _close(app, devs)


def test_the_explicit_form_on_a_gathered_block(twk, single):
    width, height, tile, n = 61, 37, (8, 8), 3
    app, devs = _handles(twk, width, height, tile, n, render=2)
    geometry, moments = [], []
    for d in devs:
        d.renderGeometryTile()
        geometry.append(d.readGeometry())
        moments.append(d.readMoments())
    block = {"g": np.ascontiguousarray(np.stack(geometry)), "m": np.ascontiguousarray(np.stack(moments))}
    buffers = {k: _DeviceBuffer(twk, a.nbytes) for k, a in block.items()}
    for k, a in block.items():
        buffers[k].upload(a)
    stride = block["g"].nbytes // n
    at = lambda k, d: buffers[k].ptr.value + d * stride
    primary = devs[0]
    primary.assembleFromWithGeometry([], [at("g", d) for d in range(n)], ())
    _same(lc._words(primary.readAssembledGeometry()), single[(width, height)], "gathered block, geometry alone")
    primary.assemble(devs, (MOMENTS,))
    want = lc._words(primary.readAssembled(MOMENTS))
    last = devs[-1]  # another primary, the same block
    last.assembleFromWithGeometry([{MOMENTS: at("m", d)} for d in range(n)], [at("g", d) for d in range(n)], (MOMENTS,))
    _same(lc._words(last.readAssembledGeometry()), single[(width, height)], "gathered block, beside the moments")
    _same(lc._words(last.readAssembled(MOMENTS)), want, "gathered block, moments")
    last.synchronizeStream()
    for b in buffers.values():
        b.free()
    _close(app, devs)


def test_on_one_device_it_is_render_geometry(twk, single):
    shape = lc.Shape(61, 37, (8, 8), 1)
    app = lc.make_app(twk, load_app, shape)
    dev = lc.new_device(twk, app, shape)
    dev.renderGeometryTile()
    _same(lc._words(dev.readGeometry()), single[(61, 37)], "one device")
    dev.assembleWithGeometry([dev], ())
    _same(lc._words(dev.readAssembledGeometry()), single[(61, 37)], "one device, assembled: the identity")
    # distribution 0 with several devices: every handle holds the whole frame, and the call is twk_render_geometry too
    whole = lc.new_device(twk, app, lc.Shape(61, 37, (8, 8), 0), index=1, count=2)
    whole.renderGeometryTile()
    _same(lc._words(whole.readGeometry()), single[(61, 37)], "distribution 0")
    whole.close()
    dev.close()
    app.close()


def _refused(twk, code, call, *words):
    with pytest.raises(twk.TwkError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def _moved(twk, app, dphi):
    i = app.info
    return twk.camera_frustum(tuple(i.center), i.phi + dphi, i.theta, i.fov, i.distance, i.resolution[0] / i.resolution[1])


def test_refusals(twk):
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    shape = lc.Shape(61, 37, (8, 8), 1)
    app, (a, b) = _handles(twk, 61, 37, (8, 8), 2)
    pair = [a, b]
    name, explicit = "twk_assemble_devices_with_geometry", "twk_assemble_with_geometry"
    # what the existing calls refuse stays refused
    _refused(twk, STATE, a.renderGeometry, "twk_render_geometry:", "packed tile")
    _refused(twk, VALUE, lambda: a.assemble(pair, ()), "twk_assemble_devices:", "mask")
    # nothing assembled yet, and no geometry rendered yet
    _refused(twk, STATE, a.readAssembledGeometry, "twk_read_assembled_geometry", "not been assembled")
    _refused(twk, STATE, a.assembledGeometryDevicePointer, "twk_get_assembled_geometry_device_pointer", "not been assembled")
    _refused(twk, STATE, lambda: a.assembleWithGeometry(pair, ()), name, "twk_render_geometry_tile")
    a.renderGeometryTile()
    _refused(twk, STATE, lambda: a.assembleWithGeometry(pair, ()), name, "index 1", "twk_render_geometry_tile")
    b.renderGeometryTile()
    a.assembleWithGeometry(pair, ())
    # the plane mask: 0 is legal here, an unknown plane is not; the handle list as in twk_assemble_devices
    handles = (C.c_void_p * 2)(a.handle.value, b.handle.value)
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble_devices_with_geometry(a.handle, C.c_uint(1 << 6), handles, 2)), name, "unknown plane")
    _refused(twk, VALUE, lambda: a.assembleWithGeometry([a], ()), name, "count")
    _refused(twk, VALUE, lambda: a.assembleWithGeometry([a, a], ()), name, "exactly once")
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble_devices_with_geometry(a.handle, C.c_uint(0), (C.c_void_p * 2)(a.handle.value, None), 2)), name, "NULL")
    # a handle with another camera: its share would be of another view
    b.updateCamera(0, _moved(twk, app, 0.004))
    _refused(twk, STATE, lambda: a.assembleWithGeometry(pair, ()), name, "index 1", "twk_render_geometry_tile")  # its geometry is stale first
    b.renderGeometryTile()
    _refused(twk, VALUE, lambda: a.assembleWithGeometry(pair, ()), name, "camera 0", "index 1")
    a.readAssembledGeometry()  # the primary's camera did not change: what it assembled stands
    b.updateCamera(0, app.cameras[0])
    b.renderGeometryTile()
    a.assembleWithGeometry(pair, ())
    # whatever clears the primary's geometry marks the assembled geometry stale: camera, state, scene
    a.updateCamera(0, app.cameras[0])
    _refused(twk, STATE, a.readAssembledGeometry, "twk_read_assembled_geometry", "camera")
    _refused(twk, STATE, a.assembledGeometryDevicePointer, "twk_get_assembled_geometry_device_pointer")
    _refused(twk, STATE, lambda: a.assembleWithGeometry(pair, ()), name, "index 0")
    a.renderGeometryTile()
    a.assembleWithGeometry(pair, ())
    a.setState(lc.state_of(app, shape))
    _refused(twk, STATE, a.readAssembledGeometry, "twk_read_assembled_geometry")
    a.renderGeometryTile()
    a.assembleWithGeometry(pair, ())
    a.readAssembledGeometry()
    # the geometry switched off on a handle, and on the primary
    b.enableGeometry(False)
    _refused(twk, STATE, lambda: a.assembleWithGeometry(pair, ()), name, "twk_enable_geometry", "every handle")
    _refused(twk, STATE, b.renderGeometryTile, "twk_render_geometry_tile:", "twk_enable_geometry")
    b.enableGeometry(True)
    a.enableGeometry(False)
    _refused(twk, STATE, lambda: a.assembleWithGeometry(pair, ()), name, "twk_enable_geometry", "primary")
    _refused(twk, STATE, lambda: a.assembleFromWithGeometry([], [4096, 4096], ()), explicit, "twk_enable_geometry", "primary")
    a.enableGeometry(True)
    # the explicit form
    _refused(twk, VALUE, lambda: a.assembleFromWithGeometry([], [4096, None], ()), explicit, "NULL geometry source", "device 1")
    _refused(twk, VALUE, lambda: a.assembleFromWithGeometry([], [4096], ()), explicit, "deviceCount")
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble_with_geometry(a.handle, C.c_uint(0), None, None, 2)), explicit, "NULL geometry sources")
    _refused(twk, VALUE, lambda: L.check(L.lib.twk_assemble_with_geometry(a.handle, C.c_uint(1), None, (C.c_void_p * 2)(4096, 4096), 2)), explicit, "NULL sources")
    _refused(twk, VALUE, lambda: a.assembleFromWithGeometry([{OUTPUT: 4096}, {}], [4096, 4096], (OUTPUT,)), explicit, "NULL source of TWK_PLANE_OUTPUT")
    # twk_render_geometry_tile's own: the lens, and a handle before its state and scene
    st = lc.state_of(app, shape)
    st.lensShader = 1
    b.setState(st)
    _refused(twk, STATE, b.renderGeometryTile, "twk_render_geometry_tile:", "pinhole")
    fresh = twk.Device(ordinal=0, index=1, count=2, miss=app.info.miss)
    fresh.enableGeometry(True)
    _refused(twk, STATE, fresh.renderGeometryTile, "twk_render_geometry_tile:", "twk_build")
    _refused(twk, STATE, lambda: a.assembleWithGeometry([fresh, a], ()), name, "twk_set_state")
    fresh.close()
    a.synchronizeStream()
    _close(app, pair)


def test_a_resize_drops_the_assembled_geometry_and_the_next_assembly_is_a_fresh_pairs(twk, single):
    """After twk_set_state with another resolution the getters refuse until the next assembly with geometry; that one gives what the
    single device gives at the new size."""
    before, after = lc.Shape(96, 64, (8, 8), 1), lc.Shape(61, 37, (8, 8), 1)
    app_before, app_after = lc.make_app(twk, load_app, before), lc.make_app(twk, load_app, after)
    devs = [lc.new_device(twk, app_before, before, index=i, count=2) for i in range(2)]
    for d in devs:
        d.render(0)
        d.renderGeometryTile()
    devs[0].assembleWithGeometry(devs, (OUTPUT,))
    assert devs[0].readAssembledGeometry().shape == (64, 96, 4)
    for d in devs:
        lc.move(d, app_after, after)
    STATE = twk._lib.TWK_ERROR_INVALID_STATE
    _refused(twk, STATE, devs[0].readAssembledGeometry, "not been assembled")
    _refused(twk, STATE, devs[0].assembledGeometryDevicePointer, "not been assembled")
    _refused(twk, STATE, lambda: devs[0].assembleWithGeometry(devs, ()), "twk_render_geometry_tile")
    for d in devs:
        d.render(0)
        d.renderGeometryTile()
    devs[0].assembleWithGeometry(devs, (OUTPUT,))
    _same(lc._words(devs[0].readAssembledGeometry()), single[(61, 37)], "the resized pair")
    assert devs[0].assembledGeometryDevicePointer()[1] == 61 * 37 * 16
    for d in devs:
        d.close()
    app_before.close()
    app_after.close()
