"""-m gpu: a device-pointer source for a geometry's vertices (twk_update_geometry_vertices_device, twk_refit_geometry_vertices_device;
csrc/vertex_source_device.h). The contract: after a _device call the handle equals, byte for byte, a handle that was given the same
records through the host call of the same name — so every test here runs two handles side by side and compares everything a reader
can get at: the acceleration structure and scene arrays (tests/scene_snapshot.py), the three kept arrays, the geometries' records
(twk_read_geometry_vertices), build / update / refit info apart from their milliseconds, pictures, the previous-position plane.
  1. attributes mode against the host call: refit, and update in selective and in full mode; a 32 x 18 picture at 2 spp in both formats
  2. positions mode against the host call given vertex_frames_host's records (recomputeFrames 1) or the old records with the new
     positions (0): from a contiguous tensor, stride-16 and stride-32 views of wider tensors, and a view with an offset
  3. the mirror: twk_build after a device refit; a host call after a device call; A -> B -> A; the built vertices change no byte
  4. the temporal history: the previous-position plane and the own-buffer merge; the oldest positions are kept whichever call made them
  5. every refusal, the handle unchanged after each
  6. tests/bvh_audit.py, whole, on a device-refit scene.
Scenes: tests/refit_scenes.py's meshes; the geometries of 1, 2, 65, 257 and 1025 build primitives are the ones deformed (65 and 257
vertices straddle a wave and a block of the per-vertex kernels), flattened and entered, both build qualities. Device memory comes from
torch.empty(..., device="cuda")."""
import ctypes as C

import numpy as np
import pytest

import bvh_audit as A
import lifecycle as lc
import refit_scenes as RS
import scene_snapshot as snapshot
import vertex_source_restate as V
from test_gpu_selective_update import _assert_same, _structure

pytestmark = pytest.mark.gpu

QUALITIES = pytest.mark.parametrize("quality", [1, 0], ids=["sah", "lbvh"])
KINDS = pytest.mark.parametrize("kind", RS.KINDS)
F32, U32 = np.float32, np.uint32
DEFORMED = (0, 1, 5, 6, 7)  # refit_scenes.SIZES: 1, 2, 65, 257 and 1025 build primitives
WIDTH, HEIGHT, SPP = 32, 18, 2


@pytest.fixture(scope="module")
def torch(twk):
    """torch beside the library in one process. A process can hold one HIP runtime: the library has loaded the system's (soname
    libamdhip64.so.7), while a torch wheel asks for its bundled copy by file name (libamdhip64.so) and would bring a second one, which
    finds no GPU. Opening the loaded runtime once more under the file names gives it those names, and torch then binds to it — the
    mirror image of bench.py, which imports torch first so that the library binds to torch's."""
    import sys
    if "torch" not in sys.modules:
        for name in ("libamdhip64.so", "libhsa-runtime64.so", "libamd_comgr.so", "librocprofiler-register.so"):
            try:
                C.CDLL(name, mode=C.RTLD_GLOBAL)
            except OSError:
                pass  # not on the loader's path: torch brings its own
    import torch as t
    assert t.cuda.is_available(), "torch sees no GPU beside the library"
    return t


def _handle(twk, kind, quality, selective=True, half=False, geometries=None):
    """A handle on the meshes of refit_scenes (or `geometries` in their place) with a camera on the largest of them."""
    st = twk.DeviceState()
    st.resolution[0], st.resolution[1] = WIDTH, HEIGHT
    st.tileSize[0], st.tileSize[1] = 8, 8
    st.pathLengths[0], st.pathLengths[1] = 1, 2
    st.distribution, st.samplesSqrt, st.lensShader = 0, 1, 0
    st.epsilonFactor, st.envRotation, st.clockFactor = 500.0, 0.0, 1000.0
    cam = twk.camera_frustum((21.0, 0.0, 0.0), 0.75, 0.5, 50.0, 0.8, WIDTH / HEIGHT)  # on the mesh of 1025 quads, 0.4 wide, at bvh_audit_scenes.place(7)
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
    dev.enableMoments(True)
    dev.enableGeometry(True)
    dev.setState(st)
    dev.initCameras([cam])
    dev.initLights([light])
    dev.initMaterials([m])
    if half:
        dev.setOutputFormat(lc.HALF4)
    dev.setBuildQuality(quality)
    dev.setFlattenPolicy(*RS.POLICY)
    dev.setUpdateMode(twk._lib.TWK_UPDATE_SELECTIVE if selective else twk._lib.TWK_UPDATE_FULL)
    for a, i in (geometries or RS.meshes()):
        dev.addGeometry(a, i)
    for g, t in RS.instances(kind):
        dev.addInstance(g, t, 0)
    dev.build()
    return dev


def _counts():
    return [np.asarray(a).reshape(-1, 12).shape[0] for a, _ in RS.meshes()]


def _state(twk, orc, dev, kept=True):
    out = _structure(twk, orc, dev)[0]
    if kept:
        wide, cost, flags = dev.debugReadKeptBuild()
        # the cost of a node no tree uses (both child words 0: a tree over pairs has fewer nodes than its triangles reserve) is never
        # written by any build — it is what the allocation held — so two handles are compared on the nodes that are used
        used = out["binaryNodes"][:cost.shape[0], 12:14].any(1)
        out["keptWide"], out["keptCost"], out["keptFlags"] = lc._words(wide), np.where(used, lc._words(cost).reshape(-1), 0), flags.astype(np.int64)
    for g, n in enumerate(_counts()):
        out[f"vertices {g}"] = lc._words(dev.readGeometryVertices(g, n))
    out["deformed"] = np.array([dev.geometryDeformed(g) for g in range(len(_counts()))], np.int64)
    return out


def _picture(dev, half):
    dev.setSampleOffset(0)
    for it in range(SPP):
        dev.render(it)
    dev.renderGeometry()
    geometry = dev.readGeometry()
    assert (geometry[..., 3].view(U32) != 0).mean() > 0.02, "the camera sees the mesh"
    return {"colour": lc._words(dev.getOutputBufferHalf() if half else dev.getOutputBufferHost()), "geometry": lc._words(geometry)}


def _info(d, drop=("milliseconds",)):
    return {k: v for k, v in d.items() if k not in drop}


def _tensor(torch, array):
    """`array` in device memory from torch.empty."""
    a = np.ascontiguousarray(array, F32)
    t = torch.empty(a.shape, dtype=torch.float32, device="cuda")
    t.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()  # the stream rule: the source is finished before the call
    return t


def _noise(g, seed):
    return RS.deform(RS.meshes()[g][0], "noise", seed=10 * seed + g)


@QUALITIES
@KINDS
def test_attributes_mode_equals_the_host_call(twk, orc, torch, kind, quality):
    """1, the refit: infos after every call, everything after the last, the picture in both formats."""
    for half in (False, True):
        host, device = _handle(twk, kind, quality, half=half), _handle(twk, kind, quality, half=half)
        try:
            for g in DEFORMED:
                b = _noise(g, 1)
                source = _tensor(torch, b)
                host.refitGeometryVertices(g, b)
                device.refitGeometryVerticesDevice(g, source)
                assert _info(device.refitInfo()) == _info(host.refitInfo()) and _info(device.updateInfo()) == _info(host.updateInfo()), g
                assert _info(device.buildInfo(), ("buildMilliseconds",)) == _info(host.buildInfo(), ("buildMilliseconds",)), g
                source.zero_()  # consumed on return: the caller may overwrite it
            torch.cuda.synchronize()
            if not half:
                _assert_same(_state(twk, orc, device), _state(twk, orc, host), f"{kind}: a refit from device records")
            _assert_same(_picture(device, half), _picture(host, half), f"{kind}: the picture after it, half {half}")
        finally:
            host.close()
            device.close()


@QUALITIES
@KINDS
@pytest.mark.parametrize("selective", [True, False], ids=["selective", "full"])
def test_an_update_in_attributes_mode_equals_the_host_call(twk, orc, torch, kind, quality, selective):
    """1, twk_update_geometry_vertices_device in both modes: infos after every call, everything after the last, the picture in both formats."""
    for half in (False, True):
        host, device = _handle(twk, kind, quality, selective, half=half), _handle(twk, kind, quality, selective, half=half)
        try:
            for g in DEFORMED:
                b = _noise(g, 2)
                host.updateGeometryVertices(g, b)
                device.updateGeometryVerticesDevice(g, _tensor(torch, b))
                assert _info(device.updateInfo()) == _info(host.updateInfo()), g
                assert _info(device.buildInfo(), ("buildMilliseconds",)) == _info(host.buildInfo(), ("buildMilliseconds",)), g
            if not half:
                _assert_same(_state(twk, orc, device, kept=selective), _state(twk, orc, host, kept=selective), f"{kind}: an update from device records")
            _assert_same(_picture(device, half), _picture(host, half), f"{kind}: the picture after it, half {half}")
        finally:
            host.close()
            device.close()


LAYOUTS = {"contiguous": (3, 0), "stride 16": (4, 0), "stride 32": (8, 0), "offset 8, stride 32": (8, 2)}  # floats per row, first float


def _layout(torch, positions, name):
    """positions [n, 3] in device memory as layout `name`: a view of a wider tensor whose other floats are NaN (they are never read)."""
    width, first = LAYOUTS[name]
    wide = np.full((positions.shape[0], width), np.nan, F32)
    wide[:, first:first + 3] = positions
    view = _tensor(torch, wide)[:, first:first + 3]
    assert view.stride(0) == width and view.storage_offset() == first
    return view


@QUALITIES
@KINDS
@pytest.mark.parametrize("recompute", [1, 0], ids=["frames", "positions only"])
def test_positions_mode_equals_the_host_call_given_the_host_forms_records(twk, orc, torch, kind, quality, recompute):
    """2: per layout every deformed geometry gets new positions; the host handle gets vertex_frames_host's records (or the old records
    with the new positions), and the device handle's records read back are those, bit for bit."""
    counts = _counts()
    host, device = _handle(twk, kind, quality), _handle(twk, kind, quality)
    try:
        for step, layout in enumerate(LAYOUTS):
            for call, refit in enumerate((True, False)):  # every layout through the refit and through the update
                for g in DEFORMED:
                    indices = RS.meshes()[g][1]
                    before = device.readGeometryVertices(g, counts[g])
                    positions = _noise(g, 3 + 2 * step + call)[:, 0:3]
                    want = twk.vertex_frames_host(positions, indices, before) if recompute else V.positions_only(positions, before)
                    view = _layout(torch, positions, layout)
                    if refit:
                        device.refitGeometryVerticesDevice(g, view, recomputeFrames=bool(recompute))
                        host.refitGeometryVertices(g, want)
                        assert _info(device.refitInfo()) == _info(host.refitInfo()), (layout, g)
                    else:
                        device.updateGeometryVerticesDevice(g, view, recomputeFrames=bool(recompute))
                        host.updateGeometryVertices(g, want)
                    assert _info(device.updateInfo()) == _info(host.updateInfo()), (layout, g)
                    got = device.readGeometryVertices(g, counts[g])
                    assert np.array_equal(got.view(U32), want.view(U32)), f"{layout}, geometry {g}: {np.nonzero((got.view(U32) != want.view(U32)).any(1))[0][:4]}"
                    if recompute:
                        assert not np.array_equal(got[:, 6:9], before[:, 6:9]) or counts[g] < 3, "the normals follow"
                _assert_same(_state(twk, orc, device), _state(twk, orc, host), f"{kind}: positions, {layout}, {'refit' if refit else 'update'}")
        _assert_same(_picture(device, False), _picture(host, False), f"{kind}: the picture")
    finally:
        host.close()
        device.close()


@QUALITIES
@KINDS
def test_the_mirror(twk, orc, torch, kind, quality):
    """3."""
    geometries = list(RS.meshes())
    new = [(_noise(g, 4), i) if g in DEFORMED else (a, i) for g, (a, i) in enumerate(geometries)]
    device, fresh, fresh_new = _handle(twk, kind, quality), _handle(twk, kind, quality), _handle(twk, kind, quality, geometries=new)
    host = _handle(twk, kind, quality)
    try:
        built = _state(twk, orc, device)
        _assert_same(built, _state(twk, orc, fresh), "two handles on one scene")
        # a refit with the vertices the trees were built from changes no byte
        for g in DEFORMED:
            device.refitGeometryVerticesDevice(g, _tensor(torch, geometries[g][0]))
        _assert_same(_state(twk, orc, device), built, f"{kind}: a device refit with the built vertices")
        picture = _picture(fresh, False)
        # A -> B -> A
        for vertices in (new, geometries):
            for g in DEFORMED:
                device.refitGeometryVerticesDevice(g, _tensor(torch, vertices[g][0]))
        _assert_same(_state(twk, orc, device), built, f"{kind}: there and back by device source")
        _assert_same(_picture(device, False), picture, f"{kind}: the picture there and back")
        # twk_build after a device refit to B: the mirror is refreshed, the build is a fresh build of B
        for g in DEFORMED:
            device.refitGeometryVerticesDevice(g, _tensor(torch, new[g][0]))
        device.build()
        _assert_same(_state(twk, orc, device), _state(twk, orc, fresh_new), f"{kind}: twk_build after a device refit")
        # a host call after a device call equals the host-only sequence, from the same build: B by device then C by host, against B and C by host
        for g in DEFORMED:
            b, c = new[g][0], _noise(g, 5)
            host.refitGeometryVerticesDevice(g, _tensor(torch, b))
            host.refitGeometryVertices(g, c)
            fresh.refitGeometryVertices(g, b)
            fresh.refitGeometryVertices(g, c)
            assert _info(host.refitInfo()) == _info(fresh.refitInfo()), g
        _assert_same(_state(twk, orc, host), _state(twk, orc, fresh), f"{kind}: a host refit after a device refit")
        # ... and a host UPDATE after a device refit, in positions mode (the mirror is stale when the host call comes)
        for g in DEFORMED:
            a = np.asarray(geometries[g][0], F32).reshape(-1, 12)
            host.refitGeometryVerticesDevice(g, _tensor(torch, a[:, 0:3]))
            host.updateGeometryVertices(g, a)
            fresh.updateGeometryVertices(g, a)
        _assert_same(_state(twk, orc, host), _state(twk, orc, fresh), f"{kind}: a host update after a device refit")
    finally:
        for d in (device, fresh, fresh_new, host):
            d.close()


TEMPORAL = dict(maxHistory=32, positionTolerance=0.1)


def _frame(dev, tp, frame):
    """One frame of a viewer: SPP samples, the geometry AOV with the previous-position plane, the own-buffer merge. Returns the plane
    and the merge's outputs as words."""
    dev.setSampleOffset(SPP * frame)
    for it in range(SPP):
        dev.render(it)
    dev.renderGeometryMotion()
    plane = lc._words(dev.readPreviousPositions())
    dev.temporalAccumulate(tp)
    return {"plane": plane, "temporal": lc._words(dev.readTemporal()), "moments": lc._words(dev.readTemporalMoments())}


def _apply(torch, dev, how, g, vertices):
    if how == "h":
        dev.refitGeometryVertices(g, vertices)
    elif how == "d":
        dev.refitGeometryVerticesDevice(g, _tensor(torch, vertices))
    elif how == "p":  # positions only: the records keep their frames, so the host call's records are these
        dev.refitGeometryVerticesDevice(g, _tensor(torch, vertices[:, 0:3]))
    else:
        dev.updateGeometryVerticesDevice(g, _tensor(torch, vertices))  # "u": a rebuild from device records


def _sequence(twk, torch, kind, quality, calls):
    """A history, then per deformed geometry the calls of `calls` (one letter each: _apply) with successive deformations, then a
    second frame: what it returns of both frames, and which geometries counted as deformed in between."""
    tp = twk._lib.Temporal(**TEMPORAL)
    dev = _handle(twk, kind, quality)
    try:
        first = _frame(dev, tp, 0)
        for g in DEFORMED:
            for k, how in enumerate(calls):
                _apply(torch, dev, how, g, _noise(g, 6 + k))
                assert dev.geometryDeformed(g)
        assert not dev.geometryDeformed(2)
        second = _frame(dev, tp, 1)
        assert not any(dev.geometryDeformed(g) for g in DEFORMED), "the merge swapped the history"
        third = _frame(dev, tp, 2)  # nothing is deformed any more: the plane is the geometry AOV's positions again
        return {f"{name} {k}": v for k, f in enumerate((first, second, third)) for name, v in f.items()}
    finally:
        dev.close()


@QUALITIES
@KINDS
def test_the_temporal_history(twk, torch, kind, quality):
    """4: one device refit against one host refit; two updates between two merges keep the positions of before the first, whichever
    call made each — device and device, host then device, device then host; a positions-only source and a device update run too."""
    references = {}
    for calls, against in (("d", "h"), ("dd", "hh"), ("hd", "hh"), ("dh", "hh"), ("pu", None)):
        got = _sequence(twk, torch, kind, quality, calls)
        if against is not None:
            if against not in references:
                references[against] = _sequence(twk, torch, kind, quality, against)
            _assert_same(got, references[against], f"{kind}: the calls {calls} against {against}")
        assert not np.array_equal(got["plane 1"], got["plane 2"]), "the deformation shows in the plane"


@QUALITIES
def test_refusals(twk, orc, torch, quality):
    """5: each refusal under the call's own name, the handle's state unchanged after every one."""
    L = twk._lib
    VALUE, STATE = L.TWK_ERROR_INVALID_VALUE, L.TWK_ERROR_INVALID_STATE
    G = 6  # the soup of 257 triangles
    records = np.asarray(RS.meshes()[G][0], F32).reshape(-1, 12)
    n = records.shape[0]
    good = _tensor(torch, records)
    positions = _tensor(torch, records[:, 0:3])

    def raw(dev, name, source, count=n, geometry=G):
        return getattr(L.lib, name)(dev.handle if dev is not None else None, geometry, None if source is None else C.byref(source), C.c_size_t(count))

    def source(**fields):
        s = L.VertexSource()
        for k, v in fields.items():
            if k == "reserved":
                s.reserved[v] = 1
            else:
                setattr(s, k, v)
        return s

    for selective in (True, False):
        dev = _handle(twk, "flat", quality, selective)
        try:
            before = _state(twk, orc, dev, kept=selective)
            for name in ("twk_refit_geometry_vertices_device", "twk_update_geometry_vertices_device"):
                def refused(code, rc, *words):
                    text = L.lib.twk_last_error().decode()
                    assert rc == code and text.startswith(name + ": "), (rc, text)
                    for w in words:
                        assert w in text, text

                ok = source(attributes=good.data_ptr())
                if name.startswith("twk_refit") and not selective:
                    refused(STATE, raw(dev, name, ok), "TWK_UPDATE_SELECTIVE")
                    continue
                refused(VALUE, raw(None, name, ok), "NULL device handle")
                refused(VALUE, raw(dev, name, None), "NULL source")
                refused(VALUE, raw(dev, name, ok, geometry=len(RS.SIZES)), "bad geometry id")
                refused(VALUE, raw(dev, name, ok, geometry=-1), "bad geometry id")
                refused(VALUE, raw(dev, name, ok, count=n - 1), "vertices")
                refused(VALUE, raw(dev, name, source()), "exactly one")
                refused(VALUE, raw(dev, name, source(attributes=good.data_ptr(), positions=positions.data_ptr())), "exactly one")
                for stride in (8, 14, 4):
                    refused(VALUE, raw(dev, name, source(positions=positions.data_ptr(), positionStride=stride)), "positionStride")
                refused(VALUE, raw(dev, name, source(attributes=good.data_ptr(), positionStride=48)), "positionStride")
                refused(VALUE, raw(dev, name, source(attributes=good.data_ptr(), recomputeFrames=1)), "recomputeFrames")
                refused(VALUE, raw(dev, name, source(positions=positions.data_ptr(), recomputeFrames=2)), "recomputeFrames")
                for word in range(3):
                    refused(VALUE, raw(dev, name, source(attributes=good.data_ptr(), reserved=word)), "reserved")
                refused(VALUE, raw(dev, name, source(attributes=good.data_ptr() + 4)), "aligned")
                refused(VALUE, raw(dev, name, source(positions=positions.data_ptr() + 2)), "aligned")
                # a plain host pointer: a numpy array's address. Nothing is dereferenced on the device.
                refused(VALUE, raw(dev, name, source(attributes=records.ctypes.data)), "not device or managed memory")
                refused(VALUE, raw(dev, name, source(positions=np.ascontiguousarray(records[:, 0:3]).ctypes.data)), "not device or managed memory")
                # a source whose allocation ends before the last vertex: ten records before the end of the segment torch holds the
                # tensor in (what hipMemGetAddressRange reports); refused before any launch, nothing is read
                big = torch.empty(20 << 18, dtype=torch.float32, device="cuda")
                segment = next(seg for seg in torch.cuda.memory_snapshot() if seg["address"] <= big.data_ptr() < seg["address"] + seg["total_size"])
                tail = segment["address"] + segment["total_size"] - 480
                refused(VALUE, raw(dev, name, source(attributes=tail)), "the allocation ends")
                refused(VALUE, raw(dev, name, source(positions=tail, positionStride=48)), "the allocation ends")
                del big
                # (a source that overlaps the handle's own attribute array is refused too; no call hands that pointer out, so no test can name it)
                # a position that is not finite: at vertex 0, at the last vertex, and at two places, where the text names the lower
                for bad, where in (((0, 0),), 0), (((n - 1, 2),), n - 1), (((200, 1), (77, 0)), 77):
                    for value in (np.nan, np.inf, -np.inf):
                        broken = records.copy()
                        for v, c in bad:
                            broken[v, c] = value
                        refused(VALUE, raw(dev, name, source(attributes=_tensor(torch, broken).data_ptr())), f"vertex {where}:", "finite")
                        refused(VALUE, raw(dev, name, source(positions=_tensor(torch, broken[:, 0:3]).data_ptr(), recomputeFrames=1)), f"vertex {where}:", "finite")
                # a NaN that is not a position is the caller's business, as in the host call
                for reader in ((dev.updateInfo, dev.refitInfo) if name.startswith("twk_refit") else (dev.updateInfo,)):
                    with pytest.raises(twk.TwkError) as e:
                        reader()
                    assert e.value.code == STATE, "a refused call is no refit and no update"
            _assert_same(_state(twk, orc, dev, kept=selective), before, "a refused call changes nothing")
            # the Python layer refuses what it can see before the call
            for wrong in (good[:, 0:5], good.double(), good[:, ::2][:, 0:3], good.reshape(-1)):
                with pytest.raises((ValueError, TypeError)):
                    dev.updateGeometryVerticesDevice(G, wrong)
            with pytest.raises(ValueError):
                dev.updateGeometryVerticesDevice(G, good, recomputeFrames=True)
        finally:
            dev.close()
    # a geometry with an instance that carries a light, and a handle that is not built
    dev = _handle(twk, "flat", quality)
    try:
        dev.clearScene()
        a, i = RS.meshes()[G]
        dev.addGeometry(a, i)
        dev.addInstance(0, RS.instances("flat")[0][1], 0, 0)
        for call, name in ((dev.refitGeometryVerticesDevice, "twk_refit_geometry_vertices_device"), (dev.updateGeometryVerticesDevice, "twk_update_geometry_vertices_device")):
            with pytest.raises(twk.TwkError) as e:
                call(0, good)
            assert e.value.code == STATE and name + ": twk_build" in str(e.value)
        dev.build()
        before = _structure(twk, orc, dev)[0]
        for call in (dev.refitGeometryVerticesDevice, dev.updateGeometryVerticesDevice):
            with pytest.raises(twk.TwkError) as e:
                call(0, good)
            assert e.value.code == VALUE and "instance 0" in str(e.value) and "light" in str(e.value)
        _assert_same(_structure(twk, orc, dev)[0], before, "a refused call changes nothing")
    finally:
        dev.close()


@QUALITIES
@KINDS
def test_a_device_refit_scene_passes_the_audit(twk, orc, torch, kind, quality):
    """6: the geometries of 65 and 1025 build primitives (and the other deformed ones) refit to the noise deformation from device
    positions with the frames recomputed; the scene the audit is given holds the records the handle reads back."""
    geometries, instances = list(RS.meshes()), RS.instances(kind)
    counts = _counts()
    dev = _handle(twk, kind, quality)
    try:
        for g in DEFORMED:
            dev.refitGeometryVerticesDevice(g, _tensor(torch, RS.deformed_meshes("noise")[g][0][:, 0:3]), recomputeFrames=True)
            geometries[g] = (dev.readGeometryVertices(g, counts[g]), geometries[g][1])
            assert np.array_equal(geometries[g][0][:, 0:3], RS.deformed_meshes("noise")[g][0][:, 0:3])
        after = snapshot.readback(twk, orc, dev)
    finally:
        dev.close()
    A.audit(A.Scene(geometries, instances, RS.POLICY, quality), after)
