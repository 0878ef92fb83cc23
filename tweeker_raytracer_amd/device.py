"""Device — Python mirror of rtigo3's per-GPU `Device` interface (reference inc/Device.h:292-404).

Method names follow the reference: initCameras/initLights/initMaterials/initScene-equivalents, setState,
render(iterationIndex), synchronizeStream, getOutputBufferHost. Every method is a direct call into the
C ABI; errors surface as TwkError (≙ the reference's std::runtime_error).
"""
import ctypes as C

import numpy as np

from . import _lib as L

KERNEL_CLASSES = ("generate", "trace", "shade", "accumulate", "tail")


def instance_motion(previous, current):
    """twk_instance_motion (pure CPU): the L.InstanceMotion record of an instance whose object-to-world matrix was `previous` when the
    history was taken and is `current` now (12 floats each, row-major 3 x 4). moved = 0 when the two are bit-equal. TwkError for an
    input that is not finite and for a singular `current`."""
    p = np.ascontiguousarray(previous, dtype=np.float32).reshape(12)
    c = np.ascontiguousarray(current, dtype=np.float32).reshape(12)
    out = L.InstanceMotion()
    L.check(L.lib.twk_instance_motion(p.ctypes.data_as(C.POINTER(C.c_float)), c.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)))
    return out


def light_moved_host(anchor, anchorTransform, transform):
    """twk_light_moved_host (pure CPU, csrc/light_motion.h): the L.LightDefinition that `anchor` — the definition of a parallelogram
    light whose instance had the object-to-world matrix anchorTransform — becomes when the instance is moved to `transform` (12 floats
    each, row-major 3 x 4). A transform with the anchor transform's bits returns the anchor's bytes. TwkError: a light that is no
    parallelogram, a transform that is not finite, a singular anchor transform, a degenerate result."""
    a = np.ascontiguousarray(anchorTransform, dtype=np.float32).reshape(12)
    t = np.ascontiguousarray(transform, dtype=np.float32).reshape(12)
    out = L.LightDefinition()
    L.check(L.lib.twk_light_moved_host(C.byref(anchor), a.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)))
    return out


def update_plan_host(instanceGeometry, geometryTriangles, flattenPolicy, moved=(), maxLeaf=2):
    """twk_update_plan_host (pure CPU): how a scene of instances instanceGeometry[i] over geometries of geometryTriangles[g]
    triangles is laid out under flattenPolicy = (maxTriangles, maxReferences), and what a selective update of the instances `moved`
    touches. Returns a dict: L.UpdatePlan's fields, `flattened` (bool per instance), `trees` (the moved flattened instances,
    ascending) and `ranges` ([(first node, count), ...]: the rebuilt trees, the top level, the two root slots)."""
    ig = np.ascontiguousarray(instanceGeometry, dtype=np.int32).reshape(-1)
    gt = np.ascontiguousarray(geometryTriangles, dtype=np.int32).reshape(-1)
    mv = np.ascontiguousarray(list(moved), dtype=np.int32).reshape(-1)
    plan = L.UpdatePlan()
    flattened = np.zeros(max(1, ig.size), np.uint8)
    trees = np.zeros(max(1, mv.size), np.int32)
    ranges = np.zeros(2 * (mv.size + 2), np.int32)
    ip = C.POINTER(C.c_int)
    L.check(L.lib.twk_update_plan_host(ig.ctypes.data_as(ip), int(ig.size), gt.ctypes.data_as(ip), int(gt.size), int(flattenPolicy[0]), int(flattenPolicy[1]), int(maxLeaf),
                                       mv.ctypes.data_as(ip) if mv.size else None, int(mv.size), C.byref(plan), flattened.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                       trees.ctypes.data_as(ip), ranges.ctypes.data_as(ip)))
    out = {name: getattr(plan, name) for name, _ in L.UpdatePlan._fields_}
    out["flattened"] = [bool(f) for f in flattened[:ig.size]]
    out["trees"] = [int(t) for t in trees[:plan.treesRebuilt]]
    out["ranges"] = [(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(plan.numRanges)]
    return out


def vertex_update_plan_host(instanceGeometry, geometryTriangles, flattenPolicy, updated=(), moved=(), maxLeaf=2):
    """twk_vertex_update_plan_host (pure CPU): update_plan_host with the geometries `updated` (new vertices) as well as the instances
    `moved`. `trees` lists a rebuilt bottom-level tree as ~geometry (negative) before the flattened instances; `ranges` has their node
    ranges in the same order, then the top level and the two root slots."""
    ig = np.ascontiguousarray(instanceGeometry, dtype=np.int32).reshape(-1)
    gt = np.ascontiguousarray(geometryTriangles, dtype=np.int32).reshape(-1)
    mv = np.ascontiguousarray(list(moved), dtype=np.int32).reshape(-1)
    up = np.ascontiguousarray(list(updated), dtype=np.int32).reshape(-1)
    plan = L.UpdatePlan()
    room = int(ig.size + gt.size + 2)
    flattened = np.zeros(max(1, ig.size), np.uint8)
    trees = np.zeros(room, np.int32)
    ranges = np.zeros(2 * room, np.int32)
    ip = C.POINTER(C.c_int)
    L.check(L.lib.twk_vertex_update_plan_host(ig.ctypes.data_as(ip), int(ig.size), gt.ctypes.data_as(ip), int(gt.size), int(flattenPolicy[0]), int(flattenPolicy[1]), int(maxLeaf),
                                              mv.ctypes.data_as(ip) if mv.size else None, int(mv.size), up.ctypes.data_as(ip) if up.size else None, int(up.size), C.byref(plan),
                                              flattened.ctypes.data_as(C.POINTER(C.c_ubyte)), trees.ctypes.data_as(ip), ranges.ctypes.data_as(ip)))
    out = {name: getattr(plan, name) for name, _ in L.UpdatePlan._fields_}
    out["flattened"] = [bool(f) for f in flattened[:ig.size]]
    out["trees"] = [int(t) for t in trees[:plan.treesRebuilt]]
    out["ranges"] = [(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(plan.numRanges)]
    return out


def refit_batch_plan_host(treeNodes, treeSlots):
    """twk_refit_batch_plan_host (pure CPU): how trees of treeNodes[k] nodes and treeSlots[k] slots share the launches of one batched
    refit (csrc/refit_batch_plan.h). Returns a dict: L.RefitBatchPlan's fields, nodeOffsets / slotOffsets / nodeBlockFirst /
    slotBlockFirst (int32 per tree) and nodeBlockTable / slotBlockTable (int32 [blocks, 2]: the block's tree, the tree-local index of its
    first thread)."""
    n = np.ascontiguousarray(treeNodes, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(treeSlots, dtype=np.int32).reshape(-1)
    if n.size != s.size:
        raise ValueError("refit_batch_plan_host: one node count and one slot count per tree")
    ip = C.POINTER(C.c_int)
    at = lambda a: a.ctypes.data_as(ip) if a.size else None
    plan = L.RefitBatchPlan()
    L.check(L.lib.twk_refit_batch_plan_host(at(n), at(s), int(n.size), C.byref(plan), None, None, None, None, None, None))  # the totals first
    per_tree = [np.zeros(n.size, np.int32) for _ in range(4)]
    nodeBlocks, slotBlocks = np.zeros((plan.nodeBlocks, 2), np.int32), np.zeros((plan.slotBlocks, 2), np.int32)
    L.check(L.lib.twk_refit_batch_plan_host(at(n), at(s), int(n.size), C.byref(plan), *[at(a) for a in per_tree], at(nodeBlocks), at(slotBlocks)))
    out = {name: getattr(plan, name) for name, _ in L.RefitBatchPlan._fields_}
    out.update(zip(("nodeOffsets", "slotOffsets", "nodeBlockFirst", "slotBlockFirst"), per_tree), nodeBlockTable=nodeBlocks, slotBlockTable=slotBlocks)
    return out


def scene_refit_plan_host(instanceGeometry, geometryTriangles, flattenPolicy, updated=(), moved=(), maxLeaf=2):
    """twk_scene_refit_plan_host (pure CPU): the batch of a refitScene call (csrc/refit_scene_plan.h) on a scene laid out as
    vertex_update_plan_host lays it out, for the geometries `updated` and the instances `moved`. Returns a dict: L.SceneRefitPlan's
    fields, per tree (int32) trees (~geometry for a bottom-level tree, else the instance), kinds (0, 1, 2), nodeBases, nodeCounts,
    slotBases, slotCounts, nodeOffsets, slotOffsets, nodeBlockFirst, slotBlockFirst, and nodeBlockTable / slotBlockTable (int32
    [blocks, 2]: the block's tree, the tree-local index of its first thread)."""
    ig = np.ascontiguousarray(instanceGeometry, dtype=np.int32).reshape(-1)
    gt = np.ascontiguousarray(geometryTriangles, dtype=np.int32).reshape(-1)
    mv = np.ascontiguousarray(list(moved), dtype=np.int32).reshape(-1)
    up = np.ascontiguousarray(list(updated), dtype=np.int32).reshape(-1)
    ip = C.POINTER(C.c_int)
    at = lambda a: a.ctypes.data_as(ip) if a.size else None
    plan = L.SceneRefitPlan()
    head = (at(ig), int(ig.size), at(gt), int(gt.size), int(flattenPolicy[0]), int(flattenPolicy[1]), int(maxLeaf), at(mv), int(mv.size), at(up), int(up.size), C.byref(plan))
    L.check(L.lib.twk_scene_refit_plan_host(*head, *([None] * 12)))  # the totals first
    names = ("trees", "kinds", "nodeBases", "nodeCounts", "slotBases", "slotCounts", "nodeOffsets", "slotOffsets", "nodeBlockFirst", "slotBlockFirst")
    count = plan.trees
    per_tree = [np.zeros(count, np.int32) for _ in names]
    nodeBlocks, slotBlocks = np.zeros((plan.nodeBlocks, 2), np.int32), np.zeros((plan.slotBlocks, 2), np.int32)
    L.check(L.lib.twk_scene_refit_plan_host(*head, *[at(a) for a in per_tree], at(nodeBlocks), at(slotBlocks)))
    out = {name: getattr(plan, name) for name, _ in L.SceneRefitPlan._fields_ if name != "trees"}
    out["numTrees"] = count
    out.update(zip(names, per_tree), nodeBlockTable=nodeBlocks, slotBlockTable=slotBlocks)
    return out


def previous_positions_host(hits, instance, primitive, geometry, indices, previousPositions, motion=None, carry=None):
    """twk_previous_positions_host (pure CPU): the previous-position plane of twk_render_geometry_motion from host arrays — hits
    float32 [n, 3] (t, beta, gamma), instance and primitive int32 [n] (instance < 0: a miss), geometry float32 [n, 4] (the geometry
    AOV), indices uint32, previousPositions float32 [m, 4], motion / carry: ctypes arrays of L.InstanceMotion / L.InstanceCarry indexed
    by instance (None: none). Returns float32 [n, 4]."""
    hits = np.ascontiguousarray(hits, dtype=np.float32).reshape(-1, 3)
    inst = np.ascontiguousarray(instance, dtype=np.int32).reshape(-1)
    prim = np.ascontiguousarray(primitive, dtype=np.int32).reshape(-1)
    geo = np.ascontiguousarray(geometry, dtype=np.float32).reshape(-1, 4)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    pos = np.ascontiguousarray(previousPositions, dtype=np.float32).reshape(-1, 4)
    if not (hits.shape[0] == inst.size == prim.size == geo.shape[0]):
        raise ValueError("previous_positions_host: one hit, instance, primitive and geometry element per pixel")
    out = np.empty((hits.shape[0], 4), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.check(L.lib.twk_previous_positions_host(hits.ctypes.data_as(fp), inst.ctypes.data_as(ip), prim.ctypes.data_as(ip), geo.ctypes.data_as(fp), C.c_size_t(hits.shape[0]),
                                              idx.ctypes.data_as(C.POINTER(C.c_uint)) if idx.size else None, C.c_size_t(idx.size), pos.ctypes.data_as(fp) if pos.size else None,
                                              C.c_size_t(pos.shape[0]), motion, int(len(motion)) if motion is not None else 0, carry, int(len(carry)) if carry is not None else 0,
                                              out.ctypes.data_as(fp)))
    return out


def refit_tree_host(nodes, wideNodes, nodeCost, slots, pairFlags, attributes, indices, nodeBase, slotBase, leafFlag=0, transform=None, idInstance=-1):
    """twk_refit_tree_host (pure CPU): the refit of ONE tree (csrc/bvh_refit.h) from host arrays, all the tree's own — nodes float32
    [n, 16], wideNodes float32 [n, 32], nodeCost float32 [n] or None, slots float32 [t, 12] (the primitive word of each is read),
    pairFlags int32 [t] or None, the geometry's attributes [v, 12] and indices; references are absolute (nodeBase, slotBase). leafFlag
    0x40000000: the world-space tree of instance idInstance under `transform`. Nothing given is changed. Returns a dict: nodes,
    wideNodes, nodeCost (or None), slots, shadeRecords float32 [t, 32], terms (sahInner, sahLeaf), rootBounds float32 [6]."""
    copy = lambda a, kind, row: np.array(a, dtype=kind).reshape(-1, row) if row else np.array(a, dtype=kind).reshape(-1)
    n, w, s = copy(nodes, np.float32, 16), copy(wideNodes, np.float32, 32), copy(slots, np.float32, 12)
    cost = None if nodeCost is None else copy(nodeCost, np.float32, 0)
    flags = None if pairFlags is None else np.ascontiguousarray(pairFlags, dtype=np.int32).reshape(-1)
    attrs = np.ascontiguousarray(attributes, dtype=np.float32).reshape(-1, 12)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    if w.shape[0] != n.shape[0] or (cost is not None and cost.size != n.shape[0]) or (flags is not None and flags.size != s.shape[0]):
        raise ValueError("refit_tree_host: one wide node and one cost per node, one pair flag per slot")
    shade = np.zeros((s.shape[0], 32), np.float32)
    terms, bounds = (C.c_double * 2)(), (C.c_float * 6)()
    t = None if transform is None else np.ascontiguousarray(transform, dtype=np.float32).reshape(12)
    fp = C.POINTER(C.c_float)
    L.check(L.lib.twk_refit_tree_host(n.ctypes.data_as(fp), w.ctypes.data_as(fp), None if cost is None else cost.ctypes.data_as(fp), s.ctypes.data_as(fp), shade.ctypes.data_as(fp),
                                      None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_int)), attrs.ctypes.data_as(C.c_void_p), C.c_size_t(attrs.shape[0]),
                                      idx.ctypes.data_as(C.POINTER(C.c_uint)), C.c_size_t(idx.size), int(nodeBase), int(n.shape[0]), int(slotBase), int(s.shape[0]), int(leafFlag),
                                      None if t is None else t.ctypes.data_as(fp), int(idInstance), terms, bounds))
    return {"nodes": n, "wideNodes": w, "nodeCost": cost, "slots": s, "shadeRecords": shade, "terms": (terms[0], terms[1]), "rootBounds": np.array(bounds, dtype=np.float32)}


def vertex_frames_host(positions, indices, before):
    """twk_vertex_frames_host (pure CPU): the records a positions-mode device source with recomputeFrames 1 leaves (csrc/
    vertex_source_device.h) — positions float32 [n, 3], indices uint32, before float32 [n, 12] (the geometry's records before the call).
    Returns float32 [n, 12]: vertex from positions, normal and tangent from the new positions, texcoord kept."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    old = np.ascontiguousarray(before, dtype=np.float32).reshape(-1, 12)
    if old.shape[0] != pos.shape[0]:
        raise ValueError("vertex_frames_host: one record per position")
    out = np.empty_like(old)
    L.check(L.lib.twk_vertex_frames_host(pos.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(pos.shape[0]), idx.ctypes.data_as(C.POINTER(C.c_uint)), C.c_size_t(idx.size),
                                         old.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def _vertex_source(source, numVertices, positions, stride, recomputeFrames):
    """(L.VertexSource, vertex count) of `source`: an integer device address (numVertices and, for positions, `positions=True` given),
    or an object with data_ptr() (a torch tensor) or __cuda_array_interface__ — float32 [n, 12] contiguous: records; float32 [n, 3]
    with unit stride along a row: positions, rows any multiple of 4 bytes >= 12 apart (a strided view is passed as it is, no copy)."""
    if isinstance(source, (int, np.integer)):
        if numVertices is None:
            raise ValueError("a device address needs numVertices")
        address, n, is_positions, row = int(source), int(numVertices), bool(positions), (0 if stride is None else int(stride))
    else:
        if hasattr(source, "data_ptr"):
            shape, item = tuple(source.shape), source.element_size()
            strides, address, kind = tuple(s * item for s in source.stride()), int(source.data_ptr()), str(source.dtype).split(".")[-1]
        elif hasattr(source, "__cuda_array_interface__"):
            cai = source.__cuda_array_interface__
            shape, item, address, kind = tuple(cai["shape"]), int(cai["typestr"][2:]), int(cai["data"][0]), {"<f4": "float32"}.get(cai["typestr"], cai["typestr"])
            strides = tuple(cai["strides"]) if cai.get("strides") else tuple(item * int(np.prod(shape[k + 1:])) for k in range(len(shape)))
        else:
            raise TypeError("a device vertex source is an address, or has data_ptr() or __cuda_array_interface__")
        if kind != "float32" or len(shape) != 2 or shape[1] not in (3, 12):
            raise ValueError(f"a device vertex source is float32 [n, 12] (records) or [n, 3] (positions), not {kind} {list(shape)}")
        if strides[1] != 4:
            raise ValueError(f"the floats of a vertex are 4 bytes apart, not {strides[1]}")
        n, is_positions, row = shape[0], shape[1] == 3, strides[0]
        if positions is not None and bool(positions) != is_positions:
            raise ValueError("positions= disagrees with the source's shape")
        if numVertices is not None and int(numVertices) != n:
            raise ValueError(f"numVertices {numVertices} is not the source's {n}")
        if is_positions and n > 1 and (row < 12 or row % 4):
            raise ValueError(f"positions are {row} bytes apart: at least 12 and a multiple of 4")
        if not is_positions and n > 1 and row != 48:
            raise ValueError(f"records are {row} bytes apart, not 48: pass a contiguous [n, 12] tensor")
        if stride is not None and is_positions and n > 1 and int(stride) != row:
            raise ValueError("stride= disagrees with the source's strides")
        row = row if is_positions and n > 1 else (0 if stride is None else int(stride))
    src = L.VertexSource()
    if is_positions:
        src.positions, src.positionStride, src.recomputeFrames = address, row, 1 if recomputeFrames else 0
    else:
        if recomputeFrames:
            raise ValueError("recomputeFrames goes with positions")
        src.attributes = address
    return src, n


def device_count():
    n = C.c_int(0)
    L.check(L.lib.twk_device_count(C.byref(n)))
    return n.value


def _as_array(ctype, items):
    items = list(items)
    arr = (ctype * max(1, len(items)))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr, len(items)


SHADE_BUILD_FLAGS = ("ENV", "TEX", "PRIMARY", "LDS_TABLES", "MEASURE", "SORT", "SLIM")  # bit 0 .. bit 6 of a shade launcher index


def shade_build_slots():
    """The launcher indices (0..127) that hold a build of the shade kernel (twk_debug_shade_build_slots); needs no GPU."""
    mask = (C.c_uint64 * 2)()
    L.check(L.lib.twk_debug_shade_build_slots(mask))
    return {i for i in range(128) if (mask[i >> 6] >> (i & 63)) & 1}


def shade_build_name(index):
    """'ENV|LDS_TABLES|SORT' for a launcher index; 'plain' for 0."""
    return "|".join(n for b, n in enumerate(SHADE_BUILD_FLAGS) if (index >> b) & 1) or "plain"


class Device:
    def __init__(self, ordinal=0, index=0, count=1, miss=1):
        self._h = C.c_void_p()
        self._cascadeLayers = 0  # layers of the last enableCascade (the shape readCascade returns)
        L.check(L.lib.twk_device_create(C.byref(self._h), int(ordinal), int(index), int(count), int(miss)))
        self.index, self.count, self.miss = index, count, miss
        self.state = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            L.lib.twk_device_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    # ---- state / scene ------------------------------------------------------------------------
    def setState(self, state):
        L.check(L.lib.twk_set_state(self._h, C.byref(state)))
        self.state = state
        # twk_set_state lets go of a shared frame that is too small for the new state: the readers are the packed buffer's again
        if getattr(self, "_sharedFrame", False) and self._sharedFrameBytes < state.resolution[0] * state.resolution[1] * (8 if self.outputFormat == L.TWK_OUTPUT_HALF4 else 16):
            self._sharedFrame = False

    def initCameras(self, cameras):
        arr, n = _as_array(L.CameraDefinition, cameras)
        L.check(L.lib.twk_init_cameras(self._h, arr, n))

    def initLights(self, lights):
        arr, n = _as_array(L.LightDefinition, lights)
        L.check(L.lib.twk_init_lights(self._h, arr, n))

    def initMaterials(self, materials):
        arr, n = _as_array(L.MaterialGUI, materials)
        L.check(L.lib.twk_init_materials(self._h, arr, n))

    def updateCamera(self, idCamera, camera):
        L.check(L.lib.twk_update_camera(self._h, int(idCamera), C.byref(camera)))

    def updateLight(self, idLight, light):
        L.check(L.lib.twk_update_light(self._h, int(idLight), C.byref(light)))

    # ---- moving a light (include/tweeker_hip.h "Moving a light", csrc/light_motion.h) ----
    def getLight(self, idLight):
        """twk_get_light: the light's definition as it is now, an L.LightDefinition."""
        out = L.LightDefinition()
        L.check(L.lib.twk_get_light(self._h, int(idLight), C.byref(out)))
        return out

    def enableEmitterMotion(self, on=True):
        """twk_enable_emitter_motion: while on, updateInstanceTransform[s], refitInstanceTransform[s] and refitScene's moved list accept
        an instance that carries a parallelogram light and move the light's definition with it, always derived from the light's anchor
        (light_moved_host). Off, the default: they refuse such an instance as they always did."""
        L.check(L.lib.twk_enable_emitter_motion(self._h, int(bool(on))))

    def emitterMotion(self):
        """twk_get_emitter_motion: whether the switch is on."""
        on = C.c_int(0)
        L.check(L.lib.twk_get_emitter_motion(self._h, C.byref(on)))
        return bool(on.value)

    def updateMaterial(self, idMaterial, material):
        L.check(L.lib.twk_update_material(self._h, int(idMaterial), C.byref(material)))

    def initTexture(self, slot, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        assert rgba.ndim == 3 and rgba.shape[2] == 4, "texture must be [height, width, 4] float32, row 0 = v 0"
        L.check(L.lib.twk_init_texture(self._h, int(slot), rgba.ctypes.data_as(C.POINTER(C.c_float)),
                                       int(rgba.shape[1]), int(rgba.shape[0])))

    def clearScene(self):
        L.check(L.lib.twk_clear_scene(self._h))

    def addGeometry(self, attributes, indices):
        """attributes: float32 [n, 12] (vertex, tangent, normal, texcoord); indices: uint32 [3 m]."""
        attributes = np.ascontiguousarray(attributes, dtype=np.float32).reshape(-1, 12)
        indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        gid = C.c_int(-1)
        L.check(L.lib.twk_add_geometry(self._h, attributes.ctypes.data_as(C.c_void_p), C.c_size_t(attributes.shape[0]),
                                       indices.ctypes.data_as(C.c_void_p), C.c_size_t(indices.shape[0]), C.byref(gid)))
        return gid.value

    def addInstance(self, idGeometry, transform, idMaterial, idLight=-1):
        t = (C.c_float * 12)(*[float(x) for x in np.asarray(transform, dtype=np.float32).reshape(12)])
        iid = C.c_int(-1)
        L.check(L.lib.twk_add_instance(self._h, int(idGeometry), t, int(idMaterial), int(idLight), C.byref(iid)))
        return iid.value

    def setSharedFrame(self, dptr, nbytes):
        """Accumulate into a shared full W x H frame (ZeroCopy / PeerAccess strategies); 0 returns to the packed buffer."""
        L.check(L.lib.twk_set_shared_frame(self._h, C.c_void_p(int(dptr)), C.c_size_t(int(nbytes))))
        self._sharedFrame, self._sharedFrameBytes = bool(dptr), int(nbytes)

    def setShaderVariant(self, variant):
        """0 = rtigo3 (a light's back face reflects through its BSDF), 1 = Optix7Gui (any light hit ends the path)."""
        L.check(L.lib.twk_set_shader_variant(self._h, int(variant)))

    def enableAov(self, enable=True):
        L.check(L.lib.twk_enable_aov(self._h, int(bool(enable))))

    def enableMoments(self, enable=True):
        """twk_enable_moments: the accumulate kernel also folds the luminance moments (mean, M2, n, 0) of the samples it keeps,
        Welford's recurrence in f32, one float4 per launch index, always float32 — what denoise(moments=...) is guided by."""
        L.check(L.lib.twk_enable_moments(self._h, int(bool(enable))))

    def readMoments(self):
        """The luminance moments: float32 [height, launchWidth, 4] = (mean, M2, n, 0); M2 / ((n - 1) n) is the variance of the pixel's mean."""
        out = np.empty((self.state.resolution[1], self.launchWidth, 4), dtype=np.float32)
        L.check(L.lib.twk_read_moments(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def momentsDevicePointer(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_moments_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def debugReadPathRadiance(self, samples):
        """The raw samples of the last wavefront pass as its accumulate kernel read them (twk_debug_read_path_radiance): float32
        [samples, height, launchWidth, 4]; `samples` = the iterations that pass rendered together (w = 0: no pixel there)."""
        out = np.empty((int(samples), self.state.resolution[1], self.launchWidth, 4), dtype=np.float32)
        L.check(L.lib.twk_debug_read_path_radiance(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    # ---- the temporal seam (include/tweeker_hip.h "The temporal seam", csrc/temporal_device.h) ----
    def setSampleOffset(self, offset):
        """twk_set_sample_offset: iteration i draws its random numbers as iteration i + offset; what counts samples is unchanged.
        A frame restarted at iteration 0 after a camera move sets frames x spp, so that its noise is independent of the history."""
        L.check(L.lib.twk_set_sample_offset(self._h, C.c_uint(int(offset))))

    def enableGeometry(self, enable=True):
        """twk_enable_geometry: one float4 (world position of the primary hit, bits of instance + 1; zeros for a miss) per launch index."""
        L.check(L.lib.twk_enable_geometry(self._h, int(bool(enable))))

    def renderGeometry(self):
        """twk_render_geometry: one closest-hit ray through the centre of every pixel with the camera as it is now. Asynchronous."""
        L.check(L.lib.twk_render_geometry(self._h))

    def renderGeometryTile(self):
        """twk_render_geometry_tile: renderGeometry for a handle whose buffers are packed tile buffers (distribution 1, several
        devices) — one ray per launch index through the centre of the pixel twk_tile_column maps it to, padding written as a miss;
        on any other handle it is renderGeometry itself. Asynchronous. TwkError (INVALID_STATE) before build or setState, with the
        geometry off, with a lens shader other than the pinhole, and on a scene with a cutout texture in use."""
        L.check(L.lib.twk_render_geometry_tile(self._h))

    def readGeometry(self):
        """The geometry AOV: float32 [height, launchWidth, 4]; [..., 3].view(uint32) is instance + 1, 0 for a miss."""
        out = np.empty((self.state.resolution[1], self.launchWidth, 4), dtype=np.float32)
        L.check(L.lib.twk_read_geometry(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def geometryDevicePointer(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_geometry_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def temporalAccumulate(self, params=None, current=None, history=None, shape=None, colourOut=None, historyOut=None, momentsOut=None):
        """twk_temporal_accumulate: reprojects the history through its camera and merges it with the current frame's samples by
        sample count. params: L.Temporal (None = the defaults). Without `current` the handle's own accumulation buffer, moments,
        geometry AOV and camera are the frame and the history is what the previous call kept (readTemporal, readTemporalMoments,
        temporalDevicePointers hand out the result). Otherwise current / history are L.TemporalFrame of device pointers to shape =
        (height, width) pixels (history None: every pixel passes through) and colourOut / historyOut / momentsOut device pointers or None."""
        tp = params if params is not None else L.Temporal()
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda f: None if f is None else C.byref(f)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate(self._h, C.byref(tp), ref(current), ref(history), int(w), int(h), ptr(colourOut), ptr(historyOut), ptr(momentsOut)))

    def temporalReset(self):
        """twk_temporal_reset: drops the history of the own-buffer form; the next temporalAccumulate() copies its frame through."""
        L.check(L.lib.twk_temporal_reset(self._h))

    def temporalDevicePointers(self):
        """(colour pointer, bytes, moments pointer, bytes) of the own-buffer form's result: denoise(beauty=colour, moments=moments, ...)."""
        c, cn, m, mn = C.c_void_p(), C.c_size_t(0), C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_temporal_device_pointers(self._h, C.byref(c), C.byref(cn), C.byref(m), C.byref(mn)))
        return c.value, cn.value, m.value, mn.value

    def _temporalWidth(self):
        """Columns of the temporal result: the picture's width on a tiled handle (temporalAccumulateAssembled), else launchWidth."""
        return self.state.resolution[0] if (self.state.distribution and self.count > 1) else self.launchWidth

    def temporalAccumulateAssembled(self, params=None):
        """twk_temporal_accumulate_assembled, on a tiled primary: temporalAccumulate()'s own-buffer form with the planes this handle
        assembled as the current frame — the assembled beauty, moments and geometry (assembleWithGeometry), this handle's camera 0,
        width x height pixels — against the history this handle kept; with enableTemporalCascade also the assembled cascade
        layers. readTemporal, readTemporalMoments, temporalDevicePointers, readTemporalCascade, temporalCascadeDevicePointer and
        temporalReset work as on one device, [height, width]. params: L.Temporal (None = the defaults). TwkError (INVALID_STATE)
        before setState, on a handle that is not tiled (use temporalAccumulate), with moments or geometry off, with cascade merging
        on but no cascade, and while the beauty, the moments, the cascade (when merged) or the geometry has not been assembled or
        the assembled geometry is stale — the text names which."""
        L.check(L.lib.twk_temporal_accumulate_assembled(self._h, None if params is None else C.byref(params)))

    def readTemporal(self):
        """The merged colour of the own-buffer form: float32 [height, launchWidth, 4] (widened exactly in half mode); [height, width,
        4] on a tiled primary (temporalAccumulateAssembled)."""
        out = np.empty((self.state.resolution[1], self._temporalWidth(), 4), dtype=np.float32)
        L.check(L.lib.twk_read_temporal(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def readTemporalMoments(self):
        """The merged luminance moments of the own-buffer form: float32 [height, launchWidth, 4] = (mean, M2, n, 0); [height, width,
        4] on a tiled primary."""
        out = np.empty((self.state.resolution[1], self._temporalWidth(), 4), dtype=np.float32)
        L.check(L.lib.twk_read_temporal_moments(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    # ---- the rectified temporal merge (include/tweeker_hip.h "The rectified temporal merge", csrc/temporal_rectify_device.h) ----
    def temporalAccumulateRectified(self, params=None, rectify=None, current=None, history=None, shape=None, colourOut=None, historyOut=None, momentsOut=None,
                                    trustOut=None):
        """twk_temporal_accumulate_rectified: temporalAccumulate with a per-pixel trust in the reprojected history — after
        updateLight / updateMaterial the history of the old lighting is discounted where a paired test over a window says the frame
        and the history differ by more than noise. params: L.Temporal, rectify: L.TemporalRectify (None = the defaults). The two
        forms and their arguments are temporalAccumulate's; trustOut: a device pointer to height*width floats or None. Own-buffer
        form: readTemporalTrust / temporalTrustDevicePointer hand out the trust, and with enableTemporalCascade the layers are
        merged with it."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda f: None if f is None else C.byref(f)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_rectified(self._h, ref(params), ref(rectify), ref(current), ref(history), int(w), int(h), ptr(colourOut), ptr(historyOut),
                                                        ptr(momentsOut), ptr(trustOut)))

    def temporalAccumulateAssembledRectified(self, params=None, rectify=None):
        """twk_temporal_accumulate_assembled_rectified, on a tiled primary: temporalAccumulateAssembled with the rectified merge."""
        ref = lambda f: None if f is None else C.byref(f)
        L.check(L.lib.twk_temporal_accumulate_assembled_rectified(self._h, ref(params), ref(rectify)))

    def temporalTrustDevicePointer(self):
        """(device pointer, bytes) of the trust plane the last own-buffer rectified merge kept: height*width floats."""
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_temporal_trust_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readTemporalTrust(self):
        """The trust of the last own-buffer rectified merge: float32 [height, launchWidth] ([height, width] on a tiled primary); 1
        where nothing was tested, 0 where the test took all of the history."""
        out = np.empty((self.state.resolution[1], self._temporalWidth()), dtype=np.float32)
        L.check(L.lib.twk_read_temporal_trust(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def temporalAccumulateCascadeTrusted(self, params=None, cascade=None, currentLayers=None, currentGeometry=None, historyLayers=None, historyGeometry=None,
                                         historyCamera=None, trust=None, shape=None, layersOut=None):
        """twk_temporal_accumulate_cascade_trusted: temporalAccumulateCascade with the capped history of every layer scaled by
        trust, a device pointer to height*width floats (a trustOut of temporalAccumulateRectified for the same frame and history)."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda s: None if s is None else C.byref(s)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_cascade_trusted(self._h, ref(params), ref(cascade), ptr(currentLayers), ptr(currentGeometry), ptr(historyLayers),
                                                              ptr(historyGeometry), ref(historyCamera), ptr(trust), int(w), int(h), ptr(layersOut)))

    # ---- moving an object (include/tweeker_hip.h "Moving an object", csrc/temporal_motion_device.h) ----
    def updateInstanceTransform(self, idInstance, transform):
        """twk_update_instance_transform: replaces the instance's object-to-world matrix (12 floats, row-major 3 x 4) and rebuilds
        the acceleration structure as build() does, but KEEPS the temporal history: the next own-buffer temporalAccumulate /
        temporalAccumulateRectified (or their assembled forms) looks the history up where the instance was. The geometry AOV is
        stale afterwards. TwkError: before build(), a bad id, a transform that is not finite or singular, an instance with a light."""
        t = (C.c_float * 12)(*[float(x) for x in np.asarray(transform, dtype=np.float32).reshape(12)])
        L.check(L.lib.twk_update_instance_transform(self._h, int(idInstance), t))

    # ---- selective instance updates (include/tweeker_hip.h "Selective instance updates", csrc/update_plan.h) ----
    def setUpdateMode(self, mode):
        """twk_set_update_mode: L.TWK_UPDATE_FULL (default: an update rebuilds everything) or L.TWK_UPDATE_SELECTIVE — the next
        build() keeps its by-products (about 136 B per node) and the updates of that scene rebuild only what the moved instances
        change. A scene built in full mode keeps updating fully until it is built again. TwkError: any other mode."""
        L.check(L.lib.twk_set_update_mode(self._h, int(mode)))

    def updateInstanceTransforms(self, ids, transforms):
        """twk_update_instance_transforms: several moves (ids: ints; transforms: 12 floats each, row-major 3 x 4), one rebuild, in
        either mode. Every refusal of updateInstanceTransform applies per entry and names it; also refused: no entry, an id listed
        twice. A refused batch changes nothing."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1)
        if t.size != 12 * ids.size:
            raise ValueError("updateInstanceTransforms: 12 floats per id")
        L.check(L.lib.twk_update_instance_transforms(self._h, int(ids.size), ids.ctypes.data_as(C.POINTER(C.c_int)), t.ctypes.data_as(C.POINTER(C.c_float))))

    # ---- deforming an object (include/tweeker_hip.h "Deforming an object", csrc/temporal_carry_device.h) ----
    def updateGeometryVertices(self, idGeometry, attributes):
        """twk_update_geometry_vertices: replaces all attributes of a geometry (float32 [n, 12]: vertex, tangent, normal, texcoord; n
        is the geometry's vertex count, the indices stay) and rebuilds the acceleration structure — everything in full mode, only what
        the new vertices change in selective mode (updateInfo). The temporal history is kept and the geometry is deformed
        (geometryDeformed) until a merge swaps the history; the geometry AOV is stale. TwkError: before build(), a bad id, another
        vertex count, a position that is not finite, a geometry an instance with a light references."""
        attributes = np.ascontiguousarray(attributes, dtype=np.float32).reshape(-1, 12)
        L.check(L.lib.twk_update_geometry_vertices(self._h, int(idGeometry), attributes.ctypes.data_as(C.c_void_p), C.c_size_t(attributes.shape[0])))

    # ---- refit (include/tweeker_hip.h "Refit", csrc/bvh_refit.h; every refit call runs the one batch of csrc/bvh_refit.hip) ----
    def refitGeometryVertices(self, idGeometry, attributes):
        """twk_refit_geometry_vertices: updateGeometryVertices on a handle built in selective mode, but the geometry's trees are refit
        in place — new boxes, the topology, the references and the wide nodes' cuts kept — instead of rebuilt. The handle is then a
        legal scene for the new vertices, not a fresh build's; refitInfo says how far its SAH cost has drifted, and
        updateGeometryVertices rebuilds. TwkError: updateGeometryVertices' refusals, and a handle not built in selective mode."""
        attributes = np.ascontiguousarray(attributes, dtype=np.float32).reshape(-1, 12)
        L.check(L.lib.twk_refit_geometry_vertices(self._h, int(idGeometry), attributes.ctypes.data_as(C.c_void_p), C.c_size_t(attributes.shape[0])))

    # ---- refit of a moved instance (include/tweeker_hip.h "Refit of a moved instance", kind 2 of csrc/refit_scene_plan.h) ----
    def refitInstanceTransform(self, idInstance, transform):
        """twk_refit_instance_transform: updateInstanceTransform on a handle built in selective mode, but the world-space tree of a
        moved flattened instance is refit in place — slots through the new matrix, boxes, wide nodes and costs updated, topology,
        cuts and shading records kept — instead of rebuilt (a direct leaf is rebuilt, an entered instance gets its world box).
        refitInfo says how far the SAH cost has drifted; updateInstanceTransform rebuilds. TwkError: updateInstanceTransform's
        refusals, and a handle not built in selective mode."""
        t = (C.c_float * 12)(*[float(x) for x in np.asarray(transform, dtype=np.float32).reshape(12)])
        L.check(L.lib.twk_refit_instance_transform(self._h, int(idInstance), t))

    def refitInstanceTransforms(self, ids, transforms):
        """twk_refit_instance_transforms: several moves (updateInstanceTransforms' arguments and refusals), every moved tree refit
        by one launch sequence and one host wait. A refused batch changes nothing."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1)
        if t.size != 12 * ids.size:
            raise ValueError("refitInstanceTransforms: 12 floats per id")
        L.check(L.lib.twk_refit_instance_transforms(self._h, int(ids.size), ids.ctypes.data_as(C.POINTER(C.c_int)), t.ctypes.data_as(C.POINTER(C.c_float))))

    # ---- a device-pointer source (include/tweeker_hip.h "A device-pointer source", csrc/vertex_source_device.h) ----
    def updateGeometryVerticesDevice(self, idGeometry, source, numVertices=None, positions=None, stride=None, recomputeFrames=False):
        """twk_update_geometry_vertices_device: updateGeometryVertices from vertices that live on the device — `source` is a torch
        tensor (or a strided view of one, passed without a copy), an object with __cuda_array_interface__, or an integer address with
        numVertices: float32 [n, 12] records, or [n, 3] positions (recomputeFrames: normals and tangents follow the new positions,
        else they stay; texcoords always stay). The source is read on the handle's stream: finish producing it first (synchronise the
        stream that wrote it); on return it has been consumed. The handle then equals one given the same records through
        updateGeometryVertices. TwkError: its refusals, a pointer that is not device memory, a position that is not finite."""
        src, n = _vertex_source(source, numVertices, positions, stride, recomputeFrames)
        L.check(L.lib.twk_update_geometry_vertices_device(self._h, int(idGeometry), C.byref(src), C.c_size_t(n)))

    def refitGeometryVerticesDevice(self, idGeometry, source, numVertices=None, positions=None, stride=None, recomputeFrames=False):
        """twk_refit_geometry_vertices_device: refitGeometryVertices from a device source (updateGeometryVerticesDevice's arguments)."""
        src, n = _vertex_source(source, numVertices, positions, stride, recomputeFrames)
        L.check(L.lib.twk_refit_geometry_vertices_device(self._h, int(idGeometry), C.byref(src), C.c_size_t(n)))

    # ---- a frame's edits in one call (include/tweeker_hip.h "A frame's edits in one call", csrc/refit_scene_plan.h) ----
    def refitScene(self, geometries=(), ids=(), transforms=()):
        """twk_refit_scene: the vertex refits of `geometries` and the transform refits of the instances `ids` in ONE call — every tree
        refit once, all in one batch with one host wait. geometries: a list of (idGeometry, array) — float32 [n, 12] host records, as
        refitGeometryVertices takes them — or (idGeometry, dict) — a device source, the dict holding refitGeometryVerticesDevice's
        arguments (source, and numVertices / positions / stride / recomputeFrames where needed). ids / transforms: as
        refitInstanceTransforms takes them. The handle then holds, byte for byte, what the single calls in that order leave; refitInfo
        and updateInfo describe the one call. TwkError: the single calls' refusals under the name twk_refit_scene, a geometry entry's
        with "geometry entry k: " in front; a refused call changes nothing."""
        geometries = list(geometries)
        edits = (L.GeometryEdit * max(1, len(geometries)))()
        keep = []  # the arrays and sources the entries point to, alive until the call returns
        for k, (idGeometry, what) in enumerate(geometries):
            edits[k].idGeometry, edits[k].reserved = int(idGeometry), 0
            if isinstance(what, dict):
                src, n = _vertex_source(what["source"], what.get("numVertices"), what.get("positions"), what.get("stride"), what.get("recomputeFrames", False))
                keep.append(src)
                edits[k].numVertices, edits[k].source = n, C.pointer(src)
            else:
                a = np.ascontiguousarray(what, dtype=np.float32).reshape(-1, 12)
                keep.append(a)
                edits[k].numVertices, edits[k].attributes = a.shape[0], a.ctypes.data
        ids = np.ascontiguousarray(list(ids), dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1)
        if t.size != 12 * ids.size:
            raise ValueError("refitScene: 12 floats per id")
        L.check(L.lib.twk_refit_scene(self._h, len(geometries), edits if geometries else None, int(ids.size),
                                      ids.ctypes.data_as(C.POINTER(C.c_int)) if ids.size else None, t.ctypes.data_as(C.POINTER(C.c_float)) if ids.size else None))

    def readGeometryVertices(self, idGeometry, numVertices):
        """twk_read_geometry_vertices: the geometry's current records, float32 [numVertices, 12], wherever they were last written."""
        out = np.empty((int(numVertices), 12), np.float32)
        L.check(L.lib.twk_read_geometry_vertices(self._h, int(idGeometry), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.shape[0])))
        return out

    def refitInfo(self):
        """twk_get_refit_info: what the last refit did, a dict of L.RefitInfo's fields (treesRefit, treesRebuilt, topLevelRebuilt,
        refitsSinceBuild, nodesRefit, slotsRewritten, sahBuilt, sahNow, milliseconds). TwkError before one."""
        r = L.RefitInfo()
        L.check(L.lib.twk_get_refit_info(self._h, C.byref(r)))
        return {name: getattr(r, name) for name, _ in L.RefitInfo._fields_}

    def debugReadKeptBuild(self):
        """twk_debug_read_kept_build: what a selective handle keeps on the device — (wide float32 [nodes + 2, 32], the full-precision
        wide nodes and the two root slots; nodeCost float32 [nodes]; pairFlags int32 [slots]), nodeCost / pairFlags None where the
        handle keeps none. TwkError on a handle not built in selective mode."""
        b = self.buildInfo()
        nodes, slots = int(b["nodes"]), int(b["triangleSlots"])
        wide = np.zeros((nodes + 2, 32), np.float32)
        L.check(L.lib.twk_debug_read_kept_build(self._h, wide.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(wide.size), None, C.c_size_t(0), None, C.c_size_t(0)))
        cost, flags = np.zeros(nodes, np.float32), np.zeros(slots, np.int32)
        if L.lib.twk_debug_read_kept_build(self._h, None, C.c_size_t(0), cost.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(cost.size), None, C.c_size_t(0)) != L.TWK_SUCCESS:
            cost = None
        if L.lib.twk_debug_read_kept_build(self._h, None, C.c_size_t(0), None, C.c_size_t(0), flags.ctypes.data_as(C.POINTER(C.c_int)), C.c_size_t(flags.size)) != L.TWK_SUCCESS:
            flags = None
        return wide, cost, flags

    def geometryDeformed(self, idGeometry):
        """twk_get_geometry_deformed: whether the handle holds the geometry's positions as of the history's frame."""
        d = C.c_int(0)
        L.check(L.lib.twk_get_geometry_deformed(self._h, int(idGeometry), C.byref(d)))
        return bool(d.value)

    def renderGeometryMotion(self):
        """twk_render_geometry_motion: renderGeometry, and beside the geometry AOV the previous-position plane (readPreviousPositions):
        per hit pixel where its surface point was when the temporal history was taken. The first call after an update (or a merge) uploads
        the per-instance records and the previous positions and waits for the upload; while nothing has changed it is asynchronous."""
        L.check(L.lib.twk_render_geometry_motion(self._h))

    def readPreviousPositions(self):
        """The previous-position plane: float32 [height, width, 4]; [..., 3].view(uint32) is instance + 1, 0 for a miss."""
        out = np.empty((self.state.resolution[1], self.launchWidth, 4), dtype=np.float32)
        L.check(L.lib.twk_read_previous_positions(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def previousPositionsDevicePointer(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_previous_position_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    @staticmethod
    def updatePlanHost(instanceGeometry, geometryTriangles, flattenPolicy, moved=(), maxLeaf=2):
        """twk_update_plan_host, pure CPU: update_plan_host of this module."""
        return update_plan_host(instanceGeometry, geometryTriangles, flattenPolicy, moved, maxLeaf)

    def updateInfo(self):
        """twk_get_update_info: what the last update did, a dict of L.UpdateInfo's fields (selective, instancesMoved, treesRebuilt,
        topLevelRebuilt, nodesRequantised, slotsRewritten, instanceRecordsUploaded, keptBytes, milliseconds). TwkError before one."""
        u = L.UpdateInfo()
        L.check(L.lib.twk_get_update_info(self._h, C.byref(u)))
        return {name: getattr(u, name) for name, _ in L.UpdateInfo._fields_}

    def instanceTransform(self, idInstance):
        """twk_get_instance_transform: the instance's transform as it is now, float32 [12]."""
        t = (C.c_float * 12)()
        L.check(L.lib.twk_get_instance_transform(self._h, int(idInstance), t))
        return np.array(t, dtype=np.float32)

    def temporalAccumulateMoving(self, params=None, rectify=None, current=None, history=None, motion=None, numMotion=0, shape=None, colourOut=None, historyOut=None,
                                 momentsOut=None, trustOut=None):
        """twk_temporal_accumulate_moving: the explicit form of temporalAccumulate (rectify None) or of temporalAccumulateRectified
        with a motion table — motion: a device pointer to numMotion L.InstanceMotion records (16-byte aligned), indexed by instance.
        motion None or numMotion 0: the existing calls, byte for byte."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda f: None if f is None else C.byref(f)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_moving(self._h, ref(params), ref(rectify), ref(current), ref(history), ptr(motion), int(numMotion), int(w), int(h),
                                                     ptr(colourOut), ptr(historyOut), ptr(momentsOut), ptr(trustOut)))

    def temporalAccumulateCascadeMoving(self, params=None, cascade=None, currentLayers=None, currentGeometry=None, historyLayers=None, historyGeometry=None,
                                        historyCamera=None, trust=None, motion=None, numMotion=0, shape=None, layersOut=None):
        """twk_temporal_accumulate_cascade_moving: temporalAccumulateCascade (trust None) or temporalAccumulateCascadeTrusted with a
        motion table, as temporalAccumulateMoving takes it."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda s: None if s is None else C.byref(s)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_cascade_moving(self._h, ref(params), ref(cascade), ptr(currentLayers), ptr(currentGeometry), ptr(historyLayers),
                                                             ptr(historyGeometry), ref(historyCamera), ptr(trust), ptr(motion), int(numMotion), int(w), int(h), ptr(layersOut)))

    def temporalAccumulateCarried(self, params=None, rectify=None, current=None, history=None, previousPositions=None, shape=None, colourOut=None, historyOut=None,
                                  momentsOut=None, trustOut=None):
        """twk_temporal_accumulate_carried: the explicit form of temporalAccumulate (rectify None) or of temporalAccumulateRectified
        that takes g' from a previous-position plane — previousPositions: a device pointer to height x width float4 (16-byte aligned),
        as previousPositionsDevicePointer hands out. previousPositions None: the existing calls, byte for byte."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda f: None if f is None else C.byref(f)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_carried(self._h, ref(params), ref(rectify), ref(current), ref(history), ptr(previousPositions), int(w), int(h),
                                                      ptr(colourOut), ptr(historyOut), ptr(momentsOut), ptr(trustOut)))

    def temporalAccumulateCascadeCarried(self, params=None, cascade=None, currentLayers=None, currentGeometry=None, historyLayers=None, historyGeometry=None, historyCamera=None,
                                         trust=None, previousPositions=None, shape=None, layersOut=None):
        """twk_temporal_accumulate_cascade_carried: the explicit merge of the cascade's layers (trust None: plain; given: trusted) that
        takes g' from a previous-position plane. previousPositions None: the existing calls, byte for byte."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda f: None if f is None else C.byref(f)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_cascade_carried(self._h, ref(params), ref(cascade), ptr(currentLayers), ptr(currentGeometry), ptr(historyLayers),
                                                              ptr(historyGeometry), ref(historyCamera), ptr(trust), ptr(previousPositions), int(w), int(h), ptr(layersOut)))

    def readTemporalMotion(self):
        """twk_read_temporal_motion: the motion table the last own-buffer (or assembled) merge used, a ctypes array of
        L.InstanceMotion, one per instance; empty when it used none (no instance had moved since the history's frame)."""
        n = C.c_int(0)
        if L.lib.twk_read_temporal_motion(self._h, None, C.c_size_t(0), C.byref(n)) == L.TWK_SUCCESS:
            return (L.InstanceMotion * 0)()
        table = (L.InstanceMotion * max(1, n.value))()  # (a capacity that is too small is refused, with the count written)
        L.check(L.lib.twk_read_temporal_motion(self._h, table, C.c_size_t(len(table)), C.byref(n)))
        return table

    def setTimeView(self, enable=True):
        """≙ USE_TIME_VIEW: alpha of the accumulation buffer = running mean of the sample's shader-clock cycles x clockFactor x 1e-9."""
        L.check(L.lib.twk_set_time_view(self._h, int(bool(enable))))

    def setNextEventEstimation(self, enable=True):
        """≙ USE_NEXT_EVENT_ESTIMATION (shaders/config.h:50-52): False = brute-force path tracing without light sampling and MIS weights."""
        L.check(L.lib.twk_set_next_event_estimation(self._h, int(bool(enable))))

    def setDebugExceptions(self, enable=True):
        """≙ USE_DEBUG_EXCEPTIONS (raygeneration.cu:205-218): NaN / Inf / negative samples accumulate as super red / green / blue."""
        L.check(L.lib.twk_set_debug_exceptions(self._h, int(bool(enable))))

    def readAov(self, which, raw=False):
        """Denoiser AOV running means: which = 0 albedo, 1 camera-space normal; float32 [height, launchWidth, 4] (widened
        exactly in half mode). raw=True: the buffer as it is held, float16 in half mode (float32 otherwise)."""
        h, w = self.state.resolution[1], self.launchWidth
        if raw:
            out = np.empty((h, w, 4), dtype=np.float16 if self.outputFormat == L.TWK_OUTPUT_HALF4 else np.float32)
            L.check(L.lib.twk_read_aov_raw(self._h, int(which), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
            return out
        out = np.empty((h, w, 4), dtype=np.float32)
        L.check(L.lib.twk_read_aov(self._h, int(which), out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def setOutputFormat(self, fmt):
        """0 = RGBA32F (default), 1 = RGBA16F output and AOV buffers (≙ Optix7Gui USE_FP32_OUTPUT 0). Reallocates them, zeroed."""
        L.check(L.lib.twk_set_output_format(self._h, int(fmt)))

    @property
    def outputFormat(self):
        f = C.c_int(0)
        L.check(L.lib.twk_get_output_format(self._h, C.byref(f)))
        return f.value

    def setBuildQuality(self, quality):
        """0 = LBVH (Morton + radix tree), 1 = binned SAH (default)."""
        L.check(L.lib.twk_set_build_quality(self._h, int(quality)))

    def buildInfo(self):
        b = L.BuildInfo()
        L.check(L.lib.twk_get_build_info(self._h, C.byref(b)))
        return {name: getattr(b, name) for name, _ in L.BuildInfo._fields_}

    def streamLayout(self):
        """'slim' or 'full': the layout of the path streams a pass over the built scene uses (twk_get_stream_layout)."""
        layout = C.c_int(0)
        L.check(L.lib.twk_get_stream_layout(self._h, C.byref(layout)))
        return "slim" if layout.value == 1 else "full"

    def setFlattenPolicy(self, maxTriangles, maxReferences):
        """Build option of the next build(): instances of geometries with <= maxTriangles triangles, or referenced by
        <= maxReferences instances, are intersected in world space in one single-level BVH; (0, 0) = pure two-level."""
        L.check(L.lib.twk_set_flatten_policy(self._h, int(maxTriangles), int(maxReferences)))

    def build(self):
        L.check(L.lib.twk_build(self._h))

    # ---- rendering ----------------------------------------------------------------------------
    def render(self, iterationIndex):
        """≙ Device::render(iterationIndex, buffer) → optixLaunch: asynchronous, one sample per pixel."""
        L.check(L.lib.twk_launch(self._h, C.c_uint(int(iterationIndex))))

    def setLaunchBatch(self, iterations):
        """Iterations rendered together per wavefront pass (1..64); results do not depend on it."""
        L.check(L.lib.twk_set_launch_batch(self._h, int(iterations)))

    def reserveLaunchBatch(self, iterations):
        """Allocate the path streams for passes of `iterations` samples per pixel now instead of on demand."""
        L.check(L.lib.twk_reserve_launch_batch(self._h, int(iterations)))

    def synchronizeStream(self):
        L.check(L.lib.twk_sync(self._h))

    @property
    def launchWidth(self):
        w = C.c_int(0)
        L.check(L.lib.twk_get_launch_width(self._h, C.byref(w)))
        return w.value

    def getOutputBufferHost(self):
        """RGBA32F running mean, shape [height, launchWidth, 4] (launchWidth == width unless tiled)."""
        h, w = self.state.resolution[1], (self.state.resolution[0] if getattr(self, "_sharedFrame", False) else self.launchWidth)
        out = np.empty((h, w, 4), dtype=np.float32)
        L.check(L.lib.twk_read_output(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def getOutputBufferHalf(self):
        """The RGBA16F running mean as held in half mode (setOutputFormat(1)): float16 [height, launchWidth, 4]."""
        h, w = self.state.resolution[1], (self.state.resolution[0] if getattr(self, "_sharedFrame", False) else self.launchWidth)
        out = np.empty((h, w, 4), dtype=np.float16)
        L.check(L.lib.twk_read_output_raw(self._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
        return out

    def outputDevicePointer(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_output_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def setOutputDevicePointer(self, dptr, nbytes):
        L.check(L.lib.twk_set_output_device_pointer(self._h, C.c_void_p(dptr), C.c_size_t(nbytes)))

    def compositor(self, tiles_dptr, output_dptr, half=False):
        """half=True: RGBA16F tiles into an RGBA16F frame (twk_compositor_half)."""
        fn = L.lib.twk_compositor_half if half else L.lib.twk_compositor
        L.check(fn(self._h, C.c_void_p(tiles_dptr), C.c_void_p(output_dptr)))

    # ---- measurement / parity taps ------------------------------------------------------------
    def profileEnable(self, enable=True):
        L.check(L.lib.twk_profile_enable(self._h, int(bool(enable))))

    def profileReset(self):
        L.check(L.lib.twk_profile_reset(self._h))

    def profileGet(self):
        ms = (C.c_float * len(KERNEL_CLASSES))()
        n = (C.c_int * len(KERNEL_CLASSES))()
        L.check(L.lib.twk_profile_get(self._h, ms, n))
        return {k: {"ms": ms[i], "launches": n[i]} for i, k in enumerate(KERNEL_CLASSES)}

    def tonemap(self, tonemapper=None, rgbaDevicePointer=None, shape=None, half=False):
        """RGBA32F → RGB8 with the reference's tonemapper (Application.cpp:2259-2297) on the device. Without a pointer
        the handle's own accumulation buffer (launchWidth x height, in its output format) is converted; returns uint8
        [H, W, 3], row 0 at the bottom like the float buffer. half=True: rgbaDevicePointer holds RGBA16F (twk_tonemap_half)."""
        tm = tonemapper if tonemapper is not None else L.Tonemapper()
        if half:
            assert rgbaDevicePointer is not None, "tonemap(half=True) needs an explicit RGBA16F device buffer"
            h, w = shape
            out = np.empty((h, w, 3), dtype=np.uint8)
            L.check(L.lib.twk_tonemap_half(self._h, C.byref(tm), C.c_void_p(int(rgbaDevicePointer)), C.c_size_t(h * w),
                                           out.ctypes.data_as(C.POINTER(C.c_ubyte))))
            return out
        if rgbaDevicePointer is None:
            h, w = self.state.resolution[1], self.launchWidth
            ptr = None
        else:
            h, w = shape
            ptr = C.c_void_p(int(rgbaDevicePointer))
        out = np.empty((h, w, 3), dtype=np.uint8)
        L.check(L.lib.twk_tonemap(self._h, C.byref(tm), ptr, C.c_size_t(h * w), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def denoise(self, params=None, beauty=None, albedo=None, normal=None, shape=None, denoised=None, variance=None, moments=None, minSamples=None,
                geometry=None, geometryBuffer=None, camera=None):
        """twk_denoise: the edge-avoiding a-trous wavelet filter (a classical filter, not a learned one) where Optix7Gui calls
        optixDenoiserInvoke. Asynchronous. params: L.Denoiser (None = the defaults). Without `beauty` the handle's own
        accumulation and AOV buffers are filtered; otherwise beauty / albedo / normal are device pointers to shape = (height,
        width) pixels in the handle's output format. denoised: device pointer of the result, None = the internal buffer that
        readDenoised / denoisedDevicePointer hand out. variance: L.DenoiserVariance = twk_denoise_variance, the variance-guided,
        firefly-clamping mode of the same filter (params.sigmaColor is ignored then); None = twk_denoise.
        minSamples (an int >= 2) or moments: twk_denoise_variance_sampled — pixels that have seen at least minSamples samples
        (default L.TWK_DENOISER_MIN_SAMPLES) are guided by the measured variance of their mean instead of the spatial estimate.
        moments: device pointer to shape float4 (mean, M2, n, .) beside an explicit beauty; without `beauty`, moments=True (or just
        minSamples) takes the handle's own (enableMoments). variance=None then means DenoiserVariance().
        geometry: L.DenoiserGeometry = twk_denoise_geometry, the same three modes with the geometry guide (plane and instance
        stops; inputKind RGB_ALBEDO_NORMAL only). geometryBuffer: device pointer to shape float4 (world position, instance + 1)
        beside an explicit beauty; without `beauty` the handle's own geometry AOV (enableGeometry, renderGeometry). camera: the 12
        floats P, U, V, W the geometry was traced from (a CameraDefinition or a sequence), None = the handle's camera 0."""
        dn = params if params is not None else L.Denoiser()
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        h, w = shape if shape is not None else (0, 0)
        if geometry is not None:
            sampled = minSamples is not None or (moments is not None and moments is not False)
            dv = variance if (variance is not None or not sampled) else L.DenoiserVariance()
            m = None if (moments is None or moments is True or moments is False) else C.c_void_p(int(moments))
            n = 0 if not sampled else (L.TWK_DENOISER_MIN_SAMPLES if minSamples is None else int(minSamples))
            cam = None
            if camera is not None:
                values = bytes(camera)[:48] if isinstance(camera, C.Structure) else None
                cam = (C.c_float * 12).from_buffer_copy(values) if values is not None else (C.c_float * 12)(*[float(v) for v in camera])
            L.check(L.lib.twk_denoise_geometry(self._h, C.byref(dn), C.byref(geometry), None if dv is None else C.byref(dv), n, ptr(beauty), ptr(albedo), ptr(normal), m,
                                               ptr(geometryBuffer), cam, int(w), int(h), ptr(denoised)))
            return
        if minSamples is not None or (moments is not None and moments is not False):
            dv = variance if variance is not None else L.DenoiserVariance()
            m = None if (moments is None or moments is True) else C.c_void_p(int(moments))
            n = L.TWK_DENOISER_MIN_SAMPLES if minSamples is None else int(minSamples)
            L.check(L.lib.twk_denoise_variance_sampled(self._h, C.byref(dn), C.byref(dv), n, ptr(beauty), ptr(albedo), ptr(normal), m, int(w), int(h), ptr(denoised)))
            return
        if variance is not None:
            L.check(L.lib.twk_denoise_variance(self._h, C.byref(dn), C.byref(variance), ptr(beauty), ptr(albedo), ptr(normal), int(w), int(h), ptr(denoised)))
            return
        L.check(L.lib.twk_denoise(self._h, C.byref(dn), ptr(beauty), ptr(albedo), ptr(normal), int(w), int(h), ptr(denoised)))

    def denoisedDevicePointer(self):
        """(device pointer, bytes) of the internal denoised buffer, in the output format: feeds tonemap(rgbaDevicePointer=...)."""
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_denoised_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readDenoised(self, raw=False, shape=None):
        """The internal denoised buffer: float32 [height, width, 4] (widened exactly in half mode); raw=True: as held, float16
        in half mode. shape = (height, width) of an explicit-buffer denoise; default: the handle's launchWidth x height."""
        h, w = shape if shape is not None else (self.state.resolution[1], self.launchWidth)
        if raw:
            out = np.empty((h, w, 4), dtype=np.float16 if self.outputFormat == L.TWK_OUTPUT_HALF4 else np.float32)
            L.check(L.lib.twk_read_denoised_raw(self._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
            return out
        out = np.empty((h, w, 4), dtype=np.float32)
        L.check(L.lib.twk_read_denoised(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def estimateNoise(self, noise=None, moments=None, numElements=0, errorMap=None):
        """twk_estimate_noise, then twk_read_noise: how noisy the frame still is, from the integrator's own samples — per element the
        relative standard error e of the luminance mean out of the luminance moments, reduced on the device to an L.NoiseSummary.
        noise: L.Noise (None = the defaults). Without `moments` the handle's own (enableMoments; a packed tile buffer is fine, its
        padding counts as empty); otherwise a device pointer to numElements float4 (mean, M2, n, .). errorMap: device pointer to
        numElements floats, or None; receives e, -1 for an unknown and -2 for an empty element. Not an error against ground truth:
        blind to bias, and no measure of a denoised picture."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        L.check(L.lib.twk_estimate_noise(self._h, None if noise is None else C.byref(noise), ptr(moments), C.c_size_t(int(numElements)), ptr(errorMap)))
        out = L.NoiseSummary()
        L.check(L.lib.twk_read_noise(self._h, C.byref(out)))
        return out

    # ---- adaptive sampling (include/tweeker_hip.h "Adaptive sampling", csrc/adaptive_device.h) ----
    def enableAdaptive(self, enable=True):
        """twk_enable_adaptive: per launch index a sample count, the iteration its next adaptive sample uses, and the active list
        adaptiveSelect fills and renderAdaptive renders. Needs enableMoments first."""
        L.check(L.lib.twk_enable_adaptive(self._h, int(bool(enable))))

    def adaptiveSelect(self, params=None, moments=None, counts=None, numElements=0, activeOut=None):
        """twk_adaptive_select: the ascending list of the elements that are not empty, whose count is below params.maxSamples and
        whose relative standard error is above params.targetNoise or unknown; returns its length (synchronises). params: L.Adaptive
        (None = the defaults). Without buffers the handle's own moments, counts and list (a packed tile buffer is fine); otherwise
        device pointers to numElements float4, numElements uint32 and, for the list, numElements uint32."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        n = C.c_uint(0)
        L.check(L.lib.twk_adaptive_select(self._h, None if params is None else C.byref(params), ptr(moments), ptr(counts), C.c_size_t(int(numElements)),
                                          ptr(activeOut), C.byref(n)))
        return n.value

    # ---- the firefly cascade (include/tweeker_hip.h "The firefly cascade", csrc/cascade_device.h) ----
    def enableCascade(self, enable=True, params=None):
        """twk_enable_cascade: the accumulate kernels also split every kept sample by its luminance over params.layers brightness
        layers (L.Cascade; None = the defaults), per-layer float32 sums beside the running mean, which does not change. A change
        of parameters while enabled zeroes the layers."""
        L.check(L.lib.twk_enable_cascade(self._h, int(bool(enable)), None if params is None else C.byref(params)))
        self._cascadeLayers = (params.layers if params is not None else L.TWK_CASCADE_LAYERS) if enable else 0

    def readCascade(self):
        """The layers: float32 [layers, height, launchWidth, 4]; .xyz the layer's weighted radiance sums, [0, ..., 3] the number of
        kept samples n, [layers - 1, ..., 3] the samples rejected as not finite."""
        out = np.empty((self._cascadeLayers, self.state.resolution[1], self.launchWidth, 4), dtype=np.float32)
        L.check(L.lib.twk_read_cascade(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def cascadeDevicePointer(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_cascade_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def cascadeResolve(self, params=None, resolve=None, layers=None, shape=None, resolved=None):
        """twk_cascade_resolve: out = (layer 0 + sum_j w_j layer j) / n with w_j = min(1, c_j / kappa), c_j the samples that landed
        around layer j in the pixel's 3x3 window; asynchronous. params: L.Cascade, resolve: L.CascadeResolve (None = the handle's
        own / the defaults). Without `layers` the handle's own layers into its internal resolved buffer (readResolved,
        resolvedDevicePointer); otherwise device pointers to [layers][height*width] float4 and to height*width pixels of the
        output format, shape = (height, width)."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_cascade_resolve(self._h, None if params is None else C.byref(params), None if resolve is None else C.byref(resolve),
                                          ptr(layers), int(w), int(h), ptr(resolved)))

    def resolvedDevicePointer(self):
        """(device pointer, bytes) of the internal resolved buffer, in the output format: feeds tonemap(rgbaDevicePointer=...) and
        denoise(beauty=...)."""
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_resolved_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readResolved(self):
        """The internal resolved buffer: float32 [height, launchWidth, 4] (widened exactly in half mode)."""
        out = np.empty((self.state.resolution[1], self.launchWidth, 4), dtype=np.float32)
        L.check(L.lib.twk_read_resolved(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    # ---- the cascade through the temporal merge (include/tweeker_hip.h, csrc/temporal_cascade_device.h) ----
    def temporalAccumulateCascade(self, params=None, cascade=None, currentLayers=None, currentGeometry=None, historyLayers=None, historyGeometry=None,
                                  historyCamera=None, shape=None, layersOut=None):
        """twk_temporal_accumulate_cascade, the explicit form: the history's per-layer sums reprojected through historyCamera (a
        CameraDefinition) and added to the current frame's; asynchronous. params: L.Temporal, cascade: L.Cascade (None = the
        defaults). Layers are device pointers to [layers][height*width] float4, the geometries to height*width float4, shape =
        (height, width). historyLayers None: every pixel passes through. layersOut is the next call's historyLayers and the explicit
        `layers` of cascadeResolve."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        ref = lambda s: None if s is None else C.byref(s)
        h, w = shape if shape is not None else (0, 0)
        L.check(L.lib.twk_temporal_accumulate_cascade(self._h, ref(params), ref(cascade), ptr(currentLayers), ptr(currentGeometry), ptr(historyLayers),
                                                      ptr(historyGeometry), ref(historyCamera), int(w), int(h), ptr(layersOut)))

    def enableTemporalCascade(self, enable=True):
        """twk_temporal_enable_cascade: while on, temporalAccumulate() on the handle's own buffers also merges the handle's cascade
        layers with the previous geometry and camera (readTemporalCascade, temporalCascadeDevicePointer); its colour and moments do
        not change. Needs enableCascade(True)."""
        L.check(L.lib.twk_temporal_enable_cascade(self._h, int(bool(enable))))

    def temporalCascadeDevicePointer(self):
        """(device pointer, bytes) of the merged layers the last temporalAccumulate() kept: cascadeResolve(layers=..., shape=(height, launchWidth), ...)."""
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_temporal_cascade_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readTemporalCascade(self):
        """The merged layers: float32 [layers, height, launchWidth, 4], as readCascade lays them out ([layers, height, width, 4] on
        a tiled primary); [0, ..., 3] is the merged (weighted, capped) sample count."""
        out = np.empty((self._cascadeLayers, self.state.resolution[1], self._temporalWidth(), 4), dtype=np.float32)
        L.check(L.lib.twk_read_temporal_cascade(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    # ---- assembling a tiled frame (include/tweeker_hip.h "Assembling a tiled frame", csrc/assemble_device.h) ----
    @staticmethod
    def _planeMask(planes):
        mask = 0
        for p in planes:
            mask |= 1 << int(p)
        return mask

    def assemble(self, devices, planes):
        """twk_assemble_devices with this handle as primary: the planes (L.TWK_PLANE_*) of every handle of `devices` (all of the
        frame's devices, any order), from their own packed tile buffers into this handle's assembled width x height buffers, in
        one launch; asynchronous, ordered by events between the handles' streams."""
        handles = (C.c_void_p * max(1, len(devices)))(*[d._h.value for d in devices])
        L.check(L.lib.twk_assemble_devices(self._h, C.c_uint(self._planeMask(planes)), handles, int(len(devices))))

    def assembleFrom(self, sources, planes):
        """twk_assemble: the same from explicit buffers — sources[d] an L.AssemblySource (or a dict plane -> device pointer) with
        the packed buffers of the device with index d, addressable from this handle's device (an RCCL caller: pointers into the
        block it gathered). Asynchronous on this handle's stream."""
        arr = (L.AssemblySource * max(1, len(sources)))()
        for d, src in enumerate(sources):
            arr[d] = src if isinstance(src, L.AssemblySource) else L.AssemblySource(src)
        L.check(L.lib.twk_assemble(self._h, C.c_uint(self._planeMask(planes)), arr, int(len(sources))))

    def assembleWithGeometry(self, devices, planes):
        """twk_assemble_devices_with_geometry with this handle as primary: assemble(devices, planes) and, in the same launch, the
        geometry AOV of every handle's tile share (renderGeometryTile) into this handle's assembled width x height geometry
        (readAssembledGeometry, assembledGeometryDevicePointer). planes may be empty: the geometry alone. Beyond assemble's
        refusals, TwkError when the geometry is off on a handle, when a handle's geometry is not valid (no renderGeometryTile since
        its camera, state or scene changed) and when a handle's camera 0 is not this handle's, byte for byte."""
        handles = (C.c_void_p * max(1, len(devices)))(*[d._h.value for d in devices])
        L.check(L.lib.twk_assemble_devices_with_geometry(self._h, C.c_uint(self._planeMask(planes)), handles, int(len(devices))))

    def assembleFromWithGeometry(self, sources, geometrySources, planes):
        """twk_assemble_with_geometry: assembleFrom(sources, planes) and, in the same launch, geometrySources[d] — a device pointer to
        the packed launchWidth x height geometry of the device with index d, addressable from this handle's device. planes may be
        empty (sources is then not looked at). Beyond assembleFrom's refusals, TwkError when the geometry is off on this handle and
        for a missing or NULL geometry source. The sources' cameras and age are the caller's to keep."""
        arr = (L.AssemblySource * max(1, len(sources)))()
        for d, src in enumerate(sources):
            arr[d] = src if isinstance(src, L.AssemblySource) else L.AssemblySource(src)
        geometry = (C.c_void_p * max(1, len(geometrySources)))(*[None if g is None else int(g) for g in geometrySources])
        L.check(L.lib.twk_assemble_with_geometry(self._h, C.c_uint(self._planeMask(planes)), arr, geometry, int(len(geometrySources))))

    def assembledGeometryDevicePointer(self):
        """(device pointer, bytes) of this handle's assembled geometry AOV; TwkError before it has been assembled, after the
        assembled buffers were dropped, and once this handle's camera, state or scene has changed (it is stale)."""
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_assembled_geometry_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readAssembledGeometry(self):
        """The assembled geometry AOV (synchronises): float32 [height, width, 4], laid out like readGeometry on one device. TwkError
        where assembledGeometryDevicePointer raises it: not assembled, dropped, or stale."""
        out = np.empty((self.state.resolution[1], self.state.resolution[0], 4), dtype=np.float32)
        L.check(L.lib.twk_read_assembled_geometry(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def assembledDevicePointer(self, plane):
        """(device pointer, bytes) of this handle's assembled buffer of `plane`; TwkError before the plane has been assembled."""
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_assembled_device_pointer(self._h, int(plane), C.byref(p), C.byref(n)))
        return p.value, n.value

    def readAssembled(self, plane):
        """The assembled buffer of `plane` as it is held (synchronises): beauty and AOVs [height, width, 4] float32 (float16 in half
        mode), moments [height, width, 4] float32, sample counts [height, width] uint32, the cascade [layers, height, width, 4]
        float32."""
        h, w = self.state.resolution[1], self.state.resolution[0]
        plane = int(plane)
        if plane == L.TWK_PLANE_SAMPLE_COUNTS:
            out = np.empty((h, w), dtype=np.uint32)
        elif plane == L.TWK_PLANE_CASCADE:
            out = np.empty((self._cascadeLayers, h, w, 4), dtype=np.float32)
        elif plane == L.TWK_PLANE_MOMENTS:
            out = np.empty((h, w, 4), dtype=np.float32)
        else:
            out = np.empty((h, w, 4), dtype=np.float16 if self.outputFormat == L.TWK_OUTPUT_HALF4 else np.float32)
        L.check(L.lib.twk_read_assembled(self._h, plane, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
        return out

    def renderAdaptive(self, samples):
        """twk_launch_adaptive: `samples` (1..64) samples of every launch index of the active list, each at the iteration its own
        count says; asynchronous. Afterwards render(i) is refused for i != 0; render(0) restarts a uniform frame."""
        L.check(L.lib.twk_launch_adaptive(self._h, int(samples)))

    def readSampleCounts(self):
        """uint32 [height, launchWidth]: per launch index the iteration index its next sample uses = the samples it has been given."""
        out = np.empty((self.state.resolution[1], self.launchWidth), dtype=np.uint32)
        L.check(L.lib.twk_read_sample_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(out.size)))
        return out

    def sampleCountsDevicePointer(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        L.check(L.lib.twk_get_sample_counts_device_pointer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readActive(self):
        """uint32 [numActive]: the launch indices the last adaptiveSelect on the handle's own buffers chose, ascending."""
        n = C.c_uint(0)
        L.check(L.lib.twk_read_active(self._h, None, C.c_size_t(0), C.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        if n.value:
            L.check(L.lib.twk_read_active(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(out.size), C.byref(n)))
        return out

    def adaptivePlan(self, ap=None, plan=None, moments=None, counts=None, numElements=0, activeOut=None, pathOffsetOut=None):
        """twk_adaptive_plan: the elements adaptiveSelect would choose for `ap`, each with the samples its noise estimate predicts
        (plan: L.AdaptivePlan; None = the defaults); returns (numActive, numPaths) and synchronises. Without buffers the handle's
        own moments and counts and a plan of its own, which renderPlanned renders and readPlan reads; otherwise device pointers to
        numElements float4, numElements uint32 and, for the outputs, numElements and numElements + 1 uint32."""
        ptr = lambda p: None if p is None else C.c_void_p(int(p))
        n, paths = C.c_uint(0), C.c_ulonglong(0)
        L.check(L.lib.twk_adaptive_plan(self._h, None if ap is None else C.byref(ap), None if plan is None else C.byref(plan), ptr(moments), ptr(counts),
                                        C.c_size_t(int(numElements)), ptr(activeOut), ptr(pathOffsetOut), C.byref(n), C.byref(paths)))
        return n.value, paths.value

    def renderPlanned(self):
        """twk_launch_adaptive_planned: the handle's plan as one wavefront pass, every entry at the iterations its own count says;
        asynchronous. A plan is rendered once: without a new adaptivePlan a second call is refused."""
        L.check(L.lib.twk_launch_adaptive_planned(self._h))

    def readPlan(self):
        """(active uint32 [numActive], pathOffset uint32 [numActive + 1]) of the last adaptivePlan on the handle's own buffers: entry
        k owns paths pathOffset[k] .. pathOffset[k + 1] - 1, pathOffset[-1] = numPaths."""
        n, paths = C.c_uint(0), C.c_ulonglong(0)
        L.check(L.lib.twk_read_plan(self._h, None, None, C.c_size_t(0), C.byref(n), C.byref(paths)))
        active, offsets = np.empty(n.value, dtype=np.uint32), np.empty(n.value + 1, dtype=np.uint32)
        L.check(L.lib.twk_read_plan(self._h, active.ctypes.data_as(C.POINTER(C.c_uint32)), offsets.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(active.size),
                                    C.byref(n), C.byref(paths)))
        return active, offsets

    def statsEnable(self, enable=True):
        L.check(L.lib.twk_stats_enable(self._h, int(bool(enable))))

    def statsGet(self, reset=True):
        s = L.LaunchStats()
        L.check(L.lib.twk_stats_get(self._h, C.byref(s), int(bool(reset))))
        return {name: (list(getattr(s, name)) if name in ("waveCycles", "shadePhaseWaveSteps", "shadePhaseLanes", "shadePhaseCycles") else getattr(s, name)) for name, _ in L.LaunchStats._fields_}

    def streamPeakGBps(self, nbytes=1 << 30, repeats=10):
        g = C.c_float(0)
        L.check(L.lib.twk_stream_peak_gbps(self._h, C.c_size_t(nbytes), int(repeats), C.byref(g)))
        return g.value

    def gatherPeak(self, table_bytes=32 << 20):
        """Divergent-gather ceiling in giga lane-loads (16 B each) per second (twk_gather_peak)."""
        g = C.c_float(0)
        L.check(L.lib.twk_gather_peak(self._h, C.c_size_t(int(table_bytes)), C.byref(g)))
        return g.value

    def debugTraceQueue(self, closest=None, shadow=None):
        """One launch of the persistent traversal kernel over explicit rays ([n, 8] each; either may be None).
        Returns (hit records float32 [n, 4] = t, beta, gamma, slot bits; instance int32 [n]; occluded int32 [m])."""
        c = np.zeros((0, 8), np.float32) if closest is None else np.ascontiguousarray(closest, np.float32).reshape(-1, 8)
        s = np.zeros((0, 8), np.float32) if shadow is None else np.ascontiguousarray(shadow, np.float32).reshape(-1, 8)
        rec = np.zeros((max(1, c.shape[0]), 4), np.float32)
        inst = np.full((max(1, c.shape[0]),), -1, np.int32)
        occ = np.zeros((max(1, s.shape[0]),), np.int32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.check(L.lib.twk_debug_trace_queue(self._h, c.ctypes.data_as(fp), C.c_size_t(c.shape[0]), s.ctypes.data_as(fp), C.c_size_t(s.shape[0]),
                                            rec.ctypes.data_as(fp), inst.ctypes.data_as(ip), occ.ctypes.data_as(ip)))
        return rec[:c.shape[0]], inst[:c.shape[0]], occ[:s.shape[0]]

    def readAcceleration(self):
        """(info dict, quantised wide nodes float32 [n, 16], triangle slots float32 [m, 12], instance records float32 [k, 32]) of the built scene."""
        info = L.AccelerationInfo()
        L.check(L.lib.twk_debug_read_acceleration(self._h, C.byref(info), None, None, None))
        nodes = np.zeros((info.numNodes, info.nodeFloats), np.float32)  # quantised 4-ary nodes (64 B) or compressed 8-ary nodes (80 B): info.nodeFloats
        tris = np.zeros((info.numTriangleSlots, 12), np.float32)
        inst = np.zeros((info.numInstances, 32), np.float32)
        L.check(L.lib.twk_debug_read_acceleration(self._h, C.byref(info), nodes.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p),
                                                  inst.ctypes.data_as(C.c_void_p)))
        return {name: getattr(info, name) for name, _ in L.AccelerationInfo._fields_}, nodes, tris, inst

    def debugShadeBuilds(self, reset=True):
        """The launcher indices of the shade kernel builds launched on this device since the last reset (twk_debug_shade_builds)."""
        mask = (C.c_uint64 * 2)()
        L.check(L.lib.twk_debug_shade_builds(self._h, mask, int(bool(reset))))
        return {i for i in range(128) if (mask[i >> 6] >> (i & 63)) & 1}

    def debugCapture(self, enable=True):
        L.check(L.lib.twk_debug_capture(self._h, int(bool(enable))))

    def debugReadFirstHits(self):
        n = self.state.resolution[1] * self.launchWidth
        tbg = np.empty((n, 3), dtype=np.float32)
        ids = np.empty((n, 2), dtype=np.int32)
        L.check(L.lib.twk_debug_read_first_hits(self._h, tbg.ctypes.data_as(C.POINTER(C.c_float)),
                                                ids.ctypes.data_as(C.POINTER(C.c_int)), C.c_size_t(n)))
        return tbg, ids

    def traceRays(self, rays, anyHit=False):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        tbg = np.zeros((n, 3), dtype=np.float32)
        ids = np.zeros((n, 2), dtype=np.int32)
        L.check(L.lib.twk_trace_rays(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(n), int(bool(anyHit)),
                                     tbg.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data_as(C.POINTER(C.c_int))))
        return tbg, ids

    def debugMath(self, op, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        yy = x if y is None else np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
        out = np.empty_like(x)
        L.check(L.lib.twk_debug_math(self._h, int(op), x.ctypes.data_as(C.POINTER(C.c_float)),
                                     yy.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                     C.c_size_t(x.size)))
        return out

    def debugExactDivision(self, first=0, count=0, x=None, d=None, seed=None):
        """The traversal kernel's short divisions against `/` on the device (twk_debug_exact_division): the reciprocal of the bit
        patterns first .. first + count - 1; or, with x and d, the quotients x / d and 1 / d of those pairs (|x| <= |d|); or, with
        seed, of `count` pairs drawn on the device. Returns (mismatches, operands that took the `/` fallback, first offenders as
        [(bits, bits), ...])."""
        fp = C.POINTER(C.c_float)
        mism, fall, off = C.c_uint64(0), C.c_uint64(0), (C.c_uint32 * 16)()
        if x is not None:
            xx = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
            dd = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
            assert xx.size == dd.size
            args = (1, 0, C.c_uint64(xx.size), xx.ctypes.data_as(fp), dd.ctypes.data_as(fp))
        elif seed is not None:
            args = (2, C.c_uint32(int(seed)), C.c_uint64(int(count)), None, None)
        else:
            args = (0, C.c_uint32(int(first)), C.c_uint64(int(count)), None, None)
        L.check(L.lib.twk_debug_exact_division(self._h, *args, C.byref(mism), C.byref(fall), off))
        n = min(8, mism.value)
        return mism.value, fall.value, [(off[2 * k], off[2 * k + 1]) for k in range(n)]
