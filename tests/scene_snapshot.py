"""Reads everything a built handle hands out about its acceleration structure: twk_debug_read_acceleration, twk_get_build_info and the
scene arrays of twk_debug_snapshot_scene (binary nodes, shading records, slots, the two top-of-tree caches, topRoot / topRoot2). What
tests/test_gpu_selective_update.py compares between two handles and tests/test_gpu_bvh_audit.py audits. A helper module, not a conftest.

The snapshot is read through the leading fields of LaunchParams that selective_scenes.SCENE_HEAD lists; tests/test_update_plan_host.py
holds those and the array sizes against the headers with a compiled program. The snapshot hands out no pair records (it clears
LaunchParams::trianglePairs: the host build of the kernels walks slots) and its quantised wide nodes are the canonical ones of
twk_debug_read_acceleration, so what the device keeps of a pair leaf shows in the two caches only."""
import ctypes as C

import numpy as np

import selective_scenes as S


class SceneHead(C.Structure):
    """The first fields of LaunchParams (csrc/device_types.h), which twk_debug_snapshot_scene fills with HOST copies of the scene arrays."""
    _fields_ = [(name, getattr(C, kind)) for name, kind in S.SCENE_HEAD]


def params_bytes(orc):
    lib = orc._load(orc.HOST_KERNELS_PATH)
    lib.hostk_params_bytes.restype = C.c_size_t
    return lib.hostk_params_bytes()


def read_scene(twk, orc, dev):
    """(arrays, TwkAccelerationInfo, TwkBuildInfo): float32 arrays `wideQ`, `slots`, `instances` (read-back), `binaryNodes`,
    `shadeRecords`, `snapshotSlots`, `topNodes`, `topNodes7` (snapshot) as rows of 4-byte words, and `topRoots`."""
    L = twk._lib
    info, nodes, tris, inst = dev.readAcceleration()
    build = dev.buildInfo()
    params = C.create_string_buffer(params_bytes(orc))
    L.check(L.lib.twk_debug_snapshot_scene(dev.handle, params, C.c_size_t(len(params))))
    head = SceneHead.from_buffer(params)
    copy = lambda pointer, nbytes, row: np.frombuffer(C.string_at(pointer, nbytes), np.float32).copy().reshape(-1, row // 4)
    out = {"wideQ": nodes, "slots": tris, "instances": inst,
           "binaryNodes": copy(head.nodes, S.NODE_BYTES * build["nodes"], S.NODE_BYTES),
           "shadeRecords": copy(head.shadeTriangles, S.SHADE_RECORD_BYTES * build["triangleSlots"], S.SHADE_RECORD_BYTES),
           "snapshotSlots": copy(head.triangles, S.SLOT_BYTES * build["triangleSlots"], S.SLOT_BYTES),
           "topNodes": copy(head.topNodes, S.QUANTISED_NODE_BYTES * S.TOP_NODES, S.QUANTISED_NODE_BYTES),
           "topNodes7": copy(head.topNodes7, S.QUANTISED_NODE_BYTES * S.TOP_NODES7, S.QUANTISED_NODE_BYTES),
           "topRoots": np.array([head.topRoot, head.topRoot2], np.int64)}
    return out, info, build


def readback(twk, orc, dev):
    """The handle as bvh_audit.Readback."""
    from bvh_audit import Readback
    a, info, build = read_scene(twk, orc, dev)
    assert np.array_equal(a["slots"].view(np.uint32), a["snapshotSlots"].view(np.uint32)), "the snapshot's slots are the read-back's"
    return Readback(nodes=a["binaryNodes"], wideQ=a["wideQ"], slots=a["slots"], shade=a["shadeRecords"], instances=a["instances"], topNodes=a["topNodes"],
                    topNodes7=a["topNodes7"], topRoot=int(a["topRoots"][0]), topRoot2=int(a["topRoots"][1]), pairs=None, info=info, build=build)
