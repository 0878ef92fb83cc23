"""CPU: the frames of a positions-mode device source (csrc/vertex_source_device.h) through their host form twk_vertex_frames_host —
no GPU. The kernel runs the same TWK_HD function, so what holds here bit for bit is what tests/test_gpu_vertex_source.py holds the
device to.
  - twk_vertex_frames_host equals tests/vertex_source_restate.py (numpy, operation by operation in float32) bit for bit on a 12 x 6
    sphere (poles with zero-area triangles, a duplicated seam), a box (every vertex on one face), a single triangle, a mesh with a
    vertex no index names, a fan folded flat and a tangent along the normal, each under the noise, scale and collapse deformations of
    tests/refit_scenes.py and as built; the three special vertices keep what the definition says they keep
  - against a float64 evaluation of the same formula on the noise-deformed sphere: the largest angle between the two normals
    measured here was 1.273e-7 rad (the tangents: 1.781e-7 rad); the asserted bound is that times 4, rounded up to a power of two:
    2^-20 rad for both (profiles/r29_vertex_source.md)
  - every refusal
  - the same host code under the address and undefined-behaviour sanitizers, in a stand-alone program (tests/vertex_source_host.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refit_scenes as RS
import vertex_source_restate as V
from conftest import ROOT

F32, U32 = np.float32, np.uint32
DEFORMATIONS = ("noise", "scale", "collapse")
ANGLE_BOUND = 2.0 ** -20  # rad; measured 1.273e-7 (normals) and 1.781e-7 (tangents), times 4, up to a power of two


def _cases(twk):
    for name, attributes, indices in V.meshes(twk):
        yield name, "as built", attributes, indices, attributes[:, 0:3].copy()
        for k, deformation in enumerate(DEFORMATIONS):
            yield name, deformation, attributes, indices, RS.deform(attributes, deformation, seed=k)[:, 0:3].copy()


def test_the_host_form_equals_the_restatement_bit_for_bit(twk):
    ran = 0
    for name, deformation, attributes, indices, positions in _cases(twk):
        got = twk.vertex_frames_host(positions, indices, attributes)
        want = V.frames(positions, indices, attributes)
        bad = np.nonzero((got.view(U32) != want.view(U32)).any(1))[0]
        assert bad.size == 0, f"{name}, {deformation}: {bad.size} records differ, first {bad[0]}: {got[bad[0]]} against {want[bad[0]]}"
        assert np.array_equal(got[:, 0:3].view(U32), positions.view(U32)) and np.array_equal(got[:, 9:12].view(U32), attributes[:, 9:12].view(U32)), f"{name}: positions in, texcoords kept"
        ran += 1
    assert ran == 6 * 4


def test_the_vertices_the_definition_keeps(twk):
    meshes = {name: (a, i) for name, a, i in V.meshes(twk)}
    # no index names vertex 3: its normal stays under every deformation (its tangent is made perpendicular to it all the same)
    a, i = meshes["an unnamed vertex"]
    a = a.copy()
    a[3, 6:9] = (0.0, 0.6, 0.8)
    for deformation in DEFORMATIONS:
        got = twk.vertex_frames_host(RS.deform(a, deformation)[:, 0:3], i, a)
        assert np.array_equal(got[3, 6:9].view(U32), a[3, 6:9].view(U32)), deformation
    # the folded fan: the two cross products at vertex 0 cancel exactly as built and scaled; the other vertices get a new normal
    a, i = meshes["a fan folded flat"]
    a = a.copy()
    a[:, 6:9] = (0.0, 0.6, 0.8)
    for positions in (a[:, 0:3], RS.deform(a, "scale")[:, 0:3]):
        got = twk.vertex_frames_host(positions, i, a)
        assert np.array_equal(got[0, 6:9].view(U32), a[0, 6:9].view(U32)), "vertex 0 keeps its normal"
        assert np.allclose(got[1, 6:9], [0, 0, 1], atol=1e-6) and np.allclose(got[3, 6:9], [0, 0, -1], atol=1e-6), got[:, 6:9]
    # a tangent along the new normal: t* is exactly zero and the old tangent stays, length and all
    a, i = meshes["a tangent along the normal"]
    a = a.copy()
    a[:, 3:6] = (0.0, 0.0, 2.0)
    got = twk.vertex_frames_host(a[:, 0:3], i, a)
    assert np.array_equal(got[:, 3:6].view(U32), a[:, 3:6].view(U32)) and np.array_equal(got[:, 6:9], np.tile(F32([0, 0, 1]), (3, 1)))
    # every vertex on one point: every sum is zero and every normal and tangent of the sphere stays
    a, i = meshes["sphere 12 x 6"]
    got = twk.vertex_frames_host(RS.deform(a, "collapse")[:, 0:3], i, a)
    assert np.array_equal(got[:, 6:9].view(U32), a[:, 6:9].view(U32))


def _angles(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


def test_against_float64_on_the_deformed_sphere(twk):
    name, attributes, indices = V.meshes(twk)[0]
    positions = RS.deform(attributes, "noise")[:, 0:3]
    got = twk.vertex_frames_host(positions, indices, attributes)
    want = V.frames(positions, indices, attributes, kind=np.float64)
    normal, tangent = _angles(got[:, 6:9], want[:, 6:9]).max(), _angles(got[:, 3:6], want[:, 3:6]).max()
    print(f"{name}, noise: largest angle to the float64 evaluation: normals {normal:.3e} rad, tangents {tangent:.3e} rad; bound {ANGLE_BOUND:.3e}")
    assert normal <= ANGLE_BOUND and tangent <= ANGLE_BOUND, (normal, tangent)
    assert np.abs(np.linalg.norm(got[:, 6:9].astype(np.float64), axis=1) - 1.0).max() < 2e-7


def test_refusals(twk):
    L = twk._lib
    VALUE = L.TWK_ERROR_INVALID_VALUE
    _, a, i = V.meshes(twk)[1]
    p, out = np.ascontiguousarray(a[:, 0:3]), np.empty_like(a)
    fp, up, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.c_void_p

    def args(indices=i, vertices=a.shape[0]):
        return [p.ctypes.data_as(fp), C.c_size_t(vertices), indices.ctypes.data_as(up), C.c_size_t(indices.size), a.ctypes.data_as(vp), out.ctypes.data_as(vp)]

    assert L.lib.twk_vertex_frames_host(*args()) == L.TWK_SUCCESS, L.lib.twk_last_error().decode()
    for k in (0, 2, 4, 5):
        x = args()
        x[k] = None
        assert L.lib.twk_vertex_frames_host(*x) == VALUE and "twk_vertex_frames_host: NULL" in L.lib.twk_last_error().decode(), k
    assert L.lib.twk_vertex_frames_host(*args(indices=i[:-1])) == VALUE and "multiple of three" in L.lib.twk_last_error().decode()
    assert L.lib.twk_vertex_frames_host(*args(indices=i[:0])) == VALUE
    beyond = i.copy()
    beyond[7] = a.shape[0]
    assert L.lib.twk_vertex_frames_host(*args(indices=beyond)) == VALUE and "index 7 is beyond the vertices" in L.lib.twk_last_error().decode()
    assert L.lib.twk_vertex_frames_host(*args(vertices=0)) == VALUE
    # the device forms refuse a NULL handle and a NULL source before any HIP call, under their own names
    src = L.VertexSource()
    for name in ("twk_update_geometry_vertices_device", "twk_refit_geometry_vertices_device"):
        assert getattr(L.lib, name)(None, 0, C.byref(src), C.c_size_t(1)) == VALUE and name + ": NULL device handle" in L.lib.twk_last_error().decode()
    assert L.lib.twk_read_geometry_vertices(None, 0, out.ctypes.data_as(vp), C.c_size_t(1)) == VALUE and "twk_read_geometry_vertices: NULL device handle" in L.lib.twk_last_error().decode()
    for method in ("updateGeometryVerticesDevice", "refitGeometryVerticesDevice", "readGeometryVertices"):
        assert callable(getattr(twk.Device, method))
    assert L.lib.twk_abi_version() == 9


def test_the_host_form_runs_clean_under_the_sanitizers(twk, tmp_path):
    """Every mesh under every deformation through the stand-alone program (tests/vertex_source_host.cpp): it exits 0 with nothing on
    stderr, and what it computed has twk_vertex_frames_host's bits. Nothing is loaded into Python under a sanitizer."""
    out = str(tmp_path / "vertex_source_host")
    hip_inc = os.environ.get("HIP_INC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "tweeker_raytracer_amd", "csrc"),
                    "-o", out, os.path.join(ROOT, "tests", "vertex_source_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    ran = 0
    for name, deformation, attributes, indices, positions in _cases(twk):
        case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
        with open(case, "wb") as f:
            f.write(np.array([attributes.shape[0], indices.size], np.int32).tobytes())
            for array, kind in ((positions, F32), (indices, U32), (attributes, F32)):
                f.write(np.ascontiguousarray(array, kind).tobytes())
        run = subprocess.run([out, case, result], capture_output=True, text=True, env=env)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
        want = twk.vertex_frames_host(positions, indices, attributes)
        assert np.array_equal(np.fromfile(result, U32), want.view(U32).reshape(-1)), f"{name}, {deformation}"
        ran += 1
    assert ran == 24
