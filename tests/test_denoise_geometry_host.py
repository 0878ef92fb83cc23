"""The geometry guide of the denoiser (twk_denoise_geometry: plane and instance stops from the geometry AOV) where it needs no GPU.
twk_denoise_geometry_host is csrc/denoise_device.h compiled for the host; tests/denoise_geometry_restate.py is the same definition in
numpy float32. They must agree in every bit, in all three modes of the filter; with a geometry of misses only the result is that of
the existing calls (through the existing restatements); and on the step scene, where albedo and normal cannot tell the two halves
apart, the guide separates them exactly. Then the refusals, the struct, the defaults and the keys of the system description."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from denoise_geometry_restate import CAMERA, restate, step_scene, synthetic

F = np.float32
MODES = ("plain", "variance", "sampled")


def _exp(orc):
    return lambda x: orc.oracle_math(2, x)


def _sqrt(orc):
    return lambda x: orc.oracle_math(6, x)


def _fp(a):
    return None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))


def host(L, dn, dg, beauty, albedo, normal, geometry, camera=CAMERA, dv=None, moments=None, min_samples=0, out=None, shape=None):
    """twk_denoise_geometry_host; returns (return code, float32 [H, W, 4])."""
    h, w = shape if shape is not None else beauty.shape[:2]
    arrays = [None if a is None else np.ascontiguousarray(a, F) for a in (beauty, albedo, normal, moments, geometry)]
    cam = None if camera is None else np.ascontiguousarray(camera, F)
    result = np.zeros((h, w, 4), F) if out is None else out
    fn = L.lib.twk_denoise_geometry_host
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.POINTER(C.c_float)] * 6 + [C.c_int, C.c_int, C.POINTER(C.c_float)]
    rc = fn(None if dn is None else C.addressof(dn), None if dg is None else C.addressof(dg), None if dv is None else C.addressof(dv), int(min_samples),
            *[_fp(a) for a in arrays], _fp(cam), int(w), int(h), result.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, result


def _mode(L, mode):
    """(dv, uses moments, minSamples) of a mode."""
    if mode == "plain":
        return None, False, 0
    if mode == "variance":
        return L.DenoiserVariance(), False, 0
    return L.DenoiserVariance(fireflyThreshold=2.0), True, 4


def _same_bits(got, expect, what):
    diff = got.view(np.uint32) != expect.view(np.uint32)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} values differ in their bits, first at {np.argwhere(diff)[:4].tolist()}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(19, 37), (21, 70)], ids=["37x19", "70x21"])
def test_host_form_equals_the_restatement_bit_for_bit(twk, orc, shape, mode):
    """5 levels (steps 8 and 16 exceed the height), demodulation on and off, instanceStop off and on, on the synthetic picture: two
    parallel planes of equal albedo and normal, misses, two instances on one plane, NaN and inf in every input, a hit at the camera."""
    L = twk._lib
    beauty, albedo, normal, moments, geometry = synthetic(*shape)
    dv, use_moments, min_samples = _mode(L, mode)
    for demod, stop, sigma in ((1, 0, 0.01), (0, 1, 0.03)):
        dn = L.Denoiser(iterations=5, demodulateAlbedo=demod, sigmaColor=1.5)
        dg = L.DenoiserGeometry(sigmaPosition=sigma, instanceStop=stop)
        rc, got = host(L, dn, dg, beauty, albedo, normal, geometry, dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
        assert rc == 0, L.lib.twk_last_error()
        expect, through = restate(beauty, albedo, normal, geometry, CAMERA, dn, dg, _exp(orc), _sqrt(orc), dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
        _same_bits(got, expect, f"{mode}, demodulate {demod}, instanceStop {stop}")
        assert np.array_equal(got[through].view(np.uint32), beauty[through].view(np.uint32))
        assert np.isfinite(got[~through][..., :3]).all()
    # the guide does something here: without the far plane's stop the picture differs
    flat = geometry.copy()
    flat[..., 3] = 0.0
    flat[..., :3] = 0.0
    _, unguided = host(L, dn, dg, beauty, albedo, normal, flat, dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
    assert not np.array_equal(unguided.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("mode", MODES)
def test_an_all_miss_geometry_gives_the_existing_calls_bits(twk, orc, mode):
    """The anchor: with misses only no tap gets a term and no centre passes through, so the result is twk_denoise's,
    twk_denoise_variance's and twk_denoise_variance_sampled's, as their own restatements (tests/test_gpu_denoise*.py) state them."""
    from test_gpu_denoise import _restate
    from test_gpu_denoise_sampled import restate_sampled
    from test_gpu_denoise_variance import restate_variance
    L = twk._lib
    beauty, albedo, normal, moments, _ = synthetic(19, 37)
    geometry = np.zeros_like(beauty)
    dv, use_moments, min_samples = _mode(L, mode)
    for demod in (1, 0):
        dn = L.Denoiser(iterations=5, demodulateAlbedo=demod, sigmaColor=1.5)
        rc, got = host(L, dn, L.DenoiserGeometry(instanceStop=demod), beauty, albedo, normal, geometry, dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
        assert rc == 0, L.lib.twk_last_error()
        if mode == "plain":
            expect, _ = _restate(beauty, albedo, normal, dn, _exp(orc))
        elif mode == "variance":
            expect, _ = restate_variance(beauty, albedo, normal, dn, dv, _exp(orc), _sqrt(orc))
        else:
            expect, _ = restate_sampled(beauty, albedo, normal, moments, min_samples, dn, dv, _exp(orc), _sqrt(orc))
        _same_bits(got, expect, f"{mode}, demodulate {demod}")
        # ... and the restatement of the guide says the same
        again, _ = restate(beauty, albedo, normal, geometry, CAMERA, dn, L.DenoiserGeometry(), _exp(orc), _sqrt(orc), dv=dv, moments=moments if use_moments else None, min_samples=min_samples)
        _same_bits(again, expect, f"restatement, {mode}, demodulate {demod}")


def test_the_step_scene_is_separated_exactly(twk, orc):
    """40 x 24: colour exactly 1 on the left, exactly 0 on the right, albedo and normal identical, sigmaColor large. twk_denoise
    (restated) bleeds across the edge. With the halves on two parallel planes every cross-edge tap has d = 1.5, vv < 40 and
    t > 2.25 x 10^4 / 40 > 87: the guided result is exactly 1 and exactly 0. With the halves on one plane as two instances the same
    holds with instanceStop 1, and with instanceStop 0 they mix (d = 0 across the edge)."""
    from test_gpu_denoise import _restate
    L = twk._lib
    beauty, albedo, normal, geometry = step_scene()
    dn = L.Denoiser(iterations=4, sigmaColor=100.0)
    dg = L.DenoiserGeometry(sigmaPosition=0.01)
    bled, _ = _restate(beauty, albedo, normal, dn, _exp(orc))
    assert ((bled[..., :3] > 0) & (bled[..., :3] < 1)).any()
    for dv in (None, L.DenoiserVariance()):
        rc, got = host(L, dn, dg, beauty, albedo, normal, geometry, dv=dv)
        assert rc == 0
        assert np.array_equal(got, beauty), "planes"
    beauty, albedo, normal, geometry = step_scene(instances=True)
    rc, got = host(L, dn, L.DenoiserGeometry(sigmaPosition=0.01, instanceStop=1), beauty, albedo, normal, geometry)
    assert rc == 0 and np.array_equal(got, beauty), "instances, instanceStop 1"
    rc, got = host(L, dn, L.DenoiserGeometry(sigmaPosition=0.01, instanceStop=0), beauty, albedo, normal, geometry)
    assert rc == 0 and ((got[..., :3] > 0) & (got[..., :3] < 1)).any(), "instances, instanceStop 0"
    expect, _ = restate(beauty, albedo, normal, geometry, CAMERA, dn, L.DenoiserGeometry(sigmaPosition=0.01), _exp(orc), _sqrt(orc))
    _same_bits(got, expect, "instances, instanceStop 0")


@pytest.mark.parametrize("name,args", [
    ("twk_denoise_geometry", (None, None, None, 0, None, None, None, None, None, None, 0, 0, None)),
    ("twk_denoiser_geometry_defaults", ()),
    ("twk_app_get_denoiser_geometry", (None, None)),
    ("twk_denoise_geometry_host", (None, None, 0, None, None, None, None, None, None, 0, 0, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    fn = getattr(L.lib, name)
    fn.argtypes = None
    rc = fn(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_refusals_of_the_host_form(twk):
    L = twk._lib
    beauty, albedo, normal, geometry = step_scene()
    good_dn, good_dg = L.Denoiser(), L.DenoiserGeometry()

    def refused(**kw):
        args = dict(dn=good_dn, dg=good_dg, beauty=beauty, albedo=albedo, normal=normal, geometry=geometry)
        args.update(kw)
        rc, _ = host(L, args.pop("dn"), args.pop("dg"), args.pop("beauty"), args.pop("albedo"), args.pop("normal"), args.pop("geometry"), **args)
        assert rc == L.TWK_ERROR_INVALID_VALUE, kw
        text = L.lib.twk_last_error().decode()
        assert "twk_denoise_geometry_host" in text
        return text

    assert host(L, good_dn, good_dg, beauty, albedo, normal, geometry)[0] == 0
    for kind in (0, 1):
        assert "inputKind" in refused(dn=L.Denoiser(inputKind=kind))
    for sigma in (0.0, -1.0, 1e30, 1e-30, float("nan"), float("inf")):
        assert "sigmaPosition" in refused(dg=L.DenoiserGeometry(sigmaPosition=sigma))
    refused(dn=L.Denoiser(iterations=9))
    refused(dn=L.Denoiser(sigmaNormal=0.0))
    refused(dv=L.DenoiserVariance(sigmaLuminance=0.0))
    refused(dv=L.DenoiserVariance(), min_samples=1, moments=beauty)
    refused(min_samples=4, moments=beauty)  # sampled variance without the mode's parameters
    refused(dv=L.DenoiserVariance(), min_samples=4)  # ... without moments
    refused(geometry=None)
    refused(camera=None)
    degenerate = CAMERA.copy()
    degenerate[3:6] = 0.0
    assert "camera" in refused(camera=degenerate)
    # the output on top of an input
    for k, name in enumerate(("beauty", "albedo", "normal", "geometry")):
        arrays = [np.ascontiguousarray(a, F) for a in (beauty, albedo, normal, geometry)]
        assert "overlaps" in refused(**{name: arrays[k], "out": arrays[k]})
    refused(shape=(0, 4))


def test_struct_defaults_and_header(twk, tmp_path):
    L = twk._lib
    path = os.path.join(ROOT, "include", "tweeker_hip.h")
    header = open(path).read()
    assert "#define TWK_ABI_VERSION 9" in header
    dg = L.DenoiserGeometry(-1.0, 1)
    assert L.lib.twk_denoiser_geometry_defaults(C.byref(dg)) == 0
    assert (dg.sigmaPosition, dg.instanceStop) == (C.c_float(L.TWK_DENOISER_SIGMA_POSITION).value, 0)
    assert bytes(L.DenoiserGeometry()) == bytes(dg)  # the Python structure's own defaults are the library's
    stated = re.search(r"#define TWK_DENOISER_SIGMA_POSITION ([0-9.]+)f", header)
    assert stated and float(stated.group(1)) == L.TWK_DENOISER_SIGMA_POSITION
    assert re.search(r"/\* sigmaPosition TWK_DENOISER_SIGMA_POSITION, instanceStop 0 \*/\s*int twk_denoiser_geometry_defaults", header)
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{path}"\nint main(void) {{ printf("%zu %zu %zu %zu %zu %d\\n", sizeof(TwkDenoiserGeometry), '
                   "offsetof(TwkDenoiserGeometry, sigmaPosition), offsetof(TwkDenoiserGeometry, instanceStop), sizeof(TwkDenoiser), sizeof(TwkDenoiserVariance), TWK_PLANE_COUNT); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, first, second, denoiser, variance, planes = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (size, first, second) == (C.sizeof(L.DenoiserGeometry), L.DenoiserGeometry.sigmaPosition.offset, L.DenoiserGeometry.instanceStop.offset) == (8, 0, 4)
    assert (denoiser, variance, planes) == (C.sizeof(L.Denoiser), C.sizeof(L.DenoiserVariance), 6) == (28, 8, 6)


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, dg = app.denoiserGeometry
        return (on, dg.sigmaPosition, dg.instanceStop), app.systemDescription()
    finally:
        app.close()


def test_geometry_keys_of_the_system_description(twk):
    L = twk._lib
    default = C.c_float(L.TWK_DENOISER_SIGMA_POSITION).value
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    off, text = _description(twk, base)
    assert off == (False, default, 0)
    for key in ("denoiserGeometry", "denoiserSigmaPosition", "denoiserInstanceStop"):
        assert key not in text
    # absent, 0 and the defaults round-trip to the unchanged text
    assert _description(twk, text) == (off, text)
    assert _description(twk, base + "\ndenoiserGeometry 0\ndenoiserInstanceStop 0\ndenoiserSigmaPosition 0.01\n") == (off, text)
    older = base + "\ndenoiser 3\ndenoiserIterations 5\ndenoiserVariance 1\n"
    assert _description(twk, older + "denoiserGeometry 0\n")[1] == _description(twk, older)[1]

    on, on_text = _description(twk, base + "\ndenoiser 3\ndenoiserGeometry 1\n")
    assert on == (True, default, 0)
    assert on_text.replace("denoiserGeometry 1\n", "").replace("denoiser 3\n", "") == text
    assert _description(twk, on_text) == (on, on_text)

    custom, custom_text = _description(twk, base + "\ndenoiser 3\ndenoiserGeometry 1\ndenoiserSigmaPosition 0.025\ndenoiserInstanceStop 1\n")
    assert custom == (True, C.c_float(0.025).value, 1)
    for line in ("denoiserGeometry 1\n", "denoiserSigmaPosition 0.025\n", "denoiserInstanceStop 1\n"):
        assert custom_text.count(line) == 1
    assert _description(twk, custom_text) == (custom, custom_text)
    # the switches are 0 or 1: anything else is off
    assert _description(twk, base + "\ndenoiserGeometry 7\n")[0][0] is False
    assert _description(twk, base + "\ndenoiserInstanceStop 3\n")[0][2] == 0
    # what twk_denoise_geometry would refuse drops the line, the previous value stays
    for bad in ("0", "-0.01", "1e30", "1e-30"):
        assert _description(twk, base + f"\ndenoiserSigmaPosition 0.025\ndenoiserSigmaPosition {bad}\n")[0] == (False, C.c_float(0.025).value, 0), bad
    # the values are settings kept beside a switch that is off
    kept, kept_text = _description(twk, base + "\ndenoiserGeometry 0\ndenoiserSigmaPosition 0.025\n")
    assert kept == (False, C.c_float(0.025).value, 0) and "denoiserSigmaPosition 0.025\n" in kept_text and "denoiserGeometry" not in kept_text
