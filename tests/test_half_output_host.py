"""The RGBA16F output format (≙ Optix7Gui's USE_FP32_OUTPUT 0, apps/Optix7Gui/shaders/app_config.h:57-59) where it needs no GPU:
the new entry points refuse a NULL handle before any HIP call, and the system description's grammar extension `outputFormat 0|1`
is read, reported and written back (only when it is 1, so that existing round-trip texts do not change)."""
import ctypes as C

import pytest

from conftest import scene_path


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        return app.outputFormat, app.systemDescription()
    finally:
        app.close()


@pytest.mark.parametrize("name,args", [
    ("twk_set_output_format", (1,)),
    ("twk_get_output_format", (C.byref(C.c_int(0)),)),
    ("twk_read_output_raw", (C.c_void_p(0), C.c_size_t(0))),
    ("twk_read_aov_raw", (0, C.c_void_p(0), C.c_size_t(0))),
    ("twk_compositor_half", (C.c_void_p(0), C.c_void_p(0))),
    ("twk_tonemap_half", (None, C.c_void_p(0), C.c_size_t(0), None)),
    ("twk_app_get_output_format", (C.byref(C.c_int(0)),)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    rc = getattr(L.lib, name)(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_output_format_constants_match_the_header():
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "tweeker_hip.h")).read()
    assert "enum { TWK_OUTPUT_FLOAT4 = 0, TWK_OUTPUT_HALF4 = 1 };" in header
    from tweeker_raytracer_amd import _lib as L
    assert (L.TWK_OUTPUT_FLOAT4, L.TWK_OUTPUT_HALF4) == (0, 1)


def test_output_format_from_the_system_description(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    fmt, text = _description(twk, base)
    assert fmt == 0 and "outputFormat" not in text
    # without the keyword the description round-trips to the same text as before
    again_fmt, again = _description(twk, text)
    assert again_fmt == 0 and again == text

    half_fmt, half_text = _description(twk, base + "\noutputFormat 1\n")
    assert half_fmt == 1
    assert "outputFormat 1\n" in half_text
    # the line is the only difference, and it survives a round trip
    assert half_text.replace("outputFormat 1\n", "") == text
    assert _description(twk, half_text) == (1, half_text)

    zero_fmt, zero_text = _description(twk, base + "\noutputFormat 0\n")
    assert zero_fmt == 0 and zero_text == text
