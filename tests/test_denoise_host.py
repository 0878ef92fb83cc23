"""The denoiser (twk_denoise: the edge-avoiding a-trous wavelet filter at the seam of Optix7Gui's optixDenoiserInvoke) where it needs
no GPU: the new entry points refuse a NULL handle before any HIP call, twk_denoiser_defaults and the enum are what the header says,
and the system description's grammar extensions `denoiser`, `denoiserIterations`, `denoiserSigmas` are read, reported and written
back only when they differ from off / the defaults, so that existing round-trip texts do not change."""
import ctypes as C
import os

import pytest

from conftest import ROOT, scene_path


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, dn = app.denoiser
        return (on, dn.inputKind, dn.iterations, dn.sigmaColor, dn.sigmaNormal, dn.sigmaAlbedo, dn.demodulateAlbedo, dn.blendFactor), app.systemDescription()
    finally:
        app.close()


def _f(v):
    return C.c_float(v).value  # the float32 nearest to v


@pytest.mark.parametrize("name,args", [
    ("twk_denoise", (None, None, None, None, 0, 0, None)),
    ("twk_read_denoised", (None, C.c_size_t(0))),
    ("twk_read_denoised_raw", (C.c_void_p(0), C.c_size_t(0))),
    ("twk_get_denoised_device_pointer", (None, None)),
    ("twk_denoiser_defaults", ()),
    ("twk_app_get_denoiser", (None, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    rc = getattr(L.lib, name)(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_defaults_and_constants_match_the_header(twk):
    L = twk._lib
    header = open(os.path.join(ROOT, "include", "tweeker_hip.h")).read()
    assert "enum { TWK_DENOISER_RGB = 0, TWK_DENOISER_RGB_ALBEDO = 1, TWK_DENOISER_RGB_ALBEDO_NORMAL = 2 };" in header
    assert (L.TWK_DENOISER_RGB, L.TWK_DENOISER_RGB_ALBEDO, L.TWK_DENOISER_RGB_ALBEDO_NORMAL) == (0, 1, 2)
    dn = L.Denoiser(0, 0, 0.0, 0.0, 0.0, 0, 1.0)
    assert C.sizeof(dn) == 28
    assert L.lib.twk_denoiser_defaults(C.byref(dn)) == 0
    got = (dn.inputKind, dn.iterations, dn.sigmaColor, dn.sigmaNormal, dn.sigmaAlbedo, dn.demodulateAlbedo, dn.blendFactor)
    assert got == (2, 3, 8.0, _f(0.3), _f(0.1), 1, 0.0)
    py = L.Denoiser()  # the Python structure's own defaults are the library's
    assert bytes(py) == bytes(dn)
    assert L.Denoiser(inputKind=L.TWK_DENOISER_RGB).demodulateAlbedo == 0


def test_denoiser_keys_of_the_system_description(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    defaults = (2, 3, 8.0, _f(0.3), _f(0.1), 1, 0.0)
    off, text = _description(twk, base)
    assert off == (False,) + defaults and "denoiser" not in text
    # absent: the description round-trips to the same text as before
    assert _description(twk, text) == (off, text)

    # `denoiser 0` writes nothing
    zero, zero_text = _description(twk, base + "\ndenoiser 0\n")
    assert zero == off and zero_text == text

    on, on_text = _description(twk, base + "\ndenoiser 3\n")
    assert on == (True,) + defaults
    assert on_text.replace("denoiser 3\n", "") == text and "denoiserIterations" not in on_text and "denoiserSigmas" not in on_text
    assert _description(twk, on_text) == (on, on_text)

    # non-default sigmas and iterations survive a round trip
    custom, custom_text = _description(twk, base + "\ndenoiser 3\ndenoiserIterations 5\ndenoiserSigmas 2.5 0.125 0.25\n")
    assert custom == (True, 2, 5, 2.5, 0.125, 0.25, 1, 0.0)
    for line in ("denoiser 3\n", "denoiserIterations 5\n", "denoiserSigmas 2.5 0.125 0.25\n"):
        assert line in custom_text
        custom_text_without = custom_text.replace(line, "")
        assert len(custom_text_without) == len(custom_text) - len(line)
    assert _description(twk, custom_text) == (custom, custom_text)

    # inputKind = key - 1; the unguided kind does not demodulate (it has no albedo to divide by)
    rgb, _ = _description(twk, base + "\ndenoiser 1\n")
    assert rgb[:2] == (True, 0) and rgb[6] == 0
    albedo, _ = _description(twk, base + "\ndenoiser 2\n")
    assert albedo[:2] == (True, 1) and albedo[6] == 1
    # out of range: off / clamped, like the other extension keys
    assert _description(twk, base + "\ndenoiser 7\n")[0][0] is False
    assert _description(twk, base + "\ndenoiser 3\ndenoiserIterations 99\n")[0][2] == 8
    # a sigma <= 0 is what twk_denoise refuses: such a line is dropped, the previous values stay
    assert _description(twk, base + "\ndenoiser 3\ndenoiserSigmas 2.5 0 0.25\n")[0] == (True,) + defaults
    # iterations and sigmas beside `denoiser 0` are settings kept for when it is switched on
    kept, kept_text = _description(twk, base + "\ndenoiser 0\ndenoiserIterations 5\n")
    assert kept == (False, 2, 5, 8.0, _f(0.3), _f(0.1), 1, 0.0) and "denoiserIterations 5\n" in kept_text and "denoiser 0" not in kept_text
