"""The variance-guided, firefly-clamping mode of the denoiser (twk_denoise_variance) where it needs no GPU: the new entry points
refuse a NULL handle before any HIP call, twk_denoiser_variance_defaults and the struct are what the header says, and the system
description's keys `denoiserVariance`, `denoiserFirefly`, `denoiserSigmaLuminance` are read, dropped when twk_denoise_variance would
refuse them, reported, and written back only when they differ from off / the defaults, so that existing round-trip texts do not
change."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT, scene_path

DEFAULTS = (3.0, 4.0)  # fireflyThreshold, sigmaLuminance


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, dv = app.denoiserVariance
        return (on, dv.fireflyThreshold, dv.sigmaLuminance), app.systemDescription()
    finally:
        app.close()


@pytest.mark.parametrize("name,args", [
    ("twk_denoise_variance", (None, None, None, None, None, 0, 0, None)),
    ("twk_denoiser_variance_defaults", ()),
    ("twk_app_get_denoiser_variance", (None, None)),
])
def test_new_entry_points_refuse_a_null_handle(twk, name, args):
    L = twk._lib
    rc = getattr(L.lib, name)(None, *args)
    assert rc == L.TWK_ERROR_INVALID_VALUE
    assert name in L.lib.twk_last_error().decode()


def test_defaults_and_struct_match_the_header(twk, tmp_path):
    L = twk._lib
    path = os.path.join(ROOT, "include", "tweeker_hip.h")
    header = open(path).read()
    assert "#define TWK_ABI_VERSION 9" in header
    dv = L.DenoiserVariance(-1.0, -1.0)
    assert L.lib.twk_denoiser_variance_defaults(C.byref(dv)) == 0
    assert (dv.fireflyThreshold, dv.sigmaLuminance) == DEFAULTS
    assert bytes(L.DenoiserVariance()) == bytes(dv)  # the Python structure's own defaults are the library's
    # the comment above the declaration states them
    stated = re.search(r"/\* fireflyThreshold ([0-9.]+), sigmaLuminance ([0-9.]+) \*/\s*int twk_denoiser_variance_defaults", header)
    assert stated and (float(stated.group(1)), float(stated.group(2))) == DEFAULTS
    # layout against the header itself, as tests/test_cabi_layouts.py does for the older structs
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{path}"\nint main(void) {{ printf("%zu %zu %zu %zu\\n", sizeof(TwkDenoiserVariance), '
                   "offsetof(TwkDenoiserVariance, fireflyThreshold), offsetof(TwkDenoiserVariance, sigmaLuminance), sizeof(TwkDenoiser)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, first, second, denoiser = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (size, first, second) == (C.sizeof(L.DenoiserVariance), L.DenoiserVariance.fireflyThreshold.offset, L.DenoiserVariance.sigmaLuminance.offset) == (8, 0, 4)
    assert denoiser == C.sizeof(L.Denoiser) == 28


def test_variance_keys_of_the_system_description(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    off, text = _description(twk, base)
    assert off == (False,) + DEFAULTS
    for key in ("denoiserVariance", "denoiserFirefly", "denoiserSigmaLuminance"):
        assert key not in text
    # absent: the description round-trips to the same text as before
    assert _description(twk, text) == (off, text)
    # off and the defaults write nothing
    assert _description(twk, base + "\ndenoiserVariance 0\ndenoiserFirefly 3\ndenoiserSigmaLuminance 4\n") == (off, text)

    on, on_text = _description(twk, base + "\ndenoiser 3\ndenoiserVariance 1\n")
    assert on == (True,) + DEFAULTS
    assert on_text.replace("denoiserVariance 1\n", "").replace("denoiser 3\n", "") == text
    assert _description(twk, on_text) == (on, on_text)

    custom, custom_text = _description(twk, base + "\ndenoiser 3\ndenoiserVariance 1\ndenoiserFirefly 2.5\ndenoiserSigmaLuminance 0.75\n")
    assert custom == (True, 2.5, 0.75)
    for line in ("denoiserVariance 1\n", "denoiserFirefly 2.5\n", "denoiserSigmaLuminance 0.75\n"):
        assert custom_text.count(line) == 1
    assert _description(twk, custom_text) == (custom, custom_text)
    # the clamp switched off is a value of its own
    assert _description(twk, base + "\ndenoiserFirefly 0\n")[0] == (False, 0.0, DEFAULTS[1])
    # the switch is 0 or 1: anything else is off
    assert _description(twk, base + "\ndenoiserVariance 7\n")[0][0] is False
    # what twk_denoise_variance would refuse drops the line, the previous value stays
    assert _description(twk, base + "\ndenoiserFirefly 2.5\ndenoiserFirefly -1\n")[0] == (False, 2.5, DEFAULTS[1])
    assert _description(twk, base + "\ndenoiserSigmaLuminance 0\n")[0] == (False,) + DEFAULTS
    assert _description(twk, base + "\ndenoiserSigmaLuminance -2\n")[0] == (False,) + DEFAULTS
    # the values are settings kept beside a switch that is off
    kept, kept_text = _description(twk, base + "\ndenoiserVariance 0\ndenoiserFirefly 2.5\n")
    assert kept == (False, 2.5, DEFAULTS[1]) and "denoiserFirefly 2.5\n" in kept_text and "denoiserVariance" not in kept_text


def test_a_description_without_the_keys_keeps_its_text(twk):
    """The keys of twk_denoise and everything else written back are what they were: with the three new keys absent the text of a
    description that uses the older denoiser keys round-trips unchanged, and holds none of the new ones."""
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    _, text = _description(twk, base + "\ndenoiser 3\ndenoiserIterations 5\ndenoiserSigmas 2.5 0.125 0.25\n")
    assert "denoiserVariance" not in text and "denoiserFirefly" not in text and "denoiserSigmaLuminance" not in text
    assert text.count("denoiser") == 3
    assert _description(twk, text)[1] == text
