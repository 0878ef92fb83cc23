"""CPU: the moving-camera loop on a tiled frame, as far as it can be checked without a device — the new entry points and Python
methods exist and the ABI is still 9, every new call refuses a NULL handle with its own name in the text before any HIP call, the
"temporal*" keys of the system description parse, drop what the calls would refuse and are read back by twk_app_get_temporal, and a
description without them round-trips unchanged."""
import ctypes as C

import numpy as np

from conftest import scene_path

NEW_SYMBOLS = ("twk_render_geometry_tile", "twk_assemble_with_geometry", "twk_assemble_devices_with_geometry", "twk_get_assembled_geometry_device_pointer",
               "twk_read_assembled_geometry", "twk_temporal_accumulate_assembled", "twk_app_get_temporal")
NEW_METHODS = ("renderGeometryTile", "assembleWithGeometry", "assembleFromWithGeometry", "assembledGeometryDevicePointer", "readAssembledGeometry",
               "temporalAccumulateAssembled")


def test_the_abi_is_still_9_and_carries_the_new_symbols_and_methods(twk):
    L = twk._lib
    assert L.lib.twk_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(L.lib, name) is not None, name
    for name in NEW_METHODS:
        method = getattr(twk.Device, name)
        assert callable(method) and "TwkError" in method.__doc__, f"{name}: the docstring states the refusals"
    assert isinstance(twk.Application.temporal, property)
    assert L.TWK_PLANE_COUNT == 6 and C.sizeof(L.AssemblySource) == 6 * C.sizeof(C.c_void_p), "the geometry is no seventh plane"


def test_null_handles_are_refused_before_any_device_call(twk):
    L = twk._lib
    p, n = C.c_void_p(), C.c_size_t(0)
    source = L.AssemblySource()
    pointers = (C.c_void_p * 1)(None)
    buffer = np.zeros(4, np.float32)
    tp = L.Temporal()
    calls = {
        "twk_render_geometry_tile": lambda: L.lib.twk_render_geometry_tile(None),
        "twk_assemble_with_geometry": lambda: L.lib.twk_assemble_with_geometry(None, C.c_uint(0), C.byref(source), pointers, 1),
        "twk_assemble_devices_with_geometry": lambda: L.lib.twk_assemble_devices_with_geometry(None, C.c_uint(0), pointers, 1),
        "twk_get_assembled_geometry_device_pointer": lambda: L.lib.twk_get_assembled_geometry_device_pointer(None, C.byref(p), C.byref(n)),
        "twk_read_assembled_geometry": lambda: L.lib.twk_read_assembled_geometry(None, buffer.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(buffer.size)),
        "twk_temporal_accumulate_assembled": lambda: L.lib.twk_temporal_accumulate_assembled(None, C.byref(tp)),
    }
    assert set(calls) | {"twk_app_get_temporal"} == set(NEW_SYMBOLS)
    for name, call in calls.items():
        assert call() == L.TWK_ERROR_INVALID_VALUE, name
        message = L.lib.twk_last_error().decode()
        assert message.startswith(name + ":") and "NULL" in message, message
    on, frames, step = C.c_int(5), C.c_int(5), C.c_float(5)
    assert L.lib.twk_app_get_temporal(None, C.byref(on), C.byref(tp), C.byref(frames), C.byref(step)) == L.TWK_ERROR_INVALID_VALUE
    assert "twk_app_get_temporal" in L.lib.twk_last_error().decode()


def _description(twk, text):
    """((enabled, maxHistory, positionTolerance, frames, orbitStep), the description written back)"""
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        on, tp, frames, step = app.temporal
        return (on, tp.maxHistory, tp.positionTolerance, frames, step), app.systemDescription()
    finally:
        app.close()


def test_description_keys_of_the_temporal_loop(twk):
    L = twk._lib
    f32 = lambda x: float(np.float32(x))
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    defaults = (False, L.TWK_TEMPORAL_MAX_HISTORY, f32(L.TWK_TEMPORAL_POSITION_TOLERANCE), 1, f32(0.001))
    off, off_text = _description(twk, base)
    assert off == defaults and "temporal" not in off_text, "off by default, nothing written back"
    assert _description(twk, off_text) == (defaults, off_text), "a description without the keys round-trips unchanged"
    assert _description(twk, base + "\ntemporalAccumulation 0\ntemporalFrames 1\n") == (defaults, off_text)

    keys = "\ntemporalAccumulation 1\ntemporalFrames 3\ntemporalOrbitStep 0.004\ntemporalMaxHistory 16\ntemporalPositionTolerance 0.1\n"
    on, on_text = _description(twk, base + keys)
    assert on == (True, 16, f32(0.1), 3, f32(0.004))
    for line in keys.strip().splitlines():
        assert line + "\n" in on_text, line
    assert _description(twk, on_text) == (on, on_text), "what is written back parses to the same"
    negative, _ = _description(twk, base + "\ntemporalOrbitStep -0.25\n")
    assert negative[4] == -0.25, "the orbit may turn the other way"
    edges, _ = _description(twk, base + "\ntemporalFrames 4096\ntemporalMaxHistory 1\ntemporalPositionTolerance 0\n")
    assert edges == (False, 1, 0.0, 4096, f32(0.001))

    # a value the calls would refuse drops the line: the previous value stays and nothing of it is written back
    for bad in ("temporalFrames 0", "temporalFrames -3", "temporalFrames 4097", "temporalMaxHistory 0", "temporalMaxHistory -1",
                "temporalPositionTolerance -0.5", "temporalAccumulation 2", "temporalAccumulation -1"):
        assert _description(twk, base + f"\n{bad}\n") == (defaults, off_text), bad
    kept, _ = _description(twk, base + "\ntemporalFrames 7\ntemporalFrames 5000\ntemporalMaxHistory 8\ntemporalMaxHistory 0\n")
    assert kept[3] == 7 and kept[1] == 8, "a refused value keeps the previous one"
