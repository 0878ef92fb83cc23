"""CPU: assembling a tiled frame (csrc/assemble_device.h) — twk_assemble_host against the numpy restatement of the map
(tests/assemble_restate.py) byte for byte, the properties of the map, the "tileAssembly" key of the system description, and the
refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import assemble_restate as R
from conftest import scene_path

SHAPES = [(61, 37), (96, 64), (7, 3), (200, 19)]
TILES = [(8, 8), (2, 4), (16, 4), (1, 1)]
DEVICES = [1, 2, 3, 5]
LAYERS = [1, 2, 8]
ELEMENTS = [4, 8, 16]


def host_assemble(twk, sources, width, height, tile, element_bytes, layers, into):
    from tweeker_raytracer_amd import _lib as L
    sources = [np.ascontiguousarray(s) for s in sources]
    pointers = (C.c_void_p * len(sources))(*[s.ctypes.data for s in sources])
    tile_c = (C.c_int * 2)(*tile)
    L.check(L.lib.twk_assemble_host(pointers, len(sources), int(width), int(height), tile_c, int(element_bytes), int(layers), into.ctypes.data_as(C.c_void_p)))
    return into


@pytest.mark.parametrize("width,height", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_host_form_equals_the_restatement(twk, width, height):
    for tile in TILES:
        for n in DEVICES:
            for element_bytes in ELEMENTS:
                for layers in LAYERS:
                    dtype, tail = R.element_dtype(element_bytes)
                    sources = R.iota_sources(width, height, tile, n, element_bytes, layers)
                    sentinel = np.full((layers, height, width) + tail, 0xA5A5 if element_bytes == 8 else 0xA5A5A5A5, dtype)
                    want = R.assemble(sources, width, height, tile, into=sentinel.copy())
                    got = host_assemble(twk, sources, width, height, tile, element_bytes, layers, sentinel.copy())
                    assert got.tobytes() == want.tobytes(), (tile, n, element_bytes, layers)


def test_the_restated_map_is_twk_tile_column_and_twk_launch_width(twk):
    from tweeker_raytracer_amd import _lib as L
    for (width, height), tile, n in [((61, 37), (8, 8), 3), ((7, 3), (2, 4), 5), ((200, 19), (16, 4), 2), ((96, 64), (1, 1), 5)]:
        lw = C.c_int(0)
        L.check(L.lib.twk_launch_width(width, tile[0], n, C.byref(lw)))
        assert lw.value == R.launch_width(width, tile[0], n)
        tile_c = (C.c_int * 2)(*tile)
        for d in range(n):
            cols = R.picture_columns(width, height, tile, n, d)
            for y in range(0, height, 3):
                for x in range(lw.value):
                    px = C.c_int(-1)
                    L.check(L.lib.twk_tile_column(x, y, tile_c, n, d, C.byref(px)))
                    assert px.value == cols[y, x]


@pytest.mark.parametrize("n", DEVICES)
def test_every_picture_element_is_written_once_and_padding_never_arrives(twk, n):
    """Sources hold one value inside the picture and a sentinel in the padding; the destination starts as another sentinel. Afterwards
    no sentinel of either kind is left anywhere, and the count of arrivals per element (assemble_restate.assemble asserts it) is 1."""
    for (width, height), tile in zip(SHAPES, TILES):
        lw = R.launch_width(width, tile[0], n)
        sources = []
        for d in range(n):
            cols = R.picture_columns(width, height, tile, n, d)
            src = np.where(cols < width, np.uint32(d + 1), np.uint32(0xDEADBEEF)).astype(np.uint32).reshape(1, height, lw)
            sources.append(src)
        got = host_assemble(twk, sources, width, height, tile, 4, 1, np.full((1, height, width), 0x0BADF00D, np.uint32))
        assert not (got == 0xDEADBEEF).any(), "source padding reached the picture"
        assert not (got == 0x0BADF00D).any(), "a picture element was not written"
        # each element came from the device the checkerboard gives it
        ys, xs = np.mgrid[0:height, 0:width]
        owner = ((xs // tile[0]) - (ys // tile[1])) % n
        assert np.array_equal(got[0], owner.astype(np.uint32) + 1)
        R.assemble(sources, width, height, tile)  # asserts "exactly once"


def test_a_wrong_device_order_gives_a_different_picture(twk):
    width, height, tile, n = 61, 37, (8, 8), 3
    sources = R.iota_sources(width, height, tile, n, 16, 1)
    right = host_assemble(twk, sources, width, height, tile, 16, 1, np.zeros((1, height, width, 4), np.uint32))
    wrong = host_assemble(twk, [sources[1], sources[0], sources[2]], width, height, tile, 16, 1, np.zeros((1, height, width, 4), np.uint32))
    assert not np.array_equal(right, wrong)
    assert np.array_equal(right, R.assemble(sources, width, height, tile))


def test_host_form_refusals(twk):
    from tweeker_raytracer_amd import _lib as L
    src = np.zeros((1, 4, 8), np.uint32)
    dst = np.zeros((1, 4, 8), np.uint32)
    pointers = (C.c_void_p * 1)(src.ctypes.data)
    tile = (C.c_int * 2)(8, 8)
    good = dict(sources=pointers, n=1, w=8, h=4, tile=tile, eb=4, layers=1, dst=dst.ctypes.data_as(C.c_void_p))
    call = lambda a: L.lib.twk_assemble_host(a["sources"], a["n"], a["w"], a["h"], a["tile"], a["eb"], a["layers"], a["dst"])
    assert call(good) == L.TWK_SUCCESS
    for change in (dict(sources=None), dict(dst=None), dict(tile=None), dict(n=0), dict(w=0), dict(h=0), dict(layers=0), dict(eb=12), dict(eb=2),
                   dict(tile=(C.c_int * 2)(6, 8)), dict(tile=(C.c_int * 2)(8, 0)), dict(sources=(C.c_void_p * 1)(None))):
        assert call({**good, **change}) == L.TWK_ERROR_INVALID_VALUE, change
        assert "twk_assemble_host" in L.lib.twk_last_error().decode()


def _description(twk, text):
    app = twk.Application(system_text=text, scene_text=open(scene_path("scene_rtigo3_cornell_box.txt")).read())
    try:
        return app.tileAssembly, app.systemDescription()
    finally:
        app.close()


def test_description_key_tile_assembly(twk):
    base = open(scene_path("system_rtigo3_cornell_box.txt")).read()
    off, off_text = _description(twk, base)
    assert off is False and "tileAssembly" not in off_text, "defaults to off and is not written back"
    assert _description(twk, base + "\ntileAssembly 0\n") == (False, off_text)
    on, on_text = _description(twk, base + "\ntileAssembly 1\n")
    assert on is True and "tileAssembly 1\n" in on_text
    assert _description(twk, on_text) == (True, on_text), "what is written back parses to the same"
    # a value that is not exactly 0 or 1 is not taken for either: the key stays off (the parser records a warning) and nothing is written back
    for bad in ("2", "-1", "0.5", "1.0", "1e0", "01"):
        assert _description(twk, base + f"\ntileAssembly {bad}\n") == (False, off_text), bad
    assert _description(twk, base + "\ntileAssembly 1\ntileAssembly 7\n") == (False, off_text), "a refused value leaves it off, not as it was"


def test_null_handles_are_refused_before_any_device_call(twk):
    from tweeker_raytracer_amd import _lib as L
    p, n = C.c_void_p(), C.c_size_t(0)
    source = L.AssemblySource()
    handles = (C.c_void_p * 1)(None)
    buffer = np.zeros(4, np.uint32)
    calls = {
        "twk_assemble": lambda: L.lib.twk_assemble(None, C.c_uint(1), C.byref(source), 1),
        "twk_assemble_devices": lambda: L.lib.twk_assemble_devices(None, C.c_uint(1), handles, 1),
        "twk_get_assembled_device_pointer": lambda: L.lib.twk_get_assembled_device_pointer(None, 0, C.byref(p), C.byref(n)),
        "twk_read_assembled": lambda: L.lib.twk_read_assembled(None, 0, buffer.ctypes.data_as(C.c_void_p), C.c_size_t(buffer.nbytes)),
    }
    for name, call in calls.items():
        assert call() == L.TWK_ERROR_INVALID_VALUE, name
        message = L.lib.twk_last_error().decode()
        assert name in message and "NULL" in message, message
    on = C.c_int(5)
    assert L.lib.twk_app_get_tile_assembly(None, C.byref(on)) == L.TWK_ERROR_INVALID_VALUE and "twk_app_get_tile_assembly" in L.lib.twk_last_error().decode()


def test_the_abi_is_still_9_and_carries_the_new_symbols(twk):
    from tweeker_raytracer_amd import _lib as L
    assert L.lib.twk_abi_version() == 9
    for name in ("twk_assemble", "twk_assemble_devices", "twk_get_assembled_device_pointer", "twk_read_assembled", "twk_assemble_host", "twk_app_get_tile_assembly"):
        assert name in L.SYMBOLS and getattr(L.lib, name) is not None
    assert (L.TWK_PLANE_OUTPUT, L.TWK_PLANE_ALBEDO, L.TWK_PLANE_NORMAL, L.TWK_PLANE_MOMENTS, L.TWK_PLANE_SAMPLE_COUNTS, L.TWK_PLANE_CASCADE, L.TWK_PLANE_COUNT) == (0, 1, 2, 3, 4, 5, 6)
    assert C.sizeof(L.AssemblySource) == 6 * C.sizeof(C.c_void_p)
