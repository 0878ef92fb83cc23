"""The map of a tiled frame (csrc/assemble_device.h) restated in numpy, written from the description of the checkerboard and not from
twk_tile_column: divisions and remainders over whole index grids, no shifts, no per-element calls. The tests compare
twk_assemble_host, the kernel and twk_tile_column against it.

A picture of `width` columns is cut into tiles of tile[0] x tile[1] pixels. Tile column t of tile row r belongs to device
(t - r) mod n, so that device d owns, in tile row r, the tile columns t = k n + (d + r) mod n for k = 0, 1, ...; it stores its k-th
tile of every row at launch columns k tile[0] .. k tile[0] + tile[0] - 1 of a packed buffer launch_width(...) columns wide."""
import numpy as np


def launch_width(width, tile_x, n):
    """Columns of one device's packed buffer: the whole width on one device, else its share rounded up to whole tiles."""
    if n == 1:
        return width
    share = -(-width // n)
    return -(-share // tile_x) * tile_x


def picture_columns(width, height, tile, n, d):
    """int64 [height, launch_width]: the picture column of every launch index of device d; a value >= width is padding."""
    lw = launch_width(width, tile[0], n)
    x_launch = np.arange(lw, dtype=np.int64)[None, :]
    y = np.arange(height, dtype=np.int64)[:, None]
    k = x_launch // tile[0]            # the device's k-th tile of the row
    row = y // tile[1]                 # the tile row
    t = k * n + (d + row) % n          # the tile column it is in the picture
    return t * tile[0] + x_launch % tile[0]


def assemble(sources, width, height, tile, into=None):
    """sources[d]: [layers, height, launch_width, ...] of device d. Returns [layers, height, width, ...] (`into`, where given, with
    only the in-picture elements replaced) and asserts that every picture element is written exactly once."""
    n = len(sources)
    first = np.asarray(sources[0])
    out = into if into is not None else np.zeros(first.shape[:1] + (height, width) + first.shape[3:], first.dtype)
    written = np.zeros((height, width), np.int64)
    for d, src in enumerate(sources):
        src = np.asarray(src)
        cols = picture_columns(width, height, tile, n, d)
        assert src.shape[1:3] == cols.shape, (src.shape, cols.shape)
        yy, xl = np.nonzero(cols < width)
        out[:, yy, cols[yy, xl]] = src[:, yy, xl]
        np.add.at(written, (yy, cols[yy, xl]), 1)
    assert (written == 1).all(), "the map must write every picture element exactly once"
    return out


def element_dtype(element_bytes):
    """An array dtype whose last axis makes one element of 4, 8 or 16 bytes: (dtype, trailing shape)."""
    return {4: (np.uint32, ()), 8: (np.uint16, (4,)), 16: (np.uint32, (4,))}[element_bytes]


def iota_sources(width, height, tile, n, element_bytes, layers, salt=0):
    """Packed buffers whose words change with device, layer and position, padding included."""
    dtype, tail = element_dtype(element_bytes)
    lw = launch_width(width, tile[0], n)
    per = layers * height * lw * int(np.prod(tail, dtype=np.int64))
    out = []
    for d in range(n):
        values = np.arange(per, dtype=np.int64) * 7 + d * 1000003 + salt
        out.append(values.astype(dtype).reshape((layers, height, lw) + tail))
    return out
