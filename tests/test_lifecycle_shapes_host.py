"""The transitions of tests/lifecycle.py do what their rows claim, through the host-only twk_launch_width and twk_tile_column and a
numpy restatement of distribute (csrc/shade_device.h): equal or different launchWidth, equal element counts, the padding counts, and
tiled states that are mostly picture. Needs no GPU."""
import numpy as np
import pytest

import lifecycle as lc


def _restated_padding(shape, index, count, launch_width):
    """distribute() in numpy: the launch indices of a packed tile buffer whose column lies outside the picture."""
    y, x = np.mgrid[0:shape.height, 0:launch_width].astype(np.uint32)
    shift = [int(np.log2(t)) for t in shape.tile]
    tile = (x >> shift[0]) * np.uint32(count) + ((np.uint32(index) + (y >> shift[1])) % np.uint32(count))
    return tile * np.uint32(shape.tile[0]) + (x & np.uint32(shape.tile[0] - 1)) >= shape.width


def test_the_table_has_the_nine_rows():
    assert [t.id for t in lc.TRANSITIONS] == ["grow", "shrink", "reshape", "tiles-pad", "tiles-tile", "tiles-shrink", "retile", "format", "batch-history"]
    for t in lc.TRANSITIONS:
        assert len(t.padding) == len(t.handles) and set(t.formats) <= {lc.FLOAT4, lc.HALF4}
        for shape in (t.before, t.after):
            assert shape.width <= 128 and shape.height <= 64 and shape.width * shape.height <= 128 * 37  # no frame larger than 128x37


@pytest.mark.parametrize("t", lc.TRANSITIONS, ids=lambda t: t.id)
def test_shapes_do_what_the_row_claims(twk, t):
    for (index, count), (pad_before, pad_after) in zip(t.handles, t.padding):
        widths = [lc.launch_width(twk, s, count) for s in (t.before, t.after)]
        elements = [w * s.height for w, s in zip(widths, (t.before, t.after))]
        assert (widths[0] == widths[1]) == t.same_launch_width, widths
        assert (elements[0] == elements[1]) == t.same_elements, elements
        for shape, width, want in ((t.before, widths[0], pad_before), (t.after, widths[1], pad_after)):
            mask = lc.padding_mask(twk, shape, index, count)
            assert mask.shape == (shape.height, width) and int(mask.sum()) == want, (shape, index, int(mask.sum()), want)
            if lc.is_tiled(shape, count):
                assert np.array_equal(mask, _restated_padding(shape, index, count, width))
                assert width % shape.tile[0] == 0 and width * count >= shape.width
            else:
                assert not mask.any() and width == shape.width
        if lc.is_tiled(t.after, count):
            assert (elements[1] - pad_after) >= 0.9 * elements[1], "a tiled case must be mostly picture"


def test_the_written_counts(twk):
    """48 / 63 at 61x37 over two handles, none at 64x37 and 128x37, and with 8x16 tiles 24 picture elements per handle become padding."""
    by = lc.BY_ID
    assert by["tiles-pad"].padding == ((0, 48), (0, 63)) and by["tiles-shrink"].padding == ((0, 48), (0, 63)) and by["retile"].padding == ((0, 63),)
    assert lc.launch_width(twk, by["tiles-pad"].before, 2) == lc.launch_width(twk, by["tiles-pad"].after, 2) == 32
    assert lc.launch_width(twk, by["tiles-shrink"].before, 2) == 64 and lc.launch_width(twk, by["retile"].before, 2) == 61
    t = by["tiles-tile"]
    total = 0
    for (index, count), become in zip(t.handles, lc.TILES_TILE_BECOME_PADDING):
        before, after = (lc.padding_mask(twk, s, index, count) for s in (t.before, t.after))
        assert int((~before & after).sum()) == become == 24
        total += int((~after).sum())
    assert total == t.after.width * t.after.height  # the two tiles are the picture, once
    assert by["reshape"].before.width * by["reshape"].before.height == by["reshape"].after.width * by["reshape"].after.height


def test_states_carry_the_tile_size(twk):
    """The state a case sets has the row's tile size and distribution whatever the system description says."""
    from conftest import load_app
    t = lc.BY_ID["tiles-tile"]
    app = lc.make_app(twk, load_app, t.after)
    st = lc.state_of(app, t.after)
    assert list(st.resolution) == [61, 37] and list(st.tileSize) == [8, 16] and st.distribution == 1
