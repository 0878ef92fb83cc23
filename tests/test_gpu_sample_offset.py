"""-m gpu: twk_set_sample_offset — iteration i draws its random numbers as iteration i + offset, and whatever counts samples (the
running mean's weight, "iteration 0 starts afresh", the moments' n) does not see the offset. The raw samples are read through the
debug tap twk_debug_read_path_radiance, which tests/test_gpu_moments.py pins to the oracle."""
import numpy as np
import pytest

from conftest import load_app
from test_moments_host import fold_mean, welford

pytestmark = pytest.mark.gpu

RES = (61, 37)
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _render(dev, first, count):
    """Iterations first .. first + count - 1 as one pass: (the tap's samples, picture, moments)."""
    for it in range(first, first + count):
        dev.render(it)
    return dev.debugReadPathRadiance(count), dev.getOutputBufferHost(), dev.readMoments()


def test_an_offset_shifts_the_random_numbers_and_nothing_else(twk):
    app = load_app(twk, "system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", RES)
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    dev.enableMoments(True)
    first_tap, first_picture, first_moments = _render(dev, 0, 4)
    later_tap, _, later_moments = _render(dev, 4, 4)  # iterations 4 .. 7 without an offset
    assert (first_moments[..., 2] == 4).all() and (later_moments[..., 2] == 8).all()
    assert not np.array_equal(_bits(first_tap), _bits(later_tap))
    dev.setSampleOffset(4)
    shifted_tap, shifted_picture, shifted_moments = _render(dev, 0, 4)
    assert np.array_equal(_bits(shifted_tap), _bits(later_tap)), "iterations 0 .. 3 with offset 4 are not the samples of iterations 4 .. 7"
    # what counts samples is unchanged: iteration 0 started afresh, the mean weighs 1 / (i + 1), n is 4
    assert (shifted_moments[..., 2] == 4).all()
    assert np.array_equal(_bits(shifted_picture), _bits(fold_mean(shifted_tap, 0, np.zeros(shifted_tap.shape[1:], F)))), "the running mean under an offset is not the mean of its four samples"
    assert np.array_equal(_bits(shifted_moments), _bits(welford(shifted_tap, 0, np.zeros(shifted_tap.shape[1:], F))))
    # one pass per iteration gives the same samples as the batch
    dev.setLaunchBatch(1)
    singles = []
    for it in range(4):
        dev.render(it)
        singles.append(dev.debugReadPathRadiance(1)[0])
    assert np.array_equal(_bits(np.stack(singles)), _bits(later_tap))
    dev.setLaunchBatch(64)
    dev.setSampleOffset(0)
    again_tap, again_picture, again_moments = _render(dev, 0, 4)
    assert np.array_equal(_bits(again_tap), _bits(first_tap)) and np.array_equal(_bits(again_picture), _bits(first_picture)), "offset 0 after an offset does not reproduce the first render"
    assert np.array_equal(_bits(again_moments), _bits(first_moments)) and (again_moments[..., 2] == 4).all()
    dev.close()
