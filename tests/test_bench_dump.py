"""CPU: bench.py --dump-outputs writes the image whole while it fits the 64 MB limit, else a seeded sample of its pixels
with their indices; the sample is the same from run to run."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("twk_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_image_within_the_limit_is_written_whole(tmp_path):
    bench = _bench()
    img = np.arange(6 * 5 * 4, dtype=np.float32).reshape(6, 5, 4)
    bench.dump_image(str(tmp_path / "out"), img)
    assert sorted(os.listdir(tmp_path / "out")) == ["image.npy"]
    got = np.load(tmp_path / "out" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)


def test_image_beyond_the_limit_is_a_fixed_sample(tmp_path):
    bench = _bench()
    # the C5 frame, 3840 x 2160 x 4 float32 = 133 MB: pixel p holds (p, p + 0.25, p + 0.5, p + 0.75)
    pix = np.arange(3840 * 2160, dtype=np.float64)
    img = (pix[:, None] + np.array([0.0, 0.25, 0.5, 0.75])).astype(np.float32).reshape(2160, 3840, 4)
    for run in ("a", "b"):
        bench.dump_image(str(tmp_path / run), img)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["image.npy", "image_pixel_index.npy"]
    sample, index = np.load(a / "image.npy"), np.load(a / "image_pixel_index.npy")
    assert sample.dtype == np.float32 and index.dtype == np.float64
    assert sample.nbytes + index.nbytes <= bench.DUMP_LIMIT_BYTES
    assert sample.shape == (1 << 21, 4) and index.shape == (1 << 21,)
    assert np.all(np.diff(index) > 0) and index[0] >= 0 and index[-1] < 3840 * 2160
    assert np.array_equal(sample, img.reshape(-1, 4)[index.astype(np.int64)])
    assert np.array_equal(np.load(b / "image.npy"), sample) and np.array_equal(np.load(b / "image_pixel_index.npy"), index)
