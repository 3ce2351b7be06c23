"""bench.py --dump-outputs without a GPU: the files it writes for a framebuffer as the timed path returns it, and the seeded
row sample that keeps a larger framebuffer (many ranks) under the 64 MB cap."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_the_image_and_counters(tmp_path):
    bench = _bench()
    img = torch.rand((768, 1024, 3), dtype=torch.float32)
    st = {"samples": 805306368, "bounces": 6990000001, "max_depth_kills": 3, "kernel_ms": 79.5}
    bench.dump_outputs(str(tmp_path), img, st)
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "stats.npy"]
    a = np.load(tmp_path / "image.npy")
    assert a.dtype == np.float32 and np.array_equal(a, img.numpy())
    s = np.load(tmp_path / "stats.npy")
    assert s.dtype == np.float64 and s.tolist() == [805306368, 6990000001, 3]


def test_dump_of_a_large_framebuffer_is_a_fixed_row_sample_under_the_cap(tmp_path):
    bench = _bench()
    img = torch.arange(8 * 768, dtype=torch.float32)[:, None, None].expand(8 * 768, 1024, 3).contiguous()    # row index in every pixel
    st = {"samples": 1, "bounces": 2, "max_depth_kills": 0}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img, st)
        assert sorted(os.listdir(tmp_path / d)) == ["image.npy", "image_rows.npy", "stats.npy"]
        assert _dir_bytes(tmp_path / d) <= bench.DUMP_CAP_BYTES
    rows = np.load(tmp_path / "a" / "image_rows.npy")
    a = np.load(tmp_path / "a" / "image.npy")
    assert rows.dtype == np.float64 and a.dtype == np.float32
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 8 * 768 and len(rows) > 5 * 768
    assert np.array_equal(a[:, 0, 0], rows.astype(np.float32))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "image_rows.npy"))
    assert np.array_equal(a, np.load(tmp_path / "b" / "image.npy"))
