"""bench.py --dump-outputs (CPU): what the last timed step computed lands as <name>.npy in float32 / float64, at most 64 MB in all; an output larger
than its share is a fixed, seeded sample of its pixels, the same in every run, with the pixel numbers beside it."""
import os

import numpy as np

import bench


def _written(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    film = np.random.default_rng(1).random((64, 48, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path), {"film": film, "ray_counts": [7, 1 << 40, 3]})
    got = _written(tmp_path)
    assert sorted(got) == ["film.npy", "ray_counts.npy"]
    assert got["film.npy"].dtype == np.float32 and np.array_equal(got["film.npy"], film)
    assert got["ray_counts.npy"].dtype == np.float64 and got["ray_counts.npy"].tolist() == [7.0, float(1 << 40), 3.0]


def test_a_large_output_is_a_fixed_sample_within_the_budget(tmp_path):
    film = np.random.default_rng(2).random((4096, 4096, 4), dtype=np.float32)  # 256 MiB: a 4096^2 frame
    outs = {"film": film, "ray_counts": [1, 2, 3]}
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    a, b = _written(tmp_path / "a"), _written(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= bench.DUMP_BYTES
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    idx = a["film_index.npy"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < 4096 * 4096
    assert np.array_equal(a["film.npy"], film.reshape(-1, 4)[idx])
    assert all(np.array_equal(a[f], b[f]) for f in a)
