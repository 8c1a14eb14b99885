"""bench.py --dump-outputs on host tensors (no GPU): a table inside the budget is written whole, a
larger one as the same sorted row sample every time, and every run's files stay under 64 MB."""
import os
import types

import numpy as np
import torch

import bench


def _agg(rows, cols=bench.F):
    y = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)
    return types.SimpleNamespace(y_own=y, y_full=None)


def test_small_table_is_written_whole(tmp_path):
    agg = _agg(1000)
    name, shape = bench.dump_outputs(str(tmp_path / "d"), agg, "single", 1, 0)
    got = np.load(tmp_path / "d" / name)
    assert name == "y.npy" and shape == (1000, bench.F) and got.dtype == np.float32
    assert np.array_equal(got, agg.y_own.numpy())


def test_large_table_is_a_fixed_row_sample_within_the_budget(tmp_path):
    rows = bench.DUMP_BYTES // (bench.F * 4) + 5000   # just over the budget, as the Reddit table is
    agg = _agg(rows)
    bench.dump_outputs(str(tmp_path / "a"), agg, "single", 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), agg, "single", 1, 0)
    a = np.load(tmp_path / "a" / "y.npy", mmap_mode="r")
    b = np.load(tmp_path / "b" / "y.npy", mmap_mode="r")
    assert os.path.getsize(tmp_path / "a" / "y.npy") <= bench.DUMP_BYTES <= 64 * 10**6
    assert a.dtype == np.float32 and a.shape == b.shape and a.shape[1] == bench.F
    assert np.array_equal(a, b)
    # whole rows of the table, in ascending row order (column 0 holds row * F)
    ids = (np.asarray(a[:, 0]).astype(np.int64)) // bench.F
    assert np.all(np.diff(ids) > 0) and ids[-1] < rows
    assert np.array_equal(np.asarray(a[:64]), agg.y_own.numpy()[ids[:64]])


def test_ranks_share_the_budget_and_name_their_files(tmp_path):
    rows = bench.DUMP_BYTES // (bench.F * 4)
    agg = _agg(rows)
    names = [bench.dump_outputs(str(tmp_path), agg, "edges", 2, r)[0] for r in range(2)]
    assert names == ["y_rank0.npy", "y_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / n) for n in names) <= bench.DUMP_BYTES
