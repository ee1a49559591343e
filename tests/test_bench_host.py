"""bench.py's --dump-outputs on the CPU: the row sample is fixed by its arguments, the files hold float64 within the
64 MB limit, and the check of the racing tables stops the run on non-finite or all-zero rows."""
import os

import numpy as np
import pytest
import torch

import bench


def test_row_sample_is_fixed_sorted_and_distinct():
    a = bench.row_sample(10_000_000, 16384)
    assert np.array_equal(a, bench.row_sample(10_000_000, 16384))
    assert len(a) == 16384 and len(np.unique(a)) == 16384 and np.all(np.diff(a) > 0) and a[-1] < 10_000_000
    assert np.array_equal(bench.row_sample(100, 16384), np.arange(100))


def test_dump_outputs_dtype_values_and_limit(tmp_path):
    walks = torch.tensor([[3, 1, -1], [2, 2, 0]], dtype=torch.int32)
    lens = torch.tensor([2, 3], dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"walks": walks, "walk_lens": lens})
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("walks", "walk_lens")}
    assert got["walks"].dtype == np.float64 and np.array_equal(got["walks"], walks.numpy())
    assert got["walk_lens"].dtype == np.float64 and got["walk_lens"].tolist() == [2, 3]
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((bench.DUMP_BYTES // 8 + 1,), np.int32)})
    assert not os.path.exists(tmp_path / "big")


def test_check_trained_rejects_nan_and_untrained_rows():
    rows = torch.randn(16, 8)
    bench.check_trained("t", rows)
    bench.check_trained("t", torch.cat([torch.zeros(15, 8), rows[:1]]))    # rows of unseen words stay zero
    for bad in (torch.zeros(16, 8), torch.where(torch.arange(8) == 3, float("nan"), rows),
                torch.where(torch.arange(8) == 5, float("inf"), rows)):
        with pytest.raises(SystemExit):
            bench.check_trained("t", bad)
