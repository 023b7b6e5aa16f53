"""bench.py --dump-outputs: which rows of the embedding table are written (no GPU needed)."""
import importlib
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path)


@pytest.fixture(scope="module")
def bench():
    saved = dict(os.environ)                 # importing bench.py sets HIP variables: keep them out of this process
    try:
        return importlib.import_module("bench")
    finally:
        os.environ.clear()
        os.environ.update(saved)


@pytest.mark.parametrize("dim", [1, 64, 90, 128])
def test_dump_sample_is_fixed_sorted_and_bounded(bench, dim):
    n = 1_639_358 + 54_571                                         # configs[1]'s table
    rows = bench.dump_rows(n, dim)
    assert np.array_equal(rows, bench.dump_rows(n, dim))           # the same rows on every run
    assert rows.dtype == np.int64 and rows[0] >= 0 and rows[-1] < n and (np.diff(rows) > 0).all()
    assert rows.size * (4 * dim + 8) <= 64 << 20                   # float32 table rows + float64 ids
    assert rows.size >= 50_000


def test_a_small_table_is_dumped_whole(bench):
    assert np.array_equal(bench.dump_rows(12_000, 64), np.arange(12_000))


def test_dump_writes_float32_rows_and_float64_ids(bench, tmp_path):
    import torch
    table = torch.arange(40, dtype=torch.float32).reshape(10, 4)
    rows = np.array([1, 4, 9], dtype=np.int64)
    bench.dump_outputs(str(tmp_path), table, rows)
    emb, ids = np.load(os.path.join(tmp_path, "embedding.npy")), np.load(os.path.join(tmp_path, "embedding_rows.npy"))
    assert emb.dtype == np.float32 and ids.dtype == np.float64
    assert np.array_equal(emb, table.numpy()[rows]) and np.array_equal(ids, rows)
