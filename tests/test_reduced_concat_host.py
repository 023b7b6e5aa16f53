"""The builder of the concatenated operator [R_H^T | G_L] on the host (lgc_reduce_concat_host: the code the kernels of
lgc_reduce_concat call, element by element) against a numpy restatement (tests/reduced_concat_support.py).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from reduced_concat_support import GRAPHS, N_GAPS, concat_numpy, reduced_csr_host
from gnn_ecommerce_amd import _native
from gnn_ecommerce_amd.graph import build_concat_csr


@pytest.mark.parametrize("n_gaps", (N_GAPS, 1, 3))
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_host_builder_against_numpy(name, n_gaps):
    csr = reduced_csr_host(name)
    if name == "all_eliminated":
        assert csr.n_h == 0 and csr.nnz == 0 and csr.gram_nnz > 0
    if name == "none_eliminated":
        assert csr.gram_nnz == 0
    got = build_concat_csr(csr, n_gaps, host=True)
    pos, gap_start, rowptr, entries = concat_numpy(csr.rowptr.numpy(), csr.entries.numpy(), csr.gram_rowptr.numpy(),
                                                   csr.gram_entries.numpy(), csr.n_h, csr.n_items, n_gaps)
    gap_rows = -(-csr.n_items // n_gaps)
    assert got.gap_rows == gap_rows and got.n_phys == csr.n_h + n_gaps * gap_rows
    assert np.array_equal(got.user_pos.numpy(), pos)
    assert np.array_equal(got.gap_start.numpy(), gap_start)
    assert np.array_equal(got.rowptr.numpy(), rowptr)
    assert np.array_equal(got.entries.numpy(), entries)
    # what the layout promises, stated without the restatement
    rp, ent = got.rowptr.numpy().astype(np.int64), got.entries.numpy()
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    user_part = rows < got.n_phys
    assert (ent[user_part, 0] >= got.n_phys).all() and (ent[user_part, 0] < got.n_phys + csr.n_items).all()
    assert (ent[~user_part, 0] >= 0).all() and (ent[~user_part, 0] < got.n_phys).all()
    item_pos = gap_start[np.arange(csr.n_items) // gap_rows] + np.arange(csr.n_items) % gap_rows
    assert np.unique(np.concatenate([pos, item_pos])).size == csr.n_h + csr.n_items, "a row owned twice"
    assert (np.diff(pos) > 0).all() and (np.diff(item_pos) > 0).all(), "both numberings keep their order"
    for j in (0, csr.n_items - 1):                                     # a gap row gathers its own item with weight one
        e = ent[rp[item_pos[j]]:rp[item_pos[j] + 1]]
        assert e.shape[0] == 1 and e[0, 0] == got.n_phys + j and e[0, 1:].view(np.float32)[0] == 1.0
    if name == "fewer_items_than_gaps" and n_gaps == N_GAPS:
        assert gap_rows == 1 and got.n_phys == csr.n_h + 8
        unused = np.setdiff1d(np.arange(got.n_phys), np.concatenate([pos, item_pos]))
        assert unused.size == 2 and (np.diff(rp)[unused] == 0).all(), "the rows of an empty gap hold nothing"


def test_bands_split_the_kept_entries_evenly():
    """Gap b sits where band b's share of the kept user rows' entries ends: the sweep planner's band rule."""
    csr = reduced_csr_host("odd_items")
    got = build_concat_csr(csr, N_GAPS, host=True)
    rp = csr.rowptr.numpy().astype(np.int64)
    ne, longest = rp[csr.n_h], int(np.diff(rp[:csr.n_h + 1]).max())
    users_upto = got.gap_start.numpy() - got.gap_rows * np.arange(N_GAPS)
    assert users_upto[-1] == csr.n_h
    for b in range(N_GAPS - 1):
        assert abs(rp[users_upto[b]] - ne * (b + 1) / N_GAPS) <= longest


def test_argument_errors():
    lib = _native.load()
    one = ctypes.c_void_p(256)                       # non-null, never dereferenced: every check precedes the first read
    base = dict(rowptr=one, entries=one, n_entries=20, gram_rowptr=one, gram_entries=one, n_gram=7, n_kept=4, n_items=6,
                n_gaps=8, user_pos=one, gap_start=one, rowptr_out=one, entries_out=one, n_out=33)
    order = tuple(base)
    for fn, tail in ((lib.lgc_reduce_concat, (None,)), (lib.lgc_reduce_concat_host, ())):
        call = lambda **kw: fn(*[{**base, **kw}[k] for k in order], *tail)
        assert call(rowptr=None) == -1 and call(gram_rowptr=None) == -1 and call(entries=None) == -1
        assert call(gram_entries=None) == -1 and call(user_pos=None) == -1 and call(gap_start=None) == -1
        assert call(rowptr_out=None) == -1 and call(entries_out=None) == -1
        assert call(n_out=32) == -1 and call(n_items=0) == -1 and call(n_gaps=0) == -1 and call(n_kept=-1) == -1
        assert call(n_gaps=65) == -4 and call(n_kept=2 ** 31) == -4 and call(n_entries=2 ** 31, n_out=2 ** 31 + 13) == -4
    assert lib.lgc_reduce_concat_rows(4, 6, 8) == 12 and lib.lgc_reduce_concat_rows(0, 30, 8) == 32
    assert lib.lgc_reduce_concat_rows(4, 0, 8) == -1 and lib.lgc_reduce_concat_rows(4, 6, 65) == -1


def test_switch_values():
    from gnn_ecommerce_amd import graph as G
    assert G.REDUCED_CONCAT == "auto", "the suite runs with the default switch"
