"""Middle-hop reduction: the native builder (lgc_reduce_*: reduced CSR in compact numbering + G_L = R_L^T R_L) and the
forward that uses it (``bipartite_sum(reduced=...)``), against fp64 references on the host (tests/eliminate_support.py).
T is forced through ``PropGraph.eliminate_max_deg``, never through the environment."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, rel_fro, worst_row_rel
from eliminate_support import (GRAPHS, UNNORMALISED, alphas_for, csr_host, dense_fp64, eliminated_users, layer_sum_fp64, ulp32)
from reduce_support import reduce_reference_fast
from gnn_ecommerce_amd import _native, graph as G, propagate, synth
from gnn_ecommerce_amd.graph import PropGraph, build_reduced_csr

TOL = 1e-5          # the project's gate on rel_fro against fp64
DIMS = (20, 64, 90)
LAYERS = (1, 2, 3, 5)

_graphs = {}


def built(name, device):
    """(PropGraph, split, n, T) of a named graph, built once per session; tests set ``eliminate_max_deg`` themselves."""
    if name not in _graphs:
        ei, ew, split, n, t = GRAPHS[name]()
        pg = PropGraph(ei.to(device), ew.to(device), n, normalize=name not in UNNORMALISED)
        assert pg.split == split
        _graphs[name] = (pg, split, n, t)
    return _graphs[name]


def forward(pg, x, alphas, max_deg, final_rows=None):
    pg.eliminate_max_deg = max_deg
    try:
        return propagate._layer_sum(pg, x, alphas, transpose=False, final_rows=final_rows)
    finally:
        pg.eliminate_max_deg = None


# ----------------------------------------------------------------------------------------
# builder
# ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_reduced_csr_and_gram_operator(device, name):
    pg, split, n, t = built(name, device)
    op = pg.forward_op
    red = build_reduced_csr(op.rowptr, op.entries, split, n, t)
    again = build_reduced_csr(op.rowptr, op.entries, split, n, t)
    for f in ("user_map", "rowptr", "entries", "gram_rowptr", "gram_entries"):
        assert torch.equal(getattr(red, f), getattr(again, f)), f"two builds differ in {f}"
    n_items = n - split
    gone = eliminated_users(op, split, t)
    n_h = int((~gone).sum())
    assert red.n_h == n_h and red.n_items == n_items
    if name == "all_eliminated":
        assert n_h == 0 and red.nnz == 0
    if name == "none_eliminated":
        assert n_h == split and red.gram_nnz == 0 and red.n_pairs == 0
    # the map: kept users in their relative order, -1 for the others
    want_map = torch.where(gone, torch.full((split,), -1), torch.cumsum((~gone).long(), 0) - 1)
    assert torch.equal(red.user_map.cpu().long(), want_map)

    # reduced CSR: the surviving entries of the full CSR in order, values bit for bit, columns renumbered
    rowptr, cols, _, rows = csr_host(op)
    bits = op.entries[:, 1].cpu()
    keep_row = torch.cat([~gone, torch.ones(n_items, dtype=torch.bool)])
    keep_col = torch.cat([~gone, torch.ones(n_items, dtype=torch.bool)])
    survive = keep_row[rows] & keep_col[cols]
    new_id = torch.cat([want_map, n_h + torch.arange(n_items)])
    assert red.nnz == int(survive.sum())
    assert torch.equal(red.entries[:, 1].cpu(), bits[survive])
    assert torch.equal(red.entries[:, 0].cpu().long(), new_id[cols[survive]])
    counts = torch.bincount(new_id[rows[survive]], minlength=n_h + n_items)
    assert torch.equal(red.rowptr.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)]))
    assert red.user_nnz == int(red.rowptr[n_h])
    if red.nnz:
        assert int(red.entries[:, 0].min()) >= 0 and int(red.entries[:, 0].max()) < n_h + n_items
    assert pg.eliminate_max_deg is None

    # G_L against the dense fp64 product over the eliminated users
    a = dense_fp64(op, n)
    r_iu, r_uj = a[split:, :split][:, gone], a[:split, split:][gone, :]
    want = r_iu @ r_uj
    # structure: a pair (i, j) is stored iff some eliminated user joins them
    _, cols_f, vals_f, rows_f = csr_host(op)
    pat = torch.zeros((n, n), dtype=torch.float64)
    pat.index_put_((rows_f, cols_f), torch.ones_like(vals_f), accumulate=True)
    want_pat = (pat[split:, :split][:, gone] @ pat[:split, split:][gone, :]) > 0
    g_rowptr = red.gram_rowptr.cpu().long()
    g_cols = red.gram_entries[:, 0].cpu().long()
    g_vals = red.gram_entries[:, 1].cpu().contiguous().view(torch.float32)
    assert g_rowptr.numel() == n_h + n_items + 1 and int(g_rowptr[n_h]) == 0 and int(g_rowptr[-1]) == red.gram_nnz
    g_rows = torch.repeat_interleave(torch.arange(n_h + n_items), g_rowptr[1:] - g_rowptr[:-1])
    if red.gram_nnz:
        assert int(g_cols.min()) >= n_h and int(g_cols.max()) < n_h + n_items and int(g_rows.min()) >= n_h
        same_row = g_rows[1:] == g_rows[:-1]
        assert (g_cols[1:][same_row] > g_cols[:-1][same_row]).all(), "columns must ascend within a row"
    got_pat = torch.zeros((n_items, n_items), dtype=torch.bool)
    got_pat[g_rows - n_h, g_cols - n_h] = True
    assert torch.equal(got_pat, want_pat)
    got = torch.zeros((n_items, n_items), dtype=torch.float64)
    got[g_rows - n_h, g_cols - n_h] = g_vals.double()
    # fp64 accumulation error is far below an fp32 ulp; rounding the fp64 sum once more costs at most one
    err = (got - want).abs()
    assert (err <= ulp32(want)).all(), float((err / ulp32(want).clamp_min(1e-300)).max())
    if name == "hub":
        assert int(g_rowptr[n_h + 1] - g_rowptr[n_h]) > 256, "the hub's row must take several chunks"
    if name == "nothing_left":
        assert n_h == 0 and red.nnz == 0 and red.gram_nnz == 0 and op.nnz > 0
    if name == "kept_but_unnamed":
        assert n_h > 0 and red.nnz == red.user_nnz > 0 and red.gram_nnz > 0

    # every output bit for bit against the exact host reference: G_L's values are the fp64 sums in expansion order
    ref = reduce_reference_fast(op.rowptr.cpu().numpy(), op.entries[:, 0].cpu().numpy(), op.entries[:, 1].cpu().numpy(),
                                split, n, t)
    assert ref.pairs_min == ref.pairs_max == red.n_pairs and (ref.n_kept, ref.user_nnz) == (red.n_h, red.user_nnz)
    for f, want_f in (("user_map", ref.user_map), ("rowptr", ref.rowptr), ("entries", ref.entries),
                      ("gram_rowptr", ref.gram_rowptr), ("gram_entries", ref.gram_entries)):
        assert torch.equal(getattr(red, f).cpu(), torch.from_numpy(want_f)), f"{f} differs from the host reference"


def test_builder_argument_errors_come_before_any_launch():
    """Every check precedes the first runtime call, so the codes come back on a box without a device too."""
    lib = _native.load()
    one = ctypes.c_void_p(256)                       # non-null, 256-byte aligned, never dereferenced
    odd = ctypes.c_void_p(260)
    count = lambda **kw: lib.lgc_reduce_count(*[{**dict(rowptr=one, entries=one, n_nodes=10, n_edges=20, split=4, max_deg=3,
                                                        ws=one, ws_bytes=1 << 30, user_map=one, totals=one, stream=None),
                                                 **kw}[k] for k in ("rowptr", "entries", "n_nodes", "n_edges", "split", "max_deg",
                                                                    "ws", "ws_bytes", "user_map", "totals", "stream")])
    assert count(rowptr=None) == -1 and count(entries=None) == -1 and count(user_map=None) == -1 and count(totals=None) == -1
    assert count(split=0) == -1 and count(split=10) == -1 and count(max_deg=-1) == -1 and count(n_edges=-1) == -1
    assert count(n_nodes=2 ** 31) == -4 and count(n_edges=2 ** 31) == -4
    assert count(ws=None) == -1 and count(ws_bytes=16) == -3 and count(ws=odd) == -5
    assert lib.lgc_reduce_workspace_bytes(-1, 0) == 0 and lib.lgc_reduce_workspace_bytes(10, 2 ** 31) == 0
    assert lib.lgc_reduce_workspace_bytes(10, 20) > 0
    fill = lambda **kw: lib.lgc_reduce_fill(*[{**dict(rowptr=one, entries=one, n_nodes=10, n_edges=20, split=4, ws=one,
                                                      user_map=one, n_kept=2, n_out=5, rowptr_out=one, entries_out=one,
                                                      stream=None), **kw}[k]
                                              for k in ("rowptr", "entries", "n_nodes", "n_edges", "split", "ws", "user_map",
                                                        "n_kept", "n_out", "rowptr_out", "entries_out", "stream")])
    assert fill(ws=None) == -1 and fill(user_map=None) == -1 and fill(rowptr_out=None) == -1 and fill(entries_out=None) == -1
    assert fill(n_kept=5) == -1 and fill(n_out=21) == -1 and fill(n_kept=-1) == -1 and fill(ws=odd) == -5
    gcount = lambda **kw: lib.lgc_reduce_gram_count(*[{**dict(rowptr=one, entries=one, n_nodes=10, n_edges=20, split=4, ws=one,
                                                              n_pairs=7, gws=one, gws_bytes=1 << 30, total=one, stream=None),
                                                       **kw}[k]
                                                      for k in ("rowptr", "entries", "n_nodes", "n_edges", "split", "ws", "n_pairs",
                                                                "gws", "gws_bytes", "total", "stream")])
    assert gcount(n_pairs=-1) == -1 and gcount(total=None) == -1 and gcount(gws=None) == -1 and gcount(ws=None) == -1
    assert gcount(n_pairs=2 ** 31) == -4, "a pair count beyond int32 is LGC_E_RANGE: the caller runs without elimination"
    assert gcount(gws_bytes=16) == -3 and gcount(gws=odd) == -5
    assert lib.lgc_reduce_gram_workspace_bytes(2 ** 31) == 0 and lib.lgc_reduce_gram_workspace_bytes(7) > 0
    gfill = lambda **kw: lib.lgc_reduce_gram_fill(*[{**dict(gws=one, n_pairs=7, n_kept=2, n_items=6, n_out=5, rowptr_out=one,
                                                            entries_out=one, stream=None), **kw}[k]
                                                    for k in ("gws", "n_pairs", "n_kept", "n_items", "n_out", "rowptr_out",
                                                              "entries_out", "stream")])
    assert gfill(gws=None) == -1 and gfill(rowptr_out=None) == -1 and gfill(entries_out=None) == -1 and gfill(n_out=8) == -1
    assert gfill(n_items=0) == -1 and gfill(n_pairs=2 ** 31) == -4 and gfill(gws=odd) == -5


# ----------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forward_with_elimination_against_fp64(device, name, dim):
    pg, split, n, t = built(name, device)
    x = synth.xavier_table(n, dim, 11, device)
    for k in LAYERS:
        for equal in (True, False):
            alphas = alphas_for(k, equal)
            want = layer_sum_fp64(pg.forward_op, x, alphas)
            plain = forward(pg, x, alphas, 0)
            got = forward(pg, x, alphas, t)
            e_got, e_plain = rel_fro(got.cpu(), want), rel_fro(plain.cpu(), want)
            print(f"{name} D={dim} K={k} {'equal' if equal else 'unequal'} alphas: rel_fro eliminated {e_got:.2e} "
                  f"(worst row {worst_row_rel(got.cpu(), want):.2e}), plain {e_plain:.2e}")
            assert e_got <= TOL and e_plain <= TOL, (name, dim, k, equal, e_got, e_plain)
            assert torch.equal(forward(pg, x, alphas, t), got), "two runs must give the same bits"
            auto = forward(pg, x, alphas, None)                       # "auto": too small a graph for the band sweep
            assert torch.equal(auto, plain), "auto must keep today's path on a small graph"
            if k == 1:
                assert torch.equal(got, plain), "K = 1 has no middle layer"
    assert G.ELIMINATE_MAX_DEG == "auto", "the suite runs with the default switch"


@pytest.mark.gpu
@pytest.mark.parametrize("items_only", (True, False))
@pytest.mark.parametrize("name", ("degrees_1_to_12", "hub", "directed", "all_eliminated"))
def test_scored_rows_forward_with_elimination(device, monkeypatch, name, items_only):
    """The training forward (``final_rows``) shares the middle layers: on the scored rows it is the full forward."""
    monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", items_only)
    pg, split, n, t = built(name, device)
    gen = torch.Generator().manual_seed(5)
    rows = torch.cat([torch.randint(0, split, (48,), generator=gen), torch.randint(split, n, (48,), generator=gen)]).to(device)
    for dim in (64, 90):
        x = synth.xavier_table(n, dim, 12, device)
        for k in (2, 3, 5):
            for equal in (True, False):
                alphas = alphas_for(k, equal)
                full = forward(pg, x, alphas, t)
                few = forward(pg, x, alphas, t, final_rows=rows)
                e = rel_fro(few[rows].cpu(), full[rows].cpu())
                assert e <= 1e-6, (name, dim, k, equal, e)
                want = layer_sum_fp64(pg.forward_op, x, alphas)
                assert rel_fro(few[rows].cpu(), want[rows.cpu()]) <= TOL


@pytest.mark.gpu
def test_reduced_item_half_through_the_forced_band_sweep(device, tmp_path):
    """LGCN_SWEEP is read at import: a fresh child (tests/eliminate_child.py) runs the 5,000 x 300 graph with the
    reduced item half as a band sweep and reports the errors."""
    out = tmp_path / "eliminate_child.json"
    env = dict(os.environ, LGCN_SWEEP="1")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eliminate_child.py"), "--out", str(out)], env=env, cwd=ROOT,
                          timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    summary = json.loads(out.read_text())
    print(summary)
    assert summary["item_route_64"].startswith("sweep") and summary["item_route_90"].startswith("sweep_wide")
    assert all(e <= TOL for e in summary["rel_fro"].values()), summary
