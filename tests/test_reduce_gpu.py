"""The middle-hop reduction builder (lgc_reduce_count / _fill / _gram_count / _gram_fill) against the exact host reference
of tests/reduce_support.py -- every output of every call for equality, value bits included -- on small named operators,
on an input large enough for the size-dependent paths, and beyond the int32 pair count; then the ``auto`` rule of
``PropGraph.reduced`` on a graph where every default switches the reduction and the concatenated operator on."""
import numpy as np
import pytest
import torch

from conftest import rel_fro
from eliminate_support import GRAPHS as SMALL_GRAPHS, alphas_for, layer_sum_fp64
from reduce_support import (CASES, INT32_MAX, LARGE_T, Case, assert_equals_reference, auto_graph, call_builder,
                            complete_bipartite, large_case, reduce_reference, reduce_reference_fast)
from gnn_ecommerce_amd import _native, graph as G, propagate, synth
from gnn_ecommerce_amd.graph import PropGraph, ReducedGraph

TOL = 1e-5          # the project's gate on rel_fro against fp64


def same_outputs(a, b):
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), f"{key} depends on what the workspaces held before the call"
        else:
            assert a[key] == b[key], key


# ----------------------------------------------------------------------------------------
# named hand-built operators
# ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case_equals_the_reference_at_every_threshold(device, name):
    """Guards: order_shows -- the stable sort and the expansion order (and fp64 products); cancels_to_zero -- the +0 start
    of a run's sum and "stored iff it has a product"; duplicates, threshold -- both halves of the keep rule, incount by
    entries; wrong_side -- the column guards and the filler slots; the others -- the degenerate shapes."""
    case = CASES[name]()
    assert {0, 1, 2, 3, INT32_MAX} <= set(case.thresholds())
    for t in case.thresholds():
        want = reduce_reference(case.rowptr, case.cols, case.val_bits, case.split, case.n_nodes, t)
        zeros = call_builder(device, case, t, fill=0x00)
        ones = call_builder(device, case, t, fill=0xFF)
        try:
            assert_equals_reference(zeros, want, case.well_formed)
            assert_equals_reference(ones, want, case.well_formed)
        except AssertionError as exc:
            raise AssertionError(f"{name} at T = {t}: {exc}") from exc
        same_outputs(zeros, ones)
    if name == "order_shows":
        got = call_builder(device, case, 3)["gram_entries"][:, 1].view(np.float32).tolist()
        assert got == [1.0, 1.0], "the runs 2^60 - 2^60 + 1 must be summed in expansion order"
    if name == "cancels_to_zero":
        assert call_builder(device, case, 1)["gram_entries"][:, 1].tolist() == [0, 0], "two stored zeros, both +0.0"
    if name == "duplicates":
        assert call_builder(device, case, 2)["user_map"].tolist() == [-1, 0], "named T + 1 times by one row: kept"
    if name == "dense_block":
        assert call_builder(device, case, 4)["total"] == 36


@pytest.mark.gpu
@pytest.mark.parametrize("name,t", (("threshold", 2), ("duplicates", 2), ("wrong_side", 4), ("dense_block", 4), ("smallest", 0),
                                    ("smallest", 1), ("order_shows", 1)))
def test_undersized_n_out_writes_nothing_at_or_beyond_it(device, name, t):
    """``n_out`` one below the true size in lgc_reduce_fill and lgc_reduce_gram_fill: the element at ``n_out`` keeps its
    sentinel (the buffers have their full size) and everything before it is the reference's."""
    case = CASES[name]()
    want = reduce_reference(case.rowptr, case.cols, case.val_bits, case.split, case.n_nodes, t)
    assert want.nnz > 0 or want.gram_entries.shape[0] > 0
    assert_equals_reference(call_builder(device, case, t, fill=0xFF, short=True), want, case.well_formed, short=True)


# ----------------------------------------------------------------------------------------
# size-dependent paths
# ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_large_input_equals_the_vectorised_reference(device):
    """More than 1,048,576 entries in the item half: a second grid-stride trip of the counting kernel, scans and a sort
    of millions of elements, scratch sized for them."""
    case = large_case()
    assert case.cols.size - int(case.rowptr[case.split]) > 4096 * 256
    want = reduce_reference_fast(case.rowptr, case.cols, case.val_bits, case.split, case.n_nodes, LARGE_T)
    assert want.pairs_min == want.pairs_max > 2_000_000 and 0 < want.n_kept < case.split
    assert want.gram_entries.shape[0] > 1_000_000
    zeros = call_builder(device, case, LARGE_T, fill=0x00)
    ones = call_builder(device, case, LARGE_T, fill=0xFF)
    assert_equals_reference(zeros, want)
    assert_equals_reference(ones, want)


def _spy_on_builder(monkeypatch):
    calls = []
    real = G.build_reduced_csr

    def counted(rowptr, entries, split, num_nodes, max_deg):
        calls.append(int(max_deg))
        return real(rowptr, entries, split, num_nodes, max_deg)
    monkeypatch.setattr(G, "build_reduced_csr", counted)
    return calls


def _forward(pg, x, alphas, max_deg):
    pg.eliminate_max_deg = max_deg
    try:
        return propagate._layer_sum(pg, x, alphas, transpose=False)
    finally:
        pg.eliminate_max_deg = None


@pytest.mark.gpu
def test_pair_count_beyond_int32_runs_without_elimination(device, monkeypatch):
    """1,000 x 1,500 complete: 3 M entries, and with T = 1500 every user goes and expands into 2.25e9 pairs."""
    n_users, n_items, t = 1000, 1500, 1500
    ei, ew = complete_bipartite(n_users, n_items)
    pg = PropGraph(ei.to(device), ew.to(device), n_users + n_items)
    assert pg.split == n_users
    op = pg.forward_op
    case = Case(op.rowptr.cpu().numpy(), op.entries[:, 0].cpu().numpy(), op.entries[:, 1].cpu().numpy(), n_users,
                n_users + n_items)
    got = call_builder(device, case, t, fill=0xFF)
    assert got["totals"].tolist() == [0, 0, 0, n_users * n_items * n_items] and got["totals"][3] == 2_250_000_000
    assert got["gram_workspace_bytes"] == 0 and got["user_map"].tolist() == [-1] * n_users
    assert G.build_reduced_csr(op.rowptr, op.entries, n_users, n_users + n_items, t) is None
    calls = _spy_on_builder(monkeypatch)
    pg.eliminate_max_deg = t
    try:
        assert pg.reduced() is None and pg.reduced() is None
    finally:
        pg.eliminate_max_deg = None
    assert calls == [t], "the refusal is cached: one build"
    x = synth.xavier_table(n_users + n_items, 64, 13, device)
    alphas = alphas_for(3, True)
    assert torch.equal(_forward(pg, x, alphas, t), _forward(pg, x, alphas, 0)), "the plain forward, bit for bit"
    assert calls == [t]


# ----------------------------------------------------------------------------------------
# the auto rule with every switch at its default
# ----------------------------------------------------------------------------------------
_auto = {}


def auto_inputs(device):
    if "edges" not in _auto:
        ei, ew, split, n = auto_graph()
        _auto["edges"] = (ei.to(device), ew.to(device), split, n)
    return _auto["edges"]


def auto_built(device):
    """The graph with nothing forced, built once; (PropGraph, split, n)."""
    if "pg" not in _auto:
        ei, ew, split, n = auto_inputs(device)
        pg = PropGraph(ei, ew, n)
        assert pg.split == split and pg.eliminate_max_deg is None
        _auto["pg"] = pg
    return _auto["pg"], _auto["edges"][2], _auto["edges"][3]


def assert_defaults():
    assert (G.ELIMINATE_MAX_DEG, G.REDUCED_CONCAT, G.USE_SWEEP) == ("auto", "auto", "auto"), "the suite runs with the defaults"
    assert (G.ELIMINATE_AUTO_MAX_DEG, G.ELIMINATE_MAX_GRAM_SHARE) == (3, 1.0)
    assert (G.ELIMINATE_AUTO_MAX_DEG_CONCAT, G.ELIMINATE_MAX_GRAM_SHARE_CONCAT) == (4, 1.25)


@pytest.mark.gpu
def test_auto_switches_itself_on(device):
    assert_defaults()
    pg, split, n = auto_built(device)
    item_half = pg.halves(False)[1]
    assert item_half.sweep_cols == (0, split), "the full item half must take the band sweep"
    red = pg.reduced()
    assert isinstance(red, ReducedGraph) and red.csr.max_deg == G.ELIMINATE_AUTO_MAX_DEG_CONCAT
    assert red.concat_for(64, n, 64) is not None, "the concatenated operator must run at D = 64"
    assert red.concat_for(64, n, 64).item_op.sweep_cols is not None and red.item_op_h.sweep_cols is not None
    removed = pg.forward_op.nnz - red.csr.nnz
    share = red.csr.gram_nnz / removed
    print(f"auto graph: n_kept {red.n_h}, removed {removed}, nnz(G_L) {red.csr.gram_nnz}, share {share:.3f}")
    assert share < 0.5 * G.ELIMINATE_MAX_GRAM_SHARE_CONCAT, "the graph must sit well inside the share limit"
    assert pg.reduced() is red and pg.reduced(transpose=True) is None
    # and the builder's output on it, bit for bit
    op = pg.forward_op
    want = reduce_reference_fast(op.rowptr.cpu().numpy(), op.entries[:, 0].cpu().numpy(), op.entries[:, 1].cpu().numpy(),
                                 split, n, red.csr.max_deg)
    assert (want.n_kept, want.user_nnz, want.pairs_min) == (red.csr.n_h, red.csr.user_nnz, red.csr.n_pairs)
    for f, w in (("user_map", want.user_map), ("rowptr", want.rowptr), ("entries", want.entries),
                 ("gram_rowptr", want.gram_rowptr), ("gram_entries", want.gram_entries)):
        assert torch.equal(getattr(red.csr, f).cpu(), torch.from_numpy(w)), f


@pytest.mark.gpu
@pytest.mark.parametrize("dim,k", ((64, 3), (90, 2)))
def test_auto_forward_against_fp64(device, dim, k):
    assert_defaults()
    pg, split, n = auto_built(device)
    assert pg.reduced() is not None
    x = synth.xavier_table(n, dim, 17, device)
    alphas = alphas_for(k, True)
    got = propagate._layer_sum(pg, x, alphas, transpose=False)
    want = layer_sum_fp64(pg.forward_op, x, alphas)
    err = rel_fro(got.cpu(), want)
    print(f"auto graph D={dim} K={k}: rel_fro {err:.2e}")
    assert err <= TOL
    assert torch.equal(propagate._layer_sum(pg, x, alphas, transpose=False), got), "two runs must give the same bits"
    forced = _forward(pg, x, alphas, G.ELIMINATE_AUTO_MAX_DEG_CONCAT)
    assert torch.equal(forced, got), "auto must be the forward with T forced to its choice"
    assert not torch.equal(_forward(pg, x, alphas, 0), got), "the reduced layers add in another order: a different path ran"


@pytest.mark.gpu
def test_auto_declines_beyond_the_share_limit(device, monkeypatch):
    assert_defaults()
    pg, split, n = auto_built(device)
    red = pg.reduced()
    removed, gram_nnz = pg.forward_op.nnz - red.csr.nnz, red.csr.gram_nnz
    ei, ew, _, _ = auto_inputs(device)
    monkeypatch.setattr(G, "ELIMINATE_MAX_GRAM_SHARE_CONCAT", (gram_nnz + 0.5) / removed)
    just_inside = PropGraph(ei, ew, n)
    got = just_inside.reduced()
    assert got is not None and got.csr.gram_nnz == gram_nnz
    monkeypatch.setattr(G, "ELIMINATE_MAX_GRAM_SHARE_CONCAT", (gram_nnz - 0.5) / removed)
    calls = _spy_on_builder(monkeypatch)
    just_outside = PropGraph(ei, ew, n)
    assert just_outside.reduced() is None and just_outside.reduced() is None
    assert calls == [G.ELIMINATE_AUTO_MAX_DEG_CONCAT], "built once, declined, and the refusal cached"
    x = synth.xavier_table(n, 64, 17, device)
    alphas = alphas_for(3, True)
    plain = _forward(just_outside, x, alphas, 0)
    assert torch.equal(propagate._layer_sum(just_outside, x, alphas, transpose=False), plain)
    assert not torch.equal(propagate._layer_sum(just_inside, x, alphas, transpose=False), plain)


@pytest.mark.gpu
def test_auto_without_the_concatenated_operator_takes_the_other_pair(device, monkeypatch):
    assert_defaults()
    ei, ew, split, n = auto_inputs(device)
    monkeypatch.setattr(G, "REDUCED_CONCAT", "0")
    monkeypatch.setattr(G, "ELIMINATE_MAX_GRAM_SHARE_CONCAT", 0.0)          # must not be the limit that is read
    calls = _spy_on_builder(monkeypatch)
    pg = PropGraph(ei, ew, n)
    red = pg.reduced()
    assert calls == [G.ELIMINATE_AUTO_MAX_DEG] and red is not None and red.csr.max_deg == G.ELIMINATE_AUTO_MAX_DEG
    assert red.concat_for(64, n, 64) is None
    removed, gram_nnz = pg.forward_op.nnz - red.csr.nnz, red.csr.gram_nnz
    assert gram_nnz <= G.ELIMINATE_MAX_GRAM_SHARE * removed
    monkeypatch.setattr(G, "ELIMINATE_MAX_GRAM_SHARE", (gram_nnz - 0.5) / removed)
    monkeypatch.setattr(G, "ELIMINATE_MAX_GRAM_SHARE_CONCAT", 1.25)
    assert PropGraph(ei, ew, n).reduced() is None
    monkeypatch.setattr(G, "ELIMINATE_MAX_GRAM_SHARE", (gram_nnz + 0.5) / removed)
    assert PropGraph(ei, ew, n).reduced() is not None
    assert calls == [G.ELIMINATE_AUTO_MAX_DEG] * 3


@pytest.mark.gpu
def test_auto_on_a_small_graph_never_calls_the_builder(device, monkeypatch):
    assert_defaults()
    ei, ew, split, n, _ = SMALL_GRAPHS["degrees_1_to_12"]()
    calls = _spy_on_builder(monkeypatch)
    pg = PropGraph(ei.to(device), ew.to(device), n)
    assert pg.halves(False)[1].sweep_cols is None
    assert pg.reduced() is None and pg.reduced(transpose=True) is None and pg.reduced() is None
    assert calls == []
    pg.eliminate_max_deg = 3
    try:
        assert pg.reduced() is not None and pg.reduced(transpose=True) is None
    finally:
        pg.eliminate_max_deg = None
    assert calls == [3]
