"""The reduced layers on the concatenated operator [R_H^T | G_L] (LGCN_REDUCED_CONCAT, ``ReducedGraph.concat_for``):
``propagate_sum``'s layer sum with the switch on against an fp64 reference built here, and against the switch-off path.
T is forced to 3 through ``PropGraph.eliminate_max_deg``, the switch through ``ReducedGraph.concat_mode``; the graphs
(tests/reduced_concat_support.py) are too small for the band sweep, which tests/reduced_concat_child.py forces in a
process of its own."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, rel_fro, worst_row_rel
from eliminate_support import alphas_for, layer_sum_fp64
from reduced_concat_support import GRAPHS, N_GAPS, NOT_COVERED, T
from gnn_ecommerce_amd import graph as G, propagate, synth
from gnn_ecommerce_amd.graph import PropGraph, build_concat_csr

TOL = 1e-5          # the project's gate on rel_fro against fp64; the hub rows' limit of tests/test_parity_gpu.py as well
TOL_PATHS = 1e-6    # two paths of one sum against each other (test_scored_rows_forward_with_elimination)

_graphs = {}


def built(name, device):
    if name not in _graphs:
        ei, ew, split, n, t = GRAPHS[name]()
        assert t == T
        pg = PropGraph(ei.to(device), ew.to(device), n)
        assert pg.split == split
        _graphs[name] = (pg, split, n)
    return _graphs[name]


def layer_sum(pg, x, alphas, mode, transpose=False):
    pg.eliminate_max_deg = T
    red = pg.reduced()
    try:
        red.concat_mode = mode
        return propagate._layer_sum(pg, x, alphas, transpose=transpose)
    finally:
        red.concat_mode = None
        pg.eliminate_max_deg = None


def concat_of(pg, dim=64):
    pg.eliminate_max_deg = T
    red = pg.reduced()
    pg.eliminate_max_deg = None
    red.concat_mode = "1"
    try:
        return red, red.concat_for(dim, pg.num_nodes, dim)
    finally:
        red.concat_mode = None


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_device_builder_equals_host_builder(device, name):
    pg, split, n = built(name, device)
    red, cc = concat_of(pg)
    if name in NOT_COVERED:
        assert cc is None
        if name == "none_eliminated":
            return
    c = red.csr
    dev_arrays = build_concat_csr(c, N_GAPS)
    host_csr = G.ReducedCSR(c.max_deg, c.n_h, c.n_items, c.user_map.cpu(), c.rowptr.cpu(), c.entries.cpu(), c.user_nnz,
                            c.n_pairs, c.gram_rowptr.cpu(), c.gram_entries.cpu())
    host_arrays = build_concat_csr(host_csr, N_GAPS, host=True)
    for f in ("user_pos", "gap_start", "rowptr", "entries"):
        assert torch.equal(getattr(dev_arrays, f).cpu(), getattr(host_arrays, f)), f
    assert dev_arrays.n_phys == host_arrays.n_phys
    if cc is not None:
        assert cc.offset == split - dev_arrays.n_phys >= 0 and torch.equal(cc.csr.entries, dev_arrays.entries)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", (64, 8))
@pytest.mark.parametrize("name", sorted(set(GRAPHS) - set(NOT_COVERED)))
def test_user_step_fills_the_gaps_with_the_item_rows(device, name, dim):
    """The one-entry gap rows: after the user step, gap row of item j holds x[item j] bit for bit, and every kept
    user's row is what the reduced user operator writes."""
    pg, split, n = built(name, device)
    red, cc = concat_of(pg, dim)
    x = synth.xavier_table(n, dim, 3, device)
    out = torch.full_like(x, float("nan"))
    cc.user_op.apply(x[cc.offset:], out[cc.offset:])
    c = cc.csr
    j = torch.arange(red.csr.n_items, device=device)
    item_rows = cc.offset + c.gap_start.long()[j // c.gap_rows] + j % c.gap_rows
    assert torch.equal(out[item_rows], x[split:])
    if red.user_op_h is not None:
        ref = torch.empty_like(x)
        red.user_op_h.apply(x[red.offset:], ref[red.offset:])
        assert torch.equal(out[cc.offset + c.user_pos.long()], ref[red.offset:split])
    assert torch.isnan(out[split:]).all() and torch.isnan(out[:cc.offset]).all(), "no row outside the view's user part is written"


@pytest.mark.gpu
@pytest.mark.parametrize("dim", (64, 8))
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_layer_sum_with_the_concatenated_operator(device, name, dim):
    pg, split, n = built(name, device)
    _, cc = concat_of(pg, dim)
    assert (cc is None) == (name in NOT_COVERED)
    x = synth.xavier_table(n, dim, 11, device)
    hubs = torch.topk(torch.bincount(pg._edge_index[1], minlength=n), min(20, n)).indices.cpu()
    for transpose in (False, True):
        op = pg.transpose_op if transpose else pg.forward_op
        for k in (2, 3, 5):
            for equal in (True, False):
                alphas = alphas_for(k, equal)
                want = layer_sum_fp64(op, x, alphas)
                on = layer_sum(pg, x, alphas, "1", transpose)
                off = layer_sum(pg, x, alphas, "0", transpose)
                auto = layer_sum(pg, x, alphas, None, transpose)
                e_on, e_off, e_paths = rel_fro(on.cpu(), want), rel_fro(off.cpu(), want), rel_fro(on.cpu(), off.cpu())
                hub = worst_row_rel(on.cpu()[hubs], want[hubs])
                print(f"{name} D={dim} K={k} {'equal' if equal else 'unequal'} alphas{' transposed' if transpose else ''}: "
                      f"rel_fro on {e_on:.2e} off {e_off:.2e} on-off {e_paths:.2e}, worst hub row {hub:.2e}")
                assert e_on <= TOL and e_off <= TOL, (name, dim, k, equal, transpose, e_on, e_off)
                assert hub <= TOL
                assert e_paths <= TOL_PATHS
                assert torch.equal(layer_sum(pg, x, alphas, "1", transpose), on), "two runs must give the same bits"
                assert torch.equal(auto, off), "auto keeps the separate launch on a graph too small for the band sweep"
                if cc is None or transpose:
                    assert torch.equal(on, off), "where the concatenated operator does not apply the path is unchanged"


@pytest.mark.gpu
def test_concatenated_operator_through_the_forced_band_sweep(device, tmp_path):
    """LGCN_SWEEP is read at import: a fresh child (tests/reduced_concat_child.py) runs every graph with the
    concatenated item step as a band sweep (D = 64), and the 5,000 x 300 graph at D = 64 and 90 with ``auto``."""
    out = tmp_path / "reduced_concat_child.json"
    env = dict(os.environ, LGCN_SWEEP="1")
    env.pop("LGCN_REDUCED_CONCAT", None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reduced_concat_child.py"), "--out", str(out)], env=env,
                          cwd=ROOT, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    summary = json.loads(out.read_text())
    print(proc.stdout)
    assert set(summary["routes"]) == set(GRAPHS) - set(NOT_COVERED) | {"sweep_graph"}
    assert all(r.startswith("sweep") for r in summary["routes"].values()), summary["routes"]
    assert summary["auto_64"] is True and summary["auto_90"] is True, "auto: on wherever the item step is a band sweep"
    assert all(e <= TOL for e in summary["rel_fro"].values()), summary
    assert all(e <= TOL for e in summary["worst_row"].values()), summary
    assert all(e <= TOL_PATHS for e in summary["on_off"].values()), summary
