"""The concatenated operator [R_H^T | G_L] through the FORCED band sweep, in a process of its own.

LGCN_SWEEP is read when ``gnn_ecommerce_amd.graph`` is imported, so ``tests/test_reduced_concat_gpu.py`` starts this
script with LGCN_SWEEP=1 (as tests/eliminate_child.py is started) and reads the JSON summary it writes to ``--out``.
Every small graph of tests/reduced_concat_support.py at D = 64 with the switch forced on, then the 5,000 x 300 graph of
eliminate_support with ``auto`` at D = 64 (the four-entry plan) and D = 90 (the two-entry plan): on for both.  Each
result against fp64 and against the switch-off path.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from conftest import rel_fro, worst_row_rel  # noqa: E402
from eliminate_support import alphas_for, graph_sweep, layer_sum_fp64  # noqa: E402
from reduced_concat_support import GRAPHS, NOT_COVERED  # noqa: E402
from gnn_ecommerce_amd import graph as G, propagate, synth  # noqa: E402
from gnn_ecommerce_amd.graph import PropGraph  # noqa: E402


def run(summary, name, make, dims_modes, layers, dev):
    ei, ew, split, n, t = make()
    pg = PropGraph(ei.to(dev), ew.to(dev), n)
    pg.eliminate_max_deg = t
    red = pg.reduced()
    assert red is not None and red.gram_op is not None
    hubs = torch.topk(torch.bincount(ei[1], minlength=n), min(20, n)).indices
    for dim, mode in dims_modes:
        x = synth.xavier_table(n, dim, 13, dev)
        t_in, t_out = propagate.scratch_table(x), propagate.scratch_table(x)          # the middle tables' layout
        red.concat_mode = mode
        cc = red.concat_for(dim, n, t_in.stride(0))
        summary[f"auto_{dim}"] = cc is not None
        red.concat_mode = "1"
        cc = red.concat_for(dim, n, t_in.stride(0))
        assert cc is not None and cc.item_op.sweep_cols == (0, cc.csr.n_phys), name
        summary["routes"][name] = cc.item_op.route(t_in[cc.offset:], t_out[cc.offset:])
        for k in layers:
            for equal in (True, False):
                alphas = alphas_for(k, equal)
                want = layer_sum_fp64(pg.forward_op, x, alphas)
                red.concat_mode = mode if (mode is not None or summary[f"auto_{dim}"]) else "1"
                got = propagate._layer_sum(pg, x, alphas, transpose=False)
                assert torch.equal(got, propagate._layer_sum(pg, x, alphas, transpose=False)), ("two runs differ", name, dim, k)
                red.concat_mode = "0"
                off = propagate._layer_sum(pg, x, alphas, transpose=False)
                key = f"{name}/{dim}/{k}/{int(equal)}"
                summary["rel_fro"][key] = rel_fro(got.cpu(), want)
                summary["rel_fro"][key + "/off"] = rel_fro(off.cpu(), want)
                summary["worst_row"][key] = worst_row_rel(got.cpu()[hubs], want[hubs])
                summary["on_off"][key] = rel_fro(got.cpu(), off.cpu())
                print(f"{key}: rel_fro {summary['rel_fro'][key]:.2e} (off {summary['rel_fro'][key + '/off']:.2e}), "
                      f"hub rows {summary['worst_row'][key]:.2e}, on against off {summary['on_off'][key]:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert G.USE_SWEEP == "1", "start this script with LGCN_SWEEP=1"
    assert G.REDUCED_CONCAT == "auto", "start this script with the default LGCN_REDUCED_CONCAT"
    dev = torch.device("cuda:0")
    summary = {"routes": {}, "rel_fro": {}, "worst_row": {}, "on_off": {}}
    for name in sorted(set(GRAPHS) - set(NOT_COVERED)):
        run(summary, name, GRAPHS[name], ((64, "1"),), (2, 3, 5), dev)
    run(summary, "sweep_graph", graph_sweep, ((90, None), (64, None)), (2, 3), dev)
    torch.cuda.synchronize()
    with open(args.out, "w") as f:
        json.dump(summary, f)


if __name__ == "__main__":
    main()
