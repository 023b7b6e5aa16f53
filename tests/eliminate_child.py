"""The reduced item half through the FORCED band sweep, in a process of its own.

LGCN_SWEEP is read when ``gnn_ecommerce_amd.graph`` is imported, so ``tests/test_eliminate_gpu.py`` starts this script
with LGCN_SWEEP=1 in its environment (as tests/route_child.py is started) and reads the JSON summary it writes to
``--out``.  5,000 users x 300 items, T = 4: the full item half and the reduced one both run as band sweeps (D = 64:
four entries per step, D = 90: two), the G_L product through chunks and tiles.  Every check is an assert.
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

from conftest import rel_fro  # noqa: E402
from eliminate_support import alphas_for, graph_sweep, layer_sum_fp64  # noqa: E402
from gnn_ecommerce_amd import graph as G, propagate, synth  # noqa: E402
from gnn_ecommerce_amd.graph import PropGraph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert G.USE_SWEEP == "1", "start this script with LGCN_SWEEP=1"
    dev = torch.device("cuda:0")
    ei, ew, split, n, t = graph_sweep()
    pg = PropGraph(ei.to(dev), ew.to(dev), n)
    assert pg.split == split
    pg.eliminate_max_deg = t
    red = pg.reduced()
    assert red is not None and 0 < red.n_h < split and red.gram_op is not None
    assert red.item_op_h.sweep_cols == (0, red.n_h) and pg.halves()[1].sweep_cols == (0, split)
    summary = {"n_h": red.n_h, "gram_nnz": red.csr.gram_nnz, "rel_fro": {}}
    for dim in (64, 90):
        x = synth.xavier_table(n, dim, 13, dev)
        t_in, t_out = propagate.scratch_table(x), propagate.scratch_table(x)      # the middle tables' layout
        summary[f"item_route_{dim}"] = red.item_op_h.route(t_in[red.offset:], t_out[red.offset:])
        for k in (2, 3, 5):
            for equal in (True, False):
                alphas = alphas_for(k, equal)
                want = layer_sum_fp64(pg.forward_op, x, alphas)
                got = propagate._layer_sum(pg, x, alphas, transpose=False)
                again = propagate._layer_sum(pg, x, alphas, transpose=False)
                assert torch.equal(got, again), ("two runs differ", dim, k, equal)
                pg.eliminate_max_deg = 0
                plain = propagate._layer_sum(pg, x, alphas, transpose=False)
                pg.eliminate_max_deg = t
                e, e_plain = rel_fro(got.cpu(), want), rel_fro(plain.cpu(), want)
                print(f"D={dim} K={k} equal={equal}: rel_fro eliminated {e:.2e}, plain {e_plain:.2e}", flush=True)
                summary["rel_fro"][f"{dim}/{k}/{int(equal)}"] = e
                summary["rel_fro"][f"{dim}/{k}/{int(equal)}/plain"] = e_plain
    torch.cuda.synchronize()
    with open(args.out, "w") as f:
        json.dump(summary, f)


if __name__ == "__main__":
    main()
