#!/usr/bin/env python3
"""T sweep of the middle-hop reduction (PropGraph.reduced) on the full-size graph, the variants interleaved in ONE process
like tools/ab_hop.py: per T the builder's counts, build / plan times and device memory, then ROUNDS rounds of 3 warm-up +
STEPS timed get_embedding steps at D=64 / K=3 and D=90 / K=5, and the result against T = 0.
Usage:  python tools/eliminate_sweep.py [out.json]     env: TS (0,2,3,4,5,6), ROUNDS (5), STEPS (20)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import gnn_ecommerce_amd as lg  # noqa: E402
from gnn_ecommerce_amd import graph as G, propagate, synth  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "eliminate_sweep.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
TS = [int(t) for t in os.environ.get("TS", "0,2,3,4,5,6").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", "5"))
STEPS = int(os.environ.get("STEPS", "20"))
CONFIGS = [(64, 3), (90, 5)]
dev = torch.device("cuda:0")
res = {"builds": {}, "timing": {}, "parity": {}, "gram_chunk_len": G.GRAM_CHUNK_LEN}


def dump():
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=0)
n = g.num_nodes
ei, ew = g.coo(dev)
pg = lg.PropGraph(ei, ew, n)
torch.cuda.synchronize()
t0 = time.perf_counter()
pg.prepare(64)
res["plan_build_s_plain_d64"] = time.perf_counter() - t0
t0 = time.perf_counter()
pg.prepare(90)
res["plan_build_s_plain_d90_after_d64"] = time.perf_counter() - t0
print("plain plans", res["plan_build_s_plain_d64"], res["plan_build_s_plain_d90_after_d64"], flush=True)

for t in TS:
    if t == 0:
        continue
    pg.eliminate_max_deg = t
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    red = pg.reduced()
    torch.cuda.synchronize()
    t_csr = time.perf_counter() - t0
    t0 = time.perf_counter()
    pg.prepare(64)
    t_plan64 = time.perf_counter() - t0
    m1 = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    pg.prepare(90)
    t_plan90 = time.perf_counter() - t0
    m2 = torch.cuda.memory_allocated()
    c = red.csr
    removed = pg.forward_op.nnz - c.nnz
    res["builds"][t] = dict(n_h=c.n_h, users_eliminated=pg.split - c.n_h, nnz_reduced=c.nnz, entries_removed=removed,
                            n_pairs=c.n_pairs, gram_nnz=c.gram_nnz, gram_share=c.gram_nnz / max(removed, 1),
                            build_csr_s=t_csr, plans_d64_s=t_plan64, plans_d90_more_s=t_plan90,
                            extra_bytes_d64=m1 - m0, extra_bytes_d90_more=m2 - m1,
                            item_h_sweep=red.item_op_h.sweep_cols is not None,
                            gram_chunks=red.gram_op.plan.n_chunks, gram_multi=red.gram_op.plan.n_multi)
    print(t, res["builds"][t], flush=True)
    dump()


def run(x0, alphas, t, steps):
    pg.eliminate_max_deg = t
    for _ in range(3):
        propagate.propagate_sum(x0, pg, alphas)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = propagate.propagate_sum(x0, pg, alphas)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, out


for dim, layers in CONFIGS:
    alphas = tuple([1.0 / (layers + 1)] * (layers + 1))
    x0 = synth.xavier_table(n, dim, 0, dev)
    key = f"d{dim}_k{layers}"
    res["timing"][key] = {t: [] for t in TS}
    ref = None
    for r in range(ROUNDS):
        for t in TS:
            ms, out = run(x0, alphas, t, STEPS)
            res["timing"][key][t].append(ms)
            if r == 0:
                if t == 0:
                    ref = out.double()
                else:
                    res["parity"][f"{key}_T{t}"] = ((out.double() - ref).norm() / ref.norm()).item()
            del out
        print(key, "round", r, {t: round(res["timing"][key][t][-1], 4) for t in TS}, flush=True)
        dump()
    del ref
pg.eliminate_max_deg = None
dump()
print("done", flush=True)
