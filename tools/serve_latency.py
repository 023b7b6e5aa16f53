#!/usr/bin/env python3
"""Latency of one serving request (torchserve/lightgcn_handler.py:73-96 -> LightGCN.recommendK, k=20) on the
cosmetics-scale graph: with the propagated table reused across requests (default) and recomputed per
request as upstream does; and of a SESSION request -- visitors the model was not trained on, 20 items each, through
LightGCN.recommend_sessions (fold-in) -- next to the known-user request on the same device path (recommend_topk),
lgc_fold_in alone under HIP events, and the one-time cost of the fold table."""
import json, os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import synth

dev = torch.device("cuda:0")
g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=0)
ei, ew = g.coo(dev)
model = lg.LightGCN(g.num_nodes, 64, 3).to(dev).eval()
out = {}
for n_users in (1, 64):
    users = list(range(7, 7 + n_users))
    seen = torch.zeros(n_users, g.n_items)
    seen_dev = seen.to(dev)                      # a caller that keeps its interaction rows on the device
    model.cache_recommend_embeddings = True
    ts = []
    with torch.no_grad():
        for _ in range(23):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.recommendK(ei, ew, g.n_users, g.n_items, seen_dev, users, 20)
            ts.append((time.perf_counter() - t0) * 1e3)
    out[f"users{n_users}_reuse_devmask_ms"] = round(statistics.median(ts[3:]), 3)
    for reuse in (True, False):
        model.cache_recommend_embeddings = reuse
        ts = []
        with torch.no_grad():
            for _ in range(13):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                model.recommendK(ei, ew, g.n_users, g.n_items, seen, users, 20)
                ts.append((time.perf_counter() - t0) * 1e3)
        out[f"users{n_users}_{'reuse' if reuse else 'recompute'}_ms"] = round(statistics.median(ts[3:]), 3)
# the select kernel alone (HIP events): dense device mask and the list form
from gnn_ecommerce_amd.propagate import SeenLists, mask_topk
for rows in (1, 64, 1024):
    sc = torch.randn(rows, g.n_items, device=dev)
    dense = (torch.rand(rows, g.n_items, device=dev) < 0.001).float()
    nz = torch.nonzero(dense)
    ptr = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(dense.sum(dim=1).long(), 0)
    lists = SeenLists(ptr, nz[:, 1].contiguous(), torch.arange(rows, device=dev))
    for name, m in (("dense", dense), ("lists", lists)):
        for _ in range(3):
            mask_topk(sc, m, 20)
        ts = []
        for _ in range(20):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); mask_topk(sc, m, 20); e.record(); torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) * 1e3)
        out[f"mask_topk_rows{rows}_{name}_us"] = round(statistics.median(ts), 1)
# session requests (fold-in): the request's lists are built and uploaded inside the timed region, as a handler would
import numpy as np
from gnn_ecommerce_amd.foldin import SessionLists, fold_in, fold_table
from gnn_ecommerce_amd.graph import get_graph
model.cache_recommend_embeddings = True
rng = np.random.default_rng(0)
graph = get_graph(ei, ew, g.num_nodes)
purchases = SeenLists(torch.zeros(g.n_users + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def median_ms(fn, runs=23, warm=3):
    ts = []
    with torch.no_grad():
        for _ in range(runs):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts[warm:]), 3)


for rows in (1, 64):
    lists = [(rng.integers(g.n_items, size=20).tolist(), rng.choice([0.01, 0.1, 1.0], size=20).tolist()) for _ in range(rows)]
    ids = torch.arange(7, 7 + rows, device=dev)
    out[f"sessions{rows}_recommend_ms"] = median_ms(
        lambda: model.recommend_sessions(ei, ew, g.n_users, g.n_items, SessionLists.from_lists(lists, dev), None, 20))
    out[f"sessions{rows}_lists_upload_ms"] = median_ms(lambda: SessionLists.from_lists(lists, dev).validate(g.n_items))
    ready = SessionLists.from_lists(lists, dev).validate(g.n_items)
    out[f"sessions{rows}_embed_ms"] = median_ms(lambda: model.embed_sessions(ei, ew, g.n_users, g.n_items, ready))
    out[f"sessions{rows}_mask_ms"] = median_ms(lambda: ready.mask("purchased"))
    # the known-user request on the same path: device ids in, device indices out, list mask
    out[f"users{rows}_recommend_topk_ms"] = median_ms(
        lambda: model.recommend_topk(ei, ew, g.n_users, g.n_items, purchases, ids, 20))
# lgc_fold_in alone (HIP events)
fold = fold_table(model, graph)
dis = graph.dis[g.n_users:]
for rows, entries in ((1, 20), (64, 20), (1024, 20), (64, 5000)):
    lists = [(rng.integers(g.n_items, size=entries), rng.choice([0.01, 0.1, 1.0], size=entries)) for _ in range(rows)]
    sess = SessionLists.from_lists(lists, dev)
    for _ in range(3):
        fold_in(fold, dis, sess)
    ts = []
    for _ in range(20):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fold_in(fold, dis, sess); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    out[f"fold_in_rows{rows}_x{entries}_us"] = round(statistics.median(ts), 1)
# the one-time fold table (K - 1 hops), the graph's plans already built by the served table
for dim, layers in ((64, 3), (90, 5)):
    m = model if (dim, layers) == (64, 3) else lg.LightGCN(g.num_nodes, dim, layers).to(dev).eval()
    with torch.no_grad():
        m._serving_embedding(ei, ew)
    ts = []
    for _ in range(4):
        m._fold = None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            fold_table(m, graph)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    out[f"fold_table_d{dim}_k{layers}_first_ms"] = round(ts[0], 3)
    out[f"fold_table_d{dim}_k{layers}_ms"] = round(statistics.median(ts[1:]), 3)
print(json.dumps(out))
