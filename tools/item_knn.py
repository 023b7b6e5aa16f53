#!/usr/bin/env python3
"""The item-kNN recommender at full size: ``lgc_knn_recommend`` (HIP events around the call: the accumulate-filter-select
kernel, and the merge where the catalogue is cut into bands) over a neighbour table of the bench's cosmetics-scale synthetic
graph, k = 20, cosine, 64 neighbours an item.

  fit        ``ItemKNN.fit``: the neighbour table of the whole catalogue (``cooccur_topk`` at k = 64).
  recommend  10^4 users' purchase lists as baskets, at bands of 4,096, 8,192 and 16,384 items and at the library's choice
             (0); session requests of 1, 8 and 64 baskets; and the user with the most purchases alone -- beside the route
             the library could compose before: the table as a sparse matrix, ``torch.sparse.mm`` with the dense 0 / 1 rows
             of a chunk of baskets into a score panel, the basket's own items and the unvoted ones set to -inf, and
             ``lgc_mask_topk`` over the panel.  The composed route sums in another order, so only the share of equal rows is
             reported.
  quality    on ``tools/train_demo.py``'s split and after its default training run: ``ItemKNN.evaluate`` beside
             ``LightGCN.evaluate_metrics`` at cutoffs 5, 10, 20.

Protocol: one process per step, both routes warmed up, then alternating blocks of ``--reps`` calls each, a HIP-event pair
around every call; the median over all calls of a route and its range (min .. max).  No speed is promised.

    python tools/item_knn.py [--k 20 --reps 5 --blocks 3]

The driver opens no GPU: every step is a child process under its own ``timeout``; one JSON line per step at its end."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bought_together import alternate  # noqa: E402  (the timing protocol has one copy)

SEED = 0
STEPS = ("fit", "recommend", "quality")
BANDS = (4096, 8192, 16384, 0)
KN = 64


def fmt(t):
    unit, div = ("ms", 1e3) if t[0] >= 1e3 else ("us", 1.0)
    return f"{t[0] / div:.1f} {unit} ({t[1] / div:.1f} .. {t[2] / div:.1f})"


def speed_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, cooccur, propagate, synth
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    nu, ni, k = g.n_users, g.n_items, args.k
    ei, _ = g.coo(dev)
    lists = cooccur.CoPurchase.from_edges(ei, nu, ni)
    res = {"step": args.step, "k": k, "kn": KN, "n_users": nu, "n_items": ni, "entries": int(lists.seen.items.numel()), "runs": []}
    if args.step == "fit":
        got = alternate({"fit": ((lambda: lg.ItemKNN.fit(lists, KN)), 0)}, args.reps, args.blocks)["fit"]
        print(f"ItemKNN.fit, {ni} items x {KN} neighbours, cosine: {fmt(got)}", flush=True)
        res["runs"].append({"route": "fit", "us": got})
        lg.check_index_status(dev)
        print(json.dumps(res))
        return 0

    knn = lg.ItemKNN.fit(lists, KN)
    sptr, sitems = lists.seen.ptr, lists.seen.items
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    filled = knn.index >= 0
    rows = torch.arange(ni, device=dev)[:, None].expand_as(knn.index)[filled]
    table_t = torch.sparse_coo_tensor(torch.stack([knn.index[filled], rows]), knn.value[filled], (ni, ni)).coalesce()   # S^T

    def outputs(n, band):
        ws_bytes = lib.lgc_knn_workspace_bytes(n, ni, k, band, stream)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
        return (torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev),
                torch.empty((n, k), dtype=torch.int32, device=dev), ws, ws_bytes)

    def fused(users, band, index, value, votes, ws, ws_bytes):
        _native.check(lib.lgc_knn_recommend(knn.index.data_ptr(), knn.value.data_ptr(), KN, ni, KN, sptr.data_ptr(),
                                            sitems.data_ptr(), None, nu, users.data_ptr(), users.numel(), None, 1, 1, k, band,
                                            index.data_ptr(), value.data_ptr(), votes.data_ptr(), _native.ptr(ws), ws_bytes,
                                            status.data_ptr(), stream), "lgc_knn_recommend")

    def composed(users, rows_per_chunk=512):
        out = []
        for lo in range(0, users.numel(), rows_per_chunk):
            u = users[lo:lo + rows_per_chunk]
            cnt = sptr[u + 1] - sptr[u]
            row = torch.repeat_interleave(torch.arange(u.numel(), device=dev), cnt)
            first = torch.cumsum(cnt, 0) - cnt
            item = sitems[torch.arange(row.numel(), device=dev) - first[row] + sptr[u][row]]
            dense = torch.zeros((ni, u.numel()), dtype=torch.float32, device=dev)
            dense[item, row] = 1.0
            panel = torch.sparse.mm(table_t, dense).t().contiguous()
            panel = torch.where(panel > 0, panel, torch.full_like(panel, float("-inf")))
            panel[row, item] = float("-inf")
            out.append(propagate.mask_topk(panel, None, k))
        return torch.cat(out)

    def compare(users, label, bands=(0,)):
        routes = {}
        for band in bands:
            bufs = outputs(users.numel(), band)
            routes[f"band {band}" if len(bands) > 1 else "fused"] = ((lambda b=band, o=bufs: fused(users, b, *o)), 0)
        routes["composed"] = ((lambda: composed(users)), 0 if users.numel() <= 64 else 1)
        got = alternate(routes, args.reps, args.blocks)
        bufs = outputs(users.numel(), 0)
        fused(users, 0, *bufs)
        equal = int((bufs[0] == composed(users)).all(dim=1).sum().item())
        entries = int((sptr[users + 1] - sptr[users]).sum().item())
        base = got["band 0" if len(bands) > 1 else "fused"]
        print(f"{label} ({users.numel()} baskets, {entries} entries): " + "; ".join(f"{name} {fmt(t)}" for name, t in got.items())
              + f"; composed / fused {got['composed'][0] / base[0]:.2f}; {equal} of {users.numel()} rows equal", flush=True)
        res["runs"].append({"what": label, "baskets": users.numel(), "entries": entries, "us": got, "rows_equal": equal})

    rng = np.random.default_rng(SEED)
    length = sptr[1:] - sptr[:-1]
    compare(torch.from_numpy(np.sort(rng.choice(nu, size=10 ** 4, replace=False))).to(dev), "10^4 users", BANDS)
    for n in (1, 8, 64):
        compare(torch.from_numpy(rng.choice(nu, size=n, replace=False)).to(dev), f"{n} session baskets")
    hub = int(torch.argmax(length).item())
    compare(torch.tensor([hub], device=dev), f"the user with the most purchases ({int(length[hub])})")
    lg.check_index_status(dev)
    assert int(status[0].item()) == 0
    print(json.dumps(res))
    return 0


def quality_step(args):
    import numpy as np
    import pandas as pd
    import torch
    import gnn_ecommerce_amd as lg
    import train_demo
    a = train_demo.parse_args([])
    dev = torch.device("cuda:0")
    n_users, n_items = a.users, a.items
    u, i = train_demo.latent_interactions(n_users, n_items, a.per_user, 0)
    held = np.random.default_rng(1).random(len(u)) < 0.15              # train_demo's split
    test = pd.DataFrame({"user_id_idx": u[held], "item_id_idx": i[held]})
    test_pos = test.groupby("user_id_idx")["item_id_idx"].apply(list).reset_index()
    test_pos.columns = ["user_id_idx", "item_id_idx_list"]
    test_pos = test_pos.iloc[:2000]
    u_t, i_t = torch.from_numpy(u[~held]), torch.from_numpy(i[~held] + n_users)
    edge_index = torch.stack((torch.cat([u_t, i_t]), torch.cat([i_t, u_t]))).to(dev)
    edge_weight = torch.ones(edge_index.size(1), device=dev)
    lists = lg.CoPurchase.from_edges(edge_index, n_users, n_items)
    users = list(test_pos["user_id_idx"])
    positives = lg.PositiveLists.from_frame(test_pos, n_users, dev)
    ks = (5, 10, 20)
    res = {"step": "quality", "n_users": n_users, "n_items": n_items, "eval_users": len(users), "ks": ks, "runs": []}

    def report(name, mean):
        print(f"{name}: " + "; ".join(f"{m}@{ks} " + " / ".join(f"{v:.4f}" for v in mean[m])
                                      for m in ("precision", "recall", "ndcg", "hit_rate", "coverage")), flush=True)
        res["runs"].append({"route": name, **{m: list(v) for m, v in mean.items()}})

    for measure in ("cosine", "count"):
        report(f"ItemKNN ({measure}, kn {KN})", lg.ItemKNN.fit(lists, KN, measure).evaluate(users, positives, ks).mean)
    model = lg.LightGCN(n_users + n_items, a.dim, a.layers).to(dev)
    opt = torch.optim.Adam(model.parameters(), 0.005)
    sampler = lg.TripleSampler.from_pairs(n_users, n_items, u[~held], i[~held] + n_users, u[~held], i[~held] + n_users, dev, seed=0)
    n_batch = max(1, int((~held).sum()) // (a.batch * 40))
    for epoch in range(a.epochs + 1):
        if epoch:
            model.train()
            for _ in range(n_batch):                                   # train_demo's default loop: BPR, one uniform negative
                opt.zero_grad()
                us, pos, neg = sampler.sample(a.batch)
                out = model(edge_index, torch.stack((torch.cat([us, us]), torch.cat([pos, neg]))), edge_weight)
                size = len(us)
                w = model.embedding.weight
                reg = 0.5 * (w[us].norm().pow(2) + w[pos].norm().pow(2) + w[neg].norm().pow(2)) / size * 1e-4
                (model.recommendation_loss(out[:size], out[size:], 0) * size + reg).backward()
                opt.step()
        model.eval()
        if epoch in (0, a.epochs):
            with torch.no_grad():
                got = model.evaluate_metrics(edge_index, edge_weight, n_users, n_items, lists.seen, users, positives, ks)
            report(f"LightGCN after {epoch} epochs of {n_batch} batches", got.mean)
    sampler.check()
    lg.check_index_status(dev)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--step", choices=["all", *STEPS], default="all")
    ap.add_argument("--gpu-timeout", type=int, default=400)
    args = ap.parse_args()
    if args.step != "all":
        return quality_step(args) if args.step == "quality" else speed_step(args)
    for step in STEPS:                                       # a step that fails or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(args.gpu_timeout), sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--step", step]
        code = subprocess.run(cmd, cwd=ROOT).returncode
        if code != 0:
            print(f"step {step} ended with status {code}")
            return code
    return 0


if __name__ == "__main__":
    sys.exit(main())
