#!/usr/bin/env python3
"""Diversified re-ranking at full size, on the bench's cosmetics-scale synthetic graph: 10^4 users x 100 candidates x
k = 20 at D = 64 / K = 3 and D = 90 / K = 5, cosine, HIP events around each call (median after warm-up):

  * ``lgc_rerank_mmr`` alone, on a ready candidate list;
  * ``recommend_diverse`` end to end beside ``recommend_topk(k = 20)`` -- the expectation to check: a small addition, because
    scoring the users against the catalogue dominates both;
  * the route composed from torch: gather the ``[n, N, D]`` block, ``bmm`` to the ``[n, N, N]`` Gram matrix, a k-step loop of
    torch ops.  Its float order is rocBLAS's, so it may break ties differently: the share of rows on which the two routes
    disagree is reported, not asserted;
  * ``lgc_list_diversity`` at cutoffs (5, 10, 20);
  * the trade-off: recall@20 on held-out purchases (a quarter of each measured user's pairs, left out of the graph) and the
    intra-list diversity @20 at lam = 1, 0.9, 0.7, 0.5.  The model is the untrained Xavier table smoothed by K hops.

    python tools/rerank_diverse.py [--users 10000 --candidates 100 --k 20 --lam 0.7 --reps 10 --config cosmetics]

The driver opens no GPU: the measurement is a child process under its own ``timeout``; one JSON line at the end."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0
CONFIGS = ((64, 3), (90, 5))
LAMS = (1.0, 0.9, 0.7, 0.5)


def event_us(fn, reps, warmup=2):
    """Median over ``reps`` of the HIP-event time around one call of ``fn`` (microseconds)."""
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def composed_mmr(item_t, scale, top, value, k, lam):
    """Greedy MMR from torch ops: the route a caller could compose before lgc_rerank_mmr.  int64 [n, k] positions."""
    import torch
    n, n_cand = top.shape
    block = item_t[top] * scale[top][..., None]                              # [n, N, D], rows normalised
    gram = torch.bmm(block, block.transpose(1, 2))                           # [n, N, N]
    rows = torch.arange(n, device=top.device)
    lrel = lam * value
    pen = torch.zeros_like(value)
    taken = torch.zeros_like(value, dtype=torch.bool)
    out = torch.empty((n, k), dtype=torch.int64, device=top.device)
    for t in range(k):
        obj = lrel if t == 0 else lrel - (1.0 - lam) * pen
        c = torch.where(taken, float("-inf"), obj).argmax(dim=1)
        out[:, t] = c
        taken[rows, c] = True
        col = gram[rows, :, c]
        pen = col if t == 0 else torch.maximum(pen, col)
    return out


def gpu_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, propagate, rerank, similar, synth
    dev = torch.device("cuda:0")
    small = dict(n_users=20000, n_items=2000, n_pairs=400000)
    g = synth.make_bipartite(**(small if args.config == "small" else synth.CONFIG_COSMETICS), seed=SEED)
    nu, ni, k, n_cand, lam = g.n_users, g.n_items, args.k, args.candidates, args.lam
    rng = np.random.default_rng(SEED)
    # the measured users, and a quarter of their pairs held out of the graph
    degree = np.bincount(g.user, minlength=nu)
    users_np = np.sort(rng.choice(np.flatnonzero(degree >= 8), size=args.users, replace=False)).astype(np.int64)
    measured = np.zeros(nu, dtype=bool)
    measured[users_np] = True
    held = measured[g.user] & (rng.random(len(g.user)) < 0.25)
    train = synth.BipartiteGraph(nu, ni, g.user[~held], g.item[~held], g.weight[~held])
    ei, ew = train.coo(dev)
    order = np.argsort(train.user, kind="stable")
    ptr = np.zeros(nu + 1, dtype=np.int64)
    np.cumsum(np.bincount(train.user, minlength=nu), out=ptr[1:])
    seen = propagate.SeenLists(torch.from_numpy(ptr).to(dev), torch.from_numpy(train.item[order]).to(dev)).validate(nu)
    h_order = np.argsort(g.user[held], kind="stable")
    h_ptr = np.zeros(nu + 1, dtype=np.int64)
    np.cumsum(np.bincount(g.user[held], minlength=nu), out=h_ptr[1:])
    users = torch.from_numpy(users_np).to(dev)
    positives = propagate.PositiveLists(torch.from_numpy(h_ptr).to(dev), torch.from_numpy(g.item[held][h_order]).to(dev), users)
    with_pos = torch.from_numpy((h_ptr[users_np + 1] > h_ptr[users_np])).to(dev)
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    n = users.numel()
    res = {"users": n, "candidates": n_cand, "k": k, "lam": lam, "held_out_pairs": int(held.sum()), "runs": []}
    print(f"{n} users x {n_cand} candidates x k = {k}, lam = {lam}, cosine; {ni} items; {int(held.sum())} pairs held out", flush=True)
    for dim, layers in CONFIGS:
        model = lg.LightGCN(g.num_nodes, dim, layers).to(dev).eval()
        with torch.no_grad():
            model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, dim, SEED, dev))
            args_m = (ei, ew, nu, ni, seen, users)
            user_t, item_t, seen_l, ids = model._eval_tables(*args_m)
            scale = similar.row_rnorm(item_t)
            top, value = propagate.recommend_topk(user_t, ids, item_t, seen_l, n_cand, return_values=True)
            index = torch.empty((n, k), dtype=torch.int64, device=dev)
            pos = torch.empty((n, k), dtype=torch.int32, device=dev)

            def mmr_alone():
                _native.check(lib.lgc_rerank_mmr(item_t.data_ptr(), item_t.stride(0), ni, dim, scale.data_ptr(), top.data_ptr(), n_cand,
                                                 value.data_ptr(), n_cand, n, n_cand, k, lam, index.data_ptr(), pos.data_ptr(), None,
                                                 status.data_ptr(), stream), "lgc_rerank_mmr")

            t_mmr = event_us(mmr_alone, args.reps)
            t_topk = event_us(lambda: model.recommend_topk(*args_m, k), args.reps)
            t_cand = event_us(lambda: model.recommend_topk(*args_m, n_cand), args.reps)
            t_div = event_us(lambda: model.recommend_diverse(*args_m, k, n_cand, lam), args.reps)
            t_rnorm = event_us(lambda: similar.row_rnorm(item_t), args.reps)
            composed = [None]

            def run_composed():
                composed[0] = composed_mmr(item_t, scale, top, value, k, lam)

            t_comp = event_us(run_composed, max(2, args.reps // 3), warmup=1)
            differ = float((composed[0] != pos.long()).any(dim=1).float().mean().item())
            composed[0] = None
            torch.cuda.empty_cache()
            cuts = (5, 10, 20) if k >= 20 else (k,)
            t_ild = event_us(lambda: rerank.list_diversity(item_t, index, cuts), args.reps)
            trade = []
            for lm in LAMS:
                lists = model.recommend_diverse(*args_m, k, n_cand, lm)
                _, metrics = propagate.rank_metrics(lists, positives, users, (k,))
                recall = metrics[with_pos, 0, _native.RM_RECALL].reshape(-1, 1).contiguous()
                ild = rerank.list_diversity(item_t, lists, (k,))
                trade.append({"lam": lm, "recall": float(propagate.column_sums(recall).item()) / recall.size(0),
                              "ild": float(propagate.column_sums(ild).item()) / n})
        lg.check_index_status(dev)
        run = {"dim": dim, "layers": layers, "route": rerank.rerank_route(n_cand, dim), "mmr_us": t_mmr, "recommend_topk_k_us": t_topk,
               "recommend_topk_candidates_us": t_cand, "recommend_diverse_us": t_div, "row_rnorm_us": t_rnorm, "composed_us": t_comp,
               "rows_that_differ": differ, "list_diversity_us": t_ild, "trade_off": trade}
        res["runs"].append(run)
        print(f"D = {dim}, K = {layers} ({run['route']} route)", flush=True)
        print(f"  lgc_rerank_mmr alone            {t_mmr:10.1f} us", flush=True)
        print(f"  recommend_topk(k = {k})          {t_topk:10.1f} us", flush=True)
        print(f"  recommend_topk(k = {n_cand})         {t_cand:10.1f} us", flush=True)
        print(f"  recommend_diverse               {t_div:10.1f} us   (+{t_div / t_topk - 1:.1%} over recommend_topk(k = {k}))", flush=True)
        print(f"  lgc_row_rnorm of the catalogue  {t_rnorm:10.1f} us", flush=True)
        print(f"  composed torch route            {t_comp:10.1f} us   ({t_comp / t_mmr:.0f} x lgc_rerank_mmr); rows that differ {differ:.2%}", flush=True)
        print(f"  lgc_list_diversity @ {cuts}  {t_ild:10.1f} us", flush=True)
        for row in trade:
            print(f"  lam {row['lam']:.1f}: recall@{k} {row['recall']:.4f}, ILD@{k} {row['ild']:.4f}", flush=True)
        torch.cuda.empty_cache()
    assert int(status[0].item()) == 0
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10000); ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--k", type=int, default=20); ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--config", choices=["cosmetics", "small"], default="cosmetics")
    ap.add_argument("--step", choices=["all", "gpu"], default="all")
    ap.add_argument("--gpu-timeout", type=int, default=540)
    args = ap.parse_args()
    if args.step == "gpu":
        return gpu_step(args)
    cmd = ["timeout", "-k", "10", str(args.gpu_timeout), sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--step", "gpu"]
    code = subprocess.run(cmd, cwd=ROOT).returncode
    if code != 0:
        print(f"the measurement ended with status {code}")
    return code


if __name__ == "__main__":
    sys.exit(main())
