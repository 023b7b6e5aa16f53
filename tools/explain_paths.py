#!/usr/bin/env python3
"""The path analysis at full size: ``LightGCN.recommendation_paths`` for 10^4 users x 20 recommended items on the
bench's cosmetics-scale synthetic graph (1,639,358 users x 54,571 items, 20.3 M entries), and, where networkx imports,
upstream's three searches per pair (has_path, shortest_path_length, shortest_path: src/inference_lightgcn.py:94-111) on a
sample of pairs on the host, extrapolated to the whole job.

    python tools/explain_paths.py [--users 10000 --k 20 --max-len 7 --nx-pairs 20] [--step all|gpu|nx]

The driver opens no GPU: each step is a child process under its own ``timeout``; a step that fails or runs out of time
ends the run (no retries).  The GPU step prints, per batch of 64 users, the levels run, and over all batches the time
of a level by level number (level 1 = first, the last levels = saturated: nearly every row is skipped) and the total;
one JSON line at the end of each step."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0


def sample(n_users_graph, n_users, seed=SEED):
    import numpy as np
    return np.sort(np.random.default_rng(seed).choice(n_users_graph, size=n_users, replace=False)).astype(np.int64)


def gpu_step(args):
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import synth
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    ei, ew = g.coo(dev)
    model = lg.LightGCN(g.num_nodes, args.dim, args.layers).to(dev).eval()
    with torch.no_grad():
        model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, args.dim, SEED, dev))
    users = torch.from_numpy(sample(g.n_users, args.users)).to(dev)
    with torch.no_grad():
        top = model.recommend_topk(ei, ew, g.n_users, g.n_items, None, users, args.k)
    graph = lg.get_graph(ei, ew, g.num_nodes)
    plan = graph.forward_op.plan
    print(f"graph: {g.num_nodes} nodes, {graph.num_edges} entries; row plan: {plan.n_chunks} chunks, {plan.n_multi} "
          f"multi-chunk rows; frontier table {g.num_nodes * 8 / 1e6:.1f} MB, entries {graph.num_edges * 8 / 1e6:.1f} MB", flush=True)
    workspace = (args.max_len + 1) * g.num_nodes * 8
    res = {"users": args.users, "k": args.k, "max_len": args.max_len, "runs": []}
    for run in range(args.runs):                          # the first run also loads the code objects
        trace = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lens, longer, paths = model.recommendation_paths(ei, ew, g.n_users, users, top, max_len=args.max_len,
                                                         workspace_bytes=workspace, trace=trace)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        lg.check_index_status(dev)
        by_level, levels_run, prev = {}, {}, {}
        for batch, level, new, settled, t in trace:
            by_level.setdefault(level, []).append((t - prev.get(batch, 0.0)) * 1e3)
            prev[batch], levels_run[batch] = t, level
        med = {lv: statistics.median(ts) for lv, ts in sorted(by_level.items())}
        last = max(med)
        hist = torch.bincount((lens.flatten() + 2).long()).tolist()
        out = {"total_ms": total * 1e3, "batches": len(levels_run), "levels_run_max": max(levels_run.values()),
               "levels_run_median": statistics.median(levels_run.values()), "level_ms_median": med,
               "first_level_ms": med.get(1), "saturated_level_ms": med[last],
               "dist_histogram_from_minus_2": hist, "longer_than_3_users": int(longer.sum()),
               "new_nodes_batch0": [new for b, _, new, _, _ in trace if b == 0]}
        res["runs"].append(out)
        print(f"run {run}: {args.users} users x {args.k} items in {total * 1e3:.1f} ms; {len(levels_run)} batches, levels run "
              f"(beyond level 0) max {out['levels_run_max']}, median {out['levels_run_median']}; ms per level (median over "
              f"batches): " + ", ".join(f"L{lv} {ms:.3f}" for lv, ms in med.items()), flush=True)
        print(f"       distances (-2, -1, 0, 1, ...): {hist}; users with an item beyond 3 hops: {out['longer_than_3_users']}; "
              f"nodes newly reached per level, batch 0: {out['new_nodes_batch0']}", flush=True)
    print(json.dumps(res))
    return 0


def nx_step(args):
    try:
        import networkx as nx
    except ImportError:
        print("networkx is not installed: no host sample")
        return 0
    import numpy as np
    from networkx import has_path, shortest_path, shortest_path_length
    from gnn_ecommerce_amd import synth
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    t0 = time.perf_counter()
    graph = nx.Graph()
    graph.add_edges_from(zip(g.user.tolist(), (g.item + g.n_users).tolist()))     # create_store_nx_graph's graph
    build = time.perf_counter() - t0
    rng = np.random.default_rng(SEED + 1)
    users = rng.choice(sample(g.n_users, args.users), size=args.nx_pairs)
    items = rng.integers(g.n_items, size=args.nx_pairs) + g.n_users               # random items: no scores on the host
    times = []
    for u, i in zip(users.tolist(), items.tolist()):
        t0 = time.perf_counter()
        if has_path(graph, u, i):
            shortest_path_length(graph, u, i)
            shortest_path(graph, u, i)
        times.append(time.perf_counter() - t0)
    per_pair = statistics.mean(times)
    n_pairs = args.users * args.k
    res = {"nx_graph_build_s": build, "nx_pairs": args.nx_pairs, "nx_s_per_pair_mean": per_pair,
           "nx_s_per_pair_median": statistics.median(times), "nx_extrapolated_s": per_pair * n_pairs, "pairs": n_pairs}
    print(f"networkx: graph built in {build:.0f} s; {args.nx_pairs} sampled pairs, {per_pair * 1e3:.2f} ms per pair (mean; "
          f"median {statistics.median(times) * 1e3:.2f} ms) -> EXTRAPOLATED to {n_pairs} pairs: {per_pair * n_pairs:.0f} s", flush=True)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10000); ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=7); ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--dim", type=int, default=64); ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--nx-pairs", type=int, default=20)
    ap.add_argument("--step", choices=["all", "gpu", "nx"], default="all")
    ap.add_argument("--gpu-timeout", type=int, default=420); ap.add_argument("--nx-timeout", type=int, default=1800)
    args = ap.parse_args()
    if args.step == "gpu":
        return gpu_step(args)
    if args.step == "nx":
        return nx_step(args)
    passed = [a for a in sys.argv[1:]]
    for step, limit in (("gpu", args.gpu_timeout), ("nx", args.nx_timeout)):
        if step == "nx" and args.nx_pairs <= 0:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", step]
        code = subprocess.run(cmd, cwd=ROOT).returncode
        if code != 0:
            print(f"step {step} ended with status {code}: stopping")
            return code
    return 0


if __name__ == "__main__":
    sys.exit(main())
