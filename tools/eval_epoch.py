#!/usr/bin/env python3
"""An epoch's evaluation at full size: ``LightGCN.evaluateK`` against the route the parent commit offers for the same
job -- ``recommendK`` with ``SeenLists`` in chunks small enough to fit, the frames concatenated, then ``MARK_MAPK``
(TrainLightGCN.test, src/train_lightgcn.py:155-162).  10^4 validation users x 54,571 items, D = 90 (internal stride 96),
k = 20, synthetic tables.

The parent's route runs on the PARENT's code: check the parent commit out beside the tree and build it,

    mkdir -p ab_libs/parent && git archive HEAD~1 gnn-ecommerce_amd include | tar -x -C ab_libs/parent
    make -C ab_libs/parent/gnn-ecommerce_amd/csrc
    python tools/eval_epoch.py [--parent ab_libs/parent] [--users 10000 --items 54571 --dim 90 --k 20 --pairs 5]

Both packages live in this one process (the parent's under another name, with its own library), so the runs interleave:
first an A/A of the parent's route against itself -- the spread of those times is the noise margin -- then pairs
parent / evaluateK.  PASS when the median of evaluateK is no larger than the parent's median plus the margin.  Also
printed: torch.cuda.max_memory_allocated of each route, evaluateK at several workspace sizes, and lgc_score_rows
against the rocBLAS product of the same panel.  One JSON line at the end.

A second leg times ``evaluate_metrics(ks=(5, 10, 20))`` -- seven metrics at three cutoffs from one ranking pass -- beside
``evaluateK(k=20)`` on the same model: ``--pairs`` interleaved runs of each, the best of each printed with their
difference.  ``--parent ""`` skips the legs that need the parent checkout and runs this one alone."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pandas as pd
import torch

import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd.propagate import PositiveLists, SeenLists, panel_rows, score_rows


def load_parent(tree):
    """The parent checkout's package under the name ``lgcn_parent`` (its relative imports and its own .so)."""
    pkg = os.path.join(os.path.abspath(tree), "gnn-ecommerce_amd")
    if not os.path.isfile(os.path.join(pkg, "csrc", "liblgconv_hip.so")):
        sys.exit(f"{pkg}/csrc/liblgconv_hip.so not found: check the parent out there and build it (see the module docstring)")
    spec = importlib.util.spec_from_file_location("lgcn_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lgcn_parent"] = mod
    spec.loader.exec_module(mod)
    assert not hasattr(mod.LightGCN, "evaluateK"), "the parent checkout already has evaluateK: not the parent"
    return mod


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated(), out


def parent_legs(args, res, k, got, parent_route, new_route):
    """The A/A of the parent's route, then interleaved pairs parent / evaluateK; fills ``res``."""
    _, _, want = timed(parent_route)                      # warm
    res["parent_metrics"] = want
    print(f"parent P@{k} {want[0]:.6f} R@{k} {want[1]:.6f} | evaluateK P@{k} {got[0]:.6f} R@{k} {got[1]:.6f}", flush=True)
    aa = [[], []]
    for _ in range(args.pairs):                           # A/A: the parent's route against itself
        for side in (0, 1):
            aa[side].append(timed(parent_route)[0])
    margin = max(abs(statistics.median(aa[0]) - statistics.median(aa[1])), max(aa[0] + aa[1]) - min(aa[0] + aa[1]))
    res["aa_ms"], res["margin_ms"] = aa, margin
    print(f"A/A parent ms: {[round(t) for t in aa[0]]} / {[round(t) for t in aa[1]]} -> margin {margin:.1f} ms", flush=True)
    t_parent, t_new, mem_parent, mem_new = [], [], 0, 0
    for _ in range(args.pairs):                           # interleaved pairs
        t, mem, _ = timed(parent_route); t_parent.append(t); mem_parent = max(mem_parent, mem)
        t, mem, _ = timed(new_route); t_new.append(t); mem_new = max(mem_new, mem)
    res.update(parent_ms=t_parent, new_ms=t_new, parent_max_memory=mem_parent, new_max_memory=mem_new)
    med_p, med_n = statistics.median(t_parent), statistics.median(t_new)
    res["pass"] = med_n <= med_p + margin
    print(f"parent route median {med_p:.1f} ms (max memory {mem_parent / 2**20:.0f} MiB) | evaluateK median {med_n:.1f} ms "
          f"(max memory {mem_new / 2**20:.0f} MiB) | margin {margin:.1f} ms -> {'PASS' if res['pass'] else 'FAIL'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab_libs", "parent"))
    ap.add_argument("--users", type=int, default=10000); ap.add_argument("--items", type=int, default=54571)
    ap.add_argument("--dim", type=int, default=90); ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--k", type=int, default=20); ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2048, help="users per recommendK call of the parent's route")
    ap.add_argument("--workspace-mib", type=int, nargs="*", default=[16, 64, 256])
    args = ap.parse_args()
    parent = load_parent(args.parent) if args.parent else None
    dev = torch.device("cuda:0")
    n_users, n_items, k = args.users, args.items, args.k
    gen = torch.Generator().manual_seed(0)
    eu, ei_ = torch.randint(n_users, (400000,), generator=gen), torch.randint(n_items, (400000,), generator=gen) + n_users
    edge_index = torch.stack((torch.cat([eu, ei_]), torch.cat([ei_, eu]))).to(dev)
    weight = 0.1 * torch.randn(n_users + n_items, args.dim, generator=gen)
    models = {}
    for name, pkg in (("parent", parent), ("new", lg)):
        if pkg is None:
            continue
        m = pkg.LightGCN(n_users + n_items, args.dim, args.layers).to(dev).eval()
        with torch.no_grad():
            m.embedding.weight.copy_(weight)
        models[name] = m
    # every user is a validation user: 30 seen items, 1..20 positives
    users = torch.randperm(n_users, generator=gen).tolist()
    seen_items = torch.randint(n_items, (n_users, 30), generator=gen).sort(dim=1).values
    ptr = (torch.arange(n_users + 1) * 30).to(dev)
    pos_lists = [torch.randint(n_items, (int(c),), generator=gen).tolist() for c in torch.randint(1, 21, (n_users,), generator=gen)]
    pos_df = pd.DataFrame({"user_id_idx": users, "item_id_idx_list": [pos_lists[u] for u in users]})
    positives = PositiveLists.from_frame(pos_df, n_users, device=dev).validate(n_users, n_items)
    seen_new = SeenLists(ptr, seen_items.reshape(-1).to(dev)).validate(n_users)
    seen_parent = parent.propagate.SeenLists(ptr, seen_items.reshape(-1).to(dev)).validate(n_users) if parent else None
    users_dev = torch.tensor(users, device=dev)

    def parent_route():
        m = models["parent"]
        with torch.no_grad():
            frames = [m.recommendK(edge_index, None, n_users, n_items, seen_parent, users[lo:lo + args.chunk], k)
                      for lo in range(0, len(users), args.chunk)]
            p, r, _ = m.MARK_MAPK(pos_df, pd.concat(frames, ignore_index=True), k)
        return float(p), float(r)

    def new_route(ws=None):
        with torch.no_grad():
            kw = {} if ws is None else {"workspace_bytes": ws}
            p, r, _ = models["new"].evaluateK(edge_index, None, n_users, n_items, seen_new, users_dev, positives, k, **kw)
        return p, r

    def metrics_route():
        with torch.no_grad():
            return models["new"].evaluate_metrics(edge_index, None, n_users, n_items, seen_new, users_dev, positives, ks=(5, 10, 20))

    res = {"users": len(users), "items": n_items, "dim": args.dim, "k": k, "chunk": args.chunk, "pass": True}
    _, _, got = timed(new_route)                          # warm: graph, propagated table, workspace
    res["new_metrics"] = got
    if parent is not None:
        parent_legs(args, res, k, got, parent_route, new_route)
    # evaluateK(k) against evaluate_metrics(ks=(5, 10, 20)): one ranking pass each, interleaved, the best of each
    _, _, full = timed(metrics_route)
    if k == 20:                                           # the same ranking: the same two floats
        assert full.mean["precision"][-1] == got[0] and full.mean["recall"][-1] == got[1]
    t_k, t_m = [], []
    for _ in range(args.pairs):
        t_k.append(timed(new_route)[0])
        t_m.append(timed(metrics_route)[0])
    res.update(evaluatek_ms=t_k, evaluate_metrics_ms=t_m, metrics_mean={name: list(v) for name, v in full.mean.items()})
    print(f"evaluateK(k={k}) best {min(t_k):.2f} ms of {[round(t, 2) for t in t_k]} | evaluate_metrics(ks=(5, 10, 20)) best "
          f"{min(t_m):.2f} ms of {[round(t, 2) for t in t_m]} | excess {min(t_m) - min(t_k):.2f} ms", flush=True)
    for name, v in full.mean.items():
        print(f"    {name:>9} @5 / @10 / @20: " + " / ".join(f"{x:.6f}" for x in v), flush=True)
    # workspace sizes, interleaved (each size keeps its own panel: the cached one is dropped between sizes)
    ws_times = {mib: [] for mib in args.workspace_mib}
    for r in range(args.pairs + 1):
        for mib in args.workspace_mib:
            lg.propagate._score_workspaces.clear()
            t = timed(lambda: new_route(mib << 20))[0]
            if r:
                ws_times[mib].append(t)
    res["workspace_ms"] = {str(mib): t for mib, t in ws_times.items()}
    for mib, t in ws_times.items():
        print(f"workspace {mib:4d} MiB ({panel_rows(n_items, mib << 20)} rows per panel): evaluateK median {statistics.median(t):.1f} ms", flush=True)
    # the score kernel against rocBLAS on one default panel (events; the product includes its row gather, as recommendK's)
    emb = models["new"]._serving_embedding(edge_index, None)
    ut, it = torch.split(emb, [n_users, n_items])
    ids = users_dev[:panel_rows(n_items)]
    out = torch.empty((ids.numel(), n_items), device=dev)
    both = {"lgc_score_rows": lambda: score_rows(ut, ids, it, out=out), "rocblas": lambda: torch.matmul(ut.index_select(0, ids), it.t(), out=out)}
    ev = {name: [] for name in both}
    for r in range(8):
        for name, fn in both.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            if r:
                ev[name].append(s.elapsed_time(e) * 1e3)
    flop = 2.0 * ids.numel() * n_items * args.dim
    res["panel_us"] = {name: statistics.median(t) for name, t in ev.items()}
    for name, t in ev.items():
        print(f"{name:>16}: {ids.numel()} x {n_items} x {args.dim} panel, median {statistics.median(t):.0f} us "
              f"({flop / statistics.median(t) / 1e6:.1f} TFLOP/s)", flush=True)
    print(json.dumps(res))
    return 0 if res["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
