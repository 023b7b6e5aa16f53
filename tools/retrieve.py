#!/usr/bin/env python3
"""Cross-table retrieval at full size: ``lgc_retrieve_topk`` (HIP events around the call: the fused kernel, and the merge
where the candidate table is cut into ranges) on the tables of the bench's cosmetics-scale synthetic graph, at D = 64 and 90.

  recommend  10^4 users x 54,571 items, k = 20, the users' lists of the graph removed and a 90 % in-stock mask -- beside the
             composed route of ``recommend_topk`` (``lgc_score_rows`` panels + ``lgc_mask_topk`` with the same lists, which
             ZEROES a listed item's score and knows no stock mask: the two routes do different things, the comparison is of
             cost only).
  audience   1, 8 and 64 items over all users, their buyers removed -- beside the time one pass over the user table takes
             from HBM at 8 TB/s, below which such a request cannot go.

Protocol: one process per step, both routes warmed up, then alternating blocks of ``--reps`` calls each, a HIP-event pair
around every call; the median over all calls of a route and its range (min .. max).  No speed is promised.

    python tools/retrieve.py [--dims 64 90 --layers 3 --k 20 --reps 5 --blocks 3]

The driver opens no GPU: every step is a child process under its own ``timeout``; one JSON line per step at its end."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0
HBM_TB = 8.0
STEPS = ("recommend", "audience")


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(routes, reps, blocks, warmup=2):
    """{name: (median us, min us, max us)} of the routes (name -> callable), timed in alternating blocks."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            times[name] += [timed(fn) for _ in range(reps)]
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def csr(rows, cols, n_rows, n_cols, dev):
    """The distinct (row, col) pairs as a device CSR, columns ascending."""
    import numpy as np
    import torch
    key = np.unique(rows.astype(np.int64) * n_cols + cols.astype(np.int64))
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_cols, minlength=n_rows), out=ptr[1:])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(key % n_cols).to(dev)


def gpu_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, propagate, synth
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    ei, ew = g.coo(dev)
    nu, ni, k = g.n_users, g.n_items, args.k
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(SEED)
    res = {"step": args.step, "k": k, "layers": args.layers, "n_users": nu, "n_items": ni, "runs": []}

    def call(q_t, c_t, ids, ok, lists, index, value, ws, ws_bytes):
        _native.check(lib.lgc_retrieve_topk(q_t.data_ptr(), q_t.stride(0), q_t.size(0), c_t.data_ptr(), c_t.stride(0), c_t.size(0),
                                            q_t.size(1), ids.data_ptr(), ids.numel(), None, None, _native.ptr(ok),
                                            lists[0].data_ptr(), lists[1].data_ptr(), None, lists[0].numel() - 1, None, k, 0,
                                            index.data_ptr(), value.data_ptr(), ws.data_ptr(), ws_bytes, status.data_ptr(), stream),
                      "lgc_retrieve_topk")

    def slices_chosen(n, n_cand):
        return max(1, min(-(-512 // -(-n // 64)), 1024, -(-n_cand // 128)))

    for dim in args.dims:
        model = lg.LightGCN(g.num_nodes, dim, args.layers).to(dev).eval()
        with torch.no_grad():
            model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, dim, SEED, dev))
            user_t, item_t = torch.split(model._serving_embedding(ei, ew).detach(), [nu, ni])
        if args.step == "recommend":
            n = min(args.users, nu)
            seen = lg.SeenLists(*csr(g.user, g.item, nu, ni, dev))
            ids = torch.from_numpy(np.sort(rng.choice(nu, size=n, replace=False)).astype(np.int64)).to(dev)
            ok = torch.from_numpy((rng.random(ni) < 0.9).astype(np.uint8)).to(dev)
            ws_bytes = lib.lgc_retrieve_workspace_bytes(n, ni, k, 0)
            ws = torch.empty(max(1, (ws_bytes + 7) // 8), dtype=torch.int64, device=dev)
            index = torch.empty((n, k), dtype=torch.int64, device=dev)
            value = torch.empty((n, k), dtype=torch.float32, device=dev)
            got = alternate({"fused": lambda: call(user_t, item_t, ids, ok, (seen.ptr, seen.items), index, value, ws, ws_bytes),
                             "composed": lambda: propagate.recommend_topk(user_t, ids, item_t, seen, k)}, args.reps, args.blocks)
            # with every item in stock the fused answer must be the composed one wherever no seen item reached the top k
            call(user_t, item_t, ids, None, (seen.ptr, seen.items), index, value, ws, ws_bytes)
            composed = propagate.recommend_topk(user_t, ids, item_t, seen, k)
            rows_equal = int((index == composed).all(dim=1).sum().item())
            f, c = got["fused"], got["composed"]
            tf = 2.0 * n * ni * dim / (f[0] * 1e-6) / 1e12
            run = {"dim": dim, "queries": n, "slices": slices_chosen(n, ni), "fused_us": f, "composed_us": c, "tf_per_s": tf,
                   "ratio": c[0] / f[0], "workspace_bytes": ws_bytes, "rows_equal_without_stock_mask": rows_equal}
            print(f"D {dim:3d}: {n} users x {ni} items, {run['slices']} ranges: fused {f[0]:.1f} us ({f[1]:.1f} .. {f[2]:.1f}), "
                  f"{tf:.1f} TF/s; composed {c[0]:.1f} us ({c[1]:.1f} .. {c[2]:.1f}); composed / fused {c[0] / f[0]:.2f}; "
                  f"{rows_equal} of {n} rows equal without the stock mask", flush=True)
            res["runs"].append(run)
        else:
            buyers = csr(g.item, g.user, ni, nu, dev)
            floor_us = nu * dim * 4 / (HBM_TB * 1e12) * 1e6
            for n in (1, 8, 64):
                ids = torch.from_numpy(np.sort(rng.choice(ni, size=n, replace=False)).astype(np.int64)).to(dev)
                ws_bytes = lib.lgc_retrieve_workspace_bytes(n, nu, k, 0)
                ws = torch.empty(max(1, (ws_bytes + 7) // 8), dtype=torch.int64, device=dev)
                index = torch.empty((n, k), dtype=torch.int64, device=dev)
                value = torch.empty((n, k), dtype=torch.float32, device=dev)
                f = alternate({"fused": lambda: call(item_t, user_t, ids, None, buyers, index, value, ws, ws_bytes)},
                              args.reps, args.blocks)["fused"]
                assert int((index >= 0).all().item())
                run = {"dim": dim, "queries": n, "slices": slices_chosen(n, nu), "fused_us": f, "hbm_floor_us": floor_us,
                       "tb_per_s": nu * dim * 4 / (f[0] * 1e-6) / 1e12, "workspace_bytes": ws_bytes}
                print(f"D {dim:3d}: audience of {n:2d} items over {nu} users, {run['slices']} ranges: {f[0]:.1f} us "
                      f"({f[1]:.1f} .. {f[2]:.1f}); one pass over the user table at {HBM_TB:.0f} TB/s {floor_us:.1f} us; "
                      f"{run['tb_per_s']:.2f} TB/s of table read", flush=True)
                res["runs"].append(run)
    lg.check_index_status(dev)
    assert int(status[0].item()) == 0
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 90]); ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--k", type=int, default=20); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3); ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--step", choices=["all", *STEPS], default="all")
    ap.add_argument("--gpu-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step != "all":
        return gpu_step(args)
    for step in STEPS:                                       # a step that fails or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(args.gpu_timeout), sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--step", step]
        code = subprocess.run(cmd, cwd=ROOT).returncode
        if code != 0:
            print(f"step {step} ended with status {code}")
            return code
    return 0


if __name__ == "__main__":
    sys.exit(main())
