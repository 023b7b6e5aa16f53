#!/usr/bin/env python3
"""Full-rank evaluation at full size: ``lgc_rank_positions`` (HIP events around the call: thresholds, sweep and seen
correction) for 10,000 validation users of the bench's cosmetics-scale synthetic graph (54,571 items), one to two held-out
items each, the users' training purchases as seen lists, mode "zero" -- at D = 64 / K = 3 and D = 90 / K = 5 -- beside the
composed route the library had before: ``lgc_score_rows`` panels of ``panel_rows`` rows, the seen entries multiplied by 0,
the comparison with the same tie rule (greater, or equal and a smaller index) and the row sums in torch.  The two routes
alternate in one process; the time is the median of ``--reps`` after warm-ups.  Reports the fp32 rate 2 n N D / t, the bytes
each route moves at the least (fused: the item table once per tile of 64 pairs, the user rows and 16 bytes a pair;
composed: the score panel written once and read once -- the boolean temporaries of the comparison come on top) and whether
all ranks are equal.

    python tools/full_rank.py [--configs 64:3 90:5 --users 10000 --reps 10]

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


def alternating_us(fns, reps, warmup=2):
    """Per function the median over ``reps`` of the HIP-event time around one call (microseconds); the functions take
    turns, so that neither has the device to itself for a stretch the other does not get."""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in times]


def gpu_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, propagate, synth
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    ei, ew = g.coo(dev)
    nu, ni = g.n_users, g.n_items
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(SEED)
    # the seen lists: every user's training purchases, ascending
    fwd = ei[0] < nu
    key = torch.unique(ei[0][fwd] * ni + (ei[1][fwd] - nu))
    seen_items = (key % ni).contiguous()
    seen_ptr = torch.zeros(nu + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(key // ni, minlength=nu), 0, out=seen_ptr[1:])
    # the pairs: one or two held-out items for each of the validation users
    users = np.sort(rng.choice(nu, size=min(args.users, nu), replace=False)).astype(np.int64)
    counts = rng.integers(1, 3, size=users.size)
    pu_np = np.repeat(users, counts)
    pu = torch.from_numpy(pu_np).to(dev)
    pi = torch.from_numpy(rng.integers(0, ni, size=pu_np.size).astype(np.int64)).to(dev)
    n = pu.numel()
    # the seen entries of every pair's user as (pair row, item), for the composed route's multiply
    lens = (seen_ptr[pu + 1] - seen_ptr[pu])
    row_of = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    start = torch.cumsum(lens, 0) - lens
    col_of = seen_items[seen_ptr[pu][row_of] + torch.arange(row_of.numel(), device=dev) - start[row_of]]
    rows = min(n, propagate.panel_rows(ni))
    bounds = torch.searchsorted(row_of, torch.arange(0, n + rows, rows, device=dev)).tolist()
    cols = torch.arange(ni, device=dev)[None, :]
    res = {"n_items": ni, "users": int(users.size), "pairs": n, "seen_entries": int(row_of.numel()), "runs": []}
    print(f"{ni} items, {users.size} users, {n} pairs, {row_of.numel()} seen entries; composed route in panels of {rows} rows", flush=True)
    print("  D | K | slices | fused us | TF/s | fused MB | workspace KB | composed us | composed MB | ratio | same", flush=True)
    for dim, layers in args.configs:
        model = lg.LightGCN(g.num_nodes, dim, layers).to(dev).eval()
        with torch.no_grad():
            model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, dim, SEED, dev))
            table = model._serving_embedding(ei, ew).detach()
        user_t, item_t = table[:nu], table[nu:]
        ws_bytes = lib.lgc_rank_positions_workspace_bytes(n, ni, 0)
        ws = torch.empty(max(1, (ws_bytes + 7) // 8), dtype=torch.int64, device=dev)
        rank = torch.empty(n, dtype=torch.int32, device=dev)
        composed_rank = torch.empty(n, dtype=torch.int64, device=dev)
        scores = torch.empty((rows, ni), dtype=torch.float32, device=dev)

        def fused():
            _native.check(lib.lgc_rank_positions(user_t.data_ptr(), user_t.stride(0), nu, item_t.data_ptr(), item_t.stride(0), ni,
                                                 dim, pu.data_ptr(), pi.data_ptr(), n, seen_ptr.data_ptr(), seen_items.data_ptr(), 0,
                                                 0, rank.data_ptr(), None, None, None, ws.data_ptr(), ws_bytes, status.data_ptr(),
                                                 stream), "lgc_rank_positions")

        def composed():
            for j, lo in enumerate(range(0, n, rows)):
                hi = min(n, lo + rows)
                part = scores[:hi - lo]
                propagate.score_rows(user_t, pu[lo:hi], item_t, part)
                r, c = row_of[bounds[j]:bounds[j + 1]] - lo, col_of[bounds[j]:bounds[j + 1]]
                part[r, c] = part[r, c] * 0.0                                   # a seen item competes as score * 0
                p = pi[lo:hi, None]
                t = part.gather(1, p)
                composed_rank[lo:hi] = ((part > t) | ((part == t) & (cols < p))).sum(1)   # no NaN in these tables

        reps = args.reps
        t_fused, t_composed = alternating_us((fused, composed), reps)
        same = bool(torch.equal(rank.to(torch.int64), composed_rank))
        tf = 2.0 * n * ni * dim / (t_fused * 1e-6) / 1e12
        row_tiles, item_tiles = -(-n // 64), -(-ni // 128)
        slices = max(1, min(-(-512 // row_tiles), 64, item_tiles))
        fused_mb = (row_tiles * ni * dim * 4 + slices * n * dim * 4 + 16 * n) / 2 ** 20
        composed_mb = 2.0 * n * ni * 4 / 2 ** 20
        run = {"dim": dim, "layers": layers, "slices": slices, "fused_us": t_fused, "tf_per_s": tf, "fused_mb": fused_mb,
               "workspace_bytes": ws_bytes, "composed_us": t_composed, "composed_mb": composed_mb, "ratio": t_composed / t_fused,
               "same_ranks": same}
        res["runs"].append(run)
        print(f"{dim:3d} | {layers} | {slices:6d} | {t_fused:8.1f} | {tf:4.1f} | {fused_mb:8.1f} | {ws_bytes / 1024:12.1f} | "
              f"{t_composed:11.1f} | {composed_mb:11.1f} | {t_composed / t_fused:5.1f} | {same}", flush=True)
    lg.check_index_status(dev)
    assert int(status[0].item()) == 0
    print(json.dumps(res))
    return 0


def config(text):
    dim, layers = text.split(":")
    return int(dim), int(layers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=config, nargs="+", default=[(64, 3), (90, 5)], metavar="D:K")
    ap.add_argument("--users", type=int, default=10000); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", choices=["all", "gpu"], default="all")
    ap.add_argument("--gpu-timeout", type=int, default=420)
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
