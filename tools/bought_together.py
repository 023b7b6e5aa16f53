#!/usr/bin/env python3
"""Bought together at full size: ``lgc_cooccur_topk`` (HIP events around the call: the count-score-select kernel, and the merge
where the catalogue is cut into bands) on the purchase lists of the bench's cosmetics-scale synthetic graph, k = 20, cosine.

  catalogue  every item of the catalogue in one call, at bands of 8,192, 16,384 and 32,768 counters and at the library's
             choice (0) -- the figure the auto rule is chosen by -- beside a route composed from torch: index ops that build
             the count rows of a chunk of queries (buyers gathered, their lists gathered, ``index_put_`` with accumulate),
             the formula in fp32 and ``lgc_mask_topk`` over the panel.
  pages      product-page requests of 1, 8 and 64 items, the 64 with the most-bought item among them, both routes; and
             the overlap@20 of the answers with ``similar_items`` over an untrained table, for information only.

Protocol: one process per step, both routes warmed up, then alternating blocks of ``--reps`` calls each, a HIP-event pair
around every call; the median over all calls of a route and its range (min .. max).  No speed is promised.

    python tools/bought_together.py [--k 20 --reps 5 --blocks 3]

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
STEPS = ("catalogue", "pages")
BANDS = (8192, 16384, 32768, 0)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(routes, reps, blocks, warmup=1):
    """{name: (median us, min us, max us)} of the routes (name -> (callable, reps of a block)), timed in alternating blocks."""
    for fn, _ in routes.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in routes}
    for _ in range(blocks):
        for name, (fn, n) in routes.items():
            times[name] += [timed(fn) for _ in range(n or reps)]
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def gpu_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, cooccur, propagate, synth
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    nu, ni, k = g.n_users, g.n_items, args.k
    ei, ew = g.coo(dev)
    lists = cooccur.CoPurchase.from_edges(ei, nu, ni)
    bptr, busers, sptr, sitems = lists.buyers.ptr, lists.buyers.users, lists.seen.ptr, lists.seen.items
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    length = bptr[1:] - bptr[:-1]
    rb = 1.0 / torch.sqrt(length.to(torch.float32))
    deg = (sptr[1:] - sptr[:-1])
    pairs = int((deg * deg).sum().item())                    # LDS adds of a whole-catalogue call, per band pass
    res = {"step": args.step, "k": k, "n_users": nu, "n_items": ni, "entries": int(busers.numel()), "pairs": pairs, "runs": []}

    def fused(ids, n, band, index, value, count, ws, ws_bytes):
        _native.check(lib.lgc_cooccur_topk(bptr.data_ptr(), busers.data_ptr(), ni, sptr.data_ptr(), sitems.data_ptr(), nu,
                                           _native.ptr(ids), n, None, 1, cooccur.MEASURES["cosine"], k, band, index.data_ptr(),
                                           value.data_ptr(), count.data_ptr(), _native.ptr(ws), ws_bytes, status.data_ptr(),
                                           stream), "lgc_cooccur_topk")

    def outputs(n, band):
        ws_bytes = lib.lgc_cooccur_workspace_bytes(n, ni, k, band, stream)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
        return (torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev),
                torch.empty((n, k), dtype=torch.int32, device=dev), ws, ws_bytes)

    def composed_rows(q):
        """int64 [len(q), k] for the query items q (a device tensor): torch index ops, the cosine formula, lgc_mask_topk."""
        n = q.numel()
        cnt = bptr[q + 1] - bptr[q]
        row = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
        first = torch.cumsum(cnt, 0) - cnt
        user = busers[torch.arange(row.numel(), device=dev) - first[row] + bptr[q][row]]
        cnt2 = sptr[user + 1] - sptr[user]
        which = torch.repeat_interleave(torch.arange(user.numel(), device=dev), cnt2)
        first2 = torch.cumsum(cnt2, 0) - cnt2
        item = sitems[torch.arange(which.numel(), device=dev) - first2[which] + sptr[user][which]]
        c = torch.zeros((n, ni), dtype=torch.int32, device=dev)
        c.index_put_((row[which], item), torch.ones(1, dtype=torch.int32, device=dev), accumulate=True)
        s = (c.to(torch.float32) * (1.0 / torch.sqrt(cnt.to(torch.float32)))[:, None]) * rb[None, :]
        s = torch.where(c > 0, s, torch.full_like(s, float("-inf")))
        s[torch.arange(n, device=dev), q] = float("-inf")
        return propagate.mask_topk(s, None, k)

    def composed(ids, rows_per_chunk=512, entries_per_chunk=1 << 20):
        """The composed route over the items ``ids`` in chunks bounded by rows and by buyer entries."""
        out, start, n = [], 0, ids.numel()
        ends = torch.cumsum(bptr[ids + 1] - bptr[ids], 0).cpu().numpy()
        while start < n:
            base = ends[start - 1] if start else 0
            stop = int(np.searchsorted(ends, base + entries_per_chunk, side="right"))
            stop = max(start + 1, min(stop, start + rows_per_chunk, n))
            out.append(composed_rows(ids[start:stop]))
            start = stop
        return torch.cat(out)

    if args.step == "catalogue":
        ids = torch.arange(ni, device=dev)
        routes = {}
        for band in BANDS:
            bufs = outputs(ni, band)
            routes[f"band {band}"] = ((lambda b=band, o=bufs: fused(None, ni, b, *o)), 0)
        routes["composed"] = ((lambda: composed(ids)), 1)
        got = alternate(routes, args.reps, args.blocks)
        bufs = outputs(ni, 0)
        fused(None, ni, 0, *bufs)
        want = composed(ids)
        some = bufs[0] >= 0
        equal = int(((bufs[0] == want) | ~some).all(dim=1).sum().item())
        for name, t in got.items():
            print(f"whole catalogue ({ni} items, {pairs / 1e6:.0f} M count adds a pass), {name}: {t[0] / 1e3:.1f} ms "
                  f"({t[1] / 1e3:.1f} .. {t[2] / 1e3:.1f})", flush=True)
            res["runs"].append({"queries": ni, "route": name, "us": t})
        print(f"{equal} of {ni} rows equal between the routes wherever an item was returned", flush=True)
        res["rows_equal"] = equal
    else:
        rng = np.random.default_rng(SEED)
        hub = int(torch.argmax(length).item())
        dim = 64
        model = lg.LightGCN(g.num_nodes, dim, 3).to(dev).eval()
        with torch.no_grad():
            model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, dim, SEED, dev))
        for n in (1, 8, 64):
            pick = np.sort(rng.choice(ni, size=n, replace=False)).astype(np.int64)
            if n == 64 and hub not in pick:
                pick[0] = hub
            ids = torch.from_numpy(pick).to(dev)
            bufs = outputs(n, 0)
            got = alternate({"fused": ((lambda: fused(ids, n, 0, *bufs)), 0), "composed": ((lambda: composed(ids)), 0)},
                            args.reps, args.blocks)
            fused(ids, n, 0, *bufs)
            want = composed(ids)
            equal = int(((bufs[0] == want) | (bufs[0] < 0)).all(dim=1).sum().item())
            with torch.no_grad():
                sim, _ = model.similar_items(ei, ew, nu, ni, ids, k)
            overlap = float(((bufs[0][:, :, None] == sim[:, None, :]) & (bufs[0][:, :, None] >= 0)).any(dim=2).float().sum(dim=1).mean().item())
            f, c = got["fused"], got["composed"]
            buyers_in = int(length[ids].sum().item())
            print(f"{n:2d} items ({buyers_in} buyers{', the most-bought item among them' if n == 64 else ''}): fused {f[0]:.1f} us "
                  f"({f[1]:.1f} .. {f[2]:.1f}); composed {c[0]:.1f} us ({c[1]:.1f} .. {c[2]:.1f}); composed / fused {c[0] / f[0]:.2f}; "
                  f"{equal} of {n} rows equal; overlap@{k} with similar_items (untrained table) {overlap:.2f}", flush=True)
            res["runs"].append({"queries": n, "buyers": buyers_in, "fused_us": f, "composed_us": c, "ratio": c[0] / f[0],
                                "rows_equal": equal, "overlap_with_similar_items": overlap})
    lg.check_index_status(dev)
    assert int(status[0].item()) == 0
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
