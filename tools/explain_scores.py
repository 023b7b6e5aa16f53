#!/usr/bin/env python3
"""Score attribution at full size: ``lgc_attribute`` alone (HIP events around the one launch) on the bench's cosmetics-scale
synthetic graph (1,639,358 users x 54,571 items, 20.3 M entries) at 1 / 64 / 1,024 request rows x 20 targets with m = 3, in
both list forms, plus the session form at 64 lists of 5,000 entries; beside each the same-shape ``lgc_fold_in`` launch (its
nearest relative: the same list walk, the same gathers) and the ``lgc_mask_topk`` launch that ranked the rows, as the
yardstick; and ``LightGCN.explain_topk`` for 10^4 users x 20 items end to end (wall clock).

    python tools/explain_scores.py [--dim 64 --layers 3 --k 20 --m 3 --users 10000 --reps 20]

The driver opens no GPU: the measurement is a child process under its own ``timeout``; one JSON line at the end."""
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


def event_us(fn, reps, warmup=3):
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


def gpu_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, propagate, synth
    from gnn_ecommerce_amd.foldin import SessionLists, fold_table
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    ei, ew = g.coo(dev)
    model = lg.LightGCN(g.num_nodes, args.dim, args.layers).to(dev).eval()
    with torch.no_grad():
        model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, args.dim, SEED, dev))
    graph = lg.get_graph(ei, ew, g.num_nodes)
    nu, ni, k, m = g.n_users, g.n_items, args.k, args.m
    with torch.no_grad():
        fold = fold_table(model, graph)
        served = model._serving_embedding(ei, ew).detach()
    item_t, init_t, dis = served[nu:], model.embedding.weight.detach()[:nu], graph.dis[nu:]
    a0 = model._alphas()[0]
    op = graph.forward_op
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(SEED)
    res = {"dim": args.dim, "layers": args.layers, "k": k, "m": m, "rows": {}}

    def attr_call(n_rows, targets, session=None, row_ids=None, init_rows=None):
        a = _native.AttrArgsC()
        if session is not None:
            a.list_ptr, a.list_items, a.item_dis, a.normalize = session.ptr.data_ptr(), session.items.data_ptr(), dis.data_ptr(), 1
        else:
            a.rowptr, a.entries, a.row_ids = op.rowptr.data_ptr(), op.entries.data_ptr(), row_ids.data_ptr()
            a.n_graph_rows, a.col_base = nu, nu
        a.n_rows, a.fold, a.items, a.fold_stride, a.item_stride, a.n_items = n_rows, fold.data_ptr(), item_t.data_ptr(), fold.stride(0), item_t.stride(0), ni
        if init_rows is not None:
            a.init_rows, a.init, a.init_stride, a.n_init_rows = init_rows.data_ptr(), init_t.data_ptr(), init_t.stride(0), nu
        a.a0, a.targets, a.target_stride, a.n_targets, a.top_m, a.dim = a0, targets.data_ptr(), k, k, m, args.dim
        out = [torch.empty((n_rows, k), device=dev), torch.empty((n_rows, k), device=dev),
               torch.empty((n_rows, k, m), dtype=torch.int32, device=dev), torch.empty((n_rows, k, m), dtype=torch.int64, device=dev),
               torch.empty((n_rows, k, m), device=dev)]
        a.base, a.total, a.top_pos, a.top_item, a.top_value = (t.data_ptr() for t in out)
        a.status = status.data_ptr()

        def fn():
            _native.check(lib.lgc_attribute(a, stream), "lgc_attribute")
        fn.keep = (a, out, targets, session, row_ids, init_rows)
        return fn

    def fold_call(session, init_rows):
        n_rows = session.n_rows
        out = torch.empty((n_rows, args.dim), device=dev)

        def fn():
            _native.check(lib.lgc_fold_in(session.ptr.data_ptr(), session.items.data_ptr(), None, n_rows, dis.data_ptr(), fold.data_ptr(),
                                          fold.stride(0), ni, _native.ptr(init_rows), _native.ptr(init_t) if init_rows is not None else None,
                                          init_t.stride(0) if init_rows is not None else 0, nu if init_rows is not None else 0, a0, 1,
                                          args.dim, out.data_ptr(), args.dim, status.data_ptr(), stream), "lgc_fold_in")
        return fn

    def own_sessions(users):
        lo, hi = op.rowptr[users].long(), op.rowptr[users + 1].long()
        counts = hi - lo
        ptr = torch.zeros(users.numel() + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(counts, 0)
        pos = torch.arange(int(ptr[-1]), device=dev) - torch.repeat_interleave(ptr[:-1] - lo, counts)
        return SessionLists(ptr, (op.entries[pos, 0].long() - nu).contiguous())

    print(f"graph {nu} users x {ni} items, {graph.num_edges} entries; D = {args.dim}, K = {args.layers}, {k} targets, m = {m}", flush=True)
    print("rows | lists           | entries | lgc_attribute us | lgc_fold_in us | lgc_mask_topk us", flush=True)
    for n_rows in (1, 64, 1024):
        users = torch.from_numpy(np.sort(rng.choice(nu, size=n_rows, replace=False)).astype(np.int64)).to(dev)
        with torch.no_grad():
            scores = propagate.score_rows(served[:nu], users, item_t)
            top = propagate.mask_topk(scores, None, k)
        sess = own_sessions(users)
        t_topk = event_us(lambda: propagate.mask_topk(scores, None, k), args.reps)
        t_fold = event_us(fold_call(sess, users), args.reps)
        t_graph = event_us(attr_call(n_rows, top, row_ids=users, init_rows=users), args.reps)
        t_sess = event_us(attr_call(n_rows, top, session=sess, init_rows=users), args.reps)
        entries = int(sess.items.numel())
        res["rows"][n_rows] = {"entries": entries, "attribute_graph_us": t_graph, "attribute_session_us": t_sess,
                               "fold_in_us": t_fold, "mask_topk_us": t_topk}
        print(f"{n_rows:4d} | graph (own rows) | {entries:7d} | {t_graph:16.1f} | {t_fold:14.1f} | {t_topk:16.1f}", flush=True)
        print(f"{n_rows:4d} | session (same)   | {entries:7d} | {t_sess:16.1f} | {t_fold:14.1f} | {t_topk:16.1f}", flush=True)
    # long lists: 64 sessions of 5,000 entries
    n_rows, length = 64, 5000
    ptr = torch.arange(n_rows + 1, dtype=torch.int64, device=dev) * length
    long = SessionLists(ptr, torch.from_numpy(rng.integers(ni, size=n_rows * length)).to(dev))
    with torch.no_grad():
        rows = lg.fold_in(fold, dis, long)
        scores = propagate.score_rows(rows, None, item_t)
        top = propagate.mask_topk(scores, None, k)
    t_topk = event_us(lambda: propagate.mask_topk(scores, None, k), args.reps)
    t_fold = event_us(fold_call(long, None), args.reps)
    t_sess = event_us(attr_call(n_rows, top, session=long), args.reps)
    res["long_lists"] = {"rows": n_rows, "entries": n_rows * length, "attribute_session_us": t_sess, "fold_in_us": t_fold, "mask_topk_us": t_topk}
    print(f"{n_rows:4d} | session 5,000    | {n_rows * length:7d} | {t_sess:16.1f} | {t_fold:14.1f} | {t_topk:16.1f}", flush=True)
    # end to end through the model
    users = torch.from_numpy(np.sort(rng.choice(nu, size=args.users, replace=False)).astype(np.int64)).to(dev)
    with torch.no_grad():
        top = model.recommend_topk(ei, ew, nu, ni, None, users, k)
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = model.explain_topk(ei, ew, nu, ni, users, top, m=m)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    lg.check_index_status(dev)
    assert int(status[0].item()) == 0
    res["explain_topk"] = {"users": args.users, "k": k, "ms": times, "explained": int((got.top_item[:, :, 0] >= 0).sum())}
    print(f"explain_topk: {args.users} users x {k} items end to end: " + ", ".join(f"{t:.2f}" for t in times) + " ms (first call, then repeats)", flush=True)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=64); ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--k", type=int, default=20); ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--users", type=int, default=10000); ap.add_argument("--reps", type=int, default=20)
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
