#!/usr/bin/env python3
"""Similar items at full size: ``lgc_item_neighbors`` (HIP events around the call: the fused kernel, and the merge where the
catalogue is cut into ranges) on the item rows of the bench's cosmetics-scale synthetic graph (54,571 items) -- the whole
catalogue at k = 20 and a product-page request of 1, 8 and 64 ids, cosine, at D = 64 and D = 90 -- each beside the composed
route the library had before: ``lgc_score_rows`` panels of ``panel_rows`` rows, the two scalings in torch, ``lgc_mask_topk``
for k + 1 and the item itself dropped.  Reports the time, the fp32 rate 2 n N D / t against the 122 TF/s of an untuned fp32
MFMA GEMM, the workspace, and whether the two routes give the same indices.

    python tools/similar_items.py [--dims 64 90 --layers 3 --k 20 --reps 10]

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
GEMM_TF = 122.0


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


def gpu_step(args):
    import numpy as np
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, propagate, similar, synth
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    ei, ew = g.coo(dev)
    nu, ni, k = g.n_users, g.n_items, args.k
    lib, stream = _native.load(), _native.stream_of(dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(SEED)
    res = {"k": k, "layers": args.layers, "n_items": ni, "runs": []}
    print(f"{ni} items; K = {args.layers}, k = {k}, cosine; composed route in panels of {propagate.panel_rows(ni)} rows", flush=True)
    print("  D | queries | slices | fused us | TF/s | of GEMM | workspace MB | composed us | ratio | same", flush=True)
    for dim in args.dims:
        model = lg.LightGCN(g.num_nodes, dim, args.layers).to(dev).eval()
        with torch.no_grad():
            model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, dim, SEED, dev))
            item_t = model._serving_embedding(ei, ew).detach()[nu:]
        scale = similar.row_rnorm(item_t)
        for n_q in (None, 1, 8, 64):
            q = None if n_q is None else torch.from_numpy(np.sort(rng.choice(ni, size=n_q, replace=False)).astype(np.int64)).to(dev)
            n = ni if q is None else n_q
            ids = torch.arange(ni, device=dev) if q is None else q
            ws_bytes = lib.lgc_item_neighbors_workspace_bytes(n, ni, k, 0)
            ws = torch.empty(max(1, (ws_bytes + 7) // 8), dtype=torch.int64, device=dev)
            index = torch.empty((n, k), dtype=torch.int64, device=dev)
            value = torch.empty((n, k), dtype=torch.float32, device=dev)

            def fused():
                _native.check(lib.lgc_item_neighbors(item_t.data_ptr(), item_t.stride(0), ni, dim, _native.ptr(q), n, scale.data_ptr(),
                                                     None, 1, k, 0, index.data_ptr(), value.data_ptr(), ws.data_ptr(), ws_bytes,
                                                     status.data_ptr(), stream), "lgc_item_neighbors")

            rows = min(n, propagate.panel_rows(ni))
            scores = torch.empty((rows, ni), dtype=torch.float32, device=dev)
            composed_index = torch.empty((n, k), dtype=torch.int64, device=dev)

            def composed():
                for lo in range(0, n, rows):
                    hi = min(n, lo + rows)
                    part, sel = scores[:hi - lo], ids[lo:hi]
                    propagate.score_rows(item_t, sel, item_t, part)
                    part.mul_(scale[sel][:, None]).mul_(scale[None, :])
                    top = propagate.mask_topk(part, None, k + 1)
                    other = top != sel[:, None]                             # the item itself leaves; the order of the rest stays
                    place = torch.cumsum(other, 1) - 1
                    keep = other & (place < k)
                    out = composed_index[lo:hi]
                    out[keep.nonzero(as_tuple=True)[0], place[keep]] = top[keep]

            reps = max(2, args.reps // 4) if q is None else args.reps
            t_fused = event_us(fused, reps)
            t_composed = event_us(composed, reps)
            same = bool(torch.equal(index, composed_index))
            tf = 2.0 * n * ni * dim / (t_fused * 1e-6) / 1e12
            # what the library chose: the count that gives about 512 workgroups, at most one per tile of 128 items
            row_tiles, item_tiles = -(-n // 64), -(-ni // 128)
            slices = max(1, min(-(-512 // row_tiles), 64, item_tiles))
            run = {"dim": dim, "queries": n, "slices": slices, "fused_us": t_fused, "tf_per_s": tf, "of_gemm": tf / GEMM_TF,
                   "workspace_bytes": ws_bytes, "composed_us": t_composed, "ratio": t_composed / t_fused, "same_indices": same}
            res["runs"].append(run)
            print(f"{dim:3d} | {n:7d} | {slices:6d} | {t_fused:8.1f} | {tf:4.1f} | {tf / GEMM_TF:6.1%} | {ws_bytes / 2 ** 20:12.2f} | "
                  f"{t_composed:11.1f} | {t_composed / t_fused:5.1f} | {same}", flush=True)
    lg.check_index_status(dev)
    assert int(status[0].item()) == 0
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 90]); ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--k", type=int, default=20); ap.add_argument("--reps", type=int, default=10)
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
