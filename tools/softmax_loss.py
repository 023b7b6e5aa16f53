#!/usr/bin/env python3
"""What the in-batch softmax loss costs and what it buys.  Three parts, each a JSON line per result:

  entry   lgc_softmax_batch alone at B = 1024, C = 2048, D = 64 and 90 beside the same outputs composed from torch ops
          (gather, mm, a mask by searchsorted, logsumexp, softmax, two mm), in alternating rounds, device events around
          each block; the two routes' outputs are compared first.
  step    the full training step with this loss (sampler -> softmax_loss + routed regulariser -> backward -> Adam) beside
          the BPR step at the same batch, on the cosmetics-scale synthetic graph under tools/train_step.py's protocol
          (three warm-up steps, a host clock around steps that each end in a host sync), in alternating blocks.
  curves  tools/train_demo.py's recall@20 per epoch for both losses at equal steps.

    python tools/softmax_loss.py [--part entry|step|curves|all] [--rounds 5] [--iters 50] [--steps 10]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import synth
from gnn_ecommerce_amd.softmax import softmax_batch

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["entry", "step", "curves", "all"], default="all")
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--steps", type=int, default=10); ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--temperature", type=float, default=0.2)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn, iters):
    """ms per call: device events around ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def entry_part():
    n_users, n_items, b, c = 20000, 4000, 1024, 2048
    n = n_users + n_items
    rng = np.random.default_rng(0)
    # ignore lists of ~12 items per user, as the demo's sampler holds them
    iu = np.repeat(np.arange(n_users), 12)
    ii = rng.integers(0, n_items, iu.size) + n_users
    sampler = lg.TripleSampler.from_pairs(n_users, n_items, iu, ii, iu, ii, dev, seed=0)
    ptr, items = sampler.ign_ptr, sampler.ign_items
    owner = torch.repeat_interleave(torch.arange(n_users, device=dev), (ptr[1:] - ptr[:-1]).long())
    keys = owner * n + items
    for dim in (64, 90):
        table = (torch.randn(n, dim, device=dev) * 0.3).contiguous()
        users, pos, neg = sampler.sample(b)
        cands = torch.cat([pos, neg])
        target = torch.arange(b, dtype=torch.int32, device=dev)
        t64, rows = target.long(), torch.arange(b, device=dev)
        inv_tau = 1.0 / args.temperature

        def fused():
            return softmax_batch(table, n_users, users, cands, target, (ptr, items), inv_tau, b)

        def composed():
            eu, ec = table[users], table[cands]
            z = (eu @ ec.t()) * inv_tau
            q = users[:, None] * n + cands[None, :]
            at = torch.searchsorted(keys, q).clamp(max=keys.numel() - 1)
            adm = (keys[at] != q) & (cands[None, :] != cands[t64][:, None])
            adm[rows, t64] = True
            zm = z.masked_fill(~adm, float("-inf"))
            loss = (torch.logsumexp(zm, 1) - z[rows, t64]).sum() / b
            p = torch.softmax(zm, 1)
            p[rows, t64] -= 1.0
            g = p * (inv_tau / b)
            return loss, g @ ec, g.t() @ eu

        f, t = fused(), composed()
        agree = {"loss_rel": abs(f.loss.item() - t[0].item()) / abs(t[0].item()),
                 "grad_users_rel": ((f.grad_users - t[1]).norm() / t[1].norm()).item(),
                 "grad_cands_rel": ((f.grad_cands - t[2]).norm() / t[2].norm()).item()}
        for _ in range(10):
            fused(); composed()
        torch.cuda.synchronize()
        ms_f, ms_t = [], []
        for _ in range(args.rounds):                                     # alternating blocks
            ms_f.append(timed(fused, args.iters)); ms_t.append(timed(composed, args.iters))
        print(json.dumps({"part": "entry", "B": b, "C": c, "D": dim, "fused_ms": statistics.median(ms_f),
                          "composed_ms": statistics.median(ms_t), "fused_rounds": [round(x, 4) for x in ms_f],
                          "composed_rounds": [round(x, 4) for x in ms_t], "agreement": agree,
                          "mean_admitted": f.n_adm.float().mean().item()}), flush=True)
    lg.check_index_status()


def step_part():
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=0)
    ei, ew = g.coo(dev)
    purchase = g.weight == 1.0
    pu, pi = g.user[purchase], g.item[purchase] + g.n_users
    sampler = lg.TripleSampler.from_pairs(g.n_users, g.n_items, pu, pi, pu, pi, dev, seed=0)
    for dim in (64, 90):
        model = lg.LightGCN(g.num_nodes, dim, 3).to(dev)
        opt = torch.optim.Adam(model.parameters(), 0.005)

        def bpr_step():
            opt.zero_grad()
            u, p, n = sampler.sample(args.batch)
            labels = torch.stack((torch.cat([u, u]), torch.cat([p, n])))
            out = model(ei, labels, ew)
            size = len(u)
            bpr = model.recommendation_loss(out[:size], out[size:], 0) * size
            reg = lg.regularization_loss(model.embedding.weight, size, u, p, n, 1e-4)
            loss = bpr + reg
            loss.backward()
            opt.step()
            return bpr.item(), reg.item(), loss.item()          # the three host syncs of train_lightgcn.py:149-151

        def softmax_step():
            opt.zero_grad()
            u, p, n = sampler.sample(args.batch)
            sm = model.softmax_loss(ei, ew, u, p, n, temperature=args.temperature, ignore=sampler)
            reg = model.regularization_loss(u, p, n, 1e-4)
            loss = sm + reg
            loss.backward()
            opt.step()
            return sm.item(), reg.item(), loss.item()

        def block(fn):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

        for _ in range(3):
            bpr_step(); softmax_step()
        ms_b, ms_s = [], []
        for _ in range(args.rounds):
            ms_b.append(block(bpr_step)); ms_s.append(block(softmax_step))
        print(json.dumps({"part": "step", "B": args.batch, "D": dim, "K": 3, "bpr_ms_per_step": statistics.median(ms_b),
                          "softmax_ms_per_step": statistics.median(ms_s), "bpr_rounds": [round(x, 3) for x in ms_b],
                          "softmax_rounds": [round(x, 3) for x in ms_s]}), flush=True)
        del model, opt
    sampler.check(); lg.check_index_status()


def curves_part():
    import train_demo
    for loss in ("bpr", "softmax"):
        print(json.dumps({"part": "curves", "loss": loss, "temperature": args.temperature if loss == "softmax" else None}), flush=True)
        train_demo.main(["--loss", loss, "--temperature", str(args.temperature), "--epochs", "4"])


if args.part in ("entry", "all"):
    entry_part()
if args.part in ("curves", "all"):
    curves_part()
if args.part in ("step", "all"):
    step_part()
