#!/usr/bin/env python3
"""Hard negatives at full size: ``lgc_sample_hard_triples`` on the bench's cosmetics-scale synthetic graph (1,639,358 users,
54,571 items), B = 1024 triples against the propagated table, M = 1 .. 256 candidates at D = 64 and D = 90 -- beside

* the floor, ``lgc_sample_triples``: the same stream in one launch without any scoring, and
* the composed torch route the library would otherwise need: an int64 ``[B, M]`` candidate matrix (drawn with
  ``torch.randint`` as a stand-in: it rejects nothing, which flatters it), a gather of the B M item rows, ``bmm`` against the
  user rows, ``argmax`` and the gather of the winners.

A call here is ``--inner`` back-to-back launches between two HIP events, divided by their number (one launch of ten
microseconds between two events measures the events); the median over ``--reps`` such windows is reported, with the
smallest and the largest.  With ``--curves`` the tool also runs ``tools/train_demo.py`` with and without hard negatives,
same seeds, and collects its epoch lines.

    python tools/hard_negatives.py [--dims 64 90 --cands 1 4 8 16 32 64 256 --batch 1024 --reps 15 --inner 50] [--curves]

The driver opens no GPU: every measurement is a child process under its own ``timeout``; one JSON line at the end."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0


def window_us(fn, reps, inner, warmup=2):
    """(median, min, max) over ``reps`` windows of the HIP-event time around ``inner`` calls of ``fn``, per call, in us."""
    import torch
    for _ in range(warmup * inner):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(times), min(times), max(times)


def gpu_step(args):
    import torch
    import gnn_ecommerce_amd as lg
    from gnn_ecommerce_amd import _native, synth
    from gnn_ecommerce_amd.sampler import TripleSampler
    dev = torch.device("cuda:0")
    g = synth.make_bipartite(**synth.CONFIG_COSMETICS, seed=SEED)
    ei, ew = g.coo(dev)
    nu, ni, n = g.n_users, g.n_items, args.batch
    purchase = g.weight == 1.0                      # positives = purchases, ignore set = the same pairs (tools/train_step.py)
    pu, pi = g.user[purchase], g.item[purchase] + nu
    s = TripleSampler.from_pairs(nu, ni, pu, pi, pu, pi, dev, seed=SEED)
    lib, stream = _native.load(), _native.stream_of(dev)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    users = s.candidates[torch.randperm(s.candidates.numel(), device=dev, generator=gen)[:n]].contiguous()
    pos, neg = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    pos0, neg0 = torch.empty_like(pos), torch.empty_like(neg)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    attempt, admissible = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    csr = [t.data_ptr() for t in (s.pos_ptr, s.pos_items, s.ign_ptr, s.ign_items)]
    step = [0]

    def floor():
        step[0] += 1
        _native.check(lib.lgc_sample_triples(users.data_ptr(), n, *csr, nu, ni, SEED, step[0], pos0.data_ptr(), neg0.data_ptr(),
                                             s.status.data_ptr(), stream), "lgc_sample_triples")

    res = {"batch": n, "layers": args.layers, "n_users": nu, "n_items": ni, "inner": args.inner, "reps": args.reps, "runs": []}
    print(f"{nu} users, {ni} items; B = {n}, K = {args.layers}; us per call: median (min .. max) of {args.reps} windows of "
          f"{args.inner} calls", flush=True)
    print("  D |   M | one launch us      | floor us           | composed torch us  | composed / one | mean attempt | mean taken", flush=True)
    for dim in args.dims:
        model = lg.LightGCN(g.num_nodes, dim, args.layers).to(dev).eval()
        with torch.no_grad():
            model.embedding.weight.copy_(synth.xavier_table(g.num_nodes, dim, SEED, dev))
            table = model.get_embedding(ei, ew).detach().contiguous()
        ut, it = table[:nu], table[nu:]
        t_floor = window_us(floor, args.reps, args.inner)
        for m in args.cands:
            def hard():
                step[0] += 1
                _native.check(lib.lgc_sample_hard_triples(users.data_ptr(), n, *csr, nu, ni, SEED, step[0], m, ut.data_ptr(),
                                                          table.stride(0), it.data_ptr(), table.stride(0), dim, pos.data_ptr(),
                                                          neg.data_ptr(), score.data_ptr(), attempt.data_ptr(),
                                                          admissible.data_ptr(), s.status.data_ptr(), stream),
                              "lgc_sample_hard_triples")

            def composed():
                cand = torch.randint(0, ni, (n, m), device=dev, generator=gen)
                sc = torch.bmm(it[cand], ut[users].unsqueeze(2)).squeeze(2)
                best = sc.argmax(1, keepdim=True)
                return cand.gather(1, best).squeeze(1) + nu, sc.gather(1, best).squeeze(1)

            t_hard = window_us(hard, args.reps, args.inner)
            t_comp = window_us(composed, args.reps, max(1, args.inner // 5))
            # one launch of each with the same step: M = 1 is the floor's triples, and the winner's score is the pair's dot
            step[0] += 1000
            floor(); step[0] -= 1; hard()
            if m == 1:
                assert torch.equal(pos, pos0) and torch.equal(neg, neg0), "n_cand = 1 differs from lgc_sample_triples"
            ref = (ut[users].double() * table[neg].double()).sum(1)
            err = (score.double() - ref).abs().max().item()
            assert err <= 1e-4 * max(1.0, ref.abs().max().item()), err
            run = {"dim": dim, "n_cand": m, "hard_us": t_hard, "floor_us": t_floor, "composed_us": t_comp,
                   "ratio": t_comp[0] / t_hard[0], "mean_attempt": attempt.float().mean().item(),
                   "mean_admissible": admissible.float().mean().item()}
            res["runs"].append(run)
            fmt = lambda t: f"{t[0]:6.1f} ({t[1]:5.1f}..{t[2]:5.1f})"
            print(f"{dim:3d} | {m:3d} | {fmt(t_hard)} | {fmt(t_floor)} | {fmt(t_comp)} | {t_comp[0] / t_hard[0]:14.1f} | "
                  f"{run['mean_attempt']:12.2f} | {run['mean_admissible']:10.2f}", flush=True)
        del model, table, ut, it
    s.check()
    lg.check_index_status(dev)
    print(json.dumps(res))
    return 0


CURVES = (("uniform", []), ("hard8_layer0", ["--hard-negatives", "8"]), ("hard8_refresh4", ["--hard-negatives", "8", "--refresh", "4"]))


def curves(args):
    """tools/train_demo.py per variant, same seeds: its epoch lines, collected."""
    out = {}
    for name, extra in CURVES:
        cmd = ["timeout", "-k", "10", str(args.gpu_timeout), sys.executable, os.path.join(ROOT, "tools", "train_demo.py"),
               "--epochs", str(args.epochs), *extra]
        proc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if proc.returncode != 0:
            print(f"{name}: train_demo ended with status {proc.returncode}")
            return proc.returncode
        out[name] = [json.loads(line) for line in proc.stdout.splitlines() if line.startswith("{")]
        for e in out[name]:
            print(f"{name:15s} epoch {e['epoch']:2d}  R@20 {e['R@20']:.4f}  P@20 {e['P@20']:.4f}  bpr {e['bpr']:8.2f}  "
                  f"grad weight {e['grad_weight']:.4f}  attempt {e['neg_attempt']}", flush=True)
    print(json.dumps({"curves": out, "epochs": args.epochs}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 90]); ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--cands", type=int, nargs="+", default=[1, 4, 8, 16, 32, 64, 256])
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50); ap.add_argument("--curves", action="store_true")
    ap.add_argument("--epochs", type=int, default=3, help="with --curves: epochs of each train_demo run")
    ap.add_argument("--step", choices=["all", "gpu"], default="all")
    ap.add_argument("--gpu-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.step == "gpu":
        return gpu_step(args)
    if args.curves:
        return curves(args)
    cmd = ["timeout", "-k", "10", str(args.gpu_timeout), sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--step", "gpu"]
    code = subprocess.run(cmd, cwd=ROOT).returncode
    if code != 0:
        print(f"the measurement ended with status {code}")
    return code


if __name__ == "__main__":
    sys.exit(main())
