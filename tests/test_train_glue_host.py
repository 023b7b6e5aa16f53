"""The references of tests/train_glue_support.py, checked without a device: against the CPU doubles of tests/cpu_ops.py,
against tiny cases worked out by hand, and -- for every bound -- against an fp32 emulation of the kernel's own order of
operations, which has to stay inside the bound the device test applies."""
import math

import numpy as np
import pytest
import torch

import train_glue_support as tgs
from cpu_ops import CpuOp, CpuOps

CPU = CpuOps()


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ----------------------------------------------------------------------------------------
# by hand
# ----------------------------------------------------------------------------------------
def test_pair_scores_by_hand():
    emb = tgs.f32([[1, 2, 3], [0.5, -1, 4], [2, 0, -1]])
    scores, mag, r0, r1, ok = tgs.pair_scores_ref(emb, [0, 1, 2, -1, 0], [1, 1, 0, 0, 3])
    assert scores[:3].tolist() == [10.5, 17.25, -1.0] and np.isnan(scores[3:]).all()
    assert mag[:3].tolist() == [14.5, 17.25, 5.0] and ok.tolist() == [1, 1, 1, 0, 0]
    assert r0[2].tolist() == [2, 0, -1] and r1[2].tolist() == [1, 2, 3] and not r0[3:].any() and not r1[3:].any()
    assert tgs.pair_scores_bound(64, 1.0) == 8 * tgs.U and tgs.pair_scores_bound(65, 1.0) == 9 * tgs.U
    assert tgs.pair_scores_bound(1, 2.0) == 16 * tgs.U and tgs.pair_scores_bound(300, 1.0) == 12 * tgs.U


def test_pair_seed_vals_by_hand():
    rows0, rows1 = tgs.f32([[1, 2], [3, 4]]), tgs.f32([[5, 6], [7, 8]])
    got = tgs.pair_seed_vals_ref([2, -1], [1, 0], 0.5, rows0, rows1)
    assert got.tolist() == [[5, 6], [0, 0], [1, 2], [0, 0]]
    assert tgs.pair_seed_vals_ref([2, -1], None, None, rows0, rows1).tolist() == [[10, 12], [-7, -8], [2, 4], [-3, -4]]
    # two roundings, in the kernel's order: fl(fl(g * scale) * row), not fl(g * fl(scale * row))
    g, s, r = np.float32(1.1), np.float32(0.37), np.float32(3.3)
    assert tgs.pair_seed_vals_ref([g], None, s, [[r]], [[r]])[0, 0] == np.float32(np.float32(g * s) * r)


def test_bpr_by_hand():
    loss, grad = tgs.bpr_ref(tgs.f32([0, 3, 1, 0, 5, 1]), None, 2)               # d = 0, -2, 0
    assert loss == pytest.approx((2 * math.log(2) + math.log1p(math.exp(2))) / 2, rel=1e-15)
    assert grad[:3] == pytest.approx([-0.25, -0.5 / (1 + math.exp(-2)), -0.25], rel=1e-15) and (grad[3:] == -grad[:3]).all()
    loss, grad = tgs.bpr_ref(tgs.f32([0, np.nan, 1, 0, 5, np.nan]), [1, 0, 0], 4)
    assert loss == pytest.approx(math.log(2) / 4, rel=1e-15) and grad.tolist() == [-0.125, 0, 0, 0.125, 0, 0]
    loss, grad = tgs.bpr_ref(tgs.f32([1e4, -1e4, 0, 0]), None, 1)                # far beyond exp's range on both sides
    assert loss == 1e4 and grad.tolist() == [0, -1, 0, 1]
    loss, grad = tgs.bpr_ref(tgs.f32([89, 0]), None, 1)
    assert 0 < grad[1] == pytest.approx(math.exp(-89), rel=1e-12) and loss == pytest.approx(math.exp(-89), rel=1e-12)
    loss, grad = tgs.bpr_ref(tgs.f32([1, 2, 3, 4]), [0, 0], 7)
    assert loss == 0.0 and not grad.any()


def test_reg_rows_by_hand():
    w = tgs.f32([[1, 2], [3, 4], [0, -1]])
    value, rows = tgs.reg_rows_ref(w, [[0, -1], [1, 1], [3, -4, 2]], 0.5)
    assert rows.tolist() == [0, 2, 1, 1, -1, -1, 2] and value == 0.5 * (5 + 1 + 25 + 25 + 1)
    assert tgs.reg_rows_ref(w, [[], [], []], 0.5)[0] == 0.0
    assert tgs.reg_rows_bound(64, 3072) == (64 + 3 + 30) * tgs.U and tgs.reg_rows_bound(1, 0) == 31 * tgs.U


def test_adam_by_hand():
    hyper = tgs.f32([0.5, 0.25, 0.75, 1.0, 2.0, 0.5])
    w, m, v = tgs.adam_ref([1.0, 1.0], [4.0, 0.0], [2.0, 0.0], [16.0, 0.0], hyper)
    assert m.tolist() == [3.0, 0.0] and v.tolist() == [16.0, 0.0]                # 0.25 * 16 + 0.75 * 16
    assert w[0] == 1.0 - 2.0 * (3.0 / (4.0 / 0.5 + 1.0)) and w[1] == 1.0
    w, m, v = tgs.adam_ref([1.0], [0.0], [0.0], [0.0], tgs.adam_hyper(1))
    assert (w[0], m[0], v[0]) == (1.0, 0.0, 0.0)
    h = tgs.adam_hyper(1)
    assert h[4] == np.float32(1e-3 / (1 - 0.9)) and h[5] == np.float32(math.sqrt(1 - 0.999)) and h[2] == np.float32(1 - 0.999)
    w, m, v = tgs.adam_ref([1.0], [1e21], [0.0], [0.0], h)                       # (1 - b2) g g leaves fp32's range
    assert v[0] == np.inf and w[0] == 1.0 and tgs.adam_errors([np.inf], v)[0] == 0 and tgs.adam_errors([1e38], v)[0] == np.inf


def test_segment_sum_by_hand():
    keys, dest = [-5, -5, 2, 9, 9, 9], [1, -7, 5, 0, -7, -7]
    vals = tgs.f32([[1], [2], [100], [0.5], [0.25], [8]])
    base = tgs.f32([[10], [20], [30]])
    assert tgs.segment_sum_ref(keys, dest, vals, None, base, 2.0, False).tolist() == [[17.5], [6], [30]]
    assert tgs.segment_sum_ref(keys, dest, vals, None, base, 2.0, True).tolist() == [[27.5], [26], [30]]
    assert tgs.segment_sum_ref(keys, dest, vals[::-1], [5, 4, 3, 2, 1, 0], base, 2.0, False).tolist() == [[17.5], [6], [30]]
    # sequential in fp32: 2^24 + 1 + 1 stays 2^24, where a pairwise or a float64 sum would give 2^24 + 2
    vals = tgs.f32([[2 ** 24], [1], [1]])
    assert tgs.segment_sum_ref([0, 0, 0], [0, -7, -7], vals, None, tgs.f32([[0]]), 1.0, False)[0, 0] == 2 ** 24
    keys, dest = tgs.segment_layout()
    assert (np.diff(keys) >= 0).all() and keys[0] < 0 and keys[-1] == 2 ** 62 and keys[-2] != keys[-1]
    assert keys.size == sum(tgs.SEGMENT_RUNS) and sorted(dest[dest != -7].tolist()) == sorted(tgs.SEGMENT_DEST)


def test_seed_prepare_by_hand():
    got = tgs.seed_prepare_ref([7, 2, 9, 2, -1, 10, 5, 2], split=6, n=10)
    assert got["rows_sorted"].tolist() == [-1, -1, 2, 2, 2, 5, 7, 9]
    assert got["perm"].tolist() == [4, 5, 1, 3, 7, 6, 0, 2] and got["perm"].dtype == np.int32
    assert got["dest_item"].tolist() == [-1, -1, -1, -1, -1, -1, 7, 9]
    assert got["dest_slot"].tolist() == [-1, -1, 2, -1, -1, 5, -1, -1]
    assert got["dest_user"].tolist() == [-1, -1, 2, -1, -1, 5, -1, -1]
    assert got["flag"].tolist() == [0, 0, 1, 0, 0, 1, 0] and got["slot"].tolist() == [-7, -7, 2, -7, -7, 5, -7]
    empty = tgs.seed_prepare_ref([], 0, 5)
    assert empty["rows_sorted"].size == 0 and empty["flag"].tolist() == [0]


def test_lincomb_by_hand():
    a, b = tgs.f32([[1, 2]]), tgs.f32([[10, 20]])
    assert tgs.lincomb_ref([(2.0, a)]).tolist() == [[2, 4]] and tgs.lincomb_ref([(2.0, a), (-0.5, b)]).tolist() == [[-3, -6]]
    c, x, y = np.float32(0.1), np.float32(3.3), np.float32(1e-3)
    assert tgs.lincomb_ref([(c, [[x]]), (c, [[y]])])[0, 0] == np.float32(np.float32(c * x) + np.float32(c * y))


def test_seed_pull_by_hand():
    rowptr, cols, vals = [0, 0, 0, 3, 3, 5], [0, 1, 0, 1, 1], tgs.f32([2, 3, 4, 0.5, 0.25])      # rows 2 and 4 of a 5-row table
    flag, slot = [0, 1, 0], [-7, 1, -7]
    x = tgs.f32([[np.nan, np.nan], [1, -2]])
    out, mag, count = tgs.seed_pull_ref(rowptr, cols, vals, 2, 5, flag, slot, x)
    assert out.tolist() == [[3, -6], [0, 0], [0.75, -1.5]] and mag.tolist() == [[3, 6], [0, 0], [0.75, 1.5]]
    assert count.tolist() == [1, 0, 2] and tgs.seed_pull_bound(mag, count)[2, 1] == 4 * tgs.U * 1.5
    emu = tgs.seed_pull_emulated(rowptr, cols, vals, 2, 5, flag, slot, x, short_max=1, chunk_len=1, groups=2)
    assert emu.tolist() == out.tolist()


# ----------------------------------------------------------------------------------------
# against the CPU doubles
# ----------------------------------------------------------------------------------------
def test_references_agree_with_the_cpu_doubles():
    rng = np.random.default_rng(0)
    n, dim, m = 50, 19, 40
    emb = tgs.f32(rng.standard_normal((n, dim)))
    idx0, idx1 = rng.integers(-2, n + 2, size=m), rng.integers(-2, n + 2, size=m)
    scores, mag, r0, r1, ok = tgs.pair_scores_ref(emb, idx0, idx1)
    c_scores, c0, c1, c_ok = CPU.pair_scores_rows(tt(emb), tt(idx0), tt(idx1))
    assert torch.equal(c_ok, tt(ok)) and 0 < ok.sum() < m and torch.equal(c0, tt(r0)) and torch.equal(c1, tt(r1))
    valid = ok != 0
    assert np.isnan(scores[~valid]).all() and bool(torch.isnan(c_scores[~tt(valid)]).all())
    assert (np.abs(c_scores.numpy()[valid] - scores[valid]) <= dim * tgs.U * mag[valid]).all()
    # seed values: the double multiplies in the same order, so the bits agree
    gs, mask = tgs.f32(rng.standard_normal(m)), (rng.random(m) < 0.5)
    want = tgs.pair_seed_vals_ref(gs, mask, 0.37, r0, r1)
    assert torch.equal(CPU.pair_seed_vals(tt(gs), tt(mask), torch.tensor(0.37), tt(r0), tt(r1)), tt(want))
    assert torch.equal(CPU.pair_seed_vals(tt(gs), None, None, tt(r0), tt(r1)), tt(tgs.pair_seed_vals_ref(gs, None, None, r0, r1)))
    # BPR: torch's fp32 logsigmoid / sigmoid on moderate differences
    s = tgs.bpr_scores(rng, 300, planted=False)
    for mk in (None, (rng.random(300) < 0.4)):
        loss, grad = tgs.bpr_ref(s, mk, 1024)
        c_loss, c_grad = CPU.bpr_loss(tt(s), None if mk is None else tt(mk), 1024)
        assert abs(c_loss.item() - loss) <= 1e-6 * abs(loss) and np.abs(c_grad.numpy() - grad).max() <= 1e-6 * np.abs(grad).max()
    # Adam
    w, g, m_, v = tgs.adam_inputs(rng, 500)
    hyper = tgs.adam_hyper(3)
    w1, m1, v1 = tgs.adam_ref(w[7:400], g[7:400], m_[7:400], v[7:400], hyper)
    cw, cg, cm, cv = (tt(x.copy()) for x in (w, g, m_, v))
    CPU.adam_rows(cw, cg, cm, cv, 7, 400, tt(hyper))
    bw, bm, bv = tgs.adam_bounds(w[7:400], g[7:400], m_[7:400], v[7:400], hyper)
    assert tgs.worst_ratio(tgs.adam_errors(cm.numpy()[7:400], m1), bm) <= 1 and tgs.worst_ratio(tgs.adam_errors(cv.numpy()[7:400], v1), bv) <= 1
    assert tgs.worst_ratio(tgs.adam_errors(cw.numpy()[7:400], w1), bw) <= 1
    assert np.array_equal(cw.numpy()[:7], w[:7]) and np.array_equal(cw.numpy()[400:], w[400:])
    # segment sums: the double adds a run with index_add_, also in position order on the host
    keys, dest = tgs.segment_layout()
    vals = tgs.f32(rng.standard_normal((keys.size, 5)))
    base = tgs.f32(rng.standard_normal((tgs.SEGMENT_ROWS, 5)))
    for scale, acc in ((1.0, False), (0.125, True)):
        out = tt(base.copy())
        CPU.segment_sum(tt(keys), tt(dest), tt(vals), out, scale=scale, accumulate=acc)
        want = tgs.segment_sum_ref(keys, dest, vals, None, base, scale, acc)
        assert np.abs(out.numpy() - want).max() <= 1e-2 and (out.numpy() == want)[[4, 9, 49, 2, 8, 12]].all()    # runs of one: same bits
    # seed preparation
    for pattern in tgs.SEED_PATTERNS:
        rows = tgs.seed_rows(pattern, 300, 120, 200, rng)
        want = tgs.seed_prepare_ref(rows, 120, 200)
        flag, slot = torch.zeros(121, dtype=torch.uint8), torch.full((121,), -7, dtype=torch.int32)
        got = CPU.seed_prepare(tt(rows), 120, 200, flag, slot)
        for g_, name in zip(got, ("rows_sorted", "perm", "dest_item", "dest_slot", "dest_user")):
            assert g_.dtype == tt(want[name]).dtype and torch.equal(g_, tt(want[name])), (pattern, name)
        assert torch.equal(flag, tt(want["flag"])) and torch.equal(slot, tt(want["slot"])), pattern
        CPU.seed_flags(got[0], 120, flag, 0)
        assert int(flag.sum()) == 0
    # linear combination: the same chain of rounded products and adds
    terms = [(c, tgs.f32(rng.standard_normal((9, 7)))) for c in (0.37, -1.25, 1.0, 0.2)]
    y = torch.empty(9, 7)
    CPU.lincomb(y, [(c, tt(s_)) for c, s_ in terms])
    assert torch.equal(y, tt(tgs.lincomb_ref(terms)))
    # seeded pull
    ei, ew, nu, ni = tgs.pull_graph()
    rowptr, cols, vals = transpose_csr(ei, ew, nu + ni)
    seeds = tgs.pull_seeds(ei, nu, ni)["forty_users"]
    prep = tgs.seed_prepare_ref(seeds, nu, nu + ni)
    x = tgs.f32(rng.standard_normal((seeds.size, 6)))
    ref, mag, count = tgs.seed_pull_ref(rowptr, cols, vals, nu, nu + ni, prep["flag"], prep["slot"], x)
    out = torch.full((nu + ni, 6), 7.5)
    CPU.seed_pull(CpuOp(tt(rowptr), tt(cols), tt(vals), nu, nu + ni), tt(prep["flag"]), tt(prep["slot"]), tt(x), out, None)
    assert bool((out[:nu] == 7.5).all()) and count.max() > 5
    assert tgs.worst_ratio(np.abs(out[nu:].numpy() - ref), tgs.seed_pull_bound(mag, count)) <= 1


def transpose_csr(ei, ew, n):
    """Rows = sources of the edge list, entries in edge order (a stable sort), the weights as they are."""
    order = np.argsort(ei[0], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int64)
    return rowptr, ei[1][order], tgs.f32(ew[order])


# ----------------------------------------------------------------------------------------
# every bound holds for the kernel's order of operations in fp32
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300])
def test_pair_scores_bound_holds_for_the_kernels_order(dim):
    rng = np.random.default_rng(dim)
    emb = tgs.f32(rng.standard_normal((37, dim)))
    idx0, idx1 = rng.integers(0, 37, size=1027), rng.integers(0, 37, size=1027)
    ref, mag, r0, r1, _ = tgs.pair_scores_ref(emb, idx0, idx1)
    r = tgs.worst_ratio(np.abs(tgs.pair_scores_emulated(r0, r1).astype(np.float64) - ref), tgs.pair_scores_bound(dim, mag))
    assert r <= 0.5, r
    # the bound is not slack enough to hide one column dropped from a pair's sum
    short = np.abs((r0[:, 1:].astype(np.float64) * r1[:, 1:]).sum(1) - ref)
    assert dim == 1 or tgs.worst_ratio(short, tgs.pair_scores_bound(dim, mag)) > 100


@pytest.mark.parametrize("b", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 3000, 8192])
def test_bpr_bounds_hold_for_the_kernels_formula(b):
    rng = np.random.default_rng(b)
    s = tgs.bpr_scores(rng, b)
    for size in sorted({1, b, 1024}):
        for mask in (None, (rng.random(b) < 0.4).astype(np.uint8)):
            loss, grad = tgs.bpr_ref(s, mask, size)
            e_loss, e_grad = tgs.bpr_emulated(s, mask, size)
            assert tgs.worst_ratio(np.abs(e_grad.astype(np.float64) - grad), tgs.bpr_grad_bound(grad, size)) <= 0.6
            assert tgs.worst_ratio(abs(float(e_loss) - loss), abs(loss) * tgs.bpr_loss_bound(b)) <= 0.6
    # a triple dropped from the loss, or a gradient off by the factor of a wrong size, is far outside
    loss, grad = tgs.bpr_ref(s, None, 1024)
    if b > 1:
        t = int(np.argmax(s[b:] - s[:b]))
        drop = np.ones(b, dtype=np.uint8)
        drop[t] = 0
        assert abs(tgs.bpr_ref(s, drop, 1024)[0] - loss) > 100 * abs(loss) * tgs.bpr_loss_bound(b)
    assert tgs.worst_ratio(np.abs(grad * (1024 / 1023) - grad), tgs.bpr_grad_bound(grad, 1024)) > 100


@pytest.mark.parametrize("dim,lens", [(1, (1, 0, 0)), (5, (0, 0, 5)), (7, (341, 342, 342)), (64, (1024, 1024, 1024)),
                                      (90, (1000, 3, 2100)), (256, (1024, 1024, 1024)), (129, (1000, 3, 2100))])
def test_reg_rows_bound_holds_for_the_kernels_order(dim, lens):
    rng = np.random.default_rng(dim)
    n = 500
    w = tgs.f32(rng.standard_normal((n, dim)) * 0.1)
    lists = [rng.integers(-n, n, size=k).astype(np.int64) for k in lens]
    ref, rows = tgs.reg_rows_ref(w, lists, 4.9e-8)
    got = float(tgs.reg_rows_emulated(w, lists, 4.9e-8))
    assert abs(got - ref) <= 0.5 * abs(ref) * tgs.reg_rows_bound(dim, sum(lens))
    if sum(lens) > 1000:                                        # one row dropped or counted twice is far outside
        one = float((w[rows[-1]].astype(np.float64) ** 2).sum()) * float(np.float32(4.9e-8))
        assert one > 10 * abs(ref) * tgs.reg_rows_bound(dim, sum(lens))


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_bounds_hold_for_the_kernels_expression(step):
    rng = np.random.default_rng(step)
    w, g, m, v = tgs.adam_inputs(rng, 100003)
    assert all((g == x).any() for x in tgs.f32([0.0, 1e-20, 1e18, 1e20])) and ((m == 0) & (v == 0)).any()
    hyper = tgs.adam_hyper(step)
    refs, bounds = tgs.adam_ref(w, g, m, v, hyper), tgs.adam_bounds(w, g, m, v, hyper)
    assert all(np.isfinite(r).all() for r in refs)
    for got, ref, bound in zip(tgs.adam_emulated(w, g, m, v, hyper), refs, bounds):
        assert tgs.worst_ratio(tgs.adam_errors(got, ref), bound) <= 1.0
    # a step with the moments of its neighbour is far outside
    w1 = tgs.adam_emulated(w, g, np.roll(m, 1), v, hyper)[0]
    assert tgs.worst_ratio(tgs.adam_errors(w1, refs[0]), bounds[0]) > 100


@pytest.mark.parametrize("plan,dim", [(plan, dim) for plan in tgs.PULL_PLANS for dim in (3, 64, 90)] + [((4, 16), 1), ((4, 16), 256)])
def test_seed_pull_bound_holds_for_the_plans_order(plan, dim):
    rng = np.random.default_rng(dim)
    ei, ew, nu, ni = tgs.pull_graph()
    rowptr, cols, vals = transpose_csr(ei, ew, nu + ni)
    seeds = tgs.pull_seeds(ei, nu, ni)["forty_users"]
    prep = tgs.seed_prepare_ref(seeds, nu, nu + ni)
    x = tgs.f32(rng.standard_normal((seeds.size, dim)))
    ref, mag, count = tgs.seed_pull_ref(rowptr, cols, vals, nu, nu + ni, prep["flag"], prep["slot"], x)
    groups = 64 // (dim if dim < 4 else (dim + 3) // 4)
    emu = tgs.seed_pull_emulated(rowptr, cols, vals, nu, nu + ni, prep["flag"], prep["slot"], x, plan[0], plan[1], groups)
    assert tgs.worst_ratio(np.abs(emu.astype(np.float64) - ref), tgs.seed_pull_bound(mag, count)) <= 0.6


# ----------------------------------------------------------------------------------------
# the inputs are what the device test says they are
# ----------------------------------------------------------------------------------------
def test_pull_graph_has_every_row_class_under_every_plan():
    ei, ew, nu, ni = tgs.pull_graph()
    assert ei.shape[1] == ew.size and ei.min() >= 0 and ei.max() < nu + ni and ((ei[0] < nu) != (ei[1] < nu)).all()
    deg = np.bincount(ei[1][ei[1] >= nu] - nu, minlength=ni)
    assert sorted(deg.tolist()) == sorted(tgs.PULL_DEGREES) and deg[-1] == 0 and (ei[0] == nu - 1).any()
    assert len(set(zip(ei[0].tolist(), ei[1].tolist()))) == ei.shape[1]           # no repeated edge
    counts = []
    for plan in tgs.PULL_PLANS:
        short, single, multi, chunks = tgs.plan_classes(deg, *plan)
        assert short + single + multi == ni
        assert (short == ni and chunks == 0) if plan[0] >= 100000 else (short > 0 and single > 0 and multi > 0), plan
        counts.append(chunks)
    assert any(0 < c < 16 for c in counts) and any(c > 16 for c in counts) and any(c % 16 for c in counts), counts
    assert tgs.plan_classes([0, 4, 5, 16, 17, 33], 4, 16) == (2, 2, 2, 7)
    # one seed user leaves most rows of every class without a seed
    seeds = tgs.pull_seeds(ei, nu, ni)
    one = int(seeds["one_user"][0])
    marked = np.zeros(ni, dtype=bool)
    marked[ei[1][ei[0] == one] - nu] = True
    assert marked.any()
    for lo, hi in ((1, 10), (33, 70), (300, 700)):
        cls = (deg >= lo) & (deg <= hi)
        assert 2 * (cls & ~marked).sum() > cls.sum()
    many = seeds["forty_users"]
    assert many.size == 50 and np.unique(many).size < many.size and (many >= nu).sum() == 10 and seeds["none"].size == 0


def test_seed_row_patterns_are_what_their_names_say():
    rng = np.random.default_rng(1)
    n = 10000
    for split in (0, 8400, n):
        for m in (0, 1, 9, 8192):
            for pattern in tgs.SEED_PATTERNS:
                rows = tgs.seed_rows(pattern, m, split, n, rng)
                assert rows.dtype == np.int64 and rows.shape == (m,), (pattern, m, split)
            if m > 1:
                assert (np.diff(tgs.seed_rows("descending", m, split, n, rng)) < 0).all()
                assert np.unique(tgs.seed_rows("all_equal", m, split, n, rng)).size == 1
                out = tgs.seed_rows("all_out_of_range", m, split, n, rng)
                assert ((out < 0) | (out >= n)).all()
    edges = tgs.seed_rows("edges", 500, 8400, n, rng)
    assert {8399, 8400, n - 1, 0, -1, n, 2 ** 40} <= set(edges.tolist())
    s = tgs.bpr_scores(rng, 3000)
    d = (s[:3000] - s[3000:]).tolist()
    assert all(any(abs(y - x) <= 1e-5 * abs(x) for y in d) for x in tgs.PLANTED_D)


def test_worst_ratio_counts_nan_and_zero_bounds():
    assert tgs.worst_ratio([0.0, 0.0], [0.0, 1.0]) == 0.0 and tgs.worst_ratio([1e-30], [0.0]) == math.inf
    assert tgs.worst_ratio([np.nan], [1.0]) == math.inf and tgs.worst_ratio([], []) == 0.0
    assert tgs.worst_ratio([1.0, 3.0], [2.0, 2.0]) == 1.5
