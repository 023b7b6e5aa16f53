"""The kernels of a training step against float64 at their edge shapes: all of csrc/lgconv_train.hip, and lgc_seed_pull /
lgc_lincomb of csrc/lgconv_hip.hip.  References and bounds: tests/train_glue_support.py (checked on the host by
tests/test_train_glue_host.py); the bounds count roundings and a failure prints the worst
error / bound ratio of its case.  The shapes are the smallest at which each code path is taken."""
import numpy as np
import pytest
import torch

import train_glue_support as tgs

import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate
from gnn_ecommerce_amd.graph import Operator, PropGraph

pytestmark = pytest.mark.gpu

OPS = propagate.DEVICE_OPS
WORST = {}          # kernel -> worst error / bound of this run, printed when the module is done (pytest -s shows it)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for name in sorted(WORST):
        print(f"\n[train glue] worst error / bound, {name}: {WORST[name]:.4f}", end="")
    print()


def within(name, err, bound, case):
    r = tgs.worst_ratio(err, bound)
    WORST[name] = max(WORST.get(name, 0.0), r)
    assert r <= 1.0, f"{name} {case}: worst error / bound = {r:.4g}"


def to_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(t):
    return t.contiguous().view(torch.int32)


def sliced(rng, rows, dim, layout, device, scale=1.0):
    """(numpy view, device view) of a [rows, dim] table: contiguous, or columns of a wider table at an odd / an even stride."""
    stride, offset = {"dense": (dim, 0), "odd_stride": ((dim + 4) | 1, 1), "even_stride": (dim + 6 + dim % 2, 3)}[layout]
    wide, offset = tgs.column_slice(rng, rows, dim, stride, offset, scale)
    return wide[:, offset:offset + dim], to_dev(wide, device)[:, offset:offset + dim]


LAYOUTS = ["dense", "odd_stride", "even_stride"]


# ----------------------------------------------------------------------------------------
# pair scores
# ----------------------------------------------------------------------------------------
def pair_ids(rng, n, m):
    idx0, idx1 = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    if m >= 3:
        idx0[1], idx1[1] = idx0[0], idx1[0]        # a repeated pair
        idx1[2] = idx0[2]                          # a node with itself
    return idx0.astype(np.int64), idx1.astype(np.int64)


@pytest.mark.parametrize("dim", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300])
def test_pair_scores_at_every_width_and_stride(device, dim):
    """lgc_pair_dot and lgc_pair_dot_rows: one wavefront per pair, lanes striding the columns -- widths around every multiple
    of the wavefront, pair counts that leave the last workgroup partly empty, tables that are column slices of a wider one."""
    rng = np.random.default_rng(dim)
    n = 37
    for layout in LAYOUTS:
        emb, emb_d = sliced(rng, n, dim, layout, device)
        for m in (1, 3, 4, 5, 1027):
            case = f"dim {dim} {layout} m {m}"
            idx0, idx1 = pair_ids(rng, n, m)
            ref, mag, rows0, rows1, ok = tgs.pair_scores_ref(emb, idx0, idx1)
            i0, i1 = to_dev(idx0, device), to_dev(idx1, device)
            plain = OPS.pair_scores(emb_d, i0, i1)
            scores, r0, r1, okd = OPS.pair_scores_rows(emb_d, i0, i1)
            assert torch.equal(bits(plain), bits(scores)), case
            bound = tgs.pair_scores_bound(dim, mag)
            within("pair_scores", np.abs(plain.cpu().numpy().astype(np.float64) - ref), bound, case)
            assert torch.equal(r0.cpu(), torch.from_numpy(rows0)) and torch.equal(r1.cpu(), torch.from_numpy(rows1)), case
            assert torch.equal(okd.cpu(), torch.from_numpy(ok)) and bool(ok.all()), case
    lg.check_index_status()            # nothing was out of range


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("dim", [2, 65, 256])
def test_pair_scores_of_invalid_ids(device, dim, slot):
    """Ids -1, n, n + 2 and 2^40 in either slot: the score is NaN, the kept rows are zeros, ok is 0, the status bit is raised
    (and consumed here); the valid pairs around them are scored as ever, the same bits from both entry points."""
    rng = np.random.default_rng(100 + dim + slot)
    n, m = 37, 11
    emb, emb_d = sliced(rng, n, dim, "odd_stride", device)
    idx = list(pair_ids(rng, n, m))
    idx[slot][[1, 4, 6, 10]] = [-1, n, n + 2, 2 ** 40]
    ref, mag, rows0, rows1, ok = tgs.pair_scores_ref(emb, idx[0], idx[1])
    assert ok.sum() == m - 4
    i0, i1 = to_dev(idx[0], device), to_dev(idx[1], device)
    plain = OPS.pair_scores(emb_d, i0, i1)
    with pytest.raises(IndexError):
        lg.check_index_status()
    lg.check_index_status()            # consumed
    scores, r0, r1, okd = OPS.pair_scores_rows(emb_d, i0, i1)
    with pytest.raises(IndexError):
        lg.check_index_status()
    valid = torch.from_numpy(ok != 0)
    for got in (plain.cpu(), scores.cpu()):
        assert bool(torch.isnan(got[~valid]).all()) and not bool(torch.isnan(got[valid]).any())
        within("pair_scores", np.abs(got.numpy().astype(np.float64) - ref)[ok != 0], tgs.pair_scores_bound(dim, mag)[ok != 0],
               f"dim {dim} invalid ids in slot {slot}")
    assert torch.equal(bits(plain.cpu()[valid]), bits(scores.cpu()[valid]))
    assert torch.equal(r0.cpu(), torch.from_numpy(rows0)) and torch.equal(r1.cpu(), torch.from_numpy(rows1))
    assert not bool(r0.cpu()[~valid].any()) and not bool(r1.cpu()[~valid].any())
    assert torch.equal(okd.cpu(), torch.from_numpy(ok))


@pytest.mark.parametrize("m", [1, 257, 1025])
@pytest.mark.parametrize("dim", [1, 7, 90, 256])
def test_pair_seed_vals_are_two_rounded_multiplies(device, dim, m):
    rng = np.random.default_rng(dim * 7 + m)
    rows0, rows1 = tgs.f32(rng.standard_normal((m, dim))), tgs.f32(rng.standard_normal((m, dim)))
    gs = tgs.f32(rng.standard_normal(m))
    r0, r1, gd = to_dev(rows0, device), to_dev(rows1, device), to_dev(gs, device)
    for mask in (None, (rng.random(m) < 0.6).astype(np.uint8)):
        for scale in (None, np.float32(0.37)):
            got = OPS.pair_seed_vals(gd, None if mask is None else to_dev(mask, device),
                                     None if scale is None else torch.tensor(float(scale), device=device), r0, r1)
            want = tgs.pair_seed_vals_ref(gs, mask, scale, rows0, rows1)
            assert got.shape == (2 * m, dim)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), f"dim {dim} m {m} mask {mask is not None} scale {scale}"


# ----------------------------------------------------------------------------------------
# BPR loss
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 3000, 8192])
def test_bpr_loss_and_gradient(device, b):
    """lgc_bpr_loss: one workgroup of 1024 threads striding the batch -- batches on both sides of one, two and several trips,
    differences out to where expf overflows and beyond, every kind of mask, NaN scores under mask-off bytes."""
    rng = np.random.default_rng(b)
    s = tgs.bpr_scores(rng, b)
    last = np.zeros(b, dtype=np.uint8)
    last[-1] = 1
    random_mask = (rng.random(b) < 0.4).astype(np.uint8)
    poisoned = s.copy()                                   # what an out-of-range pair leaves behind: NaN under a mask-off byte
    off = np.flatnonzero(random_mask == 0)
    poisoned[off[::2]] = np.nan
    poisoned[b + off[1::2]] = np.nan
    cases = [("no mask", s, None), ("random mask", s, random_mask), ("all off", s, np.zeros(b, dtype=np.uint8)),
             ("last only", s, last), ("nan under off", poisoned, random_mask)]
    for size in sorted({1, b, 1024}):
        for name, scores, mask in cases:
            case = f"B {b} size {size} {name}"
            sd, md = to_dev(scores, device), None if mask is None else to_dev(mask, device)
            loss, grad = OPS.bpr_loss(sd, md, size)
            loss2, grad2 = OPS.bpr_loss(sd, md, size)
            assert torch.equal(bits(loss.view(1)), bits(loss2.view(1))) and torch.equal(bits(grad), bits(grad2)), case
            ref_loss, ref_grad = tgs.bpr_ref(scores, mask, size)
            got_loss, got_grad = float(loss.item()), grad.cpu().numpy().astype(np.float64)
            assert np.isfinite(got_loss) and np.isfinite(got_grad).all(), case
            within("bpr_grad", np.abs(got_grad - ref_grad), tgs.bpr_grad_bound(ref_grad, size), case)
            within("bpr_loss", abs(got_loss - ref_loss), abs(ref_loss) * tgs.bpr_loss_bound(b), case)
            assert torch.equal(grad[b:], -grad[:b]), case
            if mask is not None:
                assert not got_grad[:b][mask == 0].any() and not got_grad[b:][mask == 0].any(), case
                if not mask.any():
                    assert got_loss == 0.0, case


# ----------------------------------------------------------------------------------------
# regulariser
# ----------------------------------------------------------------------------------------
REG_LISTS = [(0, 0, 0), (1, 0, 0), (0, 0, 5), (341, 342, 342), (1024, 1024, 1024), (1000, 3, 2100)]


@pytest.mark.parametrize("dim", [1, 2, 3, 4, 5, 7, 64, 90, 129, 256])
def test_reg_rows_value_and_row_list(device, dim):
    """lgc_reg_rows: a thread per row with 16-byte loads at 4-byte alignment and a scalar tail, 1024 threads striding 3 B rows
    -- widths on both sides of the vector loop, strides that misalign the rows, list lengths up to several trips, wrapping
    negative ids and duplicates."""
    rng = np.random.default_rng(dim)
    n, scale = 500, 0.5 * 1e-4 / 1024
    for layout in LAYOUTS:
        w, w_d = sliced(rng, n, dim, layout, device, scale=0.1)
        for lens in REG_LISTS:
            case = f"dim {dim} {layout} lists {lens}"
            lists = [rng.integers(-n, n, size=k).astype(np.int64) for k in lens]
            if lens[0] > 2:
                lists[0][1] = lists[0][0]
            ref, rows = tgs.reg_rows_ref(w, lists, scale)
            dl = [to_dev(x, device) for x in lists]
            value, rows_out = OPS.reg_rows(w_d, dl, scale)
            value2, _ = OPS.reg_rows(w_d, dl, scale)
            assert torch.equal(bits(value.view(1)), bits(value2.view(1))), case
            assert torch.equal(rows_out.cpu(), torch.from_numpy(rows)) and (rows >= 0).all(), case
            within("reg_rows", abs(float(value.item()) - ref), abs(ref) * tgs.reg_rows_bound(dim, sum(lens)), case)
    lg.check_index_status()


@pytest.mark.parametrize("dim", [3, 90])
def test_reg_rows_of_ids_outside_the_table(device, dim):
    rng = np.random.default_rng(dim)
    n, scale = 500, 0.25
    w, w_d = sliced(rng, n, dim, "odd_stride", device)
    lists = [rng.integers(-n, n, size=k).astype(np.int64) for k in (1000, 3, 2100)]
    lists[0][[0, 999]] = [n, -n - 1]
    lists[1][1] = 2 ** 40
    lists[2][[5, 1500, 2099]] = [-(2 ** 40), n + 2, -n - 3]
    ref, rows = tgs.reg_rows_ref(w, lists, scale)
    assert (rows < 0).sum() == 6
    value, rows_out = OPS.reg_rows(w_d, [to_dev(x, device) for x in lists], scale)
    with pytest.raises(IndexError):
        lg.check_index_status()
    assert torch.equal(rows_out.cpu(), torch.from_numpy(rows))
    within("reg_rows", abs(float(value.item()) - ref), abs(ref) * tgs.reg_rows_bound(dim, 3103), f"dim {dim} invalid ids")


# ----------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 2, 3, 4, 5, 7, 2051, 100003])
def test_adam_over_flat_ranges(device, length):
    """lgc_adam_step_hp over [start, start + length) of four flat tables: a head launch up to the 16-byte line, a float4 body, a
    scalar tail -- every start inside a line, lengths shorter than the head; lgc_adam_step (scalars by value) gives the same
    bits."""
    lib = _native.load()
    for start in (0, 1, 2, 3):
        for step in (1, 1000):
            case = f"start {start} length {length} t {step}"
            rng = np.random.default_rng(length * 8 + start * 2 + (step > 1))
            total = start + length + 6
            tables = tgs.adam_inputs(rng, total)
            hyper = tgs.adam_hyper(step)
            lo, hi = start, start + length
            dev = [to_dev(x, device) for x in tables]
            OPS.adam_rows(*dev, lo, hi, to_dev(hyper, device))
            w1, m1, v1 = tgs.adam_ref(*(x[lo:hi] for x in tables), hyper)
            bw, bm, bv = tgs.adam_bounds(*(x[lo:hi] for x in tables), hyper)
            got_w, got_g, got_m, got_v = (x.cpu().numpy() for x in dev)
            within("adam_m", tgs.adam_errors(got_m[lo:hi], m1), bm, case)
            within("adam_v", tgs.adam_errors(got_v[lo:hi], v1), bv, case)
            within("adam_w", tgs.adam_errors(got_w[lo:hi], w1), bw, case)
            outside = np.ones(total, dtype=bool)
            outside[lo:hi] = False
            for got, was in zip((got_w, got_g, got_m, got_v), tables):
                assert np.array_equal(got.view(np.int32)[outside], was.view(np.int32)[outside]), case
            assert np.array_equal(got_g.view(np.int32), tables[1].view(np.int32)), case
            by_value = [to_dev(x, device) for x in tables]
            with torch.cuda.device(device):
                code = lib.lgc_adam_step(*(_native.ptr(x) + 4 * lo for x in by_value), length, *(float(h) for h in hyper),
                                         _native.stream_of(torch.device(device)))
            _native.check(code, "lgc_adam_step")
            for a, b in zip(by_value, dev):
                assert torch.equal(bits(a), bits(b)), case


# ----------------------------------------------------------------------------------------
# segment sums, seed preparation, linear combinations
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 6, 129, 130, 255, 256])
def test_segment_sum_into_a_column_slice(device, dim):
    """lgc_segment_sum on the run layout of test_segment_sum_is_a_fixed_order_run_sum plus a head at the last position, keys
    below zero and at 2^62, the output a column slice of a wider table, the values through a permutation."""
    rng = np.random.default_rng(dim)
    keys, dest = tgs.segment_layout()
    n = keys.size
    vals = tgs.f32(rng.standard_normal((n, dim)))
    perm = rng.permutation(n).astype(np.int32)
    shuffled = np.empty_like(vals)
    shuffled[perm] = vals                                      # vals[t] = shuffled[perm[t]]
    wide, offset = tgs.column_slice(rng, tgs.SEGMENT_ROWS, dim, dim + 5, 2)
    kd, dd = to_dev(keys, device), to_dev(dest, device)
    for scale, acc in ((1.0, False), (0.125, True)):
        want = wide.copy()
        want[:, offset:offset + dim] = tgs.segment_sum_ref(keys, dest, vals, None, wide[:, offset:offset + dim], scale, acc)
        for table, index in ((vals, None), (shuffled, perm)):
            base = to_dev(wide, device)
            propagate.segment_sum(kd, dd, to_dev(table, device), base[:, offset:offset + dim], scale=scale, accumulate=acc,
                                  vals_index=None if index is None else to_dev(index, device))
            assert torch.equal(base.cpu(), torch.from_numpy(want)), f"dim {dim} scale {scale} accumulate {acc} index {index is not None}"


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 8191, 8192])
def test_seed_prepare_and_flags_at_every_slice_boundary(device, m):
    """lgc_seed_prepare ranks by counting over slices of whole uint4s, eight keys per workgroup: list lengths around every
    multiple of 4, 8, 128 and 256, against a stable argsort; lgc_seed_flags sets and clears the flags of the user rows."""
    n = 10000
    for split in (0, 8400, n):
        for pattern in tgs.SEED_PATTERNS:
            case = f"m {m} split {split} {pattern}"
            rng = np.random.default_rng(m * 31 + split)
            rows = tgs.seed_rows(pattern, m, split, n, rng)
            want = tgs.seed_prepare_ref(rows, split, n)
            flag = torch.zeros(split + 1, dtype=torch.uint8, device=device)
            slot = torch.full((split + 1,), -7, dtype=torch.int32, device=device)
            got = OPS.seed_prepare(to_dev(rows, device), split, n, flag, slot)
            for g, name in zip(got, ("rows_sorted", "perm", "dest_item", "dest_slot", "dest_user")):
                w = torch.from_numpy(want[name])
                assert g.dtype == w.dtype and torch.equal(g.cpu(), w), f"{case}: {name}"
            assert torch.equal(flag.cpu(), torch.from_numpy(want["flag"])), case
            assert torch.equal(slot.cpu(), torch.from_numpy(want["slot"])), case
            OPS.seed_flags(got[0], split, flag, 5)
            assert torch.equal(flag.cpu(), torch.from_numpy(want["flag"] * 5)), case
            OPS.seed_flags(got[0], split, flag, 0)
            assert int(flag.sum()) == 0, case


@pytest.mark.parametrize("rows", [1, 3, 2100])
@pytest.mark.parametrize("dim", [1, 7, 90, 256])
def test_lincomb_of_one_to_eight_terms(device, dim, rows):
    """lgc_lincomb: fl(c0 s0) + fl(c1 s1) + ... in term order, bit for bit; sources of different row strides, a destination
    with padded rows (left alone between the rows); 2100 x 256 elements are past the grid's cap, so the loop takes a second trip."""
    rng = np.random.default_rng(dim + rows)
    coefs = [0.37, -1.25, 1.0, 0.2, 3.0, -0.001, 0.5, 7.0]
    src, src_d = [], []
    for t in range(8):
        wide, offset = tgs.column_slice(rng, rows, dim, dim + (t % 3) * (t + 1), (t % 3) * t // 2)
        src.append(wide[:, offset:offset + dim])
        src_d.append(to_dev(wide, device)[:, offset:offset + dim])
    wide, offset = tgs.column_slice(rng, rows, dim, dim + 3, 1)
    for terms in range(1, 9):
        want = wide.copy()
        want[:, offset:offset + dim] = tgs.lincomb_ref(list(zip(coefs[:terms], src[:terms])))
        y = to_dev(wide, device)
        OPS.lincomb(y[:, offset:offset + dim], list(zip(coefs[:terms], src_d[:terms])))
        assert torch.equal(y.cpu(), torch.from_numpy(want)), f"dim {dim} rows {rows} terms {terms} padded"
        dense = torch.empty(rows, dim, device=device)
        OPS.lincomb(dense, list(zip(coefs[:terms], src_d[:terms])))
        assert torch.equal(dense.cpu(), torch.from_numpy(want[:, offset:offset + dim])), f"dim {dim} rows {rows} terms {terms} dense"


# ----------------------------------------------------------------------------------------
# seeded pull
# ----------------------------------------------------------------------------------------
class PullCase:
    """The graph of tgs.pull_graph on the device: the item half of A^T under every plan of tgs.PULL_PLANS (what the pull
    runs), the user half of A (what names the rows to mark), and the CSR of A^T on the host for the reference."""

    def __init__(self, device):
        ei, ew, self.n_users, n_items = tgs.pull_graph()
        self.n = self.n_users + n_items
        self.graph = PropGraph(to_dev(ei, device), to_dev(ew, device), self.n)
        assert self.graph.split == self.n_users
        self.split = self.n_users
        item_t = self.graph.halves(True)[1]
        self.user_fwd = self.graph.halves(False)[0]
        self.rowptr = item_t.rowptr.cpu().numpy()
        self.cols = item_t.columns().cpu().numpy()
        self.vals = item_t.values().cpu().numpy()
        self.deg = np.diff(self.rowptr.astype(np.int64))[self.split:]
        assert sorted(self.deg.tolist()) == sorted(tgs.PULL_DEGREES)
        self.ops = {plan: Operator.build(self.n, item_t.rowptr, item_t.entries, self.split, self.n, plan[0], plan[1], tiles=False)
                    for plan in tgs.PULL_PLANS}
        self.seeds = tgs.pull_seeds(ei, self.n_users, n_items)


@pytest.fixture(scope="module")
def pull_case(device):
    return PullCase(device)


def test_pull_plans_hold_the_rows_they_are_meant_to(pull_case):
    counts = []
    for plan in tgs.PULL_PLANS:
        short, single, multi, chunks = tgs.plan_classes(pull_case.deg, *plan)
        p = pull_case.ops[plan].plan
        assert (p.n_chunks, p.n_multi, p.short_max) == (chunks, multi, plan[0]), plan
        if plan[0] >= 100000:
            assert short == pull_case.deg.size and chunks == 0          # the launch without a chunk part
        else:
            assert short > 0 and single > 0 and multi > 0, plan
        counts.append(chunks)
    assert any(0 < c < 16 for c in counts) and any(c > 16 for c in counts) and any(c % 16 for c in counts), counts


PULL_DIMS = [((4, 16), d) for d in (1, 2, 3, 4, 5, 7, 16, 64, 65, 90, 128, 129, 256)] + [
    (plan, d) for plan in tgs.PULL_PLANS if plan != (4, 16) for d in (3, 64, 90)]


@pytest.mark.parametrize("plan,dim", PULL_DIMS, ids=[f"short{p[0]}_chunk{p[1]}_d{d}" for p, d in PULL_DIMS])
def test_seed_pull_directly(device, pull_case, plan, dim):
    """lgc_seed_pull as the seeded backward calls it -- seeds prepared by lgc_seed_prepare / lgc_segment_sum into a compact
    table, rows marked by lgc_seed_mark -- in its three launch shapes (marks and chunks, no marks, no chunks), with the
    combine launch where rows have several chunks."""
    pc, op = pull_case, pull_case.ops[plan]
    n, split = pc.n, pc.split
    sentinel = 7.5
    for name, rows in pc.seeds.items():
        case = f"plan {plan} dim {dim} seeds {name}"
        rng = np.random.default_rng(dim)
        m = rows.size
        flag = torch.zeros(split + 1, dtype=torch.uint8, device=device)
        slot = torch.full((split + 1,), -7, dtype=torch.int32, device=device)
        rs, perm, _, dest_slot, _ = OPS.seed_prepare(to_dev(rows, device), split, n, flag, slot)
        gu = torch.full((max(m, 1), dim), float("nan"), device=device)         # rows that are no run head stay NaN: never read
        OPS.segment_sum(rs, dest_slot, to_dev(tgs.f32(rng.standard_normal((m, dim))), device), gu, vals_index=perm)
        mark = torch.zeros(n, dtype=torch.uint8, device=device)
        OPS.seed_mark(pc.user_fwd, rs, mark, 1)
        flag_h, slot_h, mark_h = flag.cpu().numpy(), slot.cpu().numpy(), mark.cpu().numpy()
        ref, mag, count = tgs.seed_pull_ref(pc.rowptr, pc.cols, pc.vals, split, n, flag_h, slot_h, gu.cpu().numpy())
        assert np.isfinite(ref).all(), case
        assert ((count > 0) <= (mark_h[split:] != 0)).all() and not mark_h[:split].any(), case
        if name == "one_user":                     # most rows of every class have no seed among their columns
            unmarked = pc.deg[mark_h[split:] == 0]
            assert 0 < mark_h.sum() and all(2 * ((unmarked >= lo) & (unmarked <= hi)).sum() > ((pc.deg >= lo) & (pc.deg <= hi)).sum()
                                            for lo, hi in ((1, 10), (33, 70), (300, 700))), case
        if name == "none":
            assert not mark_h.any() and not flag_h.any()
        for padded in (False, True):
            outs = []
            for marks in (mark, None, mark):
                out = propagate.scratch_table(torch.empty(n, dim, device=device)) if padded else torch.empty(n, dim, device=device)
                whole = out._base if out._base is not None else out
                whole.fill_(sentinel)
                propagate._seed_pull(op, flag, slot, gu, out, marks)
                assert bool((out[:split] == sentinel).all()) and bool((whole[:, dim:] == sentinel).all()), case
                outs.append(out[split:].contiguous())
            assert torch.equal(bits(outs[0]), bits(outs[1])), f"{case}: the marked pull and the full pull differ in bits"
            assert torch.equal(bits(outs[0]), bits(outs[2])), f"{case}: two calls differ in bits"
            got = outs[0].cpu().numpy()
            within("seed_pull", np.abs(got.astype(np.float64) - ref), tgs.seed_pull_bound(mag, count), f"{case} padded {padded}")
            for o in outs[:2]:
                assert not bits(o).cpu().numpy()[mark_h[split:] == 0].any(), f"{case}: an unmarked row is not +0"
                assert not bits(o).cpu().numpy()[count == 0].any(), f"{case}: a row without a flagged column is not +0"
        OPS.seed_flags(rs, split, flag, 0)
        OPS.seed_mark(pc.user_fwd, rs, mark, 0)
        assert int(flag.sum()) == 0 and int(mark.sum()) == 0, case
