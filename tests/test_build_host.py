"""The graph build's reference and cases, checked on the host (tests/build_support.py; the device side is
tests/test_build_gpu.py): the numpy fp32 restatement is right, the cases can tell a subtly wrong kernel from a right
one, the comparison notices each such kernel, and the argument codes that return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import build_support as B
from build_support import F32
from oracle import lightgcn_oracle as oracle

from gnn_ecommerce_amd import _native


def f32(*v):
    return np.array(v, dtype=F32)


# ----------------------------------------------------------------------------------------
# the reference is right
# ----------------------------------------------------------------------------------------
def test_by_hand_weighted_graph():
    """Five edges whose degrees are powers of four, so every value is exact and can be written out."""
    #            e0   e1   e2    e3   e4
    src = [2, 0, 1, 1, 3]
    dst = [1, 1, 0, 2, 2]
    w = f32(3.0, 1.0, 0.25, 16.0, 0.0)
    ei = torch.tensor([src, dst])
    r = B.build_ref(ei, torch.from_numpy(w), 4, by_source=False, normalize=True)
    assert r.rowptr.tolist() == [0, 1, 3, 5, 5]
    assert r.cols.tolist() == [1, 2, 0, 1, 3]                     # row 0: e2; row 1: e0, e1; row 2: e3, e4
    assert r.deg.tolist() == [0.25, 4.0, 16.0, 0.0] and r.dis.tolist() == [2.0, 0.5, 0.25, 0.0]
    assert r.vals.tolist() == [0.25, 0.375, 1.0, 2.0, 0.0]        # e.g. e0: dis[2] * 3 * dis[1] = 0.25 * 3 * 0.5
    assert r.edge_val.tolist() == [0.375, 1.0, 0.25, 2.0, 0.0]
    t = B.build_ref(ei, torch.from_numpy(w), 4, by_source=True, normalize=True, dis_in=r.dis)
    assert t.rowptr.tolist() == [0, 1, 3, 4, 5]
    assert t.cols.tolist() == [1, 0, 2, 1, 2]                     # source 0: e1; source 1: e2, e3; source 2: e0; source 3: e4
    assert t.vals.tolist() == [1.0, 0.25, 2.0, 0.375, 0.0] and t.deg is None and t.dis is None
    assert np.array_equal(t.edge_val, r.edge_val)
    raw = B.build_ref(ei, torch.from_numpy(w), 4, by_source=False, normalize=False)
    assert raw.vals.tolist() == [0.25, 3.0, 1.0, 16.0, 0.0] and raw.deg is None


def test_by_hand_unweighted_duplicates():
    """edge_weight = None is ones; a duplicate edge counts twice and keeps its place."""
    ei = torch.tensor([[0, 0, 2, 1], [1, 1, 1, 0]])
    r = B.build_ref(ei, None, 3, by_source=False, normalize=True)
    third = 0x3F13CD3A                                            # fl(1 / fl(sqrt(3))) = 0.57735026
    assert r.rowptr.tolist() == [0, 1, 4, 4] and r.cols.tolist() == [1, 0, 0, 2]
    assert r.deg.tolist() == [1.0, 3.0, 0.0]
    assert B.bits(r.dis).tolist() == [0x3F800000, third, 0]
    assert B.bits(r.vals).tolist() == [third, third, third, 0]    # node 2 has no incoming edge: dis 0, its edge is worth 0
    assert B.bits(r.edge_val).tolist() == [third, third, 0, third]


def test_by_hand_parked_edge():
    """An edge with an endpoint outside [0, n) sits in row 0 in its place in edge order as (0, +0.0)."""
    ei = torch.tensor([[0, 5, 1, 0], [1, 1, 0, 0]])
    r = B.build_ref(ei, torch.from_numpy(f32(2.0, 3.0, 4.0, 5.0)), 2, by_source=False, normalize=False)
    assert r.rowptr.tolist() == [0, 3, 4]
    assert r.cols.tolist() == [0, 1, 0, 0] and r.vals.tolist() == [0.0, 4.0, 5.0, 2.0]
    assert r.edge_val.tolist() == [2.0, 0.0, 4.0, 5.0] and B.bits(r.edge_val)[1] == 0


def _non_nan_ulp(a, b):
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)), "NaNs must sit in the same positions"
    return int(B.ulp_distance(a[~nan], b[~nan]).max()) if (~nan).any() else 0


def test_reference_against_the_oracle():
    """``build_ref`` against ``oracle.gcn_norm`` (torch CPU; its ``pow(-0.5)`` is a vectorised rsqrt, which is what the
    project's 4-ulp allowance is for).  Measured maximum per generator on the build machine: 0 ulp for each of them --
    degree lengths, both order-matters graphs, the nine key widths, the six edge counts, the mixed values (NaNs in the same
    places) and the tiny / huge weights -- and 0 on ``synth``'s small_graph(0): this torch's CPU ``pow`` is exact here."""
    worst = {}
    for name, case in B.forward_cases().items():
        want = oracle.gcn_norm(case.edge_index, case.edge_weight, case.n).numpy()
        got = B.forward_ref(name)
        worst[name] = _non_nan_ulp(got.edge_val, want)
        order = np.argsort(case.edge_index[1].numpy(), kind="stable")
        assert np.array_equal(got.cols, case.edge_index[0].numpy()[order])
        assert _non_nan_ulp(got.vals, want[order]) == worst[name]
    print("max ulp of build_ref against oracle.gcn_norm:", worst)
    assert max(worst.values()) <= 4, worst
    from gnn_ecommerce_amd import synth
    ei, ew = synth.make_bipartite(300, 80, 2000, 0).coo()
    assert _non_nan_ulp(B.build_ref(ei, ew, 380, False, True).edge_val, oracle.gcn_norm(ei, ew, 380).numpy()) <= 4


def test_reference_degree_is_the_sequential_chain():
    """Equal to ``scatter_add_`` on zeros (sequential on the CPU) for every case, and to a plain Python loop."""
    for name, case in B.forward_cases().items():
        w = torch.from_numpy(case.weights())
        want = torch.zeros(case.n).scatter_add_(0, case.edge_index[1], w).numpy()
        assert np.array_equal(B.bits(B.forward_ref(name).deg), B.bits(want)), name
    for name in ("degree_lengths", "order_matters_small_first", "values_mixed"):
        case = B.forward_cases()[name]
        acc = [F32(0.0)] * case.n
        for d, wv in zip(case.edge_index[1].tolist(), case.weights()):
            acc[d] = F32(acc[d] + wv)
        assert np.array_equal(B.bits(B.forward_ref(name).deg), B.bits(np.array(acc, F32))), name


@pytest.mark.parametrize("name", B.POSITIVE_NAMES)
def test_reference_against_fp64_within_the_rounding_count(name):
    """Positive weights: each value within gamma(k) of the fp64 evaluation, k counted in ``value_bound_roundings``."""
    case, ref = B.forward_cases()[name], B.forward_ref(name)
    assert (case.weights() > 0).all()
    deg64, dis64, val64 = B.build_fp64(case.edge_index, case.edge_weight, case.n)
    length = np.diff(ref.rowptr.astype(np.int64))
    assert (np.abs(ref.deg - deg64) <= np.array([B.gamma(max(l - 1, 0)) for l in length]) * deg64).all()
    assert (np.abs(ref.dis - dis64) <= np.array([B.gamma(-(-max(l - 1, 0) // 2) + 3) for l in length]) * dis64).all()
    src, dst = case.edge_index.numpy()
    k = np.array([B.value_bound_roundings(a, b) for a, b in zip(length[src], length[dst])])
    err = np.abs(ref.edge_val.astype(np.float64) - val64)
    assert (err <= B.gamma(k) * val64).all(), float((err / np.maximum(B.gamma(k) * val64, 1e-300)).max())
    assert np.isfinite(ref.edge_val).all()


def test_tiny_and_huge_weights_stay_normal():
    ref = B.forward_ref("values_tiny_huge")
    tiny = float(np.finfo(F32).tiny)
    for a in (ref.deg, ref.dis, ref.vals):
        assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all()
    assert (ref.vals > 0).all() and ref.vals.max() <= 1.0


def test_value_cases_hold_what_they_claim():
    case, ref = B.forward_cases()["values_mixed"], B.forward_ref("values_mixed")
    src, dst = case.edge_index.numpy()
    w = case.weights()
    for node in (B.V_ZERO, B.V_CANCEL, B.V_LONE_MINUS_ZERO):
        assert B.bits(ref.deg)[node] == 0 and B.bits(ref.dis)[node] == 0 and (dst == node).sum() >= 1
    assert (w[dst == B.V_ZERO] == 0).all() and (w[dst == B.V_CANCEL] != 0).all()
    assert ref.deg[B.V_NEG] < 0 and np.isnan(ref.dis[B.V_NEG]) and np.isnan(ref.dis).sum() == 1
    touches = (src == B.V_NEG) | (dst == B.V_NEG)
    assert np.array_equal(np.isnan(ref.edge_val), touches) and touches.sum() >= 5
    into_zero = (dst == B.V_ZERO) & ~touches
    assert (B.bits(ref.edge_val)[into_zero] == 0).all()                       # +0.0, not NaN, not -0.0
    lone = dst == B.V_LONE_MINUS_ZERO
    assert lone.sum() == 1 and B.bits(w)[lone][0] == -2 ** 31 and B.bits(ref.edge_val)[lone][0] == -2 ** 31
    assert (B.bits(w)[dst == B.V_MINUS_ZERO] == -2 ** 31).sum() == 1 and ref.deg[B.V_MINUS_ZERO] > 0
    assert ((src == B.V_LOOP) & (dst == B.V_LOOP)).sum() == 2
    for node in B.V_ISOLATED:
        assert not ((src == node) | (dst == node)).any() and ref.rowptr[node] == ref.rowptr[node + 1]
    den = B.denormal_case()
    r = den.ref()
    tiny = float(np.finfo(F32).tiny)
    assert (den.weights() < tiny).all() and (r.deg[r.deg > 0] < tiny).all() and (r.deg > 0).sum() == 4
    assert (r.vals >= tiny).all() and (r.dis[r.deg > 0] > 1e19).all()
    raw = B.raw_weights_case()
    assert set(raw.weights().view(np.uint32).tolist()) == set(B.RAW_BITS.tolist())
    assert np.array_equal(raw.ref(normalize=False).edge_val.view(np.uint32), raw.weights().view(np.uint32))


def test_case_shapes():
    case = B.forward_cases()["degree_lengths"]
    ref = B.forward_ref("degree_lengths")
    length = np.diff(ref.rowptr.astype(np.int64))
    assert case.n % B.ROWS_PER_WAVE_BLOCK != 0 and 11000 <= case.edge_index.size(1) <= 13000
    assert sorted(set(B.DEGREE_LENGTHS)) == sorted(B.DEGREE_ROWS) and len(set(B.DEGREE_ROWS.values())) == len(B.DEGREE_ROWS)
    for l, r in B.DEGREE_ROWS.items():
        assert length[r] == l
    long_rows = sorted(r for l, r in B.DEGREE_ROWS.items() if l > B.SERIAL_MAX)
    assert long_rows[-1] == case.n - 1
    assert all(r % 4 in (0, 3) for r in long_rows[:-1]) and {r % 4 for r in long_rows[:-1]} == {0, 3}
    assert not np.array_equal(np.sort(case.edge_index[1].numpy()), case.edge_index[1].numpy()), "edges must be shuffled"
    src, dst = case.edge_index.numpy()
    for l, r in B.DEGREE_ROWS.items():
        if l >= 2:                                                # a duplicate (src, dst) pair with different weights
            s, w = src[dst == r], case.weights()[dst == r]
            assert any(len(set(w[s == v].tolist())) >= 2 for v in np.unique(s)), l
    for rev in ("big_first", "small_first"):
        c = B.forward_cases()["order_matters_" + rev]
        rows = B.rows_in_edge_order(c)
        assert sorted(len(w) for w in rows.values()) == sorted(B.ORDER_LENGTHS)
        for w in rows.values():
            assert w[0 if rev == "big_first" else -1] == F32(1e4) and (np.delete(w, 0 if rev == "big_first" else -1) == F32(1e-4)).all()
        assert not np.array_equal(np.sort(c.edge_index[1].numpy()), c.edge_index[1].numpy())
    for n in B.KEY_WIDTH_N:
        c = B.forward_cases()[f"key_width_n{n}"]
        ids = c.edge_index.numpy()
        assert ids.min() == 0 and ids.max() == n - 1 and ids.shape[1] == 3000
        for row in ids:
            assert {0, n // 2, n - 1} <= set(row.tolist())
    assert [B.forward_cases()[f"edge_count_e{e}"].edge_index.size(1) for e in B.EDGE_COUNTS] == list(B.EDGE_COUNTS)
    oob = B.out_of_range_case()
    bad = oob.edge_index[:, torch.from_numpy(~oob.valid)]
    assert sorted(bad[(bad < 0) | (bad >= oob.n)].tolist()) == sorted(oob.n if b is None else b for b in B.BAD_IDS)
    assert ((bad[0] < 0) | (bad[0] >= oob.n)).sum() == 3 and not (bad == 0).any()
    assert torch.equal(oob.edge_index[:, torch.from_numpy(oob.valid)], oob.clean.edge_index)


# ----------------------------------------------------------------------------------------
# the cases discriminate
# ----------------------------------------------------------------------------------------
def test_long_rows_tell_the_sequential_sum_from_every_other():
    """Every row longer than 500 entries of the degree-length graph (seed ``DEGREE_SEED``, chosen for this) and of the
    order-matters graph that starts each row with 1e4: the sequential fp32 sum differs in bits from the fp64 sum rounded to
    fp32, from the per-64-block partial sums added up and from the 64-lane-strided partial sums.

    The second order-matters graph (1e4 LAST) cannot meet that condition and is not asked to: its small weights are summed
    first, to within 1e-7 of their exact sum, and then rounded once at the ulp of 1e4 (2^-10) -- the sequential sum IS the
    correctly rounded sum there, equal to the fp64 one for every length.  What that graph is for is the direction: its
    degree differs from the first graph's on every row, so a kernel that walks a row backwards fails on both."""
    checked = 0
    for name in ("degree_lengths", "order_matters_big_first"):
        ref = B.forward_ref(name)
        for r, w in B.rows_in_edge_order(B.forward_cases()[name]).items():
            if len(w) <= B.LONG_ROW_MIN:
                continue
            seq = B.step_row_sum(w)
            assert B.bits(seq) == B.bits(ref.deg)[r]
            for how, f in B.WRONG_SUMS.items():
                assert B.bits(f(w)) != B.bits(seq), f"{name}: the {how} sum of the {len(w)}-entry row equals the chain"
            checked += 1
    assert checked == 2 * len(B.ORDER_LENGTHS)
    big, small = B.forward_ref("order_matters_big_first"), B.forward_ref("order_matters_small_first")
    for l, r in B.ORDER_ROWS.items():
        assert big.deg[r] == F32(1e4) and small.deg[r] > F32(1e4) and small.deg[r] == B.sum_fp64_rounded(
            B.rows_in_edge_order(B.forward_cases()["order_matters_small_first"])[r])
        w = B.rows_in_edge_order(B.forward_cases()["order_matters_small_first"])[r]
        assert B.step_row_sum(w[::-1]) == big.deg[r]


# ----------------------------------------------------------------------------------------
# the comparison notices
# ----------------------------------------------------------------------------------------
def end_bit_for(n):
    bits = 1
    while bits < 31 and (1 << bits) < n:
        bits += 1
    return bits


def test_comparison_passes_on_equal_builds_and_sees_signed_zero_and_nan():
    for name in B.FORWARD_NAMES:
        assert B.mismatches(B.forward_cases()[name].ref(), B.forward_ref(name)) == []
    a, b = f32(0.0, 1.0, np.nan), f32(-0.0, 1.0, np.nan)
    assert B.same_floats(a, b).tolist() == [False, True, True]
    quiet = np.array([0x7FC00000, 0xFFC00001], dtype=np.uint32).view(F32)
    assert B.same_floats(quiet[:1], quiet[1:]).all() and not B.same_floats(quiet[:1], quiet[1:], exact_nan=True).any()
    assert not B.same_floats(f32(np.nan), f32(1.0)).any()


def test_comparison_notices_an_unstable_sort():
    for name in ("degree_lengths", "key_width_n257"):
        wrong = B.forward_cases()[name].ref(steps=dict(order=lambda key: np.lexsort((-np.arange(len(key)), key))))
        bad = B.mismatches(wrong, B.forward_ref(name))
        assert "vals" in bad and "cols" in bad and "rowptr" not in bad and "deg" in bad, bad
    # duplicate pairs alone: same columns, the weights swapped
    case = B.forward_cases()["degree_lengths"]
    ref = B.forward_ref("degree_lengths")
    r = B.DEGREE_ROWS[2]
    swapped = B.SimpleNamespace(**vars(ref))
    swapped.vals = ref.vals.copy()
    lo = ref.rowptr[r]
    swapped.vals[[lo, lo + 1]] = ref.vals[[lo + 1, lo]]
    assert ref.cols[lo] == ref.cols[lo + 1] and B.mismatches(swapped, ref) == ["vals"] and case.n > r


@pytest.mark.parametrize("n", (257, 65537))
def test_comparison_notices_a_key_bit_too_few(n):
    mask = (1 << (end_bit_for(n) - 1)) - 1
    assert (n - 1) & mask != n - 1 and (n - 2) & mask == n - 2
    name = f"key_width_n{n}"
    wrong = B.forward_cases()[name].ref(steps=dict(order=lambda key: np.argsort(key & mask, kind="stable")))
    bad = B.mismatches(wrong, B.forward_ref(name))
    assert "cols" in bad and "vals" in bad, bad
    assert [end_bit_for(m) for m in (1, 2, 3, 255, 256, 257, 65535, 65536, 65537)] == [1, 1, 2, 8, 8, 9, 16, 16, 17]


def test_comparison_notices_ids_cast_to_int32_before_the_range_check():
    case = B.out_of_range_case()

    ei32 = case.edge_index.to(torch.int32).to(torch.int64)        # what a kernel sees that truncates before it checks
    _, ok = B.step_keys(*ei32.numpy(), case.n, False)
    assert (~ok).sum() == 3, "2^32, 2^32 + 1 and INT64_MIN pass an int32 range check"
    ref = case.ref()
    bad = B.mismatches(B.build_ref(ei32, case.edge_weight, case.n, False, True), ref)
    assert "vals" in bad and "edge_val" in bad, bad
    true_key, true_ok = B.step_keys(*case.edge_index.numpy(), case.n, False)
    parked = ~true_ok[B.step_order(true_key)]
    assert np.array_equal(true_ok, case.valid) and parked.sum() == len(B.BAD_IDS)
    assert (np.flatnonzero(parked) < ref.rowptr[1]).all() and (ref.cols[parked] == 0).all()
    assert (B.bits(ref.vals)[parked] == 0).all() and (B.bits(ref.edge_val)[~case.valid] == 0).all()


def test_comparison_notices_wrong_arithmetic():
    case, ref = B.forward_cases()["degree_lengths"], B.forward_ref("degree_lengths")

    def dis_off(deg):
        d = B.step_dis(deg)
        d[B.DEGREE_ROWS[63]] = np.nextafter(d[B.DEGREE_ROWS[63]], F32(np.inf))
        return d
    bad = B.mismatches(case.ref(steps=dict(dis=dis_off)), ref)
    assert "dis" in bad and "vals" in bad and "deg" not in bad, bad

    bad = B.mismatches(case.ref(steps=dict(value=lambda ds, w, dd: (w * (ds * dd).astype(F32)).astype(F32))), ref)
    assert bad == ["vals", "edge_val"], bad

    for how, f in B.WRONG_SUMS.items():
        wrong = case.ref(steps=dict(row_sum=lambda w, f=f: f(w) if len(w) == 513 else B.step_row_sum(w)))
        bad = B.mismatches(wrong, ref)
        assert "deg" in bad, (how, bad)
        assert (B.bits(wrong.deg) != B.bits(ref.deg)).sum() == 1

    short = B.SimpleNamespace(**vars(ref))
    short.rowptr = ref.rowptr.copy()
    short.rowptr[-1] -= 1
    assert B.mismatches(short, ref) == ["rowptr"]


# ----------------------------------------------------------------------------------------
# argument codes that return before any launch
# ----------------------------------------------------------------------------------------
def test_build_argument_codes_before_any_launch():
    lib = _native.load()
    one, ws = ctypes.c_void_p(16), ctypes.c_void_p(256)           # never dereferenced
    need = lib.lgc_build_workspace_bytes(10, 5)
    assert need > 0

    def build(by_source=0, normalize=1, dis_in=None, deg=one, dis=one, ws_bytes=need - 1):
        return lib.lgc_build_csr(one, None, 10, 5, by_source, normalize, dis_in, one, one, None, deg, dis, ws, ws_bytes, one, None)
    assert build() == -3, "a workspace one byte short is LGC_E_WORKSPACE"
    assert build(by_source=1) == -1, "the A^T build needs dis_in"
    assert build(deg=None) == -1 and build(dis=None) == -1, "the first build writes deg and dis"
    assert build(deg=None, dis=None, dis_in=one) == -3, "with dis_in given neither is needed: the next check answers"
    assert build(deg=None, dis=None, normalize=0) == -3 and build(by_source=1, normalize=0) == -3
