"""The ranking metrics on the device: lgc_rank_metrics on synthetic top-k rows against the numpy restatement of
rank_metrics_support (one sweep at a time over rows, k, cutoffs and list lengths), lgc_column_sums, lgc_topk_coverage,
and evaluate_ranking / LightGCN.evaluate_metrics end to end.  Every top-k matrix is built on the host."""
import numpy as np
import pytest
import torch

from conftest import load_golden, t
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate
from gnn_ecommerce_amd.propagate import (PositiveLists, SeenLists, column_sums, evaluate_ranking, evaluate_topk, metric_sums,
                                         metrics_frame, overlap_items, rank_metrics, topk_coverage, topk_hits)
from rank_metrics_support import AP, HIT, N_ITEMS, NDCG, PRECISION, RECALL, RR, case, csr, reference, reference_frame

pytestmark = pytest.mark.gpu

# NDCG and AP against numpy, absolute, per element.  Derived, not measured: at most 256 terms of at most 1 each, so a
# running sum is off by at most 255 * 2^-53 * 256 ~ 7e-12, plus one ulp per table entry between two log2 implementations.
TOL = 1e-11
LENGTHS = (1, 63, 64, 65, 300)
EIGHT = (1, 2, 63, 64, 65, 128, 192, 256)


def strided(values: np.ndarray, pad: int, device) -> torch.Tensor:
    """``values`` as the leading columns of an int64 [rows, cols + pad] buffer whose other columns hold -7."""
    buf = torch.full((values.shape[0], values.shape[1] + pad), -7, dtype=torch.int64, device=device)
    buf[:, :values.shape[1]] = torch.from_numpy(values).to(device)
    return buf[:, :values.shape[1]]


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns: NaNs included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def same_bits_or_both_nan(a: np.ndarray, b: np.ndarray) -> bool:
    """NaN where the other has NaN (0 / 0 has no one bit pattern across implementations), the same bits elsewhere."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def run(device, c, pad=3):
    pos = PositiveLists.from_arrays(c["ptr"], c["items"], np.arange(c["n_users"]), device=device)
    top = strided(c["topk"], pad, device)
    users = torch.from_numpy(c["users"]).to(device)
    return (top, pos, users) + tuple(rank_metrics(top, pos, users, c["cutoffs"], return_bits=True))


def check_case(device, c):
    top, pos, users, hits, metrics, bits = run(device, c)
    n, k, cuts = c["topk"].shape[0], c["topk"].shape[1], c["cutoffs"]
    assert top.stride(0) == k + 3
    want_h, want_m, want_b = c["want"]
    assert hits.dtype == torch.int32 and hits.shape == (n, len(cuts)) and metrics.shape == (n, len(cuts), 6)
    # 1. integers are exact; precision, RR (one IEEE division each) and the hit flag bit for bit
    assert np.array_equal(hits.cpu().numpy(), want_h)
    got_b = bits.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_b, want_b)
    for q in range(4):                                                            # words past k are zero
        if 64 * q >= k:
            assert not got_b[:, q].any()
    m = metrics.cpu().numpy()
    for col in (PRECISION, RR, HIT, RECALL):
        assert same_bits_or_both_nan(m[..., col], want_m[..., col]), col
    if cuts[-1] == k:                                                             # ... and lgc_topk_hits' two columns
        h1, r1 = topk_hits(top, pos, users)
        assert torch.equal(hits[:, -1], h1) and bits_equal(metrics[:, -1, RECALL], r1)
    # 2. NDCG and AP within the derived bound
    assert np.array_equal(np.isnan(m), np.isnan(want_m))
    err = np.nan_to_num(np.abs(m[..., [NDCG, AP]] - want_m[..., [NDCG, AP]]), nan=0.0)
    print(f"rows {n} k {k} cutoffs {cuts}: worst NDCG / AP error {err.max():.3g}, {int(want_h[:, -1].sum())} hits")
    assert err.max() <= TOL
    assert np.all((m[..., NDCG][~np.isnan(m[..., NDCG])] <= 1.0 + TOL)) and np.all(m[..., AP][~np.isnan(m[..., AP])] <= 1.0 + TOL)
    # 4. determinism
    again = rank_metrics(top, pos, users, cuts, return_bits=True)
    assert torch.equal(again[0], hits) and bits_equal(again[1], metrics) and torch.equal(again[2], bits)
    # the list of hit items, from the bits
    assert overlap_items(top, bits) == [[int(x) for j, x in enumerate(row) if (int(b[j // 64]) >> (j % 64)) & 1]
                                        for row, b in zip(c["topk"], want_b)]
    lg.check_index_status(device)


@pytest.mark.parametrize("rows", [1, 4, 5, 17])
def test_rows_sweep(device, rows):
    check_case(device, case(rows, 20, (5, 10, 20), LENGTHS))


@pytest.mark.parametrize("k", [1, 20, 64, 65, 256])
def test_k_sweep(device, k):
    check_case(device, case(17, k, tuple(sorted({1, (k + 1) // 2, k})), LENGTHS))


@pytest.mark.parametrize("k,cutoffs", [(20, (1,)), (20, (5, 10, 20)), (256, EIGHT)])
def test_cutoff_sweep(device, k, cutoffs):
    check_case(device, case(17, k, cutoffs, LENGTHS, seed=1))


@pytest.mark.parametrize("length", LENGTHS)
def test_list_length_sweep(device, length):
    c = case(17, 65, (5, 64, 65), (length,), seed=2)
    if length > 1:
        assert (np.diff(c["ptr"]) == length).all() and len(set(c["items"][c["ptr"][1]:c["ptr"][2]].tolist())) == length - 1
    check_case(device, c)


def test_a_user_without_a_list_gives_nan_and_the_same_bits_twice(device):
    ptr, items = csr([[3, 4], [], [5]])
    topk = np.array([[3, 9, 4], [3, 9, 4], [5, 3, 9]], dtype=np.int64)
    c = dict(topk=topk, ptr=ptr, items=items, users=np.array([0, 1, 2]), cutoffs=(1, 3), n_users=3,
             want=reference(topk, ptr, items, [0, 1, 2], (1, 3)))
    assert np.isnan(c["want"][1][1][:, [RECALL, NDCG, AP]]).all()
    check_case(device, c)


def test_without_distinct_counts_the_list_length_is_used(device):
    """pos_distinct = NULL: lists without duplicates give the same bits as with the counts."""
    c = case(5, 20, (5, 20), (7, 30), seed=3)
    lists = [np.unique(c["items"][c["ptr"][u]:c["ptr"][u + 1]]) for u in range(c["n_users"])]
    ptr, items = csr(lists)
    pos = PositiveLists.from_arrays(ptr, items, np.arange(c["n_users"]), device=device)
    top, users = strided(c["topk"], 3, device), torch.from_numpy(c["users"]).to(device)
    hits, metrics = rank_metrics(top, pos, users, (5, 20))
    import ctypes
    arr = (ctypes.c_int32 * 2)(5, 20)
    h2, m2 = torch.empty_like(hits), torch.empty_like(metrics)
    code = _native.load().lgc_rank_metrics(top.data_ptr(), top.stride(0), 20, pos.ptr.data_ptr(), pos.items.data_ptr(), None,
                                           users.data_ptr(), 5, c["n_users"], arr, 2, None, h2.data_ptr(), m2.data_ptr(),
                                           propagate._status(device).data_ptr(), _native.stream_of(device))
    assert code == 0 and torch.equal(h2, hits) and bits_equal(m2, metrics)


# ---------------------------------------------------------------------------------------------------------------
# 3. prefix property
# ---------------------------------------------------------------------------------------------------------------
def test_a_cutoff_is_a_prefix_bit_for_bit(device):
    c = case(17, 20, (5, 10, 20), LENGTHS)
    top, pos, users, hits, metrics, bits = run(device, c)
    short = strided(c["topk"][:, :10], 5, device)
    h10, m10, b10 = rank_metrics(short, pos, users, (10,), return_bits=True)
    assert torch.equal(h10[:, 0], hits[:, 1]) and bits_equal(m10[:, 0], metrics[:, 1])
    assert torch.equal(b10[:, 0], bits[:, 0] & 0x3FF) and not b10[:, 1:].any()
    wide = case(17, 256, EIGHT, LENGTHS, seed=1)                        # ... and across a ballot word, out of eight cutoffs
    top, pos, users, hits, metrics, _ = run(device, wide)
    h65, m65 = rank_metrics(strided(wide["topk"][:, :65], 1, device), pos, users, (65,))
    assert torch.equal(h65[:, 0], hits[:, 4]) and bits_equal(m65[:, 0], metrics[:, 4])


def randn_tables(seed, n_users, n_items, dim, stride, device):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for rows in (n_users, n_items):
        buf = torch.full((rows, stride), float("nan"), device=device)
        buf[:, :dim] = torch.randn(rows, dim, generator=gen).to(device)
        out.append(buf[:, :dim])
    return out


def test_evaluate_ranking_reports_evaluate_topk_at_a_smaller_cutoff(device):
    n_users, n_items = 50, N_ITEMS
    ut, it = randn_tables(4, n_users, n_items, 90, 96, device)
    gen = torch.Generator().manual_seed(5)
    lists = [torch.randint(n_items, (int(torch.randint(1, 40, (1,), generator=gen)),), generator=gen).tolist() for _ in range(n_users)]
    seen_items = torch.stack([torch.randperm(n_items, generator=gen)[:6].sort().values for _ in range(n_users)])
    seen = SeenLists((torch.arange(n_users + 1) * 6).to(device), seen_items.reshape(-1).to(device)).validate(n_users)
    users = torch.randperm(n_users, generator=gen).to(device)
    pos = PositiveLists.from_lists(range(n_users), lists, n_users, device=device).validate(n_users, n_items)
    res = evaluate_ranking(ut, it, seen, users, pos, (5, 20), workspace_bytes=4 * n_items * 16)
    p5, r5, h5 = evaluate_topk(ut, it, seen, users, pos, 5)
    p20, r20, h20 = evaluate_topk(ut, it, seen, users, pos, 20)
    assert res.cutoffs == (5, 20) and res.topk.shape == (n_users, 20) and h20.sum().item() > 0
    assert torch.equal(res.hits[:, 0], h5) and torch.equal(res.hits[:, 1], h20)
    assert res.mean["precision"] == (p5, p20) and res.mean["recall"] == (r5, r20)
    for name in ("ndcg", "map", "mrr", "hit_rate", "coverage"):
        assert len(res.mean[name]) == 2 and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.mean[name])
    top = res.topk.cpu().numpy()
    assert res.mean["coverage"] == (len(np.unique(top[:, :5])) / n_items, len(np.unique(top)) / n_items)
    off = evaluate_ranking(ut, it, seen, users, pos, (5, 20), coverage=False)
    assert off.mean["recall"] == res.mean["recall"] and all(np.isnan(v) for v in off.mean["coverage"])
    none = evaluate_ranking(ut, it, seen, users[:0], pos, (5, 20))
    assert all(np.isnan(v) for name in propagate.METRIC_NAMES for v in none.mean[name]) and none.hits.shape == (0, 2)
    lg.check_index_status(device)


# ---------------------------------------------------------------------------------------------------------------
# 5. column sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [1, 6, 48])
def test_column_sums_against_fp64_torch_sum(device, n_cols):
    gen = torch.Generator().manual_seed(n_cols)
    for n_rows in (1, 1023, 1024, 1025, 5000):
        x = torch.randn(n_rows, n_cols, generator=gen, dtype=torch.float64)
        buf = torch.full((n_rows, n_cols + 5), float("nan"), dtype=torch.float64, device=device)
        buf[:, :n_cols] = x.to(device)
        got = column_sums(buf[:, :n_cols])
        assert got.shape == (n_cols,) and got.dtype == torch.float64
        bound = n_rows * 2.0 ** -53 * x.abs().sum(dim=0)
        err = (got.cpu() - x.sum(dim=0)).abs()
        print(f"{n_rows} x {n_cols}: worst error / bound = {(err / bound).max().item():.3g}")
        assert bool((err <= bound).all())
        assert torch.equal(got, column_sums(buf[:, :n_cols]))
        # a column has the bits of lgc_metric_sums' recall sum
        col = x[:, n_cols // 2].contiguous().to(device)
        want = metric_sums(torch.zeros(n_rows, dtype=torch.int32, device=device), col)[1:2].view(torch.float64)
        assert bits_equal(got[n_cols // 2:n_cols // 2 + 1], want)
    assert column_sums(torch.empty((0, n_cols), dtype=torch.float64, device=device)).tolist() == [0.0] * n_cols
    with pytest.raises(ValueError):
        column_sums(torch.zeros((3, 65), dtype=torch.float64, device=device))


# ---------------------------------------------------------------------------------------------------------------
# 6. coverage
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [1, 32, 33, 300])
def test_coverage_counts_accumulate_over_calls(device, n_items):
    rng = np.random.default_rng(n_items)
    k = min(n_items, 20)
    cuts = tuple(sorted({1, (k + 1) // 2, k}))
    topk = np.stack([rng.permutation(n_items)[:k] for _ in range(23)]).astype(np.int64)
    want = [len(np.unique(topk[:, :c])) for c in cuts]
    counts, bitmap = topk_coverage(strided(topk, 3, device), cuts, n_items)
    assert counts.dtype == torch.int64 and counts.tolist() == want
    assert bitmap.shape == (len(cuts), (n_items + 31) // 32)
    first, part = topk_coverage(strided(topk[:9], 3, device), cuts, n_items)
    assert first.tolist() == [len(np.unique(topk[:9, :c])) for c in cuts]
    second, part2 = topk_coverage(strided(topk[9:], 1, device), cuts, n_items, bitmap=part)
    assert part2 is part and second.tolist() == want and torch.equal(part, bitmap)
    empty, _ = topk_coverage(strided(topk[:0], 3, device), cuts, n_items, bitmap=part)     # no rows: the counts of what is there
    assert empty.tolist() == want
    lg.check_index_status(device)


def test_coverage_entry_out_of_range_flags_and_spares_its_neighbours(device):
    n_items, cuts = 300, (5, 20)
    topk = np.stack([np.random.default_rng(r).permutation(n_items)[:20] for r in range(6)]).astype(np.int64)
    clean, clean_map = topk_coverage(strided(topk, 3, device), cuts, n_items)
    lg.check_index_status(device)
    bad = topk.copy()
    bad[1, 2], bad[3, 0], bad[5, 19] = -1, n_items, 2 ** 40
    keep = np.ones_like(bad, dtype=bool)
    keep[1, 2] = keep[3, 0] = keep[5, 19] = False
    want = [len(np.unique(bad[:, :c][keep[:, :c]])) for c in cuts]
    got, got_map = topk_coverage(strided(bad, 3, device), cuts, n_items)
    assert int(propagate._status(device)[0].item()) & _native.ST_INDEX_OOB
    with pytest.raises(IndexError):
        lg.check_index_status(device)                               # reports and clears
    lg.check_index_status(device)
    assert got.tolist() == want
    assert bool(((got_map & ~clean_map) == 0).all())                # nothing marked that the clean rows do not mark


# ---------------------------------------------------------------------------------------------------------------
# 7. a user outside the lists
# ---------------------------------------------------------------------------------------------------------------
def test_out_of_range_user_zeroes_its_row_and_spares_the_others(device):
    c = case(17, 20, (5, 10, 20), LENGTHS)
    top, pos, users, hits, metrics, bits = run(device, c)
    lg.check_index_status(device)                                   # nothing pending
    bad = users.clone()
    bad[2], bad[7], bad[16] = c["n_users"], -1, 2 ** 40
    h, m, b = rank_metrics(top, pos, bad, c["cutoffs"], return_bits=True)
    assert int(propagate._status(device)[0].item()) & _native.ST_INDEX_OOB
    with pytest.raises(IndexError):
        lg.check_index_status(device)
    lg.check_index_status(device)                                   # cleared
    hit = torch.zeros(17, dtype=torch.bool, device=device)
    hit[[2, 7, 16]] = True
    assert not h[hit].any() and not b[hit].any() and bool((m[hit].view(torch.int64) == 0).all())
    assert torch.equal(h[~hit], hits[~hit]) and bits_equal(m[~hit], metrics[~hit]) and torch.equal(b[~hit], bits[~hit])
    ut, it = randn_tables(6, c["n_users"], N_ITEMS, 64, 64, device)
    with pytest.raises(IndexError):
        evaluate_ranking(ut, it, None, bad, pos, (5, 20))
    lg.check_index_status(device)                                   # cleared there as well


# ---------------------------------------------------------------------------------------------------------------
# 8. the model's method on a golden fixture
# ---------------------------------------------------------------------------------------------------------------
def test_evaluate_metrics_on_a_golden_fixture(device):
    import pandas as pd
    z = load_golden("train_s0_d90_k3")
    ei, ew, w0 = t(z["edge_index"]).to(device), t(z["edge_weight"]).to(device), t(z["weight0"])
    n_users, n_items, ks = int(z["n_users"]), int(z["n_items"]), (5, 10, 20)
    model = lg.LightGCN(w0.size(0), w0.size(1), len(z["alpha"]) - 1)
    model.load_state_dict({"alpha": t(z["alpha"]), "embedding.weight": w0})
    model.to(device).eval()
    src, dst = t(z["edge_index"])
    mask = torch.zeros(n_users, n_items)
    mask[src[src < n_users], dst[src < n_users] - n_users] = 1.0
    seen = SeenLists.from_dense(mask, list(range(n_users)), n_users, device=device).validate(n_users)
    rng = np.random.default_rng(3)
    listed = rng.permutation(n_users)[:60].tolist()
    lists = [rng.integers(n_items, size=int(rng.integers(1, 12))).tolist() for _ in listed]
    listed.append(listed[4])                                        # a user listed twice
    lists.append(lists[4])
    pos_df = pd.DataFrame({"user_id_idx": listed, "item_id_idx_list": lists})
    positives = PositiveLists.from_frame(pos_df, n_users, device=device).validate(n_users, n_items)
    with torch.no_grad():
        res = model.evaluate_metrics(ei, ew, n_users, n_items, seen, None, pos_df, ks=ks, workspace_bytes=4 * n_items * 16)
        same = model.evaluate_metrics(ei, ew, n_users, n_items, seen, listed, positives, ks)
        each = [model.evaluateK(ei, ew, n_users, n_items, seen, listed, positives, k) for k in ks]
    assert res.mean == same.mean and torch.equal(res.topk, same.topk) and bits_equal(res.metrics, same.metrics)
    assert res.mean["precision"] == tuple(e[0] for e in each) and res.mean["recall"] == tuple(e[1] for e in each)
    for ci in range(3):
        assert torch.equal(res.hits[:, ci], each[ci][2])
    assert res.hits[:, -1].sum().item() > 0
    top = res.topk.cpu().numpy()
    want_h, want_m, want_b = reference(top, positives.ptr.cpu().numpy(), positives.items.cpu().numpy(), listed, ks)
    assert np.array_equal(res.hits.cpu().numpy(), want_h) and np.array_equal(res.hit_bits.cpu().numpy().view(np.uint64), want_b)
    for col, name in enumerate(propagate.METRIC_NAMES):
        for ci in range(3):
            err = abs(res.mean[name][ci] - want_m[:, ci, col].mean())
            print(f"{name}@{ks[ci]}: {res.mean[name][ci]!r} (numpy {want_m[:, ci, col].mean()!r})")
            assert err <= TOL, (name, ks[ci], err)
    assert res.mean["coverage"] == tuple(len(np.unique(top[:, :c])) / n_items for c in ks)
    # the frame of MARK_MAPK, at the largest cutoff and at a smaller one
    for c in (20, 5):
        top_df = pd.DataFrame({"user_ID": listed[:-1], "top_rlvnt_itm": top[:-1, :c].tolist()})
        _, _, frame = model.MARK_MAPK(pos_df, top_df, c)
        mine = metrics_frame(pos_df, res, None if c == 20 else c)
        assert list(mine.columns) == list(frame.columns) and list(mine.dtypes) == list(frame.dtypes) and len(mine) == len(frame)
        for col in ("user_id_idx", "item_id_idx_list", "user_ID", "top_rlvnt_itm", "recall", "precision"):
            assert mine[col].tolist() == frame[col].tolist(), col
        assert [set(o) for o in mine["overlap_item"]] == [set(o) for o in frame["overlap_item"]]
        assert [len(o) for o in mine["overlap_item"]] == [len(o) for o in frame["overlap_item"]]
        ref = reference_frame(pos_df, listed, top, positives.ptr.cpu().numpy(), positives.items.cpu().numpy(), c)
        assert mine["overlap_item"].tolist() == ref["overlap_item"].tolist()             # ... in the ranking's order
    lg.check_index_status(device)
