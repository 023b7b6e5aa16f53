"""The reference, the route rule and the case table of tests/topk_support.py, checked without a device: the reference
against a brute-force selection, against torch.topk's values and against rows written by hand; every case against the
route and the candidate count it is in the table for; and the table as a whole against the list of paths of k_mask_topk it
has to reach (csrc/lgconv_serve.hip)."""
import numpy as np
import pytest
import torch

import topk_support as ts

INF = float("inf")


def brute_force(x, k):
    """O(n k): k times the best remaining element -- a NaN beats everything, then the larger value, then the lower index."""
    left, out = list(range(len(x))), []
    for _ in range(k):
        best = left[0]
        for i in left[1:]:
            a, b = x[i], x[best]
            if (np.isnan(a) and not np.isnan(b)) or (not np.isnan(a) and not np.isnan(b) and a > b):
                best = i                                   # ascending i: an equal element never replaces an earlier one
        out.append(best)
        left.remove(best)
    return out


# ----------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_topk_ref_is_the_brute_force_selection(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 90))
    rows = [ts.f32(rng.standard_normal(n)),
            ts.f32(rng.integers(-2, 3, size=n)),                                  # ties everywhere
            ts.f32(rng.choice([0.0, -0.0, 1.0, -1.0, INF, -INF, np.nan], size=n))]
    rows[1][::5] = -0.0
    for x in rows:
        for k in sorted({1, min(n, 7), n}):
            idx, val = ts.topk_ref(x, k)
            assert idx.tolist() == brute_force(x, k), (seed, k)
            assert ts.values_match(val, x[idx]) and idx.dtype == np.int64 and val.dtype == np.float32
    two, vals = ts.topk_ref(np.stack(rows), min(n, 7))
    assert [r.tolist() for r in two] == [brute_force(x, min(n, 7)) for x in rows] and vals.shape == two.shape


@pytest.mark.parametrize("cols,k", [(1, 1), (300, 256), (5000, 20), (70001, 33)])
def test_topk_ref_values_are_torch_topk_values_without_ties(cols, k):
    rng = np.random.default_rng(cols)
    x = ts.f32(rng.permutation(3 * cols).reshape(3, cols) * 0.25 - cols / 3)      # distinct, exact in fp32
    idx, val = ts.topk_ref(x, k)
    want = torch.from_numpy(x).topk(k, dim=-1)
    assert np.array_equal(val, want.values.numpy())
    assert np.array_equal(idx, want.indices.numpy())                               # no ties: the indices are determined too


def test_topk_ref_order_by_hand():
    nan_pos, nan_neg = ts.from_bits([0x7FC00000, 0xFFC00001])
    x = ts.f32([1.0, -INF, nan_neg, 0.0, INF, -0.0, nan_pos, 1.0, -1.0, INF, 0.0])
    idx, val = ts.topk_ref(x, x.size)
    #            NaNs by index | +inf | finite descending, -0 = +0 by index | -inf
    assert idx.tolist() == [2, 6, 4, 9, 0, 7, 3, 5, 10, 8, 1]
    assert ts.bits_of(val).tolist() == ts.bits_of(x[idx]).tolist()                # the values keep their own bits
    assert ts.topk_ref(x, 3)[0].tolist() == [2, 6, 4]
    assert ts.topk_ref(ts.f32([-0.0, 0.0, -0.0]), 2)[0].tolist() == [0, 1]
    assert ts.topk_ref(ts.f32([-INF, -INF, -3e38]), 2)[0].tolist() == [2, 0]


def test_values_match_is_bitwise_except_among_nans():
    nan_pos, nan_neg = ts.from_bits([0x7FC00000, 0xFF800001])
    assert ts.values_match([nan_pos, 1.0], [nan_neg, 1.0])
    assert not ts.values_match([0.0], [-0.0]) and not ts.values_match([nan_pos], [INF])
    assert not ts.values_match([1.0], [np.nextafter(np.float32(1.0), np.float32(2.0))])
    assert not ts.values_match([1.0, 2.0], [1.0])


def test_masked_ref_is_one_subtract_and_one_multiply_in_fp32():
    s, m = np.float32(1.04), np.float32(0.11)
    assert ts.masked_ref([s], [m])[0] == np.float32(s * np.float32(np.float32(1.0) - m))
    assert ts.masked_ref([s], [m])[0] != np.float32(np.float64(s) * (1.0 - np.float64(m)))     # not one rounding of the exact result
    got = ts.masked_ref(ts.f32([2.0, -2.0, INF, -INF, 3.0, 3.0]), ts.f32([1.0, 1.0, 1.0, 1.0, 2.0, -1.0]))
    assert ts.bits_of(got[:2]).tolist() == [0, 0x80000000] and np.isnan(got[2:4]).all() and got[4:].tolist() == [-3.0, 6.0]
    same = ts.masked_ref(ts.f32([1.5, -0.0]), None)
    assert ts.bits_of(same).tolist() == ts.bits_of(ts.f32([1.5, -0.0])).tolist()


def test_lists_dense_ignores_entries_outside_the_row_and_repeats():
    lists = ts.Lists([0, 2, 7], [1, 1, 4, -1, 0, 2 ** 40 + 3, 4], [1, 0, 1])
    assert lists.dense(3, 4).tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]]
    rng = np.random.default_rng(0)
    mask = (rng.random((3, 50)) < 0.2).astype(np.float32)
    for with_rows in (False, True):
        for junk in (False, True):
            got = ts.lists_of(mask, rng, with_rows, junk)
            assert np.array_equal(got.dense(3, 50), mask) and (got.rows is None) == (not with_rows)
            if junk:
                row0 = got.items[got.ptr[1 if with_rows else 0]:got.ptr[2 if with_rows else 1]]
                assert (row0 < 0).any() and (row0 >= 50).any() and len(set(row0.tolist())) < len(row0)


# ----------------------------------------------------------------------------------------
# the route rule
# ----------------------------------------------------------------------------------------
def test_topk_route_by_hand():
    row = np.zeros(2048, dtype=np.float32)
    row[:600] = 1.0 + np.arange(600) * 2.0 ** -12                  # threads 0..599 hold a value of the bin [1, 1.25)
    assert ts.topk_route(row, 5) == ("regs_radix", 600)           # the bin of the 5th largest thread maximum: 600 > 512
    row[512:600] = 0.0
    assert ts.topk_route(row, 5) == ("short", 512)
    assert ts.topk_route(row, 513) == ("regs_radix", 2048)        # the 513th thread maximum is a zero: everything is a candidate
    row[0] = np.nan
    assert ts.topk_route(row, 1) == ("short", 1)                   # a NaN has a bin of its own, above +inf's
    row[0] = ts.from_bits([0xFFC00000])[0]
    assert ts.topk_route(row, 1) == ("short", 1)                   # whatever its sign bit
    assert ts.topk_route(np.zeros(ts.REGS_COLS, dtype=np.float32), 1) == ("regs_radix", ts.REGS_COLS)
    assert ts.topk_route(np.zeros(ts.REGS_COLS + 1, dtype=np.float32), 1) == ("stream", None)
    # thread = column mod 1024: columns 3 and 1027 share a thread, whose maximum counts once
    row = np.zeros(2048, dtype=np.float32)
    row[3], row[1027], row[9] = 8.0, 9.0, 2.0
    assert ts.topk_route(row, 2) == ("short", 3)                   # second maximum is 2.0 (thread 9): candidates 8, 9, 2
    assert ts.tie_cut(ts.f32([5, 1, 5, 5, 0]), 2) == (3, 2, 1)
    assert ts.tie_cut(ts.f32([5, 1, 4, 3, 0]), 2) == (1, 1, 1)     # no tie at the cut: as many equal as needed


def test_order_keys_ascend_with_the_order():
    nan_pos, nan_neg = ts.from_bits([0x7F800001, 0xFFFFFFFF])
    x = ts.f32([-INF, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, INF, nan_neg, nan_pos])
    keys = ts.order_keys(x).astype(np.int64)
    assert (np.diff(keys) >= 0).all() and keys[4] == keys[5] and keys[-1] == keys[-2] == 0xFFFFFFFF
    assert (np.diff(keys)[[0, 1, 2, 3, 5, 6, 7, 8, 9]] > 0).all() and keys.min() >= 1


# ----------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------
def test_case_table_lists_what_the_issue_names():
    names = set(ts.CASE_NAMES)
    assert len(names) == len(ts.CASE_NAMES)
    for want in ["boundary_511", "boundary_512", "boundary_513", "cluster_low_bits", "cluster_with_ties", "ties_carried",
                 "ties_carried_stream", "one_thread_owns_the_top", "many_rows", "nan_short", "nan_regs_radix", "nan_stream",
                 "nan_from_mask", "dense_values_and_strides", "past_list_limit"]:
        assert want in names
    assert {f"width_{c}" for c in (1, 2, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537)} <= names
    assert {f"list_mask_{c}" for c in (131072, 131073, 983040)} <= names
    assert ts.case("k_edges_2048").ks == (1, 2, 3, 127, 128, 129, 255, 256)
    assert ts.case("past_list_limit").scores.shape[1] == ts.LIST_COLS_MAX + 1 == 983041
    assert ts.case("many_rows").scores.shape == (70000, 8) and ts.case("many_rows").ks == (3,)
    assert ts.case("boundary_512") is ts.case("boundary_512")                     # built once


@pytest.mark.parametrize("name", ts.CASE_NAMES)
def test_case_is_well_formed_and_takes_the_route_it_claims(name):
    c = ts.case(name)
    rows, cols = c.scores.shape
    assert c.scores.dtype == np.float32 and c.scores.strides[1] == 4 and c.claims
    assert all(1 <= k <= min(cols, ts.K_MAX) for k in c.ks)
    for form, dense, lists in c.forms:
        assert dense is None or lists is None
        if dense is not None:
            assert dense.shape == c.scores.shape and dense.dtype == np.float32 and dense.strides[1] == 4
        if lists is not None:
            assert cols <= ts.LIST_COLS_MAX and lists.ptr[0] == 0 and lists.ptr[-1] <= lists.items.size
            assert (np.diff(lists.ptr) >= 0).all()
            assert lists.ptr.size - 1 >= (rows if lists.rows is None else int(lists.rows.max()) + 1)
    for form, row, k, route, count in c.claims:
        assert k in c.ks
        got_route, got_count = ts.topk_route(c.masked(form)[row], k)
        assert got_route == route, (form, row, k, got_route, got_count)
        if count is not None:
            assert got_count == count, (form, row, k, got_count)
    for (form, row, k), slices in c.tie_slices.items():
        # a tie case keeps more elements equal to the k-th value than fit, in at least as many slices as it says
        equal, need, got = ts.tie_cut(c.masked(form)[row], k)
        assert equal > need >= 1 and got >= slices, (form, row, k, equal, need, got)


def test_boundary_cases_sit_on_both_sides_of_the_short_cut_limit():
    for n, route in ((511, "short"), (512, "short"), (513, "regs_radix")):
        c = ts.case(f"boundary_{n}")
        assert c.scores.shape[1] == 4096 and c.ks == (1, 20, 256)
        for row in range(c.scores.shape[0]):
            x = c.scores[row]
            top = x[x >= 1.0]
            assert top.size == n == np.unique(top).size and (top < 1.25).all() and (x[x < 1.0] < 0.9).all()
            assert np.flatnonzero(x >= 1.0).tolist() == list(range(min(n, 512))) + ([1024] if n == 513 else [])
            assert all(ts.topk_route(x, k) == (route, n) for k in c.ks)


def test_the_table_reaches_every_route_with_and_without_a_cut_tie():
    """All three routes, each on a row with no tie at the cut and on a row whose cut tie spans at least two 1,024-column
    slices (on the radix routes the count of ties taken so far is carried from slice to slice)."""
    clean, tied = set(), set()
    for name in ts.CASE_NAMES:
        c = ts.case(name)
        for form, row, k, route, _ in c.claims:
            x = c.masked(form)[row]
            assert ts.topk_route(x, k)[0] == route
            equal, need, slices = ts.tie_cut(x, k)
            if equal == need:
                clean.add(route)
            elif slices >= 2 and c.tie_slices.get((form, row, k), 0) >= 2:
                tied.add(route)
    assert clean == {"short", "regs_radix", "stream"}
    assert tied == {"short", "regs_radix", "stream"}


def test_the_table_holds_the_paths_no_random_row_reaches():
    # register radix decided by the low bits: 3,000 distinct keys that agree in their top 11 bits, k-th and (k+1)-th differ
    c = ts.case("cluster_low_bits")
    keys = ts.order_keys(c.scores[0])
    assert np.unique(keys).size == 3000 and np.unique(keys >> 21).size == 1 and np.unique(keys >> 10).size > 1
    assert np.unique(keys & 0x3FF).size > 1
    # ties of four across the cut
    c = ts.case("cluster_with_ties")
    assert [ts.tie_cut(c.scores[0], k)[:2] for k in c.ks] == [(4, 1), (4, 2), (4, 3)]
    # larger values found after the ties (n_gt > 0 with the tie slots already being filled)
    c = ts.case("ties_carried")
    assert c.scores.shape[1] == 4200 and ts.tie_cut(c.scores[0], 256)[0] == 263
    above = np.flatnonzero(c.scores[1] > 2.0)
    assert above.size == 10 and above.min() > np.flatnonzero(c.scores[1] == 2.0)[245]
    c = ts.case("ties_carried_stream")
    assert c.scores.shape[1] == 66000 and ts.tie_cut(c.scores[0], 64) == (129, 64, 32)
    # one thread owns the top: the k-th per-thread maximum is far below the k-th element
    c = ts.case("one_thread_owns_the_top")
    for row in range(2):
        idx, val = ts.topk_ref(c.scores[row], 8)
        assert sorted(idx.tolist()) == list(range(7, 8192, 1024)) and idx.tolist() != sorted(idx.tolist())
        thread_max = np.sort(c.scores[row].reshape(-1, 1024).max(axis=0))[::-1]
        assert thread_max[4] < 1.0 < val[-1]
    # NaNs of both sign bits on every route, none of them made by arithmetic; infinities beside them
    for name in ("nan_short", "nan_regs_radix", "nan_stream", "nan_many"):
        x = ts.case(name).scores[0]
        signs = ts.bits_of(x[np.isnan(x)]) >> 31
        assert set(signs.tolist()) == {0, 1}
        assert name == "nan_many" or ((x == INF).sum() == 2 and (x == -INF).sum() == 2 and np.isnan(x).sum() == 8)
    c = ts.case("nan_from_mask")
    masked = c.masked("dense")
    assert np.isnan(masked[0, [100, 2000]]).all() and np.isnan(masked[1, [0, 2999]]).all()
    assert masked[0, 50] == INF and masked[0, 60] == -INF and np.isnan(masked).sum() == 4
    assert ts.topk_ref(masked, 3)[0].tolist() == [[100, 2000, 50], [0, 2999, int(np.argmax(np.nan_to_num(masked[1], nan=-INF)))]]
    # the dense mask with other values than 0 and 1, scores and mask at different row strides, both wider than the row
    c = ts.case("dense_values_and_strides")
    mask = c.forms[1][1]
    assert {0.0, 0.5, 1.0, 2.0, -1.0} == set(np.unique(mask).tolist())
    assert c.scores.strides[0] // 4 == 3011 and mask.strides[0] // 4 == 3037 and c.scores.shape[1] == 3000
    # the list form: a repeated entry and entries outside the row, with and without the row -> user index
    for cols in (131072, 131073, 983040):
        c = ts.case(f"list_mask_{cols}")
        assert c.scores.shape == (2, cols) and [f[0] for f in c.forms] == ["none", "dense", "lists_rows", "lists_null"]
        assert c.forms[2][2].rows is not None and c.forms[3][2].rows is None
        for form in ("lists_rows", "lists_null"):
            assert np.array_equal(c.masked(form), c.masked("dense"))
        seen = c.forms[1][1]
        assert 0.005 < seen.mean() < 0.02
        assert not np.array_equal(ts.topk_ref(c.masked("dense"), 20)[0], ts.topk_ref(c.scores, 20)[0])     # the mask matters
