"""The host reference of the middle-hop reduction builder (tests/reduce_support.py) checked on its own: against arrays
written out by hand, against its vectorised form, against the numpy restatement of the concat tests, and against the wrong
rules the device tests are meant to catch (tests/test_reduce_gpu.py).  No GPU."""
import numpy as np
import pytest

import reduced_concat_support as RC
from reduce_support import (CASES, INT32_MAX, Case, csr_from_edges, f32_bits, reduce_reference, reduce_reference_fast, same)


def ref(case, t, **kw):
    return reduce_reference(case.rowptr, case.cols, case.val_bits, case.split, case.n_nodes, t, **kw)


def ent(pairs):
    """[(column, fp32 value)] -> int32 [n, 2] with the value's bits."""
    out = np.zeros((len(pairs), 2), dtype=np.int32)
    if pairs:
        out[:, 0] = [c for c, _ in pairs]
        out[:, 1] = f32_bits([v for _, v in pairs])
    return out


# name, T -> user_map, (n_kept, entries of the kept user rows, entries of the reduced CSR, pairs: least, most),
#            rowptr_out, entries_out, gram rowptr, gram entries -- worked out by hand from the rows in reduce_support
BY_HAND = {
    ("order_shows", 3): ([-1, -1, -1, -1], (0, 0, 0, 6, 6), [0, 0, 0, 0, 0], [], [0, 1, 1, 2, 2], [(1, 1.0), (3, 1.0)]),
    ("order_shows", 1): ([-1, -1, -1, 0], (1, 3, 4, 3, 3), [0, 3, 3, 3, 4, 4],
                         [(4, 2.0 ** 60), (4, -2.0 ** 60), (4, 1.0), (0, 1.0)], [0, 0, 1, 1, 1, 1], [(2, 1.0)]),
    ("cancels_to_zero", 1): ([-1, -1, -1], (0, 0, 0, 3, 3), [0, 0, 0, 0], [], [0, 1, 1, 2], [(1, 0.0), (2, 0.0)]),
    ("duplicates", 2): ([-1, 0], (1, 1, 4, 4, 4), [0, 1, 1, 4], [(1, 7.0), (0, 1.0), (0, 2.0), (0, 4.0)], [0, 0, 1, 1],
                        [(2, 20.0)]),
    ("duplicates", 3): ([-1, -1], (0, 0, 0, 7, 7), [0, 0, 0], [], [0, 1, 2], [(1, 20.0), (0, 49.0)]),
    ("threshold", 2): ([-1, 0, -1, 1], (2, 4, 8, 6, 6), [0, 3, 4, 6, 7, 8],
                       [(2, 1.0), (3, 1.0), (4, 1.0), (4, 5.0), (0, 1.0), (1, 1.0), (1, 2.0), (1, 4.0)], [0, 0, 0, 3, 6, 6],
                       [(2, 1.0), (3, 2.0), (4, 3.0), (2, 2.0), (3, 4.0), (4, 6.0)]),
    ("wrong_side", 4): ([-1, 0], (1, 2, 4, 1, 4), [0, 2, 3, 4], [(1, 5.0), (2, 6.0), (0, 3.0), (0, 7.0)], [0, 0, 1, 1],
                        [(2, 8.0)]),
    ("smallest", 1): ([-1], (0, 0, 0, 1, 1), [0, 0], [], [0, 1], [(0, 6.0)]),
    ("smallest", 0): ([0], (1, 1, 2, 0, 0), [0, 1, 2], [(1, 3.0), (0, 2.0)], [0, 0, 0], []),
    ("no_entries", 0): ([-1, -1], (0, 0, 0, 0, 0), [0, 0, 0], [], [0, 0, 0], []),
    ("nothing_left", 2): ([-1, -1, -1], (0, 0, 0, 0, 0), [0, 0, 0], [], [0, 0, 0], []),
}


@pytest.mark.parametrize("name,t", sorted(BY_HAND))
def test_reference_against_arrays_written_by_hand(name, t):
    user_map, (n_kept, user_nnz, nnz, pairs_min, pairs_max), rowptr, entries, gram_rowptr, gram_entries = BY_HAND[(name, t)]
    for fn in (reduce_reference, reduce_reference_fast):
        case = CASES[name]()
        got = fn(case.rowptr, case.cols, case.val_bits, case.split, case.n_nodes, t)
        assert got.user_map.tolist() == user_map
        assert (got.n_kept, got.user_nnz, got.nnz, got.pairs_min, got.pairs_max) == (n_kept, user_nnz, nnz, pairs_min, pairs_max)
        assert got.rowptr.tolist() == rowptr and got.gram_rowptr.tolist() == gram_rowptr
        assert np.array_equal(got.entries, ent(entries))
        assert np.array_equal(got.gram_entries, ent(gram_entries)), (got.gram_entries, ent(gram_entries))
        assert got.rowptr.dtype == got.entries.dtype == got.gram_rowptr.dtype == got.gram_entries.dtype == np.int32


def test_zero_sums_are_stored_as_plus_zero():
    got = ref(CASES["cancels_to_zero"](), 1)
    assert got.gram_entries[:, 1].tolist() == [0, 0], "bits 0x00000000 for the cancelled run and for the lone -0.0"
    minus = ref(CASES["cancels_to_zero"](), 1, start=-0.0)
    assert minus.gram_entries[1, 1] == np.int32(-2 ** 31), "a sum that does not start at +0 keeps the -0.0: the case sees it"
    assert same(got, minus) == "gram_entries"


def test_order_shows_tells_the_orders_apart():
    case = CASES["order_shows"]()
    want = ref(case, 3)
    assert want.gram_entries[:, 1].view(np.float32).tolist() == [1.0, 1.0]
    by_column = ref(case, 3, order="columns")
    assert by_column.gram_entries[:, 1].view(np.float32).tolist() == [0.0, 1.0], "user columns ascending: the first run is lost"
    unstable = ref(case, 3, order="reversed")
    assert unstable.gram_entries[:, 1].view(np.float32).tolist() == [0.0, 0.0], "equal keys in another order: both are lost"
    assert same(want, by_column) == same(want, unstable) == "gram_entries"
    # the products need fp64, and the tree p0 + (p1 + p2) is another sum
    p = np.float64(2.0 ** 60), np.float64(-2.0 ** 60), np.float64(1.0)
    assert (p[0] + p[1]) + p[2] == 1.0 and p[0] + (p[1] + p[2]) == 0.0
    assert np.float32(2.0 ** 30) * np.float32(2.0 ** 30) == np.float32(2.0 ** 60), "the inputs are exact in fp32"


def test_incount_counts_entries_not_rows():
    case = CASES["duplicates"]()
    want, rows = ref(case, 2), ref(case, 2, distinct_rows=True)
    assert want.user_map.tolist() == [-1, 0] and rows.user_map.tolist() == [-1, -1]
    assert same(want, rows) is not None
    case = CASES["threshold"]()
    assert ref(case, 2).user_map.tolist() == [-1, 0, -1, 1]
    assert ref(case, 1).user_map.tolist() == [0, 1, 2, 3] and ref(case, 3).user_map.tolist() == [-1, -1, -1, -1]


def test_wrong_side_columns_are_as_if_absent():
    """The malformed entries only lengthen the stored rows: with T chosen so that the same users go, every output but the
    upper end of the pair count is that of the graph without them."""
    case = CASES["wrong_side"]()
    rows = np.repeat(np.arange(case.n_nodes), np.diff(case.rowptr))
    good = np.where(rows < case.split, (case.cols >= case.split) & (case.cols < case.n_nodes),
                    (case.cols >= 0) & (case.cols < case.split))
    assert int((~good).sum()) == 9
    clean = Case(np.concatenate([[0], np.cumsum(np.bincount(rows[good], minlength=case.n_nodes))]).astype(np.int32),
                 case.cols[good], case.val_bits[good], case.split, case.n_nodes)
    dirty, want = ref(case, 4), ref(clean, 1)
    assert want.user_map.tolist() == [-1, 0] and want.pairs_min == want.pairs_max == dirty.pairs_min == 1
    for f in ("user_map", "rowptr", "entries", "gram_rowptr", "gram_entries"):
        assert np.array_equal(getattr(dirty, f), getattr(want, f)), f
    unguarded = ref(case, 4, guards=False)
    assert unguarded.nnz == dirty.nnz + 3 and same(dirty, unguarded) is not None, "without the column guard the case differs"


@pytest.mark.parametrize("name", sorted(CASES))
def test_vectorised_form_gives_the_same_bits(name):
    case = CASES[name]()
    assert case.thresholds()[0] == 0 and case.thresholds()[-1] == INT32_MAX
    for t in case.thresholds():
        slow = ref(case, t)
        fast = reduce_reference_fast(case.rowptr, case.cols, case.val_bits, case.split, case.n_nodes, t)
        assert same(slow, fast) is None, (name, t, same(slow, fast))
        assert (slow.pairs_min == slow.pairs_max) or not case.well_formed
        n_items = case.n_nodes - case.split
        assert slow.rowptr.size == slow.gram_rowptr.size == slow.n_kept + n_items + 1
        assert slow.gram_rowptr[slow.n_kept] == 0 and slow.rowptr[slow.n_kept] == slow.user_nnz


def test_named_cases_are_what_their_names_say():
    c = CASES["all_user_side"]()
    assert c.rowptr[c.split] == c.cols.size > 0
    c = CASES["all_item_side"]()
    assert c.rowptr[c.split] == 0 and c.cols.size > 0
    assert ref(c, 3).user_map.tolist() == [-1, 0, -1], "user 1 is named four times"
    assert CASES["no_entries"]().cols.size == 0
    c = CASES["smallest"]()
    assert (c.split, c.n_nodes, c.cols.size) == (1, 2, 2)
    got = ref(CASES["nothing_left"](), 2)
    assert got.n_kept == 0 and got.nnz == 0 and got.gram_entries.shape[0] == 0 and got.pairs_max == 0
    got = ref(CASES["kept_but_unnamed"](), 2)
    assert got.n_kept == 2 and got.nnz == got.user_nnz == 7 and got.gram_entries.shape[0] > 0
    c = CASES["empty_rows"]()
    lengths = np.diff(c.rowptr)
    assert lengths[0] == 0 and lengths[c.split - 1] == 0 and lengths[c.split] == 0 and lengths[-1] == 0
    got = ref(CASES["dense_block"](), 4)
    assert got.n_kept == 1 and got.gram_entries.shape[0] == 36
    assert got.gram_rowptr.tolist() == [0, 0] + [6 * (i + 1) for i in range(6)]
    assert got.gram_entries[:, 0].tolist() == [1 + j for _ in range(6) for j in range(6)]


@pytest.mark.parametrize("name", sorted(RC.GRAPHS))
def test_agrees_with_the_restatement_of_the_concat_tests(name):
    ei, ew, split, n, t = RC.GRAPHS[name]()
    rowptr, cols, bits = csr_from_edges(ei, ew, n)
    rp, en, grp, gen, n_h = RC.reduced_csr_numpy(ei, ew, split, n, t)
    for fn in (reduce_reference, reduce_reference_fast):
        got = fn(rowptr, cols, bits, split, n, t)
        assert got.n_kept == n_h and got.pairs_min == got.pairs_max
        assert np.array_equal(got.rowptr, rp) and np.array_equal(got.entries, en)
        assert np.array_equal(got.gram_rowptr, grp) and np.array_equal(got.gram_entries, gen)
