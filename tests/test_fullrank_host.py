"""CPU-only checks of full-rank evaluation: the two entry points in the header (an addition to ABI 14), the ctypes table and
the library; the argument validation, which happens before any launch; the workspace size; the numpy reference on
hand-worked lists with integer scores; the metric formulas on hand-worked ranks; the case table's reach; and
tools/train_demo.py's arguments."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, fullrank, propagate
import fullrank_support as fs
import topk_support as ts

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_DIM, E_WORKSPACE, E_RANGE, E_ALIGN = -1, -2, -3, -4, -5
NAMES = ("lgc_rank_positions_workspace_bytes", "lgc_rank_positions")
NEG0 = ts.from_bits([0x80000000])[0]


def test_entry_points_are_declared_bound_and_exported_as_an_addition_to_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    assert "Full-rank evaluation (an addition to ABI 14: exports only)" in header
    for name, value in (("ZERO", 0), ("REMOVE", 1)):
        assert int(re.search(r"#define LGC_RANK_SEEN_" + name + r"\s+(\d+)", header).group(1)) == value
        assert _native.RANK_SEEN_MODES[name.lower()] == value and fs.MODES[value] == name.lower()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        decl = re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert decl, name
        restype, argtypes = _native.SIGNATURES[name]
        assert hasattr(lib, name)
        assert restype is (ctypes.c_size_t if decl.group(1) == "size_t" else ctypes.c_int)
        want = []
        for arg in decl.group(2).split(","):
            arg = arg.strip()
            kind = "ptr" if "*" in arg else re.match(r"(?:const\s+)?(\w+)", arg).group(1)
            want.append({"ptr": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
                         "size_t": ctypes.c_size_t}[kind])
        assert want == list(argtypes), name
    for name in ("positive_ranks", "evaluate_full_rank"):
        assert name in lg.__all__ and hasattr(lg, name)
    assert hasattr(lg.LightGCN, "evaluate_full_rank")
    makefile = open(os.path.join(ROOT, "gnn-ecommerce_amd", "csrc", "Makefile")).read()
    assert "lgconv_fullrank" in re.search(r"^UNITS\s*:=((?:.*\\\n)*.*)$", makefile, flags=re.M).group(1).replace("\\", " ").split()


# addresses of host words: valid, 16-byte aligned, never read or written by a call that returns before its launch
_words = (ctypes.c_int64 * 8)()
ONE = ctypes.addressof(_words) + (-ctypes.addressof(_words)) % 16
ORDER = ("users", "user_stride", "n_user_rows", "items", "item_stride", "n_items", "dim", "pair_users", "pair_items", "n_pairs",
         "seen_ptr", "seen_items", "seen_mode", "slices", "rank", "n_equal", "n_cand", "value", "workspace", "workspace_bytes",
         "status")


def positions(**kw):
    a = dict(users=ONE, user_stride=64, n_user_rows=50, items=ONE, item_stride=64, n_items=300, dim=64, pair_users=ONE,
             pair_items=ONE, n_pairs=4, seen_ptr=ONE, seen_items=ONE, seen_mode=0, slices=0, rank=ONE, n_equal=ONE, n_cand=ONE,
             value=ONE, workspace=ONE, workspace_bytes=1 << 40, status=ONE)
    assert set(kw) <= set(a)
    a.update(kw)
    return _native.load().lgc_rank_positions(*[a[name] for name in ORDER], None)


def ws_bytes(n_pairs=100, n_items=1000, slices=0):
    return _native.load().lgc_rank_positions_workspace_bytes(n_pairs, n_items, slices)


def test_argument_errors_come_before_any_launch():
    for bad in (dict(users=None), dict(items=None), dict(pair_users=None), dict(pair_items=None), dict(rank=None),
                dict(status=None), dict(n_pairs=-1), dict(n_user_rows=-1), dict(user_stride=63), dict(item_stride=63),
                dict(seen_mode=2), dict(seen_mode=-1), dict(seen_items=None)):
        assert positions(**bad) == E_INVAL, bad
    for dim in (0, -1, 257):
        assert positions(dim=dim, user_stride=300, item_stride=300) == E_DIM
    for bad in (dict(slices=-1), dict(slices=65), dict(n_items=0), dict(n_items=-1), dict(n_items=2 ** 31 - 1),
                dict(n_items=2 ** 31), dict(n_pairs=2 ** 31 - 1), dict(n_pairs=2 ** 31), dict(n_user_rows=2 ** 31 - 1)):
        assert positions(**bad) == E_RANGE, bad
    for name in ("users", "items", "rank", "n_equal", "n_cand", "value", "workspace", "status"):
        assert positions(**{name: ONE + 2}) == E_ALIGN, name
    for name in ("pair_users", "pair_items", "seen_ptr", "seen_items"):
        assert positions(**{name: ONE + 4}) == E_ALIGN, name
    # the workspace: what the size function says is enough, one byte less is not
    for slices in (0, 1, 2, 64):
        need = ws_bytes(4, 300, slices)
        assert need == 16
        assert positions(slices=slices, n_pairs=0, workspace_bytes=need) == 0
        assert positions(slices=slices, workspace_bytes=need - 1) == E_WORKSPACE
        assert positions(slices=slices, workspace=None) == E_WORKSPACE
    # n_pairs == 0: validated, nothing launched; the optional pointers may be NULL
    assert positions(n_pairs=0) == 0
    assert positions(n_pairs=0, seen_ptr=None, seen_items=None, n_equal=None, n_cand=None, value=None, workspace=None,
                     workspace_bytes=0, seen_mode=1) == 0
    assert positions(n_pairs=0, seen_ptr=None) == 0                                     # seen_items alone is ignored,
    assert positions(n_pairs=0, seen_ptr=None, seen_items=ONE + 4) == 0                 # and so is its alignment
    assert positions(n_pairs=0, slices=64) == 0 and positions(n_pairs=0, n_items=1, n_user_rows=0) == 0
    assert positions(n_pairs=0, dim=1, user_stride=1, item_stride=1) == 0
    assert positions(n_pairs=0, dim=256, user_stride=259, item_stride=256) == 0
    assert positions(n_pairs=0, item_stride=63) == E_INVAL and positions(n_pairs=0, slices=65) == E_RANGE   # still validated
    assert positions(n_pairs=0, seen_mode=3) == E_INVAL


def test_workspace_size_refuses_what_the_call_refuses_and_grows_with_every_argument():
    for bad in (dict(n_pairs=-1), dict(n_items=0), dict(slices=-1), dict(slices=65), dict(n_pairs=2 ** 31 - 1),
                dict(n_pairs=2 ** 31), dict(n_items=2 ** 31 - 1), dict(n_items=2 ** 31)):
        assert ws_bytes(**bad) == 0, bad
    grid_p = (0, 1, 63, 64, 65, 1000, 15000, 10 ** 6, 2 ** 31 - 2)
    grid_i = (1, 128, 129, 1000, 54571, 10 ** 6, 2 ** 31 - 2)
    for slices in (0, 1, 2, 3, 7, 64):
        for n_items in grid_i:
            sizes = [ws_bytes(p, n_items, slices) for p in grid_p]
            assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] > 0, ("n_pairs", slices, n_items)
        for p in grid_p:
            sizes = [ws_bytes(p, n_items, slices) for n_items in grid_i]
            assert sizes == sorted(sizes), ("n_items", slices, p)
    for p in grid_p:
        for n_items in grid_i:
            sizes = [ws_bytes(p, n_items, s) for s in range(1, 65)]
            assert sizes == sorted(sizes), ("slices", p, n_items)
            assert ws_bytes(p, n_items, 0) <= ws_bytes(p, n_items, 64)
    assert ws_bytes(15000, 54571, 0) <= 64 << 10                                        # tens of kilobytes, not a score panel


def test_python_layer_validates_before_it_touches_a_device():
    users, items = torch.zeros(4, 8), torch.zeros(5, 8)
    pu, pi = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="seen_mode"):
        fullrank.positive_ranks(users, items, pu, pi, seen_mode="drop")
    for slices in (-1, 65, 1.0, True):
        with pytest.raises(ValueError, match="slices"):
            fullrank.positive_ranks(users, items, pu, pi, slices=slices)
    with pytest.raises(_native.NativeLibraryError):                                     # no CPU route
        fullrank.positive_ranks(users, items, pu, pi)
    pos = propagate.PositiveLists.from_lists([0], [[1]], 4)
    with pytest.raises(ValueError, match="cutoffs"):
        fullrank.evaluate_full_rank(users, items, None, pu, pos, ks=())
    with pytest.raises(_native.NativeLibraryError):
        fullrank.evaluate_full_rank(users, items, None, pu, pos)
    # an unsorted list is refused once, and the verdict is kept on the object
    for ptr, items_of, ok in (([0, 3], [3, 1, 2], False), ([0, 3, 5], [1, 1, 3, 0, 2], True), ([0, 0], [], True), ([0, 1], [2], True),
                              ([0, 2, 4], [0, 5, 6, 5], False)):
        lists = propagate.SeenLists(torch.tensor(ptr), torch.tensor(items_of, dtype=torch.int64))
        if ok:
            fullrank._check_ascending(lists)
        else:
            with pytest.raises(ValueError, match="ascending"):
                fullrank._check_ascending(lists)
        assert lists._ascending is ok
        lists.items = None                                                              # the verdict is not computed again
        if ok:
            fullrank._check_ascending(lists)


# ---------------------------------------------------------------------------------------------------------------
# the reference, on lists worked by hand
# ---------------------------------------------------------------------------------------------------------------
def test_reference_counts_ties_before_and_after_p():
    #                   0  1  2  3  4  5  6
    scores = np.array([[5, 7, 7, 1, 7, 9, 7]] * 4, dtype=np.float32)
    rank, n_equal, n_cand, value = fs.ranks_ref(scores, [2, 1, 6, 3])
    assert rank.tolist() == [2, 1, 4, 6]                      # 9 and the 7 at index 1; 9; 9 and three 7s; everything
    assert n_equal.tolist() == [3, 3, 3, 0] and n_cand.tolist() == [7] * 4 and value.tolist() == [7, 7, 7, 1]
    # a permutation: every item of one row
    rank, _, _, _ = fs.ranks_ref(np.repeat(scores[:1], 7, axis=0), np.arange(7))
    assert sorted(rank.tolist()) == list(range(7)) and rank.tolist() == [5, 1, 2, 6, 3, 0, 4]


def test_reference_orders_nan_inf_and_both_zeros_as_mask_topk_does():
    nan_neg, nan_pos = ts.from_bits([0xFFC00000, 0x7FC00000])
    #                  0       1        2    3        4        5     6    7
    row = np.array([np.inf, nan_neg, 3.0, nan_pos, -np.inf, NEG0, 0.0, -2.0], dtype=np.float32)
    rank, n_equal, _, value = fs.ranks_ref(np.repeat(row[None], 8, axis=0), np.arange(8))
    assert rank.tolist() == [2, 0, 3, 1, 7, 4, 5, 6]          # NaNs by index, +inf, 3, -0 = +0 by index, -2, -inf
    assert n_equal.tolist() == [0, 1, 0, 1, 0, 1, 1, 0]       # the NaN threshold ties with the other NaN; -0 with +0
    assert np.isnan(value[[1, 3]]).all() and ts.bits_of(value)[5] == 0x80000000


def test_reference_masks_seen_items_in_both_modes():
    #                  0    1     2       3    4     5
    row = np.array([4.0, -3.0, np.inf, 2.0, 0.0, -np.inf], dtype=np.float32)
    panel = np.repeat(row[None], 6, axis=0)
    seen = [1, 2, 2, 7, -1, 3]                                # a repeat and two entries out of range
    lists = [seen] * 6
    # mode zero: m = [4, -0, NaN, +0, 0, -inf]; the seen inf is a NaN and leads, the zeros tie by index
    rank, n_equal, n_cand, value = fs.ranks_ref(panel, np.arange(6), lists, "zero")
    assert rank.tolist() == [1, 2, 0, 3, 4, 5] and n_equal.tolist() == [0, 2, 0, 2, 2, 0] and n_cand.tolist() == [6] * 6
    assert ts.bits_of(value)[1] == 0x80000000 and np.isnan(value[2]) and ts.bits_of(value)[3] == 0
    # mode remove: candidates 0, 4, 5; a seen p has no rank, its raw score is still reported
    rank, n_equal, n_cand, value = fs.ranks_ref(panel, np.arange(6), lists, "remove")
    assert rank.tolist() == [0, -1, -1, -1, 1, 2] and n_equal.tolist() == [0, -1, -1, -1, 0, 0] and n_cand.tolist() == [3] * 6
    assert value.tolist() == row.tolist()
    # no lists: the modes coincide; a pair marked invalid is voided
    a = fs.ranks_ref(panel, np.arange(6), None, "zero", valid=[True, False] * 3)
    b = fs.ranks_ref(panel, np.arange(6), None, "remove", valid=[True, False] * 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].tolist() == [1, -1, 0, -1, 3, -1] and a[2].tolist() == [6, 0] * 3 and a[3][1] == 0


def test_reference_agrees_with_a_sort_by_device_keys():
    rng = np.random.default_rng(5)
    row = rng.integers(-3, 4, size=200).astype(np.float32)
    row[[3, 50]] = ts.from_bits([0x7FC00000, 0xFFC00000])
    row[[7, 9]] = [np.inf, -np.inf]
    row[11] = NEG0
    order, _ = ts.topk_ref(row, 200)
    rank, _, _, _ = fs.ranks_ref(np.repeat(row[None], 200, axis=0), np.arange(200))
    assert np.array_equal(order[rank], np.arange(200))        # the item at column rank[p] of the sorted row is p


# ---------------------------------------------------------------------------------------------------------------
# the metric formulas, on ranks worked by hand
# ---------------------------------------------------------------------------------------------------------------
def test_metrics_on_hand_worked_ranks():
    # user 0: positives at ranks 0, 3 of 10 candidates (list length 3: a duplicate); user 1: P = 1 at rank 4 of 5;
    # user 2: P = n_c = 2 (every candidate is a positive); user 3: all pairs invalid; user 4: no pairs at all
    rank = np.array([0, 3, 4, 0, 1, -1, -1])
    n_cand = np.array([10, 10, 5, 2, 2, 9, 0])
    owner = np.array([0, 0, 1, 2, 2, 3, 3])
    lengths = [3, 1, 2, 2, 1]
    ks = (1, 4, 300)
    auc, mpr, rr, recall, hit = fs.metrics_ref(rank, n_cand, owner, lengths, ks)
    assert auc[0] == 1.0 - 2.0 / 16.0 and mpr[0] == 3.0 / 18.0 and rr[0] == 1.0       # 3 - 1 wrong pairs of 2 * 8
    assert auc[1] == 0.0 and mpr[1] == 1.0 and rr[1] == 0.2
    assert np.isnan(auc[2]) and mpr[2] == 0.5 and rr[2] == 1.0
    assert np.isnan(auc[3:]).all() and np.isnan(mpr[3:]).all() and rr[3:].tolist() == [0.0, 0.0]
    assert recall.tolist() == [[1 / 3, 2 / 3, 2 / 3], [0, 0, 1], [0.5, 1, 1], [0, 0, 0], [0, 0, 0]]
    assert hit.tolist() == [[1, 1, 1], [0, 0, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0]]
    # the library's integer reductions give the same bits
    got = fullrank.pair_metrics(torch.from_numpy(rank).to(torch.int32), torch.from_numpy(n_cand).to(torch.int32),
                                torch.from_numpy(owner), torch.tensor(lengths), ks)
    for name, ref in (("auc", auc), ("mpr", mpr), ("rr", rr), ("recall", recall), ("hit", hit)):
        assert np.array_equal(got[name].numpy().view(np.uint64), ref.view(np.uint64)), name
    assert got["n_pos"].tolist() == [2, 1, 2, 0, 0] and got["n_cand"].tolist() == [10, 5, 2, 0, 0]


def test_pairs_are_the_distinct_items_of_every_listed_user():
    pos = propagate.PositiveLists.from_lists([4, 1, 2], [[7, 3, 7], [5], [2, 2]], 6)
    users = torch.tensor([2, 4, 1, 4, 0])                     # a user twice, a user without a list
    owner, pair_users, pair_items, length = fullrank._pairs_of(pos, users)
    assert owner.tolist() == [0, 1, 1, 2, 3, 3] and pair_users.tolist() == [2, 4, 4, 1, 4, 4]
    assert pair_items.tolist() == [2, 3, 7, 5, 3, 7] and length.tolist() == [2, 3, 1, 3, 0]
    assert pos.distinct.tolist() == [0, 1, 1, 0, 2, 0]
    assert fullrank._pairs_of(pos, users)[0] is owner          # kept
    empty = fullrank._pairs_of(pos, torch.zeros(0, dtype=torch.int64))
    assert [t.numel() for t in empty] == [0, 0, 0, 0]


def test_kept_pairs_never_answer_for_another_user_set():
    """The kept pairs belong to one id tensor: another tensor of the same length -- at the same address after the first
    was freed, too -- a write in place, or another length each build their own; a view of the same memory reuses them."""
    pos = propagate.PositiveLists.from_lists([4, 1, 2], [[7, 3, 7], [5], [2, 2]], 6)
    n = 5_000_000                                             # large enough that the allocator hands the block out again
    first = torch.full((n,), 0, dtype=torch.int64)
    assert fullrank._pairs_of(pos, first)[2].numel() == 0     # user 0 has no list
    address = first.data_ptr()
    del first
    second = torch.full((n,), 2, dtype=torch.int64)           # whether or not it lands on `address`, the answer is its own
    owner, pair_users, pair_items, length = fullrank._pairs_of(pos, second)
    assert owner.numel() == n and bool((pair_users == 2).all()) and bool((pair_items == 2).all()) and bool((length == 2).all())
    assert second.data_ptr() != address                       # the entry kept `first` alive, so nothing could alias it
    del second, owner, pair_users, pair_items, length
    a, b = torch.tensor([4, 1, 0]), torch.tensor([1, 2, 4])   # equal lengths, one after the other, then again
    for _ in range(2):
        assert fullrank._pairs_of(pos, a)[2].tolist() == [3, 7, 5] and fullrank._pairs_of(pos, b)[2].tolist() == [5, 2, 3, 7]
    kept = fullrank._pairs_of(pos, a)
    assert fullrank._pairs_of(pos, a.view(-1))[0] is kept[0]  # the same memory, unchanged
    a[0] = 2                                                  # a write in place
    got = fullrank._pairs_of(pos, a)
    assert got[0] is not kept[0] and got[1].tolist() == [2, 1] and got[2].tolist() == [2, 5]
    assert fullrank._pairs_of(pos, a[:2].contiguous())[2].tolist() == [2, 5]
    assert pos._entries is not None and not hasattr(pos, "_sorted")   # the sorted arrays are not kept, the distinct entries are
    only_counts = propagate.PositiveLists.from_lists([4, 1, 2], [[7, 3, 7], [5], [2, 2]], 6)
    assert only_counts.distinct.tolist() == [0, 1, 1, 0, 2, 0] and only_counts._entries is None


# ---------------------------------------------------------------------------------------------------------------
# the case table; the tool's arguments
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_path_and_every_shape_of_the_issue():
    reached = set()
    for case in fs.CASES:
        got = fs.paths(case)
        assert got <= fs.ALL_PATHS
        reached |= got
    assert reached == fs.ALL_PATHS
    assert {c.dim for c in fs.CASES} == {1, 3, 4, 5, 16, 17, 63, 64, 90, 256}
    assert {c.n_items for c in fs.CASES} == {1, 2, 127, 128, 129, 257, 641}
    assert {c.n_pairs for c in fs.CASES} == {1, 63, 64, 65, 130}
    assert {s for c in fs.CASES for s in c.slices} == {0, 1, 2, 3, 64}
    assert {c.layout for c in fs.CASES if c.dim % 4 == 0} == {"aligned", "strided"}
    for case in fs.CASES:                                     # p at item 0, 127, 128 and n_items - 1 wherever they exist
        _, _, _, pair_items, ptr, entries = case.build()
        if case.n_pairs >= 63:
            assert {0, case.n_items - 1} <= set(pair_items.tolist())
            assert {i for i in (127, 128) if i < case.n_items} <= set(pair_items.tolist())
        for u in range(case.n_users):                         # the lists are ascending, as the entry point demands
            assert (np.diff(entries[ptr[u]:ptr[u + 1]]) >= 0).all()
    assert fs.slices_used(0, 130, 641) == 6 and fs.slices_used(64, 130, 641) == 6 and fs.slices_used(0, 10 ** 5, 10 ** 5) == 1


def test_train_demo_takes_the_full_rank_flag_and_defaults_to_off():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_demo
    finally:
        sys.path.pop(0)
    args = train_demo.parse_args([])
    assert args.full_rank is False and args.hard_negatives == 0 and args.k == 20 and args.epochs == 3
    args = train_demo.parse_args(["--full-rank", "--hard-negatives", "8", "--refresh", "10", "--epochs", "20"])
    assert args.full_rank is True and args.hard_negatives == 8 and args.refresh == 10 and args.epochs == 20
    with pytest.raises(SystemExit):
        train_demo.parse_args(["--full-rank", "yes"])
