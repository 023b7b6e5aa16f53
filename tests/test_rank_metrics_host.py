"""CPU-only checks of the ranking metrics (lgc_rank_metrics / lgc_column_sums / lgc_topk_coverage and the Python above
them): the three names in the header, the ctypes table and the library at ABI 14, argument validation that happens
before any launch, the numpy restatement the GPU tests use as their reference against hand-computed rows and against
the class's own MARK_MAPK, and PositiveLists.distinct."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate
from gnn_ecommerce_amd.propagate import PositiveLists
from rank_metrics_support import AP, HIT, NDCG, PRECISION, RECALL, RR, csr, discount, reference, reference_frame

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_RANGE = -1, -4
NEW = ("lgc_rank_metrics", "lgc_column_sums", "lgc_topk_coverage")


def cut_array(*values):
    return (ctypes.c_int32 * max(len(values), 1))(*values)


def test_three_new_entry_points_at_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", code) and name in _native.SIGNATURES and hasattr(lib, name)
        assert _native.SIGNATURES[name][1][-1] is ctypes.c_void_p                    # the last argument is the stream
    defines = dict(re.findall(r"#define (LGC_RM_[A-Z_]+|LGC_COLUMN_SUMS_MAX)\s+(\d+)", code))
    assert [int(defines[f"LGC_RM_{n}"]) for n in ("PRECISION", "RECALL", "NDCG", "AP", "RR", "HIT", "COUNT")] == list(range(7))
    assert (_native.RM_PRECISION, _native.RM_RECALL, _native.RM_NDCG, _native.RM_AP, _native.RM_RR, _native.RM_HIT,
            _native.RM_COUNT) == tuple(range(7)) == (PRECISION, RECALL, NDCG, AP, RR, HIT, 6)
    assert int(defines["LGC_RM_MAX_CUTOFFS"]) == _native.RM_MAX_CUTOFFS == 8
    assert int(defines["LGC_COLUMN_SUMS_MAX"]) == _native.COLUMN_SUMS_MAX == 64
    assert propagate.METRIC_NAMES == ("precision", "recall", "ndcg", "map", "mrr", "hit_rate")
    for name in ("rank_metrics", "evaluate_ranking", "overlap_items", "metrics_frame", "RankingResult"):
        assert name in lg.__all__ and hasattr(lg, name)
    assert hasattr(lg.LightGCN, "evaluate_metrics")


def test_rank_metrics_argument_errors_come_before_any_launch():
    lib = _native.load()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below must end in validation

    def rank(**kw):
        a = dict(topk=one, ts=20, k=20, ptr=one, items=one, distinct=one, rows=one, n=4, nu=10, cuts=cut_array(5, 10, 20),
                 nc=3, bits=one, hits=one, metrics=one, status=one)
        a.update(kw)
        return lib.lgc_rank_metrics(a["topk"], a["ts"], a["k"], a["ptr"], a["items"], a["distinct"], a["rows"], a["n"],
                                    a["nu"], a["cuts"], a["nc"], a["bits"], a["hits"], a["metrics"], a["status"], None)
    for bad in (dict(topk=None), dict(ptr=None), dict(hits=None), dict(metrics=None), dict(status=None), dict(cuts=None),
                dict(n=-1), dict(nu=-1), dict(k=0), dict(ts=19), dict(nc=0), dict(nc=9, cuts=cut_array(*range(1, 10))),
                dict(cuts=cut_array(5, 5, 20)), dict(cuts=cut_array(10, 5, 20)), dict(cuts=cut_array(0, 5, 20)),
                dict(cuts=cut_array(5, 10, 21)), dict(cuts=cut_array(21), nc=1)):
        assert rank(**bad) == E_INVAL, bad
    assert rank(k=257, ts=257) == E_RANGE and rank(n=2 ** 31) == E_RANGE
    assert rank(k=256, ts=300, cuts=cut_array(5, 10, 257)) == E_RANGE                # a cutoff above 256
    assert rank(n=0) == 0 and rank(n=0, rows=None, items=None, distinct=None, bits=None) == 0
    assert rank(n=0, nc=8, k=256, ts=256, cuts=cut_array(1, 2, 63, 64, 65, 128, 192, 256)) == 0
    assert rank(n=0, cuts=cut_array(5, 5, 20)) == E_INVAL                             # still validated


def test_column_sums_and_coverage_argument_errors_come_before_any_launch():
    lib = _native.load()
    one = ctypes.c_void_p(16)
    sums = lib.lgc_column_sums
    assert sums(one, 6, 5, 6, None, None) == E_INVAL                                  # no output
    assert sums(None, 6, 5, 6, one, None) == E_INVAL                                  # rows without an input
    assert sums(one, 6, -1, 6, one, None) == E_INVAL and sums(one, 6, 5, 0, one, None) == E_INVAL
    assert sums(one, 5, 5, 6, one, None) == E_INVAL                                   # stride below the width
    assert sums(one, 65, 5, 65, one, None) == E_RANGE and sums(one, 65, 0, 65, one, None) == E_RANGE
    assert sums(one, 64, 0, 64, one, None) == 0 and sums(None, 6, 0, 6, one, None) == 0   # no rows: nothing written

    def cover(**kw):
        a = dict(topk=one, ts=20, k=20, n=4, cuts=cut_array(5, 10, 20), nc=3, ni=300, bitmap=one, counts=one, status=one)
        a.update(kw)
        return lib.lgc_topk_coverage(a["topk"], a["ts"], a["k"], a["n"], a["cuts"], a["nc"], a["ni"], a["bitmap"],
                                     a["counts"], a["status"], None)
    for bad in (dict(topk=None), dict(bitmap=None), dict(counts=None), dict(status=None), dict(cuts=None), dict(n=-1),
                dict(ni=0), dict(ni=-3), dict(k=0), dict(ts=19), dict(nc=0), dict(nc=9, cuts=cut_array(*range(1, 10))),
                dict(cuts=cut_array(5, 5, 20)), dict(cuts=cut_array(5, 10, 21))):
        assert cover(**bad) == E_INVAL, bad
    assert cover(k=257, ts=257) == E_RANGE and cover(n=2 ** 31) == E_RANGE and cover(ni=2 ** 31) == E_RANGE
    assert cover(k=256, ts=256, cuts=cut_array(5, 10, 300)) == E_RANGE


def test_python_wrappers_refuse_bad_cutoffs_without_a_device():
    for bad in ((), tuple(range(1, 10)), (5, 5), (10, 5), (0, 5), (5, 30)):
        with pytest.raises(ValueError):
            propagate._host_cutoffs(bad, 20)
    cuts, arr = propagate._host_cutoffs((5, 10, 20), 20)
    assert cuts == [5, 10, 20] and list(arr) == [5, 10, 20]
    with pytest.raises(_native.NativeLibraryError):                                   # no CPU route: a host tensor is refused
        propagate.rank_metrics(torch.zeros((2, 5), dtype=torch.int64), PositiveLists.from_lists([0], [[1]], 2),
                               torch.zeros(2, dtype=torch.int64), (5,))


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement against known answers
# ---------------------------------------------------------------------------------------------------------------
def d(j):
    return float(discount(j))


def test_restatement_on_hand_computed_rows():
    lists = [[50, 51], [10], [1, 2, 3, 4], [20, 21, 22, 23, 24, 25], [7, 9, 7]]
    ptr, items = csr(lists)
    topk = np.array([[1, 2, 3, 4],          # user 0: no hit
                     [10, 2, 3, 4],         # user 1: a hit at position 0 only
                     [4, 3, 2, 1],          # user 2: all hits
                     [20, 9, 21, 8],        # user 3: a list longer than c
                     [5, 7, 9, 6]])         # user 4: a list with a duplicate (len 3, 2 distinct)
    hits, m, bits = reference(topk, ptr, items, [0, 1, 2, 3, 4], (2, 4))
    assert hits.tolist() == [[0, 0], [1, 1], [2, 4], [1, 2], [1, 2]]
    assert bits[:, 0].tolist() == [0b0000, 0b0001, 0b1111, 0b0101, 0b0110] and not bits[:, 1:].any()
    assert m[0].tolist() == [[0.0] * 6] * 2
    assert m[1].tolist() == [[1 / 2, 1.0, 1.0, 1.0, 1.0, 1.0], [1 / 4, 1.0, 1.0, 1.0, 1.0, 1.0]]
    assert m[2, 0].tolist() == [1.0, 2 / 4, 1.0, 1.0, 1.0, 1.0] and m[2, 1].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    # user 3, six positives: hits at 0 and 2
    assert m[3, 0].tolist() == [1 / 2, 1 / 6, d(0) / (d(0) + d(1)), (1 / 1) / 2, 1.0, 1.0]
    assert m[3, 1, PRECISION] == 2 / 4 and m[3, 1, RECALL] == 2 / 6 and m[3, 1, RR] == 1.0 and m[3, 1, HIT] == 1.0
    assert abs(m[3, 1, NDCG] - (d(0) + d(2)) / (d(0) + d(1) + d(2) + d(3))) <= 1e-15
    assert abs(m[3, 1, AP] - (1 / 1 + 2 / 3) / 4) <= 1e-15
    # user 4: recall divides by the length with the duplicate (3), the ideal ranking and AP have 2 distinct items
    assert m[4, 0].tolist() == [1 / 2, 1 / 3, d(1) / (d(0) + d(1)), (1 / 2) / 2, 1 / 2, 1.0]
    assert m[4, 1, RECALL] == 2 / 3 and m[4, 1, RR] == 1 / 2
    assert abs(m[4, 1, NDCG] - (d(1) + d(2)) / (d(0) + d(1))) <= 1e-15 and abs(m[4, 1, AP] - (1 / 2 + 2 / 3) / 2) <= 1e-15
    # a user outside the lists: an all-zero row; a user without a list: 0 / 0
    hits, m, bits = reference(topk[:2], ptr, items, [5, -1], (4,))
    assert not hits.any() and not m.any() and not bits.any()
    ptr2, items2 = csr([[], [10]])
    hits, m, _ = reference(topk[:1], ptr2, items2, [0], (4,))
    assert hits.tolist() == [[0]] and m[0, 0, PRECISION] == 0.0 and m[0, 0, RR] == 0.0 and m[0, 0, HIT] == 0.0
    assert np.isnan(m[0, 0, [RECALL, NDCG, AP]]).all()


def test_restatement_is_mark_mapk_on_a_random_frame():
    import pandas as pd
    rng = np.random.default_rng(5)
    n_users, n_items, k = 30, 40, 6
    listed = rng.permutation(n_users)[:20]
    lists = [rng.integers(n_items, size=int(rng.integers(1, 9))).tolist() for _ in listed]      # duplicates happen
    assert any(len(set(x)) < len(x) for x in lists)
    pos_df = pd.DataFrame({"user_id_idx": listed, "item_id_idx_list": lists})
    topk = np.stack([rng.permutation(n_items)[:k] for _ in listed])
    top_df = pd.DataFrame({"user_ID": listed, "top_rlvnt_itm": topk.tolist()})
    precision, recall, frame = lg.LightGCN(n_users + n_items, 8, 1).MARK_MAPK(pos_df, top_df, k)
    pos = PositiveLists.from_frame(pos_df, n_users).validate(n_users, n_items)
    hits, m, _ = reference(topk, pos.ptr.numpy(), pos.items.numpy(), listed, (3, k))
    assert hits[:, 1].sum() > 0
    assert m[:, 1, PRECISION].tolist() == frame["precision"].tolist() and m[:, 1, RECALL].tolist() == frame["recall"].tolist()
    assert abs(m[:, 1, PRECISION].mean() - precision) <= 1e-15 and abs(m[:, 1, RECALL].mean() - recall) <= 1e-15
    mine = reference_frame(pos_df, listed, topk, pos.ptr.numpy(), pos.items.numpy(), k)
    assert list(mine.columns) == list(frame.columns) and list(mine.dtypes) == list(frame.dtypes) and len(mine) == len(frame)
    assert [set(o) for o in mine["overlap_item"]] == [set(o) for o in frame["overlap_item"]]
    assert [len(o) for o in mine["overlap_item"]] == [len(o) for o in frame["overlap_item"]]
    for col in ("user_id_idx", "item_id_idx_list", "user_ID", "top_rlvnt_itm", "recall", "precision"):
        assert mine[col].tolist() == frame[col].tolist(), col


# ---------------------------------------------------------------------------------------------------------------
# PositiveLists.distinct
# ---------------------------------------------------------------------------------------------------------------
def test_distinct_counts_with_and_without_duplicates_and_for_users_without_a_list():
    pos = PositiveLists.from_lists([4, 1, 6, 2], [[3, 9, 3], [0], [7, 8], [5, 5, 5, 5]], 8)
    assert pos._distinct is None                                                      # lazy
    got = pos.distinct
    assert got.dtype == torch.int64 and got.tolist() == [0, 1, 1, 0, 2, 0, 2, 0]
    assert (pos.ptr[1:] - pos.ptr[:-1]).tolist() == [0, 1, 4, 0, 3, 0, 2, 0]          # the lengths keep the duplicates
    assert pos.distinct is got                                                        # kept
    moved = pos.to("cpu")
    assert moved._distinct is not None and torch.equal(moved.distinct, got)           # carried along
    assert PositiveLists.from_arrays([0, 0, 0], [], []).distinct.tolist() == [0, 0]   # no entries at all
    same = PositiveLists.from_arrays(pos.ptr, pos.items, pos.users)                   # the constructors stay call-compatible
    assert same._distinct is None and same.distinct.tolist() == got.tolist()
    rng = np.random.default_rng(2)
    lists = [rng.integers(12, size=int(rng.integers(0, 30))).tolist() for _ in range(50)]
    ptr, items = csr(lists)
    big = PositiveLists.from_arrays(ptr, items, np.arange(50))
    assert big.distinct.tolist() == [len(set(x)) for x in lists]


# ---------------------------------------------------------------------------------------------------------------
# the host side of the frame: overlap_items and metrics_frame on a result assembled from the restatement
# ---------------------------------------------------------------------------------------------------------------
def test_metrics_frame_from_bits_is_mark_mapks_frame():
    import pandas as pd
    from gnn_ecommerce_amd.propagate import RankingResult, metrics_frame, overlap_items
    rng = np.random.default_rng(1)
    n_users, n_items, k = 30, 40, 20
    listed = rng.permutation(n_users)[:12].tolist()
    lists = [rng.integers(n_items, size=int(rng.integers(1, 9))).tolist() for _ in listed]
    listed.append(listed[2])                                                          # a user evaluated twice
    lists.append(lists[2])
    pos_df = pd.DataFrame({"user_id_idx": listed, "item_id_idx_list": lists})
    pos = PositiveLists.from_frame(pos_df, n_users)
    topk = np.stack([rng.permutation(n_items)[:k] for _ in listed])
    topk[-1] = topk[2]
    hits, m, bits = reference(topk, pos.ptr.numpy(), pos.items.numpy(), listed, (5, k))
    res = RankingResult((5, k), {}, torch.tensor(listed), torch.from_numpy(topk), torch.from_numpy(hits), torch.from_numpy(m),
                        torch.from_numpy(bits.view(np.int64)))
    assert [len(o) for o in overlap_items(res.topk, res.hit_bits)] == hits[:, 1].tolist()
    assert [len(o) for o in overlap_items(res.topk, res.hit_bits, 5)] == hits[:, 0].tolist()
    for c in (5, k):
        mine = metrics_frame(pos_df, res, None if c == k else c)
        top_df = pd.DataFrame({"user_ID": listed[:-1], "top_rlvnt_itm": topk[:-1, :c].tolist()})
        _, _, frame = lg.LightGCN(n_users + n_items, 8, 1).MARK_MAPK(pos_df, top_df, c)
        assert list(mine.columns) == list(frame.columns) and list(mine.dtypes) == list(frame.dtypes) and len(mine) == len(frame)
        for col in ("user_id_idx", "item_id_idx_list", "user_ID", "top_rlvnt_itm", "recall", "precision"):
            assert mine[col].tolist() == frame[col].tolist(), col
        assert [set(o) for o in mine["overlap_item"]] == [set(o) for o in frame["overlap_item"]]
        ref = reference_frame(pos_df, listed, topk, pos.ptr.numpy(), pos.items.numpy(), c)
        assert mine["overlap_item"].tolist() == ref["overlap_item"].tolist()         # the ranking's order
    with pytest.raises(ValueError):
        metrics_frame(pos_df, res, 7)                                                 # not one of the result's cutoffs
