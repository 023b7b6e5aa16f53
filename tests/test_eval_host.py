"""CPU-only checks of the epoch evaluation (lgc_score_rows / lgc_topk_hits / lgc_metric_sums and the Python above
them): the ABI number, argument validation that happens before any launch, the panel arithmetic, the dense-mask and
positive-list converters, and a numpy restatement of hits / recall against the class's own MARK_MAPK."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native
from gnn_ecommerce_amd.propagate import DEFAULT_WORKSPACE_BYTES, PositiveLists, SeenLists, panel_rows

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_DIM, E_RANGE = -1, -2, -4


def test_abi_14_in_header_library_and_binding():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("lgc_score_rows", "lgc_topk_hits", "lgc_metric_sums"):
        assert re.search(rf"\bint {name}\s*\(", code) and name in _native.SIGNATURES and hasattr(lib, name)
        assert _native.SIGNATURES[name][1][-1] is ctypes.c_void_p                    # the last argument is the stream


def test_score_rows_argument_errors_come_before_any_launch():
    lib = _native.load()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below must end in validation

    def score(**kw):
        a = dict(users=one, us=96, nu=10, ids=one, n=4, items=one, its=96, ni=7, dim=90, out=one, os=7, status=one)
        a.update(kw)
        return lib.lgc_score_rows(a["users"], a["us"], a["nu"], a["ids"], a["n"], a["items"], a["its"], a["ni"], a["dim"],
                                  a["out"], a["os"], a["status"], None)
    for dim in (0, -1, 257, 300):
        assert score(dim=dim) == E_DIM
    for bad in (dict(users=None), dict(items=None), dict(out=None), dict(status=None), dict(n=-1), dict(nu=-1), dict(ni=0),
                dict(us=89), dict(its=89), dict(os=6)):
        assert score(**bad) == E_INVAL, bad
    assert score(n=2 ** 31) == E_RANGE and score(nu=2 ** 31) == E_RANGE
    assert score(n=0) == 0 and score(n=0, ids=None) == 0                              # nothing to do: no launch
    assert score(n=0, dim=300) == E_DIM                                               # still validated


def test_topk_hits_and_metric_sums_argument_errors_come_before_any_launch():
    lib = _native.load()
    one = ctypes.c_void_p(16)

    def hits(**kw):
        a = dict(topk=one, ts=20, k=20, ptr=one, items=one, rows=one, n=4, nu=10, hits=one, recall=one, status=one)
        a.update(kw)
        return lib.lgc_topk_hits(a["topk"], a["ts"], a["k"], a["ptr"], a["items"], a["rows"], a["n"], a["nu"], a["hits"],
                                 a["recall"], a["status"], None)
    for bad in (dict(topk=None), dict(ptr=None), dict(hits=None), dict(recall=None), dict(status=None), dict(n=-1),
                dict(nu=-1), dict(k=0), dict(ts=19)):
        assert hits(**bad) == E_INVAL, bad
    assert hits(k=257, ts=257) == E_RANGE and hits(n=2 ** 31) == E_RANGE
    assert hits(n=0) == 0 and hits(n=0, rows=None, items=None) == 0
    sums = lib.lgc_metric_sums
    assert sums(one, one, 5, None, None, None) == E_INVAL                             # nothing asked for
    assert sums(None, one, 5, one, one, None) == E_INVAL                              # a sum without its input
    assert sums(one, None, 5, one, one, None) == E_INVAL
    assert sums(one, one, -1, one, one, None) == E_INVAL
    assert sums(one, one, 0, one, one, None) == 0 and sums(None, None, 0, one, None, None) == 0


def test_panel_arithmetic():
    assert DEFAULT_WORKSPACE_BYTES == 64 << 20
    assert panel_rows(54571) == (64 << 20) // (4 * 54571) == 307
    assert panel_rows(54571, 16 << 20) == 76 and panel_rows(54571, 256 << 20) == 1229
    assert panel_rows(20000, 4 << 20) == 52
    assert panel_rows(1025, 4 * 1025 * 7) == 7 and panel_rows(1025, 4 * 1025 * 7 - 1) == 6
    assert panel_rows(10 ** 6, 1024) == 1 and panel_rows(1, 0) == 1                    # never less than one row
    for n_items, ws in ((54571, 64 << 20), (800, 1 << 20), (65537, 4 << 20)):
        rows = panel_rows(n_items, ws)
        assert rows * n_items * 4 <= ws < (rows + 1) * n_items * 4


def test_from_dense_round_trips_and_refuses_what_lists_cannot_say():
    gen = torch.Generator().manual_seed(3)
    n_users, n_items = 40, 57
    users = [31, 2, 17, 39, 0, 8]
    mask = (torch.rand(len(users), n_items, generator=gen) < 0.2).float()
    mask[2] = 0.0                                                                     # a user without purchases
    mask[3] = 1.0                                                                     # one who bought everything
    lists = SeenLists.from_dense(mask, users, n_users).validate(n_users)
    assert lists.ptr.dtype == torch.int64 and lists.ptr.shape == (n_users + 1,) and lists.items.dtype == torch.int64
    assert torch.equal(lists.to_dense(users, n_items), mask)
    others = [u for u in range(n_users) if u not in users]
    assert lists.to_dense(others, n_items).sum() == 0                                 # unlisted users: empty rows
    assert int(lists.ptr[-1]) == int(mask.sum())
    for u, row in zip(users, mask):                                                   # items ascending within a user
        assert lists.items[lists.ptr[u]:lists.ptr[u + 1]].tolist() == row.nonzero().flatten().tolist()
    # cached on the tensor's identity and version: the same object until the mask is written to
    builds = SeenLists.dense_builds
    assert SeenLists.from_dense(mask, users, n_users) is lists and SeenLists.dense_builds == builds
    mask[0, 0] = 1.0 - mask[0, 0]
    again = SeenLists.from_dense(mask, users, n_users)
    assert again is not lists and SeenLists.dense_builds == builds + 1 and torch.equal(again.to_dense(users, n_items), mask)
    # a user listed twice: fine with equal rows, refused with different ones
    twice = torch.cat([mask, mask[1:2]])
    assert torch.equal(SeenLists.from_dense(twice, users + [users[1]], n_users).to_dense(users, n_items), mask)
    twice[-1, 5] = 1.0 - twice[-1, 5]
    with pytest.raises(ValueError, match="twice"):
        SeenLists.from_dense(twice, users + [users[1]], n_users)
    for value in (2.0, 0.5, -1.0, float("nan")):                                      # upstream sums a repeated purchase to 2
        bad = mask.clone()
        bad[4, 9] = value
        with pytest.raises(ValueError, match="other than 0 and 1"):
            SeenLists.from_dense(bad, users, n_users)
    with pytest.raises(ValueError):
        SeenLists.from_dense(mask, users[:-1], n_users)                               # rows and users disagree
    with pytest.raises(ValueError):
        SeenLists.from_dense(mask, users[:-1] + [n_users], n_users)                   # a user outside the table


def test_positive_lists_from_a_frame_and_the_empty_list():
    import pandas as pd
    frame = pd.DataFrame({"user_id_idx": [4, 1, 6], "item_id_idx_list": [[3, 9, 3], [0], [7, 8]]})
    pos = PositiveLists.from_frame(frame, 8).validate(8, 10)
    assert pos.users.tolist() == [4, 1, 6]
    assert pos.ptr.tolist() == [0, 0, 1, 1, 1, 4, 4, 6, 6] and pos.items.tolist() == [0, 3, 9, 3, 7, 8]   # duplicates kept
    same = PositiveLists.from_arrays(pos.ptr.numpy(), pos.items.tolist(), [4, 1, 6]).validate(8)
    assert torch.equal(same.ptr, pos.ptr) and torch.equal(same.items, pos.items)
    empty = pd.DataFrame({"user_id_idx": [4, 1], "item_id_idx_list": [[3], []]})
    with pytest.raises(ValueError, match="empty"):
        PositiveLists.from_frame(empty, 8).validate(8)
    with pytest.raises(ValueError, match="empty"):
        PositiveLists.from_arrays(pos.ptr, pos.items, [4, 0]).validate(8)               # user 0 is listed but has no items
    with pytest.raises(ValueError):
        PositiveLists.from_frame(frame, 8).validate(8, 9)                             # item 9 outside 9 columns
    with pytest.raises(ValueError):
        PositiveLists.from_frame(frame, 6)                                            # user 6 outside 6 users
    with pytest.raises(ValueError, match="twice"):
        PositiveLists.from_lists([4, 4], [[1], [2]], 8)
    assert PositiveLists.from_lists([4, 4], [[1, 2], [1, 2]], 8).validate(8).users.tolist() == [4, 4]


def hits_and_recall(topk, ptr, items, users):
    """What lgc_topk_hits computes, restated: distinct top-k entries found in the user's list; the list's length, with
    duplicates, underneath."""
    hits = np.array([sum(1 for t in row if t in set(items[ptr[u]:ptr[u + 1]])) for row, u in zip(topk, users)])
    return hits, hits / np.array([ptr[u + 1] - ptr[u] for u in users], dtype=np.float64)


def test_numpy_restatement_of_hits_and_recall_is_mark_mapk():
    import pandas as pd
    k = 4
    pos_df = pd.DataFrame({"user_id_idx": [5, 2, 7, 2], "item_id_idx_list": [[1, 9, 1, 4], [3], [0, 6, 8], [3]]})
    top_df = pd.DataFrame({"user_ID": [2, 5, 7], "top_rlvnt_itm": [[9, 3, 0, 1], [1, 2, 4, 7], [5, 4, 3, 2]]})
    precision, recall, frame = lg.LightGCN(12, 8, 1).MARK_MAPK(pos_df, top_df, k)
    pos = PositiveLists.from_frame(pos_df, 8).validate(8, 10)
    users = pos.users.tolist()
    top = {u: row for u, row in zip(top_df["user_ID"], top_df["top_rlvnt_itm"])}
    hits, rec = hits_and_recall([top[u] for u in users], pos.ptr.tolist(), pos.items.tolist(), users)
    assert hits.tolist() == [len(o) for o in frame["overlap_item"]] == [2, 1, 0, 1]   # item 1 is listed twice: one hit
    assert rec.tolist() == frame["recall"].tolist() == [2 / 4, 1.0, 0.0, 1.0]         # ... but counts twice underneath
    assert abs(hits.sum() / (k * len(users)) - precision) <= 1e-15 and abs(rec.mean() - recall) <= 1e-15
