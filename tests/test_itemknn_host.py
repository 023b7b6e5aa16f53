"""CPU-only checks of the item-kNN recommender: the two entry points in the header (an addition to ABI 14), the ctypes table
and the library; their argument validation, which happens before any launch and touches no output; the workspace size; the
numpy reference on hand-worked tables whose answers are written out; the two order cases against exact arithmetic, with
mutants that give other bits; the torch restatement of ``knn_recommend`` against the reference on every case; ``ItemKNN``
on CPU tensors against a dict-of-lists restatement; the argument checks of the model method and the handler's parser; and
the case table of the device tests held to what it has to reach.  No tolerance anywhere: bits and integers."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, cooccur, itemknn, serving
import cooccur_support as cs
import itemknn_support as ks
import topk_support as ts

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_WORKSPACE, E_RANGE, E_ALIGN = -1, -3, -4, -5
NAMES = ("lgc_knn_workspace_bytes", "lgc_knn_recommend")


def test_entry_points_are_declared_bound_and_exported_as_an_addition_to_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    assert "Item-kNN recommender (an addition to ABI 14: exports only)" in header
    assert int(re.search(r"#define LGC_KNN_MAX_K (\d+)", header).group(1)) == _native.KNN_MAX_K == ks.MAX_K == 64
    assert int(re.search(r"#define LGC_KNN_MAX_NEIGHBORS (\d+)", header).group(1)) == _native.KNN_MAX_NEIGHBORS == ks.MAX_NEIGHBORS == 64
    assert int(re.search(r"#define LGC_KNN_MAX_BAND (\d+)", header).group(1)) == _native.KNN_MAX_BAND == ks.MAX_BAND == 16384
    assert _native.KNN_MAX_NEIGHBORS == _native.COOCCUR_MAX_K == _native.NEIGHBORS_MAX_K      # what the two producers build
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        decl = re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert decl, name
        restype, argtypes = _native.SIGNATURES[name]
        assert hasattr(lib, name)
        assert restype is (ctypes.c_size_t if decl.group(1) == "size_t" else ctypes.c_int)
        args = [a.strip() for a in decl.group(2).split(",")]
        assert re.fullmatch(r"void\s*\*\s*stream", args[-1]), name                     # both end in the stream
        want = []
        for arg in args:
            kind = "ptr" if "*" in arg else re.match(r"(?:const\s+)?(\w+)", arg).group(1)
            want.append({"ptr": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
                         "size_t": ctypes.c_size_t}[kind])
        assert want == list(argtypes), name
    for name in ("knn_recommend", "ItemKNN"):
        assert name in lg.__all__ and hasattr(lg, name)
    assert hasattr(lg.LightGCN, "recommend_itemknn")
    for name in ("parse_itemknn", "inference_itemknn"):
        assert hasattr(serving.RecommendHandler, name)
    makefile = open(os.path.join(ROOT, "gnn-ecommerce_amd", "csrc", "Makefile")).read()
    assert "lgconv_itemknn" in re.search(r"^UNITS\s*:=((?:.*\\\n)*.*)$", makefile, flags=re.M).group(1).split()
    unit = open(os.path.join(ROOT, "gnn-ecommerce_amd", "csrc", "lgconv_itemknn.hip")).read()
    assert '#include "lgconv_select.h"' in unit
    for restated in ("pack_candidate(float", "compact_row(u64", "merge_keep(u64", "write_candidate(int64_t", "order_key(float"):
        assert restated not in unit, restated                                           # the selection keeps its one copy
    assert "atomicAdd" not in unit and "embedding" not in unit.split("namespace")[1]    # no float atomics, no embedding


# addresses of host words: valid, 16-byte aligned, never read or written by a call that returns before its launch
_words = (ctypes.c_int64 * 8)()
ONE = ctypes.addressof(_words) + (-ctypes.addressof(_words)) % 16
# the outputs and the status word are real host arrays filled with a sentinel: a refusal must leave them as they are
K0 = 20
_out_index = (ctypes.c_int64 * (4 * K0 + 2))(*([-77] * (4 * K0 + 2)))
_out_value = (ctypes.c_float * (4 * K0 + 4))(*([77.0] * (4 * K0 + 4)))
_out_votes = (ctypes.c_int32 * (4 * K0 + 4))(*([-77] * (4 * K0 + 4)))
_status = (ctypes.c_int32 * 4)(*([0x5A5A] * 4))
OUT_INDEX = ctypes.addressof(_out_index) + (-ctypes.addressof(_out_index)) % 8
OUT_VALUE = ctypes.addressof(_out_value) + (-ctypes.addressof(_out_value)) % 16
OUT_VOTES = ctypes.addressof(_out_votes) + (-ctypes.addressof(_out_votes)) % 16
STATUS = ctypes.addressof(_status)


def outputs_untouched():
    return (all(v == -77 for v in _out_index) and all(v == 77.0 for v in _out_value) and all(v == -77 for v in _out_votes)
            and all(v == 0x5A5A for v in _status))


def call(**kw):
    a = dict(nbr_index=ONE, nbr_value=ONE, nbr_stride=64, n_items=300, kn=64, list_ptr=ONE, list_items=ONE, list_weight=ONE,
             n_lists=50, list_rows=ONE, n_queries=4, item_ok=ONE, exclude_basket=1, min_votes=1, k=K0, band=0,
             out_index=OUT_INDEX, out_value=OUT_VALUE, out_votes=OUT_VOTES, workspace=ONE, workspace_bytes=1 << 40, status=STATUS)
    assert set(kw) <= set(a)
    a.update(kw)
    code = _native.load().lgc_knn_recommend(
        a["nbr_index"], a["nbr_value"], a["nbr_stride"], a["n_items"], a["kn"], a["list_ptr"], a["list_items"], a["list_weight"],
        a["n_lists"], a["list_rows"], a["n_queries"], a["item_ok"], a["exclude_basket"], a["min_votes"], a["k"], a["band"],
        a["out_index"], a["out_value"], a["out_votes"], a["workspace"], a["workspace_bytes"], a["status"], None)
    assert outputs_untouched(), kw
    return code


def ws_bytes(n_queries=100, n_items=1000, k=20, band=0):
    return _native.load().lgc_knn_workspace_bytes(n_queries, n_items, k, band, None)


def test_argument_errors_come_before_any_launch_and_touch_no_output():
    for bad in (dict(nbr_index=None), dict(nbr_value=None), dict(list_ptr=None), dict(list_items=None), dict(out_index=None),
                dict(status=None), dict(n_queries=-1), dict(n_lists=-1), dict(nbr_stride=63), dict(nbr_stride=0, kn=1),
                dict(nbr_stride=-1, kn=1)):
        assert call(**bad) == E_INVAL, bad
    big = (2 ** 31 - 1, 2 ** 31)
    for bad in ([dict(k=0), dict(k=-1), dict(k=65), dict(kn=0), dict(kn=-1), dict(kn=65, nbr_stride=65), dict(band=-64), dict(band=32),
                 dict(band=65), dict(band=100), dict(band=16384 + 64), dict(band=32768), dict(band=2 ** 30), dict(min_votes=0),
                 dict(min_votes=-1), dict(n_items=0), dict(n_items=-1), dict(list_rows=None, n_queries=51),
                 dict(list_rows=None, n_lists=3)]
                + [{name: v} for name in ("n_items", "n_lists", "n_queries") for v in big]):
        assert call(**bad) == E_RANGE, bad
    for name in ("nbr_index", "list_ptr", "list_items", "list_rows", "workspace"):
        assert call(**{name: ONE + 4}) == E_ALIGN, name
    for name in ("nbr_value", "list_weight"):
        assert call(**{name: ONE + 2}) == E_ALIGN and call(**{name: ONE + 4, "n_queries": 0}) == 0      # fp32: dword aligned
    assert call(out_index=OUT_INDEX + 4) == E_ALIGN and call(out_value=OUT_VALUE + 2) == E_ALIGN
    assert call(out_votes=OUT_VOTES + 2) == E_ALIGN and call(status=STATUS + 2) == E_ALIGN
    # the order of the checks: a null pointer before a range before an alignment before the workspace
    assert call(nbr_index=None, k=0) == E_INVAL and call(k=0, list_ptr=ONE + 4) == E_RANGE
    assert call(list_ptr=ONE + 4, workspace=None, band=64) == E_ALIGN
    # the workspace: what the size function says is enough, one byte less is not, none is needed for one band
    for kw in (dict(band=64), dict(band=128), dict(band=256), dict(band=0, n_items=10 ** 5), dict(band=16384, n_items=54571)):
        n_items = kw.get("n_items", 300)
        need = ws_bytes(4, n_items, K0, kw["band"])
        assert need > 0
        assert call(n_queries=0, workspace_bytes=need, **kw) == 0
        assert call(workspace_bytes=0, **kw) == E_WORKSPACE and call(workspace=None, **kw) == E_WORKSPACE
        assert call(workspace_bytes=need - 1, **kw) == E_WORKSPACE
    assert ws_bytes(4, 300, K0, 64) == 4 * 5 * K0 * 12                                  # 4 rows, 5 bands, 20 places of 12 bytes
    assert ws_bytes(4, 300, K0, 128) == 4 * 3 * K0 * 12 and ws_bytes(4, 54571, K0, 0) == 4 * 7 * K0 * 12
    assert ws_bytes(4, 300, K0, 320) == 0 and ws_bytes(4, 300, K0, 0) == 0 and ws_bytes(4, 64, K0, 64) == 0
    assert call(workspace=None, workspace_bytes=0, n_queries=0) == 0                   # one band: no workspace
    # n_queries == 0: validated, nothing launched; the optional pointers may be NULL
    assert call(n_queries=0) == 0
    assert call(n_queries=0, list_weight=None, list_rows=None, item_ok=None, out_value=None, out_votes=None, workspace=None,
                workspace_bytes=0) == 0
    assert call(n_queries=0, n_lists=0, list_rows=None, k=64, kn=1, nbr_stride=1, band=16384, min_votes=2 ** 31 - 1, n_items=1,
                exclude_basket=0) == 0
    assert call(n_queries=0, nbr_stride=63) == E_INVAL and call(n_queries=0, k=65) == E_RANGE      # still validated


def test_workspace_size_refuses_what_the_call_refuses_and_grows_with_every_argument():
    for bad in (dict(n_queries=-1), dict(n_items=0), dict(k=0), dict(k=65), dict(band=-1), dict(band=63), dict(band=96),
                dict(band=16384 + 64), dict(n_queries=2 ** 31 - 1), dict(n_items=2 ** 31 - 1)):
        assert ws_bytes(**bad) == 0, bad
    grid_q = (0, 1, 63, 64, 65, 1000, 54571, 10 ** 6)
    grid_i = (1, 64, 65, 128, 129, 200, 1000, 8192, 8193, 16384, 16385, 54571, 1640000)
    grid_k = (1, 5, 20, 64)
    for band in (0, 64, 128, 192, 256, 8192, 16384):
        for n_items in grid_i:
            for k in grid_k:
                sizes = [ws_bytes(q, n_items, k, band) for q in grid_q]
                assert sizes == sorted(sizes), ("n_queries", band, n_items, k)
        for q in grid_q:
            for k in grid_k:
                sizes = [ws_bytes(q, n_items, k, band) for n_items in grid_i]
                assert sizes == sorted(sizes), ("n_items", band, q, k)
            for n_items in grid_i:
                sizes = [ws_bytes(q, n_items, k, band) for k in grid_k]
                assert sizes == sorted(sizes), ("k", band, q, n_items)
                bands = -(-n_items // min(band or 8192, -(-n_items // 64) * 64))
                assert ws_bytes(q, n_items, 20, band) == (q * bands * 20 * 12 if bands > 1 else 0)
    assert ws_bytes(10 ** 4, 54571, 20, 0) == 10 ** 4 * 7 * 20 * 12                     # 10^4 users of the cosmetics catalogue: 16.8 MB


# ---------------------------------------------------------------------------------------------------------------
# the reference, on a table worked by hand
# ---------------------------------------------------------------------------------------------------------------
#   item 0 -> {1: 0.5, 2: 0.25}   item 1 -> {0: 0.5, 3: 0.125}   item 2 -> {0: 0.25, 3: 0.125, 1: 1.0}   item 3 -> nothing
T_INDEX = np.array([[1, 2, -1], [0, -1, 3], [0, 3, 1], [-1, -1, -1]], dtype=np.int64)
T_VALUE = np.array([[0.5, 0.25, 9.0], [0.5, 9.0, 0.125], [0.25, 0.125, 1.0], [9.0, 9.0, 9.0]], dtype=np.float32)


def ref(baskets, weights=None, rows=None, ok=None, exclude=True, min_votes=1, k=3, index=T_INDEX, value=T_VALUE, kn=3):
    return ks.knn_reference(index, value, kn, ks.csr(baskets, weights), rows, ok, exclude, min_votes, k)


def test_reference_on_the_four_item_table_gives_the_written_answers():
    # basket {0, 1}: item 2 gets 0.25 (one vote), item 3 gets 0.125; items 0 and 1 vote for each other but are in the basket
    idx, val, votes, st = ref([[0, 1]])
    assert st == 0 and idx.tolist() == [[2, 3, -1]] and val.tolist() == [[0.25, 0.125, -np.inf]] and votes.tolist() == [[1, 1, 0]]
    idx, val, votes, _ = ref([[0, 1]], exclude=False)
    assert idx.tolist() == [[0, 1, 2]] and val.tolist() == [[0.5, 0.5, 0.25]] and votes.tolist() == [[1, 1, 1]]      # a tie, by index
    # basket {1, 2}: item 0 gets 0.5 + 0.25, item 3 gets 0.125 + 0.125; two votes each
    idx, val, votes, _ = ref([[1, 2]])
    assert idx.tolist() == [[0, 3, -1]] and val.tolist() == [[0.75, 0.25, -np.inf]] and votes.tolist() == [[2, 2, 0]]
    idx, _, votes, _ = ref([[0, 1], [1, 2], [3], []], min_votes=2)
    assert idx.tolist() == [[-1] * 3, [0, 3, -1], [-1] * 3, [-1] * 3] and votes.tolist() == [[0] * 3, [2, 2, 0], [0] * 3, [0] * 3]
    # weights: 2 * 0.25 = 0.5 for item 2 out of basket entry 0; a repeated entry contributes each time
    idx, val, votes, _ = ref([[0, 1], [0, 0, 0]], [[2.0, 1.0], [1.0, 2.0, 4.0]])
    assert idx.tolist() == [[2, 3, -1], [1, 2, -1]] and val.tolist() == [[0.5, 0.125, -np.inf], [3.5, 1.75, -np.inf]]
    assert votes.tolist() == [[1, 1, 0], [3, 3, 0]]
    # item_ok removes the best item, any non-zero byte allows; rows pick baskets, a bad number is flagged and empty
    idx, _, _, _ = ref([[1, 2]], ok=np.array([0, 1, 1, 200], dtype=np.uint8))
    assert idx.tolist() == [[3, -1, -1]]
    idx, val, votes, st = ref([[0, 1], [1, 2]], rows=np.array([1, 2, 1, -1, 0]), k=2)
    assert st == ks.ST_INDEX_OOB and idx.tolist() == [[0, 3], [-1, -1], [0, 3], [-1, -1], [2, 3]]
    assert np.all(val[[1, 3]] == -np.inf) and votes.tolist() == [[2, 2], [0, 0], [2, 2], [0, 0], [1, 1]]
    assert ref([[0, 1], [1, 2]], rows=np.array([1, 0]))[3] == 0
    # k above the candidate count; kn 2 never reads place 2 (item 2's vote for item 1 is gone)
    assert ref([[2]], k=5)[0].tolist() == [[1, 0, 3, -1, -1]]
    assert ref([[2]], k=5, kn=2)[0].tolist() == [[0, 3, -1, -1, -1]]
    # entries and indices outside the catalogue are skipped and flagged; -1 in the table is silent
    idx, val, _, st = ref([[0, 4, -1, 1]])
    assert st == ks.ST_INDEX_OOB and idx.tolist() == [[2, 3, -1]] and val.tolist() == [[0.25, 0.125, -np.inf]]
    bad = T_INDEX.copy()
    bad[0, 2], bad[1, 1] = 4, -2
    idx, val, _, st = ref([[0, 1]], index=bad)
    assert st == ks.ST_INDEX_OOB and idx.tolist() == [[2, 3, -1]] and val.tolist() == [[0.25, 0.125, -np.inf]]
    assert ref([[2, 3]], index=bad)[3] == 0                                             # those rows are not walked
    # what is written: a NaN score as 0x7FFFFFFF and first, -0 as +0
    value = T_VALUE.copy()
    value[0, 0], value[0, 1] = ts.from_bits([0xFFC00123])[0], ts.from_bits([0x80000000])[0]
    idx, val, _, _ = ref([[0]], value=value)
    assert idx.tolist() == [[1, 2, -1]] and ts.bits_of(val).tolist() == [[0x7FFFFFFF, 0, 0xFF800000]]


def exact(x):
    return Fraction(float(x))


def round32(q):
    """The fp32 nearest to the rational q, ties to even, by exact arithmetic (|q| in the normal range, or 0)."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = 0
    while q >= 2:
        q, e = q / 2, e + 1
    while q < 1:
        q, e = q * 2, e - 1
    scaled = q * 2 ** 23
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    return np.float32(sign * float(Fraction(m, 2 ** 23) * Fraction(2) ** e))


def test_the_two_order_cases_hold_in_exact_arithmetic_and_the_mutants_give_other_bits():
    index, value, kn = ks.table("order")
    lists = ks.csr(ks.ORDER_BASKETS, ks.ORDER_WEIGHTS)
    # 1. the sum order shows: 2^24, 1, 1 in that order stays 2^24; with the 2^24 last it is 2^24 + 2
    big, one = exact(value[0, 0]), exact(value[1, 0])
    assert big == 2 ** 24 and one == 1
    assert round32(exact(round32(big + one)) + one) == np.float32(16777216.0)
    assert round32(exact(round32(one + one)) + big) == np.float32(16777218.0)
    # 2. fusing shows: acc = -(1 + 2^-11), then w = v = 1 + 2^-12: the product rounds to 1 + 2^-11, the sum is +0; fused it is 2^-24
    first, wv = exact(value[4, 0]), exact(value[5, 0])
    assert first == -(1 + Fraction(1, 2 ** 11)) and wv == 1 + Fraction(1, 2 ** 12) == exact(np.float32(ks.ORDER_WEIGHTS[2][1]))
    assert exact(round32(wv * wv)) == -first and round32(first + exact(round32(wv * wv))) == 0
    assert round32(first + wv * wv) == np.float32(2.0 ** -24) == ks.chain.fma32(np.float32(wv), np.float32(wv), np.float32(first))
    for weighted in (False, True):
        got, st = ks.accumulate(index, value, kn, lists, None, weighted)
        assert st == 0 and got[0][0] == {3: np.float32(16777216.0)} and got[1][0] == {3: np.float32(16777218.0)}
        assert got[0][1] == {3: 3} and got[0][2] == {0, 1, 2}
    assert ts.bits_of(got[2][0][6]) == 0 and got[2][0][7] == np.float32(1.0 + 2.0 ** -12) and got[2][1] == {6: 2, 7: 1}
    want = [ks.accumulate(index, value, kn, lists, None, True)[0][r][0] for r in range(3)]
    mutants = {"reversed": dict(entry_order=lambda order, items: order[::-1]),
               "ascending items": dict(entry_order=lambda order, items: sorted(order, key=lambda t: int(items[t]))),
               "fused": dict(fused=True), "weights after the sum": dict(weight_last=True)}
    moved = {"reversed": (0, 1), "ascending items": (1,), "fused": (2,), "weights after the sum": (2,)}
    for name, how in mutants.items():
        got = [ks.accumulate(index, value, kn, lists, None, True, **how)[0][r][0] for r in range(3)]
        for r in moved[name]:
            key = 6 if r == 2 else 3
            assert ts.bits_of(got[r][key]) != ts.bits_of(want[r][key]), (name, r)
    # through the whole reference: the values that come back
    _, val, votes, _ = ks.knn_reference(index, value, kn, lists, None, None, True, 1, 2)
    assert ts.bits_of(val).tolist() == [[0x4B800000, 0xFF800000], [0x4B800001, 0xFF800000], [0x3F800800, 0]]
    assert votes.tolist() == [[3, 0], [3, 0], [1, 2]]


# ---------------------------------------------------------------------------------------------------------------
# knn_recommend's torch restatement (CPU tensors) against the reference, on every case
# ---------------------------------------------------------------------------------------------------------------
def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def host_tables(name):
    index, value, kn = ks.table(name)
    return torch.from_numpy(index)[:, :kn], torch.from_numpy(value)[:, :kn]          # views: the poison stays beside them


def same(got, want, what):
    got = [a.numpy() if torch.is_tensor(a) else a for a in got]
    assert np.array_equal(got[0], want[0]), (what, got[0][:3], want[0][:3])
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(ts.bits_of(got[1]).reshape(want[1].shape), ts.bits_of(want[1]).reshape(want[1].shape)), what


@pytest.mark.parametrize("name", ks.CASE_NAMES)
def test_cpu_restatement_equals_the_reference(name):
    case = ks.CASES[ks.CASE_NAMES.index(name)]
    index, value, kn = ks.table(case["table"])
    n_items = index.shape[0]
    nbr_i, nbr_v = host_tables(case["table"])
    ok = ks.item_mask(case["ok"], n_items)
    for weighted in (False, True):
        lists = ks.csr(case["baskets"], case["weights"] if weighted else None)
        scored, want_st = ks.accumulate(index, value, kn, lists, case["rows"], weighted)
        for min_votes in case["min_votes"]:
            floor = ks.largest_votes(scored) + 1 if min_votes == "max+1" else min_votes
            for exclude in (True, False):
                for k in (5, 64):
                    want = ks.select(scored, n_items, ok, exclude, floor, k)
                    lg.check_index_status()
                    got = itemknn.knn_recommend(nbr_i, nbr_v, n_items, tuple(t(a) for a in lists if a is not None), k,
                                                t(case["rows"]), exclude, floor, t(ok))
                    if want_st:
                        with pytest.raises(IndexError):
                            lg.check_index_status()
                    lg.check_index_status()
                    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
                    same(got, want, (name, weighted, min_votes, exclude, k))


def test_knn_recommend_validates_its_arguments():
    nbr_i, nbr_v = host_tables("kn 7")
    n_items = nbr_i.size(0)
    baskets = tuple(t(a) for a in ks.csr([[1, 2], [3]]))[:2]
    for k in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="k must be"):
            itemknn.knn_recommend(nbr_i, nbr_v, n_items, baskets, k)
    for min_votes in (0, -1, True, 1.0):
        with pytest.raises(ValueError, match="min_votes"):
            itemknn.knn_recommend(nbr_i, nbr_v, n_items, baskets, 3, min_votes=min_votes)
    for band in (-64, 32, 65, 16384 + 64, 64.0, True):
        with pytest.raises(ValueError, match="band"):
            itemknn.knn_recommend(nbr_i, nbr_v, n_items, baskets, 3, band=band)
    with pytest.raises(ValueError, match="catalogue"):
        itemknn.knn_recommend(nbr_i, nbr_v, 0, baskets, 3)
    wide = torch.zeros((n_items, 65), dtype=torch.int64)
    for bad in (dict(nbr_index=nbr_i.to(torch.int32)), dict(nbr_index=nbr_i[:-1]), dict(nbr_index=wide, nbr_value=wide.float()),
                dict(nbr_value=nbr_v.double()), dict(nbr_value=nbr_v.contiguous()), dict(nbr_value=nbr_v[:, :3]),
                dict(baskets=(baskets[0].to(torch.int32), baskets[1])), dict(baskets=(baskets[0],)),
                dict(baskets=(baskets[0], baskets[1], torch.ones(3, dtype=torch.float64))),
                dict(baskets=(baskets[0], baskets[1], torch.ones(2))), dict(rows=torch.zeros(2, dtype=torch.int32)),
                dict(rows=torch.zeros((1, 2), dtype=torch.int64)), dict(item_ok=torch.ones(n_items - 1, dtype=torch.uint8)),
                dict(item_ok=torch.ones(n_items))):
        args = dict(nbr_index=nbr_i, nbr_value=nbr_v, n_items=n_items, baskets=baskets, k=3)
        args.update(bad)
        with pytest.raises(TypeError):
            itemknn.knn_recommend(**args)
    index, value, votes = itemknn.knn_recommend(nbr_i, nbr_v, n_items, baskets, 3, torch.zeros(0, dtype=torch.int64))
    assert index.shape == (0, 3) and value.shape == (0, 3) and votes.shape == (0, 3)
    index, _, _ = itemknn.knn_recommend(nbr_i, nbr_v, n_items, lg.SessionLists(*baskets), 3, item_ok=torch.ones(n_items, dtype=torch.bool),
                                        band=128)
    assert index.shape == (2, 3)


# ---------------------------------------------------------------------------------------------------------------
# ItemKNN on CPU tensors against dicts of lists
# ---------------------------------------------------------------------------------------------------------------
def dict_recommend(neighbours, basket, weights, k, exclude=True):
    """Per candidate the float32 sum in basket order and the votes, ranked by (score descending, index ascending): plain
    Python over {item: [(neighbour, similarity), ...]} (finite positive scores only)."""
    acc, votes = {}, {}
    for i, w in zip(basket, weights):
        for j, s in neighbours[i]:
            acc[j] = np.float32(acc.get(j, np.float32(0)) + np.float32(np.float32(w) * np.float32(s)))
            votes[j] = votes.get(j, 0) + 1
    order = sorted((j for j in acc if not (exclude and j in basket)), key=lambda j: (-float(acc[j]), j))[:k]
    return order, [acc[j] for j in order], [votes[j] for j in order]


def test_itemknn_fit_recommend_and_sessions_equal_a_dict_of_lists():
    g = cs.graph("random 65")
    lists = cooccur.CoPurchase(lg.SeenLists(t(g["seen"][0]), t(g["seen"][1])), lg.BuyerLists(t(g["buyers"][0]), t(g["buyers"][1])),
                               g["n_users"], g["n_items"])
    knn = lg.ItemKNN.fit(lists, kn=8, measure="cosine")
    want = cs.cooccur_reference(g["buyers"], g["seen"], g["n_users"], g["n_items"], None, None, 1, cs.COSINE, 8)
    assert np.array_equal(knn.index.numpy(), want[0]) and np.array_equal(ts.bits_of(knn.value.numpy()), ts.bits_of(want[1]))
    assert knn.n_items == 65 and knn.seen is lists.seen
    neighbours = {i: [(int(j), v) for j, v in zip(want[0][i], want[1][i]) if j >= 0] for i in range(65)}
    bought = cs.rows_of(g["seen"])
    users = [5, 0, 39, 5]
    index, value, votes = knn.recommend(users, k=6)
    for r, u in enumerate(users):
        items, scores, counts = dict_recommend(neighbours, bought[u], [1.0] * len(bought[u]), 6)
        assert index[r, :len(items)].tolist() == items and votes[r, :len(items)].tolist() == counts
        assert np.array_equal(ts.bits_of(value[r, :len(items)].numpy()), ts.bits_of(np.asarray(scores, dtype=np.float32)))
        assert torch.all(index[r, len(items):] == -1) and not set(items) & set(bought[u])
    index, _, _ = knn.recommend(torch.tensor(users), k=6, exclude_seen=False)
    assert index[0].tolist() == dict_recommend(neighbours, bought[5], [1.0] * len(bought[5]), 6, exclude=False)[0]
    # sessions: the weights are the sessions'
    sessions = lg.SessionLists.from_lists([([3, 9, 3], [1.0, 0.1, 0.01]), ([], None), ([64], None)])
    index, value, votes = knn.recommend_sessions(sessions, k=4)
    for r, (basket, weights) in enumerate((([3, 9, 3], [1.0, 0.1, 0.01]), ([], []), ([64], [1.0]))):
        items, scores, counts = dict_recommend(neighbours, basket, weights, 4)
        assert index[r, :len(items)].tolist() == items and votes[r, :len(items)].tolist() == counts
        assert np.array_equal(ts.bits_of(value[r, :len(items)].numpy()), ts.bits_of(np.asarray(scores, dtype=np.float32)))
    # any table: from_neighbors; without purchase lists users cannot be asked
    other = lg.ItemKNN.from_neighbors(knn.index, knn.value, 65)
    assert torch.equal(other.recommend_sessions(sessions, k=4)[0], index)
    with pytest.raises(ValueError, match="purchase lists"):
        other.recommend([1])
    with pytest.raises(TypeError):
        knn.recommend(torch.zeros(2))
    with pytest.raises(TypeError):
        knn.recommend_sessions((sessions.ptr, sessions.items))
    with pytest.raises(TypeError):
        lg.ItemKNN.fit((lists.seen, lists.buyers))
    with pytest.raises(TypeError):
        lg.ItemKNN(knn.index, knn.value, 65, seen=(lists.seen.ptr, lists.seen.items))
    # evaluate ranks on the device only, as every metric of the library
    positives = lg.PositiveLists.from_lists([0, 5], [[1, 2], [3]], g["n_users"])
    for bad in ((), (0, 5), (5, 5), (10, 5), (65,)):
        with pytest.raises(ValueError, match="ks must be"):
            knn.evaluate([0, 5], positives, ks=bad)
    with pytest.raises(_native.NativeLibraryError):
        knn.evaluate([0, 5], positives, ks=(1, 5))


# ---------------------------------------------------------------------------------------------------------------
# the model method validates before it touches a device; the handler's parser, with a stub
# ---------------------------------------------------------------------------------------------------------------
def test_recommend_itemknn_validates_before_it_touches_a_device():
    model = lg.LightGCN(10, 8, 0)
    edges = torch.tensor([[0, 1, 2], [4, 5, 4]], dtype=torch.int64)
    sessions = lg.SessionLists.from_lists([([1], None)])
    with pytest.raises(ValueError, match="nodes"):
        model.recommend_itemknn(edges, None, 4, 7, users=[1])
    with pytest.raises(ValueError, match="exactly one"):
        model.recommend_itemknn(edges, None, 4, 6)
    with pytest.raises(ValueError, match="exactly one"):
        model.recommend_itemknn(edges, None, 4, 6, users=[1], sessions=sessions)
    for k in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="k must be"):
            model.recommend_itemknn(edges, None, 4, 6, users=[1], k=k)
    for kn in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="kn must be"):
            model.recommend_itemknn(edges, None, 4, 6, users=[1], kn=kn)
    with pytest.raises(ValueError, match="measure"):
        model.recommend_itemknn(edges, None, 4, 6, users=[1], measure="dot")
    with pytest.raises(TypeError, match="item_ok"):
        model.recommend_itemknn(edges, None, 4, 6, users=[1], item_ok=torch.ones(4, dtype=torch.bool))
    with pytest.raises(TypeError, match="int64"):
        model.recommend_itemknn(edges, None, 4, 6, users=torch.zeros(2))
    with pytest.raises(TypeError, match="sessions"):
        model.recommend_itemknn(edges, None, 4, 6, sessions=[[1]])
    with pytest.raises(TypeError, match="seen"):
        model.recommend_itemknn(edges, None, 4, 6, users=[1], seen=torch.zeros(1, 6))
    with pytest.raises(TypeError, match="knn"):
        model.recommend_itemknn(edges, None, 4, 6, users=[1], knn="cosine")
    with pytest.raises(ValueError, match="edge_index"):
        model.recommend_itemknn(None, None, 4, 6, users=[1])
    with pytest.raises(_native.NativeLibraryError):                                     # no CPU route through the model's fit
        model.recommend_itemknn(edges, None, 4, 6, users=[1])
    # a prebuilt ItemKNN is taken as it is: here one on CPU tensors, the restatement answers
    index = torch.tensor([[1, -1], [0, 2], [1, -1], [-1, -1], [-1, -1], [-1, -1]], dtype=torch.int64)
    value = torch.tensor([[0.5, 0], [0.5, 0.25], [0.25, 0], [0, 0], [0, 0], [0, 0]])
    seen = lg.SeenLists(torch.tensor([0, 1, 2, 2, 3]), torch.tensor([0, 1, 2]))
    knn = lg.ItemKNN.from_neighbors(index, value, 6, seen)
    got = model.recommend_itemknn(None, None, 4, 6, users=[1, 2, 0], k=2, knn=knn)
    assert got[0].tolist() == [[0, 2], [-1, -1], [1, -1]] and got[2].tolist() == [[1, 1], [0, 0], [1, 0]]
    got = model.recommend_itemknn(None, None, 4, 6, sessions=lg.SessionLists.from_lists([([0, 2], [1.0, 2.0])]), k=2, knn=knn)
    assert got[0].tolist() == [[1, -1]] and got[1][0, 0].item() == 1.0 and got[2].tolist() == [[2, 0]]
    with pytest.raises(TypeError, match="knn"):
        model.recommend_itemknn(None, None, 3, 7, users=[1], knn=knn)


class StubKNN:
    def __init__(self):
        self.calls = []

    def recommend_sessions(self, sessions, k, item_ok=None):
        rows = cs.rows_of((sessions.ptr.numpy(), sessions.items.numpy()))
        self.calls.append((rows, None if sessions.weights is None else sessions.weights.tolist(), k,
                           None if item_ok is None else item_ok.tolist()))
        n = len(rows)
        index = torch.tensor([[r + j for j in range(k)] for r in range(n)], dtype=torch.int64).reshape(n, k)
        value = torch.tensor([[1.0 / (1 + j) for j in range(k)] for _ in range(n)]).reshape(n, k)
        votes = torch.tensor([[k - j for j in range(k)] for _ in range(n)], dtype=torch.int32).reshape(n, k)
        index[:, k - 1:], value[:, k - 1:], votes[:, k - 1:] = -1, -np.inf, 0
        return index, value, votes


class NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was asked for {name}")


def stub_handler():
    h = serving.RecommendHandler()
    h.device, h.n_users, h.n_items, h.k = torch.device("cpu"), 4, 6, 2
    h.graph = None
    h.seen = lg.SeenLists(torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    h.model = NoModel()
    h.copurchase = None
    h.itemknn = StubKNN()
    return h


def test_parse_itemknn_takes_good_bodies():
    h = stub_handler()
    assert h.parse_itemknn({"itemknn": [{"items": [3, 0, 5]}]}) == ([([3, 0, 5], None)], 2, None)
    lists, k, ok = h.parse_itemknn({"itemknn": ({"items": (1, 1), "weights": [0.5, 1]}, {"items": []}), "k": 64, "deny": [3, 0]})
    assert lists == [([1, 1], [0.5, 1]), ([], None)] and k == 64
    assert ok.dtype == torch.uint8 and ok.tolist() == [0, 1, 1, 0, 1, 1]
    assert h.parse_itemknn({"itemknn": [], "allow": [4]})[2].tolist() == [0, 0, 0, 0, 1, 0]
    out = h.handle([{"body": {"itemknn": [{"items": [4, 1], "weights": [1.0, 0.1]}, {"items": [2]}], "k": 3, "deny": [2]}}])[0]
    assert out == {"items": [[0, 1], [1, 2]], "scores": [[1.0, 0.5], [1.0, 0.5]], "votes": [[3, 2], [3, 2]]}          # -1 dropped
    (rows, weights, k, ok), = h.itemknn.calls
    assert rows == [[4, 1], [2]] and k == 3 and ok == [1, 1, 0, 1, 1, 1]
    assert np.array_equal(np.asarray(weights, dtype=np.float32), np.asarray([1.0, 0.1, 1.0], dtype=np.float32))
    assert h.handle([{"body": {"itemknn": []}}]) == [{"items": [], "scores": [], "votes": []}] and len(h.itemknn.calls) == 1


@pytest.mark.parametrize("body", [
    {"itemknn": 3}, {"itemknn": "3"}, {"itemknn": [1]}, {"itemknn": [[1]]}, {"itemknn": None}, {"itemknn": {"items": [1]}},
    {"itemknn": [{"item": [1]}]}, {"itemknn": [{"items": [1], "user": 0}]}, {"itemknn": [{"items": 1}]}, {"itemknn": [{"items": [1.0]}]},
    {"itemknn": [{"items": [True]}]}, {"itemknn": [{"items": [1], "weights": [1, 2]}]}, {"itemknn": [{"items": [1], "weights": ["1"]}]},
    {"itemknn": [{"items": [1], "weights": 1.0}]}, {"itemknn": [{"items": [1], "weights": [True]}]},
    {"itemknn": [{"items": [1]}], "k": 0}, {"itemknn": [{"items": [1]}], "k": 65}, {"itemknn": [{"items": [1]}], "k": None},
    {"itemknn": [{"items": [1]}], "k": True}, {"itemknn": [{"items": [1]}], "allow": [1], "deny": [2]},
    {"itemknn": [{"items": [1]}], "allow": 1}, {"itemknn": [{"items": [1]}], "deny": ["1"]}, {"itemknn": [{"items": [1]}], "measure": "cosine"},
    {"itemknn": [{"items": [1]}], "min_votes": 2}, {"itemknn": [{"items": [1]}], "similar": [1]},
    {"itemknn": [{"items": [1]}], "bought_together": [1]}, {"itemknn": [{"items": [1]}], "requests": [1]}])
def test_parse_itemknn_refuses_malformed_bodies(body):
    h = stub_handler()
    with pytest.raises(ValueError):
        h.inference(body)
    assert h.itemknn.calls == []


def test_itemknn_body_refuses_ids_outside_the_catalogue_and_other_bodies_are_answered_as_before():
    for body in ({"itemknn": [{"items": [6]}]}, {"itemknn": [{"items": [0, -1]}]}, {"itemknn": [{"items": [0]}], "deny": [6]},
                 {"itemknn": [{"items": [0]}], "allow": [-1]}):
        h = stub_handler()
        with pytest.raises(IndexError):
            h.inference(body)
        assert h.itemknn.calls == []
    h = stub_handler()
    with pytest.raises(ValueError, match="'requests' and 'explain'"):                   # a dict without the key: the older parsers
        h.inference({"k": 3})
    with pytest.raises(ValueError, match="bought_together"):
        h.inference({"bought_together": [1], "itemknn": []})


# ---------------------------------------------------------------------------------------------------------------
# the case table of the device tests reaches what it has to
# ---------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_edge_of_the_geometry():
    assert len(set(ks.CASE_NAMES)) == len(ks.CASES) and {c["table"] for c in ks.CASES} == set(ks.TABLES)
    assert all(c["why"] for c in ks.CASES)
    tables = {name: ks.table(name) for name in ks.TABLES}
    sizes = {idx.shape[0] for idx, _, _ in tables.values()}
    assert max(sizes) <= 200 and {1, 65, 129, 130, 200} <= sizes                        # band 64: up to four bands, last bands of one item
    assert {kn for _, _, kn in tables.values()} >= {1, 7, 64}
    for name, (idx, val, kn) in tables.items():
        n_items = idx.shape[0]
        assert idx.shape[1] > kn, name                                                  # a stride above kn, the padding poisoned
        assert np.all((idx[:, kn:] < -1) | (idx[:, kn:] >= n_items)) and np.all(np.isnan(val[:, kn:])), name
        for row in idx[:, :kn]:
            valid = row[(row >= 0) & (row < n_items)]
            assert len(set(valid.tolist())) == valid.size, name                         # the valid indices of a row are distinct
    lengths = {len(b) for c in ks.CASES for b in c["baskets"]}
    assert {0, 1, 63, 64, 65, 127, 128, 129} <= lengths and max(lengths) >= 130          # both sides of 64 and 128 entries
    assert any(len(set(b)) < len(b) for c in ks.CASES for b in c["baskets"])            # repeated entries
    assert {1, 2, "max+1"} <= set().union(*[set(c["min_votes"]) for c in ks.CASES])
    assert {c["ok"] for c in ks.CASES} == {"none", "zero", "some"}
    assert any(c["rows"] is not None for c in ks.CASES)
    # an all -1 row is named by a basket; bad list numbers, entries and indices each set the status word, the others do not
    idx, _, kn = tables["bad indices"]
    assert np.all(idx[20, :kn] == -1) and any(20 in b for c in ks.CASES if c["table"] == "bad indices" for b in c["baskets"])
    flagged = set()
    for c in ks.CASES:
        idx, val, kn = tables[c["table"]]
        scored, st = ks.accumulate(idx, val, kn, ks.csr(c["baskets"]), c["rows"], False)
        if st:
            flagged.add(c["name"])
        if c["name"] == "bad list numbers":
            assert [row is None for row in scored] == [False, True, False, True, True, False]
    assert flagged == {"bad list numbers", "bad entries and indices"}
    case = ks.CASES[ks.CASE_NAMES.index("bad entries and indices")]
    entries = [i for b in case["baskets"] for i in b]
    assert min(entries) < 0 and 65 in entries and max(entries) >= 2 ** 32
    idx, _, kn = tables["bad indices"]
    used = idx[[i for i in entries if 0 <= i < 65]][:, :kn]
    assert (used == 65).any() and (used < -1).any() and (used >= 2 ** 32).any()
    # special values among values and weights
    _, val, kn = tables["specials"]
    bits = set(ts.bits_of(val[:, :kn]).reshape(-1).tolist())
    assert {0x7FC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000} <= bits
    case = ks.CASES[ks.CASE_NAMES.index("special values")]
    weights = np.asarray([w for ws in case["weights"] for w in ws], dtype=np.float32)
    assert np.isnan(weights).any() and np.isposinf(weights).any() and np.isneginf(weights).any() and (ts.bits_of(weights) == 1).any()
    assert (ts.bits_of(weights) == 0x80000000).any()
    # ties: equal scores in every band of 64, and on both sides of each border, among the first places
    case = ks.CASES[ks.CASE_NAMES.index("ties across the bands")]
    idx, val, kn = tables["borders"]
    top, value, _, _ = ks.knn_reference(idx, val, kn, ks.csr(case["baskets"]), None, None, True, 1, 64)
    first = top[0][ts.bits_of(value[0]) == ts.bits_of(value[0, 0])]
    assert {int(j) // 64 for j in first} == {0, 1, 2, 3} and {63, 64} & set(first.tolist()) == {63, 64} - {0} \
        and {127, 128} <= set(first.tolist())
    case = ks.CASES[ks.CASE_NAMES.index("integer ties")]
    idx, val, kn = tables["integer 200"]
    _, value, _, _ = ks.knn_reference(idx, val, kn, ks.csr(case["baskets"]), None, None, True, 1, 64)
    assert len(set(ts.bits_of(value[-1]).tolist())) <= 12                               # 64 places, a handful of scores
    # every eligibility rule changes some answer
    case = ks.CASES[ks.CASE_NAMES.index("kn 7")]
    idx, val, kn = tables["kn 7"]
    lists = ks.csr(case["baskets"], case["weights"])
    base = ks.knn_reference(idx, val, kn, lists, None, None, False, 1, 5)[0]
    assert not np.array_equal(base, ks.knn_reference(idx, val, kn, lists, None, None, True, 1, 5)[0])
    assert not np.array_equal(base, ks.knn_reference(idx, val, kn, lists, None, ks.item_mask("some", 129), False, 1, 5)[0])
    assert not np.array_equal(base, ks.knn_reference(idx, val, kn, lists, None, None, False, 2, 5)[0])
    assert (base[:, -1] == -1).any() and (base[:, 0] >= 0).any()                        # k above the candidate count in some row
