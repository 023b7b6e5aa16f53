"""CPU-only checks of diversified re-ranking: the three entry points in the header (an addition to ABI 14), the ctypes table
and the library; their argument validation, which happens before any launch; the numpy references on hand-worked lists;
the route rule against the device tests' case table; the Python layer's own checks; and the handler's parser."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, rerank, serving
import rerank_support as rs
import topk_support as ts

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_DIM, E_WORKSPACE, E_RANGE, E_ALIGN = -1, -2, -3, -4, -5
NAMES = ("lgc_rerank_route", "lgc_rerank_mmr", "lgc_list_diversity")


def test_entry_points_are_declared_bound_and_exported_as_an_addition_to_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    assert "Diversified re-ranking (an addition to ABI 14: exports only)" in header
    assert int(re.search(r"#define LGC_RERANK_MAX_CAND (\d+)", header).group(1)) == _native.RERANK_MAX_CAND == rs.MAX_CAND == ts.K_MAX
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"ptr": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)), "int64_t": (ctypes.c_int64,), "int32_t": (ctypes.c_int32,),
             "float": (ctypes.c_float,)}
    for name in NAMES:
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert decl and hasattr(lib, name), name
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is ctypes.c_int
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == len(argtypes), name
        for arg, have in zip(args, argtypes):
            kind = "ptr" if "*" in arg else re.match(r"(?:const\s+)?(\w+)", arg).group(1)
            assert have in kinds[kind], (name, arg)
    for name in ("mmr_rerank", "list_diversity"):
        assert name in lg.__all__ and hasattr(lg, name)
    for name in ("recommend_diverse", "rerank_diverse", "list_diversity"):
        assert hasattr(lg.LightGCN, name)
    assert hasattr(serving.RecommendHandler, "parse_diversify") and hasattr(serving.RecommendHandler, "inference_diverse")
    makefile = open(os.path.join(ROOT, "gnn-ecommerce_amd", "csrc", "Makefile")).read()
    assert "lgconv_rerank" in re.search(r"^UNITS\s*:=((?:.*\\\n)*.*)$", makefile, flags=re.M).group(1).split()


# addresses of host words: valid, 16-byte aligned, never read or written by a call that returns before its launch
_words = (ctypes.c_int64 * 8)()
ONE = ctypes.addressof(_words) + (-ctypes.addressof(_words)) % 16


def mmr(**kw):
    a = dict(items=ONE, item_stride=64, n_items=300, dim=64, scale=ONE, cand=ONE, cand_stride=256, rel=ONE, rel_stride=256,
             n_rows=4, n_cand=100, k=20, lam=0.7, out_index=ONE, out_pos=ONE, out_value=ONE, status=ONE)
    assert set(kw) <= set(a)
    a.update(kw)
    return _native.load().lgc_rerank_mmr(a["items"], a["item_stride"], a["n_items"], a["dim"], a["scale"], a["cand"],
                                         a["cand_stride"], a["rel"], a["rel_stride"], a["n_rows"], a["n_cand"], a["k"], a["lam"],
                                         a["out_index"], a["out_pos"], a["out_value"], a["status"], None)


def diversity(**kw):
    a = dict(items=ONE, item_stride=64, n_items=300, dim=64, scale=ONE, lists=ONE, list_stride=256, n_rows=4, k=20,
             cutoffs=(5, 10, 20), out=ONE, out_stride=8, status=ONE)
    assert set(kw) <= set(a)
    a.update(kw)
    cuts = a["cutoffs"]
    cuts_c = None if cuts is None else (ctypes.c_int32 * max(len(cuts), 1))(*cuts)
    return _native.load().lgc_list_diversity(a["items"], a["item_stride"], a["n_items"], a["dim"], a["scale"], a["lists"],
                                             a["list_stride"], a["n_rows"], a["k"], cuts_c, 0 if cuts is None else len(cuts),
                                             a["out"], a["out_stride"], a["status"], None)


def test_rerank_mmr_argument_errors_come_before_any_launch():
    for bad in (dict(items=None), dict(cand=None), dict(rel=None), dict(out_index=None), dict(status=None), dict(n_rows=-1),
                dict(item_stride=63), dict(cand_stride=99), dict(rel_stride=99), dict(lam=float("nan"))):
        assert mmr(**bad) == E_INVAL, bad
    for dim in (0, -1, 257):
        assert mmr(dim=dim, item_stride=300) == E_DIM
    for bad in (dict(n_cand=0), dict(n_cand=-1), dict(n_cand=257), dict(k=0), dict(k=-1), dict(k=101), dict(lam=-0.001),
                dict(lam=1.001), dict(lam=float("inf")), dict(n_items=0), dict(n_items=-1), dict(n_items=2 ** 31),
                dict(n_rows=2 ** 31)):
        assert mmr(**bad) == E_RANGE, bad
    for name in ("items", "scale", "rel", "out_value", "out_pos"):
        assert mmr(**{name: ONE + 2}) == E_ALIGN, name
    for name in ("cand", "out_index"):
        assert mmr(**{name: ONE + 4}) == E_ALIGN, name
    # n_rows == 0: validated, nothing launched; the optional pointers may be NULL
    assert mmr(n_rows=0) == 0 and mmr(n_rows=0, scale=None, out_pos=None, out_value=None) == 0
    for ok in (dict(lam=0.0), dict(lam=1.0), dict(n_cand=1, k=1), dict(n_cand=256, k=256), dict(k=100), dict(n_items=1),
               dict(dim=1, item_stride=1), dict(dim=256, item_stride=259), dict(cand_stride=100, rel_stride=100)):
        assert mmr(n_rows=0, **ok) == 0, ok
    assert mmr(n_rows=0, item_stride=63) == E_INVAL and mmr(n_rows=0, k=101) == E_RANGE     # still validated


def test_list_diversity_argument_errors_come_before_any_launch():
    for bad in (dict(items=None), dict(lists=None), dict(cutoffs=None), dict(out=None), dict(status=None), dict(n_rows=-1),
                dict(item_stride=63), dict(list_stride=19), dict(out_stride=2), dict(cutoffs=())):
        assert diversity(**bad) == E_INVAL, bad
    for dim in (0, -1, 257):
        assert diversity(dim=dim, item_stride=300) == E_DIM
    for bad in (dict(k=0), dict(k=257, list_stride=300), dict(n_items=0), dict(n_items=2 ** 31), dict(n_rows=2 ** 31),
                dict(cutoffs=(0, 5)), dict(cutoffs=(5, 5)), dict(cutoffs=(10, 5)), dict(cutoffs=(5, 21)), dict(cutoffs=(-1,)),
                dict(cutoffs=tuple(range(1, 10)), out_stride=9)):
        assert diversity(**bad) == E_RANGE, bad
    for name in ("items", "scale"):
        assert diversity(**{name: ONE + 2}) == E_ALIGN, name
    for name in ("lists", "out"):
        assert diversity(**{name: ONE + 4}) == E_ALIGN, name
    assert diversity(n_rows=0) == 0 and diversity(n_rows=0, scale=None) == 0
    for ok in (dict(cutoffs=(1,)), dict(cutoffs=(20,)), dict(cutoffs=tuple(range(1, 9))), dict(k=256, cutoffs=(1, 2, 256)),
               dict(k=1, cutoffs=(1,)), dict(list_stride=20, out_stride=3)):
        assert diversity(n_rows=0, **ok) == 0, ok
    assert diversity(n_rows=0, cutoffs=(5, 21)) == E_RANGE                                  # still validated


def test_route_rule_and_the_device_case_table_reaches_every_route():
    lib = _native.load()
    seen = set()
    for n_cand, dim in rs.GPU_SHAPES:
        code = lib.lgc_rerank_route(n_cand, dim)
        assert _native.RERANK_ROUTES[code] == rs.route(n_cand, dim) == rerank.rerank_route(n_cand, dim), (n_cand, dim)
        seen.add(_native.RERANK_ROUTES[code])
    assert seen == {"lds", "global"}
    # the boundary itself: 36 KiB of rows 68 floats apart is 135 candidates of width 64
    assert rs.row_stride(64) == 68 and rs.row_stride(90) == 92 and rs.row_stride(1) == 4 and rs.row_stride(256) == 260
    assert rs.route(135, 64) == "lds" and rs.route(136, 64) == "global"
    assert lib.lgc_rerank_route(135, 64) == 1 and lib.lgc_rerank_route(136, 64) == 2
    assert lib.lgc_rerank_route(100, 90) == 1 and lib.lgc_rerank_route(101, 90) == 2       # the workload's shapes are staged
    assert lib.lgc_rerank_route(0, 64) == E_RANGE and lib.lgc_rerank_route(257, 64) == E_RANGE
    assert lib.lgc_rerank_route(10, 0) == E_DIM


# ---------------------------------------------------------------------------------------------------------------
# the references, on lists worked by hand
# ---------------------------------------------------------------------------------------------------------------
SIM4 = np.array([[9, 1.0, 0.25, 0.0], [1.0, 9, 0.25, 0.0], [0.25, 0.25, 9, 0.5], [0.0, 0.0, 0.5, 9]], dtype=np.float32)


def sim4(ps, c):
    return SIM4[ps, c]


def test_mmr_reference_on_a_worked_example():
    """rel = (1, 0.875, 0.75, 0.5), lam = 0.5; candidates 0 and 1 are near-duplicates (sim 1), 2 is a little like both
    (0.25) and half like 3, 3 is unlike 0 and 1.
      step 0: obj = (0.5, 0.4375, 0.375, 0.25)                              -> position 0
      step 1: pen = (-, 1, 0.25, 0); obj = (-, -0.0625, 0.25, 0.25)         -> a tie: position 2
      step 2: pen = (-, max(1, 0.25), -, max(0, 0.5)); obj = (-, -0.0625, -, 0)  -> position 3
      step 3: position 1 with -0.0625."""
    rel = np.array([1.0, 0.875, 0.75, 0.5], dtype=np.float32)
    cand = np.array([40, 41, 42, 43])
    index, pos, value = rs.mmr_ref(rel, cand, sim4, 4, 0.5)
    assert pos.tolist() == [0, 2, 3, 1] and index.tolist() == [40, 42, 43, 41]
    assert value.tolist() == [0.5, 0.25, 0.0, -0.0625]
    assert rs.mmr_ref(rel, cand, sim4, 2, 0.5)[1].tolist() == [0, 2]                    # a shorter k is a prefix


def test_mmr_reference_with_lam_1_is_the_plain_ranking_and_with_lam_0_minimises_the_running_maximum():
    rng = np.random.default_rng(1)
    rel = rng.integers(0, 6, size=40).astype(np.float32)
    rel[[3, 30]] = ts.from_bits([0x7FC00000, 0xFFC00000])
    rel[[5, 6]] = [np.inf, -np.inf]
    rel[7] = -0.0
    sim = rng.standard_normal((40, 40)).astype(np.float32)
    index, pos, value = rs.mmr_ref(rel, np.arange(40), lambda ps, c: sim[ps, c], 25, 1.0)
    want_i, want_v = ts.topk_ref(rel, 25)
    assert pos.tolist() == want_i.tolist() and rs.ss.same_values(value, want_v)
    # lam = 0: every objective of step 0 is 0 -> position 0; then the candidate least like anything chosen
    rel4 = np.array([0.0, 5.0, 9.0, 1.0], dtype=np.float32)
    _, pos, value = rs.mmr_ref(rel4, np.arange(4), sim4, 4, 0.0)
    assert pos.tolist() == [0, 3, 2, 1]        # pen after 0: (1, 0.25, 0) -> 3; then max(0.25, 0.5) = 0.5 against 1 -> 2
    assert rs.ss.same_values(value, np.array([0.0, 0.0, -0.5, -1.0], dtype=np.float32))


def test_mmr_reference_nan_first_ties_by_position_empty_places_and_duplicates():
    nan = ts.from_bits([0xFFC00000])[0]
    # a NaN objective is chosen first: from rel at step 0, from a similarity later; a NaN penalty sticks
    rel = np.array([3.0, nan, 2.0, 1.0], dtype=np.float32)
    sim = SIM4.copy()
    sim[3, 1] = sim[1, 3] = nan
    _, pos, value = rs.mmr_ref(rel, np.arange(4), lambda ps, c: sim[ps, c], 4, 0.5)
    assert pos.tolist() == [1, 3, 0, 2] and np.isnan(value[:2]).all()                   # 3's penalty is NaN after step 0
    # equal objectives fall to the lower position, step after step
    flat = np.ones((6, 6), dtype=np.float32)
    _, pos, _ = rs.mmr_ref(np.full(6, 2.0, dtype=np.float32), np.arange(6), lambda ps, c: flat[ps, c], 6, 0.3)
    assert pos.tolist() == [0, 1, 2, 3, 4, 5]
    # -1 places are skipped, ids out of range too when the table size is given; short rows end in -1 / -1 / -inf
    cand = np.array([-1, 41, 7000, 43, -1])
    rel5 = np.array([9.0, 1.0, 8.0, 2.0, 7.0], dtype=np.float32)
    s5 = np.zeros((5, 5), dtype=np.float32)
    index, pos, value = rs.mmr_ref(rel5, cand, lambda ps, c: s5[ps, c], 4, 0.5, n_items=100)
    assert index.tolist() == [43, 41, -1, -1] and pos.tolist() == [3, 1, -1, -1] and value.tolist() == [1.0, 0.5, -np.inf, -np.inf]
    assert rs.mmr_ref(rel5, cand, lambda ps, c: s5[ps, c], 3, 0.5)[0].tolist() == [7000, 43, 41]
    assert rs.mmr_ref(rel5[:1], cand[:1], None, 1, 0.5)[0].tolist() == [-1]
    # a repeated id is two candidates: with lam < 1 the twin pays the full penalty and goes last
    table = np.array([[2, 0], [0, 2], [1, 1]], dtype=np.float32)
    cand = np.array([0, 0, 1, 2])
    index, pos, _ = rs.mmr_ref(np.array([4, 4, 1, 3], dtype=np.float32), cand, rs.exact_sims(table, cand), 4, 0.5)
    assert pos.tolist() == [0, 2, 3, 1] and index.tolist() == [0, 1, 2, 0]              # step 1: 2 - 2, 0.5 - 0, 1.5 - 1 -> a tie: position 2


def test_ild_reference_on_worked_lists():
    ones, zeros = np.ones((5, 5), dtype=np.float32), np.zeros((5, 5), dtype=np.float32)
    all_valid = np.ones(5, dtype=bool)
    assert rs.ild_ref(ones, all_valid, (2, 3, 5)).tolist() == [0.0, 0.0, 0.0]           # all-equal items
    assert rs.ild_ref(zeros, all_valid, (2, 3, 5)).tolist() == [1.0, 1.0, 1.0]          # orthogonal ones
    got = rs.ild_ref(zeros, all_valid, (1, 2))
    assert np.isnan(got[0]) and got[1] == 1.0                                           # one item has no pair
    few = np.array([False, True, False, False, True])
    got = rs.ild_ref(zeros, few, (1, 2, 4, 5))
    assert np.isnan(got[:3]).all() and got[3] == 1.0
    # a prefix: the value at a cutoff does not depend on the later cutoffs or places
    sim = np.triu(np.arange(25, dtype=np.float32).reshape(5, 5) / 32, 1)
    full = rs.ild_ref(sim, all_valid, (2, 3, 4, 5))
    assert full[0] == 1 - 1 / 32 and full[1] == ((1 - 1 / 32) + (1 - 2 / 32) + (1 - 7 / 32)) / 3
    for j, c in enumerate((2, 3, 4, 5)):
        assert rs.ild_ref(sim, all_valid, (c,))[0] == full[j] == rs.ild_ref(sim[:c, :c], all_valid[:c], (c,))[0]
    valid = np.array([True, False, True, True, True])
    assert rs.ild_ref(sim, valid, (4,))[0] == ((1 - 2 / 32) + (1 - 3 / 32) + (1 - 13 / 32)) / 3
    assert rs.same_doubles(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0])) and not rs.same_doubles([1.0], [1.0 + 2 ** -52])


# ---------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------
def test_python_layer_validates_before_it_touches_a_device():
    items = torch.zeros(50, 8)
    cand = torch.zeros((2, 10), dtype=torch.int64)
    rel = torch.zeros((2, 10))
    for lam in (-0.1, 1.1, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="lam"):
            rerank.mmr_rerank(items, cand, rel, 3, lam)
    with pytest.raises(ValueError, match="metric"):
        rerank.mmr_rerank(items, cand, rel, 3, metric="l2")
    assert rerank.check_lam(np.float32(0.5)) == 0.5 and rerank.check_lam(np.float64(1.0)) == 1.0 and rerank.check_lam(0) == 0.0
    assert rerank.check_lam(torch.tensor(0.25)) == 0.25 and isinstance(rerank.check_lam(np.int64(1)), float)
    for lam in (np.bool_(True), np.float32(1.5), np.float32("nan"), torch.tensor(2.0), torch.tensor([0.5]), torch.tensor(1)):
        with pytest.raises(ValueError, match="lam"):
            rerank.check_lam(lam)
    for not_a_table in (None, [[0.0] * 8] * 50, np.zeros((50, 8), dtype=np.float32)):
        with pytest.raises(TypeError):
            rerank.mmr_rerank(not_a_table, cand, rel, 3)
        with pytest.raises(TypeError):
            rerank.list_diversity(not_a_table, cand, (5,))
    for k in (0, 11, True, 2.0):
        with pytest.raises(ValueError, match="k must be"):
            rerank.mmr_rerank(items, cand, rel, k)
    with pytest.raises(TypeError):
        rerank.mmr_rerank(items, cand.to(torch.int32), rel, 3)
    with pytest.raises(ValueError, match="256"):
        rerank.mmr_rerank(items, torch.zeros((2, 257), dtype=torch.int64), torch.zeros((2, 257)), 3)
    with pytest.raises(_native.NativeLibraryError):                                     # no CPU route
        rerank.mmr_rerank(items, cand, rel, 3)
    with pytest.raises(ValueError, match="metric"):
        rerank.list_diversity(items, cand, (5,), metric="l2")
    for cuts in ((), (0,), (5, 5), (11,), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            rerank.list_diversity(items, cand, cuts)
    with pytest.raises(_native.NativeLibraryError):
        rerank.list_diversity(items, cand, (5, 10))
    model = lg.LightGCN(10, 8, 0)
    for bad in (dict(k=0), dict(k=5, candidates=4), dict(candidates=257), dict(candidates=True), dict(lam=2.0)):
        with pytest.raises(ValueError):
            model.recommend_diverse(None, None, 4, 6, None, [1], **bad)
    with pytest.raises(ValueError, match="nodes"):
        model.rerank_diverse(None, None, 4, 7, cand, rel, 3)
    with pytest.raises(ValueError, match="nodes"):
        model.list_diversity(None, None, 4, 7, cand)
    with pytest.raises(_native.NativeLibraryError):
        model.rerank_diverse(None, None, 4, 6, cand, rel, 3)


# ---------------------------------------------------------------------------------------------------------------
# the handler's parser, with a stub model
# ---------------------------------------------------------------------------------------------------------------
class StubModel:
    def __init__(self):
        self.calls = []

    def recommendK(self, graph, ew, n_users, n_items, seen, users, k):
        import pandas as pd
        return pd.DataFrame({"user_ID": list(users), "top_rlvnt_itm": [[u + j for j in range(k)] for u in users]})

    def recommend_diverse(self, graph, ew, n_users, n_items, seen, users, k, candidates, lam, metric):
        self.calls.append(("ids", list(users), k, candidates, lam, metric))
        return torch.tensor([[u + 2 * j for j in range(k)] for u in users], dtype=torch.int64)


def stub_handler():
    h = serving.RecommendHandler()
    h.device, h.n_users, h.n_items, h.k = torch.device("cpu"), 10, 30, 2
    h.graph = h.seen = None
    h.model = StubModel()
    return h


def test_parse_diversify_takes_good_bodies():
    h = stub_handler()
    assert h.parse_diversify({"requests": [3, 0], "diversify": 0.5}) == ([3, 0], 0.5, 10, "cosine")   # min(5 k, 256, n_items)
    assert h.parse_diversify({"requests": [], "diversify": 1, "candidates": 256, "metric": "dot"}) == ([], 1.0, 256, "dot")
    assert h.parse_diversify({"requests": ({"items": [1]}, 2), "diversify": 0, "candidates": 2}) == ([{"items": [1]}, 2], 0.0, 2, "cosine")
    h.k, h.n_items = 20, 10 ** 6
    assert h.parse_diversify({"requests": [1], "diversify": 0.7})[2] == 100
    h.k = 60
    assert h.parse_diversify({"requests": [1], "diversify": 0.7})[2] == 256
    out = stub_handler().handle([{"body": {"requests": [4, 7], "diversify": 0.25, "candidates": 5}}])[0]
    assert out == {"items": [[4, 6], [7, 9]]}


@pytest.mark.parametrize("body", [
    {"requests": [1], "diversify": True}, {"requests": [1], "diversify": "0.5"}, {"requests": [1], "diversify": None},
    {"requests": [1], "diversify": -0.1}, {"requests": [1], "diversify": 1.5}, {"requests": [1], "diversify": float("nan")},
    {"requests": [1], "diversify": [0.5]}, {"requests": 1, "diversify": 0.5}, {"diversify": 0.5},
    {"requests": [1], "diversify": 0.5, "candidates": 1}, {"requests": [1], "diversify": 0.5, "candidates": 257},
    {"requests": [1], "diversify": 0.5, "candidates": True}, {"requests": [1], "diversify": 0.5, "candidates": 20.0},
    {"requests": [1], "diversify": 0.5, "candidates": None}, {"requests": [1], "diversify": 0.5, "metric": "l2"},
    {"requests": [1], "diversify": 0.5, "metric": None}, {"requests": [1], "diversify": 0.5, "k": 5},
    {"requests": [1], "diversify": 0.5, "explain": 2}, {"requests": [1.0], "diversify": 0.5}, {"requests": [True], "diversify": 0.5},
    {"requests": ["1"], "diversify": 0.5}, {"requests": [{"item": [1]}], "diversify": 0.5},
    {"requests": [{"items": [30]}], "diversify": 0.5}])
def test_parse_diversify_refuses_malformed_bodies(body):
    h = stub_handler()
    with pytest.raises(ValueError):
        h.inference(body)
    assert h.model.calls == []


def test_parse_diversify_refuses_users_outside_the_table_and_other_bodies_are_as_before():
    for bad in ([10], [-1], [0, 11]):
        with pytest.raises(IndexError):
            stub_handler().inference({"requests": bad, "diversify": 0.5})
    h = stub_handler()
    with pytest.raises(ValueError):
        h.parse_diversify({"requests": [1], "explain": 2})                              # not this parser's body
    assert h.handle([{"body": [2, 5]}]) == [{"items": [[2, 3], [5, 6]]}] and h.model.calls == []
    with pytest.raises(ValueError, match="'requests' and 'explain'"):
        h.inference({"requests": [1]})                                                  # the explain parser still answers
    with pytest.raises(ValueError, match="similar"):
        h.inference({"similar": [1], "diversify": 0.5})                                 # "similar" is dispatched first
    assert h.handle([{"body": {"requests": [], "diversify": 0.5}}]) == [{"items": []}] and h.model.calls == []
