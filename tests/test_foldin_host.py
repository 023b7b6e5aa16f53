"""CPU-only checks of fold-in: lgc_fold_in in the header, the ctypes table and the library at ABI 14; its argument
validation, which happens before any launch; the identity it rests on -- the formula (fp64, and the fp32 emulation of the
kernel's specified order) against the CPU oracle's get_embedding on the graph augmented with one-way edges --;
SessionLists; and the handler's request parsing with a stub model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_fro
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, serving
from gnn_ecommerce_amd.foldin import SessionLists
from gnn_ecommerce_amd.propagate import SeenLists
from oracle import lightgcn_oracle as oracle
import foldin_support as fs

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_DIM, E_RANGE = -1, -2, -4


def test_fold_in_is_declared_bound_and_exported_at_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint lgc_fold_in\s*\(([^;]*)\)\s*;", code)
    assert decl and "lgc_fold_in" in _native.SIGNATURES and hasattr(lib, "lgc_fold_in")
    restype, argtypes = _native.SIGNATURES["lgc_fold_in"]
    assert restype is ctypes.c_int and len(argtypes) == len(decl.group(1).split(",")) == 19
    assert argtypes[-1] is ctypes.c_void_p and argtypes[12] is ctypes.c_float
    for ref in ("torchserve/lightgcn_handler.py:73-96", "src/lightgcn.py:91-99"):      # the lines it stands in for
        assert ref in header
    for name in ("SessionLists", "fold_table", "fold_in"):
        assert name in lg.__all__ and hasattr(lg, name)
    assert hasattr(lg.LightGCN, "embed_sessions") and hasattr(lg.LightGCN, "recommend_sessions")


def test_fold_in_argument_errors_come_before_any_launch():
    lib = _native.load()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below must end in validation

    def fold(**kw):
        a = dict(ptr=one, items=one, w=one, n=4, dis=one, fold=one, fs=64, ni=300, rows=one, init=one, istride=64, nir=10,
                 a0=0.25, norm=1, dim=64, out=one, os=64, status=one)
        a.update(kw)
        return lib.lgc_fold_in(a["ptr"], a["items"], a["w"], a["n"], a["dis"], a["fold"], a["fs"], a["ni"], a["rows"],
                               a["init"], a["istride"], a["nir"], a["a0"], a["norm"], a["dim"], a["out"], a["os"],
                               a["status"], None)
    for bad in (dict(ptr=None), dict(items=None), dict(fold=None), dict(out=None), dict(status=None), dict(n=-1),
                dict(ni=-1), dict(ni=0), dict(nir=-1), dict(fs=63), dict(os=63), dict(istride=63), dict(norm=2),
                dict(norm=-1), dict(dis=None), dict(init=None)):
        assert fold(**bad) == E_INVAL, bad
    for dim in (0, -1, 257):
        assert fold(dim=dim, fs=300, os=300, istride=300) == E_DIM
    assert fold(n=2 ** 31 - 1) == E_RANGE and fold(n=2 ** 31) == E_RANGE and fold(ni=2 ** 31) == E_RANGE
    # what is optional: weights, the init rows (then init is not looked at), item_dis without normalisation
    assert fold(n=0) == 0 and fold(n=0, w=None, rows=None, init=None, istride=0, nir=0) == 0
    assert fold(n=0, norm=0, dis=None) == 0 and fold(n=0, dim=1, fs=1, os=1, istride=1) == 0
    assert fold(n=0, dim=256, fs=256, os=259, istride=256) == 0
    assert fold(n=0, fs=63) == E_INVAL and fold(n=0, norm=1, dis=None) == E_INVAL      # still validated


def test_python_layer_refuses_host_tensors_and_bad_shapes():
    s = SessionLists.from_lists([([1, 2], None)])
    with pytest.raises(_native.NativeLibraryError):                                     # no CPU route
        lg.fold_in(torch.zeros(5, 8), torch.ones(5), s)
    with pytest.raises(ValueError, match="nothing to fold"):
        lg.fold_table(lg.LightGCN(10, 8, 0), None)


# ---------------------------------------------------------------------------------------------------------------
# the identity, on the CPU oracle
# ---------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 7, 32, 33, 65, 200)


@pytest.mark.parametrize("dim,layers", [(7, 1), (64, 2), (90, 3), (130, 5), (64, 5), (90, 1)])
def test_formula_is_get_embedding_on_the_one_way_augmented_graph(dim, layers):
    n_users, n_items = 40, 23
    rng = np.random.default_rng(dim * 10 + layers)
    ei, ew = fs.small_graph(n_users, n_items, 300, seed=dim + layers)
    n = n_users + n_items
    weight = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32) * 0.1)
    alpha = torch.from_numpy(rng.uniform(0.1, 0.5, layers + 1).astype(np.float32))
    lists = [rng.integers(n_items, size=m).tolist() for m in LENGTHS] * 2               # repeats inside a list happen
    weights = [np.array([0.01, 0.1, 1.0], dtype=np.float32)[rng.integers(3, size=len(x))] for x in lists]
    init_rows = [-1] * len(LENGTHS) + rng.integers(n_users, size=len(LENGTHS)).tolist()  # without and with an init row
    base = oracle.get_embedding(weight, alpha, ei, ew, layers)
    w2, ei2, ew2 = fs.augmented(weight, ei, ew, n_users, lists, weights, init_rows)
    full = oracle.get_embedding(w2, alpha, ei2, ew2, layers)
    assert torch.equal(full[:n], base)                                                  # old rows: bit-identical
    fold, dis = fs.oracle_fold_table(weight, alpha, ei, ew, layers, n_users)
    ptr, items = fs.csr(lists)
    wcat = np.concatenate(weights).astype(np.float32)
    args = (ptr, items, wcat, dis.numpy(), fold.numpy(), np.array(init_rows), weight[:n_users].numpy(), float(alpha[0]), True)
    y64, _ = fs.reference64(*args)
    y32 = fs.emulate32(*args)
    new = full[n:]
    for r, m in enumerate(LENGTHS):
        if m == 0:                                                                      # an empty list: a0 * z or zeros, exactly
            assert torch.equal(new[r], torch.zeros(dim)) and not y32[r].any() and not y64[r].any()
    err64, err32 = rel_fro(torch.from_numpy(y64), new), rel_fro(torch.from_numpy(y32), new)
    print(f"D={dim} K={layers}: fp64 formula vs oracle {err64:.2e}, fp32 emulation vs oracle {err32:.2e}")
    assert err64 <= 1e-5 and err32 <= 1e-5
    for r in range(len(lists)):                                                         # and no single row hides in the norm
        if np.abs(new[r].numpy()).max() > 0:
            assert rel_fro(torch.from_numpy(y32[r:r + 1]), new[r:r + 1]) <= 1e-5, (r, len(lists[r]))
    assert (np.abs(y32 - y64) <= fs.bound(ptr, items, n_items, fs.reference64(*args)[1])).all()   # the derived element bound


def test_emulation_skips_out_of_range_items_and_zero_total_weight():
    rng = np.random.default_rng(0)
    fold = rng.standard_normal((6, 5)).astype(np.float32)
    dis = rng.uniform(0.1, 1.0, 6).astype(np.float32)
    init = rng.standard_normal((3, 5)).astype(np.float32)
    ptr, items = fs.csr([[1, 9, 2, -4], [1, 2], [3, 4], []])
    w = np.array([1.0, 0.5, 0.1, 0.5, 1.0, 0.1, 0.0, 0.0], dtype=np.float32)
    rows = np.array([-1, -1, 2, 1])
    y = fs.emulate32(ptr, items, w, dis, fold, rows, init, 0.5, True)
    assert np.array_equal(y[0], y[1])                                                   # the two bad entries: left out of deg too
    assert np.array_equal(y[2], np.float32(0.5) * init[2]) and np.array_equal(y[3], np.float32(0.5) * init[1])
    y64, s = fs.reference64(ptr, items, w, dis, fold, rows, init, 0.5, True)
    assert np.abs(y - y64).max() <= 1e-6 and (np.abs(y - y64) <= fs.bound(ptr, items, 6, s)).all()
    raw = fs.emulate32(ptr, items, w, dis, fold, None, None, 0.0, False)                # normalize = 0: c = w
    assert np.allclose(raw[1], 1.0 * fold[1] + 0.1 * fold[2], rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------
# SessionLists
# ---------------------------------------------------------------------------------------------------------------
def test_session_lists_from_lists_validate_and_mask():
    s = SessionLists.from_lists([([3, 1, 3], [1.0, 0.1, 1.0]), ([], None), ([5], None), ([2, 4], (0.01, 1))])
    assert s.ptr.tolist() == [0, 3, 3, 4, 6] and s.items.tolist() == [3, 1, 3, 5, 2, 4] and s.n_rows == 4
    assert s.ptr.dtype == s.items.dtype == torch.int64 and s.weights.dtype == torch.float32
    assert s.weights.tolist() == [1.0, np.float32(0.1), 1.0, 1.0, np.float32(0.01), 1.0]   # a row without weights: ones
    assert s.validate(6) is s
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        s.validate(5)
    bought = s.mask("purchased")
    assert isinstance(bought, SeenLists) and bought.ptr.tolist() == [0, 2, 2, 3, 4] and bought.items.tolist() == [3, 3, 5, 4]
    assert s.mask() .ptr.tolist() == bought.ptr.tolist()                                # the default rule
    every = s.mask("all")
    assert every.ptr is s.ptr and every.items is s.items and s.mask(None) is None
    with pytest.raises(ValueError):
        s.mask("viewed")
    plain = SessionLists.from_lists([([1, 2], None), ([0], None)])
    assert plain.weights is None and plain.mask("purchased").items.tolist() == [1, 2, 0]
    assert SessionLists.from_lists([]).validate(3).n_rows == 0
    nothing = SessionLists.from_lists([([], None), ([], [])])                           # nothing listed: nothing to mask
    assert nothing.mask("purchased") is None and nothing.mask("all") is None
    assert SessionLists.from_lists([([1, 2], [0.1, 0.01])]).mask("purchased") is None and plain.mask("all") is not None
    for bad in ([([1, 2], [1.0])], [([1.5], None)], [([1], ["a"])], [5]):
        with pytest.raises(ValueError):
            SessionLists.from_lists(bad)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    direct = SessionLists(i64(0, 3, 3, 5), i64(3, 1, 3, 2, 4), torch.tensor([1.0, 0.1, 1.0, 0.01, 1.0]))   # no host copy kept
    assert direct.mask("purchased").ptr.tolist() == [0, 2, 2, 3] and direct.mask("purchased").items.tolist() == [3, 3, 4]
    assert SessionLists(i64(0, 1), i64(3), torch.tensor([0.5])).mask("purchased") is None
    for ptr, items, w in ((i64(0, 3), i64(1, 2), None), (i64(1, 2), i64(1, 2), None), (i64(0, 2, 1, 2), i64(1, 2), None),
                          (i64(0, 2), i64(1, -1), None), (i64(0, 2), i64(1, 7), None),
                          (i64(0, 2), i64(1, 2), torch.tensor([1.0, float("nan")])),
                          (i64(0, 2), i64(1, 2), torch.tensor([1.0, float("inf")])),
                          (i64(0, 2), i64(1, 2), torch.tensor([1.0, 2.0], dtype=torch.float64)),
                          (i64(0, 2), i64(1, 2), torch.tensor([1.0])), (i64(0, 2).int(), i64(1, 2), None),
                          (i64(), i64(), None)):
        with pytest.raises(ValueError):
            SessionLists(ptr, items, w).validate(7)
    assert SessionLists(i64(0, 2), i64(1, 6), torch.tensor([1.0, -0.5])).validate(7).n_rows == 1   # a negative weight is a number


# ---------------------------------------------------------------------------------------------------------------
# the handler's request parsing, with a stub model
# ---------------------------------------------------------------------------------------------------------------
class StubModel:
    def __init__(self):
        self.calls = []

    def recommendK(self, graph, ew, n_users, n_items, seen, users, k):
        import pandas as pd
        self.calls.append(("ids", list(users), k))
        return pd.DataFrame({"user_ID": list(users), "top_rlvnt_itm": [[u] * k for u in users]})

    def recommend_sessions(self, graph, ew, n_users, n_items, sessions, init_users, k):
        self.calls.append(("sessions", sessions, init_users, k))
        return torch.stack([torch.full((k,), 100 + r, dtype=torch.int64) for r in range(sessions.n_rows)])


def stub_handler():
    h = serving.RecommendHandler()
    h.device, h.n_users, h.n_items, h.k = torch.device("cpu"), 10, 30, 3
    h.graph = h.seen = None
    h.model = StubModel()
    return h


def test_handler_routes_ids_and_sessions_and_keeps_request_order():
    h = stub_handler()
    out = h.handle([{"body": [4, {"items": [1, 2], "weights": [1.0, 0.1]}, 7, {"items": [], "user": 9}, {"items": (5,)}]}])
    assert out == [{"items": [[4] * 3, [100] * 3, [7] * 3, [101] * 3, [102] * 3]}]
    (kind, sessions, init_users, k), ids_call = h.model.calls
    assert kind == "sessions" and k == 3 and init_users == [-1, 9, -1] and ids_call == ("ids", [4, 7], 3)
    assert sessions.ptr.tolist() == [0, 2, 2, 3] and sessions.items.tolist() == [1, 2, 5]
    assert sessions.weights.tolist() == [1.0, np.float32(0.1), 1.0]
    h = stub_handler()
    assert h.handle([{"body": [{"items": [3]}]}]) == [{"items": [[100] * 3]}]
    assert [c[0] for c in h.model.calls] == ["sessions"] and h.model.calls[0][2] is None   # nobody to start from
    h = stub_handler()
    assert h.handle([{"body": [2, 5]}]) == [{"items": [[2] * 3, [5] * 3]}]                # ids alone: today's path
    assert h.model.calls == [("ids", [2, 5], 3)]


@pytest.mark.parametrize("element", [
    "7", 2.5, None, True, [1, 2], {"weights": [1.0]}, {"items": 5}, {"items": [1.5]}, {"items": [True]}, {"items": ["1"]},
    {"items": [30]}, {"items": [-1]}, {"items": [1, 2], "weights": [1.0]}, {"items": [1], "weights": [1.0, 1.0]},
    {"items": [1], "weights": ["x"]}, {"items": [1], "weights": 1.0}, {"items": [1], "user": 10}, {"items": [1], "user": -1},
    {"items": [1], "user": "3"}, {"items": [1], "extra": 1}])
def test_handler_refuses_malformed_session_requests(element):
    h = stub_handler()
    with pytest.raises(ValueError):
        h.inference([3, {"items": [1]}, element])
    assert h.model.calls == []                                                            # nothing ran
    with pytest.raises(IndexError):
        stub_handler().inference([10, {"items": [1]}])                                    # a plain id out of range: as today
