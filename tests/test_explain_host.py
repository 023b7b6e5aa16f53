"""CPU-only checks of score attribution: lgc_attribute in the header (an addition to ABI 14), the ctypes table and the
library; its argument validation, which happens before any launch; explain.attribute's own; the identity it rests on --
score(u, t) = base + sum of contributions, fp64, against the CPU oracle's fp32 scores, for trained users through their
own CSR rows and for sessions through the one-way augmented graph --; the top-m reference on hand-worked lists; and the
handler's new body with a stub model."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_fro
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, explain, serving
from gnn_ecommerce_amd.foldin import SessionLists
from oracle import lightgcn_oracle as oracle
import explain_support as es
import foldin_support as fs
import topk_support as ts

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_DIM, E_RANGE, E_ALIGN = -1, -2, -4, -5


def test_attribute_is_declared_bound_and_exported_as_an_addition_to_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    block = header[header.index("Score attribution"):]
    assert block.startswith("Score attribution (an addition to ABI 14: exports only)")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint lgc_attribute\s*\(const lgc_attr_args \*args, void \*stream\)\s*;", code)
    assert "lgc_attribute" in _native.SIGNATURES and hasattr(lib, "lgc_attribute")
    restype, argtypes = _native.SIGNATURES["lgc_attribute"]
    assert restype is ctypes.c_int and len(argtypes) == 2 and argtypes[1] is ctypes.c_void_p
    assert int(re.search(r"#define LGC_ATTR_MAX_TARGETS (\d+)", header).group(1)) == _native.ATTR_MAX_TARGETS == 64
    assert int(re.search(r"#define LGC_ATTR_MAX_TOP (\d+)", header).group(1)) == _native.ATTR_MAX_TOP == 8
    # the struct: the same fields in the same order, pointers as pointers and sizes as the header's integer types
    body = re.search(r"typedef struct lgc_attr_args \{(.*?)\} lgc_attr_args;", code, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        got = re.match(r"\s*(?:const\s+)?(\w+)\s+(.*)", decl, flags=re.S)
        if got:
            for name in got.group(2).split(","):
                name = name.strip()
                fields.append((name.lstrip("* "), "ptr" if name.startswith("*") else got.group(1)))
    want = {"ptr": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, want[k]) for n, k in fields] == list(_native.AttrArgsC._fields_)
    for ref in ("src/inference_lightgcn.py:85-119",):
        assert ref in block
    for name in ("Attribution", "attribute"):
        assert name in lg.__all__ and hasattr(lg, name)
    assert hasattr(lg.LightGCN, "explain_topk") and hasattr(lg.LightGCN, "explain_sessions")
    assert hasattr(serving.RecommendHandler, "inference_explained")


# addresses of host words: valid, 16-byte aligned, never read or written by a call that returns before its launch
_words = (ctypes.c_int64 * 8)()
ONE = ctypes.addressof(_words) + (-ctypes.addressof(_words)) % 16


def attr_args(form="session", **kw):
    a = _native.AttrArgsC()
    if form in ("session", "both"):
        a.list_ptr, a.list_items, a.list_weight, a.item_dis, a.normalize = ONE, ONE, ONE, ONE, 1
    if form in ("graph", "both"):
        a.rowptr, a.entries, a.row_ids, a.n_graph_rows, a.col_base = ONE, ONE, ONE, 10, 10
    a.n_rows, a.fold, a.items, a.fold_stride, a.item_stride, a.n_items = 4, ONE, ONE, 64, 64, 300
    a.init_rows, a.init, a.init_stride, a.n_init_rows, a.a0 = ONE, ONE, 64, 10, 0.25
    a.targets, a.target_stride, a.n_targets, a.top_m, a.dim = ONE, 20, 20, 3, 64
    a.contrib_ptr, a.contrib, a.base, a.total = ONE, ONE, ONE, ONE
    a.top_pos, a.top_item, a.top_value, a.status = ONE, ONE, ONE, ONE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def run(form="session", **kw):
    return _native.load().lgc_attribute(ctypes.byref(attr_args(form, **kw)), None)


def test_attribute_argument_errors_come_before_any_launch():
    assert _native.load().lgc_attribute(None, None) == E_INVAL
    for form in ("session", "graph"):
        for bad in (dict(fold=None), dict(items=None), dict(targets=None), dict(status=None), dict(n_rows=-1), dict(n_items=-1),
                    dict(n_items=0), dict(n_init_rows=-1), dict(fold_stride=63), dict(item_stride=63), dict(init_stride=63),
                    dict(target_stride=19), dict(init=None), dict(contrib_ptr=None),
                    dict(top_pos=None), dict(top_item=None), dict(top_value=None),
                    dict(contrib=None, base=None, total=None, top_m=0)):
            assert run(form, **bad) == E_INVAL, (form, bad)
        for dim in (0, -1, 257):
            assert run(form, dim=dim, fold_stride=300, item_stride=300, init_stride=300) == E_DIM
        for bad in (dict(n_targets=0), dict(n_targets=65, target_stride=65), dict(n_targets=-1), dict(top_m=9), dict(top_m=-1),
                    dict(n_rows=2 ** 31 - 1), dict(n_rows=2 ** 31), dict(n_items=2 ** 31 - 1), dict(n_items=2 ** 31)):
            assert run(form, **bad) == E_RANGE, (form, bad)
        for table in ("fold", "items", "init", "contrib", "base", "total", "top_value"):
            assert run(form, **{table: ONE + 2}) == E_ALIGN, (form, table)
        # n_rows == 0: validated, nothing launched
        assert run(form, n_rows=0) == 0
        assert run(form, n_rows=0, init_rows=None, init=None, init_stride=0, n_init_rows=0) == 0
        assert run(form, n_rows=0, contrib=None, contrib_ptr=None) == 0 and run(form, n_rows=0, top_m=0, top_pos=None) == 0
        assert run(form, n_rows=0, contrib=None, base=None, total=None) == 0              # the top-m alone is an output
        assert run(form, n_rows=0, n_targets=64, target_stride=64, top_m=8) == 0
        assert run(form, n_rows=0, dim=1, fold_stride=1, item_stride=1, init_stride=1) == 0
        assert run(form, n_rows=0, dim=256, fold_stride=256, item_stride=259, init_stride=256) == 0
        assert run(form, n_rows=0, fold_stride=63) == E_INVAL                               # still validated
    # the lists: exactly one form
    assert run("both") == E_INVAL and run("none") == E_INVAL and run("both", n_rows=0) == E_INVAL
    for bad in (dict(list_ptr=None), dict(list_items=None), dict(normalize=2), dict(normalize=-1), dict(item_dis=None)):
        assert run("session", **bad) == E_INVAL, bad
    assert run("session", n_rows=0, normalize=0, item_dis=None) == 0 and run("session", n_rows=0, list_weight=None) == 0
    for bad in (dict(rowptr=None), dict(entries=None), dict(row_ids=None), dict(n_graph_rows=-1)):
        assert run("graph", **bad) == E_INVAL, bad
    assert run("graph", n_graph_rows=2 ** 31) == E_RANGE
    assert run("graph", n_rows=0, n_graph_rows=0, col_base=0) == 0


def test_python_layer_validates_before_it_touches_a_device():
    s = SessionLists.from_lists([([1, 2], None)])
    fold, items, targets = torch.zeros(5, 8), torch.zeros(5, 8), torch.zeros((1, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="exactly one form"):
        explain.attribute(fold, items, targets)
    with pytest.raises(ValueError, match="exactly one form"):
        explain.attribute(fold, items, targets, sessions=s, row_ids=torch.zeros(1, dtype=torch.int64))
    for m in (-1, 9, True, 2.0):
        with pytest.raises(ValueError, match="m must be"):
            explain.attribute(fold, items, targets, sessions=s, m=m)
    with pytest.raises(_native.NativeLibraryError):                                     # no CPU route
        explain.attribute(fold, items, targets, sessions=s, item_dis=torch.ones(5))
    model = lg.LightGCN(10, 8, 0)
    with pytest.raises(_native.NativeLibraryError):
        model.explain_topk(None, None, 4, 6, [1], [[0, 1]])


# ---------------------------------------------------------------------------------------------------------------
# the identity, on the CPU oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_users,n_items,dim,layers", [(300, 37, 64, 3), (200, 50, 90, 5), (500, 120, 7, 2), (60, 500, 130, 1)])
def test_contributions_and_base_sum_to_the_oracles_score(n_users, n_items, dim, layers):
    rng = np.random.default_rng(dim * 10 + layers)
    ei, ew = fs.small_graph(n_users, n_items, 4 * n_users, seed=dim + layers)
    n = n_users + n_items
    weight = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32) * 0.1)
    alpha = torch.from_numpy(rng.uniform(0.1, 0.5, layers + 1).astype(np.float32))
    emb = oracle.get_embedding(weight, alpha, ei, ew, layers)
    fold, item_dis = fs.oracle_fold_table(weight, alpha, ei, ew, layers, n_users)
    table = emb[n_users:].contiguous()
    k = min(20, n_items)
    # trained users: their own rows of the forward CSR -- entries in edge order, val = (dis_item * w) * dis_user
    val = oracle.gcn_norm(ei, ew, n).numpy()
    src, dst = ei[0].numpy(), ei[1].numpy()
    users = np.arange(n_users)
    lists = [np.flatnonzero(dst == u) for u in users]                                   # edge ids, ascending = edge order
    ptr, edges = fs.csr(lists)
    items = src[edges] - n_users
    assert items.min() >= 0
    scores = emb[:n_users] @ table.t()                                                  # the oracle's fp32 scores
    targets = scores.topk(k, dim=-1).indices.numpy()
    ok = np.ones(len(items), dtype=bool)
    contrib, base, total, s = es.reference64(ptr, items, val[edges], ok, fold.numpy(), table.numpy(), targets, users,
                                             weight[:n_users].numpy(), float(alpha[0]))
    want = torch.gather(scores, 1, torch.from_numpy(targets))
    err_users = rel_fro(torch.from_numpy(total), want)
    assert np.allclose(contrib.reshape(-1, k)[:ptr[1]].sum(axis=0) + base[0], total[0], rtol=1e-12, atol=1e-15)
    # sessions: nodes appended with one-way edges, with and without an init row
    lengths = (0, 1, 2, 7, 33, 65)
    s_lists = [rng.integers(n_items, size=m_).tolist() for m_ in lengths] * 2
    s_w = [np.array([0.01, 0.1, 1.0], dtype=np.float32)[rng.integers(3, size=len(x))] for x in s_lists]
    init_rows = [-1] * len(lengths) + rng.integers(n_users, size=len(lengths)).tolist()
    w2, ei2, ew2 = fs.augmented(weight, ei, ew, n_users, s_lists, s_w, init_rows)
    new = oracle.get_embedding(w2, alpha, ei2, ew2, layers)[n:]
    s_scores = new @ table.t()
    s_targets = s_scores.topk(k, dim=-1).indices.numpy()
    s_ptr, s_items = fs.csr(s_lists)
    c64, s_ok = es.session_coeffs64(s_ptr, s_items, np.concatenate(s_w), item_dis.numpy(), n_items, True)
    _, _, s_total, _ = es.reference64(s_ptr, s_items, c64, s_ok, fold.numpy(), table.numpy(), s_targets, np.array(init_rows),
                                      weight[:n_users].numpy(), float(alpha[0]))
    err_sessions = rel_fro(torch.from_numpy(s_total), torch.gather(s_scores, 1, torch.from_numpy(s_targets)))
    c32, _ = es.session_coeffs32(s_ptr, s_items, np.concatenate(s_w), item_dis.numpy(), n_items, True)
    assert np.abs(c32 - c64).max() <= 40 * es.U * np.abs(c64).max()                      # (0.5 n + 4) u, n <= 65
    print(f"{n_users}x{n_items} D={dim} K={layers}: users {err_users:.2e}, sessions {err_sessions:.2e}")
    assert err_users <= 1e-5 and err_sessions <= 1e-5


# ---------------------------------------------------------------------------------------------------------------
# the top-m reference, on lists worked by hand
# ---------------------------------------------------------------------------------------------------------------
def test_top_m_reference_on_hand_worked_lists():
    nz = ts.from_bits([0x80000000])[0]
    nan = ts.from_bits([0xFFC00000])[0]
    every = lambda n: np.ones(n, dtype=bool)
    # ties at the cut: the earlier positions win
    pos, item, val = es.top_ref([0.5, 0.7, 0.5, 0.5, 0.1], every(5), [9, 8, 7, 6, 5], 3)
    assert pos.tolist() == [1, 0, 2] and item.tolist() == [8, 9, 7] and val.tolist() == [np.float32(0.7), 0.5, 0.5]
    # -0 and +0 are equal: position decides; both rank above a negative value
    pos, _, val = es.top_ref([-1.0, nz, 0.0, nz], every(4), [1, 2, 3, 4], 4)
    assert pos.tolist() == [1, 2, 3, 0] and ts.bits_of(val).tolist() == [0x80000000, 0, 0x80000000, 0xBF800000]
    # a NaN ranks first, then +inf; -inf last
    pos, _, val = es.top_ref([1.0, np.inf, nan, -np.inf, 2.0], every(5), [0, 1, 2, 3, 4], 5)
    assert pos.tolist() == [2, 1, 4, 0, 3] and np.isnan(val[0])
    # fewer than m entries: -1 / -1 / +0 in the unused places
    pos, item, val = es.top_ref([0.25, 0.5], every(2), [3, 3], 4)                         # a repeated item stays two entries
    assert pos.tolist() == [1, 0, -1, -1] and item.tolist() == [3, 3, -1, -1] and ts.bits_of(val).tolist()[2:] == [0, 0]
    pos, item, val = es.top_ref([], every(0), [], 2)
    assert pos.tolist() == [-1, -1] and item.tolist() == [-1, -1] and not val.any()
    # skipped entries take no part, but positions count them
    keep = np.array([True, False, True, False, True])
    pos, item, _ = es.top_ref([0.1, 9.0, 0.3, nan, 0.2], keep, [5, 99, 6, -4, 7], 3)
    assert pos.tolist() == [2, 4, 0] and item.tolist() == [6, 7, 5]
    # and the sequential fp32 total leaves them out too
    rows = np.array([[1.0], [np.float32(1e8)], [2.0 ** -24], [np.nan], [1.0]], dtype=np.float32)
    assert es.sequential_total32(rows, keep, np.array([0.5], dtype=np.float32)).tolist() == [2.5]


# ---------------------------------------------------------------------------------------------------------------
# the handler's new body, with a stub model
# ---------------------------------------------------------------------------------------------------------------
class StubModel:
    def __init__(self):
        self.calls = []

    def recommendK(self, graph, ew, n_users, n_items, seen, users, k):
        import pandas as pd
        return pd.DataFrame({"user_ID": list(users), "top_rlvnt_itm": [[u + j for j in range(k)] for u in users]})

    def recommend_sessions(self, graph, ew, n_users, n_items, sessions, init_users, k):
        return torch.stack([torch.arange(k, dtype=torch.int64) + 20 + r for r in range(sessions.n_rows)])

    def _answer(self, top, m):
        rows, k = top.shape
        item = torch.full((rows, k, m), -1, dtype=torch.int64)
        item[:, :, 0] = top + 1                                                          # one contributor, two empty places
        value = torch.zeros((rows, k, m))
        value[:, :, 0] = 0.5
        return types.SimpleNamespace(base=torch.full((rows, k), 0.25), total=torch.full((rows, k), 0.75), top_item=item,
                                     top_value=value, top_pos=torch.zeros((rows, k, m), dtype=torch.int32))

    def explain_topk(self, graph, ew, n_users, n_items, users, top, m):
        self.calls.append(("ids", list(users), top.tolist(), m))
        return self._answer(top, m)

    def explain_sessions(self, graph, ew, n_users, n_items, sessions, top, init_users, m):
        self.calls.append(("sessions", sessions.items.tolist(), top.tolist(), init_users, m))
        return self._answer(top, m)


def stub_handler():
    h = serving.RecommendHandler()
    h.device, h.n_users, h.n_items, h.k = torch.device("cpu"), 10, 30, 2
    h.graph = h.seen = None
    h.model = StubModel()
    return h


def test_handler_explains_ids_and_sessions_in_request_order():
    h = stub_handler()
    requests = [4, {"items": [1, 2], "weights": [1.0, 0.1]}, 7, {"items": [], "user": 9}]
    out = h.handle([{"body": {"requests": requests, "explain": 3}}])[0]
    assert out["items"] == h.handle([{"body": requests}])[0]["items"] == [[4, 5], [20, 21], [7, 8], [21, 22]]
    assert len(out["because"]) == 4 and all(len(b) == 2 for b in out["because"])
    for row, b in zip(out["items"], out["because"]):
        for item, entry in zip(row, b):
            assert entry == {"base": 0.25, "score": 0.75, "items": [[item + 1, 0.5]]}   # the -1 places are dropped
    ids_call, s_call = h.model.calls
    assert ids_call == ("ids", [4, 7], [[4, 5], [7, 8]], 3)
    assert s_call == ("sessions", [1, 2], [[20, 21], [21, 22]], [-1, 9], 3)
    h = stub_handler()
    out = h.handle([{"body": {"requests": [2], "explain": 1}}])[0]
    assert out["items"] == [[2, 3]] and [c[0] for c in h.model.calls] == ["ids"]
    assert stub_handler().handle([{"body": {"requests": [], "explain": 2}}]) == [{"items": [], "because": []}]
    h = stub_handler()
    assert h.handle([{"body": [2, 5]}]) == [{"items": [[2, 3], [5, 6]]}] and h.model.calls == []     # no explain: as before
    assert h.inference_explained([3], 2)["because"][0][0]["items"] == [[4, 0.5]]
    # ids alone come in every form the plain path takes
    h = stub_handler()
    out = h.handle([{"body": {"requests": [np.int64(7), np.int32(2)], "explain": 1}}])[0]
    assert out["items"] == h.handle([{"body": [np.int64(7), np.int32(2)]}])[0]["items"] and h.model.calls[0][:2] == ("ids", [7, 2])


@pytest.mark.parametrize("body", [
    {"requests": [1], "explain": 0}, {"requests": [1], "explain": 9}, {"requests": [1], "explain": True},
    {"requests": [1], "explain": "3"}, {"requests": [1], "explain": 2.0}, {"requests": [1], "explain": None},
    {"requests": [1]}, {"explain": 3}, {"requests": 1, "explain": 3}, {"requests": [1], "explain": 3, "extra": 1},
    {"requests": [1, "x"], "explain": 3}, {"requests": [{"items": [1]}, "7"], "explain": 3}, {"requests": [{"items": [30]}], "explain": 3}, {}])
def test_handler_refuses_malformed_explain_bodies(body):
    h = stub_handler()
    with pytest.raises(ValueError):
        h.inference(body)
    assert h.model.calls == []
    with pytest.raises(IndexError):
        stub_handler().inference({"requests": [10], "explain": 3})                       # a plain id out of range: as today
