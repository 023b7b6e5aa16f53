"""lgc_fold_in on the device, through the C ABI and through the Python layer: the kernel against the fp64 formula inside
the DERIVED element bound |y - y64| <= (1.5 n + 8) 2^-24 S over every path of the kernel, lists of
up to 32 entries bit for bit against the fp32 emulation of the specified order, run-to-run identical bits; the status
bits and edge cases; the two identities (a trained user's own list gives its served row; the augmented one-way graph
through the library's own get_embedding); recommend_sessions against torch.topk of the fp64-rescored masked matrix; the
fold table's cache; and the handler with mixed requests."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_fro, t, worst_row_rel
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate, synth
from gnn_ecommerce_amd.foldin import SessionLists
from tests_support import assert_topk_exact_up_to_ties
import foldin_support as fs

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 257, 5000)
DIMS = (1, 3, 4, 63, 64, 65, 90, 128, 129, 256)
WEIGHT_SET = np.array([0.01, 0.1, 1.0], dtype=np.float32)


def strided(a, pad, device):
    """The rows of ``a`` inside a wider device buffer: a [rows, cols] view whose row stride is cols + pad."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=device)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(device)
    return buf[:, :a.shape[1]]


def call(dev, ptr, items, weights, dis, fold, rows, init, a0, normalize, out):
    """lgc_fold_in with device tensors (``fold``, ``init``, ``out`` may be strided views); returns the status word."""
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    code = _native.load().lgc_fold_in(
        _native.ptr(ptr), _native.ptr(items), _native.ptr(weights), ptr.numel() - 1, _native.ptr(dis), _native.ptr(fold),
        fold.stride(0), fold.size(0), _native.ptr(rows), _native.ptr(init), 0 if init is None else init.stride(0),
        0 if init is None else init.size(0), a0, int(normalize), fold.size(1), _native.ptr(out), out.stride(0),
        _native.ptr(status), _native.stream_of(dev))
    assert code == 0, code
    return int(status[0].item())


@pytest.fixture(scope="module")
def grid_lists():
    """Per n_items: the lists of one call (every length, shuffled so that long and short rows share workgroups; items
    drawn with replacement, so a list repeats items -- 37 items in 5,000 entries certainly), weights, init rows."""
    out = {}
    for n_items in (37, 5000):
        rng = np.random.default_rng(n_items)
        order = rng.permutation(len(LENGTHS))
        lists = [rng.integers(n_items, size=LENGTHS[j]) for j in order]
        lists[1][:] = lists[1][:1] if len(lists[1]) else lists[1]                      # one list of a single repeated item
        ptr, items = fs.csr(lists)
        weights = WEIGHT_SET[rng.integers(3, size=len(items))]
        dis = rng.uniform(0.05, 1.0, n_items).astype(np.float32)
        n_init = 11
        rows = rng.integers(n_init, size=len(lists))
        rows[::3] = -1                                                                 # mixed with "no row"
        out[n_items] = dict(ptr=ptr, items=items, weights=weights, dis=dis, rows=rows, n_init=n_init)
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_kernel_inside_the_derived_bound_and_short_lists_bit_for_bit(device, grid_lists, dim):
    a0 = 0.3
    worst = 0.0
    for n_items, g in grid_lists.items():
        rng = np.random.default_rng(dim * 7 + n_items)
        fold = rng.standard_normal((n_items, dim)).astype(np.float32)
        init = rng.standard_normal((g["n_init"], dim)).astype(np.float32)
        ptr, items = g["ptr"], g["items"]
        n_rows = len(ptr) - 1
        short = np.flatnonzero(np.diff(ptr) <= 32)
        d_ptr, d_items = torch.from_numpy(ptr).to(device), torch.from_numpy(items).to(device)
        d_dis, d_rows = torch.from_numpy(g["dis"]).to(device), torch.from_numpy(g["rows"]).to(device)
        refs = {}
        for pad in (0, 3):
            d_fold, d_init = strided(fold, pad, device), strided(init, pad, device)
            for weights in (None, g["weights"]):
                d_w = None if weights is None else torch.from_numpy(weights).to(device)
                for rows in (None, g["rows"]):
                    for normalize in (0, 1):
                        key = (weights is None, rows is None, normalize)
                        if key not in refs:                                            # one reference per case, shared by the strides
                            args = (ptr, items, weights, g["dis"], fold, rows, init, a0, bool(normalize))
                            y64, s = fs.reference64(*args)
                            refs[key] = (y64, fs.bound(ptr, items, n_items, s), fs.emulate32(*_rows_only(args, short)))
                        y64, bound, y32 = refs[key]
                        got = []
                        for _ in range(2):                                             # twice: the same bits on every run
                            out = strided(np.zeros((n_rows, dim), dtype=np.float32), pad, device)
                            st = call(device, d_ptr, d_items, d_w, d_dis if normalize else None, d_fold,
                                      None if rows is None else d_rows, None if rows is None else d_init, a0, normalize, out)
                            assert st == 0
                            got.append(out.cpu().numpy())
                        assert np.array_equal(got[0], got[1]), (dim, n_items, pad, key)
                        err = np.abs(got[0].astype(np.float64) - y64)
                        assert (err <= bound).all(), (dim, n_items, pad, key, float((err / np.maximum(bound, 1e-300)).max()))
                        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
                        assert np.array_equal(got[0][short], y32), (dim, n_items, pad, key)   # lists of up to 32: bit for bit
    print(f"dim {dim}: worst error / bound = {worst:.3f}")


def _rows_only(args, keep):
    """The same arguments with only the rows ``keep`` (the emulation walks entries one by one: short lists only)."""
    ptr, items, weights, dis, fold, rows, init, a0, normalize = args
    lists = [items[ptr[r]:ptr[r + 1]] for r in keep]
    p, it = fs.csr(lists)
    w = None if weights is None else np.concatenate([weights[ptr[r]:ptr[r + 1]] for r in keep]).astype(np.float32)
    return p, it, w, dis, fold, None if rows is None else rows[keep], init, a0, normalize


def test_status_bits_and_edge_cases(device):
    rng = np.random.default_rng(3)
    n_items, dim = 37, 64
    fold = rng.standard_normal((n_items, dim)).astype(np.float32)
    dis = rng.uniform(0.1, 1.0, n_items).astype(np.float32)
    init = rng.standard_normal((5, dim)).astype(np.float32)
    up = lambda a: torch.from_numpy(np.asarray(a)).to(device)
    d_fold, d_dis, d_init = up(fold), up(dis), up(init)
    # an out-of-range item is skipped -- it is left out of the degree too -- and flagged
    with_bad, without = [[3, n_items, 5, -1, 7], list(range(20)) + [2 ** 40] + list(range(20))], [[3, 5, 7], list(range(20)) * 2]
    w_bad = WEIGHT_SET[rng.integers(3, size=46)]
    keep = np.ones(46, dtype=bool)
    keep[[1, 3, 25]] = False
    ptr, items = fs.csr(with_bad)
    out = torch.empty((2, dim), device=device)
    assert call(device, up(ptr), up(items), up(w_bad), d_dis, d_fold, None, None, 0.0, 1, out) == _native.ST_INDEX_OOB
    p2, i2 = fs.csr(without)
    clean = torch.empty((2, dim), device=device)
    assert call(device, up(p2), up(i2), up(w_bad[keep]), d_dis, d_fold, None, None, 0.0, 1, clean) == 0
    assert torch.equal(out[0], clean[0])                       # a short list: the very bits of the list without the entries
    assert np.array_equal(out[:1].cpu().numpy(), fs.emulate32(ptr[:2], items, w_bad, dis, fold, None, None, 0.0, True))
    y64, s = fs.reference64(p2, i2, w_bad[keep], dis, fold, None, None, 0.0, True)
    for rows in (out, clean):                                  # (41 entries: a longer list's order depends on the positions)
        assert (np.abs(rows.cpu().numpy() - y64) <= fs.bound(p2, i2, n_items, s)).all()
    # a bad init id is flagged and adds nothing; -1 is "no row" and no error
    ptr, items = fs.csr([[1, 2], [3], [4, 5, 6]])
    for rows, want in (([0, 5, -1], _native.ST_INDEX_OOB), ([0, -2, 4], _native.ST_INDEX_OOB), ([0, -1, 4], 0)):
        out = torch.empty((3, dim), device=device)
        assert call(device, up(ptr), up(items), None, d_dis, d_fold, up(rows), d_init, 0.5, 1, out) == want
        safe = np.array([r if 0 <= r < 5 else -1 for r in rows])
        assert np.array_equal(out.cpu().numpy(), fs.emulate32(ptr, items, None, dis, fold, safe, init, 0.5, True))
    # total weight 0: dis = 0 as in the build, the row is the init term (or zeros); an empty list the same
    ptr, items = fs.csr([[1, 2, 3], [4, 5], [], []])
    w0 = np.array([0.0, 0.0, 0.0, 0.5, -0.5], dtype=np.float32)
    out = torch.empty((4, dim), device=device)
    assert call(device, up(ptr), up(items), up(w0), d_dis, d_fold, up([2, -1, 3, -1]), d_init, 0.5, 1, out) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[0], np.float32(0.5) * init[2]) and not got[1].any()
    assert np.array_equal(got[2], np.float32(0.5) * init[3]) and not got[3].any()
    # a negative total weight: NaN, as upstream's deg ** -0.5
    ptr, items = fs.csr([[1, 2]])
    out = torch.empty((1, dim), device=device)
    assert call(device, up(ptr), up(items), up(np.array([0.5, -1.0], dtype=np.float32)), d_dis, d_fold, None, None, 0.0, 1, out) == 0
    assert torch.isnan(out).all()
    # no rows: nothing is written
    out = torch.full((2, dim), 7.0, device=device)
    assert call(device, up(np.zeros(1, dtype=np.int64)), up(np.zeros(1, dtype=np.int64)), None, d_dis, d_fold, None, None, 0.0, 1,
                out) == 0
    assert (out == 7.0).all()
    assert lg.fold_in(d_fold, d_dis, SessionLists.from_lists([], device)).shape == (0, dim)
    only_empty = lg.fold_in(d_fold, d_dis, SessionLists.from_lists([([], None), ([], [])], device))   # no item array at all
    assert only_empty.shape == (2, dim) and not only_empty.any()
    # the Python layer reports the flag the way score_rows does
    lg.check_index_status(device)
    s = SessionLists(up(np.array([0, 2])), up(np.array([1, 99])))
    lg.fold_in(d_fold, d_dis, s)
    with pytest.raises(IndexError):
        lg.check_index_status(device)
    with pytest.raises(ValueError):
        s.validate(n_items)


# ---------------------------------------------------------------------------------------------------------------
# the identities, through the library
# ---------------------------------------------------------------------------------------------------------------
def trained_model(g, dim, layers, device, seed=0):
    model = lg.LightGCN(g.num_nodes, dim, layers)
    rng = np.random.default_rng(seed)
    alpha = torch.from_numpy(rng.uniform(0.1, 0.4, layers + 1).astype(np.float32))
    model.load_state_dict({"alpha": alpha, "embedding.weight": synth.xavier_table(g.num_nodes, dim, seed)})
    return model.to(device).eval()


def own_lists(g, users):
    """Each user's own edge list in edge order: (item indices, weights)."""
    return [(g.item[g.user == u].tolist(), g.weight[g.user == u].tolist()) for u in users]


@pytest.fixture(scope="module", params=[(300, 37, 1500), (2000, 500, 16000)], ids=["300x37", "2000x500"])
def shop(request):
    return synth.make_bipartite(*request.param, seed=4)


@pytest.mark.parametrize("dim,layers", [(64, 3), (90, 5)])
def test_own_list_with_own_row_is_the_served_embedding(device, shop, dim, layers):
    g = shop
    model = trained_model(g, dim, layers, device)
    ei, ew = g.coo(device)
    users = np.random.default_rng(1).permutation(g.n_users)[:64]
    sessions = SessionLists.from_lists(own_lists(g, users), device)
    with torch.no_grad():
        got = model.embed_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users=users.tolist())
        want = model._serving_embedding(ei, ew)[torch.from_numpy(users).to(device)]
    lg.check_index_status(device)
    e_fro, e_row = rel_fro(got.cpu(), want.cpu()), worst_row_rel(got.cpu(), want.cpu())
    print(f"own lists {g.n_users}x{g.n_items} D={dim} K={layers}: rel_fro {e_fro:.2e}, worst row {e_row:.2e}")
    assert e_fro <= 1e-5 and e_row <= 1e-5


@pytest.mark.parametrize("dim,layers", [(64, 3), (90, 5)])
def test_appended_one_way_nodes_through_get_embedding(device, shop, dim, layers):
    g = shop
    model = trained_model(g, dim, layers, device)
    ei, ew = g.coo()
    rng = np.random.default_rng(2)
    lists = [rng.integers(g.n_items, size=m).tolist() for m in (1, 5, 20, 33, 70, 0)]
    weights = [WEIGHT_SET[rng.integers(3, size=len(x))] for x in lists]
    init_users = [-1, 7, -1, 3, 0, 5]
    n = g.num_nodes
    w2, ei2, ew2 = fs.augmented(model.embedding.weight.detach().cpu(), ei, ew, g.n_users, lists, weights, init_users)
    big = lg.LightGCN(n + 6, dim, layers)
    big.load_state_dict({"alpha": model.alpha.cpu(), "embedding.weight": w2})
    big.to(device).eval()
    ei_d, ew_d = ei.to(device), ew.to(device)
    with torch.no_grad():
        full = big.get_embedding(ei2.to(device), ew2.to(device))
        base = model.get_embedding(ei_d, ew_d)
        sessions = SessionLists.from_lists(list(zip(lists, weights)), device)
        got = model.embed_sessions(ei_d, ew_d, g.n_users, g.n_items, sessions, init_users=init_users)
    lg.check_index_status(device)
    # the trained nodes do not move: the project's gates, not bits -- the larger graph is no longer user|item, so the
    # library sums the same rows along its general route (the oracle's rows ARE bit-identical: test_foldin_host.py)
    assert rel_fro(full[:n].cpu(), base.cpu()) <= 1e-5 and worst_row_rel(full[:n].cpu(), base.cpu()) <= 1e-5
    e_fro, e_row = rel_fro(got.cpu(), full[n:].cpu()), worst_row_rel(got.cpu(), full[n:].cpu())
    print(f"appended nodes {g.n_users}x{g.n_items} D={dim} K={layers}: rel_fro {e_fro:.2e}, worst row {e_row:.2e}")
    assert e_fro <= 1e-5 and e_row <= 1e-5


# ---------------------------------------------------------------------------------------------------------------
# recommend_sessions
# ---------------------------------------------------------------------------------------------------------------
def test_recommend_sessions_ranking_mask_panels_and_table_cache(device):
    g = synth.make_bipartite(2000, 500, 16000, seed=4)
    dim, layers, k = 64, 3, 20
    model = trained_model(g, dim, layers, device)
    ei, ew = g.coo(device)
    rng = np.random.default_rng(5)
    lists = [rng.permutation(g.n_items)[:m].tolist() for m in (20, 1, 0, 40, 20, 7, 33)]
    weights = [WEIGHT_SET[rng.integers(3, size=len(x))] for x in lists]
    weights[0][:4] = 1.0
    init_users = [-1, 3, 9, -1, -1, 11, -1]
    sessions = SessionLists.from_lists(list(zip(lists, weights)), device)
    built = model.fold_tables_built
    with torch.no_grad():
        rows = model.embed_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users)
        top, val = model.recommend_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users, k=k, return_values=True)
        top_all = model.recommend_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users, k=k, mask="all")
        top_none = model.recommend_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users, k=k, mask=None)
        small = model.recommend_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users, k=k, return_values=True,
                                         workspace_bytes=3 * 4 * g.n_items)      # three score rows per panel
        item_t = model._serving_embedding(ei, ew)[g.n_users:]
    assert model.fold_tables_built == built + 1                                      # computed once across the five calls
    assert top.dtype == torch.int64 and top.shape == (7, k) and top.is_cuda
    assert torch.equal(small[0], top) and torch.equal(small[1], val)                 # independent of the panel size, bit for bit
    scores = rows.double().cpu() @ item_t.double().cpu().t()                         # the fp64 rescoring of the same rows
    for rule, got in (("purchased", top), ("all", top_all), (None, top_none)):
        masked = scores.clone()
        for r, (x, w) in enumerate(zip(lists, weights)):
            seen = [i for i, wi in zip(x, w) if rule == "all" or (rule == "purchased" and wi == 1.0)]
            masked[r, seen] *= 0.0
        want = masked.topk(k, dim=-1).indices
        assert_topk_exact_up_to_ties(got.cpu().numpy(), want.numpy(), masked.numpy())
    # "purchased" zeroes exactly the weight-1.0 items: their masked score is 0, everything else keeps its score
    with torch.no_grad():
        panel = propagate.score_rows(rows, None, item_t)
    for r, (x, w) in enumerate(zip(lists, weights)):
        bought = {i for i, wi in zip(x, w) if wi == 1.0}
        for p, i in enumerate(top[r].tolist()):
            assert val[r, p].item() == (0.0 if i in bought else panel[r, i].item())
    assert any(w_.tolist().count(1.0) for w_ in weights)
    # the fold table: again after an optimizer step, and after invalidate()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    model.embedding.weight.grad = torch.ones_like(model.embedding.weight)
    opt.step()
    with torch.no_grad():
        moved = model.embed_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users)
        model.embed_sessions(ei, ew, g.n_users, g.n_items, sessions, init_users)
    assert model.fold_tables_built == built + 2 and not torch.equal(moved, rows)
    model.invalidate()
    with torch.no_grad():
        again = model.embed_sessions(g.coo(device)[0], g.coo(device)[1], g.n_users, g.n_items, sessions, init_users)
    assert model.fold_tables_built == built + 3 and torch.equal(again, moved)
    lg.check_index_status(device)


# ---------------------------------------------------------------------------------------------------------------
# the handler
# ---------------------------------------------------------------------------------------------------------------
def test_handler_answers_mixed_requests_position_by_position(device, tmp_path):
    from gnn_ecommerce_amd import ingest, serving
    z = load_golden("ingest_ref")
    it = ingest.relabel(z["user_id"], z["item_id"], z["weight"])
    d = str(tmp_path)
    ingest.save_serving_graph(os.path.join(d, serving.GRAPH_FILE), it, device=device)
    model = lg.LightGCN(it.n_users + it.n_items, 64, 2)
    torch.save({"model_state_dict": model.state_dict(), "hyperparams": {"latent_dim": 64, "n_layers": 2}}, os.path.join(d, "m.pt"))
    h = serving.RecommendHandler()
    h.initialize(types.SimpleNamespace(manifest={"model": {"serializedFile": "m.pt"}},
                                       system_properties={"model_dir": d, "gpu_id": None}))
    k = min(20, it.n_items)
    h.k = k
    a = {"items": [0, 1, 2], "weights": [1.0, 0.1, 0.01]}
    b = {"items": [1], "user": 2}
    c = {"items": []}
    mixed = h.handle([{"body": [1, a, 0, b, c, it.n_users - 1]}])[0]["items"]
    assert len(mixed) == 6 and all(isinstance(x, list) and len(x) == k for x in mixed)
    ids = h.handle([{"body": [1, 0, it.n_users - 1]}])[0]["items"]
    assert [mixed[0], mixed[2], mixed[5]] == ids
    assert [mixed[1], mixed[3], mixed[4]] == h.handle([{"body": [a, b, c]}])[0]["items"]
    for el, row in zip((a, b, c), (mixed[1], mixed[3], mixed[4])):
        assert h.handle([{"body": [el]}])[0]["items"] == [row]
    # and directly: the same ranking recommend_sessions gives
    s = SessionLists.from_lists([(a["items"], a["weights"]), (b["items"], None), ([], None)], device)
    with torch.no_grad():
        want = h.model.recommend_sessions(h.graph, None, it.n_users, it.n_items, s, [-1, 2, -1], k)
    assert want.cpu().tolist() == [mixed[1], mixed[3], mixed[4]]
    with pytest.raises(ValueError):
        h.handle([{"body": [1, {"items": [it.n_items]}]}])
    with pytest.raises(IndexError):
        h.handle([{"body": [it.n_users]}])                                           # ids alone: today's error


def test_ids_only_requests_still_give_the_reference_handlers_answers(device, tmp_path):
    """serve_ref.npz through the handler as before: a request of plain ids takes the unchanged path."""
    from gnn_ecommerce_amd import serving
    from gnn_ecommerce_amd.graph import PropGraph
    from oracle import lightgcn_oracle as oracle
    z = load_golden("serve_ref")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    d = str(tmp_path)
    graph = PropGraph(t(z["edge_index"]).to(device), t(z["edge_weight"]).to(device), nu + ni)
    si = z["seen_indices"]
    ptr = np.zeros(nu + 1, dtype=np.int64)
    np.cumsum(np.bincount(si[0], minlength=nu), out=ptr[1:])
    graph.save(os.path.join(d, serving.GRAPH_FILE), extra={"seen_ptr": torch.from_numpy(ptr), "seen_items": t(si[1])},
               meta={"n_users": nu, "n_items": ni})
    torch.save({"model_state_dict": {"alpha": t(z["alpha"]), "embedding.weight": t(z["weight0"])},
                "hyperparams": {"latent_dim": int(z["dim"]), "n_layers": int(z["layers"])}}, os.path.join(d, "model.pt"))
    h = serving.RecommendHandler()
    h.initialize(types.SimpleNamespace(manifest={"model": {"serializedFile": "model.pt"}},
                                       system_properties={"model_dir": d, "gpu_id": 0}))
    emb = oracle.get_embedding(t(z["weight0"]), t(z["alpha"]), t(z["edge_index"]), t(z["edge_weight"]), int(z["layers"]))
    seen = torch.zeros(nu, ni)
    seen[si[0], si[1]] = 1.0
    users, items = torch.split(emb, [nu, ni])
    for r in range(int(z["n_requests"])):
        req = z[f"request{r}"].tolist()
        got = h.handle([{"body": req}])[0]["items"]
        masked = (users[req] @ items.t()) * (1 - seen[req])
        assert_topk_exact_up_to_ties(np.array(got), z[f"response{r}"], masked.numpy())
