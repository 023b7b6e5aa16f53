"""Diversified re-ranking on the device, through the C ABI: lgc_rerank_mmr and lgc_list_diversity against the numpy
restatement of their contract (rerank_support), with the similarities taken from the device's own bits -- lgc_score_rows
at the candidate columns, scaled in fp32 as test_similar_gpu.py does.  The order is strict and the arithmetic stated, so
every comparison is an equality: indices, positions, and values bit for bit (after x + 0, any NaN matching any NaN)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate, rerank, similar, synth
from gnn_ecommerce_amd.propagate import SeenLists
import rerank_support as rs
import similar_support as ss
import topk_support as ts

pytestmark = pytest.mark.gpu


def up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def strided(table, device, pad=3):
    """The table on the device with rows `pad` floats further apart than they are wide; the padding holds NaN."""
    n, dim = table.shape
    if pad == 0:
        return up(table, device)
    buf = torch.full((n, dim + pad), float("nan"), dtype=torch.float32, device=device)
    buf[:, :dim] = up(table, device)
    return buf[:, :dim]


def mmr_abi(t, cand, rel, k, lam, scale=None, values=True):
    """(index, pos, value, status word) of one lgc_rerank_mmr call; outputs pre-filled with junk, one row past the end too."""
    dev, (n, n_cand) = t.device, cand.shape
    index = torch.full((n + 1, k), -77, dtype=torch.int64, device=dev)
    pos = torch.full((n + 1, k), -77, dtype=torch.int32, device=dev) if values else None
    value = torch.full((n + 1, k), 77.0, dtype=torch.float32, device=dev) if values else None
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    code = _native.load().lgc_rerank_mmr(t.data_ptr(), t.stride(0), t.size(0), t.size(1), _native.ptr(scale), cand.data_ptr(),
                                         cand.stride(0), rel.data_ptr(), rel.stride(0), n, n_cand, k, lam, index.data_ptr(),
                                         _native.ptr(pos), _native.ptr(value), status.data_ptr(), _native.stream_of(dev))
    assert code == 0
    assert index[n].tolist() == [-77] * k                                               # nothing written past the rows
    if not values:
        return index[:n].cpu().numpy(), None, None, int(status[0].item())
    assert pos[n].tolist() == [-77] * k and value[n].tolist() == [77.0] * k
    return index[:n].cpu().numpy(), pos[:n].cpu().numpy(), value[:n].cpu().numpy(), int(status[0].item())


def diversity_abi(t, lists, cutoffs, scale=None):
    dev, (n, k) = t.device, lists.shape
    cuts = (ctypes.c_int32 * len(cutoffs))(*cutoffs)
    out = torch.full((n + 1, len(cutoffs)), 77.0, dtype=torch.float64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    code = _native.load().lgc_list_diversity(t.data_ptr(), t.stride(0), t.size(0), t.size(1), _native.ptr(scale), lists.data_ptr(),
                                             lists.stride(0), n, k, cuts, len(cutoffs), out.data_ptr(), len(cutoffs),
                                             status.data_ptr(), _native.stream_of(dev))
    assert code == 0 and out[n].tolist() == [77.0] * len(cutoffs)
    return out[:n].cpu().numpy(), int(status[0].item())


def device_sims(t, scale, cand_np):
    """``sims(r)`` -> row r's ``sim_of(ps, c)`` from the device's bits: lgc_score_rows of every item the lists name against
    the table, then the two multiplies in torch fp32, left to right -- entry [i, j] = (dot(i, j) * scale[i]) * scale[j]."""
    n_items = t.size(0)
    ok = (cand_np >= 0) & (cand_np < n_items)
    uniq = np.unique(cand_np[ok]) if ok.any() else np.zeros(1, dtype=np.int64)
    ids = up(uniq.astype(np.int64), t.device)
    panel = propagate.score_rows(t, ids, t)
    if scale is not None:
        panel = (panel * scale[ids][:, None]) * scale[None, :]
    lg.check_index_status(t.device)
    panel = panel.cpu().numpy()
    where = np.full(n_items, -1, dtype=np.int64)
    where[uniq] = np.arange(uniq.size)
    return lambda r: (lambda ps, c: panel[where[cand_np[r, ps]], cand_np[r, c]])


def check_mmr(t, scale, cand_np, rel_np, k, lam, what, sims=None, want_status=0):
    """One call against the reference: indices and positions equal, values bit-equal after x + 0."""
    sims = sims or device_sims(t, scale, cand_np)
    want = rs.mmr_ref_rows(rel_np, cand_np, sims, k, lam, t.size(0))
    got_i, got_p, got_v, status = mmr_abi(t, up(cand_np, t.device), up(rel_np, t.device), k, lam, scale)
    assert status == want_status, what
    assert np.array_equal(got_p, want[1]), (what, np.argwhere(got_p != want[1])[:5].tolist())
    assert np.array_equal(got_i, want[0]), what
    assert ss.same_values(got_v, want[2]), what
    return want


def scale_of(t, metric):
    return similar.row_rnorm(t) if metric == "cosine" else None


# ---------------------------------------------------------------------------------------------------------------
# 1. every shape at which the kernel takes another path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sorted({d for _, d in rs.GPU_SHAPES}))
def test_mmr_equals_the_reference_at_every_edge_shape(device, dim):
    """Every list length x both tables (37 items, rows D apart; 5,000 items, rows D + 3 apart) x both metrics x every k;
    lambda rotates so that every (k, lambda, table, metric) combination occurs from 63 candidates on, the number of rows
    with a counter that advances once per call."""
    assert _native.load().lgc_dim_ok(dim)
    rng = np.random.default_rng(100 + dim)
    tables = ((37, strided(ss.random_table(rng, 37, dim), device, 0)), (5000, strided(ss.random_table(rng, 5000, dim), device, 3)))
    assert tables[0][1].stride(0) == dim and tables[1][1].stride(0) == dim + 3
    scales = {(n_items, metric): scale_of(t, metric) for n_items, t in tables for metric in ("cosine", "dot")}
    case, loop, routes, covered, combos = 0, 0, set(), set(), set()
    for ni, n_cand in enumerate([n for n, d in rs.GPU_SHAPES if d == dim]):
        routes.add(rerank.rerank_route(n_cand, dim))
        for n_items, t in tables:
            for metric in ("cosine", "dot"):
                scale = scales[n_items, metric]
                for ki, k in enumerate(rs.ks_of(n_cand)):
                    lam, n_rows = (0.0, 0.3, 0.7, 1.0)[(ki + loop + ni) % 4], (1, 3)[(case // 3) % 2]
                    case += 1
                    cand = rs.candidates(rng, n_rows, n_cand, n_items)
                    rel = ss.random_table(rng, n_rows, n_cand)
                    check_mmr(t, scale, cand, rel, k, lam, (dim, n_cand, k, lam, metric, n_items, n_rows))
                    if k > 1:                                                           # a call that computes dots
                        covered.add((lam, n_rows))
                    if n_cand > 2:
                        combos.add((ki, lam, n_items, metric))
                loop += 1
    assert routes == ({"lds"} if dim <= 4 else {"lds", "global"})                       # 256 rows of up to 4 floats fit; of 63 and more not
    assert covered == {(lam, n_rows) for lam in (0.0, 0.3, 0.7, 1.0) for n_rows in (1, 3)}
    assert len(combos) == 4 * 4 * 2 * 2


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_every_lambda_and_metric_on_more_rows_than_compute_units(device, lam, metric):
    rng = np.random.default_rng(200)
    n_cand, k, dim = 100, 20, 24
    for n_items, kind, n_rows in ((37, "repeated", 300), (5000, "distinct", 40)):
        t = strided(ss.random_table(rng, n_items, dim), device)
        cand = rs.candidates(rng, n_rows, n_cand, n_items, kind)
        if n_items == 5000:
            cand = cand % 600                                                           # a panel of 600 rows, not of 5,000
        rel = rs.descending_rel(rng, n_rows, n_cand)
        want = check_mmr(t, scale_of(t, metric), cand, rel, k, lam, (lam, metric, n_items))
        if lam == 1.0:                                                                  # the plain ranking of the relevances
            assert np.array_equal(want[1], ts.topk_ref(rel, k)[0])


def test_without_positions_and_values_the_indices_are_the_same(device):
    rng = np.random.default_rng(3)
    t = strided(ss.random_table(rng, 300, 8), device)
    cand, rel = up(rs.candidates(rng, 5, 70, 300), device), up(ss.random_table(rng, 5, 70), device)
    a, _, _, _ = mmr_abi(t, cand, rel, 9, 0.5)
    b, p, v, _ = mmr_abi(t, cand, rel, 9, 0.5, values=False)
    assert p is None and v is None and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# 2. ties go by position
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand", [100, 256])
def test_long_runs_of_equal_objectives_fall_to_the_lower_position(device, n_cand):
    rng = np.random.default_rng(300 + n_cand)
    n_items, dim, k = 300, 4, 20
    table = ss.integer_table(rng, n_items, dim, hi=1)
    t = strided(table, device)
    cand = rs.candidates(rng, 3, n_cand, n_items)
    rel = rs.descending_rel(rng, 3, n_cand)
    rel[2] = 1.0                                                                        # one row of all-equal relevance
    # lam = 0.5 and relevances in eighths: every objective is exact, so the device's similarities are the integers' and
    # the reference can be stated without the device
    want = check_mmr(t, None, cand, rel, k, 0.5, ("ties", n_cand))
    for r in range(3):
        exact = rs.mmr_ref(rel[r], cand[r], rs.exact_sims(table, cand[r]), k, 0.5)
        assert np.array_equal(want[1][r], exact[1]) and ss.same_values(want[2][r], exact[2])
    assert want[1][2, 0] == 0                                                           # the premise: step 0 of row 2 is one tie
    check_mmr(t, up(np.full(n_items, 0.5, dtype=np.float32), device), cand, rel, n_cand, 0.5, ("ties, scaled, k = n_cand", n_cand))
    # every item the same and every relevance equal: positions in order, whatever lambda
    same = strided(np.ones((n_cand, dim), dtype=np.float32), device)
    ones = torch.ones((1, n_cand), dtype=torch.float32, device=device)
    got_i, got_p, _, _ = mmr_abi(same, up(np.arange(n_cand)[None, ::-1].copy(), device), ones, n_cand, 0.3)
    assert got_p[0].tolist() == list(range(n_cand)) and got_i[0].tolist() == list(range(n_cand))[::-1]


# ---------------------------------------------------------------------------------------------------------------
# 3. duplicates, empty places, short rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand", [65, 200])
def test_repeated_ids_and_empty_places(device, n_cand):
    rng = np.random.default_rng(400 + n_cand)
    n_items, dim = 50, 12
    t = strided(ss.random_table(rng, n_items, dim), device)
    scale = scale_of(t, "cosine")
    for kind in ("repeated", "short"):
        cand = rs.candidates(rng, 6, n_cand, n_items, kind)
        if kind == "short":
            cand[0] = -1                                                                # a row of nothing
            cand[1, 1:] = -1                                                            # a row of one
        rel = ss.random_table(rng, 6, n_cand)
        for k in (1, 20, n_cand):
            want_i, want_p, want_v = check_mmr(t, scale, cand, rel, k, 0.7, (kind, n_cand, k))
            n_valid = (cand >= 0).sum(axis=1)
            for r in range(6):
                m = min(k, int(n_valid[r]))
                assert (want_p[r, :m] >= 0).all() and (want_p[r, m:] == -1).all() and (want_i[r, m:] == -1).all()
                assert np.all(want_v[r, m:] == -np.inf) and len(set(want_p[r, :m].tolist())) == m
                assert np.array_equal(cand[r, want_p[r, :m]], want_i[r, :m])
    # the twin of a chosen item pays the whole penalty: with the cosine it is the last of the finite places
    cand = np.array([[7, 3, 7, 9, 11]], dtype=np.int64)
    rel = np.ones((1, 5), dtype=np.float32)
    _, pos, _ = check_mmr(t, scale, cand, rel, 5, 0.1, "twin")
    assert pos[0, 0] == 0 and pos[0, -1] == 2


# ---------------------------------------------------------------------------------------------------------------
# 4. ids outside the table
# ---------------------------------------------------------------------------------------------------------------
def test_ids_out_of_range_are_skipped_and_flagged_and_nothing_else_moves(device):
    rng = np.random.default_rng(500)
    n_items, dim, n_cand, k = 300, 16, 130, 20
    t = strided(ss.random_table(rng, n_items, dim), device)
    scale = scale_of(t, "cosine")
    rel = ss.random_table(rng, 5, n_cand)
    rel[:, [0, 64, 129]] = 50.0                                                         # the planted places would lead
    bad = rs.candidates(rng, 5, n_cand, n_items)
    clean = bad.copy()
    bad[0, [0, 64, 129]] = [n_items, -2, 2 ** 40 + 3]                                   # the low 32 bits of the last name an item
    bad[2, 0] = -2 ** 40
    bad[4, 64] = n_items + 1000
    clean[bad != clean] = -1
    want = check_mmr(t, scale, bad, rel, k, 0.7, "out of range", want_status=_native.ST_INDEX_OOB)
    same = check_mmr(t, scale, clean, rel, k, 0.7, "the same places empty")
    assert all(np.array_equal(a, b) for a, b in zip(want[:2], same[:2])) and ss.same_values(want[2], same[2])
    assert not np.isin(want[1][0], [0, 64, 129]).any() and (want[1][1] >= 0).all()
    # through the library the status word raises
    lg.check_index_status(device)
    index = rerank.mmr_rerank(t, up(bad, device), up(rel, device), k, 0.7)
    with pytest.raises(IndexError):
        lg.check_index_status(device)
    assert np.array_equal(index.cpu().numpy(), want[0])
    lg.check_index_status(device)                                                       # cleared
    got, status = diversity_abi(t, up(bad, device), (5, 130), scale)
    clean_got, clean_status = diversity_abi(t, up(clean, device), (5, 130), scale)
    assert status & _native.ST_INDEX_OOB and clean_status == 0 and rs.same_doubles(got, clean_got)


# ---------------------------------------------------------------------------------------------------------------
# 5. special values
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_nan_inf_zero_rows_and_subnormals_follow_the_contract(device, metric):
    rng = np.random.default_rng(600)
    n_items, dim, n_cand, k = 80, 20, 70, 70
    table, rows = ss.special_table(rng, n_items, dim)
    t = strided(table, device)
    scale = scale_of(t, metric)
    cand = rs.candidates(rng, 4, n_cand, n_items)
    for r in range(4):                                                                  # every special row is a candidate
        missing = np.setdiff1d(rows, cand[r])
        cand[r, rng.permutation(n_cand)[:missing.size]] = missing
    rel = ss.random_table(rng, 4, n_cand)
    for lam in (0.0, 0.3, 1.0):
        want = check_mmr(t, scale, cand, rel, k, lam, ("special rows", metric, lam))
        if lam < 1.0:                                                                   # the premise: NaN objectives arose and led
            assert np.isnan(want[2][:, 1:]).any()
    # the relevances: NaNs of both signs and several payloads, +-inf
    plain = strided(ss.random_table(rng, n_items, dim), device)
    for r in range(4):
        ts.plant_specials(rng, rel[r])
    for lam in (0.3, 1.0):
        want = check_mmr(plain, scale_of(plain, metric), cand, rel, k, lam, ("special relevances", metric, lam))
        assert np.isnan(want[2][:, :8]).all() and not np.isnan(want[2][:, 8:]).any()
        assert np.all(want[2][:, 8:10] == np.inf) and np.all(want[2][:, -2:] == -np.inf)
    sub = strided(ss.subnormal_table(rng, n_items, dim), device)
    sub_scale = None if metric == "dot" else up(rng.uniform(0.5, 2.0, n_items).astype(np.float32), device)
    check_mmr(sub, sub_scale, cand, ss.subnormal_table(rng, 4, n_cand), k, 0.3, ("subnormal", metric))
    check_mmr(sub, sub_scale, cand, np.zeros((4, n_cand), dtype=np.float32), 20, 0.0, ("subnormal, lam 0", metric))


# ---------------------------------------------------------------------------------------------------------------
# 6. both sides of the LDS-staging boundary
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,edge", [(64, 135), (90, 100), (256, 35)])
def test_both_routes_give_the_same_answer_at_the_staging_boundary(device, dim, edge):
    assert _native.load().lgc_dim_ok(dim)
    assert rerank.rerank_route(edge, dim) == "lds" and rerank.rerank_route(edge + 1, dim) == "global"
    rng = np.random.default_rng(700 + dim)
    n_items, k = 400, 20
    t = strided(ss.random_table(rng, n_items, dim), device)
    scale = scale_of(t, "cosine")
    wide = rs.candidates(rng, 7, edge + 1, n_items)
    rel = ss.random_table(rng, 7, edge + 1)
    check_mmr(t, scale, wide, rel, k, 0.5, ("global side", dim))
    wide[:, edge] = -1                                                                  # the same lists, one empty place longer
    a = check_mmr(t, scale, wide, rel, k, 0.5, ("global side, last place empty", dim))
    b = check_mmr(t, scale, np.ascontiguousarray(wide[:, :edge]), np.ascontiguousarray(rel[:, :edge]), k, 0.5, ("lds side", dim))
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and ss.same_values(a[2], b[2])
    for cand in (wide, wide[:, :edge]):                                                 # lgc_list_diversity routes by k
        got, _ = diversity_abi(t, up(np.ascontiguousarray(cand), device), (2, 20, edge), scale)
        sims = device_sims(t, scale, cand)
        for r in range(7):
            sim = sims(r)(np.arange(edge)[:, None], np.arange(edge)[None, :])
            assert rs.same_doubles(got[r], rs.ild_ref(sim, np.ones(edge, dtype=bool), (2, 20, edge))), (dim, cand.shape, r)


# ---------------------------------------------------------------------------------------------------------------
# 7. lgc_list_diversity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 20, 256])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_list_diversity_equals_the_reference(device, k, metric):
    rng = np.random.default_rng(800 + k)
    n_items = 300
    cutoffs = tuple(sorted({1, 2, k}))
    for dim in (24, 65):                                                                # at k = 256: staged, and read from memory
        t = strided(ss.random_table(rng, n_items, dim), device)
        scale = scale_of(t, metric)
        lists = rs.candidates(rng, 5, k, n_items, "repeated")
        lists[1, rng.random(k) < 0.3] = -1
        lists[2] = -1
        lists[3, 1:] = -1
        lists[4, 0] = -1
        got, status = diversity_abi(t, up(lists, device), cutoffs, scale)
        assert status == 0
        sims = device_sims(t, scale, lists)
        for r in range(5):
            valid = lists[r] >= 0
            sim = sims(r)(np.arange(k)[:, None], np.arange(k)[None, :])
            want = rs.ild_ref(sim, valid, cutoffs)
            assert rs.same_doubles(got[r], want), (k, metric, dim, r, got[r], want)
        assert np.isnan(got[:, 0]).all() and np.isnan(got[2]).all() and np.isnan(got[3]).all()
        assert np.isfinite(got[0]).sum() == len(cutoffs) - 1
        # a cutoff is a snapshot: alone, and with a longer list behind it, it has the same bits
        alone, _ = diversity_abi(t, up(lists, device), cutoffs[-1:], scale)
        assert rs.same_doubles(alone[:, 0], got[:, -1])
        wrapped = rerank.list_diversity(t, up(lists, device), cutoffs, metric)
        assert wrapped.dtype == torch.float64 and rs.same_doubles(wrapped.cpu().numpy(), got)


def test_a_list_of_equal_items_has_diversity_0_and_of_orthogonal_ones_1(device):
    eye = strided(np.concatenate([np.eye(8, dtype=np.float32) * 2, np.ones((4, 8), dtype=np.float32)]), device)
    lists = up(np.array([[0, 1, 2, 3, 4, 5], [8, 9, 10, 11, 8, 9], [0, 0, 1, 1, -1, -1]], dtype=np.int64), device)
    got = rerank.list_diversity(eye, lists, (2, 4, 6)).cpu().numpy()
    assert got[0].tolist() == [1.0, 1.0, 1.0]
    assert np.abs(got[1]).max() <= 8 * 2.0 ** -24                                       # 1 - (8 * rnorm) * rnorm, rnorm = fl(1 / sqrt(8)): five roundings
    assert got[2, 0] == 0.0 and got[2, 1] == got[2, 2] == 4 / 6
    assert rerank.list_diversity(eye, lists, (2, 6), "dot").cpu().numpy()[0].tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------
# 8. through the library
# ---------------------------------------------------------------------------------------------------------------
def served_model(device, n_users, n_items, n_edges, dim, layers, seed, item_rows=None):
    g = synth.make_bipartite(n_users, n_items, n_edges, seed=seed)
    ei, ew = g.coo()
    model = lg.LightGCN(g.num_nodes, dim, layers)
    w = synth.xavier_table(g.num_nodes, dim, 1)
    if item_rows is not None:
        w = w.clone()
        w[n_users:] = torch.from_numpy(item_rows)
    model.load_state_dict({"alpha": model.alpha, "embedding.weight": w})
    model.to(device)
    return model, ei.to(device), ew.to(device), g


def random_seen(rng, n_users, n_items, per_user, device):
    lists = [np.sort(rng.permutation(n_items)[:per_user]) for _ in range(n_users)]
    ptr = np.arange(n_users + 1, dtype=np.int64) * per_user
    return SeenLists(up(ptr, device), up(np.concatenate(lists).astype(np.int64), device)).validate(n_users)


def test_recommend_diverse_with_lambda_1_is_recommend_topk_and_reranking_its_answer_is_the_same(device):
    model, ei, ew, g = served_model(device, 2000, 500, 20000, 32, 2, seed=6)
    rng = np.random.default_rng(900)
    users = rng.permutation(2000)[:130].tolist()
    k = 20
    for seen in (None, random_seen(rng, 2000, 500, 30, device)):
        args = (ei, ew, g.n_users, g.n_items, seen, users)
        plain = model.recommend_topk(*args, k)
        for metric in ("cosine", "dot"):
            same = model.recommend_diverse(*args, k, 100, 1.0, metric)
            assert same.dtype == torch.int64 and same.shape == (130, k) and torch.equal(same, plain)
        diverse = model.recommend_diverse(*args, k, 100, 0.5)
        assert torch.equal(diverse[:, 0], plain[:, 0]) and not torch.equal(diverse, plain)
        user_t, item_t, seen_l, ids = model._eval_tables(*args)
        top, value = propagate.recommend_topk(user_t, ids, item_t, seen_l, 100, return_values=True)
        again = model.rerank_diverse(ei, ew, g.n_users, g.n_items, top, value, k, 0.5)
        assert torch.equal(again, diverse)
        assert torch.equal(model.recommend_diverse(*args, k, 100, 0.5), diverse)        # two runs, the same bits
        index, pos, val = rerank.mmr_rerank(item_t, top, value, k, 0.5, return_values=True)
        index2, pos2, val2 = rerank.mmr_rerank(item_t, top, value, k, 0.5, return_values=True)
        assert torch.equal(index, diverse) and torch.equal(pos, pos2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))
        assert torch.equal(torch.gather(top, 1, pos.long()), index)
    lg.check_index_status(device)
    few = model.recommend_diverse(ei, ew, g.n_users, g.n_items, None, users[:3], 5, 256, 0.7)      # more candidates than needed
    assert few.shape == (3, 5)


def test_diverse_lists_are_at_least_as_diverse_as_plain_ones_on_a_catalogue_of_duplicated_groups(device):
    rng = np.random.default_rng(1000)
    n_users, groups, per_group, dim, k, n_cand = 60, 12, 8, 16, 10, 40
    n_items = groups * per_group
    table = rs.grouped_table(rng, groups, per_group, dim)
    model, ei, ew, g = served_model(device, n_users, n_items, 600, dim, 0, seed=7, item_rows=table)   # no layers: served = trained
    users = list(range(n_users))
    args = (ei, ew, n_users, n_items, None, users)
    with torch.no_grad():
        item_t = model._serving_embedding(ei, ew)[n_users:]
    assert torch.equal(item_t.cpu(), torch.from_numpy(table))
    # the reference first: from the device's similarity bits, greedy MMR at 0.3 is at least as diverse as the plain list
    user_t, item_t, _, ids = model._eval_tables(*args)
    top, value = propagate.recommend_topk(user_t, ids, item_t, None, n_cand, return_values=True)
    top_np, value_np = top.cpu().numpy(), value.cpu().numpy()
    scale = similar.row_rnorm(item_t)
    sims = device_sims(item_t, scale, top_np)
    ref = {}
    for lam in (0.3, 1.0):
        _, pos, _ = rs.mmr_ref_rows(value_np, top_np, sims, k, lam, n_items)
        ild = np.empty(n_users)
        for r in range(n_users):
            sim = sims(r)(pos[r][:, None], pos[r][None, :])
            ild[r] = rs.ild_ref(sim, np.ones(k, dtype=bool), (k,))[0]
        ref[lam] = (np.take_along_axis(top_np, pos.astype(np.int64), axis=1), ild)
    assert (ref[0.3][1] >= ref[1.0][1]).all() and (ref[0.3][1] > ref[1.0][1]).mean() > 0.5
    assert np.array_equal(ref[0.3][0][:, 0], ref[1.0][0][:, 0])                         # the first pick is shared
    # then the device: the same lists, the same diversity bits, the same means
    got = {}
    for lam in (0.3, 1.0):
        lists = model.recommend_diverse(*args, k, n_cand, lam)
        assert np.array_equal(lists.cpu().numpy(), ref[lam][0])
        values, mean = model.list_diversity(ei, ew, n_users, n_items, lists, (5, k))
        assert rs.same_doubles(values[:, 1].cpu().numpy(), ref[lam][1])
        sums = propagate.column_sums(values).cpu().numpy()
        assert isinstance(mean, tuple) and all(isinstance(m, float) for m in mean)
        assert mean == tuple(float(s) / n_users for s in sums)
        got[lam] = values[:, 1]
    assert bool((got[0.3] >= got[1.0]).all())


def test_handler_answers_a_diversify_body_like_the_library_and_other_bodies_as_before(device, tmp_path):
    from gnn_ecommerce_amd import ingest, serving
    from gnn_ecommerce_amd.foldin import SessionLists
    z = load_golden("ingest_ref")
    it = ingest.relabel(z["user_id"], z["item_id"], z["weight"])
    d = str(tmp_path)
    ingest.save_serving_graph(os.path.join(d, serving.GRAPH_FILE), it, device=device)
    dim = 64
    model = lg.LightGCN(it.n_users + it.n_items, dim, 2)
    torch.save({"model_state_dict": model.state_dict(), "hyperparams": {"latent_dim": dim, "n_layers": 2}}, os.path.join(d, "m.pt"))
    h = serving.RecommendHandler()
    h.initialize(types.SimpleNamespace(manifest={"model": {"serializedFile": "m.pt"}}, system_properties={"model_dir": d, "gpu_id": None}))
    h.k = min(5, it.n_items)
    n_cand = min(5 * h.k, 256, it.n_items)
    session = {"items": [0, it.n_items - 1], "weights": [1.0, 0.5]}
    known = {"items": [1], "user": 0}
    requests = [1, session, 0, known]
    def answer(body):
        return [[int(i) for i in row] for row in h.handle([{"body": body}])[0]["items"]]
    plain = answer(requests)
    out = h.handle([{"body": {"requests": requests, "diversify": 0.4}}])[0]
    assert sorted(out) == ["items"] and len(out["items"]) == 4 and all(len(row) == h.k for row in out["items"])
    assert answer(requests) == plain                                                    # without the key: today's answer
    assert answer({"requests": requests, "diversify": 1.0}) == plain                    # lambda 1: the plain ranking
    m, args = h.model, (h.graph, None, h.n_users, h.n_items)
    with torch.no_grad():
        ids = m.recommend_diverse(*args, h.seen, [1, 0], h.k, n_cand, 0.4, "cosine").cpu().tolist()
        sessions = SessionLists.from_lists([([0, it.n_items - 1], [1.0, 0.5]), ([1], None)], device)
        top, value = m.recommend_sessions(*args, sessions, [-1, 0], n_cand, return_values=True)
        folded = m.rerank_diverse(*args, top, value, h.k, 0.4, "cosine").cpu().tolist()
    assert out["items"] == [ids[0], folded[0], ids[1], folded[1]]
    dot = answer({"requests": [1], "diversify": 0.4, "candidates": h.k, "metric": "dot"})
    assert sorted(dot[0]) == sorted(answer([1])[0])                                     # k out of k candidates: the same set
    with pytest.raises(IndexError):
        h.handle([{"body": {"requests": [it.n_users], "diversify": 0.4}}])
    with pytest.raises(ValueError):
        h.handle([{"body": {"requests": [1], "diversify": 0.4, "explain": 2}}])
