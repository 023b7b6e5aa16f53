"""Full-rank evaluation on the device, through the C ABI: lgc_rank_positions against the numpy counting of
fullrank_support over lgc_score_rows' panel of the same padded tables, then the identities that tie it to
``recommend_topk``, then the library on top.

Everything is held exactly: the scores are claimed to be lgc_score_rows' chain and the order is strict, so ranks, tie
counts and candidate counts are compared as integers and values as bits (any NaN standing for any NaN)."""
import numpy as np
import pytest
import torch

import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, fullrank, propagate, synth
import fullrank_support as fs
import topk_support as ts

pytestmark = pytest.mark.gpu

NAN = float("nan")


def up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def padded(table, device, layout):
    """The table on the device with every float that must not be read a NaN.  "strided": rows dim + 3 floats apart from a
    base 4 bytes past a 16-byte line; "aligned": rows dim + 4 apart from an aligned base (dim % 4 == 0: the 16-byte loads)."""
    n, dim = table.shape
    if layout == "aligned":
        buf = torch.full((n, dim + 4), NAN, dtype=torch.float32, device=device)
        view = buf[:, :dim]
    else:
        buf = torch.full((n * (dim + 3) + 5,), NAN, dtype=torch.float32, device=device)
        view = buf[1:1 + n * (dim + 3)].view(n, dim + 3)[:, :dim]
        assert view.data_ptr() % 16 == 4
    view.copy_(up(table, device))
    return view


def rank_abi(users, items, pu, pi, seen=None, mode="zero", slices=0, outputs=(True, True, True)):
    """(rank, n_equal, n_cand, value, status word) of one lgc_rank_positions call as numpy (None for an output not asked
    for); outputs pre-filled with junk, one guard word behind the workspace."""
    lib, dev, n = _native.load(), users.device, pu.numel()
    rank = torch.full((n,), -77, dtype=torch.int32, device=dev)
    opt = [torch.full((n,), -77, dtype=torch.int32, device=dev) if outputs[0] else None,
           torch.full((n,), -77, dtype=torch.int32, device=dev) if outputs[1] else None,
           torch.full((n,), 77.0, dtype=torch.float32, device=dev) if outputs[2] else None]
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    need = lib.lgc_rank_positions_workspace_bytes(n, items.size(0), slices)
    assert need % 4 == 0
    ws = torch.full((need // 4 + 1,), -1, dtype=torch.int32, device=dev)
    ptr, entries = (None, None) if seen is None else seen
    code = lib.lgc_rank_positions(users.data_ptr(), users.stride(0), users.size(0), items.data_ptr(), items.stride(0),
                                  items.size(0), users.size(1), pu.data_ptr(), pi.data_ptr(), n, _native.ptr(ptr),
                                  _native.ptr(entries), fs.MODES.index(mode), slices, rank.data_ptr(), _native.ptr(opt[0]),
                                  _native.ptr(opt[1]), _native.ptr(opt[2]), ws.data_ptr(), need, status.data_ptr(),
                                  _native.stream_of(dev))
    assert code == 0
    assert int(ws[-1].item()) == -1                                                     # nothing written past the size
    host = [None if t is None else t.cpu().numpy() for t in [rank] + opt]
    return host[0], host[1], host[2], host[3], int(status[0].item())


def panel_of(users, items, pu):
    """The composed route's scores, one row per pair: lgc_score_rows on the same tables (a bad user is scored as user 0;
    the reference voids its row)."""
    out = propagate.score_rows(users, pu.clamp(0, users.size(0) - 1).contiguous(), items)
    lg.check_index_status(users.device)
    return out.cpu().numpy()


def same(got, want, what):
    for name, g, w in zip(("rank", "n_equal", "n_cand"), got[:3], want[:3]):
        assert np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:5].tolist(), g[g != w][:5].tolist(), w[g != w][:5].tolist())
    assert ts.values_match(got[3], want[3]), (what, "value")


def seen_of(ptr, entries, device):
    """The CSR on the device; an empty entry array still gets an address."""
    e = entries if entries.size else np.zeros(1, dtype=np.int64)
    return up(ptr, device), up(e, device)


# ---------------------------------------------------------------------------------------------------------------
# 1. the case table: every width, layout, catalogue size, pair count, slice count, list length and both modes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fs.CASE_NAMES)
def test_counts_equal_the_reference_on_every_path(device, name):
    case = fs.case(name)
    assert _native.load().lgc_dim_ok(case.dim), f"dim {case.dim} must be a width of this library"
    for kind in ("int", "float"):
        users_np, items_np, pu_np, pi_np, ptr, entries = case.build(kind)
        users, items = padded(users_np, device, case.layout), padded(items_np, device, case.layout)
        pu, pi = up(pu_np, device), up(pi_np, device)
        panel = panel_of(users, items, pu)
        lists = [entries[ptr[u]:ptr[u + 1]] for u in pu_np]
        seen = seen_of(ptr, entries, device)
        first = None
        for mode in fs.MODES:
            want = fs.ranks_ref(panel, pi_np, lists, mode)
            plain = fs.ranks_ref(panel, pi_np, None, mode)
            for slices in case.slices:
                got = rank_abi(users, items, pu, pi, seen, mode, slices)
                assert got[4] == 0
                same(got, want, (name, kind, mode, slices, "lists"))
                got = rank_abi(users, items, pu, pi, None, mode, slices)
                assert got[4] == 0
                same(got, plain, (name, kind, mode, slices, "no lists"))
                if first is None:
                    first = got
                for a, b in zip(got[:3], first[:3]):                                    # without lists the modes coincide
                    assert np.array_equal(a, b)
                assert np.array_equal(ts.bits_of(got[3]), ts.bits_of(first[3]))
            if kind == "int":
                assert (want[0] < 0).any() == (mode == "remove" and any(p in l for p, l in zip(pi_np, lists)))


def test_optional_outputs_may_be_null_and_two_runs_give_the_same_bytes(device):
    case = fs.case("d17")
    users_np, items_np, pu_np, pi_np, ptr, entries = case.build("float")
    users, items = padded(users_np, device, "strided"), padded(items_np, device, "strided")
    pu, pi, seen = up(pu_np, device), up(pi_np, device), seen_of(ptr, entries, device)
    for mode in fs.MODES:
        full = rank_abi(users, items, pu, pi, seen, mode, 2)
        again = rank_abi(users, items, pu, pi, seen, mode, 2)
        for a, b in zip(full[:3], again[:3]):
            assert np.array_equal(a, b)
        assert np.array_equal(ts.bits_of(full[3]), ts.bits_of(again[3]))
        for outputs in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
            got = rank_abi(users, items, pu, pi, seen, mode, 3, outputs)
            assert np.array_equal(got[0], full[0])
            for j, asked in enumerate(outputs):
                assert (got[1 + j] is None) == (not asked)
                if asked and j < 2:
                    assert np.array_equal(got[1 + j], full[1 + j])
                if asked and j == 2:
                    assert np.array_equal(ts.bits_of(got[3]), ts.bits_of(full[3]))


# ---------------------------------------------------------------------------------------------------------------
# 2. the order: ties on both sides of p and across a tile edge, zeros of both signs, NaN, +-inf, subnormal products
# ---------------------------------------------------------------------------------------------------------------
def special_tables():
    rng = np.random.default_rng(42)
    dim, n_items = 8, 2 * fs.ITEM_TILE + 44
    items = fs.f32(rng.integers(-2, 3, size=(n_items, dim)))
    items[120] = np.abs(items[120]) + 1                       # positive against user 0, negative against user 1
    items[100:141] = items[120]                               # 41 rows tie with p = 120, across the edge at 128
    items[250:260] = items[120]
    items[10], items[11] = 0.0, -0.0                          # rows of zeros of both signs
    items[20, 3], items[21, 0] = np.nan, ts.from_bits([0xFFC00001])[0]
    items[30, 1], items[31, 1], items[32] = np.inf, -np.inf, np.inf
    items[40:50] *= np.float32(2.0 ** -75)                    # subnormal products against user 3
    users = fs.f32(rng.integers(-2, 3, size=(6, dim)))
    users[0] = np.abs(users[0]) + 1                           # all positive: item 32 scores +inf, item 31 -inf
    users[1] = -users[0]
    users[2, 5] = np.nan                                      # a NaN threshold: every score of this user is a NaN
    users[3] = fs.f32(rng.integers(1, 4, size=dim)) * np.float32(2.0 ** -74)
    users[4] = 0.0
    # lists: user 0 has seen the +-inf items (NaN in mode zero), items with negative scores (-0) and ties of p
    lists = [np.array([5, 30, 31, 32, 100, 101, 120, 130, 255], dtype=np.int64), np.array([31, 32, 120], dtype=np.int64),
             np.array([1, 20], dtype=np.int64), np.arange(38, 52, dtype=np.int64), np.array([10, 11], dtype=np.int64),
             np.zeros(0, dtype=np.int64)]
    ptr = np.zeros(7, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    ps = [0, 10, 11, 20, 21, 30, 31, 32, 45, 99, 100, 119, 120, 121, 127, 128, 140, 141, 255, n_items - 1]
    pu = np.repeat(np.arange(6, dtype=np.int64), len(ps))
    pi = np.tile(np.array(ps, dtype=np.int64), 6)
    return users, items, pu, pi, ptr, np.concatenate(lists)


@pytest.mark.parametrize("mode", fs.MODES)
def test_ties_zeros_nan_and_inf_rank_as_in_mask_topk(device, mode):
    users_np, items_np, pu_np, pi_np, ptr, entries = special_tables()
    users, items = padded(users_np, device, "strided"), padded(items_np, device, "strided")
    pu, pi, seen = up(pu_np, device), up(pi_np, device), seen_of(ptr, entries, device)
    panel = panel_of(users, items, pu)
    lists = [entries[ptr[u]:ptr[u + 1]] for u in pu_np]
    want = fs.ranks_ref(panel, pi_np, lists, mode)
    # the premises: many ties with p on both sides of it, a NaN threshold, infinite and subnormal scores, -0 from the mask
    r = int(np.flatnonzero((pu_np == 5) & (pi_np == 120))[0])
    assert want[1][r] >= 50 and np.isnan(panel[np.flatnonzero(pu_np == 2)[0]]).all()
    assert np.isinf(panel[0]).sum() >= 3 and (np.abs(panel[np.flatnonzero(pu_np == 3)[0], 40:50]) < 2.0 ** -126).all()
    if mode == "zero":
        row = ts.masked_ref(panel[0], fs.seen_mask(lists[0], items_np.shape[0]))
        assert np.isnan(row[[30, 31, 32]]).all()
        r1 = int(np.flatnonzero(pu_np == 1)[0])
        assert ts.bits_of(ts.masked_ref(panel[r1], fs.seen_mask(lists[r1], items_np.shape[0])))[120] == 0x80000000
    for slices in (1, 2, 3):
        got = rank_abi(users, items, pu, pi, seen, mode, slices)
        assert got[4] == 0
        same(got, want, (mode, slices))
    got = rank_abi(users, items, pu, pi, None, mode, 0)
    same(got, fs.ranks_ref(panel, pi_np, None, mode), (mode, "no lists"))


def test_tables_of_zeros_and_one_user_against_every_item(device):
    n_items = 257
    z_users, z_items = padded(np.zeros((3, 5), dtype=np.float32), device, "strided"), padded(np.zeros((n_items, 5), dtype=np.float32), device, "strided")
    pi_np = np.arange(n_items, dtype=np.int64)
    pu, pi = up(np.full(n_items, 2, dtype=np.int64), device), up(pi_np, device)
    for slices in (0, 1, 3):
        rank, n_equal, n_cand, value, status = rank_abi(z_users, z_items, pu, pi, None, "zero", slices)
        assert status == 0 and np.array_equal(rank, pi_np) and (n_equal == n_items - 1).all() and (n_cand == n_items).all()
        assert (ts.bits_of(value) == 0).all()
    rng = np.random.default_rng(7)
    items_np = fs.f32(rng.standard_normal((n_items, 24)))
    items_np[rng.permutation(n_items)[:60]] = items_np[:60]                              # equal scores among them
    users, items = padded(fs.f32(rng.standard_normal((3, 24))), device, "aligned"), padded(items_np, device, "aligned")
    for slices in (0, 2):
        rank, n_equal, _, _, _ = rank_abi(users, items, pu, pi, None, "remove", slices)
        assert sorted(rank.tolist()) == list(range(n_items)) and n_equal.max() >= 1      # a permutation of 0 .. 256


# ---------------------------------------------------------------------------------------------------------------
# 3. pairs outside the tables
# ---------------------------------------------------------------------------------------------------------------
def test_bad_pairs_are_flagged_voided_and_leave_their_neighbours_alone(device):
    case = fs.case("d90")
    users_np, items_np, pu_np, pi_np, ptr, entries = case.build("float")
    users, items = padded(users_np, device, "strided"), padded(items_np, device, "strided")
    seen = seen_of(ptr, entries, device)
    bad_u, bad_i = pu_np.copy(), pi_np.copy()
    rows = [0, 17, 63, 64, 129]
    bad_u[[0, 63]] = [case.n_users, -1]
    bad_i[[17, 64]] = [case.n_items, -2 ** 40]
    bad_u[129], bad_i[129] = 2 ** 40, -1
    valid = np.ones(case.n_pairs, dtype=bool)
    valid[rows] = False
    lists = [entries[ptr[u]:ptr[u + 1]] if ok else None for u, ok in zip(bad_u, valid)]
    panel = panel_of(users, items, up(np.where(valid, bad_u, 0), device))
    for mode in fs.MODES:
        for slices in (1, 3):
            got = rank_abi(users, items, up(bad_u, device), up(bad_i, device), seen, mode, slices)
            assert got[4] & _native.ST_INDEX_OOB
            same(got, fs.ranks_ref(panel, np.where(valid, bad_i, 0), lists, mode, valid), (mode, slices))
            assert (got[0][rows] == -1).all() and (got[1][rows] == -1).all() and (got[2][rows] == 0).all() and (ts.bits_of(got[3][rows]) == 0).all()
            clean = rank_abi(users, items, up(pu_np, device), up(pi_np, device), seen, mode, slices)
            assert clean[4] == 0
            for a, b in zip(got[:4], clean[:4]):
                assert np.array_equal(ts.bits_of(a[valid]) if a.dtype == np.float32 else a[valid],
                                      ts.bits_of(b[valid]) if b.dtype == np.float32 else b[valid])
    # through the library the status word raises
    lg.check_index_status(device)
    out = fullrank.positive_ranks(users, items, up(bad_u, device), up(bad_i, device))
    with pytest.raises(IndexError):
        lg.check_index_status(device)
    assert out.rank[17].item() == -1 and out.n_cand[17].item() == 0
    lg.check_index_status(device)                                                       # cleared


# ---------------------------------------------------------------------------------------------------------------
# 4. the identity with recommend_topk: rank is the column of p
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5", "d64_vec", "d90"])
def test_rank_is_the_column_of_p_in_recommend_topk(device, name):
    case = fs.case(name)
    users_np, items_np, pu_np, pi_np, ptr, entries = case.build("float")
    items_np[case.n_items // 2:] = items_np[:case.n_items - case.n_items // 2]           # ties between the halves
    users, items = padded(users_np, device, case.layout), padded(items_np, device, case.layout)
    pu, pi = up(pu_np, device), up(pi_np, device)
    seen = propagate.SeenLists(up(ptr, device), up(entries, device))
    k = min(256, case.n_items)
    for lists in (seen, None):
        out = fullrank.positive_ranks(users, items, pu, pi, lists, "zero")
        index, value = propagate.recommend_topk(users, pu, items, lists, k, return_values=True)
        lg.check_index_status(device)
        rank, got_v = out.rank.cpu().numpy(), out.value.cpu().numpy()
        index, value = index.cpu().numpy(), value.cpu().numpy()
        assert (rank >= 0).all() and (rank < k).any()
        for r in range(case.n_pairs):
            if rank[r] < k:
                assert index[r, rank[r]] == pi_np[r], (name, r)
                assert ts.values_match(got_v[r:r + 1] + np.float32(0.0), value[r, rank[r]:rank[r] + 1] + np.float32(0.0))
            else:
                assert pi_np[r] not in index[r]


# ---------------------------------------------------------------------------------------------------------------
# 5. through the library
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(device):
    g = synth.make_bipartite(120, 2 * fs.ITEM_TILE + 85, 1500, seed=9)
    ei, ew = g.coo()
    dim = 24
    model = lg.LightGCN(g.num_nodes, dim, 2)
    model.load_state_dict({"alpha": model.alpha, "embedding.weight": synth.xavier_table(g.num_nodes, dim, 3)})
    model.to(device)
    ei, ew = ei.to(device), ew.to(device)
    rng = np.random.default_rng(11)
    ids = rng.permutation(g.n_users)[:70].astype(np.int64)
    seen_lists = [np.sort(rng.permutation(g.n_items)[:rng.integers(0, 40)]).astype(np.int64) for _ in range(g.n_users)]
    seen_lists[ids[3]] = np.array([1, 5, 300], dtype=np.int64)
    ptr = np.zeros(g.n_users + 1, dtype=np.int64)
    np.cumsum([len(x) for x in seen_lists], out=ptr[1:])
    seen = propagate.SeenLists(up(ptr, device), up(np.concatenate(seen_lists), device))
    pos = []
    for j, u in enumerate(ids):
        lst = rng.integers(0, g.n_items, size=rng.integers(1, 6)).tolist()
        if j % 4 == 0:
            lst += lst[:1]                                                              # a duplicate in the positive list
        if j % 5 == 0 and len(seen_lists[u]):
            lst.append(int(seen_lists[u][0]))                                           # a positive that is seen
        pos.append(lst)
    pos[3] = [1, 300]                                                                   # every positive seen: no rank in "remove"
    positives = propagate.PositiveLists.from_lists(ids.tolist(), pos, g.n_users, device)
    return g, model, ei, ew, seen, seen_lists, ids, pos, positives


@pytest.mark.parametrize("mode", fs.MODES)
def test_evaluate_full_rank_equals_the_reference_metrics(device, served, mode):
    g, model, ei, ew, seen, seen_lists, ids, pos, positives = served
    ks = (5, 20, 300)                                                                   # 300 > TOPK_MAX
    res = model.evaluate_full_rank(ei, ew, g.n_users, g.n_items, seen, up(ids, device), positives, ks, mode)
    with torch.no_grad():
        table = model._serving_embedding(ei, ew)
    users_t, items_t = table[:g.n_users], table[g.n_users:]
    # the reference's pairs: the distinct items of every listed user, by position and then by item
    owner = np.concatenate([[j] * len(set(p)) for j, p in enumerate(pos)]).astype(np.int64)
    pair_items = np.concatenate([sorted(set(p)) for p in pos]).astype(np.int64)
    assert np.array_equal(res.pair_owner.cpu().numpy(), owner) and np.array_equal(res.pair_items.cpu().numpy(), pair_items)
    assert np.array_equal(res.pair_users.cpu().numpy(), ids[owner])
    panel = panel_of(users_t, items_t, up(ids[owner], device))
    want = fs.ranks_ref(panel, pair_items, [seen_lists[u] for u in ids[owner]], mode)
    same([t.cpu().numpy() for t in res.pairs], want, mode)
    lengths = [len(p) for p in pos]
    auc, mpr, rr, recall, hit = fs.metrics_ref(want[0], want[2], owner, lengths, ks)
    for name, got, ref in (("auc", res.auc, auc), ("mpr", res.mpr, mpr), ("rr", res.rr, rr), ("recall", res.recall, recall), ("hit", res.hit, hit)):
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), name
    if mode == "remove":
        assert np.isnan(auc[3]) and rr[3] == 0.0 and (want[0] < 0).sum() >= 3
    assert abs(res.mean["auc"] - np.nanmean(auc)) < 1e-12 and abs(res.mean["mpr"] - np.nanmean(mpr)) < 1e-12
    assert abs(res.mean["mrr"] - rr.mean()) < 1e-12 and 0.0 <= res.mean["auc"] <= 1.0
    if mode == "zero":                                                                  # the bits of evaluate_metrics
        base = model.evaluate_metrics(ei, ew, g.n_users, g.n_items, seen, up(ids, device), positives, ks=(5, 20), coverage=False)
        assert res.mean["recall"][:2] == base.mean["recall"] and res.mean["hit_rate"][:2] == base.mean["hit_rate"]
        assert torch.equal(res.recall[:, :2], base.metrics[:, :, _native.RM_RECALL])
        assert torch.equal(res.hit[:, :2], base.metrics[:, :, _native.RM_HIT])
    assert res.mean["recall"][2] >= res.mean["recall"][1] >= res.mean["recall"][0]
    lg.check_index_status(device)


def test_equal_length_user_sets_on_one_positive_lists_get_their_own_pairs(device, served):
    """Two different user chunks of the same length, one after the other on the same ``PositiveLists``, with each id tensor
    freed before the next is made (the allocator may hand its block out again): every chunk's rows are the rows the whole
    set gets, which the test above holds to the reference."""
    g, model, ei, ew, seen, seen_lists, ids, pos, positives = served
    args = (ei, ew, g.n_users, g.n_items, seen)
    whole = model.evaluate_full_rank(*args, up(ids, device), positives, (5, 20), "zero")
    half = len(ids) // 2
    assert not np.array_equal(np.sort(ids[:half]), np.sort(ids[half:2 * half]))
    for _ in range(2):
        for lo in (0, half):
            part = model.evaluate_full_rank(*args, up(ids[lo:lo + half], device), positives, (5, 20), "zero")
            rows = (whole.pair_owner >= lo) & (whole.pair_owner < lo + half)
            assert torch.equal(part.pair_users, whole.pair_users[rows]) and torch.equal(part.pair_items, whole.pair_items[rows])
            assert torch.equal(part.pair_owner, whole.pair_owner[rows] - lo)
            assert torch.equal(part.pairs.rank, whole.pairs.rank[rows]) and torch.equal(part.pairs.n_cand, whole.pairs.n_cand[rows])
            for name in ("auc", "mpr", "rr", "recall", "hit"):
                got, want = getattr(part, name), getattr(whole, name)[lo:lo + half]
                assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (lo, name)
            del part
    lg.check_index_status(device)
