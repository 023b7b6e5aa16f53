"""The epoch evaluation on the device: score panels (lgc_score_rows), ranking through them (recommend_topk), hits and
metric sums (evaluateK).  References are fp64 on the same fp32 rows; every input is torch.randn with a fixed seed."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate
from gnn_ecommerce_amd.propagate import PositiveLists, SeenLists, panel_rows, recommend_topk, score_rows
from tests_support import assert_topk_exact_up_to_ties, hub_inputs

pytestmark = pytest.mark.gpu

TIE_CAP = 1e-3          # positions excused as ties, as a fraction of a case's positions


def padded(values: torch.Tensor, stride: int, device) -> torch.Tensor:
    """``values`` as the leading columns of a [rows, stride] buffer whose other columns are NaN."""
    buf = torch.full((values.size(0), stride), float("nan"), device=device)
    buf[:, :values.size(1)] = values.to(device)
    return buf[:, :values.size(1)]


def randn_tables(seed, n_users, n_items, dim):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n_users, dim, generator=gen), torch.randn(n_items, dim, generator=gen)


def shuffled_ids(seed, n_rows, n_users):
    """Row ids in no order, with repeats (and, from 2 rows on, at least one repeat)."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(n_users, (n_rows,), generator=gen)
    if n_rows > 1:
        ids[-1] = ids[0]
    return ids


# ---------------------------------------------------------------------------------------------------------------
# 1. scores
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,stride", [(1, 1), (3, 8), (64, 64), (90, 96), (130, 135), (256, 260)])
def test_scores_against_fp64_within_the_running_sum_bound(device, dim, stride):
    """|s - s64| <= dim * 2^-24 * sum_d |u_d i_d| per element (a chain of dim roundings, each at most half an ulp of a
    partial sum that |u|.|i| bounds), at every (n_rows, n_items) of the grid; NaN in the padding columns of both tables
    stays out."""
    n_users = 50
    for n_items in (1, 255, 1025):
        u, it = randn_tables(1000 * dim + n_items, n_users, n_items, dim)
        ud, itd = padded(u, stride, device), padded(it, stride, device)
        assert ud.stride(0) == stride and itd.stride(0) == stride
        for n_rows in (1, 17, 300):
            ids = shuffled_ids(n_rows, n_rows, n_users)
            got = score_rows(ud, ids.to(device), itd)
            assert got.shape == (n_rows, n_items) and got.dtype == torch.float32
            rows = u[ids].to(device).double()
            ref = rows @ it.to(device).double().t()
            bound = dim * 2.0 ** -24 * (rows.abs() @ it.to(device).double().abs().t())
            err = (got.double() - ref).abs()
            assert not torch.isnan(got).any()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f"dim {dim} items {n_items} rows {n_rows}: worst error / bound = {worst:.3g}")
            assert bool((err <= bound).all()), (dim, n_items, n_rows, worst)
    # row_ids = None: every user row in order; out= is written in place, also with a wider row stride
    wide = torch.full((n_users, n_items + 3), 7.0, device=device)
    out = score_rows(ud, None, itd, out=wide[:, :n_items])
    assert out.data_ptr() == wide.data_ptr() and bool((wide[:, n_items:] == 7.0).all())
    assert torch.equal(out, score_rows(ud, torch.arange(n_users, device=device), itd))


def test_out_of_range_row_id_flags_zero_fills_and_spares_its_neighbours(device):
    dim, n_users, n_items = 90, 40, 300
    u, it = randn_tables(5, n_users, n_items, dim)
    ud, itd = padded(u, 96, device), padded(it, 96, device)
    ids = shuffled_ids(9, 70, n_users)
    clean = score_rows(ud, ids.to(device), itd)
    lg.check_index_status(device)                                   # nothing pending
    bad = ids.clone()
    bad[3], bad[64], bad[69] = n_users, -1, 2 ** 40
    got = score_rows(ud, bad.to(device), itd)
    assert int(propagate._status(device)[0].item()) & _native.ST_INDEX_OOB
    with pytest.raises(IndexError):
        lg.check_index_status(device)                               # reports and clears
    lg.check_index_status(device)
    hit = torch.zeros(70, dtype=torch.bool)
    hit[[3, 64, 69]] = True
    assert bool((got[hit.to(device)] == 0).all())
    assert torch.equal(got[~hit.to(device)], clean[~hit.to(device)])


# ---------------------------------------------------------------------------------------------------------------
# 2. position independence, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [90, 130, 3])
def test_a_score_has_the_same_bits_wherever_it_is_computed(device, dim):
    n_users, n_items, n_rows = 120, 1025, 300
    u, it = randn_tables(dim, n_users, n_items, dim)
    ids = shuffled_ids(dim, n_rows, n_users)
    ud, itd = u.to(device), it.to(device)                           # dense rows: stride = dim
    base = score_rows(ud, ids.to(device), itd)
    # one row at a time (first, one inside, last of a tile, last)
    for r in (0, 63, 64, 299):
        assert torch.equal(score_rows(ud, ids[r:r + 1].to(device), itd)[0], base[r])
    # another row, another column, other strides: rows reversed, items permuted, both tables padded with NaN
    perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(1))
    stride = (dim + 31) // 32 * 32 + 32
    moved = score_rows(padded(u, stride, device), ids.flip(0).to(device), padded(it[perm], stride, device))
    assert torch.equal(moved.flip(0), base[:, perm.to(device)])
    # other n_rows / n_items: a sub-panel of fewer rows against a prefix of the items, written into a wider buffer
    wide = torch.empty((17, 300), device=device)
    sub = score_rows(ud, ids[40:57].to(device), itd[:255], out=wide[:, :255])
    assert torch.equal(sub, base[40:57, :255])


@pytest.mark.parametrize("dim", [90, 64])
def test_panel_size_is_invisible_in_recommend_topk(device, dim):
    n_users, n_items, n_sel, k = 80, 1025, 37, 20
    u, it = randn_tables(70 + dim, n_users, n_items, dim)
    ud, itd = padded(u, 96, device), it.to(device)
    sel = shuffled_ids(4, n_sel, n_users)
    per_user = (torch.rand(n_users, n_items, generator=torch.Generator().manual_seed(2)) < 0.02).float()
    mask = per_user[sel]                                            # repeated users: the same row each time
    assert len(set(sel.tolist())) < n_sel
    seen = SeenLists.from_dense(mask, sel.tolist(), n_users, device=device)
    full = score_rows(ud, sel.to(device), itd)
    masked = torch.where(mask.to(device) != 0, full * 0.0, full)
    want_i, want_v = None, None
    for rows in (1, n_sel, n_sel - 1, n_sel + 1, 5):
        ws = 4 * n_items * rows + 3                                 # not a whole number of rows either
        assert panel_rows(n_items, ws) == rows
        idx, val = recommend_topk(ud, sel.to(device), itd, seen, k, workspace_bytes=ws, return_values=True)
        assert idx.shape == (n_sel, k) and idx.dtype == torch.int64 and val.dtype == torch.float32
        if want_i is None:
            want_i, want_v = idx, val
            assert torch.equal(val, torch.gather(masked, 1, idx))   # the values are the panel's scores, masked
            assert torch.equal(val, masked.topk(k, dim=1).values)
        assert torch.equal(idx, want_i) and torch.equal(val, want_v), rows
    assert torch.equal(recommend_topk(ud, sel.to(device), itd, seen, k), want_i)        # the default workspace
    none = recommend_topk(ud, sel.to(device), itd, None, k, workspace_bytes=4 * n_items * 7)
    assert torch.equal(torch.gather(full, 1, none), full.topk(k, dim=1).values)         # no mask: mode 0
    with pytest.raises(ValueError, match="k <= 256"):
        recommend_topk(ud, sel.to(device), itd, seen, 257)
    assert recommend_topk(ud, sel[:0].to(device), itd, seen, k).shape == (0, k)


# ---------------------------------------------------------------------------------------------------------------
# 3. ranking
# ---------------------------------------------------------------------------------------------------------------
def ranking_case(device, rows, n_items, dim, k, seed=7):
    """(got, want, fp64 masked scores) of one case: 2 % seen, one user without seen items, one with every item seen."""
    n_users = rows + 9
    u, it = randn_tables(seed, n_users, n_items, dim)
    sel = torch.randperm(n_users, generator=torch.Generator().manual_seed(seed))[:rows]
    mask = (torch.rand(rows, n_items, generator=torch.Generator().manual_seed(seed + 1)) < 0.02).float()
    mask[1] = 0.0
    mask[2] = 1.0
    seen = SeenLists.from_dense(mask, sel.tolist(), n_users, device=device).validate(n_users)
    stride = 96 if dim == 90 else dim
    got = recommend_topk(padded(u, stride, device), sel.to(device), padded(it, stride, device), seen, k,
                         workspace_bytes=4 * n_items * 24)                            # several panels, the last one short
    ref = (u[sel].to(device).double() @ it.to(device).double().t()) * (1.0 - mask.to(device).double())
    want = torch.sort(-ref, dim=1, stable=True).indices[:, :k]                        # value descending, index ascending
    return got.cpu(), want.cpu(), ref.cpu()


@pytest.mark.parametrize("rows,n_items,dim,k", [(64, 65537, 90, 20), (64, 65537, 8, 20), (300, 1025, 64, 256),
                                                (40, 255, 3, 255)])
def test_ranking_against_topk_of_fp64_masked_scores(device, rows, n_items, dim, k):
    got, want, ref = ranking_case(device, rows, n_items, dim, k)
    assert got[2].tolist() == list(range(k))                        # everything seen: a flat row, ranked by index
    ties = assert_topk_exact_up_to_ties(got.numpy(), want.numpy(), ref.numpy())
    print(f"{rows} x {n_items}, dim {dim}, k {k}: {ties} of {rows * k} positions excused as ties")
    assert ties <= TIE_CAP * rows * k


# ---------------------------------------------------------------------------------------------------------------
# 4. consistency with recommendK
# ---------------------------------------------------------------------------------------------------------------
def hub_model(device, n_users, n_items, dim, layers=3):
    ei, ew, _ = hub_inputs(3, n_users, n_items, dim)
    model = lg.LightGCN(n_users + n_items, dim, layers).to(device).eval()
    with torch.no_grad():
        model.embedding.weight.copy_(0.1 * torch.randn(n_users + n_items, dim, generator=torch.Generator().manual_seed(11)))
    return model, ei.to(device), ew.to(device)


def purchase_lists(seed, n_users, n_items, per_user, device):
    """SeenLists of ``per_user`` random items for every user (sorted, distinct)."""
    gen = torch.Generator().manual_seed(seed)
    items = torch.stack([torch.randperm(n_items, generator=gen)[:per_user].sort().values for _ in range(n_users)])
    ptr = torch.arange(n_users + 1) * per_user
    return SeenLists(ptr.to(device), items.reshape(-1).contiguous().to(device)).validate(n_users)


def test_recommend_topk_agrees_with_recommendk(device):
    n_users, n_items, dim, k = 3000, 500, 90, 20
    model, ei, ew = hub_model(device, n_users, n_items, dim)
    seen = purchase_lists(5, n_users, n_items, 10, device)
    users = torch.randperm(n_users, generator=torch.Generator().manual_seed(6))[:700].tolist()
    with torch.no_grad():
        frame = model.recommendK(ei, ew, n_users, n_items, seen, users, k)
        got = model.recommend_topk(ei, ew, n_users, n_items, seen, users, k, workspace_bytes=4 * n_items * 100)
        emb = model.get_embedding(ei, ew)
    assert got.is_cuda and got.shape == (len(users), k)
    ue, ie = torch.split(emb.double(), [n_users, n_items])
    ref = ue[users] @ ie.t() * (1.0 - seen.to_dense(users, n_items).to(device).double())
    ties = assert_topk_exact_up_to_ties(got.cpu().numpy(), np.array(frame["top_rlvnt_itm"].tolist()), ref.cpu().numpy())
    print(f"recommend_topk vs recommendK: {ties} of {len(users) * k} positions excused as ties")
    assert ties <= TIE_CAP * len(users) * k


# ---------------------------------------------------------------------------------------------------------------
# 5. metrics
# ---------------------------------------------------------------------------------------------------------------
def test_evaluatek_is_mark_mapk_on_the_device_topk(device):
    import pandas as pd
    n_users, n_items, dim, k = 600, 300, 64, 20
    model, ei, ew = hub_model(device, n_users, n_items, dim, layers=2)
    seen = purchase_lists(8, n_users, n_items, 6, device)
    gen = torch.Generator().manual_seed(9)
    listed = torch.randperm(n_users, generator=gen)[:250].tolist()
    lists = [torch.randint(n_items, (int(torch.randint(1, 40, (1,), generator=gen)),), generator=gen).tolist() for _ in listed]
    lists[0] = lists[0] + lists[0][:1]                              # a duplicated positive
    listed.append(listed[5])                                        # a user listed twice
    lists.append(lists[5])
    pos_df = pd.DataFrame({"user_id_idx": listed, "item_id_idx_list": lists})
    positives = PositiveLists.from_frame(pos_df, n_users, device=device).validate(n_users, n_items)
    with torch.no_grad():
        precision, recall, hits = model.evaluateK(ei, ew, n_users, n_items, seen, listed, positives, k,
                                                  workspace_bytes=4 * n_items * 64)
        again = model.evaluateK(ei, ew, n_users, n_items, seen, None, pos_df, k)         # a frame, its own users, other panels
        top = model.recommend_topk(ei, ew, n_users, n_items, seen, listed[:-1], k)
    assert isinstance(precision, float) and isinstance(recall, float)
    assert hits.is_cuda and hits.dtype == torch.int32 and hits.shape == (len(listed),)
    top_df = pd.DataFrame({"user_ID": listed[:-1], "top_rlvnt_itm": top.cpu().numpy().tolist()})
    want_p, want_r, frame = model.MARK_MAPK(pos_df, top_df, k)
    assert len(frame) == len(listed)
    assert hits.cpu().tolist() == [len(o) for o in frame["overlap_item"]] and hits.sum().item() > 0
    print(f"precision {precision!r} vs {want_p!r}; recall {recall!r} vs {want_r!r}")
    assert abs(precision - want_p) <= 1e-12 and abs(recall - want_r) <= 1e-12
    assert again[0] == precision and again[1] == recall and torch.equal(again[2], hits)   # the same bits on every run
    lg.check_index_status(device)


def test_evaluatek_reports_a_user_outside_the_table(device):
    n_users, n_items = 200, 100
    model, ei, ew = hub_model(device, n_users, n_items, 64, layers=1)
    positives = PositiveLists.from_lists([3, 7], [[1, 2], [5]], n_users, device=device)
    with torch.no_grad(), pytest.raises(IndexError):
        model.evaluateK(ei, ew, n_users, n_items, None, [3, n_users + 4], positives, 5)
    lg.check_index_status(device)                                   # cleared


# ---------------------------------------------------------------------------------------------------------------
# 6. memory
# ---------------------------------------------------------------------------------------------------------------
def test_evaluatek_memory_is_bounded_by_the_workspace(device):
    n_users, n_items, dim, k, n_sel, ws = 2500, 20000, 64, 20, 2000, 4 << 20
    gen = torch.Generator().manual_seed(12)
    eu, ei_ = torch.randint(n_users, (30000,), generator=gen), torch.randint(n_items, (30000,), generator=gen) + n_users
    ei = torch.stack((torch.cat([eu, ei_]), torch.cat([ei_, eu]))).to(device)
    model = lg.LightGCN(n_users + n_items, dim, 2).to(device).eval()
    users = torch.randperm(n_users, generator=gen)[:n_sel]
    seen = purchase_lists(13, n_users, n_items, 8, device)
    positives = PositiveLists.from_lists(users.tolist(), torch.randint(n_items, (n_sel, 5), generator=gen).tolist(), n_users,
                                         device=device).validate(n_users, n_items)
    users_d = users.to(device)
    with torch.no_grad():
        model.evaluateK(ei, None, n_users, n_items, seen, users_d[:3], positives, k, workspace_bytes=ws)   # graph, table, status
        propagate._score_workspaces.clear()                          # ... but the panel is allocated inside the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(device)
        before = torch.cuda.memory_allocated(device)
        precision, recall, hits = model.evaluateK(ei, None, n_users, n_items, seen, users_d, positives, k, workspace_bytes=ws)
        rise = torch.cuda.max_memory_allocated(device) - before
    bound = ws + n_sel * k * 8 + n_sel * 12 + (1 << 20)
    print(f"rise {rise} bytes, bound {bound}; a dense score matrix would be {4 * n_sel * n_items}")
    assert rise <= bound
    assert 0.0 <= precision <= 1.0 and 0.0 <= recall <= 1.0 and hits.shape == (n_sel,)
    # the reference's dense mask: converted once, then found again by identity + version
    few = users[:200]
    dense = seen.to_dense(few.tolist(), n_items)
    sub = PositiveLists.from_arrays(positives.ptr, positives.items, few, device=device)
    builds = SeenLists.dense_builds
    with torch.no_grad():
        first = model.evaluateK(ei, None, n_users, n_items, dense, few.tolist(), sub, k, workspace_bytes=ws)
        second = model.evaluateK(ei, None, n_users, n_items, dense, few.tolist(), sub, k, workspace_bytes=ws)
    assert SeenLists.dense_builds == builds + 1
    assert first[:2] == second[:2] and torch.equal(first[2], second[2]) and torch.equal(first[2], hits[:200])


# ---------------------------------------------------------------------------------------------------------------
# 7. end to end on the demo's data
# ---------------------------------------------------------------------------------------------------------------
def test_evaluatek_reproduces_the_demo_loop_metrics(device):
    """tools/train_demo.py's data at 6,000 x 800 and its evaluation lines (recommendK with the dense mask, then
    MARK_MAPK) against evaluateK on the same model."""
    import pandas as pd
    spec = importlib.util.spec_from_file_location("train_demo", os.path.join(ROOT, "tools", "train_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    n_users, n_items, dim, k = 6000, 800, 64, 20
    u, i = demo.latent_interactions(n_users, n_items, 12, 0)
    held = np.random.default_rng(1).random(len(u)) < 0.15
    test = pd.DataFrame({"user_id_idx": u[held], "item_id_idx": i[held]})
    test_pos = test.groupby("user_id_idx")["item_id_idx"].apply(list).reset_index()
    test_pos.columns = ["user_id_idx", "item_id_idx_list"]
    test_pos = test_pos.iloc[:2000]
    u_t, i_t = torch.from_numpy(u[~held]), torch.from_numpy(i[~held] + n_users)
    edge_index = torch.stack((torch.cat([u_t, i_t]), torch.cat([i_t, u_t]))).to(device)
    edge_weight = torch.ones(edge_index.size(1), device=device)
    users = list(test_pos["user_id_idx"])
    row_of = {uu: r for r, uu in enumerate(users)}
    seen = torch.zeros(len(users), n_items)
    keep = np.isin(u[~held], users)
    seen[[row_of[uu] for uu in u[~held][keep]], i[~held][keep]] = 1.0
    model = lg.LightGCN(n_users + n_items, dim, 3).to(device).eval()
    with torch.no_grad():
        model.embedding.weight.copy_(0.1 * torch.randn(n_users + n_items, dim, generator=torch.Generator().manual_seed(2)))
    version = model.embedding.weight._version
    with torch.no_grad():
        top_df = model.recommendK(edge_index, edge_weight, n_users, n_items, seen, users, k)
        want_p, want_r, frame = model.MARK_MAPK(test_pos, top_df, k)
        precision, recall, hits = model.evaluateK(edge_index, edge_weight, n_users, n_items, seen, users, test_pos, k)
        got = model.recommend_topk(edge_index, edge_weight, n_users, n_items, seen, users, k).cpu()
        emb = model.get_embedding(edge_index, edge_weight)
    assert model.embedding.weight._version == version
    ue, ie = torch.split(emb.double(), [n_users, n_items])
    ref = (ue[users] @ ie.t() * (1.0 - seen.to(device).double())).cpu().numpy()
    ties = assert_topk_exact_up_to_ties(got.numpy(), np.array(top_df["top_rlvnt_itm"].tolist()), ref)
    print(f"demo data: {ties} of {len(users) * k} positions excused as ties; P {precision!r} / {want_p!r}, R {recall!r} / {want_r!r}")
    assert ties <= TIE_CAP * len(users) * k
    own_p, own_r, own = model.MARK_MAPK(test_pos, pd.DataFrame({"user_ID": users, "top_rlvnt_itm": got.numpy().tolist()}), k)
    assert hits.cpu().tolist() == [len(o) for o in own["overlap_item"]]
    assert abs(precision - own_p) <= 1e-12 and abs(recall - own_r) <= 1e-12
    if ties == 0:                                                    # the two routes ranked alike: the demo's own numbers
        assert abs(precision - want_p) <= 1e-12 and abs(recall - want_r) <= 1e-12
        assert hits.cpu().tolist() == [len(o) for o in frame["overlap_item"]]
