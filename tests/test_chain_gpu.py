"""The score chain and the MFMA tile against the exact host reference of tests/chain_support.py.

Every other suite holds the holders of "lgc_score_rows' chain, with its bits" to lgc_score_rows on the same device; here
lgc_score_rows itself, lgc_row_rnorm and each holder are held to ``chain32`` / ``rnorm32`` computed on the host, at every
width of ``chain_support.WIDTHS``, on data that tells a wrong summation order apart (tests/test_chain_host.py proves that it
does).  Nothing is compared within a tolerance: scores as bits, ranks and indices as integers.

Two places follow include/lgconv_hip.h where it promises less than raw bits.  The chain runs over d = 0 .. round_up(dim, 4)
- 1 with zeros past dim (``chain32`` does the same), so at dim % 4 != 0 a sum of -0 is +0.  And the MFMA kernels pad the
width with zeros to 16 columns and may give +0 for a sum of -0: lgc_item_neighbors' values (which it returns folded anyway)
are compared under ``same_folded``; lgc_rank_positions' ``value`` is the chain's own and is compared raw."""
import numpy as np
import pytest
import torch

import chain_support as cs
import fullrank_support as fs
import hardneg_support as hs
import rerank_support as rs
import sampler_support as sp
import similar_support as ss

from gnn_ecommerce_amd import _native

pytestmark = pytest.mark.gpu

N_ROWS, N_ITEMS = cs.N_ROWS, cs.N_ITEMS


def accepted(widths):
    """The widths lgc_dim_ok takes; without the library every width stays and the tests fail at their first call."""
    try:
        lib = _native.load()
    except _native.NativeLibraryError:
        return list(widths)
    return [d for d in widths if lib.lgc_dim_ok(d)]


WIDTHS, CLASS_WIDTHS = accepted(cs.WIDTHS), accepted(cs.CLASS_WIDTHS)


def up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class Table:
    """A table on the device in one of ``chain_support.LAYOUTS``: ``t`` is the [rows, dim] view of the flat buffer."""

    def __init__(self, table, layout, device):
        flat, off, stride = cs.laid_out(table, layout)
        self.buf = up(flat, device)
        rows, dim = table.shape
        self.t = self.buf[off:off + rows * stride].view(rows, stride)[:, :dim]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * off and self.t.stride(0) == stride
        self.ptr, self.stride, self.rows, self.dim = self.t.data_ptr(), stride, rows, dim


class World:
    def __init__(self, device, dim, kind, layout):
        users, items = cs.tables(kind, dim)
        self.dim, self.kind, self.layout, self.device = dim, kind, layout, device
        self.users, self.items = Table(users, layout, device), Table(items, layout, device)


_worlds = {}


def world(device, dim, kind, layout):
    """The device copy of (width, data kind, layout), made once and left unchanged; the host panels are chain_support's."""
    key = (dim, kind, layout)
    if key not in _worlds:
        _worlds[key] = World(device, dim, kind, layout)
    return _worlds[key]


def lib_and_stream(device):
    return _native.load(), _native.stream_of(device)


# ---------------------------------------------------------------------------------------------------------------
# 1. lgc_score_rows: the root of the bit contract
# ---------------------------------------------------------------------------------------------------------------
GUARD = -7.25
SCORE_COMBOS = [(k, l) for k in ("permuted", "random", "wide") for l in cs.LAYOUTS] + [("specials", "dense")]


def score_rows_abi(w, ids):
    lib, stream = lib_and_stream(w.device)
    n = N_ROWS if ids is None else ids.numel()
    out = torch.full((n + 1, N_ITEMS + 3), GUARD, device=w.device)
    status = torch.zeros(1, dtype=torch.int32, device=w.device)
    code = lib.lgc_score_rows(w.users.ptr, w.users.stride, w.users.rows, _native.ptr(ids), n, w.items.ptr, w.items.stride,
                              N_ITEMS, w.dim, out.data_ptr(), N_ITEMS + 3, status.data_ptr(), stream)
    assert code == 0 and int(status.item()) == 0
    got = out.cpu().numpy()
    assert (got[n] == GUARD).all() and (got[:, N_ITEMS:] == GUARD).all()               # nothing written around the panel
    return got[:n, :N_ITEMS]


def first_difference(got, want):
    bad = np.argwhere(~((np.isnan(got) & np.isnan(want)) | (got.view(np.uint32) == want.view(np.uint32))))
    if not len(bad):
        return None
    r, c = bad[0]
    return len(bad), int(r), int(c), hex(int(got.view(np.uint32)[r, c])), hex(int(want.view(np.uint32)[r, c]))


@pytest.mark.parametrize("dim", WIDTHS)
def test_score_rows_is_the_host_chain_bit_for_bit(device, dim):
    """Raw bits: a -0 stays -0 (at dim % 4 == 0; otherwise the header's padded steps make it +0, as ``chain32`` does)."""
    shuffled = np.random.default_rng([1, dim]).permutation(N_ROWS).astype(np.int64)
    for kind, layout in SCORE_COMBOS:
        w = world(device, dim, kind, layout)
        want = cs.panel(kind, dim)
        for ids in (None, shuffled):
            got = score_rows_abi(w, None if ids is None else up(ids, device))
            ref = want if ids is None else want[ids]
            assert cs.same_bits(got, ref), (dim, kind, layout, ids is not None, first_difference(got, ref))
    if dim % 4 == 0:                                         # the premise: the wide data does produce sums of -0
        assert np.signbit(cs.panel("wide", dim)[cs.panel("wide", dim) == 0]).any()


# ---------------------------------------------------------------------------------------------------------------
# 2. lgc_row_rnorm
# ---------------------------------------------------------------------------------------------------------------
def rnorm_abi(table):
    lib, stream = lib_and_stream(table.t.device)
    out = torch.full((table.rows + 1,), GUARD, device=table.t.device)
    assert lib.lgc_row_rnorm(table.ptr, table.stride, table.rows, table.dim, out.data_ptr(), stream) == 0
    assert float(out[-1]) == GUARD
    return out[:-1]


@pytest.mark.parametrize("dim", WIDTHS)
def test_row_rnorm_is_the_header_rule_bit_for_bit(device, dim):
    for kind in ("random", "wide"):
        table = cs.tables(kind, dim)[1].copy()
        table[0] = 0.0
        table[1, dim - 1] = np.nan
        want = cs.rnorm32(table)
        assert want[0] == 0.0 and np.isnan(want[1])
        for layout in cs.LAYOUTS:
            got = rnorm_abi(Table(table, layout, device)).cpu().numpy()
            assert cs.same_bits(got, want), (dim, kind, layout, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5])
    assert (cs.rnorm32(cs.tables("wide", dim)[1]) == 0).any()                          # squares that underflow: "similar to nothing"


# ---------------------------------------------------------------------------------------------------------------
# 3. lgc_item_neighbors
# ---------------------------------------------------------------------------------------------------------------
def neighbors_abi(items, q, scale, exclude_self, k, slices):
    dev = items.t.device
    lib, stream = lib_and_stream(dev)
    n = q.numel()
    index = torch.full((n, k), -77, dtype=torch.int64, device=dev)
    value = torch.full((n, k), 77.0, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.lgc_item_neighbors_workspace_bytes(n, items.rows, k, slices)
    ws = torch.full(((need + 7) // 8 + 1,), -1, dtype=torch.int64, device=dev)
    code = lib.lgc_item_neighbors(items.ptr, items.stride, items.rows, items.dim, q.data_ptr(), n, _native.ptr(scale), None,
                                  exclude_self, k, slices, index.data_ptr(), value.data_ptr(), ws.data_ptr() if need else None,
                                  need, status.data_ptr(), stream)
    assert code == 0 and int(status.item()) == 0 and int(ws[-1].item()) == -1
    return index.cpu().numpy(), value.cpu().numpy()


_query_panels = {}


def query_panel(kind, dim):
    if (kind, dim) not in _query_panels:
        items = cs.tables(kind, dim)[1]
        _query_panels[kind, dim] = cs.chain32(items[cs.query_ids(dim)], items)
    return _query_panels[kind, dim]


@pytest.mark.parametrize("dim", WIDTHS)
def test_item_neighbors_rank_and_return_the_host_chain(device, dim):
    """Values under ``same_folded``: the header's documented fold of the padded tile (and of the returned values)."""
    q_np, k = cs.query_ids(dim), 64
    settings = {"dense": ((0, 1), (1, 3)), "poisoned": ((0, 3), (1, 1))}                # (exclude_self, slices)
    for kind in ("permuted", "random"):
        dots = query_panel(kind, dim)
        for layout in cs.LAYOUTS:
            w = world(device, dim, kind, layout)
            q = up(q_np, device)
            rnorm = rnorm_abi(w.items)                       # pinned by test 2
            rn = rnorm.cpu().numpy()
            with np.errstate(all="ignore"):
                cosine = ((dots * rn[q_np][:, None]).astype(np.float32) * rn[None, :]).astype(np.float32)
            for scale, scores in ((None, dots), (rnorm, cosine)):
                for exclude_self, slices in settings[layout]:
                    want_i, want_v = ss.neighbors_ref(scores, q_np, k, None, bool(exclude_self))
                    got_i, got_v = neighbors_abi(w.items, q, scale, exclude_self, k, slices)
                    what = (dim, kind, layout, scale is not None, exclude_self, slices)
                    assert np.array_equal(got_i, want_i), (what, np.argwhere(got_i != want_i)[:5].tolist())
                    assert cs.same_folded(got_v, want_v), what


# ---------------------------------------------------------------------------------------------------------------
# 4. lgc_rank_positions
# ---------------------------------------------------------------------------------------------------------------
def rank_abi(w, pu, pi, seen, mode, slices):
    dev = w.device
    lib, stream = lib_and_stream(dev)
    n = pu.numel()
    outs = [torch.full((n,), -77, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.full((n,), 77.0, device=dev)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.lgc_rank_positions_workspace_bytes(n, N_ITEMS, slices)
    ws = torch.full((need // 4 + 1,), -1, dtype=torch.int32, device=dev)
    ptr, entries = (None, None) if seen is None else seen
    code = lib.lgc_rank_positions(w.users.ptr, w.users.stride, w.users.rows, w.items.ptr, w.items.stride, N_ITEMS, w.dim,
                                  pu.data_ptr(), pi.data_ptr(), n, _native.ptr(ptr), _native.ptr(entries), fs.MODES.index(mode),
                                  slices, *(o.data_ptr() for o in outs), ws.data_ptr(), need, status.data_ptr(), stream)
    assert code == 0 and int(status.item()) == 0 and int(ws[-1].item()) == -1
    return [o.cpu().numpy() for o in outs]


def same_ranks(got, want, what):
    for name, g, x in zip(("rank", "n_equal", "n_cand"), got[:3], want[:3]):
        assert np.array_equal(g, x), (what, name, np.flatnonzero(g != x)[:5].tolist(), g[g != x][:5].tolist(), x[g != x][:5].tolist())
    assert cs.same_bits(got[3], want[3]), (what, "value")


@pytest.mark.parametrize("dim", WIDTHS)
def test_rank_positions_count_over_the_host_chain(device, dim):
    pu_np, pi_np, ptr, entries = cs.rank_case(dim)
    lists = [entries[ptr[u]:ptr[u + 1]] for u in pu_np]
    pu, pi, seen = up(pu_np, device), up(pi_np, device), (up(ptr, device), up(entries, device))
    for kind in ("permuted", "random"):
        panel = cs.panel(kind, dim)[pu_np]
        plain = fs.ranks_ref(panel, pi_np, None, "zero")
        if kind == "permuted" and dim >= 3:
            assert plain[1].max() > 10                       # the ties are long: a one-ulp change of the chain moves counts
        same_ranks(rank_abi(world(device, dim, kind, "poisoned"), pu, pi, None, "zero", 0), plain, (dim, kind, "no lists"))
        for mode in fs.MODES:
            want = fs.ranks_ref(panel, pi_np, lists, mode)
            for slices, layout in ((0, "poisoned"), (1, "dense"), (3, "poisoned")):
                got = rank_abi(world(device, dim, kind, layout), pu, pi, seen, mode, slices)
                same_ranks(got, want, (dim, kind, mode, slices, layout))


# ---------------------------------------------------------------------------------------------------------------
# 5. the other holders of the chain, each against chain32 of the rows involved
# ---------------------------------------------------------------------------------------------------------------
HOLDER_KINDS = ("random", "wide")


@pytest.mark.parametrize("dim", CLASS_WIDTHS)
def test_hard_negative_scores_are_the_host_chain(device, dim):
    lib, stream = lib_and_stream(device)
    n, n_cand, seed, step = 2 * N_ROWS, 8, 7 + dim, 3
    users = [i % N_ROWS for i in range(n)]
    csrs = (sp.csr(N_ROWS, {u: [N_ROWS + (7 * u) % N_ITEMS] for u in range(N_ROWS)}), sp.csr(N_ROWS, {}))
    dev = lambda a, dt: torch.tensor(list(a) or [0], dtype=dt, device=device)
    (pp, pi), (ip, ii) = csrs
    args = [dev(users, torch.int64), dev(pp, torch.int32), dev(pi, torch.int64), dev(ip, torch.int32), dev(ii, torch.int64)]
    for kind in HOLDER_KINDS:
        w, panel = world(device, dim, kind, "poisoned"), cs.panel(kind, dim)
        recs = hs.walk(users, csrs, N_ROWS, N_ITEMS, seed, step, n_cand, lambda u, item: panel[u, item])
        want = np.array([panel[r.user, r.neg - N_ROWS] for r in recs], dtype=np.float32)
        pos, neg = (torch.full((n,), -9, dtype=torch.int64, device=device) for _ in range(2))
        score = torch.full((n + 1,), GUARD, device=device)
        attempt, adm = (torch.full((n,), -9, dtype=torch.int32, device=device) for _ in range(2))
        status = torch.zeros(1, dtype=torch.int32, device=device)
        code = lib.lgc_sample_hard_triples(args[0].data_ptr(), n, *(t.data_ptr() for t in args[1:]), N_ROWS, N_ITEMS,
                                           seed, step, n_cand, w.users.ptr, w.users.stride, w.items.ptr, w.items.stride, dim,
                                           pos.data_ptr(), neg.data_ptr(), score.data_ptr(), attempt.data_ptr(), adm.data_ptr(),
                                           status.data_ptr(), stream)
        assert code == 0 and int(status.item()) == 0 and float(score[-1]) == GUARD
        assert neg.tolist() == [r.neg for r in recs] and attempt.tolist() == [r.attempt for r in recs], (dim, kind)
        assert pos.tolist() == [r.pos for r in recs] and adm.tolist() == [n_cand] * n
        got = score[:-1].cpu().numpy()
        assert cs.same_bits(got, want), (dim, kind, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5])


@pytest.mark.parametrize("dim", CLASS_WIDTHS)
def test_attribution_base_and_contributions_are_the_host_chain(device, dim):
    """Session form, unit weights, normalize = 0, a0 = 1: contrib = 1 * dot(F[i], E[t]) and base = 1 * dot(z, E[t]), with
    F = E = the item table and z the user rows -- the item x item and the user x item panels of ``chain32``."""
    lib, stream = lib_and_stream(device)
    rng = np.random.default_rng([5, dim])
    n_t, lengths = 16, [(1, 5, 33)[r % 3] for r in range(N_ROWS)]
    ptr = np.zeros(N_ROWS + 1, dtype=np.int64)
    np.cumsum(lengths, out=ptr[1:])
    listed = rng.integers(0, N_ITEMS, size=int(ptr[-1])).astype(np.int64)
    targets = np.stack([rng.permutation(N_ITEMS)[:n_t] for _ in range(N_ROWS)]).astype(np.int64)
    owner = np.repeat(np.arange(N_ROWS), lengths)
    for kind in HOLDER_KINDS:
        w = world(device, dim, kind, "poisoned")
        hold = [up(x, device) for x in (ptr, listed, targets, np.arange(N_ROWS, dtype=np.int64))]
        contrib = torch.full(((int(ptr[-1]) + 1) * n_t,), GUARD, device=device)
        base = torch.full((N_ROWS + 1, n_t), GUARD, device=device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        a = _native.AttrArgsC()
        a.list_ptr, a.list_items, a.targets, a.init_rows = (x.data_ptr() for x in hold)
        a.contrib_ptr, a.normalize, a.n_rows, a.n_items = hold[0].data_ptr(), 0, N_ROWS, N_ITEMS
        a.fold, a.fold_stride, a.items, a.item_stride = w.items.ptr, w.items.stride, w.items.ptr, w.items.stride
        a.init, a.init_stride, a.n_init_rows, a.a0 = w.users.ptr, w.users.stride, N_ROWS, 1.0
        a.target_stride, a.n_targets, a.top_m, a.dim = n_t, n_t, 0, dim
        a.contrib, a.base, a.status = contrib.data_ptr(), base.data_ptr(), status.data_ptr()
        assert lib.lgc_attribute(a, stream) == 0 and int(status.item()) == 0
        got_c, got_b = contrib.cpu().numpy(), base.cpu().numpy()
        assert (got_c[-n_t:] == GUARD).all() and (got_b[-1] == GUARD).all()
        want_c = cs.panel(kind, dim, "items")[listed[:, None], targets[owner]]
        want_b = cs.panel(kind, dim)[np.arange(N_ROWS)[:, None], targets]
        assert cs.same_bits(got_c[:-n_t].reshape(-1, n_t), want_c), (dim, kind, "contrib")
        assert cs.same_bits(got_b[:-1], want_b), (dim, kind, "base")


@pytest.mark.parametrize("dim", CLASS_WIDTHS)
def test_mmr_objective_at_lambda_0_is_the_host_chain(device, dim):
    """lambda = 0: step 0 takes position 0 (every objective is 0 * rel = +0), and from step 1 on the objective is
    0 - (1 * pen) with pen the running maximum of dot(p, chosen) -- ``chain32`` of the two item rows.  The whole greedy walk
    (``rerank_support.mmr_ref``) runs over the host panel; ``out_value`` is compared after x + 0, as the header returns it."""
    lib, stream = lib_and_stream(device)
    LDS, GLOBAL = 1, 2
    routes = {n_cand: lib.lgc_rerank_route(n_cand, dim) for n_cand in (8, 256)}
    assert routes[8] == LDS and routes[256] == (LDS if 256 * rs.row_stride(dim) * 4 <= rs.LDS_PER_WAVE else GLOBAL)
    assert (routes[256] == GLOBAL) == (dim >= 48)            # both routes from 48 columns on; below, the lists all fit
    k = 4
    for kind in HOLDER_KINDS:
        w, sim = world(device, dim, kind, "poisoned"), cs.panel(kind, dim, "items")
        for n_cand in routes:
            rng = np.random.default_rng([6, dim, n_cand])
            cand, rel = rs.candidates(rng, N_ROWS, n_cand, N_ITEMS), rs.descending_rel(rng, N_ROWS, n_cand)
            want = rs.mmr_ref_rows(rel, cand, lambda r: (lambda ps, c: sim[cand[r, ps], cand[r, c]]), k, 0.0, N_ITEMS)
            index = torch.full((N_ROWS + 1, k), -77, dtype=torch.int64, device=device)
            pos = torch.full((N_ROWS, k), -77, dtype=torch.int32, device=device)
            value = torch.full((N_ROWS + 1, k), 77.0, device=device)
            status = torch.zeros(1, dtype=torch.int32, device=device)
            c_dev, r_dev = up(cand, device), up(rel, device)
            code = lib.lgc_rerank_mmr(w.items.ptr, w.items.stride, N_ITEMS, dim, None, c_dev.data_ptr(), n_cand, r_dev.data_ptr(),
                                      n_cand, N_ROWS, n_cand, k, 0.0, index.data_ptr(), pos.data_ptr(), value.data_ptr(),
                                      status.data_ptr(), stream)
            assert code == 0 and int(status.item()) == 0 and index[-1].tolist() == [-77] * k and value[-1].tolist() == [77.0] * k
            what = (dim, kind, n_cand)
            assert np.array_equal(pos.cpu().numpy(), want[1]) and np.array_equal(index[:-1].cpu().numpy(), want[0]), what
            assert (want[1][:, 0] == 0).all() and not np.isnan(want[2]).any()
            with np.errstate(invalid="ignore"):
                folded = want[2] + np.float32(0.0)
            assert cs.same_bits(value[:-1].cpu().numpy(), folded), what


# 6. lgc_softmax_batch's logits are no output: its widths of one, two and three 16-column groups are cases of
# tests/softmax_support.py and run under tests/test_softmax_gpu.py's derived bounds, which start from lgc_score_rows' panel --
# pinned by test 1.
