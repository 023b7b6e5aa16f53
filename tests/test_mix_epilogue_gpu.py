"""The layer sum written by the item step before the last layer (LGCN_MIX_IN_ITEM_STEP, lgc_apply2, the two-row combine).

One graph, 600 users x 40 items, whose item half runs as a FORCED band sweep under a small planner configuration: item
HUB is in every user's list (600 entries, cut into more than 32 partial slots: the workgroup-per-row branch of the
combine), item EMPTY in none (its row is the epilogue alone), item SINGLE in one, the others in a handful to a few
hundred.  User degrees 1 .. 12, so that T = 3 eliminates most users and keeps some.

1. the kernel: ``apply(x, y, a, r, b, r2, b2)`` bit for bit ``apply(x, t)`` + ``lincomb(y, [(b2, r2), (b, r), (a, t)])``,
   and against fp64, at the widths of every sweep route; r aliasing y.
2. ``propagate_sum`` with the switch on bit for bit the switch off, K = 2, 3, 4, three operator settings, two widths,
   on NaN-filled scratch tables; no lgc_lincomb launch at K = 3.
3. unequal alphas and listed result rows: the new branch is not taken, the bits are those of the switch-off path.

Widths.  The band sweep serves 61..64, 68..96 and 97..128 columns: 64 is the four-entry plan, 90 the two-entry plan on
tables of row stride 96 with the last lane of a row overlapping its neighbour (90 % 4 = 2), 128 the two-pass route, 62
the four-entry plan with lane overlap.  20 columns never reach the sweep's combine: there the call must be refused.
"""
import numpy as np
import pytest
import torch

from conftest import rel_fro
from eliminate_support import _coo, alphas_for, csr_host, layer_sum_fp64
from gnn_ecommerce_amd import _native, propagate, synth
from gnn_ecommerce_amd import graph as G
from gnn_ecommerce_amd.graph import PropGraph

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 600, 40
N = N_USERS + N_ITEMS
HUB, EMPTY, SINGLE = 5, 17, 23
LIGHT = (30, 31, 32, 33, 34, 35, 36, 37)
T = 3
A, B, B2 = 0.75, 0.5, 0.25                 # exact in fp32, all different
TOL_FP64 = 1e-6                            # relative Frobenius against the fp64 restatement
TOL = 1e-5                                 # the project's gate on a whole propagation
SWEPT = (62, 64, 90, 128)
ROUTE_OF = {62: "sweep", 64: "sweep", 90: "sweep_wide", 128: "sweep_two_pass"}
# pieces of at most 8 entries: the hub row gets 75 or more partial slots, beyond SweepPlan.WIDE_SLOTS = 32
SMALL_PLAN = dict(waves_per_band_round=8, row_cap=20, piece_cap=8)


def edge_list():
    rng = np.random.default_rng(20261019)
    others = np.array([i for i in range(N_ITEMS) if i not in (HUB, EMPTY, SINGLE) + LIGHT])
    pairs = []
    for u in range(N_USERS):
        pairs.append((u, HUB))
        for i in rng.choice(others, size=u % 12, replace=False):
            pairs.append((u, int(i)))
    pairs.append((7, SINGLE))
    for j, i in enumerate(LIGHT):                                 # 2, 5, 8, ... 23 entries
        for u in rng.choice(N_USERS, size=2 + 3 * j, replace=False):
            pairs.append((int(u), i))
    return _coo(N_USERS, pairs)


_state = {}


def swept_graph(device, monkeypatch):
    """The graph with every item operator (full, kept users', concatenated) a band sweep under SMALL_PLAN; built once.
    The knobs are set again for every test: the sweep plans are built lazily, at the first apply of each width."""
    monkeypatch.setattr(G, "USE_SWEEP", "1")
    monkeypatch.setattr(G, "SWEEP_CFG", dict(G.SWEEP_CFG, **SMALL_PLAN))
    monkeypatch.setattr(G, "SWEEP_CFG_WIDE", dict(G.SWEEP_CFG_WIDE, **SMALL_PLAN))
    monkeypatch.setattr(G, "SWEEP_WIDE", True)
    if "pg" not in _state:
        ei, ew = edge_list()
        pg = PropGraph(ei.to(device), ew.to(device), N)
        assert pg.split == N_USERS
        user_op, item_op = pg.halves()
        assert item_op.sweep_cols == (0, N_USERS)
        rowptr = item_op.rowptr.cpu().long()
        deg = (rowptr[1:] - rowptr[:-1])[N_USERS:]
        assert deg[EMPTY] == 0 and deg[SINGLE] == 1 and deg[HUB] == N_USERS and ((deg > 1) & (deg < 64)).sum() >= 5
        _state["pg"] = pg
    return _state["pg"]


def table(dim, seed, device, lo=-1.0, hi=1.0):
    """[N, dim] fp32 in the layout of the middle tables: rows of 96 floats at 90 columns (NaN in the padding)."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.empty((N, dim)).uniform_(lo, hi, generator=gen)
    stride = dim if dim % 32 == 0 or dim < 68 else (dim + 31) // 32 * 32
    full = torch.full((N, stride), float("nan"), device=device)
    full[:, :dim] = t.to(device)
    return full[:, :dim]


def nan_like(t):
    full = torch.full((t.size(0), t.stride(0)), float("nan"), device=t.device)
    return full[:, :t.size(1)]


_refs = {}


def item_product_fp64(item_op, x, dim):
    """(A x)[items] in fp64 from the operator's own fp32 values; once per width."""
    if dim not in _refs:
        rowptr, cols, vals, rows = csr_host(item_op)
        keep = rows >= N_USERS
        p = torch.zeros((N, dim), dtype=torch.float64).index_add_(0, rows[keep], vals[keep].view(-1, 1) * x.cpu().double()[cols[keep]])
        _refs[dim] = p[N_USERS:]
    return _refs[dim]


@pytest.mark.parametrize("dim", SWEPT)
def test_two_row_combine_against_two_launches_and_fp64(device, monkeypatch, dim):
    pg = swept_graph(device, monkeypatch)
    item_op = pg.halves()[1]
    x = table(dim, 100 + dim, device)
    r, r2 = table(dim, 200 + dim, device, 0.25, 1.0), table(dim, 300 + dim, device, 0.25, 1.0)
    t, want, got = nan_like(x), nan_like(x), nan_like(x)
    assert item_op.route(x, got, r).split("+")[0] == ROUTE_OF[dim] and item_op.takes_second_row(x, got, r)
    item_op.apply(x, t)
    plan = item_op._sweep[2 if dim == 90 else 4]
    slots = plan.multi[:, 2] - plan.multi[:, 1]
    assert plan.multi_wide.size(0) >= 1 and (slots == 0).sum() >= 1 and (slots == 1).sum() >= 1, "the rows this test is about"
    _native.lincomb(want[N_USERS:], [(B2, r2[N_USERS:]), (B, r[N_USERS:]), (A, t[N_USERS:])])
    item_op.apply(x, got, a=A, r=r, b=B, r2=r2, b2=B2)
    assert torch.isnan(got[:N_USERS]).all(), "only the rows of the plan are written"
    assert not torch.isnan(got[N_USERS:]).any()
    assert torch.equal(got[N_USERS:], want[N_USERS:]), "one launch must give the bits of the two"
    ref = A * item_product_fp64(item_op, x, dim) + B * r[N_USERS:].cpu().double() + B2 * r2[N_USERS:].cpu().double()
    err = rel_fro(got[N_USERS:].cpu(), ref)
    print(f"D={dim}: rel_fro against fp64 {err:.2e}")
    assert err <= TOL_FP64
    exact = torch.tensor(B2) * r2[N_USERS + EMPTY].cpu() + torch.tensor(B) * r[N_USERS + EMPTY].cpu()
    assert torch.equal(got[N_USERS + EMPTY].cpu(), exact), "a row without entries holds fl(fl(b2 * r2) + fl(b * r))"
    # a = 1: the sum is not scaled at all
    _native.lincomb(want[N_USERS:], [(B2, r2[N_USERS:]), (B, r[N_USERS:]), (1.0, t[N_USERS:])])
    item_op.apply(x, got, a=1.0, r=r, b=B, r2=r2, b2=B2)
    assert torch.equal(got[N_USERS:], want[N_USERS:])
    # r aliasing y (the alias the reduced path relies on for its single row), then r2 aliasing y
    _native.lincomb(want[N_USERS:], [(B2, r2[N_USERS:]), (B, r[N_USERS:]), (A, t[N_USERS:])])
    for alias in ("r", "r2"):
        y = nan_like(x)
        y[N_USERS:] = (r if alias == "r" else r2)[N_USERS:]
        item_op.apply(x, y, a=A, r=y if alias == "r" else r, b=B, r2=y if alias == "r2" else r2, b2=B2)
        assert torch.equal(y[N_USERS:], want[N_USERS:]), alias
        assert torch.isnan(y[:N_USERS]).all()


def test_widths_and_operators_without_a_sweep_are_refused(device, monkeypatch):
    pg = swept_graph(device, monkeypatch)
    user_op, item_op = pg.halves()
    for op, dim in ((item_op, 20), (item_op, 66), (user_op, 64)):
        x, r = table(dim, 1, device), table(dim, 2, device)
        y = nan_like(x)
        assert not op.takes_second_row(x, y, r)
        with pytest.raises(_native.NativeLibraryError):
            op.apply(x, y, a=A, r=r, b=B, r2=r, b2=B2)
        assert torch.isnan(y).all(), "a refused call launches nothing"
    x = table(64, 1, device)
    with pytest.raises(ValueError):
        item_op.apply(x, nan_like(x), r2=x, b2=B2)


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def watch(monkeypatch):
    """Counting wrappers around lgc_lincomb and around the applies that carry a second row."""
    lincomb = Counter(_native.lincomb)
    monkeypatch.setattr(_native, "lincomb", lincomb)
    second = Counter(lambda: None)
    real_apply = G.Operator.apply

    def apply(self, x, out, a=1.0, r=None, b=0.0, r2=None, b2=0.0):
        if r2 is not None:
            second()
        return real_apply(self, x, out, a=a, r=r, b=b, r2=r2, b2=b2)
    monkeypatch.setattr(G.Operator, "apply", apply)
    return lincomb, second


def nan_scratch(monkeypatch):
    real = propagate.scratch_table

    def scratch(like):
        t = real(like)
        torch.as_strided(t, (t.size(0), t.stride(0)), (t.stride(0), 1)).fill_(float("nan"))
        return t
    monkeypatch.setattr(propagate, "scratch_table", scratch)


SETTINGS = {"no_elimination": (0, None), "concat": (T, "1"), "separate_gram": (T, "0")}


def layer_sum(pg, x, alphas, setting, mix, monkeypatch, final_rows=None):
    max_deg, mode = SETTINGS[setting]
    monkeypatch.setattr(propagate, "MIX_IN_ITEM_STEP", mix)
    pg.eliminate_max_deg = max_deg
    red = pg.reduced()
    try:
        if red is not None:
            red.concat_mode = mode
        return propagate._layer_sum(pg, x, alphas, transpose=False, final_rows=final_rows)
    finally:
        if red is not None:
            red.concat_mode = None
        pg.eliminate_max_deg = None


@pytest.mark.parametrize("dim", (64, 90))
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_layer_sum_is_bit_identical_with_the_switch_on_and_off(device, monkeypatch, setting, dim):
    pg = swept_graph(device, monkeypatch)
    if dim == 90:
        monkeypatch.setattr(propagate, "UNIFORM_ALPHA_SHORTCUT", "force")
    nan_scratch(monkeypatch)
    lincomb, second = watch(monkeypatch)
    x = synth.xavier_table(N, dim, 11, device)
    if setting != "no_elimination":
        pg.eliminate_max_deg = T
        red = pg.reduced()
        pg.eliminate_max_deg = None
        assert red is not None and red.gram_op is not None and red.item_op_h is not None and 0 < red.n_h < N_USERS
        red.concat_mode = "1"
        cc = red.concat_for(dim, N, propagate.scratch_table(x).stride(0))
        red.concat_mode = None
        assert cc is not None and cc.item_op.sweep_cols == (0, cc.csr.n_phys)
    for k in (2, 3, 4):
        alphas = alphas_for(k, True)
        counts = {}
        outs = {}
        for mix in (True, False):
            lincomb.calls = second.calls = 0
            outs[mix] = layer_sum(pg, x, alphas, setting, mix, monkeypatch)
            counts[mix] = (lincomb.calls, second.calls)
        assert not torch.isnan(outs[True]).any() and not torch.isnan(outs[False]).any(), (k, "a stale or unwritten block was read")
        assert torch.equal(outs[True], outs[False]), (setting, dim, k)
        err = rel_fro(outs[True].cpu(), layer_sum_fp64(pg.forward_op, x, alphas))
        print(f"{setting} D={dim} K={k}: launches (lincomb, two-row applies) on {counts[True]} off {counts[False]}, rel_fro {err:.2e}")
        assert err <= TOL
        assert counts[False][1] == 0 and counts[False][0] >= 1, "the switch off is the path with the lincomb"
        if k == 4 or (k == 3 and setting == "separate_gram"):
            assert counts[True] == counts[False], "K >= 4 and the separate G_L launch keep their launches"
        elif k == 3:
            assert counts[True] == (0, 1), "K = 3: no lgc_lincomb, one apply with two rows"
        else:
            assert counts[True] == (counts[False][0] - 1, 0), "K = 2: the single row does it"


@pytest.mark.parametrize("dim", (64, 90))
def test_unequal_alphas_and_listed_rows_keep_their_path(device, monkeypatch, dim):
    pg = swept_graph(device, monkeypatch)
    if dim == 90:
        monkeypatch.setattr(propagate, "UNIFORM_ALPHA_SHORTCUT", "force")
    nan_scratch(monkeypatch)
    lincomb, second = watch(monkeypatch)
    x = synth.xavier_table(N, dim, 12, device)
    gen = torch.Generator().manual_seed(5)
    rows = torch.cat([torch.randint(0, N_USERS, (48,), generator=gen), N_USERS + torch.randint(0, N_ITEMS, (48,), generator=gen)]).to(device)
    for setting in sorted(SETTINGS):
        for k in (2, 3):
            for alphas, final_rows in ((alphas_for(k, False), None), (alphas_for(k, True), rows), (alphas_for(k, False), rows)):
                outs, counts = {}, {}
                for mix in (True, False):
                    lincomb.calls = second.calls = 0
                    outs[mix] = layer_sum(pg, x, alphas, setting, mix, monkeypatch, final_rows)
                    counts[mix] = (lincomb.calls, second.calls)
                assert counts[True] == counts[False] and counts[True][1] == 0, (setting, k, counts)
                a, b = (outs[True], outs[False]) if final_rows is None else (outs[True][rows], outs[False][rows])
                assert not torch.isnan(a).any() and torch.equal(a, b), (setting, dim, k, final_rows is not None)
