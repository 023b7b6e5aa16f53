"""``propagate.bipartite_sum`` on every path it takes, row by row against fp64 (graph, references and recorder:
tests/layer_sum_support.py).

One 700 x 45 graph whose item operators (full, kept users', concatenated) all run as a FORCED band sweep under the small
planner configuration of tests/test_mix_epilogue_gpu.py.  Per (setting, width): K = 1, 2, 3, 4, 5, 7, equal and unequal
alphas, the whole result and 96 listed rows (``final_rows``) with SCORED_ITEM_ROWS_ONLY on and off and
``Operator.listed_rows_pay`` forced to yes and to no, and at widths that are no multiple of 32 all of it once more with
UNIFORM_ALPHA_SHORTCUT = "force"; every scratch table NaN-filled, padding included.  Each case asserts

1. the path: which operator objects ``Operator.apply`` and ``apply_rows`` ran on, how often, and the route of the item step;
2. per compared row r  ||got_r - want_r||_2 <= 1e-5 ||mag_r||_2  with want = sum_l alpha_l A^l x0 and
   mag = sum_l |alpha_l| |A|^l |x0| in fp64 from the operator's own fp32 values, and rel_fro <= 1e-5 over those rows
   (1e-5 is the project's gate on a propagation, TOL in the neighbouring tests);
3. the rows without entries (item EMPTY, the isolated user) hold fl(alpha_0 * x0[r]) exactly;
4. no NaN in a compared row and the same bits on a second run;
5. listed rows against the full result of the same setting: rel_fro <= 1e-6 (TOL_PATHS of test_reduced_concat_gpu.py).

Measured worst per-row ratios (MI355X), the maximum over all cases of a (setting, width); the gate is 1e-5:
    D      no_elimination  separate_gram_t3  separate_gram_t4         concat_t3         concat_t4
    62           5.68e-08          5.68e-08          5.68e-08          5.68e-08          5.68e-08
    64           6.17e-08          6.16e-08          6.16e-08          6.17e-08          6.17e-08
    68           7.79e-08          7.79e-08          7.79e-08          7.79e-08          7.79e-08
    90           5.58e-08          5.58e-08          5.58e-08          5.58e-08          5.58e-08
    96           6.64e-08          6.76e-08          6.76e-08          6.64e-08          6.65e-08
    97           6.65e-08          6.65e-08          6.65e-08          6.65e-08          6.65e-08
    128          6.85e-08          6.86e-08          6.86e-08          6.85e-08          6.85e-08
    20           5.71e-08          5.71e-08          5.71e-08          5.71e-08          5.71e-08
Every maximum is an item row of the whole result at K = 7 (K = 5 at D = 20) with unequal alphas, whose last additions are
the same lgc_lincomb in every setting; the worst rel_fro of any case is 6.5e-08.  The training step (the last test): scores,
gradient and seed rows within 1.1e-07 of fp64 in every setting.
"""
import contextlib

import pytest
import torch

import layer_sum_support as S
from conftest import rel_fro
from eliminate_support import alphas_for
from partition_edges_support import loss_fp64
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, propagate, synth
from gnn_ecommerce_amd import graph as G
from gnn_ecommerce_amd.graph import PropGraph

pytestmark = pytest.mark.gpu

TOL = 1e-5            # the project's gate on a whole propagation, here per row against the row's magnitude as well
TOL_PATHS = 1e-6      # two paths of one sum against each other
SETTINGS = {"no_elimination": (0, None), "separate_gram_t3": (3, "0"), "separate_gram_t4": (4, "0"),
            "concat_t3": (3, "1"), "concat_t4": (4, "1")}
DIMS = S.SWEPT + (S.NOT_SWEPT,)
# lgc_sweep_ok's width classes: four entries per step, two entries on rows of 96 floats, two passes of the four-entry plan
ROUTE_OF = {62: "sweep", 64: "sweep", 68: "sweep_wide", 90: "sweep_wide", 96: "sweep_wide", 97: "sweep_two_pass",
            128: "sweep_two_pass"}

_state = {}


def force_sweep(monkeypatch):
    """The knobs of test_mix_epilogue_gpu.swept_graph; set again for every test, the sweep plans are built lazily."""
    monkeypatch.setattr(G, "USE_SWEEP", "1")
    monkeypatch.setattr(G, "SWEEP_CFG", dict(G.SWEEP_CFG, **S.SMALL_PLAN))
    monkeypatch.setattr(G, "SWEEP_CFG_WIDE", dict(G.SWEEP_CFG_WIDE, **S.SMALL_PLAN))
    monkeypatch.setattr(G, "SWEEP_WIDE", True)
    assert G.SWEEP_CFG["n_bands"] == S.N_GAPS


def swept_graph(device, monkeypatch):
    force_sweep(monkeypatch)
    if "pg" not in _state:
        ei, ew = S.edge_list()
        _state["ei"], _state["ew"] = ei, ew
        _state["ei_d"], _state["ew_d"] = ei.to(device), ew.to(device)
        pg = PropGraph(_state["ei_d"], _state["ew_d"], S.N)
        assert pg.split == S.N_USERS
        user_op, item_op = pg.halves()
        assert item_op.sweep_cols == (0, S.N_USERS) and user_op.sweep_cols is None
        _state["coo"] = S.operator_coo(pg.forward_op)
        _state["listed"], _state["gone_user"], _state["kept_user"] = S.listed_rows(ei)
        _state["pg"] = pg
    return _state["pg"]


def nan_scratch(monkeypatch):
    real = propagate.scratch_table

    def scratch(like):
        t = real(like)
        torch.as_strided(t, (t.size(0), t.stride(0)), (t.stride(0), 1)).fill_(float("nan"))
        return t
    monkeypatch.setattr(propagate, "scratch_table", scratch)


_tables, _refs = {}, {}


def table(dim):
    if dim not in _tables:
        _tables[dim] = synth.xavier_table(S.N, dim, 100 + dim)
    return _tables[dim]


def references(dim, k, equal):
    """(want, mag) in fp64 on the host, once per (width, K, alphas); never written to."""
    key = (dim, k, equal)
    if key not in _refs:
        alphas = alphas_for(k, equal)
        _refs[key] = (S.want_fp64(*_state["coo"], table(dim), alphas), S.mag_fp64(*_state["coo"], table(dim), alphas))
    return _refs[key]


@contextlib.contextmanager
def setting_on(pg, setting):
    """T through ``pg.eliminate_max_deg``, the operator through ``red.concat_mode``; both put back."""
    max_deg, mode = SETTINGS[setting]
    pg.eliminate_max_deg = max_deg
    red = None
    try:
        red = pg.reduced()
        if red is not None:
            red.concat_mode = mode
        yield red
    finally:
        if red is not None:
            red.concat_mode = None
        pg.eliminate_max_deg = None


def named_operators(pg, red, cc):
    user_op, item_op = pg.halves()
    ops = {"user_op": user_op, "item_op": item_op}
    if red is not None:
        ops.update(user_op_h=red.user_op_h, item_op_h=red.item_op_h, gram_op=red.gram_op)
    if cc is not None:
        ops.update({"cc.user_op": cc.user_op, "cc.item_op": cc.item_op})
    return ops


def expected_calls(kind, k, listed, pay):
    """How often each operator runs, from ``bipartite_sum``'s description of itself.  K item steps and K user steps.  The
    last user step is the full operator, for the listed rows when there are any.  ``pay`` (listed rows, SCORED_ITEM_ROWS_ONLY
    and ``listed_rows_pay``): the last item step is ``apply_rows(item_op, split=True)``.  With elimination (K >= 2) layer 1's
    item step stays the full operator, the item steps of layers 2 .. K and the user steps of layers 1 .. K - 1 are the
    reduced ones -- but the user step of layer K - 1 is the full one when the listed item rows pay, whose launch gathers
    every user row."""
    reduced = kind != "none" and k >= 2
    last_item_apply = 0 if pay else 1
    if reduced:
        n_item = k - 2 + last_item_apply
        n_user = k - 1 - (1 if pay else 0)
        want = {"item_op": 1, "user_op": (1 if pay else 0) + (0 if listed else 1)}
        if kind == "concat":
            want.update({"cc.item_op": n_item, "cc.user_op": n_user})
        else:
            want.update({"gram_op": n_item, "item_op_h": n_item, "user_op_h": n_user})
    else:
        want = {"item_op": k - 1 + last_item_apply, "user_op": k - 1 + (0 if listed else 1)}
    return {name: n for name, n in want.items() if n}, (1 if pay else 0), (1 if listed else 0)


def assert_path(rec, ops, kind, k, listed, pay, case):
    want, n_split, n_rows = expected_calls(kind, k, listed, pay)
    got = {name: rec.applies(op) for name, op in ops.items() if op is not None and rec.applies(op)}
    assert got == want, (case, got, want)
    assert all(any(o is op for op in ops.values()) for o in rec.operators()), (case, "an operator nobody named ran")
    user_op, item_op = ops["user_op"], ops["item_op"]
    assert rec.rows_calls(item_op, True) == n_split and rec.rows_calls(user_op, False) == n_rows, case
    assert sum(1 for e in rec.events if e[0] == "rows") == n_split + n_rows, case
    if pay and k >= 2:
        at = [i for i, e in enumerate(rec.events) if e[0] == "rows" and e[1] is item_op][0]
        assert rec.events[at - 1][0] == "apply" and rec.events[at - 1][1] is user_op, \
            (case, "the listed item rows gather every user row: the user step before them is the full one")


def item_route(op, offset, x):
    """The route of an item step between two middle tables (views of ``scratch_table`` geometry at the operator's offset)."""
    t_in, t_out = propagate.scratch_table(x), propagate.scratch_table(x)
    return op.route(t_in[offset:], t_out[offset:])


def assert_rows(out, sel, want, mag, alpha0, x_host, case):
    """Checks 2-4 on the rows ``sel`` of ``out`` (None: all); returns the worst per-row ratio and the rel_fro."""
    got = out.cpu() if sel is None else out[sel.to(out.device)].cpu()
    w, m = (want, mag) if sel is None else (want[sel], mag[sel])
    assert not torch.isnan(got).any(), (case, "a stale or unwritten block was read")
    ratios = S.row_ratios(got, w, m)
    worst, fro = ratios.max().item(), rel_fro(got, w)
    for r in (S.ISOLATED, S.N_USERS + S.EMPTY):
        exact = torch.tensor(alpha0) * x_host[r]
        assert exact.dtype == torch.float32 and torch.equal(out[r].cpu(), exact), (case, r, "a row without entries is fl(alpha_0 * x0[r])")
    return worst, fro, int(ratios.argmax())


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_every_path_row_by_row_against_fp64(device, monkeypatch, setting, dim):
    pg = swept_graph(device, monkeypatch)
    nan_scratch(monkeypatch)
    rec = S.Recorder(monkeypatch, G, propagate)
    kind = "none" if setting == "no_elimination" else setting.rsplit("_", 1)[0].replace("separate_gram", "separate")
    x_host = table(dim)
    x = x_host.to(device)
    listed = _state["listed"]
    listed_d, compared = listed.to(device), torch.unique(listed)
    assert {S.ISOLATED, S.N_USERS + S.EMPTY, S.N_USERS + S.HUB, S.N_USERS + S.SINGLE, _state["gone_user"],
            _state["kept_user"]} <= set(compared.tolist()) and compared.numel() < listed.numel()
    worst, worst_fro, worst_case, ran = 0.0, 0.0, None, set()
    with setting_on(pg, setting) as red:
        assert (red is None) == (kind == "none")
        cc = None
        if red is not None:
            assert red.gram_op is not None and red.item_op_h is not None and red.user_op_h is not None and 0 < red.n_h < S.N_USERS
            assert red.item_op_h.sweep_cols == (0, red.n_h)
            cc = red.concat_for(dim, S.N, propagate.scratch_table(x).stride(0))
            assert (cc is not None) == (kind == "concat")
            if cc is not None:
                assert cc.item_op.sweep_cols == (0, cc.csr.n_phys) and cc.csr.gap_rows == 6 and cc.offset >= 0
        ops = named_operators(pg, red, cc)
        # the route of the item steps: the full operator's (layer 1 and the plain path) and the reduced layers' own
        routes = {"item_op": item_route(ops["item_op"], 0, x)}
        if kind == "concat":
            routes["cc.item_op"] = item_route(cc.item_op, cc.offset, x)
        elif kind == "separate":
            routes["item_op_h"] = item_route(red.item_op_h, red.offset, x)
        for name, route in routes.items():
            if dim in ROUTE_OF:
                assert route.split("+")[0] == ROUTE_OF[dim], (name, route)
            else:
                assert not route.startswith("sweep"), (name, route)

        def run(alphas, final_rows):
            rec.clear()
            return propagate._layer_sum(pg, x, alphas, transpose=False, final_rows=final_rows)

        for shortcut in (True,) + (("force",) if dim % 32 else ()):
            monkeypatch.setattr(propagate, "UNIFORM_ALPHA_SHORTCUT", shortcut)
            for k in S.LAYERS:
                for equal in (True, False):
                    alphas = alphas_for(k, equal)
                    want, mag = references(dim, k, equal)
                    case = (setting, dim, shortcut, k, equal, "all rows")
                    full = run(alphas, None)
                    assert_path(rec, ops, kind, k, False, False, case)
                    ran |= {name for name, op in ops.items() if op is not None and rec.applies(op)}
                    ratio, fro, at = assert_rows(full, None, want, mag, alphas[0], x_host, case)
                    if ratio > worst:
                        worst, worst_case = ratio, case + (f"row {at}",)
                    worst_fro = max(worst_fro, fro)
                    assert fro <= TOL and ratio <= TOL, (case, fro, ratio, at)
                    assert torch.equal(run(alphas, None), full), (case, "two runs must give the same bits")
                    for items_only in (True, False):
                        for share in (1e9, 0.0):
                            monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", items_only)
                            monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", share)
                            pays = ops["item_op"].listed_rows_pay(listed.numel())
                            assert pays == (share > 0)
                            case = (setting, dim, shortcut, k, equal, f"listed rows, items_only {items_only}, pay {pays}")
                            few = run(alphas, listed_d)
                            assert_path(rec, ops, kind, k, True, items_only and pays, case)
                            ran |= {name for name, op in ops.items() if op is not None and rec.applies(op)}
                            ratio, fro, at = assert_rows(few, compared, want, mag, alphas[0], x_host, case)
                            if ratio > worst:
                                worst, worst_case = ratio, case + (f"row {int(compared[at])}",)
                            worst_fro = max(worst_fro, fro)
                            assert fro <= TOL and ratio <= TOL, (case, fro, ratio, int(compared[at]))
                            paths = rel_fro(few[listed_d].cpu(), full[listed_d].cpu())
                            assert paths <= TOL_PATHS, (case, paths)
                            again = run(alphas, listed_d)
                            assert torch.equal(again[listed_d], few[listed_d]), (case, "two runs must give the same bits")
                    monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", True)
    assert pg.eliminate_max_deg is None and (red is None or red.concat_mode is None)
    if kind == "concat":
        assert {"cc.item_op", "cc.user_op"} <= ran and not ran & {"gram_op", "item_op_h", "user_op_h"}
    elif kind == "separate":
        assert {"gram_op", "item_op_h", "user_op_h"} <= ran and not ran & {"cc.item_op", "cc.user_op"}
    else:
        assert ran == {"user_op", "item_op"}
    print(f"\n{setting} D={dim}: ran {sorted(ran)}; routes {routes}; worst row ratio {worst:.2e} at {worst_case}; "
          f"worst rel_fro {worst_fro:.2e}")


@pytest.mark.parametrize("t", (3, 4))
def test_auto_takes_the_concatenated_operator_exactly_where_it_is_swept(device, monkeypatch, t):
    """``concat_mode`` None under the forced sweep: the concatenated operator at every swept width, the separate G_L launch
    at D = 20 -- and ``_layer_sum`` runs what ``concat_for`` answered."""
    pg = swept_graph(device, monkeypatch)
    nan_scratch(monkeypatch)
    rec = S.Recorder(monkeypatch, G, propagate)
    assert G.REDUCED_CONCAT == "auto", "the suite runs with the default switch"
    pg.eliminate_max_deg = t
    try:
        red = pg.reduced()
        assert red is not None and red.concat_mode is None
        for dim in DIMS:
            x_host = table(dim)
            x = x_host.to(device)
            stride = propagate.scratch_table(x).stride(0)
            red.concat_mode = "1"
            forced = red.concat_for(dim, S.N, stride)
            red.concat_mode = None
            auto = red.concat_for(dim, S.N, stride)
            swept = G.sweep_choice(_native.load(), dim, S.N - forced.offset, stride) != 0
            assert swept == (dim in S.SWEPT), dim
            assert (auto is forced) if swept else (auto is None), dim
            ops = named_operators(pg, red, forced)
            for k, equal in ((3, True), (4, False)):
                alphas = alphas_for(k, equal)
                rec.clear()
                out = propagate._layer_sum(pg, x, alphas, transpose=False)
                assert_path(rec, ops, "concat" if swept else "separate", k, False, False, (t, dim, k, equal))
                want, mag = references(dim, k, equal)
                ratio, fro, at = assert_rows(out, None, want, mag, alphas[0], x_host, (t, dim, k, equal))
                assert fro <= TOL and ratio <= TOL, (t, dim, k, equal, fro, ratio, at)
    finally:
        pg.eliminate_max_deg = None


def triples():
    """B = 64 (user, positive, negative) triples on the host: HUB and SINGLE among the positives, EMPTY among the
    negatives, the eliminated, the kept and the isolated user among the users."""
    rng = torch.Generator().manual_seed(64)
    users = torch.randint(0, S.N_USERS, (64,), generator=rng)
    pos = torch.randint(0, S.N_ITEMS, (64,), generator=rng) + S.N_USERS
    neg = torch.randint(0, S.N_ITEMS, (64,), generator=rng) + S.N_USERS
    users[:4] = torch.tensor([_state["gone_user"], _state["kept_user"], S.ISOLATED, S.SINGLE_USER])
    pos[:4] = torch.tensor([S.HUB, S.HUB, S.LIGHT[0], S.SINGLE]) + S.N_USERS
    neg[:2] = torch.tensor([S.EMPTY, S.SINGLE]) + S.N_USERS
    return users, pos, neg


@pytest.mark.parametrize("seeded", (False, True), ids=("dense_backward", "seeded_backward"))
@pytest.mark.parametrize("dim,layers", ((64, 3), (90, 5)))
@pytest.mark.parametrize("setting", ("no_elimination", "separate_gram_t4", "concat_t4"))
def test_training_step_against_fp64_autograd(device, monkeypatch, setting, dim, layers, seeded):
    """One step of ``LightGCN`` on the graph ``get_graph`` caches, the forward on the reduced operators and the backward
    on the plain transposed ones: scores and ``embedding.weight.grad`` are still the value and the gradient of the fp64
    function.  ``seeded``: the scoring node that lists its rows (``final_rows``) and starts the backward from the sparse
    seed, which a table of 745 rows takes only with SEED_ROWS_FACTOR lowered to 1; else the dense pair of nodes."""
    swept_graph(device, monkeypatch)
    nan_scratch(monkeypatch)
    rec = S.Recorder(monkeypatch, G, propagate)
    if seeded:
        monkeypatch.setattr(propagate, "SEED_ROWS_FACTOR", 1)
    b, decay = 64, 1e-4
    users, pos, neg = triples()
    w0 = synth.xavier_table(S.N, dim, 7)
    model = lg.LightGCN(S.N, dim, layers)
    model.load_state_dict({"alpha": model.alpha, "embedding.weight": w0})
    model.to(device)
    alphas = model._alphas()
    ei_d, ew_d = _state["ei_d"], _state["ew_d"]
    graph = lg.get_graph(ei_d, ew_d, S.N)
    assert graph.split == S.N_USERS and graph.halves()[1].sweep_cols == (0, S.N_USERS)
    coo = S.operator_coo(graph.forward_op)
    w64 = w0.double().requires_grad_(True)
    ref_scores, ref_loss = loss_fp64(w64, coo, alphas, users, pos, neg, decay)
    ref_loss.backward()
    ud, pd_, nd = users.to(device), pos.to(device), neg.to(device)
    labels = torch.stack((torch.cat([ud, ud]), torch.cat([pd_, nd])))
    with setting_on(graph, setting) as red:
        cc = red.concat_for(dim, S.N, propagate.scratch_table(w0.to(device)).stride(0)) if red is not None else None
        assert (cc is not None) == setting.startswith("concat")
        ops = named_operators(graph, red, cc)
        out = model(ei_d, labels, ew_d)
        assert lg.get_graph(ei_d, ew_d, S.N) is graph
        assert ("ScoresFromTable" in type(out.grad_fn).__name__) == seeded
        forward_ran = {name for name, op in ops.items() if op is not None and rec.applies(op)}
        if setting.startswith("concat"):
            assert {"cc.item_op", "cc.user_op"} <= forward_ran and "gram_op" not in forward_ran
        elif setting.startswith("separate"):
            assert {"gram_op", "item_op_h", "user_op_h"} <= forward_ran
        else:
            assert forward_ran == {"user_op", "item_op"}
        assert (rec.rows_calls(ops["user_op"], False) == 1) == seeded
        loss = model.recommendation_loss(out[:b], out[b:], 0) * b + model.regularization_loss(ud, pd_, nd, decay)
        rec.clear()
        loss.backward()
        assert not any(any(o is op for name, op in ops.items() if name not in ("user_op", "item_op")) for o in rec.operators()), \
            "the backward runs the plain transposed operators"
    lg.check_index_status()
    grad = model.embedding.weight.grad.cpu()
    seeds = torch.unique(torch.cat([users, pos, neg]))
    e_scores = rel_fro(out.detach().cpu().view(1, -1), ref_scores.detach().view(1, -1))
    e_grad, e_seeds = rel_fro(grad, w64.grad), rel_fro(grad[seeds], w64.grad[seeds])
    print(f"\n{setting} D={dim} K={layers} {'seeded' if seeded else 'dense'}: scores {e_scores:.2e}  grad {e_grad:.2e}  "
          f"seed rows {e_seeds:.2e}  loss {loss.item():.6f} (fp64 {ref_loss.item():.6f})")
    assert e_scores <= TOL and e_grad <= TOL and e_seeds <= TOL
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * abs(ref_loss.item())
