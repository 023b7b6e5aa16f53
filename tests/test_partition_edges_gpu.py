"""``partition.PartitionedPropagator`` on awkward partitions through the HIP kernels (``HipOps``): the cases of
tests/test_partition_edges_host.py on the device, the ranks as threads sharing one stream.  Graphs, fp64 references (on the
host, once per graph, K, alphas and width) and checks: tests/partition_edges_support.py.

What a rank's kernels and planners meet here and nowhere else in the suite: ``Operator.build`` on an empty row range and
on an empty edge list, item operators over the columns of ONE user, item rows whose slices are empty, tiled and chunked
side by side, the halves of A^T of a directed edge list, the compact listed-rows table on a rank that holds none of the
rows, the seeded backward on a rank without a triple, and -- with the sweep forced on -- a band sweep over a column range
that starts above 0 (or is one column wide) as part of a whole partitioned sum.

Every compared row r carries  ||got_r - want_r||_2 <= 1e-5 ||mag_r||_2  (the project's gate on a propagation); foreign
user rows are exactly zero, rows without entries exactly fl(alpha_0 x0[r]), a second call gives the same bits and
``check_index_status`` stays clean.

Measured worst per-row ratios (MI355X), the maximum over worlds, K, alphas and both directions; the gate is 1e-5:
    graph                              D=7        D=64        D=90       D=128
    hub_first                     7.42e-08    4.99e-08    5.03e-08    5.32e-08
    hub_last                      9.13e-08    4.98e-08    5.23e-08    5.24e-08
    isolated_ends                 5.58e-08    4.30e-08    4.18e-08    4.31e-08
    few_users                     6.28e-08    5.59e-08    5.01e-08    4.94e-08
    directed                      7.39e-08    5.07e-08    5.09e-08    4.57e-08
    skew                          6.32e-08    5.17e-08    4.79e-08    5.18e-08
    skew, sweep forced                   -    5.13e-08    4.77e-08    5.34e-08
    hub_first, sweep forced              -    4.99e-08    5.03e-08    5.32e-08
The figures of a graph barely move with the number of ranks: a row's sum is the same chain of adds whoever owns it, only
the all-reduce of the item block associates differently.  The step halves (bpr, reg, gradient of the own rows and of the
seed rows) stay within 1.36e-07 of the fp64 step in every case.

What the first run on the device found: on a rank that owns no user, the local edge list -- and with it the entry array of
its item operator and of the user half of its A^T -- is empty, and ``lgc_spmm_rows`` / ``lgc_spmm_rows_split`` refused the
NULL array with "invalid argument" (``graph.apply_rows`` now hands them a stand-in address; no entry is read).
"""
import threading

import pytest
import torch

import partition_edges_support as S
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import graph as G, propagate
from gnn_ecommerce_amd.partition import HipOps, PartitionedPropagator, partitioned_bpr_loss
from gnn_ecommerce_amd.trainer import PartitionedTrainer

pytestmark = pytest.mark.gpu

DIMS = (7, 64, 90, 128)            # the narrow kernels and the three width classes of lgc_sweep_ok
SWEPT_DIMS = (64, 90, 128)
CASES = [(name, world) for name in S.SMALL_GRAPHS for world in S.WORLDS] + [("skew", 2), ("skew", 3)]
_cases, _tables = {}, {}


def case_of(device, name, world, tag="default"):
    """The propagators of a (graph, world), built once; ``tag`` keeps those built under a forced sweep apart."""
    key = (name, world, tag)
    if key not in _cases:
        _cases[key] = S.Case(name, world, HipOps, device)
    return _cases[key]


def table(device, name, dim, seed=0):
    key = (name, dim, seed)
    if key not in _tables:
        _tables[key] = S.table(name, dim, seed).to(device)
    return _tables[key]


def sums(case, device, dims, report):
    for dim in dims:
        x0 = table(device, case.name, dim)
        worst = 0.0
        for k in S.LAYERS:
            for equal in (True, False):
                for transpose in (False, True):
                    worst = max(worst, S.check_sum(case, dim, k, equal, transpose, x0, again=True))
                    lg.check_index_status()
        print(f"\n{report} {case.name} world {case.world} D={dim}: worst row ratio {worst:.2e}")


@pytest.mark.parametrize("name,world", CASES)
def test_forward_and_transposed_sums_row_by_row_against_fp64(device, name, world):
    case = case_of(device, name, world)
    S.check_partition(case)
    sums(case, device, DIMS, "RATIO")


@pytest.mark.parametrize("name,world", CASES)
def test_one_hop_with_an_epilogue_row(device, name, world):
    """``hop``: the b * r term of the exchanged item block is added by one rank only."""
    case = case_of(device, name, world)
    for dim in DIMS:
        S.check_hop(case, dim, table(device, name, dim), table(device, name, dim, 2), S.table(name, dim), S.table(name, dim, 2))
    lg.check_index_status()


@pytest.mark.parametrize("pays", (True, False), ids=("listed_item_step", "full_item_step"))
@pytest.mark.parametrize("name,world", CASES)
def test_listed_rows_against_fp64(device, monkeypatch, name, world, pays):
    """``final_rows`` / ``final_item_rows`` with the listed-rows rule forced either way: repeated ids, foreign users
    clamped into the rank's range (onto a foreign user where the range is empty), item ids outside the item block."""
    monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", 1e9 if pays else 0.0)
    monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", True)
    case = case_of(device, name, world)
    for dim in DIMS:
        x0 = table(device, name, dim)
        for k in S.LAYERS:
            for equal in (True, False):
                S.check_listed(case, dim, k, equal, False, x0, pays, again=True)
        S.check_listed(case, dim, 3, False, True, x0, pays, again=True)
    lg.check_index_status()


@pytest.mark.parametrize("name,world", [(n, w) for n, w in CASES if w in (1, 3)])
def test_repeated_listed_items_take_the_maximum_over_their_positions(device, monkeypatch, name, world):
    """The ``index_reduce_(..., "amax")`` write-back under an exchange that sums every list position differently."""
    monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", 1e9)
    monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", True)
    case = case_of(device, name, world)
    for dim in (7, 90):
        for k, equal in ((1, False), (3, True), (5, False)):
            S.check_repeats_take_the_maximum(case, dim, k, equal, table(device, name, dim))
    lg.check_index_status()


def item_entries(case, rank, transposed):
    """Entries of a rank's item half of A (user -> item edges of its own users) or of A^T (item -> user edges to them)."""
    lo, hi = case.ranges[rank]
    src, dst = case.ei[0], case.ei[1]
    if transposed:
        return int(((dst >= lo) & (dst < hi) & (src >= case.n_users)).sum())
    return int(((src >= lo) & (src < hi) & (dst >= case.n_users)).sum())


@pytest.mark.parametrize("name,world", [("skew", 2), ("skew", 3), ("hub_first", 2)])
def test_forced_sweep_over_a_ranks_own_columns(device, monkeypatch, name, world):
    """LGCN_SWEEP=1 with the small planner configuration: a rank's item half sweeps the columns [u0, u1) of its own users
    exactly where ``Operator.build``'s rule says so -- on ``skew`` at world 3 the first two ranks (the second with
    u0 > 0) and not the third; on ``hub_first`` rank 0 sweeps ONE column -- and the whole partitioned sum still holds."""
    S.force_small_sweep(monkeypatch, G)
    case = case_of(device, name, world, "forced_sweep")
    swept = []
    for rank, pp in enumerate(case.pps):
        for transposed, op in ((False, pp.item_op), (True, pp._transposed_ops()[1])):
            want = S.sweeps_when_forced(item_entries(case, rank, transposed), case.n_items)
            assert op.sweep_cols == (tuple(case.ranges[rank]) if want else None), (rank, transposed, op.sweep_cols)
            swept.append(want)
    if name == "skew":
        assert swept == ([True] * 4 if world == 2 else [True, True, True, True, False, False]), swept
    else:
        assert swept[:2] == [True, True] and case.ranges[0] == (0, 1), (swept, case.ranges)
    sums(case, device, SWEPT_DIMS, "RATIO_SWEEP")
    for rank, pp in enumerate(case.pps):
        if pp.item_op.sweep_cols is not None:
            x = table(device, name, 64)
            assert pp.item_op.route(x, torch.empty_like(x)).startswith("sweep"), rank
            assert pp.item_op._sweep, (rank, "the forced sweep built no plan")


STEP_CASES = [(name, world) for name in ("skew", "directed", "isolated_ends") for world in (2, 3)]


@pytest.mark.parametrize("pays", (True, False), ids=("listed_item_step", "full_item_step"))
@pytest.mark.parametrize("name,world", STEP_CASES)
def test_step_halves_against_fp64_autograd(device, monkeypatch, name, world, pays):
    """``step_forward`` + ``step_backward`` on every rank: bpr, reg and the gradient of the own rows against fp64; at world
    3 the middle rank owns no triple of the batch."""
    monkeypatch.setattr(propagate, "SEED_ROWS_FACTOR", 1)
    monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", 1e9 if pays else 0.0)
    case = case_of(device, name, world)
    for dim in (64, 90):
        for k in (3, 5):
            worst = S.check_step(case, dim, k, table(device, name, dim, 1))
            lg.check_index_status()
            print(f"\nSTEP {name} world {world} D={dim} K={k}: worst rel_fro {worst:.2e}")


@pytest.mark.parametrize("name,world", [("hub_last", 3), ("hub_first", 5), ("few_users", 8)])
def test_trainer_refuses_an_empty_range_on_every_rank(device, name, world):
    case = case_of(device, name, world)
    assert case.has_empty_range
    w = table(device, name, 64, 1).clone()
    raised = [None] * world

    def body(rank):
        torch.cuda.set_device(device)
        try:
            PartitionedTrainer(case.pps[rank], w, S.alphas_of(3, True), batch=64)
        except ValueError as exc:
            raised[rank] = str(exc)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(msg is not None and "cannot train" in msg for msg in raised), raised


def test_loss_takes_the_dense_path_when_a_range_is_empty(device, monkeypatch):
    """The gate of ``partitioned_bpr_loss`` reads ``pp.ranges``: a world-1 propagator with a hand-made list of ranges
    shows it (no collective runs at world 1); either path gives the fp64 loss and gradient."""
    monkeypatch.setattr(propagate, "SEED_ROWS_FACTOR", 0)
    name = "isolated_ends"
    ei, ew, nu, ni = S.graph(name)
    pp = PartitionedPropagator(ei.to(device), ew.to(device), nu, ni, 0, 1)
    users, pos, neg = S.triples(name)
    alphas = S.alphas_of(3, True)
    coo = case_of(device, name, 1).coo(False)
    for ranges, seeded in (([(0, nu)], True), ([(0, nu), (nu, nu)], False)):
        pp.ranges = ranges
        w = table(device, name, 64, 1).clone().requires_grad_(True)
        local, _, _ = partitioned_bpr_loss(pp, w, alphas, users.to(device), pos.to(device), neg.to(device), 1e-4)
        assert S.uses_node(local.grad_fn, "PartitionedStep") == seeded, ranges
        local.backward()
        lg.check_index_status()
        bpr, reg, grad = S.step_fp64(w.detach().cpu(), coo, alphas, users, pos, neg, 1e-4)
        assert abs(local.item() - (bpr + reg)) <= 1e-5 * abs(bpr + reg)
        assert ((w.grad.cpu().double() - grad).norm() / grad.norm()).item() <= 1e-5
