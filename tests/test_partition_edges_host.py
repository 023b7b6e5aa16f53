"""``partition.PartitionedPropagator`` on awkward partitions -- empty ranges, a one-user range, isolated rows at both
ends, a directed edge list -- with the arithmetic of the CPU test double (tests/cpu_ops.py) and the ranks as threads: what
is under test here is partition.py itself; the same cases run through the HIP kernels in
tests/test_partition_edges_gpu.py.  Graphs, references and checks: tests/partition_edges_support.py.

Every sum is compared row by row against fp64, ||got_r - want_r|| <= 1e-5 ||mag_r||, the project's gate on a propagation.
"""
import threading

import pytest
import torch

import partition_edges_support as S
from cpu_ops import CpuOps
from gnn_ecommerce_amd import graph as G, propagate
from gnn_ecommerce_amd.partition import PartitionedPropagator, balanced_user_ranges, partitioned_bpr_loss
from gnn_ecommerce_amd.trainer import PartitionedTrainer

DIMS = (3, 7)
CASES = [(name, world) for name in S.GRAPHS for world in S.WORLDS]
_cases = {}


def case_of(name, world):
    if (name, world) not in _cases:
        _cases[(name, world)] = S.Case(name, world, CpuOps)
    return _cases[(name, world)]


@pytest.mark.parametrize("degrees,world,want", [
    ([90, 1, 1, 1, 1, 1, 1, 1, 1, 2], 4, [(0, 1), (1, 1), (1, 1), (1, 10)]),
    ([1, 1, 1, 1, 1, 1, 1, 1, 2, 90], 4, [(0, 10), (10, 10), (10, 10), (10, 10)]),
    ([3, 2, 1], 5, [(0, 1), (1, 1), (1, 2), (2, 2), (2, 3)]),
    ([0, 0, 0], 2, [(0, 1), (1, 3)])])
def test_cuts_of_awkward_degree_vectors(degrees, world, want):
    """Cut k sits right after the first user whose cumulative degree reaches k / world of the total."""
    assert balanced_user_ranges(torch.tensor(degrees), world) == want == S.expected_ranges(degrees, world)


@pytest.mark.parametrize("name,world", CASES)
def test_partition_tiles_users_and_entries(name, world):
    S.check_partition(case_of(name, world))


@pytest.mark.parametrize("name,world", CASES)
def test_forward_and_transposed_sums_row_by_row_against_fp64(name, world):
    case = case_of(name, world)
    for dim in DIMS:
        x0 = S.table(name, dim)
        for k in S.LAYERS:
            for equal in (True, False):
                for transpose in (False, True):
                    S.check_sum(case, dim, k, equal, transpose, x0)


@pytest.mark.parametrize("name,world", CASES)
def test_one_hop_with_an_epilogue_row(name, world):
    """``hop``: the b * r term of the exchanged item block is added by one rank only."""
    case = case_of(name, world)
    for dim in DIMS:
        x, r = S.table(name, dim), S.table(name, dim, seed=2)
        S.check_hop(case, dim, x, r, x, r)


@pytest.mark.parametrize("pays", (True, False), ids=("listed_item_step", "full_item_step"))
@pytest.mark.parametrize("name,world", CASES)
def test_listed_rows_against_fp64(monkeypatch, name, world, pays):
    """``final_rows`` / ``final_item_rows`` with the listed-rows rule forced either way: repeated ids, foreign users
    clamped into the rank's range (onto a foreign user where the range is empty), item ids outside the item block."""
    monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", 1e9 if pays else 0.0)
    monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", True)
    case = case_of(name, world)
    for dim, equal in zip(DIMS, (True, False)):
        x0 = S.table(name, dim)
        for k in S.LAYERS:
            S.check_listed(case, dim, k, equal, False, x0, pays)
        S.check_listed(case, dim, 3, not equal, True, x0, pays)


@pytest.mark.parametrize("name,world", [(n, w) for n, w in CASES if w in (1, 3)])
def test_repeated_listed_items_take_the_maximum_over_their_positions(monkeypatch, name, world):
    """The ``index_reduce_(..., "amax")`` write-back under an exchange that sums every list position differently."""
    monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", 1e9)
    monkeypatch.setattr(propagate, "SCORED_ITEM_ROWS_ONLY", True)
    case = case_of(name, world)
    for k, equal in ((1, False), (3, True), (5, False)):
        S.check_repeats_take_the_maximum(case, 7, k, equal, S.table(name, 7))


EMPTY = [(n, w) for n, w in CASES if any(hi <= lo for lo, hi in balanced_user_ranges(
    S.user_degrees(S.graph(n)[0], S.graph(n)[2]), w))]


@pytest.mark.parametrize("pays", (True, False), ids=("listed_item_step", "full_item_step"))
@pytest.mark.parametrize("name,world", [c for c in CASES if c not in EMPTY])
def test_step_halves_against_fp64_autograd(monkeypatch, name, world, pays):
    """Every partition without an empty range (one with an empty range cannot train: the tests below)."""
    case = case_of(name, world)
    monkeypatch.setattr(G, "LISTED_ROWS_MAX_SHARE", 1e9 if pays else 0.0)
    for dim, k in zip(DIMS, (1, 3)):
        S.check_step(case, dim, k, S.table(name, dim, seed=1))


def test_some_partitions_have_empty_ranges():
    assert ("hub_last", 3) in EMPTY and ("hub_first", 5) in EMPTY and ("few_users", 8) in EMPTY and len(EMPTY) >= 8
    assert case_of("hub_first", 2).ranges == [(0, 1), (1, S.HUB_USERS)]         # a one-user range that does train


@pytest.mark.parametrize("name,world", EMPTY)
def test_trainer_refuses_an_empty_range_on_every_rank(name, world):
    """One rank raising alone would leave its peers waiting in the first all-reduce: every rank refuses, so no step is
    ever started here (the barrier of the thread ranks would time the test out otherwise)."""
    case = case_of(name, world)
    w = S.table(name, 7, seed=1).clone()
    raised = [None] * world
    barrier = threading.Barrier(world)

    def body(rank):
        try:
            PartitionedTrainer(case.pps[rank], w, S.alphas_of(3, True), batch=64)
        except ValueError as exc:
            raised[rank] = str(exc)
        barrier.wait(timeout=30)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(msg is not None and "cannot train" in msg for msg in raised), raised


def test_loss_takes_the_dense_path_when_a_range_is_empty(monkeypatch):
    """The gate of ``partitioned_bpr_loss`` reads ``pp.ranges``: a world-1 propagator with a hand-made list of ranges
    shows it (no collective runs at world 1)."""
    from oracle import lightgcn_oracle as oracle
    monkeypatch.setattr(propagate, "SEED_ROWS_FACTOR", 0)
    monkeypatch.setattr(propagate, "pair_dot", oracle.pair_scores)              # the dense path's scores, on the host
    ei, ew, nu, ni = S.graph("isolated_ends")
    pp = PartitionedPropagator(ei, ew, nu, ni, 0, 1, ops=CpuOps())
    users, pos, neg = S.triples("isolated_ends")
    alphas = S.alphas_of(3, True)
    for ranges, seeded in (([(0, nu)], True), ([(0, nu), (nu, nu)], False)):
        pp.ranges = ranges
        w = S.table("isolated_ends", 7, seed=1).clone().requires_grad_(True)
        local, _, _ = partitioned_bpr_loss(pp, w, alphas, users, pos, neg, 1e-4)
        assert S.uses_node(local.grad_fn, "PartitionedStep") == seeded, ranges
        local.backward()
        bpr, reg, grad = S.step_fp64(w.detach(), S.Case.coo(case_of("isolated_ends", 1), False), alphas, users, pos, neg, 1e-4)
        assert abs(local.item() - (bpr + reg)) <= 1e-5 * abs(bpr + reg)
        assert ((w.grad.double() - grad).norm() / grad.norm()).item() <= 1e-5
