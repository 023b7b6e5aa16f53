"""Awkward partitions for ``partition.PartitionedPropagator``: small named graphs whose nnz-balanced user cuts come out
empty, one user wide or lopsided, thread ranks that stand in for a process group, fp64 references on the host and the
checks that tests/test_partition_edges_host.py (``CpuOps``) and tests/test_partition_edges_gpu.py (``HipOps``) share.

Every graph is a directed edge list in the reference's layout (edge_index int64 [2, E], row 0 = source, row 1 = target,
users first), built without a random seed that could drift: ``numpy.random.default_rng`` with a constant.  Weights lie in
[0.5, 1.5].  Both directions of a (user, item) pair are present unless the graph says otherwise.

The references are computed from the operator's own fp32 edge values (``edge_values`` of a rank's global build, asserted
bit-equal across the ranks): ``want`` = sum_l alpha_l M^l x0 and ``mag`` = sum_l |alpha_l| |M|^l |x0| for M = A or A^T.
The gate on a row r is ||got_r - want_r||_2 <= TOL ||mag_r||_2 with TOL = 1e-5, the project's gate on a propagation.

Nothing here needs a device to be imported.
"""
import threading

import numpy as np
import torch

import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import synth
from gnn_ecommerce_amd import partition
from gnn_ecommerce_amd.partition import ITEM_SHORT_MAX, PartitionedPropagator, balanced_user_ranges
from layer_sum_support import SMALL_PLAN, mag_fp64, row_ratios, want_fp64

TOL = 1e-5
WORLDS = (1, 2, 3, 5, 8)
LAYERS = (1, 3, 5)


def _where(mask):
    """The positions of a bool vector's True entries, int64."""
    return mask.nonzero().view(-1)


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
def _edges(n_users, pairs, seed, keep_item_to_user=None):
    """(edge_index, edge_weight) of the (user, item) pairs in list order: first the item -> user direction of every pair
    (an entry of the USER's row), then the user -> item direction (an entry of the ITEM's row).  ``keep_item_to_user``:
    bool per pair, False = that pair's item -> user direction is left out."""
    u = np.array([p[0] for p in pairs], dtype=np.int64)
    i = np.array([p[1] for p in pairs], dtype=np.int64) + n_users
    keep = np.ones(len(pairs), dtype=bool) if keep_item_to_user is None else np.asarray(keep_item_to_user, dtype=bool)
    src, dst = np.concatenate([i[keep], u]), np.concatenate([u[keep], i])
    rng = np.random.default_rng(seed)
    ew = rng.uniform(0.5, 1.5, src.size).astype(np.float32).clip(0.5, 1.5)
    return torch.from_numpy(np.stack([src, dst])), torch.from_numpy(ew)


HUB_USERS, HUB_ITEMS, HUB_REPEATS = 41, 45, 8


def _hub(hub):
    others = [u for u in range(HUB_USERS) if u != hub]
    pairs = [(hub, i) for _ in range(HUB_REPEATS) for i in range(HUB_ITEMS)]
    pairs += [(u, (7 * k) % HUB_ITEMS) for k, u in enumerate(others)]          # 40 distinct items, one entry per user
    assert HUB_REPEATS * HUB_ITEMS > 7 * len(others)                           # every cut of up to 8 ranks lands on the hub
    return (*_edges(HUB_USERS, pairs, 41 + hub), HUB_USERS, HUB_ITEMS)


def hub_first():
    """41 x 45.  User 0 holds 360 of 400 entries: its pair with every item is listed 8 times (duplicate entries), every
    other user has one entry.  Rank 0 owns user 0 alone -- each of its item rows is a slice of 8 entries over ONE column --
    and at worlds 3, 5, 8 every rank but the first and the last is empty."""
    return _hub(0)


def hub_last():
    """The same with the hub as the last user: every cut lands at n_users, rank 0 owns everything."""
    return _hub(HUB_USERS - 1)


def isolated_ends():
    """120 x 20.  The first 5 and the last 10 users have no entries, nor have the first and the last item."""
    rng = np.random.default_rng(120)
    pairs = []
    for u in range(5, 110):
        for i in rng.choice(np.arange(1, 19), size=1 + u % 6, replace=False):
            pairs.append((u, int(i)))
    return (*_edges(120, pairs, 121), 120, 20)


def few_users():
    """3 users, 4 items, 6 pairs, user degrees 3, 2, 1: more ranks than users at worlds 5 and 8."""
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 3), (2, 0)]
    return (*_edges(3, pairs, 3), 3, 4)


def directed():
    """150 x 30, user degrees 1 .. 7, every second item -> user direction missing: A is not structurally symmetric, the
    halves of A^T are not those of A, and some users are named by item rows without having a row of their own."""
    rng = np.random.default_rng(150)
    pairs = []
    for u in range(150):
        for i in rng.choice(30, size=1 + u % 7, replace=False):
            pairs.append((u, int(i)))
    keep = np.arange(len(pairs)) % 2 == 0
    return (*_edges(150, pairs, 151, keep), 150, 30)


SKEW_USERS, SKEW_ITEMS = 700, 45


def skew_degree(u):
    """User degrees 1 .. 12: one entry (item 0) for most, every 11th user a longer list cycling through 2 .. 12."""
    return 2 + (u // 11 + 1) % 11 if u % 11 == 6 else 1


def skew():
    """700 x 45, item 0 in every user's list.  1,084 entries: at world 3 the ranks' item halves hold 362, 370 and 352, on
    either side of the 8 entries per row that the ``long_rows`` rule of ``Operator.build`` asks for -- the ranks over
    [0, u1) and [u0 > 0, u1) sweep when forced, the last one does not --, and item 0's slice of about 230 entries sits
    beside slices of a few (both facts asserted by ``skew_facts``)."""
    rng = np.random.default_rng(700)
    pairs = []
    for u in range(SKEW_USERS):
        pairs.append((u, 0))
        for i in rng.choice(np.arange(1, SKEW_ITEMS), size=skew_degree(u) - 1, replace=False):
            pairs.append((u, int(i)))
    return (*_edges(SKEW_USERS, pairs, 701), SKEW_USERS, SKEW_ITEMS)


GRAPHS = {"hub_first": hub_first, "hub_last": hub_last, "isolated_ends": isolated_ends, "few_users": few_users,
          "directed": directed, "skew": skew}
SMALL_GRAPHS = ("hub_first", "hub_last", "isolated_ends", "few_users", "directed")
_graphs = {}


def graph(name):
    """(edge_index, edge_weight, n_users, n_items) on the host, built once."""
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def user_degrees(ei, n_users):
    """Entries per user row of A (what ``PartitionedPropagator`` balances the ranges by), int64 on the host."""
    dst = ei[1]
    return torch.bincount(dst[dst < n_users], minlength=n_users)[:n_users]


def expected_ranges(deg, world):
    """``balanced_user_ranges`` as its docstring states it, in plain Python: cut k is the first user whose cumulative
    degree reaches k / world of the total (that user included), never below the cut before it."""
    deg = [int(d) for d in deg]
    n, total = len(deg), sum(deg)
    cuts = [0]
    for k in range(1, world):
        target = -(-total * k // world)
        run, cut = 0, n
        for u, d in enumerate(deg):
            run += d
            if run >= target:
                cut = u + 1
                break
        cuts.append(max(min(cut, n), cuts[-1]))
    cuts.append(n)
    return [(cuts[k], cuts[k + 1]) for k in range(world)]


def item_slice_lengths(ei, n_users, n_items, lo, hi):
    """Entries per item row among the sources [lo, hi): the rows of a rank's item operator."""
    src, dst = ei[0], ei[1]
    mine = (dst >= n_users) & (src >= lo) & (src < hi)
    return torch.bincount(dst[mine] - n_users, minlength=n_items)


def sweeps_when_forced(n_entries, n_rows):
    """``Operator.build``'s rule with the sweep forced on (USE_SWEEP "1"): the rows must hold 8 entries each on average."""
    return n_entries >= 8 * max(n_rows, 1)


def skew_facts():
    """What ``skew`` is for, from its CSR; a later edit of the graph cannot lose these silently."""
    ei, _, nu, ni = graph("skew")
    deg = user_degrees(ei, nu)
    assert int(deg.min()) == 1 and int(deg.max()) == 12 and set(deg.tolist()) == set(range(1, 13))
    assert int(item_slice_lengths(ei, nu, ni, 0, nu)[0]) == nu                  # item 0 is in every user's list
    ranges = balanced_user_ranges(deg, 3)
    both, forced = [], []
    for lo, hi in ranges:
        lens = item_slice_lengths(ei, nu, ni, lo, hi)
        both.append(bool((lens > ITEM_SHORT_MAX).any()) and bool(((lens > 0) & (lens <= ITEM_SHORT_MAX)).any()))
        forced.append(sweeps_when_forced(int(lens.sum()), ni))
    assert all(both), "every rank's item half holds slices beyond ITEM_SHORT_MAX beside shorter ones"
    assert any(forced[1:]) and not all(forced), (forced, "a rank beyond the first must pass long_rows and one must not")
    return forced


skew_facts()


# ---------------------------------------------------------------------------------------------------------------------
# thread ranks
# ---------------------------------------------------------------------------------------------------------------------
class _ThreadComm:
    """Stand-in for partition.Comm when the ranks of a partition are THREADS of one process sharing one device and one
    stream: a collective = barrier, rank 0 sums the ranks' tensors, barrier, every rank copies the sum.
    All launches go to the same stream in the order the barriers impose, so no device synchronisation is needed."""

    def __init__(self, rank, world, shared):
        self.rank, self.world, self.shared = rank, world, shared

    def _total(self, slots):
        total = slots[0].clone()
        for other in slots[1:]:
            total += other
        return total

    def _sum(self, t):
        sh = self.shared
        sh["slots"][self.rank] = t
        sh["barrier"].wait()
        if self.rank == 0:
            sh["total"] = self._total(sh["slots"])
        sh["barrier"].wait()
        t.copy_(sh["total"])
        sh["barrier"].wait()

    def start(self, block):
        self._sum(block)
        return None

    def wait(self, handle):
        pass

    def reduce_now(self, t):
        self._sum(t)


class _PerturbingComm(_ThreadComm):
    """A thread all-reduce that associates differently per list position, as a ring does per chunk: the sum of a
    [``length``, D] table (the listed item rows; no other exchanged tensor has that many rows) leaves position m scaled by
    1 + (m % 5 - 2) * 2^-18.  ``level``: afterwards every position of a repeated id holds the elementwise maximum over the
    id's positions -- the table a reduction by "amax" must behave as if it had been given."""

    def __init__(self, rank, world, shared, ids, level):
        super().__init__(rank, world, shared)
        self.ids, self.level = ids, level

    def _total(self, slots):
        total = super()._total(slots)
        if total.dim() == 2 and total.size(0) == self.ids.numel():
            m = torch.arange(total.size(0), device=total.device)
            total *= (1.0 + (m % 5 - 2).to(total.dtype) * 2.0 ** -18).view(-1, 1)
            if self.level:
                ids = self.ids.to(total.device)
                top = torch.full((int(ids.max()) + 1, total.size(1)), float("-inf"), dtype=total.dtype, device=total.device)
                top.index_reduce_(0, ids, total, "amax", include_self=True)
                total = top[ids]
        return total


def _run_thread_ranks(world, fn, device=None, comm=_ThreadComm):
    """``fn(rank, comm)`` on ``world`` threads; returns the ranks' results.  ``device``: the CUDA device every thread
    selects first (None: host tensors only).  ``comm(rank, world, shared)`` makes a rank's communicator."""
    shared = {"slots": [None] * world, "barrier": threading.Barrier(world), "total": None}
    results, errors = [None] * world, []

    def body(rank):
        try:
            if device is not None:
                torch.cuda.set_device(device)
            results[rank] = fn(rank, comm(rank, world, shared))
        except BaseException as exc:                      # a failing rank must not leave the others at a barrier
            errors.append((rank, exc))
            shared["barrier"].abort()

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    real = [e for e in errors if not isinstance(e[1], threading.BrokenBarrierError)]
    assert not real, real
    return results


# ---------------------------------------------------------------------------------------------------------------------
# partitions, inputs and fp64 references
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One graph cut into ``world`` ranks: the propagators (every table they hand out NaN-filled), the COO of A from the
    operator's own fp32 values on the host, and what the graph promises."""

    def __init__(self, name, world, make_ops, device=None):
        ei, ew, nu, ni = graph(name)
        self.name, self.world, self.device = name, world, device
        self.n_users, self.n_items, self.n = nu, ni, nu + ni
        self.ei = ei
        dev = device if device is not None else "cpu"
        ei_d, ew_d = ei.to(dev), ew.to(dev)
        self.pps = [PartitionedPropagator(ei_d, ew_d, nu, ni, r, world, ops=make_ops()) for r in range(world)]
        for pp in self.pps:
            nan_tables(pp)
        vals = [pp._coo[1] for pp in self.pps]
        assert all(v.dtype == torch.float32 and torch.equal(v, vals[0]) for v in vals), "edge values differ between ranks"
        self.vals = vals[0].cpu().double()
        self.ranges = self.pps[0].ranges
        assert all(pp.ranges == self.ranges for pp in self.pps)
        self.has_empty_range = any(hi <= lo for lo, hi in self.ranges)

    def coo(self, transpose):
        """(rows, cols, vals fp64) of M = A (rows are the targets) or A^T."""
        src, dst = self.ei[0], self.ei[1]
        return (src, dst, self.vals) if transpose else (dst, src, self.vals)

    def rows_without_entries(self, transpose):
        rows = self.coo(transpose)[0]
        return _where(torch.bincount(rows, minlength=self.n) == 0)

    def own_mask(self, rank):
        """bool [N]: the rows a rank's result is defined on -- its users and the item block."""
        lo, hi = self.ranges[rank]
        own = torch.zeros(self.n, dtype=torch.bool)
        own[lo:hi] = True
        own[self.n_users:] = True
        return own

    def run(self, fn, comm=_ThreadComm):
        """``fn(pp, rank)`` on every rank as a thread, the propagators' communicators replaced for the call."""
        def body(rank, c):
            pp = self.pps[rank]
            pp.comm = c
            return fn(pp, rank)
        return _run_thread_ranks(self.world, body, self.device, comm)


def nan_tables(pp):
    """Every internal table ``pp._tables`` hands out is NaN-filled before each call: a foreign user row (or a stale block
    of an earlier call) read by mistake poisons the result."""
    if getattr(pp, "_nan_tables", False):
        return
    real = pp._tables

    def tables(like, count, tag):
        got = real(like, count, tag)
        for t in got:
            t.fill_(float("nan"))
        return got
    pp._tables = tables
    pp._nan_tables = True


_inputs, _refs = {}, {}


def table(name, dim, seed=0):
    """The input table of a (graph, width) on the host; never written to."""
    key = (name, dim, seed)
    if key not in _inputs:
        _, _, nu, ni = graph(name)
        _inputs[key] = synth.xavier_table(nu + ni, dim, 1000 + 10 * dim + seed)
    return _inputs[key]


def alphas_of(k, equal):
    """K + 1 weights: the reference's 1 / (K + 1), or a falling sequence of all different values."""
    from eliminate_support import alphas_for
    return alphas_for(k, equal)


def references(case, dim, k, equal, transpose):
    """(want, mag) in fp64 on the host, once per (graph, K, alphas, D, direction): the edge values are the same on every
    partition of a graph (asserted bit-equal per case against the first one seen)."""
    first = _refs.setdefault(("vals", case.name), case.vals)
    assert torch.equal(first, case.vals), "the edge values of a graph must not depend on the partition"
    key = (case.name, dim, k, equal, transpose)
    if key not in _refs:
        alphas, x0 = alphas_of(k, equal), table(case.name, dim)
        _refs[key] = (want_fp64(*case.coo(transpose), x0, alphas), mag_fp64(*case.coo(transpose), x0, alphas))
    return _refs[key]


def check_rows(got, rows, want, mag, label):
    """The per-row gate on ``rows`` (int64 ids) of ``got`` (host, [N, D]); returns the worst ratio."""
    if rows.numel() == 0:
        return 0.0
    g = got[rows]
    assert not torch.isnan(g).any(), (label, "NaN in a compared row: a foreign or stale row was read")
    ratios = row_ratios(g, want[rows], mag[rows])
    worst = float(ratios.max())
    assert worst <= TOL, (label, worst, int(rows[int(ratios.argmax())]))
    return worst


def check_exact(got, rows, expect, label):
    """Rows without entries: exactly the given fp32 rows."""
    if rows.numel():
        assert expect.dtype == torch.float32 and torch.equal(got[rows], expect[rows]), (label, "a row without entries")


def check_foreign_zero(case, got, rank, label):
    lo, hi = case.ranges[rank]
    foreign = torch.ones(case.n_users, dtype=torch.bool)
    foreign[lo:hi] = False
    assert bool((got[:case.n_users][foreign] == 0).all()), (label, "foreign user rows must be exactly zero")


def check_partition(case):
    """The ranges are the documented cuts, tile [0, n_users), and the ranks' item halves hold every item-row entry once."""
    deg = user_degrees(case.ei, case.n_users)
    assert case.ranges == expected_ranges(deg, case.world), (case.name, case.world, case.ranges)
    assert case.ranges[0][0] == 0 and case.ranges[-1][1] == case.n_users
    assert all(a[1] == b[0] for a, b in zip(case.ranges, case.ranges[1:])) and all(lo <= hi for lo, hi in case.ranges)
    # local_nnz counts a rank's item-row entries twice (the symmetric edge list of the product: both directions)
    item_entries = int((case.ei[1] >= case.n_users).sum())
    assert sum(pp.local_nnz for pp in case.pps) == 2 * item_entries
    if case.name != "directed":
        assert sum(pp.local_nnz for pp in case.pps) == case.ei.size(1)          # == nnz where both directions are present


def check_sum(case, dim, k, equal, transpose, x0_dev, again=False):
    """One forward or transposed sum on every rank with ``zero_foreign_rows=True`` against fp64; returns the worst ratio.
    ``again``: a second call must give the same bits on the compared rows."""
    alphas = alphas_of(k, equal)
    want, mag = references(case, dim, k, equal, transpose)
    x0 = table(case.name, dim)
    exact = torch.tensor(alphas[0]) * x0
    empty = case.rows_without_entries(transpose)
    label = (case.name, case.world, dim, k, equal, "A^T" if transpose else "A")

    def body(pp, rank):
        out = pp.propagate_sum(x0_dev, alphas, transpose=transpose, zero_foreign_rows=True)
        second = pp.propagate_sum(x0_dev, alphas, transpose=transpose, zero_foreign_rows=True) if again else None
        return out, second

    worst = 0.0
    for rank, (out, second) in enumerate(case.run(body)):
        got, own = out.cpu(), case.own_mask(rank)
        rows = _where(own)
        worst = max(worst, check_rows(got, rows, want, mag, label + (rank,)))
        check_exact(got, empty[own[empty]], exact, label + (rank,))
        check_foreign_zero(case, got, rank, label + (rank,))
        if second is not None:
            assert torch.equal(second.cpu()[rows], got[rows]), (label, rank, "two calls must give the same bits")
    return worst


def listed_ids(case, seed=5):
    """(user ids, item node ids), int64 on the host, 24 each: users from everywhere with a repeat -- every rank clamps them
    into its own range as ``step_forward`` does --, items with repeats at positions whose exchanged rows differ
    (``_PerturbingComm``), the first and the last item, and ids outside the item block on either side, which
    ``propagate_sum`` clamps into it."""
    rng = np.random.default_rng(seed)
    nu, ni, n = case.n_users, case.n_items, case.n
    users = rng.integers(0, nu, 24)
    users[1] = users[0]
    items = rng.integers(0, ni, 24) + nu
    items[0], items[1], items[2] = nu + ni // 2, nu + ni // 2, nu + ni // 2      # positions 0, 1, 2: scaled down, down, not
    items[3], items[4] = nu, n - 1
    items[5], items[6] = 0, n + 3                                               # clamped to the first / the last item
    items[7] = items[23]
    return torch.from_numpy(users), torch.from_numpy(items)


def check_listed(case, dim, k, equal, transpose, x0_dev, pays, again=False, comm=_ThreadComm):
    """The sum for listed rows only (``final_rows``, ``final_item_rows``): the listed own users and the listed items --
    the whole item block when the listed item step does not pay -- carry the per-row gate.  Returns the ranks' results."""
    alphas = alphas_of(k, equal)
    want, mag = references(case, dim, k, equal, transpose)
    x0 = table(case.name, dim)
    exact = torch.tensor(alphas[0]) * x0
    empty = case.rows_without_entries(transpose)
    users, items = listed_ids(case)
    items_clamped = items.clamp(case.n_users, case.n - 1)
    label = (case.name, case.world, dim, k, equal, "A^T" if transpose else "A", "listed", pays)
    dev = x0_dev.device

    def body(pp, rank):
        assert pp.listed_rows_pay(2 * items.numel()) == pays
        uc = users.clamp(pp.u0, pp.u1 - 1).to(dev)
        kw = dict(transpose=transpose, zero_foreign_rows=True, final_rows=uc, final_item_rows=items.to(dev))
        out = pp.propagate_sum(x0_dev, alphas, **kw)
        return out, (pp.propagate_sum(x0_dev, alphas, **kw) if again else None)

    results = case.run(body, comm)
    if comm is not _ThreadComm:
        return results
    for rank, (out, second) in enumerate(results):
        lo, hi = case.ranges[rank]
        got = out.cpu()
        mine = users.clamp(lo, hi - 1)
        mine = torch.unique(mine[(mine >= lo) & (mine < hi)])                 # (an empty range clamps onto a foreign user)
        item_rows = torch.unique(items_clamped) if pays else torch.arange(case.n_users, case.n)
        rows = torch.cat([mine, item_rows])
        check_rows(got, rows, want, mag, label + (rank,))
        check_exact(got, rows[torch.isin(rows, empty)], exact, label + (rank,))
        check_foreign_zero(case, got, rank, label + (rank,))
        if second is not None:
            assert torch.equal(second.cpu()[rows], got[rows]), (label, rank, "two calls must give the same bits")
    return results


def check_repeats_take_the_maximum(case, dim, k, equal, x0_dev):
    """The write-back of the listed item rows when the exchange leaves the positions of a repeated id with different
    sums: the row must be the elementwise maximum over its positions whatever order the writes land in -- the bits of
    the same call on an exchanged table whose repeats already agree on that maximum."""
    users, items = listed_ids(case)
    ids = items.clamp(case.n_users, case.n - 1)
    x0 = table(case.name, dim)
    assert ids[0] == ids[1] == ids[2] and bool((x0[ids[0]] > 0).any()) and bool((x0[ids[0]] < 0).any())

    def make(level):
        return lambda rank, world, shared: _PerturbingComm(rank, world, shared, ids, level)

    plain = check_listed(case, dim, k, equal, False, x0_dev, True)
    raw = check_listed(case, dim, k, equal, False, x0_dev, True, comm=make(False))
    level = check_listed(case, dim, k, equal, False, x0_dev, True, comm=make(True))
    rows = torch.unique(ids)
    for rank in range(case.world):
        a, b, c = raw[rank][0].cpu()[rows], level[rank][0].cpu()[rows], plain[rank][0].cpu()[rows]
        assert not torch.isnan(a).any() and torch.equal(a, b), (case.name, case.world, dim, k, equal, rank)
        if k > 0 and bool((case.vals != 0).any()):
            assert not torch.equal(a, c), "the perturbed exchange must have changed the listed rows"


def check_hop(case, dim, x_dev, r_dev, x, r, a=0.5, b=0.25):
    """``pp.hop``: out = a A x + b r on the own users and the item block -- the epilogue row enters the exchanged item
    block on ONE rank -- against fp64, rows without entries exactly fl(b r)."""
    coo = case.coo(False)
    want = want_fp64(*coo, x, (0.0, a)) + b * r.double()
    mag = mag_fp64(*coo, x, (0.0, a)) + abs(b) * r.double().abs()
    exact = torch.tensor(b) * r
    empty = case.rows_without_entries(False)

    def body(pp, rank):
        out = torch.full_like(x_dev, float("nan"))
        return pp.hop(x_dev, out, a, r_dev, b)

    for rank, out in enumerate(case.run(body)):
        got, own = out.cpu(), case.own_mask(rank)
        label = (case.name, case.world, dim, "hop", rank)
        check_rows(got, _where(own), want, mag, label)
        check_exact(got, empty[own[empty]], exact, label)


# ---------------------------------------------------------------------------------------------------------------------
# one training step
# ---------------------------------------------------------------------------------------------------------------------
def loss_fp64(w, coo, alphas, users, pos, neg, decay):
    """(scores, loss) of one training step in fp64 on the host: the layer sum, the pair dots, then the model's own loss
    expressions (``BPRLoss``, ``regularization_loss``) on plain torch ops."""
    rows, cols, vals = coo
    x = w
    out = alphas[0] * x
    for alpha in alphas[1:]:
        x = torch.zeros_like(x).index_add(0, rows, vals.view(-1, 1) * x[cols])
        out = out + alpha * x
    b = users.numel()
    scores = (out[torch.cat([users, users])] * out[torch.cat([pos, neg])]).sum(-1)
    return scores, lg.BPRLoss(0)(scores[:b], scores[b:]) * b + lg.regularization_loss(w, b, users, pos, neg, decay)


def step_fp64(w, coo, alphas, users, pos, neg, decay):
    """(bpr, reg, gradient of bpr + reg) of one step of src/train_lightgcn.py in fp64: ``loss_fp64`` and its two terms."""
    w64 = w.double().requires_grad_(True)
    _, loss = loss_fp64(w64, coo, alphas, users, pos, neg, decay)
    loss.backward()
    with torch.no_grad():
        reg = lg.regularization_loss(w64, users.numel(), users, pos, neg, decay)
    return float(loss.detach() - reg), float(reg), w64.grad


def triples(name):
    """One batch of 64 (user, positive, negative) triples on the host, node ids: a repeated user, a repeated item, a
    triple with pos == neg, a user and an item without entries where the graph has them, and the users drawn so that at
    world 3 the middle rank owns no triple (where that partition has no empty range)."""
    ei, _, nu, ni = graph(name)
    deg = user_degrees(ei, nu)
    ranges = balanced_user_ranges(deg, 3)
    allowed = torch.ones(nu, dtype=torch.bool)
    if all(hi > lo for lo, hi in ranges):
        allowed[ranges[1][0]:ranges[1][1]] = False
    pool = _where(allowed)
    rng = torch.Generator().manual_seed(64 + nu)
    users = pool[torch.randint(0, pool.numel(), (64,), generator=rng)]
    pos = torch.randint(0, ni, (64,), generator=rng) + nu
    neg = torch.randint(0, ni, (64,), generator=rng) + nu
    users[1] = users[0]
    pos[3] = pos[2]
    neg[4] = pos[4]
    touched = torch.bincount(torch.cat([ei[0], ei[1]]), minlength=nu + ni) > 0
    lonely_users = _where(~touched[:nu] & allowed)
    lonely_items = _where(~touched[nu:]) + nu
    if lonely_users.numel():
        users[5] = lonely_users[0]
    if lonely_items.numel():
        pos[6], neg[7] = lonely_items[0], lonely_items[-1]
    return users, pos, neg


_steps = {}


def check_step(case, dim, k, w_dev, decay=1e-4):
    """``step_forward`` + ``step_backward`` on every rank, called directly (autograd's engine would run every rank's
    backward on one worker thread): the reduced bpr and reg within 1e-5 relative of fp64, the gradient of the own rows
    and of the seed rows among them within rel_fro 1e-5, foreign rows exactly zero."""
    from conftest import rel_fro
    assert not case.has_empty_range
    alphas = alphas_of(k, True)
    users, pos, neg = triples(case.name)
    w = table(case.name, dim, seed=1)
    key = (case.name, dim, k)
    if key not in _steps:
        _steps[key] = step_fp64(w, case.coo(False), alphas, users, pos, neg, decay)
    bpr, reg, grad_ref = _steps[key]
    dev = w_dev.device
    u_d, p_d, n_d = users.to(dev), pos.to(dev), neg.to(dev)
    size = users.numel()
    if case.world == 3:
        lo, hi = case.ranges[1]
        assert not bool(((users >= lo) & (users < hi)).any()), "the middle rank of three owns no triple of the batch"

    def body(pp, rank):
        with torch.no_grad():
            _, bpr_l, reg_u, reg_i, saved = partition.step_forward(pp, w_dev, tuple(alphas), u_d, p_d, n_d, decay)
            grad = partition.step_backward(pp, saved, tuple(alphas), None, decay / size, zero_foreign=True)
            part = torch.stack([bpr_l, reg_u])
            pp.comm.reduce_now(part)
        return grad, float(part[0]), float(part[1] + reg_i)

    seeds = torch.unique(torch.cat([users, pos, neg]))
    worst = 0.0
    for rank, (grad, got_bpr, got_reg) in enumerate(case.run(body)):
        label = (case.name, case.world, dim, k, "step", rank)
        assert abs(got_bpr - bpr) <= 1e-5 * abs(bpr) and abs(got_reg - reg) <= 1e-5 * abs(reg), (label, got_bpr, bpr, got_reg, reg)
        got, own = grad.cpu(), case.own_mask(rank)
        assert not torch.isnan(got[own]).any(), label
        e_own = rel_fro(got[own], grad_ref[own])
        own_seeds = seeds[own[seeds]]
        e_seeds = rel_fro(got[own_seeds], grad_ref[own_seeds])
        assert e_own <= 1e-5 and e_seeds <= 1e-5, (label, e_own, e_seeds)
        check_foreign_zero(case, got, rank, label)
        worst = max(worst, e_own, e_seeds)
    return worst


def uses_node(fn, name, depth=6):
    """Whether an autograd graph contains a node whose class name holds ``name`` (searched a few levels deep)."""
    if fn is None or depth == 0:
        return False
    return name in type(fn).__name__ or any(uses_node(nxt, name, depth - 1) for nxt, _ in fn.next_functions)


def force_small_sweep(monkeypatch, graph_module):
    """The band sweep forced on every item half that qualifies at all, under the small planner configuration of
    tests/test_layer_sum_paths_gpu.py (pieces of at most 8 entries, item 0's slice beyond 32 slots)."""
    monkeypatch.setattr(graph_module, "USE_SWEEP", "1")
    monkeypatch.setattr(graph_module, "SWEEP_CFG", dict(graph_module.SWEEP_CFG, **SMALL_PLAN))
    monkeypatch.setattr(graph_module, "SWEEP_CFG_WIDE", dict(graph_module.SWEEP_CFG_WIDE, **SMALL_PLAN))
    monkeypatch.setattr(graph_module, "SWEEP_WIDE", True)
