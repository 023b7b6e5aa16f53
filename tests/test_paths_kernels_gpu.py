"""The path kernels one call at a time at the C ABI (lgc_bfs_init / _level / _resolve / _backtrack, csrc/lgconv_paths.hip)
against the word-level references of paths_kernels_support.py, on its small named graphs; then hop_distances /
shortest_paths on graphs the library builds from the same edge lists.  Every output is filled with junk before a call and
every comparison is of integers and exact.  The premises that let these tests fail are asserted on the CPU in
test_paths_kernels_host.py."""
import numpy as np
import pytest
import torch

import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import PropGraph, _native
from gnn_ecommerce_amd.paths import hop_distances, shortest_paths
import paths_kernels_support as K
import paths_support as ps

pytestmark = pytest.mark.gpu

GUARD = 3                                                    # words past n_nodes that no call may touch
COUNTERS = np.array([1000, 77, 1 << 17, 55], np.uint64)      # a launch adds to what it finds
JUNK = -99
_dev = {}


def up(a, device):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(K.words(a) if a.dtype == np.uint64 else a).to(device)


def down(t):
    """An int64 tensor of bit containers -> numpy uint64."""
    return K.words(t.cpu().numpy())


def padded(a, fill=K.SENTINEL):
    return np.concatenate([np.asarray(a, K.U64), np.full(GUARD, fill, K.U64)])


class Dev:
    def __init__(self, g, device):
        self.g, self.device = g, device
        self.rowptr = up(np.array(g.rowptr), device)
        self.entries = up(g.entries(), device)
        self._plans = {}

    def chunks(self, plan):
        key = id(plan)
        if key not in self._plans:
            self._plans[key] = (plan, up(plan.chunks, self.device) if plan.n_chunks else None)
        return self._plans[key][1]


def on_device(g, device):
    if g.name not in _dev:
        _dev[g.name] = Dev(g, device)
    return _dev[g.name]


def stream(device):
    return _native.stream_of(device)


def init_call(device, sources, n_nodes, seen, frontier, status):
    lib = _native.load()
    with torch.cuda.device(device):
        return lib.lgc_bfs_init(_native.ptr(sources), sources.numel(), n_nodes, _native.ptr(seen), _native.ptr(frontier),
                                _native.ptr(status), stream(device))


def level_call(D, plan, row_begin, row_end, active, fin, fout, seen, counters):
    lib = _native.load()
    chunks = D.chunks(plan)
    with torch.cuda.device(D.device):
        return lib.lgc_bfs_level(_native.ptr(D.rowptr), _native.ptr(D.entries), row_begin, row_end, plan.short_max,
                                 _native.ptr(chunks), plan.n_chunks, int(active), _native.ptr(fin), _native.ptr(fout),
                                 _native.ptr(seen), _native.ptr(counters), stream(D.device))


def run_level(D, plan, frontier_in, seen_in, active, row_begin=0, row_end=None):
    """One lgc_bfs_level from the given state: (frontier_out, seen, counters) with their guard words, as numpy uint64."""
    n = D.g.n_nodes
    fin = up(frontier_in, D.device)
    fout = up(np.full(n + GUARD, K.SENTINEL, K.U64), D.device)
    seen = up(padded(seen_in), D.device)
    counters = up(COUNTERS, D.device)
    code = level_call(D, plan, row_begin, n if row_end is None else row_end, active, fin, fout, seen, counters)
    assert code == 0
    return down(fout), down(seen), down(counters)


def want_level(frontier_out, seen_out, newly, bits):
    counters = COUNTERS.copy()
    counters[0] += K.U64(newly)
    counters[2] |= bits
    return padded(frontier_out), padded(seen_out), counters


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def describe(got, want):
    names = ("frontier_out", "seen", "counters")
    return [(name, np.flatnonzero(a != b)[:5].tolist()) for name, a, b in zip(names, got, want) if not np.array_equal(a, b)]


# ---------------------------------------------------------------------------------------------------------------------
# lgc_bfs_init
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sources", [1, 63, 64])
def test_init_defines_every_word_sets_every_bit_and_flags_a_source_outside(device, n_sources):
    n = 777                                                          # four workgroups of k_bfs_zero, the last one partial
    rng = np.random.default_rng(n_sources)
    clean = rng.integers(0, n, size=n_sources).astype(np.int64)
    clean[-1] = n - 1
    if n_sources > 1:
        clean[1] = clean[0]                                          # two sources on one node: both bits
        clean[n_sources // 2] = 0
    cases = [clean]
    for where, bad in ((0, -1), (n_sources - 1, n), (0, n), (n_sources - 1, -(2 ** 40))):
        s = clean.copy()
        s[where] = bad
        cases.append(s)
    both = clean.copy()
    both[0], both[-1] = -1, n + 2 ** 33
    cases.append(both)
    for src in cases:
        seen = up(np.full(n + GUARD, K.SENTINEL, K.U64), device)
        frontier = up(np.full(n + GUARD, ~K.SENTINEL, K.U64), device)
        status = torch.tensor([2, JUNK, JUNK, JUNK], dtype=torch.int32, device=device)      # another flag is pending
        assert init_call(device, up(src, device), n, seen, frontier, status) == 0
        want_seen, want_frontier, oob = K.init_ref(src, n)
        assert oob == bool(((src < 0) | (src >= n)).any())
        if n_sources > 1 and not oob:
            assert bin(int(want_seen[src[0]])).count("1") >= 2
        assert np.array_equal(down(seen), padded(want_seen)), src.tolist()
        assert np.array_equal(down(frontier), padded(want_frontier, ~K.SENTINEL)), src.tolist()
        assert status.tolist() == [2 | (K.ST_INDEX_OOB if oob else 0), JUNK, JUNK, JUNK]


# ---------------------------------------------------------------------------------------------------------------------
# lgc_bfs_level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", K.level_graphs(), ids=lambda g: g.name)
def test_every_level_under_every_plan_is_the_reference(device, g):
    D = on_device(g, device)
    n = g.n_nodes
    for src in (K.batch64(g), K.batch1(g)):
        active = K.valid_mask(src, n)
        steps = K.level_steps(g, src)
        if "self_row" in g.marks and src.size == 64:                 # the row that lists only itself reads its own bits
            assert any(s.frontier_in[g.marks["self_row"]] != 0 for s in steps)
        first = None
        plans = K.plans(g)
        for plan in plans + plans[:1]:                               # the multi-chunk plan once more at the end: a second run
            got = [run_level(D, plan, s.frontier_in, s.seen_in, active) for s in steps]
            for s, one in zip(steps, got):
                want = want_level(s.frontier_out, s.seen_out, s.newly, s.bits)
                assert same(one, want), (g.name, src.size, plan.name, s.level, describe(one, want))
            if first is None:
                first = got
            assert all(same(a, b) for a, b in zip(got, first)), (g.name, plan.name)     # whatever the cut, the same words


@pytest.mark.parametrize("g", K.level_graphs(), ids=lambda g: g.name)
def test_a_sub_range_of_rows_leaves_the_rows_outside_alone(device, g):
    D = on_device(g, device)
    n = g.n_nodes
    rb, re = g.marks["sub_range"]
    src = K.batch64(g)
    active = K.valid_mask(src, n)
    steps = K.level_steps(g, src)                                    # the states of the whole-graph search as inputs
    before = np.full(n, K.SENTINEL, K.U64)
    for plan in K.plans(g, rb, re):
        for s in steps:
            ref = K.level_ref(g.rowptr, g.cols, rb, re, active, s.frontier_in, s.seen_in, before)
            assert np.all(ref[0][:rb] == K.SENTINEL) and np.all(ref[0][re:] == K.SENTINEL)
            got, want = run_level(D, plan, s.frontier_in, s.seen_in, active, rb, re), want_level(*ref)
            assert same(got, want), (g.name, plan.name, s.level, describe(got, want))
    whole = sum(s.newly for s in steps)
    part = sum(K.level_ref(g.rowptr, g.cols, rb, re, active, s.frontier_in, s.seen_in)[2] for s in steps)
    assert 0 < part < whole                                          # rows on both sides of the range would have been new


@pytest.mark.parametrize("g", K.level_graphs(), ids=lambda g: g.name)
def test_a_row_every_active_source_has_reached_is_finished(device, g):
    """``active`` a strict subset of the seeded bits.  A row with (~seen & active) == 0 gives 0 although its neighbours
    carry inactive bits; any other row gets all of the OR, inactive bits included.  One thing is left open by the header
    and checked as such: a row cut into several chunks may lose inactive bits (a chunk that finds the row finished by a
    sibling chunk of the same level skips), never active ones and never its count."""
    D = on_device(g, device)
    n = g.n_nodes
    src = K.batch64(g)
    active = K.subset_active(g, src)
    steps = K.level_steps(g, src, active=active)
    for plan in K.plans(g):
        loose = plan.multi_rows
        for s in steps:
            got = run_level(D, plan, s.frontier_in, s.seen_in, active)
            want = want_level(s.frontier_out, s.seen_out, s.newly, s.bits)
            what = (g.name, plan.name, s.level)
            if loose.size == 0:
                assert same(got, want), what + (describe(got, want),)
                continue
            tight = np.ones(n + GUARD, bool)
            tight[loose] = False
            for a, b in zip(got[:2], want[:2]):
                assert np.array_equal(a[tight], b[tight]), what
                assert np.array_equal(a[loose] & active, b[loose] & active) and np.all(a[loose] & ~b[loose] == 0), what
            assert got[2][[0, 1, 3]].tolist() == want[2][[0, 1, 3]].tolist(), what
            assert got[2][2] & active == want[2][2] & active and got[2][2] & ~want[2][2] == 0, what
    # active == 0: nothing is launched, nothing is written
    s = steps[0]
    for plan in K.plans(g)[:2]:
        got = run_level(D, plan, s.frontier_in, s.seen_in, 0)
        assert same(got, (padded(np.full(n, K.SENTINEL, K.U64)), padded(s.seen_in), COUNTERS)), (g.name, plan.name)


# ---------------------------------------------------------------------------------------------------------------------
# lgc_bfs_resolve
# ---------------------------------------------------------------------------------------------------------------------
def resolve_call(device, src, tgt, n_nodes, frontier, level, dist):
    """(dist, counters, status) after one lgc_bfs_resolve."""
    lib = _native.load()
    s, t, f = up(src, device), up(tgt, device), up(frontier, device)
    d = up(np.concatenate([dist.flatten(), np.full(GUARD, JUNK, np.int32)]), device)
    counters = up(COUNTERS, device)
    status = torch.tensor([2, JUNK, JUNK, JUNK], dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        code = lib.lgc_bfs_resolve(_native.ptr(s), _native.ptr(t), src.size, tgt.shape[1], n_nodes, _native.ptr(f), level,
                                   _native.ptr(d), _native.ptr(counters), _native.ptr(status), stream(device))
    assert code == 0
    d = d.cpu().numpy()
    assert d[-GUARD:].tolist() == [JUNK] * GUARD
    return d[:-GUARD].reshape(dist.shape), down(counters), status.tolist()


@pytest.mark.parametrize("n_targets", [1, 20, 65])
def test_resolve_settles_the_unset_pairs_of_this_level_and_counts_them(device, n_targets):
    g = K.lengths()
    n = g.n_nodes
    rng = np.random.default_rng(n_targets)
    clean_src = K.batch64(g)
    clean_tgt = rng.integers(0, n, size=(64, n_targets)).astype(np.int64)
    frontier = np.frombuffer(rng.bytes(8 * n), dtype=np.uint64).copy()            # any words: resolve only reads bits
    frontier[::7] = 0
    bad_src, bad_tgt = clean_src.copy(), clean_tgt.copy()
    bad_src[7], bad_src[33] = -1, n
    bad_tgt[2, 0], bad_tgt[40, -1], bad_tgt[63, 0] = n, -5, 2 ** 35
    dist0 = np.full((64, n_targets), K.UNSET, np.int32)
    preset = rng.random(dist0.shape) < 0.3
    dist0[preset] = rng.choice([-1, -2, 0, 5, 123], size=int(preset.sum()))       # set already: left alone, not counted
    dist0[7, 0] = 4                                                               # ... even where the source is bad
    for src, tgt in ((clean_src, clean_tgt), (bad_src, bad_tgt)):
        for level in (3, 9):                                                      # the same frontier at two levels
            want, settled, oob = K.resolve_ref(src, tgt, n, frontier, level, dist0)
            assert 0 < settled < (dist0 == K.UNSET).sum() and oob == (src is bad_src)
            got, counters, status = resolve_call(device, src, tgt, n, frontier, level, dist0)
            assert np.array_equal(got, want), (n_targets, level, np.argwhere(got != want)[:5].tolist())
            assert np.array_equal(got[preset], dist0[preset]) and level in got
            assert counters.tolist() == [1000, 77 + settled, 1 << 17, 55]
            assert status == [2 | (K.ST_INDEX_OOB if oob else 0), JUNK, JUNK, JUNK]
    # level 0 on lgc_bfs_init's frontier: source == target gives 0, and two sources on one node both get it
    _, start, _ = K.init_ref(clean_src, n)
    own = clean_tgt.copy()
    own[:, 0] = clean_src
    fresh = np.full(own.shape, K.UNSET, np.int32)
    want, settled, _ = K.resolve_ref(clean_src, own, n, start, 0, fresh)
    got, counters, status = resolve_call(device, clean_src, own, n, start, 0, fresh)
    assert np.array_equal(got, want) and (got[:, 0] == 0).all() and set(np.unique(got).tolist()) <= {0, K.UNSET}
    assert counters.tolist() == [1000, 77 + settled, 1 << 17, 55] and settled >= 64 and status[0] == 2


# ---------------------------------------------------------------------------------------------------------------------
# lgc_bfs_backtrack
# ---------------------------------------------------------------------------------------------------------------------
def device_levels(D, src, n_levels, plan):
    """int64 [n_levels, n_nodes] on the device: row 0 from lgc_bfs_init, row l from lgc_bfs_level on row l - 1."""
    g, device = D.g, D.device
    n = g.n_nodes
    levels = torch.full((n_levels, n), JUNK, dtype=torch.int64, device=device)
    seen = torch.full((n,), JUNK, dtype=torch.int64, device=device)
    status = torch.zeros(4, dtype=torch.int32, device=device)
    assert init_call(device, up(src, device), n, seen, levels[0], status) == 0
    counters = torch.zeros(4, dtype=torch.int64, device=device)
    for l in range(1, n_levels):
        assert level_call(D, plan, 0, n, K.valid_mask(src, n), levels[l - 1], levels[l], seen, counters) == 0
    assert status.tolist() == [0, 0, 0, 0]
    return levels


def backtrack_call(D, levels, n_levels, tgt, dist, path_len):
    lib = _native.load()
    S, T = dist.shape
    paths = torch.full((S * T * path_len + GUARD,), JUNK, dtype=torch.int64, device=D.device)
    t, d = up(tgt, D.device), up(dist, D.device)
    with torch.cuda.device(D.device):
        code = lib.lgc_bfs_backtrack(_native.ptr(D.rowptr), _native.ptr(D.entries), D.g.n_nodes, _native.ptr(levels), n_levels,
                                     _native.ptr(t), _native.ptr(d), S, T, _native.ptr(paths), path_len, stream(D.device))
    assert code == 0
    paths = paths.cpu().numpy()
    assert paths[-GUARD:].tolist() == [JUNK] * GUARD
    return paths[:-GUARD].reshape(S, T, path_len)


def walked(D, src, tgt, plan):
    """(dist, the reference's levels, the device's levels) of a batch; the device's levels are checked word for word."""
    dist, _, kept = K.search_ref(D.g, src, tgt)
    levels = device_levels(D, src, kept[0].shape[0], plan)
    assert np.array_equal(down(levels), kept[0])
    return dist, kept[0], levels


def small_batch(g):
    """Three sources, so that 3 x 3 pairs end in a workgroup of k_bfs_backtrack that is not full."""
    c = g.marks["corners"]
    return np.array([c[1], c[3], c[2]], np.int64)


@pytest.mark.parametrize("variant", K.FIRST_HIT_VARIANTS)
def test_backtrack_takes_the_first_carrier_in_entry_order(device, variant):
    g = K.first_hit(variant)
    D = on_device(g, device)
    row = g.row(g.marks["target"])
    for src, b_of_a in ((K.batch64(g), 63), (small_batch(g), 1)):
        tgt = K.pair_targets(g, src, 3)
        assert (src.size * 3) % K.WAVES_PER_BLOCK != 0 or src.size == 64
        dist, ref_levels, levels = walked(D, src, tgt, K.planned(g, 8, 64))
        want = K.backtrack_ref(g.rowptr, g.cols, ref_levels, ref_levels.shape[0], tgt, dist, 4)
        assert want[b_of_a, 0].tolist() == [g.marks["a"], int(row[g.marks["first"]]), g.marks["target"], -1]
        got = backtrack_call(D, levels, ref_levels.shape[0], tgt, dist, 4)
        assert np.array_equal(got, want), (variant, src.size, np.argwhere(got != want)[:5].tolist())
        again = backtrack_call(D, levels, ref_levels.shape[0], tgt, dist, 4)
        assert np.array_equal(again, got)


def test_backtrack_on_diamonds_follows_first_predecessors_at_every_level(device):
    g = K.diamonds()
    D = on_device(g, device)
    for src, n_tgt in ((K.batch64(g), 7), (small_batch(g), 3)):
        tgt = K.pair_targets(g, src, n_tgt)
        if src.size == 3:
            tgt[:] = [g.marks["layers"][l][1] for l in (5, 3, 2)]
        dist, ref_levels, levels = walked(D, src, tgt, K.planned(g, 0, 16))
        n_levels = ref_levels.shape[0]
        assert dist.max() == 5 and n_levels >= 6
        for path_len in (6, 9):
            want = K.backtrack_ref(g.rowptr, g.cols, ref_levels, n_levels, tgt, dist, path_len)
            got = backtrack_call(D, levels, n_levels, tgt, dist, path_len)
            assert np.array_equal(got, want), (src.size, path_len, np.argwhere(got != want)[:5].tolist())
            for wrong in ("last", "smallest"):
                other = K.backtrack_ref(g.rowptr, g.cols, ref_levels, n_levels, tgt, dist, path_len, wrong)
                assert src.size == 3 or not np.array_equal(got, other)


def test_backtrack_refuses_what_it_cannot_walk_and_stops_where_the_levels_end(device):
    g = K.diamonds()
    D = on_device(g, device)
    n = g.n_nodes
    src = K.batch64(g)
    tgt = K.pair_targets(g, src, 7)
    dist, ref_levels, levels = walked(D, src, tgt, K.planned(g, 8, 64))
    n_levels = ref_levels.shape[0]
    assert all((dist == d).any() for d in range(6)) and (dist == -1).any()

    def check(what, n_lev=n_levels, path_len=6, t=tgt, d=dist, lev=None):
        ref_lev = ref_levels if lev is None else lev
        dev_lev = levels if lev is None else up(lev, device)
        want = K.backtrack_ref(g.rowptr, g.cols, ref_lev, n_lev, t, d, path_len)
        got = backtrack_call(D, dev_lev, n_lev, t, d, path_len)
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())
        return got

    got = check("d == n_levels", n_lev=3)
    assert (got[dist == 3] == -1).all() and (got[dist == 2][:, 2] >= 0).all()
    got = check("d == path_len", path_len=3)
    assert (got[dist == 3] == -1).all() and (got[dist == 2] >= 0).all()
    got = check("path_len 1", path_len=1)
    assert np.array_equal(got[..., 0], np.where(dist == 0, tgt, -1)) and (dist == 0).sum() >= 4
    rng = np.random.default_rng(5)
    bad = dist.copy()
    pick = rng.random(dist.shape) < 0.4
    bad[pick] = rng.choice([-1, -2, K.UNSET, -7], size=int(pick.sum()))
    got = check("negative dist", d=bad)
    assert (got[pick] == -1).all() and (dist[pick] >= 2).any()
    out_tgt, out_dist = tgt.copy(), dist.copy()
    for (b, c), node in zip(((0, 0), (31, 1), (32, 2), (63, 3), (10, 6)), (n, -1, 2 ** 40, n + 1, -(2 ** 33))):
        out_tgt[b, c], out_dist[b, c] = node, 2
    got = check("a target outside the graph", t=out_tgt, d=out_dist)
    assert (got[[0, 31, 32, 63, 10], [0, 1, 2, 3, 6]] == -1).all()
    # levels and dist disagree: no node at level 2 / no node with bit 63 at level 1 -- the walk stops there
    cut = ref_levels.copy()
    cut[2] = 0
    got = check("level 2 emptied", lev=cut)
    deep = dist >= 4
    assert (got[deep][:, :3] == -1).all() and (got[deep][:, 3] >= 0).all() and deep.any()
    assert np.array_equal(got[dist <= 2], check("intact")[dist <= 2])
    cut = ref_levels.copy()
    cut[1] &= ~K.bit(63)
    got = check("bit 63 cleared at level 1", lev=cut)
    far = dist[63] >= 2
    assert far.any() and (got[63][far][:, :2] == -1).all() and (got[63][far][:, 2] >= 0).all()
    assert np.array_equal(got[:63], check("intact")[:63])


# ---------------------------------------------------------------------------------------------------------------------
# the library on top
# ---------------------------------------------------------------------------------------------------------------------
def built(g, device, **kw):
    """The PropGraph of the graph's edge list (weights: zeros and negative numbers); the build keeps the entry order."""
    ei, ew = up(g.edge_index(), device), up(g.edge_weight(), device)
    graph = PropGraph(ei, ew, g.n_nodes, **kw)
    op = graph.forward_op
    assert np.array_equal(op.rowptr.cpu().numpy(), g.rowptr)
    assert np.array_equal(op.entries.cpu().numpy()[:g.cols.size, 0], g.cols)
    return graph


def trace_cases(g):
    """[(sources, targets, max_hops, dist, trace)] from the reference: 65 and 129 sources (two and three batches, the last
    of one source, whose targets are the source itself: it settles at level 0), with and without a hop limit; between
    them the batches stop for each of the three reasons."""
    out, stops = [], set()
    for count, n_tgt, max_hops in ((65, 4, None), (129, 3, None), (129, 2, 2), (65, g.n_nodes, None)):
        src = K.many_sources(g, count)
        if n_tgt < g.n_nodes:
            tgt = K.pair_targets(g, src, n_tgt)
            tgt[-1] = src[-1]
        else:
            tgt = np.tile(np.arange(g.n_nodes, dtype=np.int64), (count, 1))
        want, trace, _ = K.search_ref(g, src, tgt, max_hops)
        assert np.array_equal(want, ps.reference(g.edge_index(), g.n_nodes, src, tgt, max_hops))
        assert [t[0] for t in trace if t[1] == 0] == list(range(-(-count // 64)))          # batches of 64, the last of one
        last = {}
        for batch, level, new, settled in trace:
            last[batch] = (level, new)
        stops |= {"max_hops" if level == max_hops else "nothing new" if level and new == 0 else "all settled"
                  for level, new in last.values()}
        out.append((src, tgt, max_hops, want, trace))
    assert stops == {"max_hops", "nothing new", "all settled"}, stops
    return out


@pytest.mark.parametrize("g", [K.lengths(), K.diamonds(), K.chain(), K.two_islands()], ids=lambda g: g.name)
def test_the_trace_is_the_references_level_by_level(device, g):
    lg.check_index_status(device)
    graphs = [built(g, device)] + ([built(g, device, short_max=0, chunk_len=16)] if g.name == "lengths" else [])
    for src, tgt, max_hops, want, want_trace in trace_cases(g):
        for graph in graphs:
            trace = []
            got = hop_distances(graph, up(src, device), up(tgt, device), max_hops=max_hops, trace=trace)
            assert [t[:4] for t in trace] == want_trace, (g.name, src.size, max_hops)
            assert all(len(t) == 5 and t[4] >= 0 for t in trace)
            assert np.array_equal(got.cpu().numpy(), want)
    lg.check_index_status(device)


@pytest.mark.parametrize("g", [K.chain(), K.diamonds()], ids=lambda g: g.name)
def test_a_max_len_below_the_depth_keeps_the_distances_and_the_short_paths(device, g):
    """Levels above max_len go to the two spare buffers instead of levels[l]; the distances stay exact, those pairs'
    paths are all -1, the others are the first-predecessor paths."""
    graph = built(g, device)
    src = np.concatenate([np.array(g.marks["corners"], np.int64), K.batch64(g)[:7]])
    tgt = np.tile(np.arange(g.n_nodes, dtype=np.int64), (src.size, 1))
    want, _, kept = K.search_ref(g, src, tgt)
    assert want.max() >= 5 and (want == -1).any()
    for max_len in (0, 1, 2, int(want.max())):
        dist, paths = shortest_paths(graph, up(src, device), up(tgt, device), max_len=max_len)
        assert np.array_equal(dist.cpu().numpy(), want), max_len
        want_paths = K.keep_paths(g, src, tgt, want, kept, max_len)
        got = paths.cpu().numpy()
        assert np.array_equal(got, want_paths), (max_len, np.argwhere(got != want_paths)[:5].tolist())
        assert (got[(want > max_len) | (want < 0)] == -1).all() and (got[(want >= 0) & (want <= max_len)][:, 0] >= 0).all()
        capped, paths2 = shortest_paths(graph, up(src, device), up(tgt, device), max_len=max_len, max_hops=3)
        assert np.array_equal(capped.cpu().numpy(), ps.reference(g.edge_index(), g.n_nodes, src, tgt, 3))
        near = (want >= 0) & (want <= 3)
        assert np.array_equal(paths2.cpu().numpy()[near], want_paths[near]) and (paths2.cpu().numpy()[~near] == -1).all()
    lg.check_index_status(device)


def test_max_hops_on_two_islands_tells_no_path_from_not_yet(device):
    g = K.two_islands()
    graph = built(g, device)
    src = np.array([0, 2, 8, 10, 11, 6, 5, 0], np.int64)
    tgt = np.tile(np.arange(g.n_nodes, dtype=np.int64), (src.size, 1))
    ecc = max(int(ps.bfs_all(g.edge_index(), g.n_nodes, int(s)).max()) for s in src)
    assert ecc == 4
    seen_values = set()
    for max_hops in (0, 1, ecc, ecc + 1):
        want = ps.reference(g.edge_index(), g.n_nodes, src, tgt, max_hops)
        got = hop_distances(graph, up(src, device), up(tgt, device), max_hops=max_hops).cpu().numpy()
        assert np.array_equal(got, want), (max_hops, np.argwhere(got != want)[:5].tolist())
        for s in range(src.size):                                    # -1 against -2 source by source
            seen_values.add((max_hops, s, tuple(sorted(set(want[s][want[s] < 0].tolist())))))
    assert (ecc, 0, (-2,)) in seen_values and (ecc, 1, (-1,)) in seen_values          # in one batch, at one limit
    assert (ecc + 1, 0, (-1,)) in seen_values and (0, 3, (-2,)) in seen_values and (1, 3, (-1,)) in seen_values
    lg.check_index_status(device)


@pytest.mark.parametrize("normalize", [True, False])
def test_edges_of_weight_zero_and_of_negative_weight_are_edges(device, normalize):
    g = K.chain()
    ei = up(g.edge_index(), device)
    src = np.array([0, 8, 3], np.int64)
    tgt = np.tile(np.arange(g.n_nodes, dtype=np.int64), (3, 1))
    want, _, kept = K.search_ref(g, src, tgt)
    want_paths = K.keep_paths(g, src, tgt, want, kept, 11)
    for weights in (np.zeros(g.cols.size, np.float32), np.full(g.cols.size, -2.5, np.float32), g.edge_weight()):
        graph = PropGraph(ei, up(weights, device), g.n_nodes, normalize=normalize)
        dist, paths = shortest_paths(graph, up(src, device), up(tgt, device), max_len=11)
        assert np.array_equal(dist.cpu().numpy(), want) and np.array_equal(paths.cpu().numpy(), want_paths)
    lg.check_index_status(device)
