"""CPU-only: the word-level references of paths_kernels_support.py against the plain BFS of paths_support.py and the
fixture from upstream, and the premises that let test_paths_kernels_gpu.py fail -- every named graph has the cases its
docstring claims."""
import numpy as np
import pytest

import paths_kernels_support as K
import paths_support as ps


def fixture_graph():
    """The golden graph as a PathGraph: its edges stably sorted by target, which is the order lgc_build_csr keeps."""
    z = ps.fixture()
    n = int(z["n_users"]) + int(z["n_items"])
    src, dst = z["edge_index"]
    order = np.argsort(dst, kind="stable")
    rows = [[] for _ in range(n)]
    for j, v in zip(src[order].tolist(), dst[order].tolist()):
        rows[v].append(j)
    return z, K._graph("fixture", rows)


def searches(g):
    yield K.batch64(g), K.pair_targets(g, K.batch64(g), 5)
    yield K.batch1(g), K.pair_targets(g, K.batch1(g), 5)
    yield K.many_sources(g, 70), np.tile(np.arange(g.n_nodes, dtype=np.int64), (70, 1))


@pytest.mark.parametrize("g", K.all_graphs(), ids=lambda g: g.name)
def test_iterating_the_word_references_gives_the_plain_bfs(g):
    edge_index = g.edge_index()
    for sources, targets in searches(g):
        dist, trace, kept = K.search_ref(g, sources, targets)
        assert np.array_equal(dist, ps.reference(edge_index, g.n_nodes, sources, targets))
        # and word by word: bit b of level l is "source b is l hops away"
        for batch, levels in enumerate(kept):
            for b, s in enumerate(sources[batch * 64:(batch + 1) * 64].tolist()):
                d_all = ps.bfs_all(edge_index, g.n_nodes, s)
                for l, words in enumerate(levels):
                    assert np.array_equal((words & K.bit(b)) != 0, d_all == l), (g.name, batch, b, l)
        for hops in (0, 1, 2, 3):
            capped, _, _ = K.search_ref(g, sources, targets, max_hops=hops)
            assert np.array_equal(capped, ps.reference(edge_index, g.n_nodes, sources, targets, hops)), (g.name, hops)


def test_the_references_reproduce_the_fixtures_lengths_and_paths():
    z, g = fixture_graph()
    sources, targets = z["out_user_id_idx"], z["out_top_rlvnt_itm"]
    dist, trace, kept = K.search_ref(g, sources, targets)
    assert np.array_equal(dist, z["path_lens"]) and dist.max() >= 5
    assert np.array_equal(dist, ps.reference(z["edge_index"], g.n_nodes, sources, targets))
    everyone = np.tile(np.arange(g.n_nodes, dtype=np.int64), (len(sources), 1))
    whole, _, _ = K.search_ref(g, sources, everyone)                             # to the fixed point: bfs_all per source
    for r, s in enumerate(sources.tolist()):
        assert np.array_equal(whole[r], ps.bfs_all(z["edge_index"], g.n_nodes, s)), r
    max_len = z["paths"].shape[2] - 1
    assert np.array_equal(K.keep_paths(g, sources, targets, dist, kept, max_len), z["paths"])
    # the fixture is a tree: one shortest path, whatever rule picks the predecessor
    levels = kept[0][:max_len + 1]
    n = min(64, len(sources))
    for pick in ("last", "smallest"):
        got = K.backtrack_ref(g.rowptr, g.cols, levels, levels.shape[0], targets[:n], dist[:n], max_len + 1, pick)
        assert np.array_equal(got, z["paths"][:n])


def test_out_of_range_ids_in_the_references():
    g = K.chain()
    sources = np.array([0, -1, 12, 3], np.int64)
    seen, frontier, oob = K.init_ref(sources, g.n_nodes)
    assert oob and seen[0] == 1 and seen[3] == 8 and int(seen.sum()) == 9 and np.array_equal(seen, frontier)
    assert K.valid_mask(sources, g.n_nodes) == 9
    targets = np.array([[0, 5], [0, 1], [2, 3], [3, 12]], np.int64)
    dist = np.full((4, 2), K.UNSET, np.int32)
    dist[0, 1] = 7
    got, settled, flagged = K.resolve_ref(sources, targets, g.n_nodes, frontier, 0, dist)
    assert got.tolist() == [[0, 7], [-1, -1], [-1, -1], [0, -1]] and settled == 7 and flagged
    full, _, _ = K.search_ref(g, sources, targets)
    assert np.array_equal(full, ps.reference(g.edge_index(), g.n_nodes, sources, targets))


def test_the_skip_rule_and_the_sub_range_in_level_ref():
    g = K.chain()
    seen, frontier, _ = K.init_ref(np.array([0, 1], np.int64), g.n_nodes)     # bit 0 at node 0, bit 1 at node 1
    out, after, newly, bits = K.level_ref(g.rowptr, g.cols, 0, g.n_nodes, 3, frontier, seen)
    assert out.tolist() == [0, 1, 2] + [0] * 9 and newly == 2 and bits == 3 and after[:3].tolist() == [1, 3, 2]
    # active = bit 1 only: node 1 has been reached by every active source, so its row is finished (0) although node 0
    # carries bit 0; node 2 is not, and gets bit 1 -- fresh is masked by seen, never by active
    out, after, newly, bits = K.level_ref(g.rowptr, g.cols, 0, g.n_nodes, 2, frontier, seen)
    assert out.tolist() == [0, 0, 2] + [0] * 9 and newly == 1 and bits == 2
    seen2 = seen.copy()
    seen2[2] = 2
    frontier2 = frontier.copy()
    frontier2[8] = 1                                                              # an inactive bit at node 8, which row 2 lists
    out, *_ = K.level_ref(g.rowptr, g.cols, 0, g.n_nodes, 2, frontier2, seen2)
    assert out[2] == 0                                                            # finished: the inactive bit is not picked up
    out, *_ = K.level_ref(g.rowptr, g.cols, 0, g.n_nodes, 6, frontier2, seen2)
    assert out[2] == 1                                                            # not finished (bit 2 is missing): all of the OR
    # a sub-range leaves the rows outside alone; active == 0 leaves everything alone
    before = np.full(g.n_nodes, K.SENTINEL, K.U64)
    out, after, newly, _ = K.level_ref(g.rowptr, g.cols, 2, 10, 3, frontier, seen, before)
    assert out[2] == 2 and newly == 1 and np.all(out[:2] == K.SENTINEL) and np.all(out[10:] == K.SENTINEL)
    assert np.all(out[3:10] == 0) and np.array_equal(after[:2], seen[:2])
    out, after, newly, bits = K.level_ref(g.rowptr, g.cols, 0, g.n_nodes, 0, frontier, seen, before)
    assert np.all(out == K.SENTINEL) and np.array_equal(after, seen) and newly == 0 and bits == 0


def test_backtrack_ref_breaks_where_levels_and_dist_disagree():
    g = K.chain()
    sources, targets = np.array([0], np.int64), np.array([[6, 2, 0]], np.int64)
    dist, _, kept = K.search_ref(g, sources, targets)
    assert dist.tolist() == [[6, 2, 0]]                                           # the back edge 8 -> 2 shortens nothing
    levels = kept[0]
    want = [[0, 1, 2, 3, 4, 5, 6, -1], [0, 1, 2, -1, -1, -1, -1, -1], [0] + [-1] * 7]
    assert K.backtrack_ref(g.rowptr, g.cols, levels, 7, targets, dist, 8)[0].tolist() == want
    assert K.backtrack_ref(g.rowptr, g.cols, levels, 6, targets, dist, 8)[0].tolist() == [[-1] * 8] + want[1:]   # d == n_levels
    assert K.backtrack_ref(g.rowptr, g.cols, levels, 7, targets, dist, 6)[0].tolist() == [[-1] * 6, want[1][:6], want[2][:6]]
    assert K.backtrack_ref(g.rowptr, g.cols, levels, 7, targets, dist, 1)[0].tolist() == [[-1], [-1], [0]]
    cut = levels.copy()
    cut[3] = 0                                                                    # nobody was reached at level 3
    got = K.backtrack_ref(g.rowptr, g.cols, cut, 7, targets, dist, 8)[0].tolist()
    assert got == [[-1, -1, -1, -1, 4, 5, 6, -1]] + want[1:]                      # the break and below: -1; above: kept
    for bad in (-1, -2, K.UNSET):
        d = np.full((1, 3), bad, np.int32)
        assert (K.backtrack_ref(g.rowptr, g.cols, levels, 7, targets, d, 8) == -1).all()
    outside = np.array([[12, -1, 2 ** 40]], np.int64)
    assert (K.backtrack_ref(g.rowptr, g.cols, levels, 7, outside, np.full((1, 3), 2, np.int32), 8) == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# premises
# ---------------------------------------------------------------------------------------------------------------------
def test_lengths_has_the_listed_rows_and_fills_neither_kernels_last_workgroup():
    g = K.lengths()
    assert g.lengths[:16].tolist() == list(K.LENGTHS) and np.all(g.lengths[16:] == 1)
    assert g.n_nodes <= 1000 and g.lengths.max() == 300
    assert g.n_nodes > K.ROWS_PER_BLOCK and g.n_nodes % K.ROWS_PER_BLOCK != 0
    assert set(g.row(g.marks["self_row"]).tolist()) == {g.marks["self_row"]}
    assert len(np.unique(g.row(15))) < 300 and g.row(15).min() < 5 and g.row(15).max() > g.n_nodes - 5   # repeats, whole range
    fine = K.planned(g, 0, 16)
    assert fine.n_chunks > K.WAVES_PER_BLOCK and fine.n_chunks % K.WAVES_PER_BLOCK != 0
    assert fine.n_chunks == 147 and fine.multi_rows.tolist() == list(range(7, 16))            # rows of 17 .. 300 entries
    assert K.planned(g, 300, 4096).n_chunks == 0                                               # every row short
    mid = K.planned(g, 8, 64)
    assert sorted(set(mid.chunks[:, 0].tolist())) == list(range(4, 16)) and mid.multi_rows.tolist() == [12, 13, 14, 15]
    assert K.planned(g, 32, 100).multi_rows.tolist() == [13, 14, 15]


@pytest.mark.parametrize("g", K.all_graphs(), ids=lambda g: g.name)
def test_every_plan_covers_its_long_rows_once(g):
    assert g.n_nodes <= 1000
    rb, re = g.marks["sub_range"]
    assert 0 < rb < re < g.n_nodes
    for lo, hi in ((0, g.n_nodes), (rb, re)):
        plans = K.plans(g, lo, hi)
        assert len(plans) == 10
        for plan in plans:
            K.check_plan(g, plan, lo, hi)
    cuts = {p.name: p for p in K.plans(g)}
    longest = int(g.lengths.argmax())
    if g.lengths[longest] >= 9:
        one = cuts["one_plus_rest(0)"].chunks
        assert np.diff(one[one[:, 0] == longest, 1:3], axis=1).flatten().tolist() == [1, g.lengths[longest] - 1]
        three = np.diff(cuts["three_unequal(0)"].chunks[cuts["three_unequal(0)"].chunks[:, 0] == longest, 1:3], axis=1)
        assert three.size == 3 and len(set(three.flatten().tolist())) == 3
        back = cuts["reversed(0,16)"].chunks
        assert np.all(np.diff(back[:, 1]) < 0)                                             # last chunk first


@pytest.mark.parametrize("g", K.level_graphs(), ids=lambda g: g.name)
def test_the_corner_bits_sit_on_distinct_nodes_and_two_sources_share_one(g):
    src = K.batch64(g)
    assert src.size == 64 and len({int(src[b]) for b in K.CORNER_BITS}) == 4
    assert src[5] == src[40] == src[63]
    seen, _, oob = K.init_ref(src, g.n_nodes)
    assert not oob and bin(int(seen[src[63]])).count("1") >= 3
    steps = K.level_steps(g, src)
    assert len(steps) >= 2 and steps[-1].newly == 0 and all(s.newly > 0 for s in steps[:-1])
    for b in K.CORNER_BITS:                                             # each corner bit travels: a wrong shift shows
        assert any(int(s.bits) >> b & 1 for s in steps) or (g.name.startswith("first_hit") and b in (0, 32))


def test_lengths_has_a_multi_chunk_row_that_finds_nothing_and_one_that_is_new_in_two_chunks():
    g = K.lengths()
    plan = K.planned(g, 0, 16)
    nothing = twice = 0
    for src in (K.batch1(g), K.batch64(g)):
        for s in K.level_steps(g, src):
            for v in plan.multi_rows.tolist():
                if (~s.seen_in[v] & K.valid_mask(src, g.n_nodes)) == 0:
                    continue
                parts = [np.bitwise_or.reduce(s.frontier_in[g.cols[b:e]], initial=K.ZERO) & ~s.seen_in[v]
                         for r, b, e, _ in plan.chunks.tolist() if r == v]
                nothing += all(p == 0 for p in parts)
                twice += sum(p != 0 for p in parts) >= 2                # counting per chunk would count this node twice
    assert nothing >= 1 and twice >= 1


@pytest.mark.parametrize("g", K.level_graphs(), ids=lambda g: g.name)
def test_a_strict_subset_of_active_bits_meets_the_skip_rule(g):
    """The rows the skip rule decides: reached by every active source while a neighbour carries an inactive bit the row
    has not seen.  Without the rule such a row would publish that bit."""
    src = K.batch64(g)
    active = K.subset_active(g, src)
    assert active != 0 and active != K.valid_mask(src, g.n_nodes) and (active & ~K.valid_mask(src, g.n_nodes)) == 0
    steps = K.level_steps(g, src, active=active)
    skipped = 0
    for s in steps:
        for v in range(g.n_nodes):
            if (~s.seen_in[v] & active) == 0 and (K.row_or(g.rowptr, g.cols, v, s.frontier_in) & ~s.seen_in[v]) != 0:
                skipped += 1
                assert s.frontier_out[v] == 0
    assert skipped >= 1, g.name
    assert any(s.newly for s in steps)
    if g.name.startswith("first_hit"):                                  # ... the 200-entry row among them: the chunk kernel's skip
        assert any((~s.seen_in[0] & active) == 0 and K.row_or(g.rowptr, g.cols, 0, s.frontier_in) & ~s.seen_in[0] for s in steps)


@pytest.mark.parametrize("variant", K.FIRST_HIT_VARIANTS)
def test_first_hit_puts_the_first_carrier_where_it_says(variant):
    g = K.first_hit(variant)
    m = g.marks
    assert g.lengths[m["target"]] == K.FIRST_HIT_ROW and g.n_nodes <= 1000
    src = K.batch64(g)
    assert src[63] == m["a"] and src[31] == m["b"]
    targets = K.pair_targets(g, src, 3)
    dist, _, kept = K.search_ref(g, src, targets)
    assert dist[63, 0] == 2 and dist[63, 1] == 1
    row = g.row(m["target"])
    carries = (kept[0][1][row] >> K.U64(63)) & K.ONE != 0                  # entries of the target's row with A's bit at level 1
    at = np.flatnonzero(carries)
    assert at[0] == m["first"] and tuple(at.tolist()) == m["carriers"]
    if variant.startswith("at_"):
        assert m["first"] == int(variant[3:])
        assert at.size >= 2 or m["first"] == K.FIRST_HIT_ROW - 1            # later carriers, except behind the last entry
        if m["first"]:
            other = (kept[0][1][row[:m["first"]]] >> K.U64(31)) & K.ONE != 0
            assert other.any()                                              # B's bit alone comes first and is passed over
    if variant == "both_steps":
        assert at.tolist() == [10, 70, 130]
    if variant == "twice":
        assert row[5] == row[80] and row[2] == row[50] and at.tolist() == [5, 80, 120] and row[120] != row[5]
    if variant == "other_source":
        assert at[0] == 20 and np.all((kept[0][1][row[:20]] >> K.U64(31)) & K.ONE != 0)
    # the three rules give three paths (two where nothing follows the first carrier)
    paths = {pick: K.backtrack_ref(g.rowptr, g.cols, kept[0], kept[0].shape[0], targets, dist, 4, pick)[63, 0].tolist()
             for pick in ("first", "last", "smallest")}
    assert paths["first"] == [m["a"], int(row[m["first"]]), m["target"], -1]
    if at.size >= 2:
        assert paths["last"] != paths["first"]
        assert paths["smallest"] != paths["first"] or variant == "both_steps"
    if variant == "twice":
        assert paths["last"][1] == row[120]


def test_diamonds_tells_first_from_last_from_smallest_at_every_depth():
    g = K.diamonds()
    layers = g.marks["layers"]
    for l in range(1, len(layers)):
        for v in layers[l]:
            assert set(g.row(v).tolist()) <= set(layers[l - 1]) and not np.all(np.diff(g.row(v)) > 0)
    src = K.batch64(g)
    targets = K.pair_targets(g, src, 7)
    dist, _, kept = K.search_ref(g, src, targets)
    levels = kept[0]
    paths = {pick: K.backtrack_ref(g.rowptr, g.cols, levels, levels.shape[0], targets, dist, 6, pick)
             for pick in ("first", "last", "smallest")}
    for depth in range(2, len(layers)):
        at = np.argwhere(dist == depth)
        three = [(b, c) for b, c in at.tolist()
                 if len({tuple(paths[p][b, c].tolist()) for p in paths}) == 3]
        assert three, depth
        # ... among them a pair of a corner bit, and one that differs at every level below the target
        assert any(b in (31, 32, 63) for b, _ in three) or depth == len(layers) - 1, depth
    deep = np.argwhere(dist == len(layers) - 1)
    assert deep.size and any(np.all(paths["first"][b, c, 1:5] != paths["last"][b, c, 1:5]) for b, c in deep.tolist())


def test_chain_and_two_islands_have_their_cases():
    g = K.chain()
    assert g.n_nodes == 12 and 3 in g.row(3) and g.row(5).tolist() == [4, 4] and g.row(2).tolist() == [1, 8]
    d = ps.bfs_all(g.edge_index(), 12, 0)
    assert d.tolist() == list(range(12))
    assert ps.bfs_all(g.edge_index(), 12, 8).tolist() == [-1, -1, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3]
    g = K.two_islands()
    ei = g.edge_index()
    ecc = {s: int(ps.bfs_all(ei, 12, s).max()) for s in (0, 2, 8, 10, 11)}
    assert ecc == {0: 4, 2: 3, 8: 1, 10: 0, 11: 0}
    assert (ps.bfs_all(ei, 12, 0)[6:] == -1).all() and (ps.bfs_all(ei, 12, 6)[:6] == -1).all()
    assert g.lengths[10] == 0 and g.row(11).tolist() == [11, 11, 11]
    assert all(not np.all(np.diff(g.row(v)) > 0) for v in range(12) if g.lengths[v] > 1)
