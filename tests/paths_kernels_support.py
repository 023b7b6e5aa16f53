"""Small named graphs, hand-cut row plans and a word-level numpy reference for the tests that take the path kernels apart
(tests/test_paths_kernels_host.py, tests/test_paths_kernels_gpu.py): lgc_bfs_init / _level / _resolve / _backtrack of
csrc/lgconv_paths.hip, one call at a time at the C ABI.

Every graph is a forward CSR written by hand in numpy: ``rowptr`` int32 and, per entry, the 8-byte (int32 column, fp32
value) pair of ``lgc_entry``, uploaded as int32 ``[E, 2]`` the way the tile and build tests upload theirs.  Row v lists the
sources j of the edges j -> v in exactly the order the test wrote them: nothing here goes through ``lgc_build_csr``, so
"the first column in stored entry order" is a fact of the test and not of a sort.  The values are junk (0, a negative
number, NaN, -0): the header says they are never read.  Each graph exists for the cases its docstring names, and
test_paths_kernels_host.py asserts that it has them.

The references are written from the text of include/lgconv_hip.h, not from the kernels: bit containers are numpy uint64,
one word per node, bit b = source b of the batch.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

U64 = np.uint64
ONE = U64(1)
ZERO = U64(0)
UNSET = -3                                   # LGC_BFS_UNSET
ST_INDEX_OOB = 1                             # LGC_ST_INDEX_OOB
MAX_SOURCES = 64                             # LGC_BFS_MAX_SOURCES
ROWS_PER_BLOCK = 32                          # k_bfs_rows: 256 threads, 8 lanes per row
WAVES_PER_BLOCK = 4                          # k_bfs_chunks (chunks) and k_bfs_backtrack (pairs): one wavefront each
SENTINEL = U64(0x5A5A5A5A5A5A5A5A)           # what an output word holds before a call
CORNER_BITS = (0, 31, 32, 63)                # where 1 << b and 1ull << b part ways, and both ends of the word
PLAN_SETTINGS = ((0, 16), (8, 64), (32, 100), (300, 4096))      # (short_max, chunk_len) given to graph.build_row_plan
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65, 128, 129, 300)
FIRST_HIT_AT = (0, 1, 63, 64, 65, 127, 128, 199)
FIRST_HIT_ROW = 200


def bit(b):
    return ONE << U64(b)


def words(a):
    """numpy uint64 -> the int64 view torch uploads, and back."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.uint64 else a.view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class PathGraph:
    name: str
    rowptr: np.ndarray                       # int32 [n_nodes + 1]
    cols: np.ndarray                         # int32 [E]
    marks: dict = field(default_factory=dict)    # the nodes and entries the graph's tests name

    @property
    def n_nodes(self):
        return self.rowptr.size - 1

    @property
    def lengths(self):
        return np.diff(self.rowptr)

    def row(self, v):
        return self.cols[int(self.rowptr[v]):int(self.rowptr[v + 1])]

    def values(self):
        """fp32 [E]: never read by a path kernel."""
        return np.resize(np.array([0.0, -1.5, np.nan, -0.0, 3.0], np.float32), self.cols.size)

    def entries(self):
        """int32 [max(E, 1), 2]: (column, the value's bits)."""
        ent = np.zeros((max(self.cols.size, 1), 2), np.int32)
        ent[:self.cols.size, 0], ent[:self.cols.size, 1] = self.cols, self.values().view(np.int32)
        return ent

    def edge_index(self):
        """int64 [2, E], the edges j -> v in CSR order: a stable sort by target gives this CSR back, entry for entry."""
        dst = np.repeat(np.arange(self.n_nodes, dtype=np.int64), self.lengths)
        return np.stack([self.cols.astype(np.int64), dst])

    def edge_weight(self):
        """fp32 [E] for a graph built by the library: zeros and negative numbers, which are edges like any other."""
        return np.resize(np.array([0.0, -1.5, 2.0, -0.0, -3.0], np.float32), self.cols.size)


def _graph(name, rows, **marks):
    lengths = np.array([len(r) for r in rows], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    cols = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    assert cols.size == rowptr[-1] and (cols.size == 0 or (cols.min() >= 0 and cols.max() < len(rows)))
    rowptr.setflags(write=False)
    cols.setflags(write=False)
    return PathGraph(name, rowptr, cols, marks)


@functools.lru_cache(maxsize=None)
def lengths():
    """Row-length edges of both level kernels.  Rows 0..15 have 0, 1, 7, 8, 9, 15, 16, 17 (a group of 8 lanes: none, one
    lane, one step less one, one step, one more, two steps less one, two, two and one), 32, 33, 63, 64, 65, 128, 129 (a
    wavefront per chunk: one step less one, one step, one more, two, two and one) and 300 entries, columns drawn from the
    whole node range with repeats.  85 one-entry rows follow: 101 rows = 3 workgroups of k_bfs_rows and 5 rows; under
    short_max = 0, chunk_len = 16 the plan has 147 chunks = 36 workgroups of k_bfs_chunks and 3 chunks.  Row 16 lists only
    itself; rows 17.. list one lower-numbered or random node each, so a search takes several levels."""
    rng = np.random.default_rng([20261020, 1])
    n = len(LENGTHS) + 85
    rows = [rng.integers(0, n, size=k) for k in LENGTHS]
    rows.append([len(LENGTHS)])                                     # row 16: all of its entries point at itself
    for v in range(len(LENGTHS) + 1, n):
        rows.append([int(rng.integers(0, v)) if v % 3 else int(rng.integers(0, n))])
    return _graph("lengths", rows, self_row=len(LENGTHS), corners=(40, 3, 77, 15), sub_range=(3, n - 7))


FIRST_HIT_VARIANTS = tuple(f"at_{p}" for p in FIRST_HIT_AT) + ("both_steps", "twice", "other_source")


@functools.lru_cache(maxsize=None)
def first_hit(variant):
    """The backtrack's "first column in stored entry order".  Node 0 (the target) has a row of 200 entries that list the
    "mid" nodes 1..200 in a shuffled order; a mid node lists source A (node 201), source B (node 202), both or neither,
    so A reaches the target in two hops along every mid that lists A (a "carrier" of A's bit at level 1).  ``at_p``: the
    first carrier of A sits at entry p of the target's row -- the first and last lane of the first 64-entry step, the
    second step, the third, the fourth, the row's last entry -- carriers of B alone come before it and, unless p is 199,
    further carriers of A after it.  ``both_steps``: carriers of A at entries 10, 70 and 130 only (a hit in the first
    step must stop the walk before the second).  ``twice``: entries 5 and 80 name the same carrier, entries 2 and 50 the
    same non-carrier.  ``other_source``: entries 0..19 carry B only, entry 20 is the first that carries A.  Nodes 203 and
    204 are isolated spares."""
    rng = np.random.default_rng([20261020, 2, FIRST_HIT_VARIANTS.index(variant)])
    L, target, a, b, spare0, spare1 = FIRST_HIT_ROW, 0, 201, 202, 203, 204
    order = 1 + rng.permutation(L)                                  # the target's row: mid node at entry e
    has_a, has_b = np.zeros(L, bool), rng.random(L) < 0.4
    if variant.startswith("at_"):
        first = int(variant[3:])
        has_a[first] = True
        has_a[first + 1:] = rng.random(L - first - 1) < 0.3
        if first + 1 < L:
            has_a[rng.integers(first + 1, L)] = True
        has_b[:first] |= rng.random(first) < 0.5
        if first:
            has_b[0] = True
    elif variant == "both_steps":
        first = 10
        has_a[[10, 70, 130]] = True
    elif variant == "twice":
        first = 5
        order[80], order[50] = order[5], order[2]
        has_a[[5, 80, 120]] = True
        has_a[[2, 50]] = False
        has_b[[2, 50]] = True
    else:
        first = 20
        has_a[20:] = rng.random(L - 20) < 0.5
        has_a[20] = True
        has_b[:20] = True
    mids = [[] for _ in range(L)]
    for e in range(L):
        # where an entry repeats a node the first listing decides (the variant "twice" sets both alike)
        if not mids[order[e] - 1]:
            mids[order[e] - 1] = ([b] if has_b[e] else []) + ([a] if has_a[e] else [])
    rows = [list(order)] + mids + [[], [], [], []]
    carriers = [e for e in range(L) if a in rows[order[e]]]
    return _graph(f"first_hit[{variant}]", rows, target=target, a=a, b=b, first=first, carriers=tuple(carriers),
                  corners=(spare0, b, spare1, a), pool=(a, b, spare0, spare1, int(order[first]), int(order[L - 1])),
                  targets=(target, int(order[first]), spare0), skip_node=int(order[first]), sub_range=(1, L - 3))


DIAMOND_LAYERS = (4, 6, 6, 6, 6, 6)


@functools.lru_cache(maxsize=None)
def diamonds():
    """Several shortest paths at every level.  Six layers of 4, 6, 6, 6, 6, 6 nodes; every node of layer l + 1 lists four
    nodes of layer l (three for layer 1) in a shuffled order that is not ascending, so for a pair at depth 2 or more the
    path along first predecessors, the one along last predecessors and the one along smallest ids are three different
    paths (depth 1 has one path: the edge)."""
    rng = np.random.default_rng([20261020, 3])
    starts = np.concatenate([[0], np.cumsum(DIAMOND_LAYERS)])
    rows = [[] for _ in range(DIAMOND_LAYERS[0])]
    for l in range(1, len(DIAMOND_LAYERS)):
        below = np.arange(starts[l - 1], starts[l])
        for _ in range(DIAMOND_LAYERS[l]):
            while True:
                pick = rng.permutation(below)[:min(4, below.size - 1)]
                if not np.all(np.diff(pick) > 0):
                    break
            rows.append(pick)
    layers = tuple(tuple(range(int(starts[l]), int(starts[l + 1]))) for l in range(len(DIAMOND_LAYERS)))
    return _graph("diamonds", rows, layers=layers, corners=layers[0], pool=layers[0] + layers[1][:2], skip_node=layers[1][0],
                  sub_range=(5, int(starts[-1]) - 4))


@functools.lru_cache(maxsize=None)
def chain():
    """A directed path 0 -> 1 -> ... -> 11 (row v lists v - 1): a search 11 levels deep with one new node per level.  Node
    3 also lists itself (a self-loop), row 5 lists node 4 twice (a doubled edge), and row 2 lists node 8 after node 1 (a
    back edge 8 -> 2, which shortens nothing from node 0 and gives nodes 3.. a way back to 2)."""
    rows = [[]] + [[v - 1] for v in range(1, 12)]
    rows[3] = [3, 2]
    rows[5] = [4, 4]
    rows[2] = [1, 8]
    return _graph("chain", rows, corners=(0, 3, 8, 10), sub_range=(2, 10))


@functools.lru_cache(maxsize=None)
def two_islands():
    """Frontiers that empty.  An undirected path 0 - 1 - 2 - 3 - 4 - 5 with a chord 1 - 3, an undirected triangle
    6 - 7 - 8 with a tail 8 - 9, node 10 without any edge, node 11 whose three entries all name itself.  No source
    reaches the other island: its frontier empties (eccentricity 4 from node 0, 3 from node 2, 1 from node 8, 0 from
    nodes 10 and 11, so levels 5, 4, 2 and 1 are the first that reach nothing)."""
    und = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (1, 3), (6, 7), (7, 8), (6, 8), (8, 9)]
    rows = [[] for _ in range(12)]
    for u, v in und:
        rows[v].append(u)
        rows[u].append(v)
    rows = [r[::-1] for r in rows]                                  # not ascending
    rows[11] = [11, 11, 11]
    return _graph("two_islands", rows, corners=(0, 6, 2, 5), self_row=11, sub_range=(1, 9))


def all_graphs():
    return [lengths()] + [first_hit(v) for v in FIRST_HIT_VARIANTS] + [diamonds(), chain(), two_islands()]


def level_graphs():
    """Every graph the level-by-level tests walk: all of them."""
    return all_graphs()


# ---------------------------------------------------------------------------------------------------------------------
# sources and pairs
# ---------------------------------------------------------------------------------------------------------------------
def batch64(g):
    """int64 [64]: the graph's four corner nodes (distinct) at bits 0, 31, 32 and 63, the other bits drawn with repeats
    from the graph's pool (all nodes unless it names one); bits 5 and 40 repeat the node of bit 63."""
    rng = np.random.default_rng([20261020, 10, g.n_nodes])
    pool = np.array(g.marks.get("pool", range(g.n_nodes)), np.int64)
    src = pool[rng.integers(0, pool.size, size=MAX_SOURCES)]
    corners = g.marks["corners"]
    assert len(set(corners)) == 4
    for b, node in zip(CORNER_BITS, corners):
        src[b] = node
    src[5] = src[40] = src[63]
    return src


def batch1(g):
    return np.array([g.marks["corners"][3]], np.int64)


def many_sources(g, count):
    """int64 [count] for the library on top: batch64 first, then further nodes, the last one a corner node."""
    rng = np.random.default_rng([20261020, 11, g.n_nodes, count])
    src = np.concatenate([batch64(g), rng.integers(0, g.n_nodes, size=count)])[:count]
    src[-1] = g.marks["corners"][0]
    return src


def pair_targets(g, sources, n_targets):
    """int64 [S, n_targets]: the graph's named targets first (if any), then random nodes; column 0 of the rows at the
    corner bits is the source itself."""
    rng = np.random.default_rng([20261020, 12, g.n_nodes, len(sources), n_targets])
    tgt = rng.integers(0, g.n_nodes, size=(len(sources), n_targets)).astype(np.int64)
    named = g.marks.get("targets", ())[:n_targets]
    tgt[:, :len(named)] = named
    if not named:
        for b in CORNER_BITS:
            if b < len(sources):
                tgt[b, 0] = sources[b]
    return tgt


def subset_active(g, sources):
    """A strict subset of the seeded bits: those of the sources that sit on one node (the graph's ``skip_node``, else the
    node of bit 63).  Every row that node reaches is then reached by every active source, while the other sources'
    bits still arrive at its neighbours: the rows the skip rule of lgc_bfs_level decides."""
    node = g.marks.get("skip_node", int(sources[63]))
    m = ZERO
    for b, s in enumerate(np.asarray(sources).tolist()):
        if s == node:
            m |= bit(b)
    return m


def valid_mask(sources, n_nodes):
    """``active`` as paths.py forms it: the bits of the batch's sources that lie inside the graph."""
    m = ZERO
    for b, s in enumerate(np.asarray(sources).tolist()):
        if 0 <= s < n_nodes:
            m |= bit(b)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# row plans: the planner's, and chunk lists it would never emit
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Plan:
    name: str
    short_max: int
    chunks: np.ndarray                       # int32 [C, 4]: (row, begin, end, slot); slot -1 = the row's only chunk

    @property
    def n_chunks(self):
        return self.chunks.shape[0]

    @property
    def multi_rows(self):
        return np.unique(self.chunks[self.chunks[:, 3] >= 0, 0])


def planned(g, short_max, chunk_len, row_begin=0, row_end=None):
    """``graph.build_row_plan`` (the host planner) on the graph's rowptr."""
    import torch
    from gnn_ecommerce_amd import graph as G
    row_end = g.n_nodes if row_end is None else row_end
    plan = G.build_row_plan(torch.from_numpy(np.array(g.rowptr)), row_begin, row_end, short_max, chunk_len)
    return Plan(f"planner({short_max},{chunk_len})", short_max, plan.chunks.numpy().astype(np.int32).reshape(-1, 4))


def _cut(g, short_max, row_begin, row_end, sizes_of):
    out, slot = [], 0
    for v in range(row_begin, row_end):
        b, e = int(g.rowptr[v]), int(g.rowptr[v + 1])
        if e - b <= short_max:
            continue
        sizes = [s for s in sizes_of(e - b) if s > 0]
        assert sum(sizes) == e - b
        at = b
        for s in sizes:
            out.append((v, at, at + s, slot if len(sizes) > 1 else -1))
            slot += len(sizes) > 1
            at += s
    return np.array(out, np.int32).reshape(-1, 4)


def hand_cut(g, short_max, row_begin=0, row_end=None):
    """Three chunk lists over the rows longer than ``short_max``: every such row cut as one entry plus the rest; as three
    unequal chunks (1, a third, the rest); and the planner's 16-entry chunks listed last to first.  A chunk list is any
    partition of the long rows into (row, begin, end) with slot >= 0 where a row has several; the result must not depend
    on it."""
    row_end = g.n_nodes if row_end is None else row_end
    one = _cut(g, short_max, row_begin, row_end, lambda n: (1, n - 1))
    three = _cut(g, short_max, row_begin, row_end, lambda n: (1, n // 3, n - 1 - n // 3) if n >= 3 else (1, n - 1))
    back = planned(g, short_max, 16, row_begin, row_end).chunks[::-1].copy()
    return [Plan(f"one_plus_rest({short_max})", short_max, one), Plan(f"three_unequal({short_max})", short_max, three),
            Plan(f"reversed({short_max},16)", short_max, back)]


def plans(g, row_begin=0, row_end=None):
    """Every plan a level test runs: the planner at PLAN_SETTINGS, the hand cuts with every non-empty row long
    (short_max 0) and with the rows above 8 entries long."""
    out = [planned(g, s, c, row_begin, row_end) for s, c in PLAN_SETTINGS]
    return out + hand_cut(g, 0, row_begin, row_end) + hand_cut(g, 8, row_begin, row_end)


def check_plan(g, plan, row_begin=0, row_end=None):
    """A plan lists every entry of every row of the range longer than short_max exactly once, nothing else, in bounds."""
    row_end = g.n_nodes if row_end is None else row_end
    covered = np.zeros(g.cols.size, np.int64)
    rows = set()
    for v, b, e, slot in plan.chunks.tolist():
        assert row_begin <= v < row_end and g.rowptr[v] <= b < e <= g.rowptr[v + 1], (plan.name, v, b, e)
        covered[b:e] += 1
        rows.add(v)
    for v in range(row_begin, row_end):
        b, e = int(g.rowptr[v]), int(g.rowptr[v + 1])
        long_row = e - b > plan.short_max
        assert (v in rows) == long_row and np.all(covered[b:e] == int(long_row)), (plan.name, v)
    assert covered.sum() == sum(int(g.lengths[v]) for v in rows)
    for v in rows:
        slots = plan.chunks[plan.chunks[:, 0] == v, 3]
        assert (slots.size == 1 and slots[0] == -1) or (slots.size > 1 and np.all(slots >= 0)), (plan.name, v)


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def init_ref(sources, n_nodes):
    """(seen, frontier, oob): every word 0, then bit b set at sources[b] in both; a source outside [0, n_nodes) sets the
    flag and no bit."""
    seen = np.zeros(n_nodes, U64)
    oob = False
    for b, s in enumerate(np.asarray(sources).tolist()):
        if 0 <= s < n_nodes:
            seen[s] |= bit(b)
        else:
            oob = True
    return seen, seen.copy(), oob


def row_or(rowptr, cols, v, frontier_in):
    return np.bitwise_or.reduce(frontier_in[cols[int(rowptr[v]):int(rowptr[v + 1])]], initial=ZERO)


def level_ref(rowptr, cols, row_begin, row_end, active, frontier_in, seen, frontier_out=None):
    """(frontier_out, seen_after, newly, bits) of one lgc_bfs_level.  For every row v of the range: a row with
    (~seen[v] & active) == 0 is finished, frontier_out[v] = 0; any other row gets fresh = (OR of frontier_in over the
    row's columns) & ~seen[v] -- masked by seen, not by active -- in frontier_out[v] and ORed into seen[v].  ``newly``
    counts the rows with fresh != 0, ``bits`` is the OR of their fresh words.  Rows outside the range keep what
    ``frontier_out`` held (zeros if it is not given) and their seen.  active == 0 launches nothing."""
    active = U64(active)
    out = np.zeros(seen.size, U64) if frontier_out is None else np.array(frontier_out, U64)
    seen_after = np.array(seen, U64)
    newly, bits = 0, ZERO
    if active == ZERO:
        return out, seen_after, newly, bits
    for v in range(row_begin, row_end):
        if (~seen[v] & active) == ZERO:
            out[v] = ZERO
            continue
        fresh = row_or(rowptr, cols, v, frontier_in) & ~seen[v]
        out[v] = fresh
        seen_after[v] |= fresh
        if fresh != ZERO:
            newly += 1
            bits |= fresh
    return out, seen_after, newly, bits


def resolve_ref(sources, targets, n_nodes, frontier, level, dist):
    """(dist_after, settled, oob) of one lgc_bfs_resolve: only pairs that hold UNSET are looked at; a source or target
    outside the graph gives -1, sets the flag and counts as settled; bit b of frontier[target] set gives ``level``."""
    out = np.array(dist, np.int32)
    settled, oob = 0, False
    for b, s in enumerate(np.asarray(sources).tolist()):
        for c, t in enumerate(np.asarray(targets)[b].tolist()):
            if out[b, c] != UNSET:
                continue
            if not (0 <= s < n_nodes and 0 <= t < n_nodes):
                out[b, c], oob = -1, True
                settled += 1
            elif frontier[t] & bit(b):
                out[b, c] = level
                settled += 1
    return out, settled, oob


def backtrack_ref(rowptr, cols, levels, n_levels, targets, dist, path_len, pick="first"):
    """paths int64 [S, T, path_len] of one lgc_bfs_backtrack.  A pair with 0 <= d < min(n_levels, path_len) and its target
    inside the graph: paths[d] = the target, and for l = d - 1 ... 0 paths[l] = the first column, in stored entry order,
    of the row of paths[l + 1] that has bit b set in levels[l]; positions past d are -1.  Where no column has the bit
    (levels and dist disagree) that position and everything below it are -1, the positions above it stay.  Every other
    pair: all -1.  ``pick`` = "last" / "smallest" are the WRONG rules the graphs must tell from the right one."""
    n_nodes = levels.shape[1]
    S, T = np.asarray(dist).shape
    paths = np.full((S, T, path_len), -1, np.int64)
    for b in range(S):
        for c in range(T):
            d, cur = int(dist[b, c]), int(targets[b, c])
            if not (0 <= d < n_levels and d < path_len and 0 <= cur < n_nodes):
                continue
            paths[b, c, d] = cur
            for l in range(d - 1, -1, -1):
                row = cols[int(rowptr[cur]):int(rowptr[cur + 1])]
                hits = row[(levels[l][row] & bit(b)) != ZERO]
                if hits.size == 0:
                    break
                cur = int({"first": hits[0], "last": hits[-1], "smallest": hits.min()}[pick])
                paths[b, c, l] = cur
    return paths


@dataclass(eq=False)
class LevelStep:
    """One lgc_bfs_level call of a search: its inputs and what the reference says it leaves."""
    level: int
    frontier_in: np.ndarray
    seen_in: np.ndarray
    frontier_out: np.ndarray
    seen_out: np.ndarray
    newly: int
    bits: np.uint64


def level_steps(g, sources, active=None, row_begin=0, row_end=None, max_levels=64):
    """The level calls of a search from ``sources`` until a level reaches nothing new (that level included), each from
    the reference's own state; rows outside the range start every call with SENTINEL in frontier_out."""
    row_end = g.n_nodes if row_end is None else row_end
    active = valid_mask(sources, g.n_nodes) if active is None else U64(active)
    seen, frontier, _ = init_ref(sources, g.n_nodes)
    steps = []
    for level in range(1, max_levels + 1):
        before = np.full(g.n_nodes, SENTINEL, U64)
        out, seen_after, newly, bits = level_ref(g.rowptr, g.cols, row_begin, row_end, active, frontier, seen, before)
        steps.append(LevelStep(level, frontier, seen, out, seen_after, newly, bits))
        if newly == 0:
            break
        # outside a sub-range the sentinel is not a frontier: the next level reads zeros there
        frontier = out.copy()
        frontier[:row_begin] = ZERO
        frontier[row_end:] = ZERO
        seen = seen_after
    return steps


def search_ref(g, sources, targets, max_hops=None):
    """(dist int32 [S, T], trace, levels) of the search paths.py describes, in batches of 64 sources: level 0 is
    lgc_bfs_init's frontier, every level ends with lgc_bfs_resolve, and a batch stops at the level where its last pair
    settles, where a level reaches nothing new, or at max_hops.  A pair still unset then gets -1 if its source's frontier
    has emptied, else -2.  ``trace``: one (batch, level, nodes newly reached, pairs settled) per level; ``levels``: per
    batch the uint64 [levels run, n_nodes] frontiers."""
    sources, targets = np.asarray(sources, np.int64), np.asarray(targets, np.int64)
    n = g.n_nodes
    dist = np.full(targets.shape, UNSET, np.int32)
    trace, kept = [], []
    for batch, lo in enumerate(range(0, sources.size, MAX_SOURCES)):
        src, tgt = sources[lo:lo + MAX_SOURCES], targets[lo:lo + MAX_SOURCES]
        active = valid_mask(src, n)
        seen, frontier, _ = init_ref(src, n)
        d = dist[lo:lo + MAX_SOURCES]
        unset, dead, level, levels = d.size, ZERO, 0, [frontier]
        while True:
            newly = 0
            if level > 0:
                frontier, seen, newly, bits = level_ref(g.rowptr, g.cols, 0, n, active, levels[-1], seen)
                levels.append(frontier)
                dead |= active & ~bits
            d[:], settled, _ = resolve_ref(src, tgt, n, frontier, level, d)
            unset -= settled
            trace.append((batch, level, newly, settled))
            emptied = level > 0 and newly == 0
            if unset == 0 or emptied or (max_hops is not None and level >= max_hops):
                break
            level += 1
        for b in range(src.size):
            gone = emptied or (dead & bit(b)) != ZERO
            d[b][d[b] == UNSET] = -1 if gone else -2
        kept.append(np.stack(levels))
    return dist, trace, kept


def keep_paths(g, sources, targets, dist, kept, max_len):
    """paths int64 [S, T, max_len + 1] as shortest_paths defines them: levels 0..max_len of every batch walked back."""
    out = np.full(targets.shape + (max_len + 1,), -1, np.int64)
    for batch, lo in enumerate(range(0, len(sources), MAX_SOURCES)):
        levels = kept[batch][:max_len + 1]
        out[lo:lo + MAX_SOURCES] = backtrack_ref(g.rowptr, g.cols, levels, levels.shape[0], targets[lo:lo + MAX_SOURCES],
                                                 dist[lo:lo + MAX_SOURCES], max_len + 1)
    return out
