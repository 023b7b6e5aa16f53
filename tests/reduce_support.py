"""An exact host reference of the middle-hop reduction builder (lgc_reduce_count / _fill / _gram_count / _gram_fill), the
named hand-built operators it is pinned on, the generated graphs of the size-dependent paths, and a driver that calls the
four C entry points directly (tests/test_reduce_host.py, tests/test_reduce_gpu.py, tests/test_eliminate_gpu.py).

The reference is written from the contract in include/lgconv_hip.h ("Middle-hop reduction of a user|item graph"), not from
the kernels: it works on a CSR (rowptr, columns, fp32 value bits), users are rows [0, split), items rows [split, n_nodes).
"""
from dataclasses import dataclass

import numpy as np
import torch

INT32_MAX = 2 ** 31 - 1
SPARE = 64                          # sentinel elements behind every output of call_builder
SENTINEL32 = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A


def f32_bits(values):
    """fp32 values -> their bit patterns as int32."""
    return np.asarray(values, dtype=np.float32).view(np.int32)


@dataclass
class Reduced:
    """What the four calls return for one input, every array int32 in the compact numbering (kept users 0 .. n_kept - 1,
    item i = n_kept + i); ``pairs_min`` / ``pairs_max``: the range totals[3] may lie in (equal on well-formed input)."""
    user_map: np.ndarray
    n_kept: int
    user_nnz: int
    nnz: int
    pairs_min: int
    pairs_max: int
    rowptr: np.ndarray
    entries: np.ndarray             # [nnz, 2]: column, value bits
    gram_rowptr: np.ndarray
    gram_entries: np.ndarray        # [nnz(G_L), 2]


def _keep_rule(rowptr, cols, split, n_nodes, max_deg, distinct_rows=False):
    """(eliminated bool [split], stored row length [split]).  ``distinct_rows``: the WRONG rule that counts the item rows
    naming a user once each (the host tests show that the named cases tell the two apart)."""
    deg = np.diff(rowptr[:split + 1])
    lo, hi = int(rowptr[split]), int(rowptr[n_nodes])
    c = cols[lo:hi]
    ok = (c >= 0) & (c < split)
    if distinct_rows:
        rows = np.repeat(np.arange(split, n_nodes), np.diff(rowptr[split:n_nodes + 1]))
        named = np.unique(np.stack([rows[ok], c[ok]]), axis=1)[1] if ok.any() else np.zeros(0, dtype=np.int64)
    else:
        named = c[ok]
    incount = np.bincount(named, minlength=split)[:split]
    return (deg <= max_deg) & (incount <= max_deg), deg


def _reduced_part(rowptr, cols, val_bits, split, n_nodes, gone, guards=True):
    """user_map and the reduced CSR: the surviving entries in CSR order, columns renumbered, value bits copied."""
    n_items = n_nodes - split
    user_map = np.where(gone, -1, np.cumsum(~gone) - 1).astype(np.int32)
    n_kept = int((~gone).sum())
    rows = np.repeat(np.arange(n_nodes), np.diff(rowptr))
    in_users, in_items = (cols >= 0) & (cols < split), (cols >= split) & (cols < n_nodes)
    kept_col = np.zeros(cols.size, dtype=bool)
    kept_col[in_users] = ~gone[cols[in_users]]
    kept_row = np.zeros(cols.size, dtype=bool)
    kept_row[rows < split] = ~gone[rows[rows < split]]
    survive = np.where(rows < split, kept_row & (in_items | (not guards)), kept_col)
    new_col = np.where(rows < split, cols - split + n_kept, 0)
    new_col[kept_col] = user_map[cols[kept_col]]
    new_row = np.where(rows < split, 0, rows - split + n_kept)
    new_row[kept_row] = user_map[rows[kept_row]]
    counts = np.bincount(new_row[survive], minlength=n_kept + n_items)
    rowptr_out = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    entries = np.stack([new_col[survive], val_bits[survive]], axis=1).astype(np.int32).reshape(-1, 2)
    user_nnz = int((survive & (rows < split)).sum())
    return user_map, n_kept, user_nnz, rowptr_out, entries


def _pack_gram(n_kept, n_items, key_rows, key_cols, sums):
    """G_L from its keys in ascending (row, column) order and their fp64 sums: rounded once to fp32."""
    counts = np.bincount(np.asarray(key_rows, dtype=np.int64), minlength=n_items)
    rowptr = np.concatenate([np.zeros(n_kept + 1, dtype=np.int64), np.cumsum(counts)]).astype(np.int32)
    ent = np.zeros((len(sums), 2), dtype=np.int32)
    ent[:, 0] = np.asarray(key_cols, dtype=np.int64) + n_kept
    ent[:, 1] = np.asarray(sums, dtype=np.float64).astype(np.float32).view(np.int32)
    return rowptr, ent


def reduce_reference(rowptr, cols, val_bits, split, n_nodes, max_deg, order="expansion", distinct_rows=False, start=0.0,
                     guards=True):
    """The loop form.  ``order``: "expansion" is the contract; "columns" (each run summed in ascending order of the
    eliminated user, the order a column-sorted item row would give) and "reversed" (equal keys in the reverse of their
    expansion order, what an unstable sort may leave) are WRONG orders for the host tests to tell apart; so are
    ``distinct_rows`` (_keep_rule), a ``start`` of the sums other than +0.0 and ``guards=False`` (a kept user row keeps its
    entries whatever their column)."""
    rowptr, cols = np.asarray(rowptr, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    val_bits = np.asarray(val_bits, dtype=np.int32)
    vals = val_bits.view(np.float32).astype(np.float64)
    n_items = n_nodes - split
    gone, deg = _keep_rule(rowptr, cols, split, n_nodes, max_deg, distinct_rows)
    user_map, n_kept, user_nnz, rowptr_out, entries = _reduced_part(rowptr, cols, val_bits, split, n_nodes, gone, guards)
    pairs_min = pairs_max = 0
    key_rows, key_cols, sums = [], [], []
    for i in range(n_items):
        runs = {}                                                   # item column -> its products in expansion order
        item_entries = range(int(rowptr[split + i]), int(rowptr[split + i + 1]))
        if order == "columns":
            item_entries = sorted(item_entries, key=lambda e: cols[e])          # stable: ties keep the CSR order
        for e in item_entries:
            u = int(cols[e])
            if not (0 <= u < split) or not gone[u]:
                continue
            pairs_max += int(deg[u])
            for f in range(int(rowptr[u]), int(rowptr[u + 1])):
                j = int(cols[f])
                if split <= j < n_nodes:
                    pairs_min += 1
                    runs.setdefault(j - split, []).append(float(vals[e]) * float(vals[f]))
        for j in sorted(runs):
            total = start                                           # +0: a lone product -0.0 is stored as +0.0
            for p in (reversed(runs[j]) if order == "reversed" else runs[j]):
                total = total + p
            key_rows.append(i), key_cols.append(j), sums.append(total)
    gram_rowptr, gram_entries = _pack_gram(n_kept, n_items, key_rows, key_cols, sums)
    return Reduced(user_map, n_kept, user_nnz, int(rowptr_out[-1]), pairs_min, pairs_max, rowptr_out, entries, gram_rowptr,
                   gram_entries)


def reduce_reference_fast(rowptr, cols, val_bits, split, n_nodes, max_deg):
    """The same answer for large inputs: the pairs in expansion order, one stable sort by key, then one pass per position
    within a run, so that every run is still summed sequentially from +0."""
    rowptr, cols = np.asarray(rowptr, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    val_bits = np.asarray(val_bits, dtype=np.int32)
    vals = val_bits.view(np.float32).astype(np.float64)
    n_items = n_nodes - split
    gone, deg = _keep_rule(rowptr, cols, split, n_nodes, max_deg)
    user_map, n_kept, user_nnz, rowptr_out, entries = _reduced_part(rowptr, cols, val_bits, split, n_nodes, gone)
    lo, hi = int(rowptr[split]), int(rowptr[n_nodes])
    e = np.arange(lo, hi)
    c = cols[lo:hi]
    ok = (c >= 0) & (c < split)
    ok[ok] = gone[c[ok]]
    e, u = e[ok], c[ok]                                             # the expanded item entries, in CSR order
    cnt = deg[u]
    pairs_max = int(cnt.sum())
    first = np.cumsum(cnt) - cnt
    which = np.repeat(np.arange(e.size), cnt)                       # the pairs of one entry are consecutive ...
    f = rowptr[u][which] + (np.arange(pairs_max) - first[which])    # ... and in the order of the user's row
    item_col = (cols[f] >= split) & (cols[f] < n_nodes)
    which, f = which[item_col], f[item_col]
    pairs_min = int(which.size)
    i = np.repeat(np.arange(n_nodes), np.diff(rowptr))[e[which]] - split
    key = i * n_items + (cols[f] - split)
    prod = vals[e[which]] * vals[f]
    by_key = np.argsort(key, kind="stable")
    key, prod = key[by_key], prod[by_key]
    head = np.ones(key.size, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    run = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    rank = np.arange(key.size) - start[run] if key.size else np.zeros(0, dtype=np.int64)
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=1))]) if key.size else np.zeros(1, dtype=np.int64)
    sums = np.zeros(start.size, dtype=np.float64)
    for p in range(bounds.size - 1):                                # every run appears at most once per position
        sel = by_rank[bounds[p]:bounds[p + 1]]
        sums[run[sel]] = sums[run[sel]] + prod[sel]
    gram_rowptr, gram_entries = _pack_gram(n_kept, n_items, key[start] // n_items, key[start] % n_items, sums)
    return Reduced(user_map, n_kept, user_nnz, int(rowptr_out[-1]), pairs_min, pairs_max, rowptr_out, entries, gram_rowptr,
                   gram_entries)


def same(a: Reduced, b: Reduced):
    """The field in which two results differ, or None."""
    for f in ("n_kept", "user_nnz", "nnz", "pairs_min", "pairs_max"):
        if getattr(a, f) != getattr(b, f):
            return f
    for f in ("user_map", "rowptr", "entries", "gram_rowptr", "gram_entries"):
        if not np.array_equal(getattr(a, f), getattr(b, f)):
            return f
    return None


# ----------------------------------------------------------------------------------------
# named hand-built operators
# ----------------------------------------------------------------------------------------
@dataclass
class Case:
    rowptr: np.ndarray              # int32 [n_nodes + 1]
    cols: np.ndarray                # int32 [n_edges]
    val_bits: np.ndarray            # int32 [n_edges]
    split: int
    n_nodes: int
    well_formed: bool = True

    @property
    def largest_degree(self) -> int:
        named = self.cols[self.rowptr[self.split]:]
        named = named[(named >= 0) & (named < self.split)]
        return int(max(np.diff(self.rowptr).max(initial=0), np.bincount(named, minlength=1).max()))

    def thresholds(self):
        """The T every case runs at (0 is legal through the C ABI only)."""
        return sorted({0, 1, 2, 3, self.largest_degree, INT32_MAX})


def _case(split, rows, well_formed=True):
    """A case from its rows, each a list of (column as a node id, fp32 value); users first."""
    flat = [en for r in rows for en in r]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    cols = np.array([c for c, _ in flat], dtype=np.int32)
    bits = f32_bits([v for _, v in flat]) if flat else np.zeros(0, dtype=np.int32)
    return Case(rowptr, cols, bits, split, len(rows), well_formed)


def case_order_shows():
    """Two runs whose fp32 value depends on the order of the sum.  Users 0-3, items 4-7.
    Run (item 4, item 5) goes through the eliminated users 2, 0, 1 -- item 4's row lists them in that order -- with the
    products 2^60, -2^60, 1: the contract's order gives 1.0.  Summed in ascending user column (a column-sorted item row, or
    a sort that also orders by user) it is (-2^60 + 1) + 2^60 = 0.0; in the reverse order (an unstable sort of equal keys)
    (1 - 2^60) + 2^60 = 0.0; as the tree p0 + (p1 + p2) it is 0.0 as well; fp32 accumulation gives 0.0 too (the products
    need fp64: 2^30 * 2^30).  Only (p0, p1, p2) and (p1, p0, p2) give 1.0.
    Run (item 6, item 7) has its three products 2^60, -2^60, 1 inside user 3's row, which lists item 7 three times: it
    pins the order WITHIN one entry's pairs (the reverse, or a sort of the row by value, gives 0.0)."""
    big = 2.0 ** 30
    return _case(4, [[(5, big)], [(5, 1.0)], [(5, big)], [(7, 2.0 ** 60), (7, -2.0 ** 60), (7, 1.0)],
                     [(2, big), (0, -big), (1, 1.0)], [], [(3, 1.0)], []])


def case_cancels_to_zero():
    """Users 0-2, items 3-5.  Run (3, 4): 2 * 1.5 + (-2) * 1.5 = exactly zero, stored with bits 0x00000000 (structure, not
    value, decides what is stored).  Run (5, 5): the single product 1 * -0.0 = -0.0 is stored as +0.0, because the sum
    starts at +0: bits 0x00000000, not 0x80000000."""
    return _case(3, [[(4, 1.5)], [(4, 1.5)], [(5, -0.0)], [(0, 2.0), (1, -2.0)], [], [(2, 1.0)]])


def case_duplicates():
    """Users 0-1, items 2-3.  User 0 twice in item 2's row and item 3 twice in user 0's row: four products in the one run
    (2, 3), 6 + 10 + 1.5 + 2.5 = 20.  User 1 has one entry and is named three times by the single item row 3: at T = 2 it
    is KEPT (incount counts entries, 3 > 2; counting distinct rows would say 1 and eliminate it), at T = 3 it goes."""
    return _case(2, [[(3, 3.0), (3, 5.0)], [(2, 7.0)], [(0, 2.0), (0, 0.5)], [(1, 1.0), (1, 2.0), (1, 4.0)]])


def case_threshold():
    """Users 0-3, items 4-6, directed.  At T = 2: user 0 has degree T (eliminated), user 1 degree T + 1 (kept), user 2
    degree 1 and incount T (eliminated), user 3 degree 1 and incount T + 1 (kept)."""
    return _case(4, [[(4, 1.0), (5, 2.0)], [(4, 1.0), (5, 1.0), (6, 1.0)], [(6, 3.0)], [(6, 5.0)],
                     [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0)], [(0, 2.0), (2, 2.0), (3, 2.0)], [(3, 4.0)]])


def case_wrong_side():
    """Users 0-1, items 2-3.  User 0 (eliminated at T = 4) and user 1 (kept, five entries) each name a user, a negative
    column and a column >= n_nodes beside their items; item 2's row names an item, a negative column and a column
    >= n_nodes beside users 0 and 1.  All of them are dropped and not counted: user_map, both CSRs and nnz(G_L) are those
    of the graph without them -- only the stored row length (the keep rule, the upper end of totals[3]) sees them."""
    return _case(2, [[(1, 1.0), (-1, 2.0), (6, 3.0), (3, 4.0)], [(0, 1.0), (-3, 2.0), (4, 3.0), (2, 5.0), (3, 6.0)],
                     [(3, 9.0), (0, 2.0), (-2, 9.0), (1, 3.0), (7, 9.0)], [(1, 7.0)]], well_formed=False)


def case_empty_rows():
    """Users 0-4, items 5-8.  User 0 has no row but is named; user 2 is named by nobody; user 4 (the last) has no row and
    nobody names it; the first and the last item row are empty."""
    return _case(5, [[], [(6, 1.5), (7, 2.5)], [(6, 3.0)], [(6, 1.0), (7, 1.0), (8, 1.0), (5, 1.0)], [],
                     [], [(0, 2.0), (1, 3.0), (3, 0.5)], [(1, 4.0), (0, 1.0), (3, 2.0)], []])


def case_all_user_side():
    """rowptr[split] == n_edges: only the user rows hold entries.  Users 0-2, items 3-4."""
    return _case(3, [[(3, 1.0)], [(3, 2.0), (4, 3.0), (3, 4.0), (4, 5.0)], [(4, 6.0), (4, 7.0)], [], []])


def case_all_item_side():
    """rowptr[split] == 0: only the item rows hold entries.  Users 0-2, items 3-4; user 1 is named four times."""
    return _case(3, [[], [], [], [(0, 1.0), (1, 2.0), (1, 3.0)], [(1, 4.0), (2, 5.0), (1, 6.0)]])


def case_no_entries():
    """n_edges = 0.  Users 0-1, items 2-3."""
    return _case(2, [[], [], [], []])


def case_smallest():
    """split = 1, n_nodes = 2, one entry each way: at T >= 1 G_L is the one diagonal entry 2 * 3 = 6."""
    return _case(1, [[(1, 3.0)], [(0, 2.0)]])


def case_nothing_left():
    """Everyone is eliminated at T >= 2 and no item row names anybody: n_kept = 0 and both CSRs are empty.
    Users 0-2, items 3-4."""
    return _case(3, [[(3, 1.0)], [(4, 2.0), (3, 0.5)], [(4, 3.0)], [], []])


def case_kept_but_unnamed():
    """At T = 2 users 1 and 3 are kept (three and four entries) and no item row names them: the item part of the reduced
    CSR is empty while G_L (through users 0 and 2) is not.  Users 0-3, items 4-6."""
    return _case(4, [[(4, 1.0), (5, 2.0)], [(4, 1.0), (5, 1.0), (6, 1.0)], [(6, 3.0)], [(4, 2.0), (5, 2.0), (6, 2.0), (4, 2.0)],
                     [(0, 1.5), (2, 0.5)], [(0, 2.5)], [(2, 4.0)]])


def case_dense_block():
    """Users 0-3, items 4-9.  Users 0-2 (four entries each, items {0,1,2,3}, {2,3,4,5}, {0,1,4,5}) join every pair of the
    six items: at T = 4 G_L is the full 6 x 6 block, diagonal included, columns ascending although the item rows list
    their users in descending order and the user rows their items in no order.  User 3 (seven entries) stays."""
    user_items = ([3, 0, 2, 1], [5, 2, 4, 3], [0, 5, 1, 4])
    rows = [[(4 + j, 1.0 + 0.25 * j + u) for j in items] for u, items in enumerate(user_items)]
    rows.append([(4 + j % 6, 0.5 + j) for j in range(7)])
    for j in range(6):
        rows.append([(u, 3.0 + 0.125 * j - 0.5 * u) for u in (3, 2, 1, 0) if u == 3 or j in user_items[u]])
    return _case(4, rows)


CASES = {"order_shows": case_order_shows, "cancels_to_zero": case_cancels_to_zero, "duplicates": case_duplicates,
         "threshold": case_threshold, "wrong_side": case_wrong_side, "empty_rows": case_empty_rows,
         "all_user_side": case_all_user_side, "all_item_side": case_all_item_side, "no_entries": case_no_entries,
         "smallest": case_smallest, "nothing_left": case_nothing_left, "kept_but_unnamed": case_kept_but_unnamed,
         "dense_block": case_dense_block}


# ----------------------------------------------------------------------------------------
# generated inputs
# ----------------------------------------------------------------------------------------
def csr_from_edges(ei, ew, n_nodes):
    """(rowptr, cols, value bits) of an edge list with row = target, column = source, rows in edge order (a stable sort):
    the layout tests/reduced_concat_support.reduced_csr_numpy walks."""
    src, dst = ei[0].numpy(), ei[1].numpy()
    order = np.argsort(dst, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n_nodes))]).astype(np.int32)
    return rowptr, src[order].astype(np.int32), ew.numpy().astype(np.float32)[order].view(np.int32)


def interactions_csr(users, items, n_users, n_items, seed):
    """A user|item CSR from (user, item) interactions, both directions, duplicates kept: user rows in list order, item rows
    in list order too; values uniform in [0.5, 2), independent per direction."""
    rng = np.random.default_rng(seed)
    by_user, by_item = np.argsort(users, kind="stable"), np.argsort(items, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.concatenate([np.bincount(users, minlength=n_users),
                                                            np.bincount(items, minlength=n_items)]))]).astype(np.int32)
    cols = np.concatenate([items[by_user] + n_users, users[by_item]]).astype(np.int32)
    bits = rng.uniform(0.5, 2.0, cols.size).astype(np.float32).view(np.int32)
    return Case(rowptr, cols, bits, n_users, n_users + n_items)


LARGE_T = 3


def large_case():
    """1,130,000 interactions: 500,000 users of 1-3 entries (eliminated at T = 3), 20,000 of 4-9 (kept), 3,000 items drawn
    with a skew.  The item half holds more than 1,048,576 entries: the counting kernel's grid (4,096 blocks of 256) takes
    a second trip, and the scans and the sort of about 2.6 M pairs span many tiles."""
    rng = np.random.default_rng(31)
    deg = np.concatenate([1 + rng.integers(0, 3, 500_000), 4 + rng.integers(0, 6, 20_000)])
    deg = deg[rng.permutation(deg.size)]
    users = np.repeat(np.arange(deg.size), deg)
    items = np.minimum((3000 * rng.random(users.size) ** 2).astype(np.int64), 2999)
    return interactions_csr(users, items, deg.size, 3000, 32)


def complete_bipartite(n_users, n_items):
    """Every user x every item, both directions, as an edge list (edge_index int64 [2, E], edge_weight fp32 [E])."""
    u = np.repeat(np.arange(n_users), n_items)
    i = np.tile(np.arange(n_items), n_users) + n_users
    ei = torch.from_numpy(np.stack([np.concatenate([i, u]), np.concatenate([u, i])]))
    ew = torch.from_numpy(np.random.default_rng(41).uniform(0.5, 2.0, ei.size(1)).astype(np.float32))
    return ei, ew


AUTO_USERS, AUTO_ITEMS = 250_000, 400


def auto_graph():
    """The graph on which every default switches the reduction and the concatenated operator on: 150,000 users of 8 entries
    (1.2 M entries: the kept half sweeps too) and 100,000 users of 1-4 entries, shuffled, over 400 items.  About 1.45 M
    interactions; at T = 4 G_L is nearly the dense 400 x 400 block, about a third of an entry per entry removed."""
    rng = np.random.default_rng(51)
    deg = np.concatenate([np.full(150_000, 8), 1 + rng.integers(0, 4, 100_000)])
    deg = deg[rng.permutation(deg.size)]
    u = np.repeat(np.arange(deg.size), deg)
    i = rng.integers(0, AUTO_ITEMS, u.size) + AUTO_USERS
    assert i.min() == AUTO_USERS, "the first item must appear in an edge"
    ei = torch.from_numpy(np.stack([np.concatenate([i, u]), np.concatenate([u, i])]))
    ew = torch.from_numpy(rng.uniform(0.5, 2.0, ei.size(1)).astype(np.float32))
    return ei, ew, AUTO_USERS, AUTO_USERS + AUTO_ITEMS


# ----------------------------------------------------------------------------------------
# the four C entry points, called directly
# ----------------------------------------------------------------------------------------
def _guarded(n, width, dtype, device):
    shape = (n + SPARE,) if width == 1 else (n + SPARE, width)
    return torch.full(shape, SENTINEL64 if dtype == torch.int64 else SENTINEL32, dtype=dtype, device=device)


def _take(buf, n, what):
    """The first n elements of a guarded output on the host; everything behind them must still be the sentinel."""
    host = buf.cpu().numpy()
    sentinel = SENTINEL64 if host.dtype == np.int64 else SENTINEL32
    assert (host[n:] == sentinel).all(), f"{what}: written behind its {n} elements"
    return host[:n].copy()


def call_builder(device, case, max_deg, fill=0x00, short=False):
    """lgc_reduce_count, _fill, _gram_count, _gram_fill on one case, through ``_native`` directly.  Every output has SPARE
    sentinel elements behind it, asserted untouched.  ``fill``: the byte both workspaces are prefilled with (a missing
    memset hides behind fresh zeroed memory).  ``short``: ``n_out`` one below the true size in both fill calls -- the
    buffers keep their full size, and the element at ``n_out`` must keep the sentinel.
    Returns a dict of host arrays; ``gram_*`` are None where the pair count does not fit (workspace size 0)."""
    from gnn_ecommerce_amd import _native
    lib = _native.load()
    i32 = dict(dtype=torch.int32, device=device)
    n_nodes, split, n_edges, n_items = case.n_nodes, case.split, int(case.cols.size), case.n_nodes - case.split
    rowptr = torch.from_numpy(case.rowptr).to(device)
    entries = torch.from_numpy(np.stack([case.cols, case.val_bits], axis=1).astype(np.int32).reshape(-1, 2)).to(device)
    args = (_native.ptr(rowptr), _native.ptr(entries) if n_edges else None, n_nodes, n_edges, split)
    ws_bytes = lib.lgc_reduce_workspace_bytes(n_nodes, n_edges)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=device)
    user_map, totals = _guarded(split, 1, torch.int32, device), _guarded(4, 1, torch.int64, device)
    out = {}
    with torch.cuda.device(device):
        st = _native.stream_of(device)
        _native.check(lib.lgc_reduce_count(*args, int(max_deg), _native.ptr(ws), ws_bytes, _native.ptr(user_map),
                                           _native.ptr(totals), st), "lgc_reduce_count")
        out["user_map"] = _take(user_map, split, "user_map")
        out["totals"] = _take(totals, 4, "totals")
        n_h, _, nnz, n_pairs = (int(v) for v in out["totals"])
        assert 0 <= n_h <= split and 0 <= nnz <= n_edges
        n_out = nnz - 1 if (short and nnz > 0) else nnz
        rowptr_out, entries_out = _guarded(n_h + n_items + 1, 1, torch.int32, device), _guarded(nnz, 2, torch.int32, device)
        _native.check(lib.lgc_reduce_fill(*args, _native.ptr(ws), _native.ptr(user_map), n_h, n_out, _native.ptr(rowptr_out),
                                          _native.ptr(entries_out), st), "lgc_reduce_fill")
        out["rowptr_out"] = _take(rowptr_out, n_h + n_items + 1, "rowptr_out")
        out["entries_out"] = _take(entries_out, n_out, "entries_out")
        gws_bytes = lib.lgc_reduce_gram_workspace_bytes(n_pairs)
        out["gram_workspace_bytes"] = gws_bytes
        out["total"] = out["gram_rowptr"] = out["gram_entries"] = None
        if gws_bytes == 0:
            return out
        gws = torch.full((gws_bytes,), fill, dtype=torch.uint8, device=device)
        total = _guarded(1, 1, torch.int64, device)
        _native.check(lib.lgc_reduce_gram_count(*args, _native.ptr(ws), n_pairs, _native.ptr(gws), gws_bytes,
                                                _native.ptr(total), st), "lgc_reduce_gram_count")
        out["total"] = int(_take(total, 1, "total")[0])
        gram_nnz = out["total"]
        assert 0 <= gram_nnz <= n_pairs
        g_out = gram_nnz - 1 if (short and gram_nnz > 0) else gram_nnz
        gram_rowptr, gram_entries = _guarded(n_h + n_items + 1, 1, torch.int32, device), _guarded(gram_nnz, 2, torch.int32, device)
        _native.check(lib.lgc_reduce_gram_fill(_native.ptr(gws), n_pairs, n_h, n_items, g_out, _native.ptr(gram_rowptr),
                                               _native.ptr(gram_entries), st), "lgc_reduce_gram_fill")
        out["gram_rowptr"] = _take(gram_rowptr, n_h + n_items + 1, "gram_rowptr")
        out["gram_entries"] = _take(gram_entries, g_out, "gram_entries")
    return out


def assert_equals_reference(got, want: Reduced, well_formed=True, short=False):
    """Every output of every call against the reference, for equality, value bits included."""
    assert np.array_equal(got["user_map"], want.user_map), "user_map"
    assert [int(v) for v in got["totals"][:3]] == [want.n_kept, want.user_nnz, want.nnz], "totals[0..2]"
    pairs = int(got["totals"][3])
    if well_formed:
        assert want.pairs_min == want.pairs_max
        assert pairs == want.pairs_min, "totals[3]: the exact pair count on well-formed input"
    else:
        assert want.pairs_min <= pairs <= want.pairs_max, "totals[3]: the documented range"
    assert np.array_equal(got["rowptr_out"], want.rowptr), "rowptr_out"
    cut = 1 if (short and want.nnz > 0) else 0
    assert np.array_equal(got["entries_out"], want.entries[:want.nnz - cut]), "entries_out"
    assert got["total"] == want.gram_entries.shape[0], "*total"
    assert np.array_equal(got["gram_rowptr"], want.gram_rowptr), "gram rowptr"
    cut = 1 if (short and want.gram_entries.shape[0] > 0) else 0
    assert np.array_equal(got["gram_entries"], want.gram_entries[:want.gram_entries.shape[0] - cut]), "gram entries"
