"""Reference, path rule and case table for full-rank evaluation, lgc_rank_positions (tests/test_fullrank_host.py and
tests/test_fullrank_gpu.py).  Everything here is numpy; no project code is imported.

``ranks_ref`` takes a score panel -- row r holds the scores of pair r's user against every item -- and does no
floating-point arithmetic of its own beyond the ``x 0`` of a seen item (``topk_support.masked_ref``); the order is
``topk_support.order_keys``' and everything after it is integer counting.  ``metrics_ref`` restates the per-user metrics
in float64.  ``paths`` restates which of the kernels' paths a case reaches; only the host tests use it, to prove that the
case table reaches every path -- the device tests never branch on it."""
import numpy as np

from topk_support import masked_ref, order_keys

ROW_TILE, ITEM_TILE, WAVE = 64, 128, 64          # pairs of a workgroup, items of a tile, list entries of a round
MODES = ("zero", "remove")
ALL_PATHS = {"vec", "dword", "one_tile", "several_tiles", "ragged_tile", "one_slice", "several_slices", "clamped_slices",
             "one_row_tile", "several_row_tiles", "list_0", "list_1", "list_64", "list_65", "list_129", "p_seen", "p_unseen",
             "mode_zero", "mode_remove", "no_lists"}


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ----------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------
def seen_mask(entries, n_items):
    """The 0 / 1 row a user's list stands for: entries outside [0, n_items) are ignored, a repeated one counts once."""
    mask = np.zeros(n_items, dtype=np.float32)
    if entries is not None:
        e = np.asarray(entries, dtype=np.int64)
        mask[e[(e >= 0) & (e < n_items)]] = 1.0
    return mask


def ranks_ref(panel, pair_items, lists=None, mode="zero", valid=None):
    """(rank, n_equal, n_cand int32 [n], value fp32 [n]).  ``panel``: fp32 [n, n_items]; ``pair_items``: int [n];
    ``lists``: per pair the list entries of its user (any iterable of ints, or None), or None for no lists; ``valid``:
    bool [n], False = a pair with a bad id (-1, -1, 0, 0)."""
    assert mode in MODES
    panel = np.asarray(panel, dtype=np.float32)
    n, n_items = panel.shape
    rank, n_equal, n_cand = (np.zeros(n, dtype=np.int32) for _ in range(3))
    value = np.zeros(n, dtype=np.float32)
    idx = np.arange(n_items)
    for r in range(n):
        if valid is not None and not valid[r]:
            rank[r] = n_equal[r] = -1
            continue
        p = int(pair_items[r])
        seen = seen_mask(None if lists is None else lists[r], n_items)
        m = masked_ref(panel[r], seen) if mode == "zero" else panel[r]
        keys = order_keys(m).astype(np.int64)
        cand = np.ones(n_items, dtype=bool) if mode == "zero" else seen == 0
        n_cand[r] = int(cand.sum())
        value[r] = m[p]
        if not cand[p]:
            rank[r] = n_equal[r] = -1
            continue
        others = cand & (idx != p)
        rank[r] = int(np.count_nonzero(others & ((keys > keys[p]) | ((keys == keys[p]) & (idx < p)))))
        n_equal[r] = int(np.count_nonzero(others & (keys == keys[p])))
    return rank, n_equal, n_cand, value


def metrics_ref(rank, n_cand, owner, lengths, ks):
    """Per user, float64: auc, mpr, rr, recall [n, C], hit [n, C] from per-pair ranks (rank < 0 does not count)."""
    n = len(lengths)
    auc, mpr, rr = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n)
    recall, hit = np.zeros((n, len(ks))), np.zeros((n, len(ks)))
    for j in range(n):
        mine = [int(x) for x, o in zip(rank, owner) if o == j and x >= 0]
        ncs = [int(c) for x, c, o in zip(rank, n_cand, owner) if o == j and x >= 0]
        big_p = len(mine)
        if big_p:
            n_c = max(ncs)
            if n_c > big_p:
                auc[j] = 1.0 - float(sum(mine) - big_p * (big_p - 1) // 2) / float(big_p * (n_c - big_p))
            if n_c > 1:
                mpr[j] = float(sum(mine)) / float(big_p * (n_c - 1))
            rr[j] = 1.0 / float(min(mine) + 1)
        for ci, k in enumerate(ks):
            inside = sum(1 for x in mine if x < k)
            recall[j, ci] = float(inside) / float(lengths[j])
            hit[j, ci] = 1.0 if inside else 0.0
    return auc, mpr, rr, recall, hit


# ----------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------
LIST_LENGTHS = (0, 1, 64, 65, 129)


class Case:
    """One shape: tables of width ``dim`` (``layout`` "aligned": 16-byte rows, "strided": row stride dim + 3 from a
    misaligned base), ``n_items`` items, ``n_pairs`` pairs over ``n_users`` users, the slice counts to ask for, and whether
    the users have lists (user u's list has LIST_LENGTHS[u % 5] entries)."""

    def __init__(self, name, dim, layout, n_items, n_pairs, slices, lists=True, n_users=10, seed=0):
        self.name, self.dim, self.layout, self.n_items, self.n_pairs = name, dim, layout, n_items, n_pairs
        self.slices, self.lists, self.n_users, self.seed = tuple(slices), lists, n_users, seed

    def build(self, kind="int"):
        """(users fp32 [n_users, dim], items fp32 [n_items, dim], pair_users, pair_items, ptr, entries).  ``kind`` "int":
        small integers, so that ties are common and every sum is exact; "float": normal deviates, so that every step of the
        chain rounds.  Pairs and lists do not depend on it; a user with a list has p seen in some pairs and not in others
        where that can be."""
        rng = np.random.default_rng(1000 + self.seed)
        if kind == "int":
            users = f32(rng.integers(-2, 3, size=(self.n_users, self.dim)))
            items = f32(rng.integers(-2, 3, size=(self.n_items, self.dim)))
        else:
            users, items = f32(rng.standard_normal((self.n_users, self.dim))), f32(rng.standard_normal((self.n_items, self.dim)))
        rng = np.random.default_rng(2000 + self.seed)
        lists = []
        for u in range(self.n_users):
            length = LIST_LENGTHS[u % len(LIST_LENGTHS)] if self.lists else 0
            # ascending, with repeats and entries on either side of [0, n_items)
            lists.append(np.sort(rng.integers(-2, self.n_items + 2, size=length)).astype(np.int64))
        ptr = np.zeros(self.n_users + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=ptr[1:])
        entries = np.concatenate(lists) if ptr[-1] else np.zeros(0, dtype=np.int64)
        pair_users = rng.integers(0, self.n_users, size=self.n_pairs).astype(np.int64)
        pair_items = rng.integers(0, self.n_items, size=self.n_pairs).astype(np.int64)
        edge = [i for i in (0, 127, 128, self.n_items - 1) if i < self.n_items]
        for r in range(self.n_pairs):
            inside = [int(x) for x in lists[pair_users[r]] if 0 <= x < self.n_items]
            if r % 3 == 0 and inside:
                pair_items[r] = inside[r % len(inside)]                     # p is seen
            elif r % 3 == 1:
                pair_items[r] = edge[(r // 3) % len(edge)]                   # p at a tile edge
        return users, items, pair_users, pair_items, ptr, entries

    def vec(self):
        return self.layout == "aligned" and self.dim % 4 == 0


def slices_used(slices, n_pairs, n_items):
    """The library's rule: the count asked for, or with 0 the smallest that gives about 512 workgroups; at most 64 and at
    most one per item tile."""
    item_tiles, row_tiles = -(-n_items // ITEM_TILE), max(1, -(-n_pairs // ROW_TILE))
    s = slices if slices > 0 else -(-512 // row_tiles)
    return max(1, min(s, 64, item_tiles))


def paths(case):
    """The names of ALL_PATHS a case reaches (over its slice counts, both modes, with and without lists)."""
    got = {"vec" if case.vec() else "dword", "mode_zero", "mode_remove", "no_lists"}
    tiles = -(-case.n_items // ITEM_TILE)
    got.add("one_tile" if tiles == 1 else "several_tiles")
    if case.n_items % ITEM_TILE:
        got.add("ragged_tile")
    for s in case.slices:
        used = slices_used(s, case.n_pairs, case.n_items)
        got.add("one_slice" if used == 1 else "several_slices")
        if s > used:
            got.add("clamped_slices")
    got.add("one_row_tile" if case.n_pairs <= ROW_TILE else "several_row_tiles")
    if case.lists:
        _, _, pair_users, pair_items, ptr, entries = case.build()
        for u, p in zip(pair_users, pair_items):
            mine = entries[ptr[u]:ptr[u + 1]]
            got.add(f"list_{len(mine)}")
            got.add("p_seen" if p in mine else "p_unseen")
    return got


ALL_SLICES = (0, 1, 2, 3, 64)
CASES = [
    Case("d1", 1, "strided", 129, 130, ALL_SLICES, seed=1),
    Case("d3", 3, "strided", 2, 63, (0, 64), seed=2),
    Case("d4_vec", 4, "aligned", 641, 65, ALL_SLICES, seed=3),
    Case("d4", 4, "strided", 1, 1, (0, 1, 2), seed=4),
    Case("d5", 5, "strided", 127, 64, (0, 3), seed=5),
    Case("d16_vec", 16, "aligned", 128, 1, (0, 2), seed=6),
    Case("d17", 17, "strided", 257, 130, ALL_SLICES, seed=7),
    Case("d63", 63, "strided", 641, 63, (0, 2, 64), seed=8),
    Case("d64_vec", 64, "aligned", 257, 65, ALL_SLICES, seed=9),
    Case("d64", 64, "strided", 129, 64, (1, 3), seed=10),
    Case("d90", 90, "strided", 641, 130, ALL_SLICES, seed=11),
    Case("d256_vec", 256, "aligned", 129, 65, (0, 2), seed=12),
    Case("d256", 256, "strided", 257, 63, (1, 64), seed=13),
]
CASE_NAMES = [c.name for c in CASES]


def case(name):
    return next(c for c in CASES if c.name == name)
