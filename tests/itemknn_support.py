"""Reference and case table for the item-kNN recommender tests (lgc_knn_recommend).

The reference walks a basket in list order and keeps, per candidate, the score in numpy float32 SCALARS -- one rounded
operation per step: the product ``w * v`` (with weights), then ``acc + term`` -- and the votes in Python integers; entries
outside their table are skipped and flagged.  It then applies the eligibility rule and ranks with
``topk_support.topk_ref``, the order of lgc_mask_topk, and writes a value as the kernel's key does: every NaN as
0x7FFFFFFF, -0 as +0.  ``fused`` and ``entry_order`` exist for the mutants of the host tests only."""
import numpy as np

import chain_support as chain
import topk_support as ts

MAX_K, MAX_NEIGHBORS, MAX_BAND = 64, 64, 16384
ST_INDEX_OOB = 1
NEG_INF = np.float32(-np.inf)
F0 = np.float32(0.0)
NAN_OUT = 0x7FFFFFFF


def csr(rows, weights=None):
    """(ptr int64, entries int64, weights fp32 or None) of a list of lists (and a list of weight lists)."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    flat = np.asarray([int(v) for x in rows for v in x], dtype=np.int64).reshape(-1)
    w = None if weights is None else np.asarray([v for x in weights for v in x], dtype=np.float32).reshape(-1)
    assert w is None or w.size == flat.size
    return ptr, flat, w


def accumulate(index, value, kn, lists, rows, weighted, fused=False, entry_order=None, weight_last=False):
    """(per query None -- a list number outside the CSR -- or (scores {j: float32}, votes {j: int}, the basket's valid
    items as a set), status).  ``index`` / ``value``: [n_items, stride >= kn]; places at or past kn are never read."""
    ptr, items, weights = lists
    n_items, n_lists = index.shape[0], len(ptr) - 1
    n = n_lists if rows is None else len(rows)
    out, status = [], 0
    for r in range(n):
        l = r if rows is None else int(rows[r])
        if not 0 <= l < n_lists:
            status |= ST_INDEX_OOB
            out.append(None)
            continue
        acc, votes, listed = {}, {}, set()
        order = list(range(int(ptr[l]), int(ptr[l + 1])))
        if entry_order is not None:
            order = entry_order(order, items)
        for t in order:
            i = int(items[t])
            if not 0 <= i < n_items:
                status |= ST_INDEX_OOB
                continue
            listed.add(i)
            for p in range(kn):
                j = int(index[i, p])
                if j == -1:
                    continue
                if not 0 <= j < n_items:
                    status |= ST_INDEX_OOB
                    continue
                v, a = np.float32(value[i, p]), acc.get(j, F0)
                with np.errstate(all="ignore"):
                    if not weighted or weight_last:
                        a = np.float32(a + v)
                    elif fused:
                        a = np.float32(chain.fma32(np.float32(weights[t]), v, a))
                    else:
                        a = np.float32(a + np.float32(np.float32(weights[t]) * v))
                acc[j] = a
                votes[j] = votes.get(j, 0) + 1
        if weighted and weight_last:                          # a mutant: one weight for the whole sum, the basket's first
            with np.errstate(all="ignore"):
                acc = {j: np.float32(np.float32(weights[order[0]]) * a) for j, a in acc.items()}
        out.append((acc, votes, listed))
    return out, status


def as_written(values):
    """fp32 values as write_candidate writes them: every NaN 0x7FFFFFFF, -0 as +0."""
    v = np.asarray(values, dtype=np.float32)
    bits = ts.bits_of(v).copy()
    bits[np.isnan(v)] = NAN_OUT
    bits[bits == 0x80000000] = 0
    return bits.view(np.float32).reshape(v.shape)


def select(scored, n_items, item_ok, exclude_basket, min_votes, k):
    """(index int64 [n, k], value fp32 [n, k], votes int32 [n, k]) from ``accumulate``'s rows."""
    n = len(scored)
    index = np.full((n, k), -1, dtype=np.int64)
    value = np.full((n, k), NEG_INF, dtype=np.float32)
    count = np.zeros((n, k), dtype=np.int32)
    for r, row in enumerate(scored):
        if row is None:
            continue
        acc, votes, listed = row
        cols = [j for j in sorted(acc) if votes[j] >= max(min_votes, 1) and (item_ok is None or int(item_ok[j]) != 0)
                and not (exclude_basket and j in listed)]
        m = min(k, len(cols))
        if m == 0:
            continue
        idx, val = ts.topk_ref(np.asarray([acc[j] for j in cols], dtype=np.float32), m)
        index[r, :m] = np.asarray(cols, dtype=np.int64)[idx]
        value[r, :m] = as_written(val)
        count[r, :m] = [votes[cols[i]] for i in idx]
    return index, value, count


def knn_reference(index, value, kn, lists, rows, item_ok, exclude_basket, min_votes, k, weighted=None):
    """(index, value, votes, status) of one call; ``weighted`` None = iff the lists carry weights."""
    weighted = lists[2] is not None if weighted is None else weighted
    scored, status = accumulate(index, value, kn, lists, rows, weighted)
    return select(scored, index.shape[0], item_ok, exclude_basket, min_votes, k) + (status,)


def largest_votes(scored):
    return max([max(row[1].values(), default=0) for row in scored if row is not None], default=0)


# ----------------------------------------------------------------------------------------
# neighbour tables: (index int64 [n_items, stride], value fp32 [n_items, stride], kn).  What lies at or past kn is poison:
# indices outside the catalogue and NaN values, so that a read of it raises the status word or changes bits
# ----------------------------------------------------------------------------------------
def poisoned(index, value, stride):
    n_items, kn = index.shape
    wide_i = np.empty((n_items, stride), dtype=np.int64)
    wide_v = np.full((n_items, stride), np.nan, dtype=np.float32)
    wide_i[:] = np.resize(np.asarray([n_items, -5, 2 ** 40 + 1], dtype=np.int64), stride)
    wide_i[:, :kn], wide_v[:, :kn] = index, value
    return wide_i, wide_v, kn


def random_table(n_items, kn, stride, seed, integer=False, fill=0.7):
    """Per row up to kn distinct neighbours (never the item itself) in random order, the other places -1; values random in
    (0, 1], or small integers, in which almost every score ties."""
    rng = np.random.default_rng(3000 + seed)
    index = np.full((n_items, kn), -1, dtype=np.int64)
    value = np.zeros((n_items, kn), dtype=np.float32)
    for i in range(n_items):
        others = np.setdiff1d(np.arange(n_items), [i])
        m = min(len(others), int(rng.integers(0, kn + 1)) if rng.random() > fill else kn)
        places = rng.permutation(kn)[:m]
        index[i, places] = rng.permutation(others)[:m]
        value[i, places] = rng.integers(1, 3, m) if integer else 1.0 - rng.random(m, dtype=np.float32)
    return poisoned(index, value, stride)


def border_table():
    """200 items, kn 64, integer values: every row's neighbours lie on both sides of the edges of bands of 64 and of 128
    (60 .. 67, 124 .. 131, 188 .. 195) plus random others, so that equal scores straddle every band border."""
    rng = np.random.default_rng(3100)
    n_items, kn = 200, 64
    index = np.full((n_items, kn), -1, dtype=np.int64)
    value = np.zeros((n_items, kn), dtype=np.float32)
    edge = np.concatenate([np.arange(60, 68), np.arange(124, 132), np.arange(188, 196)])
    for i in range(n_items):
        rest = np.setdiff1d(np.arange(n_items), np.concatenate([edge, [i]]))
        row = np.concatenate([edge[edge != i], rng.permutation(rest)[:30]])
        row = rng.permutation(row)
        index[i, :row.size] = row
        value[i, :row.size] = np.where(np.isin(row, edge), 2.0, rng.integers(1, 3, row.size))
    return poisoned(index, value, 64 + 3)


def special_table():
    """70 items, kn 7: NaN, both infinities, the smallest subnormal, -0 and a large value among ordinary ones; row 9 all -1."""
    idx, val, kn = random_table(70, 7, 9, seed=5, fill=1.0)
    words = ts.from_bits([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x80000000, 0x7F7FFFFF])
    rng = np.random.default_rng(3200)
    for i in range(0, 70, 2):
        val[i, int(rng.integers(0, kn))] = words[(i // 2) % len(words)]
    idx[9, :kn] = -1
    return idx, val, kn


def bad_index_table():
    """65 items, kn 7: neighbour indices outside the catalogue in valid places (65, -2, 2^40 + 3, whose low bits name an
    item) and an all -1 row."""
    idx, val, kn = random_table(65, 7, 8, seed=6, fill=1.0)
    idx[3, 1], idx[3, 4], idx[10, 0], idx[64, 6] = 65, -2, 2 ** 40 + 3, 2 ** 31
    idx[20, :kn] = -1
    return idx, val, kn


def order_table():
    """8 items, kn 2.  Items 0, 1, 2 vote for item 3 with 2^24, 1, 1; items 4 and 5 vote for item 6 with -(1 + 2^-11) and
    1 + 2^-12 (and item 5 for item 7 with 1)."""
    index = np.full((8, 2), -1, dtype=np.int64)
    value = np.zeros((8, 2), dtype=np.float32)
    for i, v in ((0, 2.0 ** 24), (1, 1.0), (2, 1.0)):
        index[i, 0], value[i, 0] = 3, v
    index[4, 0], value[4, 0] = 6, -(1.0 + 2.0 ** -11)
    index[5, 0], value[5, 0] = 6, 1.0 + 2.0 ** -12
    index[5, 1], value[5, 1] = 7, 1.0
    return poisoned(index, value, 3)


ORDER_BASKETS = [[0, 1, 2], [1, 2, 0], [4, 5]]
ORDER_WEIGHTS = [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0 + 2.0 ** -12]]

TABLES = {"random 200": lambda: random_table(200, 64, 64 + 5, seed=1), "kn 1": lambda: random_table(130, 1, 2, seed=2, fill=1.0),
          "kn 7": lambda: random_table(129, 7, 11, seed=3), "kn 64 of 65": lambda: random_table(65, 64, 80, seed=4, fill=1.0),
          "integer 200": lambda: random_table(200, 20, 24, seed=7, integer=True), "borders": border_table,
          "specials": special_table, "bad indices": bad_index_table, "order": order_table,
          "one item": lambda: poisoned(np.full((1, 3), -1, dtype=np.int64), np.zeros((1, 3), dtype=np.float32), 4)}
_built = {}


def table(name):
    """The table, built once and shared by every test that asks for it; nobody writes to it."""
    if name not in _built:
        _built[name] = TABLES[name]()
    return _built[name]


def item_mask(kind, n_items):
    """None | uint8 [n_items]: "none", "zero" (nothing allowed), "some" (two thirds allowed, any non-zero byte allows)."""
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(n_items, dtype=np.uint8)
    assert kind == "some"
    return ((np.arange(n_items) % 3 != 1) * (1 + np.arange(n_items) % 255)).astype(np.uint8)


def random_baskets(n_items, lengths, seed):
    """(item lists, weight lists): items with repeats; weights the reference's 0.01 / 0.1 / 1.0 and a few inexact ones."""
    rng = np.random.default_rng(3300 + seed)
    kinds = np.asarray([0.01, 0.1, 1.0, 1.1, 0.3, 2.5], dtype=np.float32)
    items = [rng.integers(0, n_items, n).tolist() for n in lengths]
    return items, [kinds[rng.integers(0, len(kinds), n)].tolist() for n in lengths]


# ----------------------------------------------------------------------------------------
# the table the device tests walk.  A case runs every (k, band, weights or not, exclude_basket, min_votes); the scores are
# worked out once per case and weighting
# ----------------------------------------------------------------------------------------
KS = (1, 5, 64)
BANDS = (64, 128, 0)


def _c(name, why, table_name, baskets, weights, rows=None, ok="none", min_votes=(1,)):
    assert len(baskets) == len(weights) and all(len(b) == len(w) for b, w in zip(baskets, weights))
    return dict(name=name, why=why, table=table_name, baskets=baskets, weights=weights,
                rows=None if rows is None else np.asarray(rows, dtype=np.int64), ok=ok, min_votes=tuple(min_votes))


def _build_cases():
    long_items, long_weights = random_baskets(200, (63, 64, 65, 127, 128, 129, 200), 1)
    some_items, some_weights = random_baskets(129, (0, 1, 2, 9, 30), 2)
    tie_items, tie_weights = random_baskets(200, (1, 2, 3, 5, 8, 70), 3)
    tie_weights = [[1.0] * len(w) for w in tie_weights]                          # the ties survive the weights
    border_items = [[0], [61, 125], [0, 100, 150], [10, 20, 30, 40, 190]]
    sp_items, sp_weights = random_baskets(70, (1, 4, 9, 20, 66), 4)
    sp_weights[1][0], sp_weights[2][3], sp_weights[3][5] = float("nan"), float("inf"), -0.0
    sp_weights[3][6], sp_weights[4][0], sp_weights[4][1] = float(ts.from_bits([1])[0]), float("-inf"), 0.0
    sp_items[2] += [9]                                                           # the all -1 row
    sp_weights[2] += [1.0]
    bad_items = [[3, 10, 64], [1, 65, 2, -1, 2 ** 40 + 2, 3], [20], [5, 6]]
    hub = list(range(65)) * 2
    return (
        _c("empty baskets", "a basket without entries, between others, gives -1 / -inf / 0", "kn 7", [[], [4], [], [7, 8]],
           [[], [1.0], [], [0.5, 2.0]]),
        _c("one entry", "the neighbour row itself comes back", "random 200", [[0], [199], [64]], [[1.0], [0.1], [1.1]]),
        _c("a row of empty places", "an entry whose row is all -1 votes for nothing but is still excluded", "bad indices",
           [[20], [20, 21], [21, 20, 20]], [[1.0], [1.0, 0.5], [0.3, 1.0, 1.0]]),
        _c("a repeated entry", "contributes each time it occurs", "kn 7", [[4, 4, 9, 4], [9, 4, 4, 4], [4]],
           [[1.0, 0.1, 1.1, 0.3], [1.1, 0.3, 0.1, 1.0], [1.0]], min_votes=(1, 2, 3)),
        _c("long baskets", "63 .. 65, 127 .. 129 and 200 entries: both sides of a wavefront's reads of the list", "random 200",
           long_items, long_weights, min_votes=(1, 2, "max+1")),
        _c("kn 1", "one place a row, the padding beside it poisoned", "kn 1", [[0, 1, 2, 129], [5] * 3, list(range(130))],
           [[1.0] * 4, [0.1] * 3, [1.1] * 130]),
        _c("kn 7", "a narrow table with a wide stride, some baskets", "kn 7", some_items, some_weights, ok="some"),
        _c("kn 64", "the widest table, every place filled, a catalogue of one item more than a band", "kn 64 of 65",
           [[0], [64, 0], hub], [[1.0], [0.1, 1.1], [0.3] * len(hub)], min_votes=(1, 2, "max+1")),
        _c("integer ties", "small integers: almost every score ties and the index decides", "integer 200", tie_items, tie_weights,
           min_votes=(1, 2)),
        _c("ties across the bands", "equal scores on both sides of every edge of bands of 64 and 128", "borders", border_items,
           [[1.0] * len(b) for b in border_items]),
        _c("nothing allowed", "item_ok all zero", "kn 7", [[4, 5, 6]], [[1.0, 1.0, 1.0]], ok="zero"),
        _c("lists by number", "rows name the baskets, repeated and out of order; the other baskets are not read", "random 200",
           long_items[:4], long_weights[:4], rows=[3, 0, 3, 1]),
        _c("special values", "NaN, both infinities, subnormals and -0 among values and weights", "specials", sp_items, sp_weights,
           min_votes=(1, 2)),
        _c("bad list numbers", "a list number outside the CSR: flagged, -1 / -inf / 0, the others untouched", "kn 7", some_items,
           some_weights, rows=[1, -1, 4, 5, 2 ** 40, 3]),
        _c("bad entries and indices", "basket entries and neighbour indices outside the catalogue are skipped and flagged",
           "bad indices", bad_items, [[1.0] * len(b) for b in bad_items], ok="some"),
        _c("sum order and fusing", "the two hand-worked order cases", "order", ORDER_BASKETS, ORDER_WEIGHTS),
        _c("one item", "a catalogue of one item whose row is empty", "one item", [[0], []], [[1.0], []]),
    )


CASES = _build_cases()
CASE_NAMES = [c["name"] for c in CASES]
