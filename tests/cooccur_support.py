"""Reference and case table for the bought-together tests (lgc_cooccur_topk).

The reference counts in Python integers from the two CSRs -- c(q, j) = the sum over the entries u of q's buyer list of the
number of entries of u's item list equal to j, entries outside their table skipped --, scores with numpy float32 SCALARS in
the order the header states (every operand is made a float32 first: a Python or numpy integer next to a float32 would
promote to float64), applies the eligibility rule and ranks with ``topk_support.topk_ref``, the order of lgc_mask_topk."""
import numpy as np

import topk_support as ts

MAX_K, MAX_BAND = 64, 32768
COUNT, COSINE, JACCARD = 0, 1, 2
MEASURES = {"count": COUNT, "cosine": COSINE, "jaccard": JACCARD}
ST_INDEX_OOB = 1
NEG_INF = np.float32(-np.inf)
F1 = np.float32(1.0)


def csr(rows):
    """(ptr, entries) int64 of a list of lists."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    flat = [int(v) for x in rows for v in x]
    return ptr, np.asarray(flat, dtype=np.int64).reshape(-1)


def rows_of(lists):
    ptr, entries = lists
    return [[int(v) for v in entries[int(ptr[i]):int(ptr[i + 1])]] for i in range(len(ptr) - 1)]


def score(c, a, b, measure):
    """The fp32 score of count c between buyer lists of a and b entries, or None where Jaccard's denominator is <= 0."""
    fc = np.float32(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == COUNT:
            return fc
        if measure == COSINE:
            ra = F1 / np.sqrt(np.float32(a))
            rb = F1 / np.sqrt(np.float32(b))
            return np.float32(np.float32(fc * ra) * rb)
        den = a + b - c
        if den <= 0:
            return None
        return np.float32(fc / np.float32(den))


def count_rows(buyers, seen, n_users, n_items, query_ids=None):
    """(per query a dict {item: count} or None for an id outside the catalogue, status): Python integers only."""
    bptr, busers = buyers
    sptr, sitems = seen
    n = n_items if query_ids is None else len(query_ids)
    out, status = [], 0
    for r in range(n):
        q = r if query_ids is None else int(query_ids[r])
        if not 0 <= q < n_items:
            status |= ST_INDEX_OOB
            out.append(None)
            continue
        row = {}
        for u in busers[int(bptr[q]):int(bptr[q + 1])]:
            u = int(u)
            if not 0 <= u < n_users:
                status |= ST_INDEX_OOB
                continue
            for j in sitems[int(sptr[u]):int(sptr[u + 1])]:
                j = int(j)
                if not 0 <= j < n_items:
                    status |= ST_INDEX_OOB
                    continue
                row[j] = row.get(j, 0) + 1
        out.append(row)
    return out, status


def select(counts, buyers, n_items, query_ids, item_ok, min_count, measure, k, score_fn=score):
    """(index int64 [n, k], value fp32 [n, k], count int32 [n, k]) from ``count_rows``' dicts."""
    bptr = buyers[0]
    n = len(counts)
    index = np.full((n, k), -1, dtype=np.int64)
    value = np.full((n, k), NEG_INF, dtype=np.float32)
    count = np.zeros((n, k), dtype=np.int32)
    for r, row in enumerate(counts):
        if not row:
            continue
        q = r if query_ids is None else int(query_ids[r])
        a = int(bptr[q + 1]) - int(bptr[q])
        cols, vals = [], []
        for j in sorted(row):
            c = row[j]
            if j == q or c < max(min_count, 1) or (item_ok is not None and int(item_ok[j]) == 0):
                continue
            s = score_fn(c, a, int(bptr[j + 1]) - int(bptr[j]), measure)
            if s is None:
                continue
            cols.append(j)
            vals.append(s)
        m = min(k, len(cols))
        if m == 0:
            continue
        idx, val = ts.topk_ref(np.asarray(vals, dtype=np.float32), m)
        index[r, :m] = np.asarray(cols, dtype=np.int64)[idx]
        value[r, :m] = val
        count[r, :m] = [row[cols[i]] for i in idx]
    return index, value, count


def cooccur_reference(buyers, seen, n_users, n_items, query_ids, item_ok, min_count, measure, k):
    """(index, value, count, status) of one call: ``buyers`` = (ptr, users), ``seen`` = (ptr, items), numpy int64."""
    counts, status = count_rows(buyers, seen, n_users, n_items, query_ids)
    return select(counts, buyers, n_items, query_ids, item_ok, min_count, measure, k) + (status,)


# ----------------------------------------------------------------------------------------
# graphs: dict(n_users, n_items, seen = (ptr, items), buyers = (ptr, users)), built once and shared
# ----------------------------------------------------------------------------------------
def graph_of(bought, n_items):
    """From per-user ascending item lists: both CSRs, the buyers' the exact transpose (a repeated entry twice there too)."""
    buyers = [[] for _ in range(n_items)]
    for u, items in enumerate(bought):
        for j in items:
            buyers[j].append(u)
    return dict(n_users=len(bought), n_items=n_items, seen=csr(bought), buyers=csr(buyers))


def build_lengths():
    """200 items, 1,025 users.  Item 0 is bought by every user; items 1 .. 7 have buyer lists of 0, 1, 63, 64, 65, 256 and
    257 entries besides; users 1000 .. 1002 have lists of 64, 65 and 2 entries that begin and end on band edges (0 | 127,
    0 | 128); users from 600 on bought item 0 alone; the rest is sparse and random."""
    rng = np.random.default_rng(2800)
    n_users, n_items = 1025, 200
    bought = [{0} for _ in range(n_users)]
    for item, length in ((2, 1), (3, 63), (4, 64), (5, 65), (6, 256), (7, 257)):
        for s in range(length):
            bought[40 * item + s].add(item)                  # users 80 .. 536
    for u in range(300):
        bought[u].update(int(j) for j in rng.integers(8, n_items, 3))
    bought[1000].update(range(65, 128))
    bought[1001].update(range(64, 128))
    bought[1002].add(128)
    return graph_of([sorted(b) for b in bought], n_items)


def build_random(n_items, n_users=40, per_user=6, seed=0):
    def build():
        rng = np.random.default_rng(2810 + n_items + seed)
        bought = [sorted(set(int(j) for j in rng.integers(0, n_items, per_user))) for _ in range(n_users)]
        return graph_of(bought, n_items)
    return build


def build_complete():
    """Every one of 5 users bought every one of 200 items: every count is 5, the answer is ascending indices."""
    return graph_of([list(range(200))] * 5, 200)


def build_band_ties():
    """200 items; for query item 0 the best candidate of each band of 64 -- items 10, 70, 130 and 195 -- has the same count 7
    and the same 7 buyers; items 11, 71 and 131 tie at 3 behind them."""
    bought = [[0, 10, 70, 130, 195] for _ in range(7)] + [[0, 11, 71, 131] for _ in range(3)] + [[0, 12], [5, 195 - 1]]
    return graph_of(bought, 200)


def build_out_of_range():
    """65 items, 20 users, ascending lists with entries outside their tables at both ends (negative ones first, those past
    the table last), in both CSRs, and user 3 with item 5 twice (its buyer list names user 3 twice)."""
    bought = rows_of(build_random(65, 20, 5, seed=7)()["seen"])
    bought[9] = list(range(0, 40, 2))                        # longer than one step of a group: the searched path
    bought[3] = sorted(set(bought[3]) | {5}) + [5]
    bought[3].sort()
    g = graph_of(bought, 65)
    bought, buyers = rows_of(g["seen"]), rows_of(g["buyers"])
    bought[0] = [-3] + bought[0] + [65, 2 ** 40]
    bought[7] = [-2 ** 40, -1] + bought[7]
    bought[9] = bought[9] + [70]
    some = next(j for j in range(65) if len(buyers[j]) > 1)
    buyers[some] = [-1] + buyers[some] + [20, 2 ** 40 + 1]
    return dict(n_users=20, n_items=65, seen=csr(bought), buyers=csr(buyers))


GRAPHS = {"lengths": build_lengths, "complete": build_complete, "band ties": build_band_ties,
          "out of range": build_out_of_range}
GRAPHS.update({f"random {n}": build_random(n) for n in (1, 2, 63, 64, 65, 128, 129)})
_built = {}


def graph(name):
    """The graph, built once and shared by every test that asks for it; nobody writes to it."""
    if name not in _built:
        _built[name] = GRAPHS[name]()
    return _built[name]


def query_ids(kind, n_items):
    """None | int64 ids: "none" = the whole catalogue, "descending", "repeated", "out of range" (three bad ids among good)."""
    if kind == "none":
        return None
    if kind == "descending":
        return np.arange(n_items - 1, -1, -1, dtype=np.int64)
    if kind == "repeated":
        return np.asarray([0, n_items - 1, 0, n_items // 2, 0, n_items - 1], dtype=np.int64)
    assert kind == "out of range"
    return np.asarray([0, n_items, n_items - 1, -1, 2 ** 40, n_items // 2], dtype=np.int64)


def item_mask(kind, n_items):
    """None | uint8 [n_items]: "none", "zero" (nothing allowed), "some" (two thirds allowed, any non-zero byte allows)."""
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(n_items, dtype=np.uint8)
    assert kind == "some"
    return ((np.arange(n_items) % 3 != 1) * (1 + np.arange(n_items) % 255)).astype(np.uint8)


# ----------------------------------------------------------------------------------------
# the table the device tests walk: name, graph, ks, bands, measures, min_counts ("max+1" = one above the largest count),
# ids kind, mask kind.  A case runs every (k, measure, min_count) at every band; the counts are worked out once per case.
# ----------------------------------------------------------------------------------------
ALL_BANDS = (64, 128, 192, 256, 0)
ALL_MEASURES = ("count", "cosine", "jaccard")


def _c(name, graph_name, ks, bands=ALL_BANDS, measures=ALL_MEASURES, min_counts=(1,), ids="none", ok="none"):
    return dict(name=name, graph=graph_name, ks=tuple(ks), bands=tuple(bands), measures=tuple(measures),
                min_counts=tuple(min_counts), ids=ids, ok=ok)


CASES = (
    _c("one item", "random 1", (1, 64), measures=("count",)),
    _c("two items", "random 2", (1, 33)),
    _c("below one band", "random 63", (32,), measures=("cosine",), ok="some"),
    _c("one band exactly", "random 64", (33,), measures=("jaccard",)),
    _c("a last band of one item", "random 65", (64,), measures=("count", "cosine"), min_counts=(1, 2)),
    _c("two bands exactly", "random 128", (1, 32), measures=("cosine",), ids="descending"),
    _c("a last band of one item again", "random 129", (33,), measures=("jaccard", "count"), ids="repeated"),
    _c("ids out of range", "random 129", (5,), bands=(64, 0), measures=("cosine",), ids="out of range"),
    _c("list lengths", "lengths", (20,), min_counts=(1,)),
    _c("list lengths, k 64", "lengths", (64,), bands=(64, 0), measures=("count",), min_counts=(2, "max+1"), ids="repeated"),
    _c("complete bipartite", "complete", (64,), ids="repeated"),
    _c("ties across the bands", "band ties", (1, 4, 7), measures=("count", "cosine"), ids="repeated"),
    _c("nothing allowed", "random 129", (8,), bands=(64, 0), measures=("count",), ok="zero"),
    _c("entries out of range", "out of range", (64,), bands=(64, 128, 0), min_counts=(1, 2)),
)
CASE_NAMES = [c["name"] for c in CASES]


def largest_count(counts, query_ids):
    """The largest c(q, j), j != q, over the rows of ``count_rows``."""
    best = 0
    for r, row in enumerate(counts):
        q = r if query_ids is None else int(query_ids[r])
        for j, c in (row or {}).items():
            if j != q:
                best = max(best, c)
    return best
