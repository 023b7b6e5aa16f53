"""Reference and case builders for the similar-items tests (lgc_row_rnorm, lgc_item_neighbors).

The reference ranks with ``topk_support.topk_ref`` -- the order of lgc_mask_topk -- over the candidate columns of a row of
scores; where the scores come from (numpy here, lgc_score_rows on the device) is the caller's business."""
import numpy as np

import topk_support as ts

ROW_TILE = 64        # query rows of one workgroup (kTileBM of csrc/lgconv_tile.h)
ITEM_TILE = 128      # items of one tile (kTileBN)
MAX_K = 64
NEG_INF = np.float32(-np.inf)


def neighbors_ref(scores, query_ids, k, item_ok=None, exclude_self=True):
    """(index int64 [n, k], value fp32 [n, k]): per row of ``scores`` (fp32 [n, n_items], row r = the scores of query
    ``query_ids[r]``) the k best candidates.  Candidates: every column with ``item_ok != 0``, without the query's own
    column when ``exclude_self``.  Excluded columns are deleted, the rest ranked by ``topk_ref`` and the places mapped
    back; a row with fewer than k candidates ends in -1 / -inf, a query outside [0, n_items) is all -1 / -inf."""
    scores = np.asarray(scores, dtype=np.float32)
    n, n_items = scores.shape
    ids = np.arange(n_items, dtype=np.int64) if query_ids is None else np.asarray(query_ids, dtype=np.int64)
    assert ids.shape == (n,)
    ok = np.ones(n_items, dtype=bool) if item_ok is None else np.asarray(item_ok) != 0
    index = np.full((n, k), -1, dtype=np.int64)
    value = np.full((n, k), NEG_INF, dtype=np.float32)
    for r in range(n):
        q = int(ids[r])
        if q < 0 or q >= n_items:
            continue
        keep = ok.copy()
        if exclude_self:
            keep[q] = False
        cols = np.flatnonzero(keep)
        m = min(k, cols.size)
        if m == 0:
            continue
        idx, val = ts.topk_ref(scores[r, cols], m)
        index[r, :m], value[r, :m] = cols[idx], val
    return index, value


def dot_chain32(a, b):
    """fp32 [len(a), len(b)]: the chain of fused multiply-adds over ascending d from +0, evaluated exactly in float64 where
    that is exact -- small integers only (every partial sum is an integer below 2^24)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = a @ b.T
    assert np.all(out == np.rint(out)) and np.abs(a).max(initial=0) * np.abs(b).max(initial=0) * a.shape[1] < 2 ** 24
    return out.astype(np.float32)


def rnorm_ref(table):
    """float64 [n_rows]: 1 / sqrt(sum of squares), a zero row -> 0 (lgc_row_rnorm's rule), NaN stays NaN."""
    x = np.asarray(table, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 1.0 / np.sqrt((x * x).sum(axis=1))
    return np.where(np.isinf(out), 0.0, out)


def rnorm_bound(dim):
    """Relative bound of lgc_row_rnorm against ``rnorm_ref``: the fp32 sum of non-negative terms is within dim * u, the
    square root halves that and adds u, the division adds u; u = 2^-24 -- (dim / 2 + 3) u with one u to spare."""
    return (dim / 2 + 3) * 2.0 ** -24


def same_values(got, want):
    """Bit-equal after x + 0 (-0 and +0 are one value of the order), any NaN matching any NaN."""
    with np.errstate(invalid="ignore"):
        g = np.asarray(got, dtype=np.float32) + np.float32(0.0)
        w = np.asarray(want, dtype=np.float32) + np.float32(0.0)
    return ts.values_match(g, w)


# ----------------------------------------------------------------------------------------
# case builders
# ----------------------------------------------------------------------------------------
def random_table(rng, n_items, dim):
    return rng.standard_normal((n_items, dim)).astype(np.float32)


def integer_table(rng, n_items, dim, hi=1):
    """Entries in {-hi .. hi}: many duplicate rows, scores that are small integers and tie in long runs."""
    return rng.integers(-hi, hi + 1, size=(n_items, dim)).astype(np.float32)


def subnormal_table(rng, n_items, dim):
    """Rows of ordinary size next to rows near 1e-20 and 1e-25: their products are subnormal or underflow."""
    t = random_table(rng, n_items, dim)
    scale = np.float32(10.0) ** rng.choice(np.array([0, 0, -20, -25], dtype=np.float32), size=n_items)
    t = (t * scale[:, None].astype(np.float32)).astype(np.float32)
    t[rng.integers(0, n_items)] = ts.from_bits([1] * dim)                 # the smallest subnormal itself
    return t


def special_table(rng, n_items, dim):
    """NaN rows of both sign bits, +inf and -inf entries, all-zero rows, rows of -0."""
    assert n_items >= 12
    t = random_table(rng, n_items, dim)
    rows = rng.permutation(n_items)[:10]
    t[rows[0]] = ts.from_bits([0x7FC00000] * dim)
    t[rows[1]] = ts.from_bits([0xFFC00000] * dim)
    t[rows[2], 0] = ts.from_bits([0xFF800001])[0]
    t[rows[3], dim - 1] = np.inf
    t[rows[4], 0] = -np.inf
    t[rows[5]] = 0.0
    t[rows[6]] = 0.0
    t[rows[7]] = -0.0
    t[rows[8]] = np.abs(t[rows[8]])
    t[rows[8], 0] = np.inf
    t[rows[9]] = -np.abs(t[rows[9]])
    return t, rows


def queries(rng, kind, n_queries, n_items):
    """None ("all"), a permutation prefix without repeats where it fits ("permuted"), or draws with repeats ("repeated")."""
    if kind == "all":
        return None
    if kind == "permuted" and n_queries <= n_items:
        return rng.permutation(n_items)[:n_queries].astype(np.int64)
    q = rng.integers(0, n_items, size=n_queries).astype(np.int64)
    if n_queries >= 2:
        q[-1] = q[0]                                                      # at least one repeat
    return q
