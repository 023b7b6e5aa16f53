"""Reference and case table for the cross-table retrieval tests (lgc_retrieve_topk).

The reference works on a score PANEL in plain numpy: where the scores come from (integers here, lgc_score_rows on the
device) is the caller's business.  Eligibility is decided in Python integers, the ranking is ``topk_support.topk_ref`` --
the order of lgc_mask_topk -- over the eligible columns."""
import numpy as np

import similar_support as ss
import topk_support as ts

ROW_TILE, CAND_TILE = ss.ROW_TILE, ss.ITEM_TILE      # 64 queries x 128 candidates of one tile
CHUNK, GROUP = 32, 16                                # columns of one staged chunk, of one MFMA group
MAX_K, MAX_SLICES = 64, 1024
ST_INDEX_OOB = 1
NEG_INF = np.float32(-np.inf)


def buffer_cap(k):
    """Candidates a row's LDS buffer holds before it is compacted (select_cap of csrc/lgconv_select.h)."""
    return 64 if k <= 32 else 96


def retrieve_reference(panel, cand_ok, lists, list_rows, skip, k, query_ids=None, n_query_rows=None):
    """(index int64 [n, k], value fp32 [n, k], status): per row of ``panel`` (fp32 [n, n_cand], row r = the scores of query
    r) the k best eligible columns.  Column c is eligible for row r unless ``cand_ok[c] == 0``, ``skip[r] == c`` or c is an
    entry of the row's list; ``lists`` = (ptr, items) or None, the row's list is number ``list_rows[r]`` (None: the
    query's id, ``query_ids[r]``, None: r), -1 = no list.  A query id outside [0, n_query_rows) (where given) or a list
    number outside the lists voids the row (-1 / -inf) and sets ST_INDEX_OOB.  Short rows end in -1 / -inf."""
    panel = np.asarray(panel, dtype=np.float32)
    n, n_cand = panel.shape
    index = np.full((n, k), -1, dtype=np.int64)
    value = np.full((n, k), NEG_INF, dtype=np.float32)
    status = 0
    for r in range(n):
        qid = r if query_ids is None else int(query_ids[r])
        if n_query_rows is not None and not 0 <= qid < n_query_rows:
            status |= ST_INDEX_OOB
            continue
        out = set()
        if lists is not None:
            ptr, items = lists
            which = qid if list_rows is None else int(list_rows[r])
            if which != -1:
                if not 0 <= which < len(ptr) - 1:
                    status |= ST_INDEX_OOB
                    continue
                out = {int(i) for i in items[int(ptr[which]):int(ptr[which + 1])]}
        cols = [c for c in range(n_cand)
                if (cand_ok is None or int(cand_ok[c]) != 0) and (skip is None or int(skip[r]) != c) and c not in out]
        m = min(k, len(cols))
        if m == 0:
            continue
        cols = np.asarray(cols, dtype=np.int64)
        idx, val = ts.topk_ref(panel[r, cols], m)
        index[r, :m], value[r, :m] = cols[idx], val
    return index, value, status


def canonical_bits(values):
    """uint32 bits of fp32 values as the kernel returns them: -0 as +0, every NaN as 0x7FFFFFFF."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(values, dtype=np.float32) + np.float32(0.0)
    return np.where(np.isnan(v), np.uint32(0x7FFFFFFF), ts.bits_of(v).reshape(v.shape))


def csr(rows):
    """(ptr, items) int64 of a list of lists."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    items = np.concatenate([np.asarray(x, dtype=np.int64) for x in rows]) if rows else np.zeros(0, dtype=np.int64)
    return ptr, items.astype(np.int64)


def random_lists(rng, n_lists, n_cand, share=0.1):
    """Ascending distinct lists, about ``share`` of the candidates each; every fourth list is empty."""
    rows = []
    for i in range(n_lists):
        take = 0 if i % 4 == 3 else max(1, int(share * n_cand))
        rows.append(np.sort(rng.permutation(n_cand)[:min(take, n_cand)]))
    return csr(rows)


# ----------------------------------------------------------------------------------------
# the table the device tests walk: name, n_queries, n_query_rows, n_cand, dim, k, slice counts, flavour
#   flavour: table "random" | "integer"; shared: one table on both sides (n_query_rows = n_cand); ids "none" | "permuted" |
#   "repeated"; scaled; ok: share of candidates allowed (None = no mask); lists; skip
# ----------------------------------------------------------------------------------------
def _c(name, n_queries, n_query_rows, n_cand, dim, k, slices, **flavour):
    f = dict(table="random", shared=False, ids="permuted", scaled=False, ok=None, lists=False, skip=False)
    f.update(flavour)
    if f["shared"]:
        assert n_query_rows == n_cand
    return (name, n_queries, n_query_rows, n_cand, dim, k, tuple(slices), f)


CASES = (
    _c("one query, one candidate", 1, 1, 1, 1, 1, (0, 1, 1024), ids="none"),
    _c("below the tiles", 63, 70, 127, 15, 32, (0, 1, 2), lists=True, ok=0.8),
    _c("the tiles exactly", 64, 64, 128, 16, 33, (0, 1, 3), ids="none", skip=True),
    _c("above the tiles", 65, 80, 129, 17, 64, (0, 1, 2, 3), lists=True, scaled=True),
    _c("chunk below", 1, 9, 300, 31, 1, (0, 2, 3, 1024), ok=0.5),
    _c("chunk exactly", 130, 200, 300, 32, 32, (0, 1, 3), ids="repeated", lists=True, skip=True),
    _c("chunk above", 65, 65, 1000, 33, 33, (0, 1, 2, 1024), ids="none", lists=True, ok=0.9),
    _c("width 64", 130, 150, 1000, 64, 64, (0, 3), scaled=True, lists=True, ok=0.9, skip=True),
    _c("width 90", 63, 100, 300, 90, 20, (0, 2), lists=True, ok=0.9),
    _c("width 256, wide buffers", 65, 65, 300, 256, 64, (0, 1, 3), ids="none", lists=True),
    _c("one table", 64, 300, 300, 24, 33, (0, 1, 3), shared=True, scaled=True, skip=True, lists=True),
    _c("integer ties", 130, 130, 1000, 4, 64, (0, 1, 2, 3, 1024), table="integer", ids="none", lists=True, ok=0.7),
    _c("k above the eligible count", 5, 8, 129, 8, 64, (0, 1, 2), ok=0.2, lists=True),
)
CASE_NAMES = [c[0] for c in CASES]


def build_case(case, seed=0):
    """The numpy arrays of a case: dict(queries, cands, query_ids, query_scale, cand_scale, cand_ok, lists, list_rows,
    skip).  With ``shared`` queries is cands.  Lists are per query-table row (list_rows None) unless the case repeats ids,
    where list_rows redirects."""
    name, n_queries, n_query_rows, n_cand, dim, k, slices, f = case
    rng = np.random.default_rng(CASE_NAMES.index(name) * 101 + seed)
    make = ss.integer_table if f["table"] == "integer" else ss.random_table
    cands = make(rng, n_cand, dim)
    queries = cands if f["shared"] else make(rng, n_query_rows, dim)
    ids = None
    if f["ids"] == "permuted":
        ids = rng.permutation(n_query_rows)[:n_queries].astype(np.int64) if n_queries <= n_query_rows else \
            rng.integers(0, n_query_rows, n_queries).astype(np.int64)
    elif f["ids"] == "repeated":
        ids = rng.integers(0, n_query_rows, n_queries).astype(np.int64)
        ids[-1] = ids[0]
    else:
        assert n_queries == n_query_rows
    out = dict(queries=queries, cands=cands, query_ids=ids, query_scale=None, cand_scale=None, cand_ok=None, lists=None,
               list_rows=None, skip=None)
    if f["scaled"]:
        out["cand_scale"] = rng.uniform(0.5, 2.0, n_cand).astype(np.float32)
        out["query_scale"] = out["cand_scale"] if f["shared"] else rng.uniform(0.5, 2.0, n_query_rows).astype(np.float32)
    if f["ok"] is not None:
        out["cand_ok"] = (rng.random(n_cand) < f["ok"]).astype(np.uint8) * rng.integers(1, 256, n_cand).astype(np.uint8)
    if f["lists"]:
        if f["ids"] == "repeated":                           # fewer lists than rows, named per query; some queries have none
            out["lists"] = random_lists(rng, 7, n_cand)
            out["list_rows"] = rng.integers(-1, 7, n_queries).astype(np.int64)
        else:
            out["lists"] = random_lists(rng, n_query_rows, n_cand)
    if f["skip"]:
        who = np.arange(n_queries) if ids is None else ids
        out["skip"] = np.where(rng.random(n_queries) < 0.8, who % n_cand, -1).astype(np.int64)
    return out
