"""Reference and case builders for the re-ranking tests (lgc_rerank_mmr, lgc_list_diversity).  numpy only; of the project
nothing but ``topk_support`` (the order) and ``similar_support`` (its tables) is imported.

``mmr_ref`` restates the arithmetic contract of include/lgconv_hip.h in fp32: every product and every subtraction is one
numpy float32 operation, rounded once, nothing fused.  Where the similarities come from -- exact integers here,
lgc_score_rows' bits on the device -- is the caller's business: it hands in ``sim_of``."""
import numpy as np

import similar_support as ss
import topk_support as ts

MAX_CAND = 256
LDS_PER_WAVE = 36 * 1024     # bytes of staged candidate rows one wavefront may hold (kRrLdsPerWave)
NEG_INF = np.float32(-np.inf)


def row_stride(dim):
    """Floats between two staged rows: the width rounded up to 4, in 16-byte groups an odd number."""
    return 4 * (((dim + 3) // 4) | 1)


def route(n_cand, dim):
    """"lds" or "global": the rule of lgc_rerank_route, restated."""
    return "lds" if n_cand * row_stride(dim) * 4 <= LDS_PER_WAVE else "global"


def valid_positions(cand, n_items=None):
    cand = np.asarray(cand, dtype=np.int64)
    return (cand >= 0) if n_items is None else (cand >= 0) & (cand < n_items)


def mmr_ref(rel, cand, sim_of, k, lam, n_items=None):
    """(index int64 [k], pos int32 [k], value fp32 [k]) for ONE row: ``rel`` fp32 [N], ``cand`` int64 [N] (-1 = empty; with
    ``n_items`` any id outside [0, n_items) is skipped too), ``sim_of(ps, c)`` = fp32 similarities of the positions ``ps``
    (an int array) to the position ``c`` just chosen.  The choice: the largest ``topk_support.order_keys`` key, then the
    lowest position."""
    rel, cand = np.asarray(rel, dtype=np.float32), np.asarray(cand, dtype=np.int64)
    n = cand.size
    assert rel.shape == (n,) and 1 <= k <= n
    lam32 = np.float32(lam)
    oml = np.float32(1.0) - lam32
    is_open = valid_positions(cand, n_items)
    index, pos = np.full(k, -1, dtype=np.int64), np.full(k, -1, dtype=np.int32)
    value = np.full(k, NEG_INF, dtype=np.float32)
    with np.errstate(all="ignore"):
        lrel = (lam32 * rel).astype(np.float32)
        pen = np.zeros(n, dtype=np.float32)
        for t in range(k):
            ps = np.flatnonzero(is_open)
            if ps.size == 0:
                break
            obj = lrel[ps] if t == 0 else (lrel[ps] - (oml * pen[ps]).astype(np.float32)).astype(np.float32)
            keys = ts.order_keys(obj)
            c = int(ps[np.flatnonzero(keys == keys.max())[0]])              # ps ascends: the first is the lowest position
            index[t], pos[t], value[t] = cand[c], c, obj[np.flatnonzero(ps == c)[0]]
            is_open[c] = False
            ps = np.flatnonzero(is_open)
            if ps.size == 0 or t + 1 == k:
                continue
            s = np.asarray(sim_of(ps, c), dtype=np.float32)
            pen[ps] = s if t == 0 else np.where((s != s) | (s > pen[ps]), s, pen[ps])
    return index, pos, value


def mmr_ref_rows(rel, cand, sims, k, lam, n_items=None):
    """The same for every row; ``sims(r)`` gives row r's ``sim_of``."""
    out = [mmr_ref(rel[r], cand[r], sims(r), k, lam, n_items) for r in range(cand.shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def ild_ref(sim, valid, cutoffs):
    """float64 [len(cutoffs)] for ONE list: ``sim`` [k, k], sim[a, b] for a < b the fp32 similarity of positions a and b
    (a the earlier one), ``valid`` bool [k].  t_b = the sum over valid a < b of 1 - sim[a, b], ascending a, 0 for an invalid
    b; the prefix over ascending b; at cutoff c divided by the number of pairs among the valid first c."""
    valid = np.asarray(valid, dtype=bool)
    out, total, count = [], np.float64(0.0), 0
    cuts = list(cutoffs)
    with np.errstate(all="ignore"):
        for b in range(cuts[-1]):
            t = np.float64(0.0)
            if valid[b]:
                for a in range(b):
                    if valid[a]:
                        t = t + (np.float64(1.0) - np.float64(np.float32(sim[a, b])))
                count += 1
            total = total + t
            if b + 1 in cuts:
                out.append(total / np.float64(count * (count - 1) // 2) if count >= 2 else np.float64(np.nan))
    return np.array(out, dtype=np.float64)


def same_doubles(got, want):
    """Bit-equal float64, any NaN matching any NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((np.isnan(got) & np.isnan(want)) | (got.view(np.uint64) == want.view(np.uint64))))


def exact_sims(table, cand_row, scale=None):
    """``sim_of`` of a row over a table of small integers, where the chain is exact (``similar_support.dot_chain32``)."""
    dots = ss.dot_chain32(table, table)
    if scale is not None:
        sc = np.asarray(scale, dtype=np.float32)
        dots = ((dots * sc[:, None]).astype(np.float32) * sc[None, :]).astype(np.float32)
    cand_row = np.asarray(cand_row, dtype=np.int64)
    return lambda ps, c: dots[cand_row[ps], cand_row[c]]


# ----------------------------------------------------------------------------------------
# case builders
# ----------------------------------------------------------------------------------------
def candidates(rng, n_rows, n_cand, n_items, kind="distinct"):
    """int64 [n_rows, n_cand]: "distinct" ids where the table has that many (repeats otherwise), "repeated" draws with
    repeats, "short" the same with about a third of the places -1, among them whole runs at the end."""
    if kind == "distinct" and n_cand <= n_items:
        return np.stack([rng.permutation(n_items)[:n_cand] for _ in range(n_rows)]).astype(np.int64)
    cand = rng.integers(0, n_items, size=(n_rows, n_cand)).astype(np.int64)
    if n_cand >= 2:
        cand[:, -1] = cand[:, 0]                                             # at least one repeat
    if kind == "short":
        cand[rng.random(cand.shape) < 0.3] = -1
        for r in range(n_rows):
            cand[r, n_cand - rng.integers(0, n_cand + 1):] = -1              # row 0 .. all of the row empty
    return cand


def descending_rel(rng, n_rows, n_cand):
    """fp32 [n_rows, n_cand]: relevances as a top-k row carries them, descending with ties."""
    rel = np.sort(rng.integers(0, 12, size=(n_rows, n_cand)).astype(np.float32) * np.float32(0.125), axis=1)[:, ::-1]
    return np.ascontiguousarray(rel)


GPU_SHAPES = [(n_cand, dim) for dim in (1, 3, 4, 63, 64, 65, 90, 256) for n_cand in (1, 2, 63, 64, 65, 100, 255, 256)]


def ks_of(n_cand):
    return sorted({1, min(2, n_cand), min(20, n_cand), n_cand})


def grouped_table(rng, n_groups, per_group, dim):
    """fp32 [n_groups * per_group, dim]: every group is one random row repeated -- "twenty shades of one lipstick"."""
    base = ss.random_table(rng, n_groups, dim)
    return np.repeat(base, per_group, axis=0)
