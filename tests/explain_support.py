"""References for the score-attribution tests (no product code here): an fp64 statement of

    contrib[k, t] = c_k <F[i_k], E[t]>,   base[t] = a0 <z, E[t]>,   total[t] = base[t] + sum_k contrib[k, t]

and of S[r, t] = sum_k |contrib| + |base|; an fp32 emulation of c_k in lgc_fold_in's specified order (foldin_support's
pieces); and the top-m selection under lgc_mask_topk's total order as a NaN partition + stable sort (topk_support)."""
import numpy as np

import foldin_support as fs
import topk_support as ts

U = fs.U
f32 = np.float32


def session_coeffs32(ptr, items, weights, item_dis, n_items, normalize):
    """(c fp32 per entry, ok bool per entry): c_k = (item_dis * w) * d left to right, d = 1 / sqrt(deg) with deg the fp32 sum
    of the weights that count, sequentially in list order, inf -> 0; normalize False: c_k = w_k.  Skipped entries: c = 0."""
    c = np.zeros(len(items), dtype=f32)
    ok = (items >= 0) & (items < n_items)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r in range(len(ptr) - 1):
            lo, hi = int(ptr[r]), int(ptr[r + 1])
            it, w = fs._row(ptr, items, weights, r, n_items)
            d = f32(1.0)
            if normalize:
                deg = f32(0.0)
                for wk in w:
                    deg = f32(deg + wk)
                d = f32(f32(1.0) / np.sqrt(deg, dtype=f32))
                if np.isinf(d):
                    d = f32(0.0)
                ck = ((item_dis[it].astype(f32) * w).astype(f32) * d).astype(f32)
            else:
                ck = w
            c[lo:hi][ok[lo:hi]] = ck
    return c, ok


def session_coeffs64(ptr, items, weights, item_dis, n_items, normalize):
    """The same in fp64 on the fp32 inputs (no intermediate rounding)."""
    c = np.zeros(len(items))
    ok = (items >= 0) & (items < n_items)
    for r in range(len(ptr) - 1):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        it, w = fs._row(ptr, items, weights, r, n_items)
        w = w.astype(np.float64)
        ck = w
        if normalize:
            deg = w.sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                d = 1.0 / np.sqrt(deg) if len(w) else np.inf
            d = 0.0 if np.isinf(d) else d
            ck = item_dis[it].astype(np.float64) * w * d
        c[lo:hi][ok[lo:hi]] = ck
    return c, ok


def reference64(ptr, items, c, ok, fold, table, targets, init_rows, init, a0):
    """(contrib [n_entries, T], base [R, T], total [R, T], S [R, T]) in fp64.  ``ptr`` / ``items`` / ``c`` / ``ok``: the lists
    as a CSR with one coefficient and one "counts" flag per entry; ``targets`` int64 [R, T] (outside [0, n_items): nothing)."""
    n_rows, n_t = targets.shape
    n_items = fold.shape[0]
    fold64, table64 = fold.astype(np.float64), table.astype(np.float64)
    contrib = np.zeros((len(items), n_t))
    base, total, s = np.zeros((n_rows, n_t)), np.zeros((n_rows, n_t)), np.zeros((n_rows, n_t))
    for r in range(n_rows):
        t_ok = (targets[r] >= 0) & (targets[r] < n_items)
        e_t = table64[np.where(t_ok, targets[r], 0)] * t_ok[:, None]                  # [T, D], zeros where nothing
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        keep = ok[lo:hi]
        rows = fold64[np.where(keep, items[lo:hi], 0)]
        with np.errstate(invalid="ignore"):
            part = (np.asarray(c[lo:hi], dtype=np.float64) * keep)[:, None] * (rows @ e_t.T)
        part[~keep] = 0.0
        part[:, ~t_ok] = 0.0
        contrib[lo:hi] = part
        if init_rows is not None and 0 <= init_rows[r] < init.shape[0]:
            base[r] = float(f32(a0)) * (e_t @ init[init_rows[r]].astype(np.float64))
        total[r] = base[r] + part.sum(axis=0)
        s[r] = np.abs(base[r]) + np.abs(part).sum(axis=0)
    return contrib, base, total, s


def sequential_total32(contrib_rows, keep, base):
    """fp32: the contributions that count added in list order from +0, the base last.  contrib_rows [n, T], base [T]."""
    acc = np.zeros(contrib_rows.shape[1], dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in np.flatnonzero(keep):
            acc = (acc + contrib_rows[j]).astype(f32)
        return (acc + base.astype(f32)).astype(f32)


def top_ref(values, keep, items, m):
    """(pos int32 [m], item int64 [m], value fp32 [m]) of one (row, target): the entries that count ranked in
    lgc_mask_topk's order on the value -- every NaN first, +inf, finite descending with -0 = +0, -inf; equal elements
    by ascending list position --, the first m of them; unused places -1 / -1 / +0.  Positions count skipped entries."""
    pos, item, value = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int64), np.zeros(m, dtype=f32)
    where = np.flatnonzero(keep)
    k = min(m, len(where))
    if k:
        idx, _ = ts.topk_ref(np.asarray(values, dtype=f32)[where], k)
        pos[:k], item[:k], value[:k] = where[idx], np.asarray(items)[where[idx]], np.asarray(values, dtype=f32)[where[idx]]
    return pos, item, value


def top_ref_block(values, keep, items, m):
    """``top_ref`` for every target column of one row at once: values fp32 [n, T] -> (pos [T, m], item [T, m], value [T, m]).
    Columns without a NaN are ranked by one stable sort of -(x + 0) along the list; a column with a NaN goes through
    ``top_ref`` (the NaN partition)."""
    values = np.asarray(values, dtype=f32)
    n_t = values.shape[1]
    pos, item, value = np.full((n_t, m), -1, dtype=np.int32), np.full((n_t, m), -1, dtype=np.int64), np.zeros((n_t, m), dtype=f32)
    where = np.flatnonzero(keep)
    k = min(m, len(where))
    if k:
        x = values[where]
        order = np.argsort(-(x + f32(0.0)), axis=0, kind="stable")[:k]                 # [k, T] indices into `where`
        cols = np.arange(n_t)
        pos[:, :k], item[:, :k] = where[order].T, np.asarray(items)[where[order]].T
        value[:, :k] = x[order, cols[None, :]].T
        for t in np.flatnonzero(np.isnan(x).any(axis=0)):
            pos[t], item[t], value[t] = top_ref(values[:, t], keep, items, m)
    return pos, item, value
