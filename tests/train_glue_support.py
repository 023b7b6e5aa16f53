"""References, bounds and input builders for the kernels of a training step (tests/test_train_glue_host.py and
tests/test_train_glue_gpu.py).  Everything here is numpy: float64 arithmetic on the very fp32 inputs the kernels read, or
an fp32 restatement of an order of operations where the kernel promises exact bits.  No project code is imported.

Bounds count roundings; u = 2^-24 is the unit roundoff of fp32."""
import math

import numpy as np

U = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = 2.0 ** -126
WAVE = 64            # lanes of a wavefront
ONE_GROUP = 1024     # threads of the one-workgroup kernels (BPR loss, regulariser)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def worst_ratio(err, bound):
    """max err / bound; an error of exactly 0 is inside any bound (0 / 0 counts as 0), a NaN anywhere is infinitely bad."""
    err, bound = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    if err.size == 0:
        return 0.0
    if np.isnan(err).any() or np.isnan(bound).any():
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def column_slice(rng, rows, dim, stride, offset, scale=1.0):
    """(wide fp32 [rows, stride], offset): the table under test is wide[:, offset:offset + dim]."""
    assert offset + dim <= stride
    return f32(rng.standard_normal((rows, stride)) * scale), offset


# ----------------------------------------------------------------------------------------
# pair scores
# ----------------------------------------------------------------------------------------
def pair_scores_ref(emb, idx0, idx1):
    """(scores f64 with NaN for an invalid pair, sum |a||b| f64, rows0 f32, rows1 f32, ok uint8)."""
    emb = np.asarray(emb)
    n = emb.shape[0]
    idx0, idx1 = np.asarray(idx0, dtype=np.int64), np.asarray(idx1, dtype=np.int64)
    ok = (idx0 >= 0) & (idx0 < n) & (idx1 >= 0) & (idx1 < n)
    rows0 = np.where(ok[:, None], emb[np.where(ok, idx0, 0)], np.float32(0))
    rows1 = np.where(ok[:, None], emb[np.where(ok, idx1, 0)], np.float32(0))
    a, b = rows0.astype(np.float64), rows1.astype(np.float64)
    scores = (a * b).sum(1)
    scores[~ok] = np.nan
    return scores, (np.abs(a) * np.abs(b)).sum(1), f32(rows0), f32(rows1), ok.astype(np.uint8)


def pair_scores_bound(dim, mag):
    """A lane adds ceil(dim / 64) rounded products in a chain, six butterfly levels follow: ceil(dim / 64) + 6 roundings on
    any path to the result, +1 for the second-order terms."""
    return (math.ceil(dim / WAVE) + 7) * U * np.asarray(mag, dtype=np.float64)


def pair_scores_emulated(rows0, rows1):
    """The kernel's order in fp32: lane l adds columns l, l + 64, ... (product rounded, then added), then the xor butterfly."""
    p = f32(rows0) * f32(rows1)
    m, dim = p.shape
    k = math.ceil(dim / WAVE)
    padded = np.zeros((m, k * WAVE), dtype=np.float32)
    padded[:, :dim] = p
    lanes = np.zeros((m, WAVE), dtype=np.float32)
    for j in range(k):
        lanes = lanes + padded[:, j * WAVE:(j + 1) * WAVE]
    off = WAVE // 2
    while off:
        lanes = lanes + lanes[:, np.arange(WAVE) ^ off]
        off //= 2
    return lanes[:, 0]


def pair_seed_vals_ref(grad_scores, mask, scale, rows0, rows1):
    """Exact: g = mask ? grad : 0, then fl(g * scale), then fl(g * row) -- [g rows1 | g rows0]."""
    g = f32(grad_scores)
    if mask is not None:
        g = np.where(np.asarray(mask) != 0, g, np.float32(0))
    if scale is not None:
        g = g * np.float32(scale)
    g = f32(g)[:, None]
    return np.concatenate([g * f32(rows1), g * f32(rows0)])


# ----------------------------------------------------------------------------------------
# BPR loss
# ----------------------------------------------------------------------------------------
PLANTED_D = [0.0, 1e-8, -1e-8, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]


def bpr_scores(rng, b, planted=True):
    """[pos | neg] scores randn * 3 with the differences of PLANTED_D planted (as many as the batch has room for)."""
    s = f32(rng.standard_normal(2 * b) * 3)
    if planted:
        for j, d in enumerate(PLANTED_D):
            t = (j * 37 + 5) % b
            if abs(d) < 1:
                s[b + t] = 0.0           # d itself is the fp32 difference
            s[t] = np.float32(s[b + t] + np.float32(d))
    return s


def bpr_ref(scores, mask, size):
    """(loss f64, grad f64 [2B]): d is the kernel's one fp32 subtraction, everything after it float64."""
    s = f32(scores)
    b = s.size // 2
    on = np.ones(b, dtype=bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(on, s[:b] - s[b:], np.float32(0)).astype(np.float64)
    logsig = np.minimum(d, 0.0) - np.log1p(np.exp(-np.abs(d)))
    sg = np.exp(-np.logaddexp(0.0, d))                       # sigmoid(-d) without overflow
    loss = -math.fsum(logsig[on]) / size
    g = np.where(on, sg / size, 0.0)
    return loss, np.concatenate([-g, g])


def bpr_grad_bound(ref, size, rel=8 * 2.0 ** -23):
    return rel * np.abs(ref) + F32_TINY / size


def bpr_loss_bound(b, rel=8 * 2.0 ** -23):
    """Relative: every term has one sign; a thread adds ceil(B / 1024) terms, ten tree levels and the scaling follow."""
    return rel + (math.ceil(b / ONE_GROUP) + 11) * U


def bpr_emulated(scores, mask, size):
    """The kernel's formula and order in fp32 with the host's libm: thread i adds triples i, i + 1024, ...; then a halving tree."""
    s = f32(scores)
    b = s.size // 2
    on = np.ones(b, dtype=bool) if mask is None else np.asarray(mask) != 0
    inv = np.float32(1.0) / np.float32(size)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.where(on, s[:b] - s[b:], np.float32(0))
        ls = np.minimum(d, np.float32(0)) - np.log1p(np.exp(-np.abs(d)))
        sg = np.float32(1) / (np.float32(1) + np.exp(d))
    g = np.where(on, sg * inv, np.float32(0)).astype(np.float32)
    k = math.ceil(b / ONE_GROUP)
    terms = np.zeros(k * ONE_GROUP, dtype=np.float32)
    terms[:b] = np.where(on, ls, np.float32(0))
    part = np.zeros(ONE_GROUP, dtype=np.float32)
    for j in range(k):
        part = part + terms[j * ONE_GROUP:(j + 1) * ONE_GROUP]
    half = ONE_GROUP // 2
    while half:
        part = part[:half] + part[half:2 * half]
        half //= 2
    return np.float32(-part[0] * inv), np.concatenate([-g, g])


# ----------------------------------------------------------------------------------------
# regulariser
# ----------------------------------------------------------------------------------------
def reg_rows_ref(w, lists, scale):
    """(value f64, rows int64): scale * sum over the lists of |w[id]|^2; negative ids wrap, ids outside [-n, n) are -1 and add
    nothing."""
    w = np.asarray(w)
    n = w.shape[0]
    ids = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if lists else np.zeros(0, dtype=np.int64)
    wrapped = np.where(ids < 0, ids + n, ids)
    ok = (wrapped >= 0) & (wrapped < n)
    rows = np.where(ok, wrapped, -1)
    sq = (w[rows[ok]].astype(np.float64) ** 2).sum()
    return float(np.float32(scale)) * float(sq), rows


def reg_rows_bound(dim, total):
    """Relative (all terms >= 0): dim adds per row, ceil(total / 1024) rows per thread, 6 shuffle levels, 16 wave sums,
    sqrt and square, three list sums, the scale -- below 30."""
    return (dim + math.ceil(total / ONE_GROUP) + 30) * U


def reg_rows_emulated(w, lists, scale):
    """The kernel's order in fp32: a thread per row (columns in order), rows t, t + 1024, ... per thread and list, shuffle-down
    tree over a wavefront, the 16 wavefronts in order, (sqrt S)^2 per list."""
    w = f32(w)
    n, dim = w.shape
    _, rows = reg_rows_ref(w, lists, scale)
    which = np.repeat(np.arange(3), [len(x) for x in lists])
    total = rows.size
    sq = np.zeros(total, dtype=np.float32)
    safe = np.where(rows >= 0, rows, 0)
    for c in range(dim):
        x = w[safe, c]
        sq = sq + x * x
    sq = np.where(rows >= 0, sq, np.float32(0))
    k = max(math.ceil(total / ONE_GROUP), 1)
    out = np.float32(0)
    for j in range(3):
        terms = np.zeros(k * ONE_GROUP, dtype=np.float32)
        terms[:total] = np.where(which == j, sq, np.float32(0))
        acc = np.zeros(ONE_GROUP, dtype=np.float32)
        for i in range(k):
            acc = acc + terms[i * ONE_GROUP:(i + 1) * ONE_GROUP]
        lanes = acc.reshape(ONE_GROUP // WAVE, WAVE).copy()
        off = WAVE // 2
        while off:
            lanes[:, :WAVE - off] = lanes[:, :WAVE - off] + lanes[:, off:]
            off //= 2
        s = np.float32(0)
        for v in lanes[:, 0]:
            s = np.float32(s + v)
        nrm = np.sqrt(s, dtype=np.float32)
        out = np.float32(out + np.float32(nrm * nrm))
    return np.float32(out * np.float32(scale))


# ----------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------
def adam_hyper(t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The six fp32 scalars of a step: 1 - b1, b2, 1 - b2, eps, lr / (1 - b1^t), sqrt(1 - b2^t), rounded from double."""
    return f32([1.0 - beta1, beta2, 1.0 - beta2, eps, lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)])


def adam_inputs(rng, n):
    """(w, g, m, v) fp32 [n]: gradients with exact zeros, 1e-20, 1e18 and 1e20; fresh (zero) moments on a part of the normal-sized
    gradients and of the zero gradients, moments of an earlier step elsewhere."""
    w = f32(rng.standard_normal(n) * 0.1)
    g = f32(rng.standard_normal(n))
    m = f32(rng.standard_normal(n) * 0.5)
    v = f32(rng.random(n) * 0.5 + 1e-3)
    special = f32([0.0, 1e-20, 1e18, 1e20, -1e20, -1e-20])
    kind = rng.integers(0, 12, size=n)
    hit = kind < special.size
    g[hit] = special[kind[hit]]
    g[(np.abs(g) < 1e-3) & ~hit] = 0.0                                   # small random gradients become exact zeros
    fresh = (rng.random(n) < 0.3) & ((g == 0) | ((np.abs(g) >= 1e-3) & (np.abs(g) <= 10)))
    m[fresh] = 0.0
    v[fresh] = 0.0
    return w, g, m, v


def adam_ref(w, g, m, v, hyper):
    """(w', m', v') float64 from the fp32 inputs; a second moment beyond fp32's range is +inf and the update then 0."""
    omb1, b2, omb2, eps, step, bc2s = (float(x) for x in f32(hyper))
    w, g, m, v = (np.asarray(x, dtype=np.float64) for x in (w, g, m, v))
    m1 = m + (g - m) * omb1
    v1 = b2 * v + omb2 * g * g
    v1 = np.where(v1 > F32_MAX, np.inf, v1)
    w1 = w - step * (m1 / (np.sqrt(v1) / bc2s + eps))
    return w1, m1, v1


def adam_bounds(w, g, m, v, hyper):
    """(bound_w, bound_m, bound_v) as DESIGN.md section 15 states them."""
    _, _, _, eps, step, bc2s = (float(x) for x in f32(hyper))
    w1, m1, v1 = adam_ref(w, g, m, v, hyper)
    mag = np.abs(np.asarray(m, dtype=np.float64)) + np.abs(np.asarray(g, dtype=np.float64))
    bound_w = U * np.abs(w1) + 16 * U * step * mag / (np.sqrt(v1) / bc2s + eps)
    return bound_w, 4 * U * mag, 4 * U * v1


def adam_errors(got, ref):
    """|got - ref| where the reference is finite; where it is +inf the kernel must hold +inf too (error 0, else inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(ref), np.where(got == ref, 0.0, np.inf), np.abs(got - ref))


def adam_emulated(w, g, m, v, hyper):
    """The kernel's expression in fp32, every operation rounded."""
    omb1, b2, omb2, eps, step, bc2s = f32(hyper)
    w, g, m, v = (f32(x) for x in (w, g, m, v))
    with np.errstate(over="ignore"):
        m1 = m + (g - m) * omb1
        v1 = b2 * v + omb2 * g * g
        w1 = w - step * (m1 / (np.sqrt(v1) / bc2s + eps))
    return w1, m1, v1


# ----------------------------------------------------------------------------------------
# segment sums, seed preparation, linear combinations
# ----------------------------------------------------------------------------------------
SEGMENT_RUNS = [1, 1, 2, 3, 1, 40, 1, 5000, 7, 1, 1, 64, 33, 1]                      # the last position is a head
SEGMENT_DEST = [4, 9, -1, 0, 49, 17, 50, 3, 1000, 2, 8, 30, 31, 12]                  # -1, 50, 1000: skipped (50 output rows)
SEGMENT_KEYS = [-(2 ** 40), -3, 5, 8, 11, 14, 17, 20, 23, 26, 29, 32, 35, 2 ** 62]
SEGMENT_ROWS = 50


def segment_layout():
    """(keys int64 [n], dest int64 [n]) of the run layout above; positions that are no heads carry dest -7."""
    runs = np.asarray(SEGMENT_RUNS)
    keys = np.repeat(np.asarray(SEGMENT_KEYS, dtype=np.int64), runs)
    dest = np.full(keys.size, -7, dtype=np.int64)
    dest[np.cumsum(runs) - runs] = SEGMENT_DEST
    return keys, dest


def segment_sum_ref(keys, dest, vals, vals_index, base, scale, accumulate):
    """Exact: per run head with 0 <= dest < rows a sequential fp32 sum, one scaling, one add."""
    keys, dest, vals = np.asarray(keys), np.asarray(dest), f32(vals)
    out = f32(base).copy()
    if keys.size == 0:
        return out
    if vals_index is not None:
        vals = vals[np.asarray(vals_index, dtype=np.int64)]
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    ends = np.concatenate([heads[1:], [keys.size]])
    for h, e in zip(heads, ends):
        d = int(dest[h])
        if 0 <= d < out.shape[0]:
            run = np.concatenate([np.zeros((1, vals.shape[1]), dtype=np.float32), vals[h:e]])
            tot = np.cumsum(run, axis=0, dtype=np.float32)[-1]
            first = out[d] if accumulate else np.zeros_like(tot)
            out[d] = first + np.float32(scale) * tot
    return out


def seed_prepare_ref(rows, split, n):
    """A stable sort by row id with ids outside [0, n) as -1 = "no row", and what follows from it:
    dict(rows_sorted, perm int32, dest_item, dest_slot, dest_user, flag uint8 [split + 1], slot int32 [split + 1] (-7 unset))."""
    rows = np.asarray(rows, dtype=np.int64)
    r = np.where((rows >= 0) & (rows < n), rows, -1)
    order = np.argsort(r, kind="stable")
    rs = r[order]
    pos = np.arange(rs.size, dtype=np.int64)
    head = np.ones(rs.size, dtype=bool)
    head[1:] = rs[1:] != rs[:-1]
    user, item = (rs >= 0) & (rs < split), rs >= split
    flag = np.zeros(split + 1, dtype=np.uint8)
    slot = np.full(split + 1, -7, dtype=np.int32)
    hu = head & user
    flag[rs[hu]] = 1
    slot[rs[hu]] = pos[hu]
    return dict(rows_sorted=rs, perm=order.astype(np.int32), dest_item=np.where(head & item, rs, -1),
                dest_slot=np.where(hu, pos, -1), dest_user=np.where(hu, rs, -1), flag=flag, slot=slot)


SEED_PATTERNS = ["random_run", "all_equal", "descending", "all_out_of_range", "all_users", "all_items", "edges"]


def seed_rows(pattern, m, split, n, rng):
    """Row-id lists for seed preparation; "edges": ids at split - 1, split, n - 1, 0 and just outside the table."""
    if pattern == "random_run":
        rows = rng.integers(-3, n + 3, size=m)
        rows[: m // 3] = rows[0] if m else 0
        return rng.permutation(rows).astype(np.int64)
    if pattern == "all_equal":
        return np.full(m, min(7, n - 1), dtype=np.int64)
    if pattern == "descending":
        return (n - 1 - np.arange(m, dtype=np.int64) % n) if m <= n else np.sort(rng.integers(0, n, size=m))[::-1].astype(np.int64)
    if pattern == "all_out_of_range":
        return np.where(np.arange(m) % 2 == 0, -1 - np.arange(m), n + np.arange(m)).astype(np.int64)
    if pattern == "all_users":
        return rng.integers(0, max(split, 1), size=m).astype(np.int64) if split > 0 else np.full(m, -1, dtype=np.int64)
    if pattern == "all_items":
        return rng.integers(split, n, size=m).astype(np.int64) if split < n else np.full(m, n, dtype=np.int64)
    assert pattern == "edges"
    pool = np.asarray([split - 1, split, n - 1, 0, -1, n, split - 1, n - 1, 2 ** 40], dtype=np.int64)
    return pool[rng.integers(0, pool.size, size=m)]


def lincomb_ref(terms):
    """Exact: fl(c0 * s0), then + fl(ct * st) in term order."""
    acc = np.float32(terms[0][0]) * f32(terms[0][1])
    for c, s in terms[1:]:
        acc = acc + np.float32(c) * f32(s)
    return acc


# ----------------------------------------------------------------------------------------
# seeded pull
# ----------------------------------------------------------------------------------------
PULL_DEGREES = ([1, 2, 3, 4, 5, 0, 6, 7, 8, 9, 10] + [300, 33, 40, 0, 50, 700, 64, 70] + [10, 9, 8, 7, 6, 0, 5, 4, 3, 2, 1] +
                [450, 600, 0, 0])
PULL_USERS = 800
PULL_PLANS = [(0, 7), (4, 16), (32, 256), (100000, 256)]


def pull_graph(seed=11):
    """(edge_index int64 [2, E], edge_weight fp32 [E], n_users, n_items): a symmetric user|item edge list whose item degrees
    are PULL_DEGREES -- 1..10, 33..70, 300..700 and a few isolated items, in the middle and at the end; the last user has an
    edge, so the user|item split is n_users."""
    rng = np.random.default_rng(seed)
    us, its = [], []
    for i, d in enumerate(PULL_DEGREES):
        users = rng.choice(PULL_USERS, size=d, replace=False)
        if d == 700:
            users = np.arange(PULL_USERS - 700, PULL_USERS)
        us.append(users)
        its.append(np.full(d, PULL_USERS + i))
    u, i = np.concatenate(us).astype(np.int64), np.concatenate(its).astype(np.int64)
    order = rng.permutation(u.size)
    u, i = u[order], i[order]
    w = f32(rng.random(u.size) * 0.9 + 0.1)
    return np.stack([np.concatenate([u, i]), np.concatenate([i, u])]), np.concatenate([w, w]), PULL_USERS, len(PULL_DEGREES)


def pull_seeds(edge_index, n_users, n_items, seed=3):
    """Seed row lists of the pull: none; one user -- in the longest row (every user from 100 on is) and in none of the other
    long rows, so that most rows of every class hold no seed; forty users with repeats and ten items (which the pull ignores)."""
    u, i = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    fwd = u < n_users
    deg = np.bincount(i[fwd] - n_users, minlength=n_items)
    other_long = np.flatnonzero((deg >= 300) & (deg < 700)) + n_users
    in_long = np.zeros(n_users, dtype=bool)
    in_long[u[fwd][np.isin(i[fwd], other_long)]] = True
    one = int(np.flatnonzero(~in_long[100:])[0]) + 100
    rng = np.random.default_rng(seed)
    many = rng.integers(0, n_users, size=40)
    many[:5] = many[0]
    return {"none": np.zeros(0, dtype=np.int64), "one_user": np.asarray([one], dtype=np.int64),
            "forty_users": np.concatenate([many, rng.integers(n_users, n_users + n_items, size=10)]).astype(np.int64)}


def plan_classes(deg, short_max, chunk_len):
    """(short rows, single-chunk rows, multi-chunk rows, chunks) of a row plan over rows of these lengths."""
    deg = np.asarray(deg)
    long_ = deg > short_max
    nch = -(-deg[long_] // chunk_len)
    return int((~long_).sum()), int((nch == 1).sum()), int((nch > 1).sum()), int(nch.sum())


def seed_pull_ref(rowptr, cols, vals, row_begin, row_end, flag, slot, seed_vals):
    """(out f64 [row_end - row_begin, dim], sum |val||x| f64, flagged entries per row): entries whose column carries a flag read
    seed_vals[slot[col]]; everything else contributes nothing."""
    rowptr, cols, vals = np.asarray(rowptr, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    x = np.asarray(seed_vals, dtype=np.float64)
    dim = x.shape[1]
    out = np.zeros((row_end - row_begin, dim))
    mag = np.zeros_like(out)
    count = np.zeros(row_end - row_begin, dtype=np.int64)
    for r in range(row_begin, row_end):
        c, a = cols[rowptr[r]:rowptr[r + 1]], vals[rowptr[r]:rowptr[r + 1]]
        on = np.asarray(flag)[c] != 0
        if on.any():
            xs = x[np.asarray(slot, dtype=np.int64)[c[on]]]
            out[r - row_begin] = (a[on, None] * xs).sum(0)
            mag[r - row_begin] = (np.abs(a[on, None]) * np.abs(xs)).sum(0)
            count[r - row_begin] = int(on.sum())
    return out, mag, count


def seed_pull_bound(mag, count):
    return (np.asarray(count, dtype=np.float64)[:, None] + 2) * U * mag


def seed_pull_emulated(rowptr, cols, vals, row_begin, row_end, flag, slot, seed_vals, short_max, chunk_len, groups):
    """The plan's order in fp32: a short row adds its entries in order; a chunk hands entry k to lane group (k - begin) % groups,
    adds the group sums in group order; a row's chunk sums are added by lane group (slot j to group j % groups), those in
    group order again.  An unflagged entry adds val * 0."""
    rowptr, cols = np.asarray(rowptr, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals, x = f32(vals), f32(seed_vals)
    dim = x.shape[1]
    zero = np.zeros(dim, dtype=np.float32)

    def grouped(terms):
        acc = [zero.copy() for _ in range(groups)]
        for k, t in enumerate(terms):
            acc[k % groups] = acc[k % groups] + t
        tot = acc[0]
        for a in acc[1:]:
            tot = tot + a
        return tot

    out = np.zeros((row_end - row_begin, dim), dtype=np.float32)
    for r in range(row_begin, row_end):
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        terms = [vals[k] * (x[slot[cols[k]]] if flag[cols[k]] else zero) for k in range(s, e)]
        if e - s <= short_max:
            tot = zero.copy()
            for t in terms:
                tot = tot + t
        else:
            nch = -(-(e - s) // chunk_len)
            per = -(-(e - s) // nch)
            sums = [grouped(terms[j * per:min((j + 1) * per, e - s)]) for j in range(nch)]
            tot = sums[0] if nch == 1 else grouped(sums)
        out[r - row_begin] = tot
    return out
