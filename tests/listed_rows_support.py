"""Small named operators, named row lists and numpy references for the tests of the listed-rows hop
(tests/test_listed_rows_host.py, tests/test_listed_rows_gpu.py).

The listed-rows hop: ``lgc_spmm_rows`` (``k_spmm_rows``: one wavefront per list position, ``listed_row_body``) and
``lgc_spmm_rows_split`` -- ``k_rows_plan`` (one workgroup: counts the listed entries, picks the chunk length, scans the chunk
counts), ``k_rows_chunks`` (a fixed grid striding over the chunk numbers, a 64-ary search for the list position that owns a
chunk, ``listed_row_body`` / ``chunk_core``) and ``k_rows_combine`` (``combine_core``).

An operator is a ``tiles_support.TileOp``: a CSR over ``table_rows`` rows and a range ``[row_begin, row_end)`` with
``row_begin > 0``; columns are drawn with repeats from the first hundred table rows, values and tables from
``tiles_support.draw`` (sign x [2^-6, 2^6): no product and no partial sum is subnormal).  A row list is an int64 array of ids
on one operator; each list exists for one property, which test_listed_rows_host.py asserts.

The references are numpy only and written from the contract the kernels state, not from tests/cpu_ops.py, the library or
tests/train_glue_support.py:

  plan      c_m = 0 for an id outside [row_begin, row_end), 1 for a row of up to 32 entries, else ceil(len_m / L);
            work[m] = c_0 + .. + c_(m-1), work[n_ids] = the chunk count, work[n_ids + 1] = L;  L = 256 unless
            total // 256 > room (total = the listed rows' entries, room = partial_rows - n_ids), then ceil(total / room)
            rounded up to a multiple of 64
  sums      a row of up to 32 entries: acc = +0, acc = fl(acc + fl(val * x[col])) in stored order (the tile path's rule);
            a longer span [begin, end) -- a whole row, or one chunk [s + j L, min(s + (j + 1) L, e)) -- hands entry k to
            lane group (k - begin) % groups, every group adds its entries in order from +0 and the group sums are added as
            ((g0 + g1) + g2) + ..;  a cut row's chunk sums are added the same way, slot j by group j % groups
  epilogue  fl(a * acc) if a != 1, then fl(acc + fl(b * r[row])) if r is given (``tiles_support.finish``)

with groups = 64 // lpr, lpr = ceil(dim / 4) lanes per row from 4 columns up, else dim.
"""
import functools
from dataclasses import dataclass

import numpy as np

import tiles_support as T

SHORT_MAX, CHUNK_LEN, WAVE, SCAN_TILE, GRID_WAVES, DEFAULT_ROOM = 32, 256, 64, 1024, 8192, 16384
SENTINEL = T.SENTINEL
EPILOGUES = T.EPILOGUES
COLUMN_ROWS = 100                                   # every column names one of the first hundred table rows

# 64, 64, 64, 32, 16, 4, 3, 2, 2, 1, 1 lane groups; 3: an idle last lane; 7, 65, 90, 129: overlapping last lanes.  The issue's
# widths, and 16 for the 16 lane groups none of them gives.
DIMS = (1, 3, 4, 7, 16, 64, 65, 90, 128, 129, 256)
ONE_DIM_PER_GROUPS = (1, 3, 16, 7, 64, 65, 90, 129)            # 64, 21, 16, 32, 4, 3, 2, 1 lane groups
NARROW_DIMS = (1, 4)                                           # 64 lane groups: the widths that need the widest hub
LAYOUTS = ("dense", "padded", "odd")
TIGHT_ROOMS = (1, 2, 8)
CUT_LENS = (256, 320, 4096)                                    # the default chunk length and two lengthened ones (host bound test)


def lanes_per_row(dim):
    return -(-dim // 4) if dim >= 4 else dim


def groups_of(dim):
    return WAVE // lanes_per_row(dim)


ALL_GROUPS = tuple(sorted({groups_of(d) for d in DIMS}))       # 1, 2, 3, 4, 16, 21, 32, 64


def hub_chunks(groups):
    """Chunks (at 256 entries) of the hub for a lane-group count: more than 4 * groups, so every group of ``combine_core``
    runs its four-slot loop once, and groups // 2 + 1 more, so the first groups take one slot after the loop and, from 3 groups up, the others none."""
    return 4 * groups + groups // 2 + 1


def hub_length(groups):
    return (hub_chunks(groups) - 1) * CHUNK_LEN + 1 + (37 * groups) % (CHUNK_LEN - 1)        # a last chunk of 1 .. 255


SWITCH_LENGTHS = [0, 1, 3, 4, 5, 31, 32, 33, 34]               # the short / long switch of listed_row_body
ONE_CHUNK_LENGTHS = [63, 64, 65, 192, 193]                     # one chunk; at 64 lane groups the edge of the pipelined loop
BOUNDARY_LENGTHS = [255, 256, 257, 511, 512, 513, 768]         # chunk boundaries at 256
HUB_LENGTHS = [hub_length(g) for g in ALL_GROUPS if g < 64]
WIDE_HUB_LENGTH = hub_length(64)
MANY_SHORT_ROWS = 8200
MANY_SHORT_LONG = [257, 512, 513, 768, 1300, hub_length(4)]


def _build(name, seed, lengths, row_begin, after_rows, before=(), after=()):
    """Rows [row_begin, row_begin + len(lengths)) get ``lengths``; rows outside the range get ``before`` / ``after`` (missing
    ones are empty), so an id outside the range names a row that has entries too."""
    rng = np.random.default_rng([20261021, seed])
    row_end = row_begin + len(lengths)
    table_rows = row_end + after_rows
    assert table_rows >= COLUMN_ROWS and len(before) <= row_begin and len(after) <= after_rows
    full = np.zeros(table_rows, np.int64)
    full[:len(before)] = before
    full[row_begin:row_end] = lengths
    full[row_end:row_end + len(after)] = after
    rowptr = np.concatenate([[0], np.cumsum(full)]).astype(np.int64)
    cols = rng.integers(0, COLUMN_ROWS, size=int(rowptr[-1])).astype(np.int32)
    return T.TileOp(name, rowptr, cols, T.draw(rng, cols.size), row_begin, row_end, table_rows)


def _shuffled(seed, values):
    values = np.array(values, np.int64)
    np.random.default_rng([11, seed]).shuffle(values)
    return values


@functools.lru_cache(maxsize=None)
def operators():
    ops = [
        _build("lengths", 1, _shuffled(1, (SWITCH_LENGTHS + ONE_CHUNK_LENGTHS + BOUNDARY_LENGTHS + HUB_LENGTHS) * 2), 7, 41,
               before=[3, 40, 0, 300, 1, 33, 600], after=[2, 0, 257, 35, 8]),
        _build("wide_hub", 2, _shuffled(2, [WIDE_HUB_LENGTH, 257, 5, 0, 33, 256, 700, 12]), 3, 97, before=[5, 300], after=[40, 1, 258]),
        _build("many_short", 3, [i % 9 for i in range(MANY_SHORT_ROWS)] + MANY_SHORT_LONG, 4, 6, before=[300, 2, 0, 9],
               after=[3, 260]),
    ]
    return {op.name: op for op in ops}


OP_NAMES = ("lengths", "wide_hub", "many_short")


def rows_of_length(op, n):
    """The range rows of exactly ``n`` entries, ascending."""
    deg = op.lengths[op.row_begin:op.row_end]
    return (np.flatnonzero(deg == n) + op.row_begin).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the row lists
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class RowList:
    name: str
    op: str
    ids: np.ndarray             # int64 [n_ids]

    @property
    def n_ids(self):
        return int(self.ids.size)


def foreign_ids(op, n, seed):
    """``n`` ids outside [row_begin, row_end), the four kinds in rotation: below the range, in [row_end, table_rows), at or
    beyond table_rows (far beyond 2^31 too), negative."""
    rng = np.random.default_rng([13, seed])
    beyond = [op.table_rows, op.table_rows + 1, op.table_rows + 4097, 2 ** 31 + 5, 2 ** 40 + 3, 2 ** 62]
    negative = [-1, -2, -op.table_rows, -2 ** 31 - 7, -2 ** 40, -2 ** 62]
    kinds = (lambda: int(rng.integers(0, op.row_begin)), lambda: int(rng.integers(op.row_end, op.table_rows)),
             lambda: beyond[int(rng.integers(0, len(beyond)))], lambda: negative[int(rng.integers(0, len(negative)))])
    return [kinds[(i + seed) % 4]() for i in range(n)]


def is_foreign(op, ids):
    ids = np.asarray(ids, np.int64)
    return (ids < op.row_begin) | (ids >= op.row_end)


def _sized(op, n, seed):
    """``n`` positions mixing ids without a chunk, with one and with several; a multi-chunk row sits at the last position
    before and the first position after every 1024 boundary, and a chunk-less id now and then right after it."""
    rng = np.random.default_rng([17, seed, n])
    deg = op.lengths
    pool = [r for r in op.range_rows() if deg[r] <= 768]
    multi = [r for r in pool if deg[r] > CHUNK_LEN]
    ids = []
    for i in range(n):
        kind = int(rng.integers(0, 8))
        if kind < 2:
            ids.append(foreign_ids(op, 1, seed + i)[0])
        elif kind == 2:
            ids.append(multi[int(rng.integers(0, len(multi)))])
        else:
            ids.append(pool[int(rng.integers(0, len(pool)))])
    for edge in range(SCAN_TILE, n + 1, SCAN_TILE):
        ids[edge - 1] = multi[(edge // SCAN_TILE) % len(multi)]
        if edge < n:
            ids[edge] = multi[(edge // SCAN_TILE + 3) % len(multi)]
        if edge + 1 < n:
            ids[edge + 1] = foreign_ids(op, 1, edge)[0]
    if n == 2:
        ids = [foreign_ids(op, 1, 5)[0], multi[-1]]
    return ids


SIZES = (2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)


@functools.lru_cache(maxsize=None)
def lists():
    ops = operators()
    op, wide, many = ops["lengths"], ops["wide_hub"], ops["many_short"]
    every = list(op.range_rows())
    hub = rows_of_length(op, max(HUB_LENGTHS))[0]
    r257, r5 = rows_of_length(op, 257)[0], rows_of_length(op, 5)[0]
    long_rows = [r for r in every if op.lengths[r] > CHUNK_LEN]           # 56 rows
    out = []

    def add(name, ids, on=op):
        out.append(RowList(name, on.name, np.array(ids, np.int64)))

    add("each_once", every)
    add("reversed", every[::-1])
    add("repeats", [hub, hub, r257, r5, r5, rows_of_length(op, 64)[0], hub, r257, rows_of_length(op, 0)[0], r257, r5])
    add("foreign_head", foreign_ids(op, 66, 1) + every)
    add("foreign_tail", every + foreign_ids(op, 66, 2))
    runs = foreign_ids(op, 1, 3) + [long_rows[0]] + foreign_ids(op, 70, 4) + [long_rows[1]] + foreign_ids(op, 65, 5) + [hub]
    runs += foreign_ids(op, 130, 6) + [r257, r5] + foreign_ids(op, 3, 7) + [long_rows[2], rows_of_length(op, 33)[0]] + foreign_ids(op, 64, 8)
    runs += [long_rows[3]] + foreign_ids(op, 2, 9)
    add("foreign_runs", runs)
    add("all_foreign", foreign_ids(op, 70, 10))
    add("one_0", rows_of_length(op, 0)[:1])
    add("one_32", rows_of_length(op, 32)[:1])
    add("one_33", rows_of_length(op, 33)[:1])
    add("one_hub", [hub])
    deg = op.lengths
    add("only_short", [r for r in every if deg[r] <= SHORT_MAX] * 2)
    for n in SIZES:
        add(f"sized_{n}", _sized(op, n, n))
    add("wide_each_once", list(wide.range_rows()), wide)
    wide_hub_row, w257, w5 = (rows_of_length(wide, n)[0] for n in (WIDE_HUB_LENGTH, 257, 5))
    add("wide_repeats", [wide_hub_row, wide_hub_row, w257, w5, w5] + foreign_ids(wide, 3, 11) + [wide_hub_row, w257, w5, w257], wide)
    add("one_wide_hub", [wide_hub_row], wide)
    deg = many.lengths
    short = [r for r in many.range_rows() if deg[r] <= 8]
    add("beyond_the_grid", short + [r for r in many.range_rows() if deg[r] > CHUNK_LEN], many)
    return {rl.name: rl for rl in out}


LIST_NAMES = ("each_once", "reversed", "repeats", "foreign_head", "foreign_tail", "foreign_runs", "all_foreign", "one_0",
              "one_32", "one_33", "one_hub", "only_short") + tuple(f"sized_{n}" for n in SIZES) + \
             ("wide_each_once", "wide_repeats", "one_wide_hub", "beyond_the_grid")
EVERY_WIDTH_LISTS = ("each_once", "repeats", "foreign_runs")


def dims_of(name):
    """The widths a list runs at: every width for three lists, the 64-group widths for the lists of ``wide_hub``, else
    one width per lane-group count."""
    if name in EVERY_WIDTH_LISTS:
        return DIMS
    if lists()[name].op == "wide_hub":
        return NARROW_DIMS
    return ONE_DIM_PER_GROUPS


def partial_rows_of(rl, room=DEFAULT_ROOM):
    return rl.n_ids + room


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def listed_lengths(op, ids):
    """int64 [n_ids]: the row length of every position, -1 for an id outside the range."""
    ids = np.asarray(ids, np.int64)
    inside = ~is_foreign(op, ids)
    out = np.full(ids.size, -1, np.int64)
    out[inside] = op.lengths[ids[inside]]
    return out


def chunk_length(op, ids, partial_rows):
    lens = listed_lengths(op, ids)
    total = int(lens[lens >= 0].sum())
    room = partial_rows - len(ids)
    assert room >= 1
    if total // CHUNK_LEN > room:
        return -(-(-(-total // room)) // WAVE) * WAVE
    return CHUNK_LEN


def chunk_counts(op, ids, L):
    lens = listed_lengths(op, ids)
    return np.where(lens < 0, 0, np.where(lens <= SHORT_MAX, 1, -(-lens // L)))


def plan(op, ids, partial_rows):
    """int64 [n_ids + 2]: what ``work`` holds after the planning launch."""
    L = chunk_length(op, ids, partial_rows)
    c = chunk_counts(op, ids, L)
    return np.concatenate([[0], np.cumsum(c), [L]]).astype(np.int64)


def owners(work, n_ids):
    """int64 [chunk count]: the list position that owns chunk w -- the LAST position m with work[m] <= w."""
    return np.searchsorted(work[:n_ids], np.arange(int(work[n_ids])), side="right") - 1


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def f32_add(a, b):
    return np.add(a, b, dtype=np.float32)


def products(op, x, begin, end):
    """fp32 [end - begin, dim]: fl(val * x[col]) of the entries [begin, end), one rounding each."""
    return np.multiply(op.vals[begin:end, None], x[op.cols[begin:end]], dtype=np.float32)


def sequential(terms):
    """[.., n, dim] -> [.., dim]: acc = +0, acc = fl(acc + term) in order."""
    acc = np.zeros(terms.shape[:-2] + terms.shape[-1:], np.float32)
    for k in range(terms.shape[-2]):
        acc = f32_add(acc, terms[..., k, :])
    return acc


def grouped(terms, groups):
    """[.., n, dim] -> [.., dim]: term k goes to lane group k % groups, every group adds its terms in order from +0, the
    group sums are added as ((g0 + g1) + g2) + ..  A group without a term stays +0 and is added all the same."""
    n, dim = terms.shape[-2:]
    lead = terms.shape[:-2]
    acc = np.zeros(lead + (groups, dim), np.float32)
    full = n // groups
    body = terms[..., :full * groups, :].reshape(lead + (full, groups, dim))
    for t in range(full):
        acc = f32_add(acc, body[..., t, :, :])
    rest = n - full * groups
    if rest:
        acc[..., :rest, :] = f32_add(acc[..., :rest, :], terms[..., full * groups:, :])
    total = acc[..., 0, :]
    for g in range(1, groups):
        total = f32_add(total, acc[..., g, :])
    return total


def span_sum(op, x, begin, end, groups):
    """One span of more than 32 entries: a whole row or one chunk."""
    return grouped(products(op, x, begin, end), groups)


def whole_row(op, x, row, groups):
    """The raw sum of a row taken as ONE span: what ``lgc_spmm_rows`` accumulates, and ``lgc_spmm_rows_split`` for a position
    of one chunk."""
    b, e = int(op.rowptr[row]), int(op.rowptr[row + 1])
    if e - b <= SHORT_MAX:
        return sequential(products(op, x, b, e))
    return span_sum(op, x, b, e, groups)


def chunk_bounds(op, row, L):
    """[(begin, end)] of a row's chunks of ``L`` entries."""
    b, e = int(op.rowptr[row]), int(op.rowptr[row + 1])
    return [(b + j * L, min(b + (j + 1) * L, e)) for j in range(-(-(e - b) // L))]


def cut_row(op, x, row, L, groups):
    """(chunk sums fp32 [chunks, dim], their combination fp32 [dim]) of a row of more than ``L`` entries."""
    bounds = chunk_bounds(op, row, L)
    assert len(bounds) > 1
    same = [be for be in bounds if be[1] - be[0] == L]              # every chunk but possibly the last: summed side by side
    sums = np.zeros((len(bounds), x.shape[1]), np.float32)
    if same:
        terms = products(op, x, same[0][0], same[-1][1]).reshape(len(same), L, -1)
        sums[:len(same)] = grouped(terms, groups)
    for j in range(len(same), len(bounds)):
        sums[j] = span_sum(op, x, bounds[j][0], bounds[j][1], groups)
    return sums, grouped(sums, groups)


@functools.lru_cache(maxsize=64)
def table_values(name, dim, which):
    """The clean fp32 values of table ``which`` ("x" or "r") of an operator at a width; read-only."""
    op = operators()[name]
    rng = np.random.default_rng([77, OP_NAMES.index(name), dim, 1 if which == "x" else 2])
    t = T.draw(rng, (op.table_rows, dim))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=64)
def whole_rows(name, dim):
    """fp32 [range rows, dim]: every row of the range as one span (row ``row_begin + i`` at index i); rows of one length
    are summed side by side."""
    op, x, groups = operators()[name], table_values(name, dim, "x"), groups_of(dim)
    out = np.zeros((op.row_end - op.row_begin, dim), np.float32)
    deg = op.lengths
    for n in sorted({int(deg[r]) for r in op.range_rows()}):
        rows = rows_of_length(op, n)
        if n <= SHORT_MAX and n > 0:
            at = np.concatenate([np.arange(op.rowptr[r], op.rowptr[r + 1]) for r in rows])
            terms = np.multiply(op.vals[at, None], x[op.cols[at]], dtype=np.float32).reshape(len(rows), n, dim)
            out[np.array(rows) - op.row_begin] = sequential(terms)
        elif n > 0:
            for r in rows:
                out[r - op.row_begin] = whole_row(op, x, r, groups)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=512)
def cut_rows(name, dim, L):
    """row -> (chunk sums, combination) for every row of the range of more than ``L`` entries."""
    op, x, groups = operators()[name], table_values(name, dim, "x"), groups_of(dim)
    deg = op.lengths
    return {r: cut_row(op, x, r, L, groups) for r in op.range_rows() if deg[r] > L}


@functools.lru_cache(maxsize=512)
def accumulated(name, dim, L):
    """fp32 [range rows, dim]: the raw sum ``lgc_spmm_rows_split`` forms of every row at chunk length ``L`` (``None``: every
    row as one span, ``lgc_spmm_rows``); computed once, a list then costs one indexing step."""
    acc = whole_rows(name, dim)
    if L is None:
        return acc
    acc = acc.copy()
    op = operators()[name]
    for r, (_, combined) in cut_rows(name, dim, L).items():
        acc[r - op.row_begin] = combined
    acc.setflags(write=False)
    return acc


def finished(name, dim, L, rows, epilogue):
    """fp32 [len(rows), dim]: the emulated result rows (range rows only) under an epilogue (a, r given, b)."""
    a, with_r, b = epilogue
    op = operators()[name]
    rows = np.asarray(rows, np.int64)
    r_rows = table_values(name, dim, "r")[rows] if with_r else None
    return T.finish(accumulated(name, dim, L)[rows - op.row_begin], a, r_rows, b)


@functools.lru_cache(maxsize=64)
def fp64_rows(name, dim):
    """(sum val * x[col], sum |val * x[col]|, entries) of every range row in fp64 from the same fp32 inputs."""
    op = operators()[name]
    x = table_values(name, dim, "x").astype(np.float64)
    n_rows = op.row_end - op.row_begin
    val, mag = np.zeros((n_rows, dim)), np.zeros((n_rows, dim))
    for i, row in enumerate(op.range_rows()):
        s, e = int(op.rowptr[row]), int(op.rowptr[row + 1])
        if e > s:
            p = op.vals[s:e, None].astype(np.float64) * x[op.cols[s:e]]
            val[i], mag[i] = p.sum(axis=0), np.abs(p).sum(axis=0)
    return val, mag, op.lengths[op.row_begin:op.row_end].copy()


def evaluate_fp64(name, dim, epilogue):
    """(value, magnitude, entries) of a * sum val * x[col] + b * r[row] for every range row in fp64; magnitude =
    |a| * sum |val * x| + |b * r|."""
    a, with_r, b = epilogue
    op = operators()[name]
    a, b = float(np.float32(a)), float(np.float32(b))
    val, mag, n = fp64_rows(name, dim)
    val, mag = a * val, abs(a) * mag
    if with_r:
        rr = table_values(name, dim, "r").astype(np.float64)[op.row_begin:op.row_end]
        val, mag = val + b * rr, mag + np.abs(b * rr)
    return val, mag, n


# ---------------------------------------------------------------------------------------------------------------------
# what a call leaves behind: y, work, partials as int32 bit patterns
# ---------------------------------------------------------------------------------------------------------------------
GUARD_ROWS = 4          # rows beyond y_rows and beyond partial_rows, ints beyond work[n_ids + 1]: never written


def strides_of(layout, dim):
    """(x_stride, y_stride, r_stride) in floats."""
    if layout == "dense":
        return dim, dim, dim
    up = -(-dim // 4) * 4
    if layout == "padded":                  # all different, rows 16-byte aligned from 4 columns up
        return up + 4, up + 8, up + 12
    if layout == "odd":                     # y and r rows that start at any dword: strides that are odd numbers
        odd = dim + 1 if dim % 2 == 0 else dim + 2
        return up + 4, odd, odd + 2
    raise ValueError(layout)


def input_table(name, dim, which, stride, keep=None):
    """fp32 [table_rows, stride]: the clean values in the first ``dim`` columns (of the rows ``keep`` only, if given), NaN
    everywhere else -- padding columns and rows that must not be read."""
    t = np.full((operators()[name].table_rows, stride), np.nan, np.float32)
    clean = table_values(name, dim, which)
    if keep is None:
        t[:, :dim] = clean
    elif len(keep):
        keep = np.asarray(keep, np.int64)
        t[keep, :dim] = clean[keep]
    return t


def listed_range_rows(rl):
    """The ids of a list that lie in the operator's range, in list order (repeats kept)."""
    op = operators()[rl.op]
    return rl.ids[~is_foreign(op, rl.ids)]


def expected_y(rl, dim, y_stride, L, epilogue, compact=False):
    """int32 [y rows + guard, y_stride]: the emulation's bits in the ``dim`` columns of the written rows -- row ids, or list
    positions if ``compact`` --, the sentinel everywhere else."""
    op = operators()[rl.op]
    y_rows = rl.n_ids if compact else op.table_rows
    y = np.full((y_rows + GUARD_ROWS, y_stride), SENTINEL, np.int32)
    inside = np.flatnonzero(~is_foreign(op, rl.ids))
    if inside.size:
        rows = rl.ids[inside]
        y[inside if compact else rows, :dim] = T.bits(finished(rl.op, dim, L, rows, epilogue))
    return y


@functools.lru_cache(maxsize=None)
def _expected_partials(list_name, dim, partial_rows):
    rl = lists()[list_name]
    op = operators()[rl.op]
    work = plan(op, rl.ids, partial_rows)
    n, L = rl.n_ids, int(work[-1])
    total = int(work[n])
    assert total <= partial_rows
    own = owners(work, n)
    cuts = cut_rows(rl.op, dim, L)
    slots, rows = [], []
    for w in range(total):
        m = int(own[w])
        if work[m + 1] - work[m] > 1:
            slots.append(w)
            rows.append(cuts[int(rl.ids[m])][0][w - int(work[m])])
    counts = np.diff(work[:n + 1])
    assert len(slots) == counts[counts > 1].sum()           # by chunk number and by position: the same slots
    want = T.bits(np.array(rows, np.float32).reshape(len(rows), dim))
    return np.array(slots, np.int64), want, total


def expected_partials(rl, dim, partial_rows):
    """(slots int64 [k], int32 [k, dim], chunk count): the emulated raw chunk sums of the slots that belong to positions
    cut into several chunks, found chunk number by chunk number through ``owners``.  Every slot from the chunk count on
    keeps the sentinel; a slot below it whose position has one chunk is never read and not pinned."""
    return _expected_partials(rl.name, dim, partial_rows)


def expected_work(rl, partial_rows):
    """int32 [n_ids + 2 + guard]"""
    work = plan(operators()[rl.op], rl.ids, partial_rows)
    return np.concatenate([work, np.full(GUARD_ROWS, SENTINEL, np.int64)]).astype(np.int32)
