"""Small named operators, numpy references and the case table for the tests of the tiled short-row hop
(tests/test_tiles_host.py, tests/test_tiles_gpu.py).

The tile path: rows of at most 32 entries are sorted into width classes 8 / 16 / 32 (``graph.plan_tile_classes``,
``lgc_tile_classes`` + ``lgc_tile_pack``), laid out in 1 KiB pieces (``lgc_build_tiles``) and summed by one of three
kernel bodies (``tiles_body``, ``tiles_body_dpp``, ``tiles_body_dpp_wide``), launched on their own (``lgc_spmm_tiles``)
or inside ``k_apply_fused`` (``Operator.apply``).

Every operator here is a CSR over ``table_rows`` rows (rowptr int64 on the host, int32 columns, fp32 values), a row range
``[row_begin, row_end)`` and nothing else; each exists for one property, which test_tiles_host.py asserts.  Values and
table entries are drawn from sign x [2^-6, 2^6): no product and no partial sum is subnormal (a product is at least 2^-12 in
magnitude, a partial sum is zero or at least one ulp of that), so no flush-to-zero mode can make a comparison ambiguous.

The references are numpy only and written from the contract the kernels state, not from tests/cpu_ops.py or the oracle:

    acc = +0.0f;  for the row's entries in stored order  acc = fl(acc + fl(val * x[col]))
    acc = fl(a * acc)                 if a != 1
    acc = fl(acc + fl(b * r[row]))    if r is given

once in fp32, operation by operation (``emulate``), once in fp64 (``evaluate_fp64``).
"""
import functools
from dataclasses import dataclass

import numpy as np

WIDTHS = (8, 16, 32)
SHORT_MAX, CHUNK_LEN = 32, 256
SENTINEL = np.int32(0x4B1D4B1D)             # what y holds before a call: any float outside the owned rows keeps it

# (a, r given, b)
EPILOGUES = ((1.0, False, 0.0), (0.75, True, 0.3), (1.0, True, 1.0), (0.0, True, -2.0), (-1.0, False, 0.0))
# generic body: rows per batch 64 / lpr = 64, 32, 32, 32, 21, 12, 5, 4, 3, 3, 1, 1, 1 -- above R, not dividing R, 3, 1
GENERIC_DIMS = (4, 5, 7, 8, 12, 20, 44, 60, 65, 67, 129, 200, 256)
DPP_DIMS = (61, 62, 63, 64)
# two DPP rows per table row: the second holds 1 lane, 2 overlapping lanes, 2, 4, 7 (overlapping), 8, 9 (overlapping), 16
# (overlapping), 16 lanes
WIDE_DIMS = (68, 69, 71, 80, 90, 96, 97, 127, 128)
LAYOUTS = ("dense", "pad4", "pad12", "view")
BODIES = ("generic", "dpp", "dpp_wide")
ONE_DIM_OF = {"generic": 20, "dpp": 63, "dpp_wide": 90}
TILES_PER_WAVE = (1, 2, 3, 4)
MANY_TILES = (1, 2, 3, 4, 5, 9)
ORDERS = ("cold", "natural")
MAX_LENS = (32, 20, 5)


def geometry(width):
    """(L loads per lane, R rows per tile, Wk entries of a row in one load, PPR 16-byte pieces of a row in one load,
    B batches of four rows)"""
    L = 2 if width == 32 else 1
    R = 128 * L // width
    return L, R, width // L, width // L // 2, R // 4


def draw(rng, shape):
    """fp32 values of sign x [2^-6, 2^6): a 24-bit significand in [1, 2), an exponent in -6 .. 5."""
    mant = 1.0 + rng.integers(0, 1 << 23, size=shape) / float(1 << 23)
    expo = rng.integers(-6, 6, size=shape)
    sign = 1.0 - 2.0 * rng.integers(0, 2, size=shape)
    out = (sign * np.ldexp(mant, expo)).astype(np.float32)
    assert np.all(np.abs(out) >= 2.0 ** -6) and np.all(np.abs(out) < 2.0 ** 6)
    return out


@dataclass(frozen=True, eq=False)
class TileOp:
    name: str
    rowptr: np.ndarray          # int64 [table_rows + 1]
    cols: np.ndarray            # int32 [E]
    vals: np.ndarray            # float32 [E]
    row_begin: int
    row_end: int
    table_rows: int
    forced: tuple = ()          # ((width, (row ids)), ...): classes placed by hand (pack_by_hand), not by the planner
    unread: tuple = ()          # table rows no entry may name

    @property
    def lengths(self):
        return np.diff(self.rowptr)

    def row(self, i):
        b, e = int(self.rowptr[i]), int(self.rowptr[i + 1])
        return self.cols[b:e], self.vals[b:e]

    def range_rows(self):
        return range(self.row_begin, self.row_end)


def _build(name, seed, lengths, table_rows, row_begin=0, pick=None, before=(), after=(), **kw):
    """Rows [row_begin, row_begin + len(lengths)) get ``lengths``; ``before`` / ``after`` are the lengths of the rows
    outside the range (missing ones are empty); ``pick(rng, n, row)`` draws the columns of a row."""
    rng = np.random.default_rng([20261020, seed])
    row_end = row_begin + len(lengths)
    assert len(before) <= row_begin and row_end + len(after) <= table_rows
    full = np.zeros(table_rows, np.int64)
    full[:len(before)] = before
    full[row_begin:row_end] = lengths
    full[row_end:row_end + len(after)] = after
    rowptr = np.concatenate([[0], np.cumsum(full)]).astype(np.int64)
    pick = pick or (lambda rng, n, row: rng.integers(0, table_rows, size=n))
    cols = [np.asarray(pick(rng, int(n), i), np.int64) for i, n in enumerate(full)]
    cols = np.concatenate(cols).astype(np.int32) if rowptr[-1] else np.zeros(0, np.int32)
    assert cols.size == rowptr[-1] and (cols.size == 0 or (cols.min() >= 0 and cols.max() < table_rows))
    return TileOp(name, rowptr, cols, draw(rng, cols.size), row_begin, row_end, table_rows, **kw)


def _shuffled(seed, values):
    values = np.array(values, np.int64)
    np.random.default_rng([7, seed]).shuffle(values)
    return values


EXACT_8 = list(range(1, 9)) * 2                          # 16 rows of 1 .. 8 entries
EXACT_16 = list(range(9, 17))                            # 8 rows of 9 .. 16
EXACT_32 = [17, 19, 22, 24, 26, 29, 31, 32]              # 8 rows of 17 .. 32
EDGE_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 20, 21, 24, 25, 28, 29, 31, 32]
LONG_LENGTHS = [33, 64, 300]                             # one chunk, one chunk, two chunks at chunk_len = 256
ITEM_HALF_BEGIN = 21
UNREAD = (0, 20, 39)                                     # of 40 table rows


def _lopsided():
    """Per class two tiles whose batch 0 holds (W, 1, 1, 1) and whose other rows have at most one entry: meta byte 0 is W
    while three of its four rows end after one entry.  Rows of one entry cannot reach the classes 16 and 32 through the
    planner (a row goes to the narrowest class that holds it), so these classes are placed by hand."""
    lengths, forced = [], []
    for w in WIDTHS:
        r = geometry(w)[1]
        first = [1, 0, w, 0, 1, 0, 1] + [0] * (r - 7)
        second = [1, 1, 0, 1, w, 1, 1, 1] + [0] * (r - 8)
        rows = tuple(range(len(lengths), len(lengths) + 2 * r))
        lengths += first + second
        forced.append((w, rows))
    return lengths, tuple(forced)


def _many_tiles(n):
    """n tiles in every class, the last one of each partly filled."""
    l8 = [i % 9 for i in range(16 * (n - 1) + 5)]
    l16 = [9 + i % 8 for i in range(8 * (n - 1) + 3)]
    l32 = [17 + (5 * i) % 16 for i in range(8 * (n - 1) + 2)]
    return l8 + l16 + l32


@functools.lru_cache(maxsize=None)
def operators():
    """name -> TileOp, in the order of the case table."""
    ops = []
    ops.append(_build("one_row", 1, [1], 6))
    ops.append(_build("all_empty", 2, [0] * 20, 24))
    ops.append(_build("exact_tiles", 3, _shuffled(3, EXACT_8 + EXACT_16 + EXACT_32), 40))
    ops.append(_build("one_over", 4, _shuffled(4, EXACT_8 + EXACT_16 + EXACT_32 + [5, 12, 20]), 40))
    ops.append(_build("only_wide", 5, [17, 18, 20, 23, 25, 27, 30, 31, 32, 32, 17], 30))
    ops.append(_build("length_edges", 6, _shuffled(6, EDGE_LENGTHS * 2 + LONG_LENGTHS), 48))
    lengths, forced = _lopsided()
    ops.append(_build("lopsided_batches", 7, lengths, len(lengths) + 3, forced=forced))
    nb = ITEM_HALF_BEGIN
    ops.append(_build("item_half", 8, [3, 0, 8, 9, 16, 17, 32, 1, 12, 25, 5, 2, 30], nb + 13 + 5, row_begin=nb,
                      before=[2, 5, 0, 9, 1, 20, 3] * 3, after=[4, 11, 0, 18, 2],
                      pick=lambda rng, n, row: rng.integers(0, nb, size=n) if row >= nb else rng.integers(nb, nb + 18, size=n)))
    ops.append(_build("edge_columns", 9, [1, 2, 8, 9, 16, 17, 32, 4, 0, 13, 24], 30,
                      pick=lambda rng, n, row: rng.choice([0, 29], size=n)))
    allowed = np.array([c for c in range(40) if c not in UNREAD])
    ops.append(_build("unread_rows", 10, [6, 0, 8, 11, 16, 19, 32, 2, 14, 27, 1, 3], 40, unread=UNREAD,
                      pick=lambda rng, n, row: rng.choice(allowed, size=n)))
    for n in MANY_TILES:
        lengths = _many_tiles(n)
        ops.append(_build(f"many_tiles_{n}", 20 + n, lengths, len(lengths) + 7))
    return {op.name: op for op in ops}


NAMES = ("one_row", "all_empty", "exact_tiles", "one_over", "only_wide", "length_edges", "lopsided_batches", "item_half",
         "edge_columns", "unread_rows") + tuple(f"many_tiles_{n}" for n in MANY_TILES)


def op_index(name):
    return NAMES.index(name)


# ---------------------------------------------------------------------------------------------------------------------
# planner and slab
# ---------------------------------------------------------------------------------------------------------------------
def planned_classes(op, mode="cold", max_len=SHORT_MAX):
    """``graph.plan_tile_classes`` on CPU tensors: [(width, order int32, meta int32)] as numpy arrays."""
    import torch
    from gnn_ecommerce_amd import graph as G
    plan = G.plan_tile_classes(torch.from_numpy(op.rowptr.astype(np.int32)), torch.from_numpy(op.cols), op.row_begin,
                               op.row_end, max_len, mode)
    return [(w, o.numpy().copy(), m.numpy().copy()) for w, o, m in plan]


def pack_by_hand(op, width, rows):
    """(order, meta) of the given rows as ONE class of ``width``, tile by tile in list order: the rule of
    ``plan_tile_classes`` restated -- inside a tile longest first (stable), rank rho in slot (rho % 4) * B + rho // 4,
    meta byte bt = the longest of ranks 4 bt .. 4 bt + 3."""
    _, R, _, _, B = geometry(width)
    deg = op.lengths
    assert all(deg[r] <= width for r in rows)
    rows = list(rows) + [-1] * (-len(rows) % R)
    order, meta = [], []
    for t in range(len(rows) // R):
        tile = rows[t * R:(t + 1) * R]
        d = [int(deg[r]) if r >= 0 else -1 for r in tile]
        rank = sorted(range(R), key=lambda i: -d[i])               # sorted() is stable
        placed, m = [-1] * R, 0
        for rho, i in enumerate(rank):
            placed[(rho % 4) * B + rho // 4] = tile[i]
        for bt in range(B):
            m |= max(max(d[i] for i in rank[4 * bt:4 * bt + 4]), 0) << (8 * bt)
        order += placed
        meta.append(m)
    return np.array(order, np.int32), np.array(meta, np.int32)


@functools.lru_cache(maxsize=None)
def _kernel_classes(name):
    op = operators()[name]
    if op.forced:
        return tuple((w,) + pack_by_hand(op, w, rows) for w, rows in op.forced)
    return tuple(planned_classes(op))


def kernel_classes(op):
    """The classes the direct kernel tests run: the planner's ("cold", max_len 32), or the hand-placed ones."""
    return _kernel_classes(op.name)


def owned_rows(order):
    return np.sort(order[order >= 0]).astype(np.int64)


def slab_reference(op, width, order):
    """The slab of ``lgc_build_tiles`` as int32 [slots * width, 2] = (column, fp32 bits): 16-byte piece
    ((t*L + k)*R + s)*PPR + q holds entries k*Wk + 2q and k*Wk + 2q + 1 of the row in slot s of tile t; an entry the row
    does not have, and every entry of a padding slot, is (-1, 0.0f)."""
    L, R, Wk, PPR, _ = geometry(width)
    assert order.size % R == 0
    n_tiles = order.size // R
    slab = np.zeros((n_tiles * R * width, 2), np.int32)
    slab[:, 0] = -1
    bits = op.vals.view(np.int32)
    for t in range(n_tiles):
        for s in range(R):
            row = int(order[t * R + s])
            if row < 0:
                continue
            b, e = int(op.rowptr[row]), int(op.rowptr[row + 1])
            for k in range(L):
                for q in range(PPR):
                    piece = ((t * L + k) * R + s) * PPR + q
                    for h in range(2):
                        j = k * Wk + 2 * q + h
                        if b + j < e:
                            slab[2 * piece + h] = (op.cols[b + j], bits[b + j])
    return slab


def padding_slots(order):
    return int((order < 0).sum())


def meta_bytes(meta, width):
    """int [n_tiles, B]"""
    B = geometry(width)[4]
    return np.stack([(meta.astype(np.int64) >> (8 * bt)) & 0xFF for bt in range(B)], axis=1)


def chunk_rows(op):
    """Rows of the range that go to the chunk plan at short_max = 32: (row, chunks at chunk_len = 256)."""
    deg = op.lengths
    return [(r, -(-int(deg[r]) // CHUNK_LEN)) for r in op.range_rows() if deg[r] > SHORT_MAX]


def tiled_rows(op):
    deg = op.lengths
    return np.array([r for r in op.range_rows() if deg[r] <= SHORT_MAX], np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def accumulate(op, x, rows):
    """fp32 [len(rows), dim]: acc = +0, then acc = fl(acc + fl(val * x[col])) entry by entry in stored order.  Every
    numpy operation below takes fp32 operands and returns the correctly rounded fp32 result of ONE operation per
    element; nothing is fused."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    out = np.zeros((len(rows), x.shape[1]), np.float32)
    for i, row in enumerate(rows):
        cols, vals = op.row(int(row))
        acc = out[i]
        for c, v in zip(cols, vals):
            prod = np.multiply(np.float32(v), x[c], dtype=np.float32)
            acc = np.add(acc, prod, dtype=np.float32)
        out[i] = acc
    return out


def finish(acc, a, r_rows, b):
    """The epilogue on accumulated rows; ``r_rows`` = r[rows] or None."""
    acc = np.asarray(acc, np.float32)
    if np.float32(a) != np.float32(1.0):
        acc = np.multiply(np.float32(a), acc, dtype=np.float32)
    if r_rows is not None:
        acc = np.add(acc, np.multiply(np.float32(b), r_rows, dtype=np.float32), dtype=np.float32)
    return acc


def emulate(op, x, rows, a=1.0, r=None, b=0.0):
    return finish(accumulate(op, x, rows), a, None if r is None else np.asarray(r, np.float32)[rows], b)


def evaluate_fp64(op, x, rows, a=1.0, r=None, b=0.0):
    """(value, magnitude, entries) of the same expression in fp64 from the same fp32 inputs:
    value = a * sum val*x + b*r, magnitude = |a| * sum |val*x| + |b*r|, entries = n per row."""
    x = np.asarray(x, np.float64)
    a, b = float(np.float32(a)), float(np.float32(b))
    val = np.zeros((len(rows), x.shape[1]))
    mag = np.zeros_like(val)
    n = np.zeros(len(rows), np.int64)
    for i, row in enumerate(rows):
        cols, vals = op.row(int(row))
        for c, v in zip(cols, vals):
            val[i] += float(v) * x[c]
            mag[i] += np.abs(float(v) * x[c])
        n[i] = len(cols)
    val, mag = a * val, abs(a) * mag
    if r is not None:
        rr = np.asarray(r, np.float64)[rows]
        val, mag = val + b * rr, mag + np.abs(b * rr)
    return val, mag, n


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# tables: x gathered, r the epilogue row, y written -- as arenas with everything that must stay unread / unwritten marked
# ---------------------------------------------------------------------------------------------------------------------
def layout_of(layout, dim):
    """(row stride, floats before the first row, floats after the last row's padding) of a table of ``dim`` columns."""
    if layout == "dense":
        return dim, 0, 0
    if layout == "pad4":
        return dim + 4, 0, 0
    if layout == "pad12":
        return dim + 12, 0, 0
    if layout == "view":                     # a view that starts inside a larger allocation
        stride = dim + 4
        return stride, 3 * stride + 4, 2 * stride + 3
    raise ValueError(layout)


@functools.lru_cache(maxsize=256)
def table_values(name, dim, which):
    """The clean fp32 values of table ``which`` ("x" or "r") of an operator at a width; read-only."""
    op = operators()[name]
    rng = np.random.default_rng([99, op_index(name), dim, 1 if which == "x" else 2])
    t = draw(rng, (op.table_rows, dim))
    t.setflags(write=False)
    return t


def table_view(a, op, dim, layout):
    """The writable [table_rows, dim] table inside an arena."""
    stride, lead, _ = layout_of(layout, dim)
    return a[lead:lead + op.table_rows * stride].reshape(op.table_rows, stride)[:, :dim]


def arena(op, dim, layout, fill):
    """(arena float32 1-D, its [table_rows, dim] view, stride, lead)"""
    stride, lead, tail = layout_of(layout, dim)
    a = np.full(lead + op.table_rows * stride + tail, fill, np.float32)
    return a, table_view(a, op, dim, layout), stride, lead


def named_columns(op, rows):
    named = [op.row(int(r))[0] for r in rows]
    return np.unique(np.concatenate(named)) if named else np.zeros(0, np.int32)


def input_arena(op, dim, layout, which, rows):
    """The arena of x (only the table rows an entry of ``rows`` names hold values) or r (only ``rows`` do): every other
    float -- padding columns, other rows, the allocation around a view -- is NaN and must not be read."""
    a, view, stride, lead = arena(op, dim, layout, np.nan)
    keep = named_columns(op, rows) if which == "x" else np.asarray(rows, np.int64)
    if len(keep):
        view[keep] = table_values(op.name, dim, which)[keep]
    return a, stride, lead


def output_arena(op, dim, layout):
    """y before a call, as int32: the sentinel everywhere."""
    stride, lead, tail = layout_of(layout, dim)
    return np.full(lead + op.table_rows * stride + tail, SENTINEL, np.int32), stride, lead


def expected_output(op, dim, layout, rows, want):
    """y after a call, as int32: ``want`` (fp32 [len(rows), dim]) in the rows' ``dim`` columns, the sentinel elsewhere."""
    a, stride, lead = output_arena(op, dim, layout)
    view = a[lead:lead + op.table_rows * stride].reshape(op.table_rows, stride)[:, :dim]
    if len(rows):
        view[np.asarray(rows, np.int64)] = bits(want)
    return a


@functools.lru_cache(maxsize=512)
def _accumulated(name, dim):
    op = operators()[name]
    rows = tiled_rows(op)
    acc = accumulate(op, table_values(name, dim, "x"), rows)
    acc.setflags(write=False)
    return rows, acc


def wanted(op, dim, rows, epilogue):
    """The emulation on ``rows`` (tiled rows of the range) with the operator's clean tables; the running sums are computed
    once per (operator, width) and shared by the epilogues."""
    a, with_r, b = epilogue
    all_rows, acc = _accumulated(op.name, dim)
    at = np.searchsorted(all_rows, rows)
    assert np.array_equal(all_rows[at], rows)
    r_rows = table_values(op.name, dim, "r")[np.asarray(rows, np.int64)] if with_r else None
    return finish(acc[at], a, r_rows, b)


# ---------------------------------------------------------------------------------------------------------------------
# the route rule and the case table of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def fast_ok(dim, table_rows, strides):
    """``tiles_fast_ok`` restated: the DPP bodies run at 61..64 and 68..128 columns when row ids fit 24 bits, byte offsets
    32 bits, and the padding id 0xFFFFFF lands beyond every table (the 32-bit product wraps)."""
    def pad_is_oob(stride):
        nbytes = ((table_rows - 1) * stride + dim) * 4
        pad = (0xFFFFFF * stride * 4) & 0xFFFFFFFF
        return stride * 4 < (1 << 24) and nbytes < (1 << 32) and pad >= nbytes
    return (61 <= dim <= 64 or 68 <= dim <= 128) and 0 < table_rows < 0xFFFFFF and all(pad_is_oob(s) for s in strides)


def body_of(dim, table_rows, stride, has_meta=True):
    """Which kernel body ``lgc_spmm_tiles`` (and the fused launch) runs."""
    if has_meta and fast_ok(dim, table_rows, (stride,)):
        return "dpp_wide" if dim > 64 else "dpp"
    return "generic"


def route_of(dim, table_rows, stride):
    """``Operator.route`` of a tiled operator on tables this small (write-through stores: every offset fits 32 bits)."""
    return ("fused_dpp" if body_of(dim, table_rows, stride) != "generic" else "fused_generic") + "+wt"


@dataclass(frozen=True)
class Case:
    group: str          # "widths", "layouts", "stretch"
    op: str
    dim: int
    meta: bool          # False: meta = NULL, the generic body at a DPP width
    tiles_per_wave: int
    layout: str

    def body(self):
        op = operators()[self.op]
        return body_of(self.dim, op.table_rows, layout_of(self.layout, self.dim)[0], self.meta)


WIDTH_SETS = {"generic": GENERIC_DIMS, "dpp": DPP_DIMS, "dpp_wide": WIDE_DIMS, "generic_no_meta": DPP_DIMS + WIDE_DIMS}
STRETCH_OTHER = "one_over"                  # two tiles per class: beside many_tiles, the other operator of the stretch cases


@functools.lru_cache(maxsize=None)
def cases():
    """Every direct ``lgc_spmm_tiles`` case of test_tiles_gpu.py; each runs every class of its operator with every
    epilogue.  "widths": every operator at every width of every body (layouts in rotation); "layouts": every operator at
    one width per body in every layout; "stretch": many_tiles and one other operator at tiles_per_wave 1 .. 4."""
    out = []
    for name in NAMES:
        for kind, dims in WIDTH_SETS.items():
            for i, dim in enumerate(dims):
                out.append(Case("widths", name, dim, kind != "generic_no_meta", 1, LAYOUTS[(i + op_index(name)) % len(LAYOUTS)]))
        for body in BODIES:
            for layout in LAYOUTS:
                out.append(Case("layouts", name, ONE_DIM_OF[body], True, 1, layout))
    for name in tuple(f"many_tiles_{n}" for n in MANY_TILES) + (STRETCH_OTHER,):
        for dim, meta in ((20, True), (67, True), (63, True), (90, True), (128, True), (64, False), (96, False)):
            for tpw in TILES_PER_WAVE:
                out.append(Case("stretch", name, dim, meta, tpw, "pad4" if tpw % 2 else "dense"))
    return tuple(out)


def cases_of(group, name, **where):
    return [c for c in cases() if c.group == group and c.op == name and all(getattr(c, k) == v for k, v in where.items())]
