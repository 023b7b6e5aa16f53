"""Band sweep on small degenerate operators: named cases, planner configurations, an fp64 reference and its bound.

Shared by tests/test_sweep_host.py (host planner, no GPU), tests/test_sweep_gpu.py (device planner, k_sweep,
k_sweep_wide, k_sweep_combine, lgc_spmm_sweep) and tests/route_child.py (the sweep cut into several launches).

An operator is a CSR slice (rowptr, entries, row_begin, row_end, col_lo, col_hi, table_rows) inside a larger CSR: the
rows before ``row_begin`` and after ``row_end`` hold entries of their own, with columns anywhere in the table, so a
planner or kernel that looks outside its slice reads something.  Values lie in (0.01, 1), from a fixed numpy seed.

The bound is derived, not measured.  For a row of L entries the kernels compute fl(a * acc) + fl(b * r) with acc the
sum, in some order over slots and the combine, of L products rounded once each:
  * every product carries one rounding, and every path from a product to the row's sum at most L - 1 additions
    (adding the +0 an accumulator starts from is exact): |acc - sum| <= ((1 + u)^L - 1) * S, S = sum_k |v_k x[c_k]|;
  * finish_row rounds a * acc, b * r and their sum: three more roundings, of which two act on the a-part and two on
    the b-part;
so per element |got - want| <= 1.01 * u * ((L + 2) * |a| * S + 2 * |b * r|) with u = 2^-24; the factor 1.01 covers the
second-order terms (L * u <= 1e-4 for the rows here).  The project's norm-wise gates (rel_fro, worst_row_rel <= 1e-5)
are checked in addition, over the rows that have entries.
"""
from typing import NamedTuple

import numpy as np
import torch

from conftest import rel_fro, worst_row_rel

PAD_COL = 0xFFFFFF
WIDE_SLOTS = 32                    # SweepPlan.WIDE_SLOTS: rows with more slots get a workgroup of k_sweep_combine
SENTINEL = 0x7FA5A5A5              # a NaN bit pattern no kernel produces
TOL = 1e-5
U = 2.0 ** -24
A, B = 0.75, 0.25                  # exact in fp32

NARROW = (61, 62, 63, 64)                          # k_sweep, one pass
WIDE = (68, 69, 70, 71, 72, 90, 95, 96)            # k_sweep_wide
TWO_PASS = (97, 98, 99, 100, 125, 127, 128)        # k_sweep twice: columns [0, 64) and [64, dim)
ROUTE_OF = {**{d: "sweep" for d in NARROW}, **{d: "sweep_wide" for d in WIDE}, **{d: "sweep_two_pass" for d in TWO_PASS}}
STRIDE_PAD = 3                     # the strided runs: rows of dim + 3 floats (not 16-byte aligned)


class Case(NamedTuple):
    name: str
    rowptr: torch.Tensor           # int32 [table_rows + 1]
    entries: torch.Tensor          # int32 [E, 2]: column, fp32 bits of the value
    row_begin: int
    row_end: int
    col_lo: int
    col_hi: int
    table_rows: int


def _embed(name, seed, rows, col_lo, n_cols, row_begin):
    """``rows``: per row of the slice an array of columns relative to col_lo.  Rows outside the slice get 0..3 entries
    with columns anywhere in the table."""
    rng = np.random.default_rng(seed)
    n_rows = len(rows)
    row_end, col_hi = row_begin + n_rows, col_lo + n_cols
    table_rows = max(row_end, col_hi) + 6
    cols = [rng.integers(0, table_rows, size=(i * 7 + 1) % 4) for i in range(row_begin)]
    cols += [np.asarray(r, dtype=np.int64) + col_lo for r in rows]
    cols += [rng.integers(0, table_rows, size=(i * 5 + 2) % 4) for i in range(row_end, table_rows)]
    lens = np.array([len(c) for c in cols], dtype=np.int64)
    flat = np.concatenate(cols).astype(np.int32) if lens.sum() else np.zeros(0, dtype=np.int32)
    vals = rng.uniform(0.01, 1.0, size=flat.size).astype(np.float32)
    assert ((vals > np.float32(0.01)) & (vals < 1)).all()
    rowptr = np.zeros(table_rows + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(lens)
    entries = np.stack([flat, vals.view(np.int32)], axis=1)
    inside = flat[rowptr[row_begin]:rowptr[row_end]]
    assert ((inside >= col_lo) & (inside < col_hi)).all()
    return Case(name, torch.from_numpy(rowptr), torch.from_numpy(np.ascontiguousarray(entries)), row_begin, row_end, col_lo,
                col_hi, table_rows)


def _hub_and_empties():
    rng = np.random.default_rng(101)
    lens = rng.integers(0, 60, size=41)
    lens[0], lens[7] = 1500, 700
    lens[[3, 11, 12, 30, 40]] = 0                     # two neighbours and the last row of the range among them
    return _embed("hub_and_empties", 1, [rng.integers(0, 2000, size=n) for n in lens], 5, 2000, 2010)


def _one_column():
    return _embed("one_column", 2, [np.zeros(n, dtype=np.int64) for n in (0, 1, 2, 3, 40, 0, 33, 5, 64)], 0, 1, 4)


def _few_columns():
    rng = np.random.default_rng(103)
    return _embed("few_columns", 3, [rng.integers(0, 5, size=n) for n in (0, 40, 7, 1, 23, 12)], 9, 5, 3)


def _single_row():
    rng = np.random.default_rng(104)
    return _embed("single_row", 4, [rng.choice(900, size=300, replace=False)], 13, 900, 920)


def _unit_rows(n_unit):
    rng = np.random.default_rng(105 + n_unit)
    lens = rng.permutation(np.array([1] * n_unit + [0] * 3 + [2] * 8))
    return _embed(f"unit_rows_{n_unit}", 5, [rng.choice(4000, size=n, replace=False) for n in lens], 60, 4000, 20)


def _sub_range():
    rng = np.random.default_rng(107)
    lens = rng.integers(0, 90, size=60)
    return _embed("sub_range", 7, [rng.choice(500, size=n, replace=False) for n in lens], 1717, 500, 11)


def _empty():
    return _embed("empty", 8, [np.zeros(0, dtype=np.int64)] * 3, 2, 10, 1)


_BUILDERS = {"hub_and_empties": _hub_and_empties, "one_column": _one_column, "few_columns": _few_columns,
             "single_row": _single_row, "unit_rows_620": lambda: _unit_rows(620), "unit_rows_410": lambda: _unit_rows(410),
             "sub_range": _sub_range, "empty": _empty}
OPERATORS = tuple(_BUILDERS)
_cases = {}


def case(name) -> Case:
    """The named operator, built once (host tensors; nobody writes to them)."""
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]


def _cfg(**kw):
    return {**dict(n_bands=8, waves_per_band_round=4, row_cap=78, piece_cap=64, lookahead=64, groups=4, round_order=2), **kw}


# lookahead <= 64 and piece_cap <= 64 everywhere: the device planner takes every one of them
CONFIGS = {
    "g4_prod": _cfg(),
    "g4_lds_cap": _cfg(n_bands=1, row_cap=159),                    # 4 wavefronts x 160 rows x 256 B = 160 KiB
    "g4_cap1": _cfg(n_bands=2, row_cap=1, piece_cap=1, lookahead=4),
    "g4_small": _cfg(n_bands=3, row_cap=5, piece_cap=4, lookahead=4),
    "g2_prod": _cfg(row_cap=51, groups=2),
    "g2_lds_cap": _cfg(n_bands=1, row_cap=105, groups=2),          # 4 x 106 x 384 B = 159 KiB; 106 would not fit
    "g2_small": _cfg(n_bands=2, waves_per_band_round=8, row_cap=3, piece_cap=2, groups=2),
}
for _name in ("g4_small", "g2_small"):
    for _order in (0, 1):
        CONFIGS[f"{_name}_order{_order}"] = dict(CONFIGS[_name], round_order=_order)
PAIRS = [(o, c) for o in OPERATORS for c in CONFIGS]


def widths_of(cfg):
    return WIDE if cfg["groups"] == 2 else NARROW + TWO_PASS


# ----------------------------------------------------------------------------------------------
# plans
def decode_sweep(dims, arr, row_cap):
    """slot -> [(col, value bits)] in list order, checking the step invariants on the way."""
    groups = dims["groups"]
    slabs = arr["slabs"].numpy().view(np.uint32).reshape(-1, 16 * groups, 4)
    wsp, wnp = arr["wave_slab_ptr"].numpy(), arr["wave_npieces"].numpy()
    ps = arr["piece_slot"].numpy().reshape(-1, row_cap)
    out = {}
    for w in range(dims["n_waves"]):
        assert 0 <= wnp[w] <= row_cap
        for sb in range(wsp[w], wsp[w + 1]):
            for s in range(32):
                used = set()
                for grp in range(groups):
                    x, v = int(slabs[sb, 16 * grp + (s >> 1), 2 * (s & 1)]), int(slabs[sb, 16 * grp + (s >> 1), 2 * (s & 1) + 1])
                    col, pc = x & 0xFFFFFF, x >> 24
                    if col == 0xFFFFFF:                                  # padding: dummy accumulator, value 0
                        assert pc == row_cap and v == 0
                        continue
                    assert pc < wnp[w] and pc not in used                 # no two entries of a step share a piece
                    used.add(pc)
                    out.setdefault(int(ps[w, pc]), []).append((col, v))
    return out


def assert_same_plan(dims, arr, want_dims, want, what=""):
    """Two plans array by array, bit for bit.  Buffers of an empty plan still hold one element, and the piece_slot
    entries beyond a wavefront's piece count are unspecified: both are left out."""
    assert dims == want_dims, (what, dims, want_dims)
    for k in ("slabs", "wave_slab_ptr", "wave_npieces", "piece_slot", "multi"):
        a, b = arr[k].cpu(), want[k].cpu()
        if k == "slabs":
            a, b = a[: dims["n_slabs"] * 64 * dims["groups"]], b[: dims["n_slabs"] * 64 * dims["groups"]]
        if k == "wave_npieces":
            a, b = a[: dims["n_waves"]], b[: dims["n_waves"]]
        if k == "piece_slot":
            npc = want["wave_npieces"].cpu()[: dims["n_waves"]].long()
            live = torch.arange(dims["row_cap"]).view(1, -1) < npc.view(-1, 1)
            n = dims["n_waves"] * dims["row_cap"]
            a, b = a[:n].view(-1, dims["row_cap"])[live], b[:n].view(-1, dims["row_cap"])[live]
        assert torch.equal(a, b), (what, k)


def assert_preconditions(op_name, cfg_name, cfg, dims, arr):
    """What each named case is there for, so that a planner change cannot quietly empty it.  ``arr``: host arrays of
    the plan (wave_npieces, multi)."""
    c = case(op_name)
    npieces = arr["wave_npieces"].cpu().numpy()[: dims["n_waves"]]
    multi = arr["multi"].cpu().numpy()
    slots = multi[:, 2] - multi[:, 1]
    ne = int(c.rowptr[c.row_end] - c.rowptr[c.row_begin])
    base = cfg_name.split("_order")[0]
    assert npieces.sum() == dims["n_slots"] == slots.sum()
    if op_name == "hub_and_empties" and base in ("g4_small", "g4_cap1", "g2_small"):
        assert (slots > WIDE_SLOTS).any(), "no row for the workgroup-per-row branch of the combine"
        deg = (c.rowptr[c.row_begin + 1:c.row_end + 1] - c.rowptr[c.row_begin:c.row_end]).numpy()
        assert (slots == 0).sum() == (deg == 0).sum() >= 5, "no rows without a slot"
        assert ((slots > 0) & (slots <= WIDE_SLOTS)).any()
    if op_name == "unit_rows_620" and cfg_name == "g4_lds_cap":
        assert npieces.max() > 128, "no wavefront selects the third register of PieceSlots"
    if op_name == "unit_rows_410" and cfg_name == "g2_lds_cap":
        assert npieces.max() == 105, "no wavefront at the LDS cap of the two-entry step"
    if cfg_name == "g4_prod" and ne > 0:
        assert (npieces % cfg["groups"] != 0).any(), "every wavefront's piece count is a multiple of the step width"
    if op_name in ("one_column", "single_row") and cfg_name == "g4_prod":
        assert (npieces == 0).any(), "no wavefront without a piece"
    if op_name == "single_row" and cfg_name == "g4_prod":
        assert (npieces == 1).any()
    if op_name == "empty":
        assert dims["n_slots"] == 0 and dims["n_slabs"] == 0 and dims["n_waves"] > 0 and (slots == 0).all()
    if cfg["row_cap"] == 1:
        assert npieces.max() <= 1


# ----------------------------------------------------------------------------------------------
# reference and bound
def tables(c: Case, dim):
    """x in (-1, 1) and r in (0.25, 1) (no zeros: b * r is never -0), [table_rows, dim] fp32 on the host, seeded."""
    gen = torch.Generator().manual_seed(1000 + dim)
    x = torch.empty((c.table_rows, dim)).uniform_(-1.0, 1.0, generator=gen)
    r = torch.empty((c.table_rows, dim)).uniform_(0.25, 1.0, generator=gen)
    return x, r


_refs = {}


def reference(c: Case, dim):
    """(x, r, P, S, L): P = sum_k v_k x[c_k] and S = sum_k |v_k x[c_k]| per row of the slice and column, in fp64 from the
    operator's own CSR bits, L = entries per row.  Computed once per (operator, width); shared, never written to."""
    key = (c.name, dim)
    if key not in _refs:
        x, r = tables(c, dim)
        rp = c.rowptr[c.row_begin:c.row_end + 1].long()
        ent = c.entries[rp[0]:rp[-1]]
        cols, vals = ent[:, 0].long(), ent[:, 1].contiguous().view(torch.float32).double()
        L = rp[1:] - rp[:-1]
        seg = torch.repeat_interleave(torch.arange(L.numel()), L)
        prod = vals.view(-1, 1) * x.double()[cols]
        P = torch.zeros((L.numel(), dim), dtype=torch.float64).index_add_(0, seg, prod)
        S = torch.zeros((L.numel(), dim), dtype=torch.float64).index_add_(0, seg, prod.abs())
        _refs[key] = (x, r, P, S, L)
    return _refs[key]


def want_and_bound(c: Case, dim, a=1.0, b=0.0, with_r=False):
    x, r, P, S, L = reference(c, dim)
    br = b * r[c.row_begin:c.row_end].double() if with_r else torch.zeros_like(P)
    want = a * P + br
    bound = 1.01 * U * ((L.double().view(-1, 1) + 2) * abs(a) * S + 2 * br.abs())
    return want, bound


def check_rows(got, c: Case, dim, a=1.0, b=0.0, with_r=False, what=""):
    """``got``: rows [row_begin, row_end) of the output, on the host.  The element-wise bound, both norm-wise gates over
    the rows that have entries, and fl(b * r) bit for bit (+0 without r) in the rows that have none."""
    x, r, P, S, L = reference(c, dim)
    want, bound = want_and_bound(c, dim, a, b, with_r)
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32, (what, got.shape)
    err = (got.double() - want).abs()
    assert not torch.isnan(got).any(), (what, "NaN in the operator's rows")
    worst = (err - bound).max().item() if err.numel() else 0.0
    assert (err <= bound).all(), (what, "element-wise bound", worst, torch.nonzero(err > bound)[:8].tolist())
    has, none = L > 0, L == 0
    if has.any():
        e, w = rel_fro(got[has], want[has]), worst_row_rel(got[has], want[has])
        assert e <= TOL and w <= TOL, (what, "norm-wise gates", e, w)
    if none.any():
        exact = (torch.tensor(b, dtype=torch.float32) * r[c.row_begin:c.row_end][none]) if with_r else torch.zeros((int(none.sum()), dim))
        assert torch.equal(got[none].contiguous().view(torch.int32), exact.contiguous().view(torch.int32)), \
            (what, "rows without entries must hold fl(b * r), or +0 without r")


def sentinel_table(n, stride, device):
    return torch.full((n, stride), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def nan_padded(t, pad, device):
    """t on the device as the first columns of rows of t.size(1) + pad floats; the padding holds NaN."""
    full = torch.full((t.size(0), t.size(1) + pad), float("nan"), device=device)
    full[:, :t.size(1)] = t.to(device)
    return full[:, :t.size(1)]


def bits(t):
    return t.contiguous().view(torch.int32)


def run_and_check(op, c: Case, dim, device, what=""):
    """One operator at one width, three ways: a = 1 without r, a = 0.75 / b = 0.25 with r, and both again on strided
    tables (x's and r's padding NaN, y's a sentinel).  Returns the two dense outputs' rows of the slice (device)."""
    x_h, r_h, *_ = reference(c, dim)
    x, r = x_h.to(device), r_h.to(device)
    lo, hi, n = c.row_begin, c.row_end, c.table_rows
    outs = []
    for kw, ref_kw in ((dict(), dict()), (dict(a=A, r=r, b=B), dict(a=A, b=B, with_r=True))):
        y = sentinel_table(n, dim, device)
        op.apply(x, y, **kw)
        check_rows(y[lo:hi], c, dim, what=(what, dim, sorted(ref_kw)), **ref_kw)
        assert (bits(y[:lo]) == SENTINEL).all() and (bits(y[hi:]) == SENTINEL).all(), (what, dim, "wrote outside its rows")
        again = sentinel_table(n, dim, device)
        op.apply(x, again, **kw)
        assert torch.equal(bits(again), bits(y)), (what, dim, "a second run gives other bits")
        outs.append(y[lo:hi])
    xs, rs = nan_padded(x_h, STRIDE_PAD, device), nan_padded(r_h, STRIDE_PAD, device)
    for kw, dense in ((dict(), outs[0]), (dict(a=A, r=rs, b=B), outs[1])):
        ys_full = sentinel_table(n, dim + STRIDE_PAD, device)
        ys = ys_full[:, :dim]
        op.apply(xs, ys, **kw)
        assert torch.equal(bits(ys[lo:hi]), bits(dense)), (what, dim, "strided run differs from the dense run")
        assert (bits(ys_full[:lo]) == SENTINEL).all() and (bits(ys_full[hi:]) == SENTINEL).all() and \
            (bits(ys_full[:, dim:]) == SENTINEL).all(), (what, dim, "strided run wrote outside its rows or columns")
    return outs
