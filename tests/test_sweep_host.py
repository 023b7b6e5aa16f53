"""The band-sweep planner's host code on small degenerate operators (tests/sweep_support.py): runs without a GPU.

Every named operator under every named configuration: the decoded plan, summed slot by slot and then row by row in
fp64, is the row's fp64 CSR product; every entry lies in exactly one slot of its own row; the steps are
conflict-free; ``multi`` lists exactly the rows of the range with contiguous slot ranges; and the structural
conditions each case exists for hold.  Then the LDS caps of lgc_spmm_sweep, refused before any launch."""
import ctypes as ct

import numpy as np
import pytest
import torch

import sweep_support as ss
from gnn_ecommerce_amd import _native
from gnn_ecommerce_amd.graph import sweep_plan_host


@pytest.mark.parametrize("op_name,cfg_name", ss.PAIRS)
def test_host_plan_of_a_named_operator(op_name, cfg_name):
    c, cfg = ss.case(op_name), ss.CONFIGS[cfg_name]
    dims, arr = sweep_plan_host(c.rowptr, c.entries, c.row_begin, c.row_end, c.col_lo, c.col_hi, cfg)
    n_rows = c.row_end - c.row_begin
    e0, e1 = int(c.rowptr[c.row_begin]), int(c.rowptr[c.row_end])
    assert dims["n_entries"] == e1 - e0 and dims["n_rows"] == n_rows and dims["groups"] == cfg["groups"]
    assert dims["n_bands"] == cfg["n_bands"] and dims["row_cap"] == cfg["row_cap"]
    assert dims["n_waves"] == dims["rounds"] * cfg["waves_per_band_round"] * cfg["n_bands"] and dims["n_waves"] % 4 == 0
    assert cfg["piece_cap"] <= dims["piece_cap"] < 4 * cfg["piece_cap"] + 16
    assert dims["n_padding"] == dims["groups"] * dims["n_steps"] - dims["n_entries"]
    got = ss.decode_sweep(dims, arr, cfg["row_cap"])                     # conflict-free steps, padding well-formed
    multi = arr["multi"].numpy()
    assert multi.shape == (n_rows, 4) and (multi[:, 0] == np.arange(c.row_begin, c.row_end)).all()
    assert multi[0, 1] == 0 and multi[-1, 2] == dims["n_slots"] and (multi[1:, 1] == multi[:-1, 2]).all()
    assert sorted(got) == list(range(dims["n_slots"]))                   # every slot holds something, none is foreign
    dim = 7                                                              # the planner does not know the width
    x = torch.empty((c.table_rows, dim), dtype=torch.float64).uniform_(-1.0, 1.0, generator=torch.Generator().manual_seed(5))
    for row, sb, se, _ in multi:
        ent = c.entries[c.rowptr[row]:c.rowptr[row + 1]]
        want_entries = sorted((int(col), int(v) & 0xFFFFFFFF) for col, v in ent.tolist())
        mine = [e for sl in range(sb, se) for e in got[sl]]
        assert sorted(mine) == want_entries, row                         # each entry once, in a slot of its own row
        assert all(len(got[sl]) <= dims["piece_cap"] for sl in range(sb, se))
        vals = ent[:, 1].contiguous().view(torch.float32).double()
        want = (vals.view(-1, 1) * x[ent[:, 0].long()]).sum(0)
        scale = (vals.view(-1, 1) * x[ent[:, 0].long()]).abs().sum(0)
        total = torch.zeros(dim, dtype=torch.float64)
        for sl in range(sb, se):
            cols = torch.tensor([col for col, _ in got[sl]], dtype=torch.long)
            v = torch.from_numpy(np.array([b for _, b in got[sl]], dtype=np.uint32).view(np.float32)).double()
            total += (v.view(-1, 1) * x[cols]).sum(0)
        assert ((total - want).abs() <= 2.0 ** -52 * (len(ent) + 1) * scale).all(), row      # fp64 rounding only
    ss.assert_preconditions(op_name, cfg_name, cfg, dims, arr)


def test_every_structural_precondition_is_exercised():
    """The cases the preconditions speak of exist under these names (a renamed case would skip its assertions)."""
    assert {"hub_and_empties", "one_column", "single_row", "unit_rows_620", "unit_rows_410", "empty"} <= set(ss.OPERATORS)
    assert {"g4_prod", "g4_lds_cap", "g2_lds_cap", "g4_small", "g4_cap1", "g2_small"} <= set(ss.CONFIGS)
    for cfg in ss.CONFIGS.values():
        assert cfg["lookahead"] <= 64 and cfg["piece_cap"] <= 64 and cfg["round_order"] in (0, 1, 2)
    assert {c["round_order"] for n, c in ss.CONFIGS.items() if n.startswith("g4_small")} == {0, 1, 2}
    assert {c["round_order"] for n, c in ss.CONFIGS.items() if n.startswith("g2_small")} == {0, 1, 2}
    assert max(ss.case(o).table_rows for o in ss.OPERATORS) <= 4200
    for o in ss.OPERATORS:
        c = ss.case(o)
        assert 0 < c.row_begin < c.row_end < c.table_rows and c.col_hi < c.table_rows
        assert c.rowptr[c.row_begin] > 0 and c.rowptr[-1] > c.rowptr[c.row_end]       # entries before and after the slice


def test_sweep_refuses_a_row_cap_beyond_the_lds_before_any_launch():
    """160 KiB hold four wavefronts of row_cap + 1 accumulator rows: 159 rows of 64 floats, 105 of 96.  One more, and
    row_cap 255, is LGC_E_INVAL; the caps themselves pass the argument checks (no wavefront, no row: nothing launches,
    and what comes back is HIP's own status)."""
    lib = _native.load()
    one = ct.c_void_p(256)

    def sweep(row_cap, groups, dim, stride, n_waves=8, n_rows=4):
        return lib.lgc_spmm_sweep(one, one, one, one, n_waves, row_cap, groups, one, n_rows, None, 0, one, 1000, one, stride,
                                  ct.c_void_p(512), stride, None, 0, 1.0, 0.0, dim, None)
    assert sweep(160, 4, 64, 64) == -1 and sweep(160, 4, 128, 128) == -1 and sweep(254, 4, 64, 64) == -1
    assert sweep(106, 2, 90, 96) == -1 and sweep(106, 2, 68, 68) == -1 and sweep(159, 2, 96, 96) == -1
    assert sweep(255, 4, 64, 64) == -1 and sweep(255, 2, 90, 90) == -1 and sweep(0, 4, 64, 64) == -1
    assert sweep(159, 4, 64, 64, 0, 0) >= 0 and sweep(105, 2, 90, 96, 0, 0) >= 0
