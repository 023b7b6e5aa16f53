"""Which sweep configurations the two planners take: runs without a GPU.

A table of lgc_sweep_cfg settings, each one field away from a base that both planners accept, at the field's last
accepted and first rejected value.  Every row goes to lgc_sweep_plan_create (the host planner: a plan or NULL, and its
code) and to lgc_sweep_dplan_workspace_bytes (the device planner's answer to the same configuration: a size, or 0 for one
it would refuse).  The device planner has two limits of its own, piece_cap <= 64 and lookahead <= 64.  The operator is a
6-row, 12-entry CSR over 8 columns."""
import ctypes as ct

import pytest
import torch

from gnn_ecommerce_amd import _native

E_INVAL = -1    # LGC_E_INVAL
BASE = dict(n_bands=2, waves_per_band_round=4, row_cap=4, piece_cap=8, lookahead=8, groups=4, round_order=0, light_len=0)

ROWPTR = (0, 3, 3, 5, 9, 10, 12)
COLS = (0, 2, 7, 1, 6, 0, 3, 4, 5, 2, 6, 7)
N_COLS = 8

# (fields changed against BASE, host planner accepts, host planner's code, device planner accepts)
TABLE = (
    (dict(n_bands=0), False, E_INVAL, False),
    (dict(n_bands=1), True, 0, True),
    (dict(n_bands=64), True, 0, True),
    (dict(n_bands=65), False, E_INVAL, False),
    (dict(waves_per_band_round=0), False, E_INVAL, False),
    (dict(waves_per_band_round=4), True, 0, True),
    (dict(waves_per_band_round=6), False, E_INVAL, False),
    (dict(row_cap=0), False, E_INVAL, False),
    (dict(row_cap=1), True, 0, True),
    (dict(row_cap=254), True, 0, True),
    (dict(row_cap=255), False, E_INVAL, False),
    (dict(piece_cap=0), False, E_INVAL, False),
    (dict(piece_cap=1), True, 0, True),
    (dict(piece_cap=64), True, 0, True),
    (dict(piece_cap=65), True, 0, False),
    (dict(lookahead=3), False, E_INVAL, False),
    (dict(lookahead=4), True, 0, True),
    (dict(lookahead=64), True, 0, True),
    (dict(lookahead=65), True, 0, False),
    (dict(groups=0), True, 0, True),
    (dict(groups=2), True, 0, True),
    (dict(groups=3), False, E_INVAL, False),
    (dict(groups=4), True, 0, True),
    (dict(round_order=-1), False, E_INVAL, False),
    (dict(round_order=0), True, 0, True),
    (dict(round_order=2), True, 0, True),
    (dict(round_order=3), False, E_INVAL, False),
    (dict(light_len=-2), False, E_INVAL, False),
    (dict(light_len=-1), True, 0, True),
    (dict(light_len=0), True, 0, True),
    (dict(light_len=5, n_bands=3), False, E_INVAL, False),
    (dict(light_len=5, n_bands=1), False, E_INVAL, False),
    (dict(light_len=5, n_bands=4), True, 0, True),
)


def _id(change):
    return "-".join(f"{k}={v}" for k, v in change.items())


@pytest.fixture(scope="module")
def operator():
    rowptr = torch.tensor(ROWPTR, dtype=torch.int32)
    vals = torch.arange(1, len(COLS) + 1, dtype=torch.float32).view(torch.int32)
    entries = torch.stack([torch.tensor(COLS, dtype=torch.int32), vals], dim=1).contiguous()
    assert rowptr.numel() == 7 and entries.shape == (12, 2) and int(rowptr[-1]) == 12 and max(COLS) < N_COLS
    return rowptr, entries


@pytest.mark.parametrize("change,host_ok,host_code,device_ok", TABLE, ids=[_id(row[0]) for row in TABLE])
def test_configuration(operator, change, host_ok, host_code, device_ok):
    assert set(change) <= set(BASE)
    rowptr, entries = operator
    lib = _native.load()
    cfg = _native.SweepCfg(**{**BASE, **change})
    code = ct.c_int(12345)
    handle = lib.lgc_sweep_plan_create(rowptr.data_ptr(), entries.data_ptr(), 0, rowptr.numel() - 1, 0, N_COLS, ct.byref(cfg),
                                       ct.byref(code))
    try:
        assert (bool(handle), code.value) == (host_ok, host_code)
        if handle:
            dims = _native.SweepDims()
            assert lib.lgc_sweep_plan_dims(handle, ct.byref(dims)) == 0
            assert (dims.n_rows, dims.n_entries, dims.n_bands, dims.row_cap) == (6, 12, cfg.n_bands, cfg.row_cap)
            assert dims.groups == (2 if cfg.groups == 2 else 4)
    finally:
        if handle:
            lib.lgc_sweep_plan_free(handle)
    size = lib.lgc_sweep_dplan_workspace_bytes(len(COLS), rowptr.numel() - 1, N_COLS, ct.byref(cfg))
    assert (size > 0) == device_ok


def test_the_table_covers_both_sides_of_every_limit():
    """So that an edit of the table cannot quietly lose a boundary."""
    seen = {}
    for change, *_ in TABLE:
        if len(change) == 1:
            (k, v), = change.items()
            seen.setdefault(k, set()).add(v)
    assert seen == {"n_bands": {0, 1, 64, 65}, "waves_per_band_round": {0, 4, 6}, "row_cap": {0, 1, 254, 255},
                    "piece_cap": {0, 1, 64, 65}, "lookahead": {3, 4, 64, 65}, "groups": {0, 2, 3, 4},
                    "round_order": {-1, 0, 2, 3}, "light_len": {-2, -1, 0}}
    assert [c["n_bands"] for c, *_ in TABLE if c.get("light_len") == 5] == [3, 1, 4]
