"""Light rows of the band sweep (lgc_sweep_cfg.light_len) in the host planner: runs without a GPU.

A light row -- at most light_len entries in total -- gets one piece per pair of adjacent bands.  On operators of at most
a few hundred rows and 4 k entries (tests/sweep_light_support.py): light_len = 0 is the plan of a configuration without
the field; with light rows every entry still appears exactly once, in a slot of its own row, no step holds two entries of
one piece, the rows' slots are contiguous and band-major, no wavefront holds more pieces than row_cap; a case built for it
drops from three rounds to two; and an odd band count is refused."""
import ctypes as ct

import numpy as np
import pytest
import torch

import sweep_light_support as ls
import sweep_support as ss
from gnn_ecommerce_amd import _native
from gnn_ecommerce_amd.graph import sweep_plan_host


def host_plan(c, cfg):
    return sweep_plan_host(c.rowptr, c.entries, c.row_begin, c.row_end, c.col_lo, c.col_hi, cfg)


def slots_of(arr):
    m = arr["multi"].numpy()
    return m[:, 2] - m[:, 1]


@pytest.mark.parametrize("op_name", ls.OPERATORS + ("hub_and_empties", "sub_range", "empty"))
@pytest.mark.parametrize("cfg_name", ("g4_prod", "g4_cap1", "g2_small"))
def test_light_len_zero_is_the_plan_without_the_field(op_name, cfg_name):
    c = ls.case(op_name) if op_name in ls.OPERATORS else ss.case(op_name)
    cfg = ss.CONFIGS[cfg_name]
    assert "light_len" not in cfg
    want_dims, want = host_plan(c, cfg)
    dims, arr = host_plan(c, dict(cfg, light_len=0))
    assert dims["light_len"] == 0
    ss.assert_same_plan(dims, arr, want_dims, want, (op_name, cfg_name))


@pytest.mark.parametrize("op_name,cfg_name,cfg", ls.PLANS, ids=ls.PLAN_IDS)
def test_host_plan_with_light_rows(op_name, cfg_name, cfg):
    c = ls.case(op_name)
    dims, arr = host_plan(c, cfg)
    got = ls.check_light_plan(c, cfg, dims, arr)
    # the decoded plan, summed slot by slot in fp64, is the row's fp64 CSR product
    dim = 5
    x = torch.empty((c.table_rows, dim), dtype=torch.float64).uniform_(-1.0, 1.0, generator=torch.Generator().manual_seed(6))
    for row, sb, se, _ in arr["multi"].numpy():
        ent = c.entries[c.rowptr[row]:c.rowptr[row + 1]]
        vals = ent[:, 1].contiguous().view(torch.float32).double()
        prod = vals.view(-1, 1) * x[ent[:, 0].long()]
        total = torch.zeros(dim, dtype=torch.float64)
        for sl in range(sb, se):
            cols = torch.tensor([col for col, _ in got[sl]], dtype=torch.long)
            v = torch.from_numpy(np.array([b for _, b in got[sl]], dtype=np.uint32).view(np.float32)).double()
            total += (v.view(-1, 1) * x[cols]).sum(0)
        assert ((total - prod.sum(0)).abs() <= 2.0 ** -52 * (len(ent) + 1) * prod.abs().sum(0)).all(), row


def test_the_cases_hold_what_they_are_there_for():
    """So that a change of the planner or of a case cannot quietly empty one of them."""
    for name in ls.OPERATORS:
        c = ls.case(name)
        assert c.row_end - c.row_begin <= 300 and int(c.rowptr[c.row_end] - c.rowptr[c.row_begin]) <= 4000
    plans = {(o, n): (ls.case(o), cfg, *host_plan(ls.case(o), cfg)) for o, n, cfg in ls.PLANS}
    # light and heavy rows side by side; all light; none light
    c, cfg, dims, arr = plans[("light_mixed", "b8")]
    lens = ls.row_lengths(c)
    assert (lens <= 24).sum() > 10 and (lens > 24).sum() > 10 and (lens == 0).sum() >= 2
    assert (slots_of(arr)[(lens > 0) & (lens <= 24)] <= 4).all() and (slots_of(arr)[lens > 24] > 4).any()
    c, cfg, dims, arr = plans[("light_mixed", "b8_all_light")]
    assert (ls.row_lengths(c) <= cfg["light_len"]).all() and slots_of(arr).max() > 4      # the long rows are cut by the piece cap
    plain = host_plan(c, dict(cfg, light_len=0))
    assert dims["n_slots"] < plain[0]["n_slots"]
    c, cfg, dims, arr = plans[("light_threshold", "b8_none_light")]
    assert (ls.row_lengths(c) > cfg["light_len"]).all()
    ss.assert_same_plan({**dims, "light_len": 0}, arr, *host_plan(c, dict(cfg, light_len=0)), "no row light")
    # a row exactly at the threshold and one entry above it
    for n in ("b8", "b2"):
        c, cfg, dims, arr = plans[("light_threshold", n)]
        lens, slots, nb = ls.row_lengths(c), slots_of(arr), cfg["n_bands"]
        assert (lens == 24).sum() >= 12 and (lens == 25).sum() >= 12
        assert (slots[lens <= 24] == nb // 2).all() and (slots[lens >= 25] > nb // 2).all()
    # a light row with entries in only one band of a pair, on either side of the pair
    c, cfg, dims, arr = plans[("light_one_band", "b8")]
    bound, lens = ls.band_bounds(c, 8), ls.row_lengths(c)
    rp, cols = c.rowptr.numpy(), c.entries.numpy()[:, 0]
    has = [{ls.band_of(int(x), bound) for x in cols[rp[r]:rp[r + 1]]} for r in range(c.row_begin, c.row_end)]
    # (row parity, which band of the pair has the entries): all four, so also the two where the alternating home is empty
    seen = {(i & 1, b & 1) for i, bands in enumerate(has) if lens[i] <= 24 for b in bands if (b ^ 1) not in bands}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # bands without a column
    c, cfg, dims, arr = plans[("light_empty_band", "b8")]
    bound = ls.band_bounds(c, 8)
    assert sum(bound[b] == bound[b + 1] for b in range(8)) >= 2
    # a pair's run that the piece cap still cuts
    c, cfg, dims, arr = plans[("light_long_run", "b8_pcap16")]
    lens, slots = ls.row_lengths(c), slots_of(arr)
    assert dims["piece_cap"] < 150 and (lens == 150).sum() == 8 and (slots[lens == 150] >= 150 // dims["piece_cap"]).all()


def test_light_rows_save_a_round_on_the_case_built_for_it():
    """36 rows x 8 bands with 2 entries each, 4 wavefronts of 3 accumulators per band and round: 36 pieces per band are
    three rounds; as light rows the pairs' pieces alternate between the two bands, 18 per band: two rounds."""
    c = ls.case("light_rounds")
    cfg = dict(ls.PLANS[-1][2])
    assert ls.PLANS[-1][0] == "light_rounds" and cfg["row_cap"] == 3 and cfg["waves_per_band_round"] == 4
    plain, _ = host_plan(c, dict(cfg, light_len=0))
    light, arr = host_plan(c, cfg)
    assert plain["rounds"] == 3 and plain["n_slots"] == 36 * 8
    assert light["rounds"] == 2 and light["n_slots"] == 36 * 4
    assert light["n_waves"] == 2 * 4 * 8 and arr["wave_npieces"].numpy()[: light["n_waves"]].max() <= 3
    # the planner's own choice (light_len = -1): the smallest length that saves the round with 3 % to spare is the rows' 16
    auto, auto_arr = host_plan(c, dict(cfg, light_len=-1))
    assert auto["light_len"] == 16 and auto["rounds"] == 2
    ss.assert_same_plan(auto, auto_arr, {**light, "light_len": 16}, host_plan(c, dict(cfg, light_len=16))[1], "auto")
    # where no length up to twice the median saves a round, the choice is 0: the plan without light rows
    wide = dict(cfg, row_cap=78, light_len=-1)
    dims, arr2 = host_plan(c, wide)
    assert dims["light_len"] == 0 and dims["rounds"] == 1
    ss.assert_same_plan(dims, arr2, *host_plan(c, dict(wide, light_len=0)), "auto picks 0")


@pytest.mark.parametrize("n_bands", (1, 3, 7))
def test_an_odd_band_count_with_light_rows_is_refused(n_bands):
    c = ls.case("light_mixed")
    lib = _native.load()
    rp = (c.rowptr[c.row_begin:c.row_end + 1] - c.rowptr[c.row_begin]).contiguous()
    ent = c.entries[c.rowptr[c.row_begin]:c.rowptr[c.row_end]].contiguous()
    n = c.row_end - c.row_begin

    def create(**kw):
        cfg = _native.SweepCfg(**{**ls.PLANS[0][2], "n_bands": n_bands, **kw})
        code = ct.c_int(0)
        handle = lib.lgc_sweep_plan_create(rp.data_ptr(), ent.data_ptr(), 0, n, c.col_lo, c.col_hi, ct.byref(cfg), ct.byref(code))
        if handle:
            lib.lgc_sweep_plan_free(handle)
        return bool(handle), code.value
    assert create(light_len=24) == (False, -1)                 # LGC_E_INVAL
    assert create(light_len=-2) == (False, -1)
    assert create(light_len=0) == (True, 0)
    assert create(light_len=-1) == (True, 0)                   # the planner's choice for an odd count is 0
    assert lib.lgc_sweep_dplan_workspace_bytes(1000, 10, 100, ct.byref(_native.SweepCfg(**{**ls.PLANS[0][2], "n_bands": n_bands}))) == 0
