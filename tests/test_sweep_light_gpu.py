"""Light rows of the band sweep (lgc_sweep_cfg.light_len) on the GPU, on the operators of tests/sweep_light_support.py:
the device planner against the host planner array for array, and lgc_apply through the sweep route at D = 64 and D = 20
against an fp64 CSR product -- also with the epilogue row aliased to the output (r = y, b = 1), the way the reduced
middle layers run -- and bit for bit the same on a second run."""
import pytest
import torch

import sweep_light_support as ls
import sweep_support as ss
from conftest import rel_fro
from gnn_ecommerce_amd import graph as G
from gnn_ecommerce_amd.graph import Operator

pytestmark = pytest.mark.gpu

REL_FRO = 1e-6                 # the gate tests/test_sweep_gpu.py's routes are held to (the project's 1e-5 with a decade to spare)
_on_device = {}


def device_case(name, device):
    if name not in _on_device:
        c = ls.case(name)
        _on_device[name] = (c.rowptr.to(device), c.entries.to(device))
    return _on_device[name]


@pytest.mark.parametrize("op_name,cfg_name,cfg", ls.PLANS, ids=ls.PLAN_IDS)
def test_device_planner_builds_the_host_planners_plan_with_light_rows(device, op_name, cfg_name, cfg):
    c = ls.case(op_name)
    rowptr, entries = device_case(op_name, device)
    for this in (cfg, dict(cfg, light_len=0), dict(cfg, light_len=-1)):
        want_dims, want = G.sweep_plan_host(c.rowptr, c.entries, c.row_begin, c.row_end, c.col_lo, c.col_hi, this)
        got = G.sweep_plan_on_device(rowptr, entries, c.row_begin, c.row_end, c.col_lo, c.col_hi, this)
        assert got is not None, "the device planner must take this configuration"
        dims, arr = got
        ss.assert_same_plan(dims, arr, want_dims, want, (op_name, cfg_name, this["light_len"]))
    assert G.sweep_plan_on_device(rowptr, entries, c.row_begin, c.row_end, c.col_lo, c.col_hi, dict(cfg, n_bands=3)) is None


def sweep_operator(c, cfg, device, monkeypatch):
    rowptr, entries = device_case(c.name, device)
    monkeypatch.setattr(G, "SWEEP_CFG", dict(cfg, groups=4))
    monkeypatch.setattr(G, "SWEEP_CFG_WIDE", dict(cfg, groups=2))
    monkeypatch.setattr(G, "SWEEP_WIDE", True)
    monkeypatch.setattr(G, "SWEEP_PLAN_ON_DEVICE", True)
    op = Operator.build(c.table_rows, rowptr, entries, c.row_begin, c.row_end, 32, 256, tiles=False)
    op.sweep_cols, op.sweep_bands = (c.col_lo, c.col_hi), cfg["n_bands"]
    op.sweep_light_len = op.sweep_light_len_wide = cfg["light_len"]
    return op


def test_wide_sweep_route_with_light_rows(device, monkeypatch):
    """The two-entry plan (68..96 columns) takes light rows as well -- off by default, but behind a switch."""
    (op_name, cfg_name, cfg), = [p for p in ls.PLANS if p[2]["groups"] == 2]
    c = ls.case(op_name)
    op = sweep_operator(c, cfg, device, monkeypatch)
    for dim in (72, 90):
        x = torch.empty((c.table_rows, dim), device=device)
        assert op.route(x, torch.empty_like(x)) == "sweep_wide+wt"
        ss.run_and_check(op, c, dim, device, (op_name, cfg_name))
    assert op._sweep[2].dims["light_len"] == cfg["light_len"] and set(op._sweep) == {2}


@pytest.mark.parametrize("op_name,cfg_name,cfg", [p for p in ls.PLANS if p[2]["groups"] == 4],
                         ids=[i for i, p in zip(ls.PLAN_IDS, ls.PLANS) if p[2]["groups"] == 4])
def test_sweep_route_with_light_rows(device, monkeypatch, op_name, cfg_name, cfg):
    c = ls.case(op_name)
    op = sweep_operator(c, cfg, device, monkeypatch)
    lo, hi = c.row_begin, c.row_end
    # D = 64: the narrow sweep kernel with the element-wise bound and every side condition of tests/sweep_support.py
    x64 = torch.empty((c.table_rows, 64), device=device)
    assert op.route(x64, torch.empty_like(x64)) == "sweep+wt"
    ss.run_and_check(op, c, 64, device, (op_name, cfg_name))
    plan = op._sweep[4]
    assert plan.dims["light_len"] == cfg["light_len"] and plan.dims["n_bands"] == cfg["n_bands"]
    for dim in (64, 20):
        x_h, r_h, P, S, L = ss.reference(c, dim)
        x = x_h.to(device)
        has = L > 0
        y = ss.sentinel_table(c.table_rows, dim, device)
        op.apply(x, y)
        if dim == 64:
            assert op.route(x, y) == "sweep+wt"
        assert rel_fro(y[lo:hi].cpu()[has], P[has]) <= REL_FRO, (dim, "a = 1")
        # the epilogue row aliased to the output: y <- A y0 + y0, twice from the same y0
        outs = []
        for _ in range(2):
            y = r_h.to(device).clone()
            op.apply(x, y, r=y, b=1.0)
            outs.append(y)
        want = P + r_h[lo:hi].double()
        assert rel_fro(outs[0][lo:hi].cpu(), want) <= REL_FRO, (dim, "r = y")
        assert torch.equal(ss.bits(outs[0]), ss.bits(outs[1])), (dim, "a second run gives other bits")
        untouched = torch.ones(c.table_rows, dtype=torch.bool)
        untouched[lo:hi] = False
        assert torch.equal(ss.bits(outs[0].cpu()[untouched]), ss.bits(r_h[untouched])), (dim, "wrote outside its rows")
