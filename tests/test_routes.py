"""Every route of the hop dispatcher (lgc_apply) against its decision table and against an fp64 reference.

``lgc_apply_route`` names the kernels lgc_apply launches; which ones depends on the width, on the table's geometry
(24-bit row ids, 32-bit byte offsets, the padding id 0xFFFFFF's wrapped offset beyond the table) and on three switches
read once per process.  On the CPU: the decision table on both sides of every limit.  On the GPU: each switch set in a
fresh child process (tests/route_child.py), and every table-size limit just below and just above it."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, rel_fro, worst_row_rel
from gnn_ecommerce_amd import _native, synth

TOL = 1e-5
FAKE = 1 << 20                     # aligned, non-null, never dereferenced


def route_of(lib, op, rows, xs, ys=None, rs=0, dim=None):
    code = lib.lgc_apply_route(ctypes.byref(op), rows, xs, xs if ys is None else ys, rs, xs if dim is None else dim)
    return code if code < 0 else _native.route_name(code)


def fake_operator(tiles=True, groups=None, meta=True):
    """An lgc_operator with fake device pointers: one tile class (or none), the chunk plan, and optionally band-sweep
    arrays of `groups` entries per step (a host struct, as lgc_operator.sweep is)."""
    op = _native.OperatorC()
    op.rowptr = op.entries = op.chunks = op.multi = op.partials = FAKE
    op.row_begin, op.row_end, op.short_max, op.n_chunks, op.n_multi, op.tiles_per_wave = 0, 100, 32, 3, 1, 1
    if tiles:
        op.tiles[0] = _native.TileClassC(FAKE, FAKE if meta else None, FAKE, 4, 8)
        op.tiles[1] = _native.TileClassC(FAKE, None, FAKE, 0, 16)       # a class without tiles does not vote
        op.n_tile_classes = 2
    if groups is not None:
        sc = _native.SweepArraysC(FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 64, 20, 10, 0, groups)
        op.sweep = ctypes.pointer(sc)
        op._keep = sc
    return op


# (stride = dim, last row count with DPP tiles and the sweep, first row count with plain stores)
LIMITS = [(64, 16_777_214, 16_777_216), (68, 986_894, 15_790_321), (80, 3_355_442, 13_421_773),
          (90, 4_846_750, 11_930_465), (96, 5_592_404, 11_184_811), (128, 8_388_607, 8_388_608)]
SWEEP_OF = {64: "sweep", 68: "sweep_wide", 80: "sweep_wide", 90: "sweep_wide", 96: "sweep_wide", 128: "sweep_two_pass"}


@pytest.mark.parametrize("dim,fast_max,plain_from", LIMITS)
def test_route_limits_of_the_table_geometry(dim, fast_max, plain_from):
    lib = _native.load()
    tiles, sweep = fake_operator(), fake_operator(groups=2 if 64 < dim <= 96 else 4)
    wt = lambda rows: "+wt" if rows < plain_from else ""
    for rows in (1, 1000, fast_max - 1, fast_max):
        assert route_of(lib, tiles, rows, dim) == "fused_dpp" + wt(rows), rows
        assert route_of(lib, sweep, rows, dim) == SWEEP_OF[dim] + wt(rows), rows
    for rows in {fast_max + 1, fast_max + 2, plain_from - 1, plain_from, plain_from + 1, 0xFFFFFF, 1 << 25} - {fast_max}:
        assert route_of(lib, tiles, rows, dim) == "fused_generic" + wt(rows), rows
        assert route_of(lib, sweep, rows, dim) == "fused_generic" + wt(rows), rows
    rows_only = fake_operator(tiles=False)
    for rows in (fast_max, fast_max + 1, plain_from - 1, plain_from):
        assert route_of(lib, rows_only, rows, dim) == "rows" + wt(rows), rows


def test_route_at_the_24_bit_row_id_and_the_4_gib_store_limits():
    lib = _native.load()
    tiles, sweep = fake_operator(), fake_operator(groups=4)
    assert route_of(lib, tiles, 0xFFFFFE, 64) == "fused_dpp+wt" and route_of(lib, sweep, 0xFFFFFE, 64) == "sweep+wt"
    assert route_of(lib, tiles, 0xFFFFFF, 64) == "fused_generic+wt" == route_of(lib, sweep, 0xFFFFFF, 64)
    assert route_of(lib, tiles, (1 << 24) - 1, 64) == "fused_generic+wt"
    assert route_of(lib, tiles, 1 << 24, 64) == "fused_generic" == route_of(lib, sweep, 1 << 24, 64)
    # narrower rows: the 24-bit id limit alone
    assert route_of(lib, tiles, 0xFFFFFE, 61) == "fused_dpp+wt" and route_of(lib, tiles, 0xFFFFFF, 61) == "fused_generic+wt"


def test_route_with_different_strides_and_r():
    """x decides the sweep; x, y and r each decide the DPP tiles; y alone decides the write-through stores."""
    lib = _native.load()
    tiles, sweep = fake_operator(), fake_operator(groups=4)
    lim68 = 986_894
    for rows, fast in ((lim68, "fused_dpp"), (lim68 + 1, "fused_generic")):
        assert route_of(lib, tiles, rows, 64, ys=68, dim=64) == fast + "+wt"          # y's stride 68 limits
        assert route_of(lib, tiles, rows, 68, ys=64, dim=64) == fast + "+wt"          # x's
        assert route_of(lib, tiles, rows, 64, ys=64, rs=68, dim=64) == fast + "+wt"   # r's
        assert route_of(lib, tiles, rows, 64, ys=64, rs=64, dim=64) == "fused_dpp+wt"
        assert route_of(lib, sweep, rows, 64, ys=68, rs=68, dim=64) == "sweep+wt"     # the sweep reads only x by row id
        assert route_of(lib, sweep, rows, 68, ys=64, dim=64) == ("sweep" if fast == "fused_dpp" else fast) + "+wt"
    # wt_store follows y: 8,388,608 rows of 128 floats reach 4 GiB, of 64 floats they do not
    assert route_of(lib, tiles, 1 << 23, 128, ys=64, dim=64) == "fused_generic+wt"
    assert route_of(lib, tiles, 1 << 23, 64, ys=128, dim=64) == "fused_generic"
    assert route_of(lib, tiles, (1 << 23) - 1, 64, ys=128, dim=64) == "fused_dpp+wt"


@pytest.mark.parametrize("dim,tiles,sweep4,sweep2", [
    (60, "fused_generic", "fused_generic", "fused_generic"), (61, "fused_dpp", "sweep", "fused_dpp"),
    (64, "fused_dpp", "sweep", "fused_dpp"), (65, "fused_generic", "fused_generic", "fused_generic"),
    (67, "fused_generic", "fused_generic", "fused_generic"), (68, "fused_dpp", "fused_dpp", "sweep_wide"),
    (96, "fused_dpp", "fused_dpp", "sweep_wide"), (97, "fused_dpp", "sweep_two_pass", "fused_dpp"),
    (128, "fused_dpp", "sweep_two_pass", "fused_dpp"), (129, "fused_generic", "fused_generic", "fused_generic"),
    (3, "rows", "rows", "rows"), (4, "fused_generic", "fused_generic", "fused_generic")])
def test_route_by_width(dim, tiles, sweep4, sweep2):
    """A sweep plan serves only the widths of its step (4 entries: 61..64 and, in two passes, 97..128; 2: 68..96);
    every other width of the same operator falls back to the tiles."""
    lib = _native.load()
    assert route_of(lib, fake_operator(), 5000, dim) == tiles + "+wt"
    assert route_of(lib, fake_operator(groups=4), 5000, dim) == sweep4 + "+wt"
    assert route_of(lib, fake_operator(groups=0), 5000, dim) == sweep4 + "+wt"          # 0 means 4
    assert route_of(lib, fake_operator(groups=2), 5000, dim) == sweep2 + "+wt"
    assert route_of(lib, fake_operator(tiles=False), 5000, dim) == "rows+wt"
    assert route_of(lib, fake_operator(meta=False), 5000, dim) == ("rows" if dim < 4 else "fused_generic") + "+wt"


def test_route_argument_errors():
    lib = _native.load()
    op = fake_operator()
    assert lib.lgc_apply_route(None, 100, 64, 64, 0, 64) == -1
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 64, 64, 0, 0) == -2
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 300, 300, 0, 257) == -2
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 63, 64, 0, 64) == -1
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 64, 63, 0, 64) == -1
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 64, 64, 32, 64) == -1
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 64, 64, -1, 64) == -1
    assert lib.lgc_apply_route(ctypes.byref(op), -1, 64, 64, 0, 64) == -1
    op.n_tile_classes = 4
    assert lib.lgc_apply_route(ctypes.byref(op), 100, 64, 64, 0, 64) == -1


# ----------------------------------------------------------------------------------------
# GPU: the switches, one fresh process per switch set
HELPER = os.path.join(ROOT, "tests", "route_child.py")
KNOBS = ("LGCN_NO_FAST_TILES", "LGCN_NO_FUSED_APPLY", "LGCN_SWEEP_LAUNCH_WAVES")
SWITCH_SETS = {
    "no_fast_tiles": ({"LGCN_NO_FAST_TILES": "1"}, "fused_generic+wt"),
    "no_fused_apply": ({"LGCN_NO_FUSED_APPLY": "1"}, "split_dpp+wt"),
    "no_fast_tiles_no_fused_apply": ({"LGCN_NO_FAST_TILES": "1", "LGCN_NO_FUSED_APPLY": "1"}, "split_generic+wt"),
    "sweep_launch_waves_4": ({"LGCN_SWEEP_LAUNCH_WAVES": "4"}, "fused_dpp+wt"),
    "sweep_launch_waves_12": ({"LGCN_SWEEP_LAUNCH_WAVES": "12"}, "fused_dpp+wt"),
}
CHILD_TIMEOUT = 300


@pytest.fixture(scope="module")
def children(device, tmp_path_factory):
    """Each switch set once, in order.  A child killed by a signal or the time limit stops the rest from starting."""
    tmp = tmp_path_factory.mktemp("routes")
    out = {}
    crashed = None
    for name, (switches, _) in SWITCH_SETS.items():
        if crashed is not None:
            out[name] = (None, f"not started: child {crashed} did not end normally", None)
            continue
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(switches)
        path = tmp / f"{name}.json"
        try:
            proc = subprocess.run([sys.executable, HELPER, "--out", str(path)], env=env, cwd=ROOT, timeout=CHILD_TIMEOUT,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired as exc:
            out[name] = (None, f"timed out after {CHILD_TIMEOUT} s: {exc.output}", None)
            crashed = name
            continue
        if proc.returncode < 0:
            crashed = name
        summary = json.loads(path.read_text()) if proc.returncode == 0 and path.exists() else None
        out[name] = (proc.returncode, proc.stdout, summary)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWITCH_SETS))
def test_forced_route_in_a_fresh_process(children, name):
    """Routes, bit identity with the row-pointer path, fp64 parity and untouched padding under one switch set (the
    checks are in tests/route_child.py)."""
    code, output, summary = children[name]
    assert code == 0, f"child {name} ended with {code}:\n{output[-4000:]}"
    assert summary is not None and summary["tile_route"] == SWITCH_SETS[name][1]
    assert sorted(summary["widths"], key=int) == ["61", "64", "68", "80", "90", "96", "101", "128"]


@pytest.mark.gpu
def test_sweep_in_several_launches_is_bit_identical_to_one(children):
    """LGCN_SWEEP_LAUNCH_WAVES slices the sweep into launches of 4 / 12 wavefronts (p.wave_begin); the other children
    run it in one launch.  Every width's output must carry the same bits."""
    for name in SWITCH_SETS:
        assert children[name][0] == 0, f"child {name} failed: {children[name][1][-2000:]}"
    one = children["no_fast_tiles"][2]["widths"]
    for name in SWITCH_SETS:
        got = children[name][2]["widths"]
        for dim, d in one.items():
            assert d["sweep_waves"] > 12, (dim, d)        # several launches at 4 and at 12 wavefronts per launch
            assert got[dim]["sweep"] == d["sweep"] and got[dim]["sweep_epilogue"] == d["sweep_epilogue"], (name, dim)
    # a named operator of tests/sweep_support.py: rows with more than 32 slots and rows with none, in several launches
    one = children["no_fast_tiles"][2]["operators"]
    assert list(one) == ["hub_and_empties/g4_small"]
    for name in SWITCH_SETS:
        for key, d in one.items():
            assert d["sweep_waves"] > 12, (key, d)
            assert children[name][2]["operators"][key] == d, (name, key)


# ----------------------------------------------------------------------------------------
# GPU: table-geometry limits, in-process
def boundary_graph(n_nodes, n_items=3000, seed=0):
    """A user|item COO in the reference's layout (both directions): n_items items at the top of the id range, five
    of them hubs of 600+ users (longer than chunk_len); 20,000 users spread over the whole user range plus the last
    300 user ids, one to five purchases each; every other user row isolated."""
    gen = torch.Generator().manual_seed(seed)
    nu = n_nodes - n_items
    users = torch.cat([torch.randint(0, nu - 300, (20000,), generator=gen), torch.arange(nu - 300, nu)]).unique()
    u = users.repeat_interleave(torch.randint(1, 6, (users.numel(),), generator=gen))
    i = torch.randint(0, n_items, (u.numel(),), generator=gen)
    u = torch.cat([u, users[torch.randint(0, users.numel(), (3000,), generator=gen)]])
    i = torch.cat([i, torch.arange(5).repeat_interleave(600)])
    key = torch.unique(u * n_items + i)
    u, i = key // n_items, key % n_items
    w = torch.from_numpy(synth.WEIGHT_VALUES[torch.randint(7, (key.numel(),), generator=gen).numpy()])
    ei = torch.stack((torch.cat([u, i + nu]), torch.cat([i + nu, u])))
    return ei, torch.cat([w, w]), nu


def check_hop(op, x, y, r, a, b):
    """Rows of the operator with entries vs an fp64 evaluation of the operator's own CSR values (built on the host
    from the gathered rows only); every other row of its range must hold fl(b * r) exactly, checked on the device."""
    dev = x.device
    lo, hi = op.plan.row_begin, op.plan.row_end
    rowptr = op.rowptr[lo:hi + 1].cpu().long()
    deg = rowptr[1:] - rowptr[:-1]
    rows = torch.nonzero(deg).view(-1)
    ent = op.entries[rowptr[0]:rowptr[-1]].cpu()
    cols, vals = ent[:, 0].long(), ent[:, 1].contiguous().view(torch.float32).double()
    seg = torch.repeat_interleave(torch.arange(rows.numel()), deg[rows])
    ucols, inv = torch.unique(cols, return_inverse=True)
    xg = x[ucols.to(dev)].cpu().double()
    grows = (rows + lo).to(dev)
    want = torch.zeros((rows.numel(), x.size(1)), dtype=torch.float64).index_add_(0, seg, vals.view(-1, 1) * xg[inv])
    want = a * want + b * r[grows].cpu().double()
    got = y[grows].cpu()
    assert rel_fro(got, want) <= TOL and worst_row_rel(got, want) <= TOL, (rel_fro(got, want), worst_row_rel(got, want))
    iso = (op.rowptr[lo + 1:hi + 1] == op.rowptr[lo:hi])
    step = 1 << 20
    for c0 in range(0, hi - lo, step):
        c1 = min(hi - lo, c0 + step)
        m = iso[c0:c1]
        ym, rm = y[lo + c0:lo + c1][m], r[lo + c0:lo + c1][m]
        assert torch.equal(ym.contiguous().view(torch.int32), (b * rm).contiguous().view(torch.int32)), (lo + c0, lo + c1)
    return rows.numel()


def run_boundary(device, monkeypatch, dim, n_nodes, routes, strides=()):
    """Both halves of a boundary_graph with n_nodes rows at width dim: routes as expected, values against fp64.
    `strides`: also on strided tables (x's padding NaN, y's a sentinel) that must give the dense run's bits, or --
    where the stride moves the item half onto another route -- pass the fp64 check, with y's sentinel bytes intact."""
    from gnn_ecommerce_amd import graph as G
    from gnn_ecommerce_amd.graph import Operator, PropGraph
    need = 3 * n_nodes * dim * 4 + (2 << 30)
    free, _ = torch.cuda.mem_get_info(device)
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    held = torch.cuda.memory_allocated(device)                 # by earlier tests of the session
    monkeypatch.setattr(G, "USE_SWEEP", "1")
    ei, ew, nu = boundary_graph(n_nodes)
    op = PropGraph(ei.to(device), ew.to(device), n_nodes).forward_op
    users = Operator.build(n_nodes, op.rowptr, op.entries, 0, nu, 32, 256, tiles=True)
    items = Operator.build(n_nodes, op.rowptr, op.entries, nu, n_nodes, 32, 256, tiles=True, sweep_cols=(0, nu))
    assert items.sweep_cols == (0, nu) and items.plan.n_multi > 0
    gen = torch.Generator(device=device).manual_seed(dim)
    x = torch.empty((n_nodes, dim), device=device).uniform_(-1.0, 1.0, generator=gen)
    r = torch.empty((n_nodes, dim), device=device).uniform_(0.25, 1.0, generator=gen)       # no zeros: no -0 from b * r
    y = torch.empty((n_nodes, dim), device=device)
    got_routes = (users.route(x, y, r), items.route(x, y, r))
    assert got_routes == routes, (n_nodes, dim, got_routes)
    users.apply(x, y, a=0.75, r=r, b=0.3)
    items.apply(x, y, a=0.75, r=r, b=0.3)
    n_user_rows = check_hop(users, x, y, r, 0.75, 0.3)
    n_item_rows = check_hop(items, x, y, r, 0.75, 0.3)
    assert n_user_rows > 20000 and n_item_rows > 2900
    for stride, srt in strides:
        xs = torch.full((n_nodes, stride), float("nan"), device=device)[:, :dim]
        xs.copy_(x)
        rs = torch.full((n_nodes, stride), float("nan"), device=device)[:, :dim]
        rs.copy_(r)
        ys_full = torch.full((n_nodes, stride), 0x7FA5A5A5, dtype=torch.int32, device=device)
        ys = ys_full.view(torch.float32)[:, :dim]
        assert (users.route(xs, ys, rs), items.route(xs, ys, rs)) == srt, (stride, users.route(xs, ys, rs))
        users.apply(xs, ys, a=0.75, r=rs, b=0.3)
        items.apply(xs, ys, a=0.75, r=rs, b=0.3)
        assert (ys_full[:, dim:] == 0x7FA5A5A5).all(), ("padding of y written", stride)
        assert torch.equal(ys[:nu], y[:nu]), ("user rows", stride)
        if srt[1].startswith("sweep") == routes[1].startswith("sweep"):
            assert torch.equal(ys[nu:], y[nu:]), ("item rows", stride)
        else:
            check_hop(items, xs, ys, rs, 0.75, 0.3)
        del xs, rs, ys, ys_full
    peak = torch.cuda.max_memory_allocated(device) - held
    print(f"boundary D={dim} rows={n_nodes}: routes {got_routes}, peak device memory of the test {peak / 2**30:.2f} GiB")
    del x, r, y, users, items, op
    torch.cuda.empty_cache()


STRIDED_68 = [(69, ("fused_dpp+wt", "sweep_wide+wt")), (71, ("fused_dpp+wt", "sweep_wide+wt")),
              (76, ("fused_dpp+wt", "sweep_wide+wt"))]


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,routes", [(986_894, ("fused_dpp+wt", "sweep_wide+wt")),
                                            (986_895, ("fused_generic+wt", "fused_generic+wt"))])
def test_boundary_d68_padding_id_limit(device, monkeypatch, n_nodes, routes):
    """D=68: the padding id's wrapped offset, 0xFFFFFF * 272 mod 2^32, lies just past 986,894 rows.  Strided tables
    (stride 69 / 71 / 76) move that limit out again."""
    run_boundary(device, monkeypatch, 68, n_nodes, routes, STRIDED_68)


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,routes", [(4_846_750, ("fused_dpp+wt", "sweep_wide+wt")),
                                            (4_846_751, ("fused_generic+wt", "fused_generic+wt"))])
def test_boundary_d90_padding_id_limit(device, monkeypatch, n_nodes, routes):
    run_boundary(device, monkeypatch, 90, n_nodes, routes)


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,routes", [(8_388_607, ("fused_dpp+wt", "sweep_two_pass+wt")),
                                            (8_388_608, ("fused_generic", "fused_generic"))])
def test_boundary_d128_4_gib_limit(device, monkeypatch, n_nodes, routes):
    """D=128: at 2^23 rows the table reaches 4 GiB: the two-pass sweep gives way to generic tiles, sc1 buffer stores
    to plain ones."""
    run_boundary(device, monkeypatch, 128, n_nodes, routes)


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,routes", [(16_777_214, ("fused_dpp+wt", "sweep+wt")),
                                            (16_777_215, ("fused_generic+wt", "fused_generic+wt")),
                                            (16_777_216, ("fused_generic", "fused_generic"))])
def test_boundary_d64_row_id_and_4_gib_limits(device, monkeypatch, n_nodes, routes):
    """D=64: first the 24-bit row id limit (the id 0xFFFFFF is padding), then, one row later, 4 GiB of output."""
    run_boundary(device, monkeypatch, 64, n_nodes, routes)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [(1 << 23) - 1, 1 << 23, (1 << 23) + 1, 1 << 24])
def test_device_row_plan_of_power_of_two_row_ranges(device, n):
    """lgc_row_plan_count scans n + 1 counters; its scratch was sized for n, and ranges of 2^23 and 2^24 rows were
    refused (the D=128 and D=64 boundary graphs above).  The device plan must equal the host's."""
    from gnn_ecommerce_amd.graph import build_row_plan, build_row_plan_device
    deg = torch.zeros(n, dtype=torch.int32)
    deg[[0, 5, n // 2, n - 1]] = torch.tensor([300, 33, 1000, 40], dtype=torch.int32)
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    want = build_row_plan(rowptr, 0, n, 32, 256)
    got = build_row_plan_device(rowptr.to(device), 0, n, 32, 256)
    assert torch.equal(got.chunks.cpu(), want.chunks) and torch.equal(got.multi.cpu(), want.multi)
    assert got.n_slots == want.n_slots and want.n_chunks == 2 + 1 + 4 + 1 and want.n_multi == 2      # 300 and 1000
