"""lgc_apply2 (the band sweep's combine with a second epilogue row): its argument checks, on the host.

Every refused call returns before anything is launched, so fake device pointers do (as in tests/test_routes.py).  The
kernel itself: tests/test_mix_epilogue_gpu.py."""
import ctypes

from test_routes import FAKE, fake_operator
from gnn_ecommerce_amd import _native

E_INVAL, E_DIM, E_ALIGN = -1, -2, -5
ROWS = 5000


def apply2(lib, op, dim=64, x=FAKE, xs=None, y=FAKE + 4096, ys=None, r=FAKE, rs=None, r2=FAKE, r2s=None):
    s = lambda v: dim if v is None else v
    return lib.lgc_apply2(ctypes.byref(op) if op is not None else None, ROWS, x, s(xs), y, s(ys), r, s(rs), r2, s(r2s), 0.25, 0.25,
                          0.25, dim, None)


def test_second_row_needs_the_first():
    lib = _native.load()
    op = fake_operator(groups=4)
    assert apply2(lib, op, r=None) == E_INVAL
    assert apply2(lib, op, r=None, rs=0) == E_INVAL
    assert apply2(lib, op, r2=None) == E_INVAL               # without r2 it is lgc_apply's call


def test_strides_below_the_width():
    lib = _native.load()
    for dim, groups in ((64, 4), (90, 2), (128, 4)):
        op = fake_operator(groups=groups)
        assert apply2(lib, op, dim, r2s=dim - 1) == E_INVAL
        assert apply2(lib, op, dim, rs=dim - 1) == E_INVAL
        assert apply2(lib, op, dim, xs=dim - 1) == E_INVAL
        assert apply2(lib, op, dim, ys=dim - 1) == E_INVAL


def test_alignment_and_missing_tables():
    lib = _native.load()
    op = fake_operator(groups=4)
    assert apply2(lib, op, r2=FAKE + 2) == E_ALIGN
    assert apply2(lib, op, r=FAKE + 2) == E_ALIGN
    assert apply2(lib, op, x=None) == E_INVAL
    assert apply2(lib, op, y=None) == E_INVAL
    assert apply2(lib, op, y=FAKE) == E_INVAL                # out must not alias x
    assert apply2(lib, None) == E_INVAL


def test_only_the_sweep_routes_take_it():
    """Tiles, chunks and rows keep the single row: the route lgc_apply_route names decides, before any launch."""
    lib = _native.load()
    assert apply2(lib, fake_operator()) == E_DIM                          # fused tiles
    assert apply2(lib, fake_operator(tiles=False)) == E_DIM               # rows
    assert apply2(lib, fake_operator(groups=2), 64) == E_DIM              # a two-entry plan does not serve 64 columns
    assert apply2(lib, fake_operator(groups=4), 90) == E_DIM
    assert apply2(lib, fake_operator(groups=4), 20) == E_DIM              # no sweep below 61 columns
    assert apply2(lib, fake_operator(groups=4), 0) == E_DIM               # lgc_apply_route's own error comes back
    for dim, groups in ((64, 4), (90, 2), (128, 4)):
        op = fake_operator(groups=groups)
        route = lib.lgc_apply_route(ctypes.byref(op), ROWS, dim, dim, dim, dim)
        assert _native.route_name(route).startswith("sweep")
        assert apply2(lib, op, dim, r2s=dim - 1) == E_INVAL               # ... and on a sweep route the checks of r2 answer
