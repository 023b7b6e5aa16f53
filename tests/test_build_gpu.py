"""``lgc_build_csr`` bit for bit against the numpy fp32 restatement (tests/build_support.py) at its edge shapes: the
512-entry switch between the two degree kernels, the full and partial steps of the wave kernel, the last rows of a block,
the radix sort's key width at powers of two, E around the block size, ids that fail the range check only as int64, the
A^T build, duplicate edges, and every output and the workspace between guard regions.  tests/test_build_host.py checks
on the CPU that the reference is right and that these cases tell a subtly wrong kernel from a right one."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import build_support as B
from build_support import F32
from gnn_ecommerce_amd import _native
from gnn_ecommerce_amd.graph import PropGraph

pytestmark = pytest.mark.gpu

PAD = 1024            # guard bytes on either side of every buffer (a multiple of the workspace's 256-byte alignment)
FILL = 0xA5
STATUS_BEFORE = 4     # a foreign bit: the build ORs its own in and must leave this one alone


class Guarded:
    """``nbytes`` of device memory between two guard regions, all of it pre-filled with a pattern."""

    def __init__(self, device, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((PAD + self.nbytes + PAD,), FILL, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + PAD

    def view(self, dtype):
        return self.raw[PAD:PAD + self.nbytes].view(dtype)

    def intact(self):
        return bool((self.raw[:PAD] == FILL).all()) and bool((self.raw[PAD + self.nbytes:] == FILL).all())


def run_build(device, case, by_source=False, normalize=True, dis_in=None, weights=True, edge_val=True, deg_dis=True):
    """One ``lgc_build_csr`` on guarded buffers; returns the outputs as numpy arrays in build_ref's form, plus ``code``
    and ``status``.  Asserts the guards."""
    lib = _native.load()
    n, e = case.n, case.edge_index.size(1)
    ei = case.edge_index.contiguous().to(device)
    ew = case.edge_weight.to(device) if (weights and case.edge_weight is not None) else None
    dis_t = None if dis_in is None else torch.from_numpy(np.ascontiguousarray(dis_in, dtype=F32)).to(device)
    ws_bytes = lib.lgc_build_workspace_bytes(n, e)
    assert ws_bytes > 0
    buf = dict(rowptr=Guarded(device, 4 * (n + 1)), entries=Guarded(device, 8 * e), ws=Guarded(device, ws_bytes),
               status=Guarded(device, 4))
    if edge_val:
        buf["edge_val"] = Guarded(device, 4 * e)
    if deg_dis:
        buf["deg"], buf["dis"] = Guarded(device, 4 * n), Guarded(device, 4 * n)
    buf["status"].view(torch.int32).fill_(STATUS_BEFORE)
    assert buf["ws"].ptr % 256 == 0
    opt = lambda k: buf[k].ptr if k in buf else None
    with torch.cuda.device(device):
        code = lib.lgc_build_csr(_native.ptr(ei) if e else None, _native.ptr(ew), n, e, int(by_source), int(normalize),
                                 _native.ptr(dis_t), buf["rowptr"].ptr, buf["entries"].ptr, opt("edge_val"), opt("deg"),
                                 opt("dis"), buf["ws"].ptr, ws_bytes, buf["status"].ptr, _native.stream_of(device))
    torch.cuda.synchronize(device)
    for k, g in buf.items():
        assert g.intact(), f"{case.name}: the build wrote outside {k} ({g.nbytes} bytes)"
    ent = buf["entries"].view(torch.int32).view(e, 2).cpu()
    f = lambda k: buf[k].view(torch.float32).cpu().numpy() if k in buf else None
    return SimpleNamespace(code=code, status=int(buf["status"].view(torch.int32).item()),
                           rowptr=buf["rowptr"].view(torch.int32).cpu().numpy(), cols=ent[:, 0].contiguous().numpy(),
                           vals=ent[:, 1].contiguous().view(torch.float32).numpy(), edge_val=f("edge_val"), deg=f("deg"),
                           dis=f("dis"))


def assert_built(got, want, what, exact_nan=False):
    assert got.code == 0, f"{what}: lgc_build_csr returned {got.code}"
    assert got.status == STATUS_BEFORE, f"{what}: status {got.status}, the build must OR its bits into the word"
    assert B.mismatches(got, want, exact_nan) == [], f"{what}: {B.describe(got, want, exact_nan)}"


_forward = {}


def forward_build(device, name):
    """The forward build of a case on the device, once per session."""
    if name not in _forward:
        _forward[name] = run_build(device, B.forward_cases()[name])
    return _forward[name]


# ----------------------------------------------------------------------------------------
# the forward build
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.FORWARD_NAMES)
def test_forward_build_bit_for_bit(device, name):
    """by_source = 0, normalize = 1, dis_in = NULL: rowptr, columns, values, edge_val, deg and dis equal the reference."""
    got = forward_build(device, name)
    want = B.forward_ref(name)
    assert all(getattr(got, f) is not None for f in B.FIELDS)
    assert_built(got, want, name)


def test_denormal_degree(device):
    """Weights of 1e-42: the degree is a denormal, dis and the values are normal.  hipcc keeps fp32 denormals in adds,
    in the correctly rounded square root and division and in ``__fmul_rn``, as numpy does on the host: equality."""
    case = B.denormal_case()
    got, want = run_build(device, case), case.ref()
    rows = np.flatnonzero(want.deg > 0)
    print("denormal degree: deg bits", [hex(int(v)) for v in B.bits(got.deg)[rows]], "want", [hex(int(v)) for v in B.bits(want.deg)[rows]])
    print("denormal degree: dis", got.dis[rows].tolist(), "want", want.dis[rows].tolist())
    print("denormal degree: values", sorted(set(got.vals.tolist())), "want", sorted(set(want.vals.tolist())))
    assert_built(got, want, case.name)


# ----------------------------------------------------------------------------------------
# the other argument forms
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.OTHER_FORM_NAMES)
def test_transpose_build_from_the_forward_dis(device, name):
    case, fwd = B.forward_cases()[name], forward_build(device, name)
    got = run_build(device, case, by_source=True, dis_in=fwd.dis, edge_val=True, deg_dis=False)
    assert_built(got, case.ref(by_source=True, dis_in=fwd.dis), name + " (A^T)")
    src, dst = case.edge_index.numpy()
    order = np.argsort(src, kind="stable")
    assert np.array_equal(got.cols, dst[order])
    # the same per-edge values as the forward operator, in source order: the exact adjoint
    assert B.same_floats(got.vals, fwd.edge_val[order], exact_nan=True).all()
    assert B.same_floats(got.edge_val, fwd.edge_val, exact_nan=True).all()


@pytest.mark.parametrize("name", B.OTHER_FORM_NAMES)
def test_forward_build_with_a_given_dis(device, name):
    """by_source = 0 with an arbitrary dis_in and deg_out = dis_out = NULL: the values use it, nothing recomputes it."""
    case = B.forward_cases()[name]
    dis_in = np.random.default_rng(7).uniform(0.25, 4.0, size=case.n).astype(F32)
    got = run_build(device, case, dis_in=dis_in, deg_dis=False)
    assert got.deg is None and got.dis is None
    assert_built(got, case.ref(dis_in=dis_in), name + " (given dis)")


@pytest.mark.parametrize("by_source", (False, True))
@pytest.mark.parametrize("name", B.OTHER_FORM_NAMES + ("raw_weights",))
def test_unnormalised_build_carries_the_weight_bits(device, name, by_source):
    case = B.raw_weights_case() if name == "raw_weights" else B.forward_cases()[name]
    got = run_build(device, case, by_source=by_source, normalize=False, deg_dis=False)
    want = case.ref(by_source=by_source, normalize=False)
    assert_built(got, want, f"{name} (normalize = 0, by_source = {int(by_source)})", exact_nan=True)
    assert np.array_equal(B.bits(got.edge_val), B.bits(case.weights())), "NaN payloads, infinities and -0.0 included"


@pytest.mark.parametrize("name", B.OTHER_FORM_NAMES)
def test_build_without_weights_and_without_edge_val(device, name):
    case = B.forward_cases()[name]
    ones = B.Case(name=name + " (edge_weight = NULL)", edge_index=case.edge_index, edge_weight=None, n=case.n)
    assert_built(run_build(device, ones), ones.ref(), ones.name)
    assert_built(run_build(device, ones, by_source=True, normalize=False, deg_dis=False),
                 ones.ref(by_source=True, normalize=False), ones.name + " A^T raw")
    got = run_build(device, case, edge_val=False)
    assert got.edge_val is None
    want = SimpleNamespace(**{**vars(B.forward_ref(name)), "edge_val": None})
    assert_built(got, want, name + " (edge_val = NULL)")


# ----------------------------------------------------------------------------------------
# out of range
# ----------------------------------------------------------------------------------------
def test_out_of_range_edges_are_parked_in_row_zero(device):
    """Six ids that are out of range as int64 (2^32 would be node 0 as int32).  The return code is 0, the status gains
    LGC_ST_INDEX_OOB, the bad edges sit in row 0 as (0, +0.0), and every valid edge that does not touch node 0 has the
    value of the build without them; deg[0], dis[0] and the values that touch node 0 are unspecified and not compared.
    Nothing here can fault: the ids are range-checked before any address is formed from them."""
    case = B.out_of_range_case()
    got, want = run_build(device, case), case.ref()
    assert got.code == 0 and got.status == STATUS_BEFORE | _native.ST_INDEX_OOB
    assert np.array_equal(got.rowptr, want.rowptr) and np.array_equal(got.cols, want.cols)
    src, dst = case.edge_index.numpy()
    perm = np.argsort(np.where(case.valid, dst, 0), kind="stable")
    parked = ~case.valid[perm]
    assert parked.sum() == len(B.BAD_IDS) and (np.flatnonzero(parked) < got.rowptr[1]).all()
    assert (got.cols[parked] == 0).all() and (B.bits(got.vals)[parked] == 0).all()
    assert (B.bits(got.edge_val)[~case.valid] == 0).all()
    clean = run_build(device, case.clean)
    assert_built(clean, case.clean.ref(), "out_of_range_clean")
    away = case.valid & (src != 0) & (dst != 0)                   # valid edges that do not touch node 0
    assert away.sum() > 300
    clean_of = np.cumsum(case.valid) - 1                          # position of a valid edge in the clean graph
    assert B.same_floats(got.edge_val[away], clean.edge_val[clean_of[away]], exact_nan=True).all()
    clean_perm = np.argsort(case.clean.edge_index[1].numpy(), kind="stable")
    pos_clean = np.empty(len(clean_perm), dtype=np.int64)
    pos_clean[clean_perm] = np.arange(len(clean_perm))
    k = np.flatnonzero(away[perm])                                # CSR positions of those edges in the graph with bad edges
    assert B.same_floats(got.vals[k], clean.vals[pos_clean[clean_of[perm[k]]]], exact_nan=True).all()
    assert np.array_equal(got.deg[1:], clean.deg[1:]) and np.array_equal(got.dis[1:], clean.dis[1:])
    # the A^T form parks them the same way
    t = run_build(device, case, by_source=True, dis_in=clean.dis, deg_dis=False)
    assert t.code == 0 and t.status == STATUS_BEFORE | _native.ST_INDEX_OOB
    tw = case.ref(by_source=True, dis_in=clean.dis)
    assert np.array_equal(t.rowptr, tw.rowptr) and np.array_equal(t.cols, tw.cols)
    assert B.same_floats(t.vals, tw.vals).all() and B.same_floats(t.edge_val, tw.edge_val).all()


# ----------------------------------------------------------------------------------------
# through PropGraph
# ----------------------------------------------------------------------------------------
def of_graph(pg, op=None):
    op = pg.forward_op if op is None else op
    h = lambda t: None if t is None else t.cpu().numpy()
    return SimpleNamespace(rowptr=h(op.rowptr), cols=h(op.columns().contiguous()), vals=h(op.values().contiguous()),
                           edge_val=h(pg.edge_values), deg=h(pg.deg), dis=h(pg.dis))


def without(ref, *fields):
    return SimpleNamespace(**{**vars(ref), **{f: None for f in fields}})


def test_propgraph_without_edges(device):
    case = B.forward_cases()["edge_count_e0"]
    pg = PropGraph(case.edge_index.to(device), case.edge_weight.to(device), case.n, keep_edge_values=True)
    assert pg.num_edges == 0 and pg.forward_op.nnz == 0 and pg.split is None
    assert B.mismatches(of_graph(pg), B.forward_ref("edge_count_e0")) == []
    assert (pg.deg == 0).all() and (pg.dis == 0).all() and (pg.forward_op.rowptr == 0).all()


@pytest.mark.parametrize("keep", (False, True))
def test_propgraph_forms(device, keep):
    """edge_weight = None, a transposed (non-contiguous) [E, 2] edge_index, keep_edge_values on and off, the lazily built
    transposed operator."""
    case = B.forward_cases()["key_width_n257"]
    ei_t = case.edge_index.t().contiguous().to(device).t()        # [2, E] view of an [E, 2] tensor
    assert not ei_t.is_contiguous()
    for ew in (case.edge_weight, None):
        c = B.Case(name="propgraph", edge_index=case.edge_index, edge_weight=ew, n=case.n)
        pg = PropGraph(ei_t, None if ew is None else ew.to(device), case.n, keep_edge_values=keep)
        want = c.ref()
        assert (pg.edge_values is not None) == keep
        assert B.mismatches(of_graph(pg), want if keep else without(want, "edge_val")) == [], B.describe(of_graph(pg), want)
        assert pg._transpose_op is None, "A^T is built on first use"
        tp = pg.transpose_op
        assert pg._transpose_op is tp
        tw = c.ref(by_source=True, dis_in=want.dis)
        assert B.mismatches(of_graph(pg, tp), without(tw, "edge_val")) == [], B.describe(of_graph(pg, tp), tw)
        assert int(pg.status[0]) == 0


def test_propgraph_unnormalised(device):
    case = B.forward_cases()["values_mixed"]
    pg = PropGraph(case.edge_index.to(device), case.edge_weight.to(device), case.n, normalize=False, keep_edge_values=True)
    want = case.ref(normalize=False)
    assert B.mismatches(of_graph(pg), want, exact_nan=True, fields=("rowptr", "cols", "vals", "edge_val")) == []
    tw = case.ref(by_source=True, normalize=False)
    assert B.mismatches(of_graph(pg, pg.transpose_op), tw, exact_nan=True, fields=("rowptr", "cols", "vals")) == []


def test_propgraph_builds_clean_after_a_bad_graph(device):
    case = B.out_of_range_case()
    with pytest.raises(IndexError):
        PropGraph(case.edge_index.to(device), case.edge_weight.to(device), case.n)
    clean = case.clean
    pg = PropGraph(clean.edge_index.to(device), clean.edge_weight.to(device), clean.n, keep_edge_values=True)
    assert int(pg.status[0]) == 0
    assert B.mismatches(of_graph(pg), clean.ref()) == [], B.describe(of_graph(pg), clean.ref())
