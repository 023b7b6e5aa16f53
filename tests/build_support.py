"""The graph build restated in numpy fp32, and the graphs that take ``lgc_build_csr`` to its edge shapes
(tests/test_build_host.py, tests/test_build_gpu.py).  numpy and torch on the CPU only.

What the kernels promise (csrc/lgconv_hip.hip, ``k_build_*``) and ``build_ref`` restates:
  order   a stable sort of the edges by target (by source for A^T): edge order is kept inside a row
  deg     ((0 + w_0) + w_1) + ... in fp32 over a row's edges in edge order
  dis     1 / sqrt(deg), both steps correctly rounded; +inf (deg == 0) -> 0, NaN (deg < 0) stays
  val     fl(fl(dis[src] * w) * dis[dst]); with normalize = 0 the weight's bits unchanged
  an edge with an endpoint outside [0, n), tested as int64, is parked: counted in row 0 in its place in edge order, with
  column 0, value +0.0 and edge_val +0.0.  Its weight still enters deg[0]; the header leaves deg[0], dis[0] and the
  values that touch node 0 unspecified once LGC_ST_INDEX_OOB is set, so no test compares those.
Every float is compared by its int32 bit pattern: -0.0 is not +0.0.  A NaN the arithmetic PRODUCES (sqrt of a negative
degree and what it touches) matches a NaN in the same position whatever its sign and payload, which IEEE 754 leaves to
the implementation; a NaN that is only CARRIED (normalize = 0) must keep its bits (``exact_nan=True``).
"""
from types import SimpleNamespace

import numpy as np
import torch

from gnn_ecommerce_amd import synth

F32 = np.float32
U = 2.0 ** -24                       # fp32 unit roundoff
SERIAL_MAX = 512                     # kDegSerialMax: longer rows go to k_build_degree_wave
WAVE = 64
ROWS_PER_WAVE_BLOCK = 4              # kBlock / kWave rows per block of k_build_degree_wave
FIELDS = ("rowptr", "cols", "vals", "edge_val", "deg", "dis")


# ----------------------------------------------------------------------------------------
# the reference, one replaceable step per promise (test_build_host.py swaps in wrong ones)
# ----------------------------------------------------------------------------------------
def step_keys(src, dst, n, by_source):
    """(row key per edge, valid mask): the range check is on the int64 ids."""
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    return np.where(ok, src if by_source else dst, 0), ok


def step_order(key):
    return np.argsort(key, kind="stable")


def step_row_sum(w_row):
    """((0 + w_0) + w_1) + ...: numpy's cumsum is a sequential chain; the leading +0 makes a lone -0.0 come out +0.0."""
    return np.cumsum(np.concatenate([np.zeros(1, F32), w_row]), dtype=F32)[-1]


def step_dis(deg):
    with np.errstate(divide="ignore", invalid="ignore"):
        dis = (F32(1.0) / np.sqrt(deg)).astype(F32)
    dis[dis == np.inf] = 0
    return dis


def step_value(dis_src, w, dis_dst):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return ((dis_src * w).astype(F32) * dis_dst).astype(F32)


STEPS = dict(keys=step_keys, order=step_order, row_sum=step_row_sum, dis=step_dis, value=step_value)


def _np(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def build_ref(edge_index, edge_weight, n, by_source, normalize, dis_in=None, steps=None):
    """What ``lgc_build_csr`` must produce, as numpy arrays: rowptr int32 [n + 1], cols int32 [E], vals fp32 [E]
    (entries in CSR order), edge_val fp32 [E] (original edge order), deg / dis fp32 [n] (None unless computed here:
    normalize with ``dis_in`` None, which the ABI allows for by_source = 0 only)."""
    st = dict(STEPS, **(steps or {}))
    ei = _np(edge_index, np.int64).reshape(2, -1)
    src, dst = ei[0], ei[1]
    n_edges = src.size
    w = np.ones(n_edges, F32) if edge_weight is None else _np(edge_weight, F32)
    key, ok = st["keys"](src, dst, n, by_source)
    perm = st["order"](key)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))]).astype(np.int32)
    deg = dis = None
    if normalize and dis_in is None:
        assert not by_source, "the ABI computes the degree only for the forward build"
        deg = np.zeros(n, F32)
        w_sorted = w[perm]
        for r in np.unique(key):                          # k_build_sorted_weight + k_build_degree_*
            deg[r] = st["row_sum"](w_sorted[rowptr[r]:rowptr[r + 1]])
        dis = st["dis"](deg)
    d = dis if dis_in is None else _np(dis_in, F32)
    edge_val = np.zeros(n_edges, F32)
    if normalize:
        edge_val[ok] = st["value"](d[src[ok]], w[ok], d[dst[ok]])
    else:
        edge_val[ok] = w[ok]
    col = np.where(ok, dst if by_source else src, 0)
    return SimpleNamespace(rowptr=rowptr, cols=col[perm].astype(np.int32), vals=edge_val[perm], edge_val=edge_val,
                           deg=deg, dis=dis)


# ----------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def same_floats(got, want, exact_nan=False):
    """Elementwise: equal bit patterns; unless ``exact_nan``, two NaNs in the same position also match."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    if got.shape != want.shape:
        return np.zeros(max(got.size, want.size, 1), dtype=bool)
    same = bits(got) == bits(want)
    return same if exact_nan else same | (np.isnan(got) & np.isnan(want))


def mismatches(got, want, exact_nan=False, fields=FIELDS):
    """Names of the outputs of ``got`` that differ from ``want`` (both as build_ref returns them); a field that is None
    in ``want`` is not compared."""
    bad = []
    for f in fields:
        w = getattr(want, f)
        if w is None:
            continue
        g = getattr(got, f)
        if g is None:
            bad.append(f)
        elif f in ("rowptr", "cols"):
            if g.shape != w.shape or not np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)):
                bad.append(f)
        elif not same_floats(g, w, exact_nan).all():
            bad.append(f)
    return bad


def describe(got, want, exact_nan=False):
    """First differing position of every mismatching field, for an assertion message."""
    out = []
    for f in mismatches(got, want, exact_nan):
        g, w = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        if g.shape != w.shape:
            out.append(f"{f}: shape {g.shape} != {w.shape}")
            continue
        ne = ~same_floats(g, w, exact_nan) if f not in ("rowptr", "cols") else g.astype(np.int64) != w.astype(np.int64)
        i = int(np.flatnonzero(ne)[0])
        out.append(f"{f}: {int(ne.sum())} of {ne.size} differ, first at {i}: got {g[i]!r} want {w[i]!r}")
    return "; ".join(out)


def ulp_distance(a, b):
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


# ----------------------------------------------------------------------------------------
# other ways to sum a row (what a subtly wrong degree kernel would compute)
# ----------------------------------------------------------------------------------------
def sum_fp64_rounded(w_row):
    return F32(np.sum(w_row.astype(np.float64)))


def sum_blocks(w_row, block=WAVE):
    """Each block of 64 summed sequentially, the partial sums added up in block order."""
    parts = [step_row_sum(w_row[i:i + block]) for i in range(0, len(w_row), block)]
    return step_row_sum(np.array(parts, F32))


def sum_strided(w_row, lanes=WAVE):
    """Lane l sums entries l, l + 64, ... sequentially, the 64 lane sums added up in lane order."""
    parts = [step_row_sum(w_row[l::lanes]) for l in range(lanes)]
    return step_row_sum(np.array(parts, F32))


WRONG_SUMS = dict(fp64=sum_fp64_rounded, blocks=sum_blocks, strided=sum_strided)


def rows_in_edge_order(case):
    """{row: weights of its entries in edge order} of a case's forward build."""
    ei, w = case.edge_index.numpy(), case.weights()
    order = np.argsort(ei[1], kind="stable")
    dst, ws = ei[1][order], w[order]
    return {int(r): ws[dst == r] for r in np.unique(dst)}


# ----------------------------------------------------------------------------------------
# fp64 evaluation and the bound of the fp32 restatement against it (positive weights)
# ----------------------------------------------------------------------------------------
def build_fp64(edge_index, edge_weight, n):
    """(deg, dis, edge_val) of the forward normalised build, every operation in fp64 on the fp32 weights."""
    ei = _np(edge_index, np.int64)
    w = (np.ones(ei.shape[1]) if edge_weight is None else _np(edge_weight, F32)).astype(np.float64)
    deg = np.zeros(n)
    np.add.at(deg, ei[1], w)
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    return deg, dis, dis[ei[0]] * w * dis[ei[1]]


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a product of k factors (1 + d_i), |d_i| <= u."""
    return k * U / (1.0 - k * U)


def value_bound_roundings(len_src, len_dst):
    """How many roundings bound the relative error of one fp32 value against fp64, for POSITIVE weights in the normal range:
      deg of a row of L entries   L - 1 roundings (0 + w_0 is exact), all terms of one sign: relative error <= gamma(L - 1)
      dis = 1 / sqrt(deg)         the degree's error halved by the square root, (1 + d)^-1/2 <= 1 + |d| / 2 + 3 d^2 / 8
                                  (the second-order term is below u for every L <= 8192: one more rounding covers it),
                                  plus one rounding each for the square root and the division
      val = (dis_s * w) * dis_d   two products
    i.e. ceil((L_s - 1 + L_d - 1) / 2) + 2 * (2 + 1) + 2 roundings; the bound is gamma of that."""
    return -(-(max(len_src - 1, 0) + max(len_dst - 1, 0)) // 2) + 2 * 3 + 2


# ----------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------
class Case(SimpleNamespace):
    """name, edge_index (int64 [2, E] torch, CPU), edge_weight (fp32 [E] torch or None), n."""

    def weights(self):
        return np.ones(self.edge_index.size(1), F32) if self.edge_weight is None else self.edge_weight.numpy()

    def ref(self, by_source=False, normalize=True, dis_in=None, steps=None):
        return build_ref(self.edge_index, self.edge_weight, self.n, by_source, normalize, dis_in, steps)


def _case(name, src, dst, w, n, **kw):
    ei = torch.from_numpy(np.stack([np.asarray(src, np.int64), np.asarray(dst, np.int64)]))
    return Case(name=name, edge_index=ei, edge_weight=None if w is None else torch.from_numpy(np.asarray(w, F32).copy()),
                n=int(n), **kw)


def _shuffled(rng, src, dst, w):
    p = rng.permutation(len(src))
    return np.asarray(src)[p], np.asarray(dst)[p], np.asarray(w, F32)[p]


def _draw(rng, size):
    return synth.WEIGHT_VALUES[rng.integers(len(synth.WEIGHT_VALUES), size=size)]


# 1. degree lengths ---------------------------------------------------------------------
DEGREE_LENGTHS = (0, 1, 2, 63, 64, 65, 511, 512, 513, 575, 576, 577, 640, 1023, 1024, 1025, 4097)
DEGREE_N = 602                        # n % 4 == 2: the last block of the wave kernel is partial
# rows longer than 512 entries sit on the first (4k) and last (4k + 3) wave of a block and on the last row; 255 | 256 is
# the block boundary of the serial kernel
DEGREE_ROWS = {513: 0, 575: 7, 576: 100, 577: 103, 640: 256, 1023: 259, 1024: 400, 1025: 403, 4097: DEGREE_N - 1,
               512: 255, 511: 257, 0: 5, 1: 6, 2: 9, 63: 10, 64: 13, 65: 598}
LONG_ROW_MIN = 500                    # "longer than 500 entries": the rows whose sums the cases must discriminate
DEGREE_SEED = 3                       # chosen by seed_report() below; test_build_host.py asserts the condition it meets
ORDER_LENGTHS = tuple(l for l in DEGREE_LENGTHS if l >= 511)


def degree_lengths_case(seed=DEGREE_SEED):
    """One graph whose target rows have exactly the in-degrees DEGREE_LENGTHS at the rows DEGREE_ROWS (every other row:
    0 to 3 entries, so that most sources have a degree), sources random, two entries of every row the same (src, dst)
    pair with different weights, edges shuffled.  About 12 k edges."""
    rng = np.random.default_rng(seed)
    n = DEGREE_N
    length = rng.integers(0, 4, size=n)
    for l, r in DEGREE_ROWS.items():
        length[r] = l
    src, dst, w = [], [], []
    for r in range(n):
        l = int(length[r])
        if l == 0:
            continue
        s, wr = rng.integers(0, n, size=l), _draw(rng, l)
        if l >= 2:
            s[1] = s[0]
            while wr[1] == wr[0]:
                wr[1] = _draw(rng, 1)[0]
        src.append(s), dst.append(np.full(l, r)), w.append(wr)
    src, dst, w = _shuffled(rng, np.concatenate(src), np.concatenate(dst), np.concatenate(w))
    return _case("degree_lengths", src, dst, w, n, rows=dict(DEGREE_ROWS))


# 2. order matters ----------------------------------------------------------------------
ORDER_ROWS = {l: DEGREE_ROWS[l] for l in ORDER_LENGTHS}


def order_matters_case(reverse, seed=11):
    """The rows of at least 511 entries again, each with ONE weight of 1e4 as its first entry in edge order and 1e-4 on
    every later one (``reverse``: the 1e4 comes last).  1e-4 is below half an ulp of 1e4, so the sequential sum of the
    first graph is 1e4 exactly while any sum that adds the small weights to each other first is not; the second graph's
    sequential sum is the well-rounded one, and a kernel that walks a row backwards swaps the two."""
    rng = np.random.default_rng(seed)
    n = DEGREE_N
    src, dst, w = [], [], []
    for l, r in ORDER_ROWS.items():
        wr = np.full(l, 1e-4, F32)
        wr[-1 if reverse else 0] = 1e4
        src.append(rng.integers(0, n, size=l)), dst.append(np.full(l, r)), w.append(wr)
    src, dst, w = (np.concatenate(a) for a in (src, dst, w))
    # the rows are dealt into each other in a random interleaving; every row keeps its own order
    turn = rng.permutation(np.repeat(np.arange(len(ORDER_ROWS)), [l for l in ORDER_ROWS]))
    starts = np.concatenate([[0], np.cumsum([l for l in ORDER_ROWS])])[:-1]
    taken = np.zeros(len(ORDER_ROWS), dtype=np.int64)
    order = np.empty(len(turn), dtype=np.int64)
    for i, t in enumerate(turn):
        order[i] = starts[t] + taken[t]
        taken[t] += 1
    return _case("order_matters_" + ("small_first" if reverse else "big_first"), src[order], dst[order], w[order], n,
                 rows=dict(ORDER_ROWS))


# 3. key width --------------------------------------------------------------------------
KEY_WIDTH_N = (1, 2, 3, 255, 256, 257, 65535, 65536, 65537)


def key_width_case(n, seed=21, n_edges=3000):
    """About 3,000 edges on n nodes; targets and sources alternate between the ids around the powers of two
    {0, 1, n/2 - 1, n/2, n - 2, n - 1} and random ones.  n = 1 is self-loops only."""
    rng = np.random.default_rng(seed + n)
    special = np.unique(np.clip(np.array([0, 1, n // 2 - 1, n // 2, n - 2, n - 1]), 0, n - 1))

    def ids():
        a = rng.integers(0, n, size=n_edges)
        a[::2] = special[rng.integers(0, len(special), size=len(a[::2]))]
        return a
    dst = ids()
    src = np.roll(ids(), 1)                       # a special target meets a random source and the other way round
    return _case(f"key_width_n{n}", src, dst, _draw(rng, n_edges), n)


# 4. edge count -------------------------------------------------------------------------
EDGE_COUNTS = (0, 1, 255, 256, 257, 513)


def edge_count_case(n_edges, seed=31):
    rng = np.random.default_rng(seed + n_edges)
    return _case(f"edge_count_e{n_edges}", rng.integers(0, 7, size=n_edges), rng.integers(0, 7, size=n_edges),
                 _draw(rng, n_edges), 7)


# 5. values -----------------------------------------------------------------------------
V_ZERO, V_CANCEL, V_NEG, V_MINUS_ZERO, V_LOOP, V_LONE_MINUS_ZERO, V_ISOLATED = 2, 3, 4, 5, 6, 19, (20, 21, 22)


def values_mixed_case(seed=41):
    """23 nodes: node 2's incoming weights are all 0 (deg 0, dis 0, values +0, no NaN); node 3's cancel to exactly 0
    (w and -w); node 4 has a negative degree (dis NaN, NaN on exactly the entries that touch it); node 5 receives a -0.0
    weight among positive ones and node 19 nothing but one (deg = 0 + -0.0 = +0.0, value -0.0); node 6 has self-loops; nodes
    20 .. 22 are isolated; the others form a random graph, with
    edges from and to every special node."""
    rng = np.random.default_rng(seed)
    n = 23
    e = [(7, V_ZERO, 0.0), (8, V_ZERO, 0.0), (V_ZERO, V_ZERO, 0.0),
         (9, V_CANCEL, 0.11), (10, V_CANCEL, -0.11),
         (12, V_NEG, -1.0), (13, V_NEG, 0.5), (V_NEG, V_NEG, -0.02),
         (14, V_MINUS_ZERO, -0.0), (15, V_MINUS_ZERO, 0.03), (16, V_MINUS_ZERO, 0.1),
         (V_LOOP, V_LOOP, 0.5), (V_LOOP, V_LOOP, 0.01), (17, V_LOOP, 1.0), (14, V_LONE_MINUS_ZERO, -0.0)]
    for s in (V_ZERO, V_CANCEL, V_NEG, V_MINUS_ZERO, V_LOOP):           # the special nodes as sources of ordinary rows
        for d in rng.integers(7, 19, size=2):
            e.append((s, int(d), float(_draw(rng, 1)[0])))
    e.append((V_NEG, V_ZERO, 0.0)), e.append((V_ZERO, V_NEG, 0.1)), e.append((V_CANCEL, V_NEG, 0.1))
    for _ in range(60):
        e.append((int(rng.integers(7, 19)), int(rng.integers(7, 19)), float(_draw(rng, 1)[0])))
    src, dst, w = _shuffled(rng, [x[0] for x in e], [x[1] for x in e], [x[2] for x in e])
    return _case("values_mixed", src, dst, w, n)


def values_tiny_huge_case(seed=42):
    """Two components: weights of 1e-30 on nodes 0 .. 9, of 1e30 on nodes 10 .. 19.  deg ~ 1e-30 / 1e30, dis ~ 1e15 / 1e-15,
    dis * w ~ 1e-15 / 1e15, values ~ 1: every intermediate stays in the normal range."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, 10, size=40), rng.integers(10, 20, size=40)])
    dst = np.concatenate([rng.integers(0, 10, size=40), rng.integers(10, 20, size=40)])
    w = np.concatenate([np.full(40, 1e-30, F32), np.full(40, 1e30, F32)])
    return _case("values_tiny_huge", *_shuffled(rng, src, dst, w), 20)


RAW_BITS = np.array([0x7FC01234, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x3F800000, 0x7FA00000],
                    dtype=np.uint32)       # two quiet NaNs with payloads, +-inf, -0.0, the smallest denormal, 1, a signalling NaN


def raw_weights_case(seed=43):
    """normalize = 0 only: the weights' bits must come through unchanged (NaNs with payloads, +-inf, -0.0)."""
    rng = np.random.default_rng(seed)
    n_edges = 40
    w = RAW_BITS[rng.integers(0, len(RAW_BITS), size=n_edges)]
    w[:len(RAW_BITS)] = RAW_BITS
    return _case("raw_weights", rng.integers(0, 9, size=n_edges), rng.integers(0, 9, size=n_edges), w.view(F32), 9)


# 6. denormal degree --------------------------------------------------------------------
def denormal_case(seed=51):
    """Weights of 1e-42 (a denormal fp32): rows of 1, 3, 70 and 600 entries on 8 nodes.  deg stays denormal (its sums are
    exact: multiples of 2^-149), dis ~ 1e21 and the values ~ 1 are normal."""
    rng = np.random.default_rng(seed)
    dst = np.concatenate([np.full(l, r) for r, l in ((1, 1), (2, 3), (4, 70), (7, 600))])
    src = rng.choice(np.array([1, 2, 4, 7]), size=len(dst))
    w = np.full(len(dst), 1e-42, F32)
    return _case("denormal_degree", *_shuffled(rng, src, dst, w), 8)


# 7. out of range -----------------------------------------------------------------------
BAD_IDS = (-1, None, 2 ** 31, 2 ** 32, 2 ** 32 + 1, -2 ** 63)      # None: n itself


def out_of_range_case(seed=61, n=50, n_valid=400):
    """A valid graph plus six bad edges, one id each of BAD_IDS, alternately as source and as target, the other endpoint a
    valid node other than 0; they sit between the valid edges.  ``valid`` marks the valid edges; ``clean`` is the graph
    without the bad ones."""
    rng = np.random.default_rng(seed)
    src, dst, w = rng.integers(0, n, size=n_valid), rng.integers(0, n, size=n_valid), _draw(rng, n_valid)
    clean = _case("out_of_range_clean", src, dst, w, n)
    at = np.sort(rng.choice(np.arange(1, n_valid), size=len(BAD_IDS), replace=False))
    src, dst, w = list(src), list(dst), list(w)
    valid = [True] * n_valid
    for k, (pos, bad) in enumerate(zip(at[::-1], BAD_IDS[::-1])):       # insert from the back: positions stay put
        bad = n if bad is None else bad
        other = int(rng.integers(1, n))
        s, d = (bad, other) if k % 2 == 0 else (other, bad)
        src.insert(pos, s), dst.insert(pos, d), w.insert(pos, F32(0.5)), valid.insert(pos, False)
    return _case("out_of_range", src, dst, w, n, valid=np.array(valid), clean=clean)


# ----------------------------------------------------------------------------------------
_cache = {}


def forward_cases():
    """name -> case of generators 1 to 5 (every one built normalised, by target), made once."""
    if "forward" not in _cache:
        cases = [degree_lengths_case(), order_matters_case(False), order_matters_case(True)]
        cases += [key_width_case(n) for n in KEY_WIDTH_N]
        cases += [edge_count_case(e) for e in EDGE_COUNTS]
        cases += [values_mixed_case(), values_tiny_huge_case()]
        _cache["forward"] = {c.name: c for c in cases}
    return _cache["forward"]


FORWARD_NAMES = (["degree_lengths", "order_matters_big_first", "order_matters_small_first"]
                 + [f"key_width_n{n}" for n in KEY_WIDTH_N] + [f"edge_count_e{e}" for e in EDGE_COUNTS]
                 + ["values_mixed", "values_tiny_huge"])
POSITIVE_NAMES = [n for n in FORWARD_NAMES if not n.startswith(("order_matters", "values_mixed"))]
OTHER_FORM_NAMES = ("key_width_n257", "degree_lengths", "values_mixed")      # one key-width, one degree, one value case


def forward_ref(name):
    """The reference of a forward case, computed once and shared (callers must not write into it)."""
    key = ("ref", name)
    if key not in _cache:
        _cache[key] = forward_cases()[name].ref()
    return _cache[key]


def seed_report(seeds=range(64)):
    """Which seeds of degree_lengths_case make every long row's sequential sum differ from all of WRONG_SUMS."""
    good = []
    for s in seeds:
        rows = rows_in_edge_order(degree_lengths_case(s))
        if all(bits(step_row_sum(wr)) != bits(f(wr)) for wr in rows.values() if len(wr) > LONG_ROW_MIN for f in WRONG_SUMS.values()):
            good.append(s)
    return good
