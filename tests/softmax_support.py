"""What the softmax-loss tests share (tests/test_softmax_host.py, tests/test_softmax_gpu.py): the admissibility rule of
lgc_softmax_batch in Python integers, the float64 reference of loss, G, grad_users and grad_cands from a given fp32 score
panel, the DERIVED element-wise bounds, poisoned input buffers and guarded output buffers, and the
case table.  Nothing here touches a device.

Bounds count roundings; u = 2^-24 is the unit roundoff of fp32, an ulp is at most 2 u relative.  The kernel calls expf and
logf of the device library, whose documented accuracy (the OpenCL C full-profile table it implements) is 3 ulp each."""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
ULP = 2.0 * U                 # one ulp, relative, at most
E_EXP = 3 * ULP               # expf: <= 3 ulp
E_LOG = 3 * ULP               # logf: <= 3 ulp
TINY = 2.0 ** -126            # a result below the normal range may be flushed to zero
SECOND = 1.0 + 2.0 ** -10     # covers the products of two error terms, each below 2^-10
WAVE, BLOCK = 64, 256
ST_INDEX_OOB = 1

# the geometry of csrc/lgconv_softmax.hip the case table has to reach both sides of
ROW_TILE, CAND_TILE, DIM_CHUNK, DIM_GROUP = 64, 128, 32, 16          # k_sm_logits
PROD_ROWS, PROD_COLS, PROD_INNER = 16, 64, 64                         # k_sm_product


def f32(a):
    return np.asarray(a, dtype=np.float32)


def gamma(k):
    """k roundings in a row: (1 + u)^k - 1 <= k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


# ----------------------------------------------------------------------------------------
# the admissible sets, in Python integers
# ----------------------------------------------------------------------------------------
def admissible(users, cands, target, split, n, ign):
    """(adm bool [B, C], valid bool [B], status): J_i as include/lgconv_hip.h states it.  ``ign``: (ptr, items) or None."""
    b, c = len(users), len(cands)
    adm = np.zeros((b, c), dtype=bool)
    valid = np.zeros(b, dtype=bool)
    status = 0
    cand_ok = [split <= int(x) < n for x in cands]
    if not all(cand_ok):
        status |= ST_INDEX_OOB
    for i in range(b):
        u, t = int(users[i]), int(target[i])
        if not (0 <= u < split and 0 <= t < c and cand_ok[t]):
            status |= ST_INDEX_OOB
            continue
        valid[i] = True
        ignored = set()
        if ign is not None:
            ignored = set(int(x) for x in ign[1][int(ign[0][u]):int(ign[0][u + 1])])
        for j in range(c):
            adm[i, j] = j == t or (cand_ok[j] and int(cands[j]) != int(cands[t]) and int(cands[j]) not in ignored)
    return adm, valid, status


# ----------------------------------------------------------------------------------------
# the float64 reference and its bounds, from the fp32 score panel
# ----------------------------------------------------------------------------------------
def logits(scores, inv_tau, bias):
    """z as the kernel forms it from the panel's bits: one rounded multiply, then one rounded add."""
    with np.errstate(all="ignore"):
        z = f32(scores) * np.float32(inv_tau)
        if bias is not None:
            z = z + f32(bias)[None, :]
    return f32(z)


def reference(z, adm, valid, target, inv_tau, size):
    """From fp32 logits z [B, C]: a namespace of float64 ``row_loss`` [B], ``loss``, ``g`` [B, C], int ``n_adm`` [B], the
    bounds ``b_row``, ``b_loss``, ``b_g`` of the kernel's fp32 evaluation, and ``nan_rows`` (rows with a NaN or +inf among
    their admissible logits: NaN row loss, NaN in the admissible elements of G, NaN loss)."""
    b, c = z.shape
    z64 = z.astype(np.float64)
    scale = float(np.float32(inv_tau)) / float(size)
    row_loss, b_row = np.zeros(b), np.zeros(b)
    g, b_g = np.zeros((b, c)), np.zeros((b, c))
    n_adm = np.zeros(b, dtype=np.int64)
    nan_rows = np.zeros(b, dtype=bool)
    depth = math.ceil(c / WAVE) + 6                    # additions a term of S passes: the lane's chain, six butterfly levels
    with np.errstate(all="ignore"):
        for i in range(b):
            if not valid[i]:
                continue
            cols = np.flatnonzero(adm[i])
            n_adm[i] = cols.size - 1
            t = int(target[i])
            zi = z64[i, cols]
            if np.isnan(zi).any() or np.isposinf(zi).any():
                nan_rows[i] = True
                row_loss[i] = np.nan
                g[i, cols] = np.nan
                continue
            m = zi.max()
            d = zi - m
            w = np.exp(d)
            rel_e = (np.abs(d) * U + E_EXP) * SECOND   # the rounded subtraction moves exp by |d| u, expf adds its own
            rel_e = np.where(np.isfinite(d), rel_e, 0.0)   # exp(-inf) is exactly 0
            s = w.sum()
            err_s = (w * rel_e + TINY).sum() + gamma(depth) * s
            rho = err_s / s / (1.0 - err_s / s)
            row_loss[i] = (m - z64[i, t]) + math.log(s)
            b_row[i] = (U * abs(m - z64[i, t]) + rho + E_LOG * abs(math.log(s)) + U * abs(row_loss[i])) * SECOND + TINY
            p = w / s
            err_p = p * (rel_e + rho + U) + TINY
            a = p - (cols == t)
            g[i, cols] = a * scale
            b_g[i, cols] = ((err_p + U * np.abs(a)) * scale + 2 * U * np.abs(a) * scale) * SECOND + TINY
        finite = np.isfinite(row_loss)
        loss = np.nan if nan_rows.any() else row_loss[valid].sum() / size          # a row at +inf makes the loss +inf
        depth_rows = math.ceil(b / BLOCK) + 8          # a thread's chain, eight tree levels
        inner = b_row[valid & finite].sum() + gamma(depth_rows) * np.abs(row_loss[valid & finite]).sum()
        b_loss = (inner / size + U * abs(loss)) * SECOND + TINY if np.isfinite(loss) else np.nan
    return SimpleNamespace(row_loss=row_loss, loss=loss, g=g, n_adm=n_adm, b_row=b_row, b_loss=b_loss, b_g=b_g, nan_rows=nan_rows)


def product_reference(g_bits, rows, transpose):
    """(out float64, bound): the product of the kernel's OWN fp32 G with fp32 table rows (zeros for an id out of range), and
    the bound of a chain of K fused or unfused multiply-adds: every term passes at most K + 1 roundings."""
    a = g_bits.astype(np.float64)
    if transpose:
        a = a.T
    r = rows.astype(np.float64)
    k = a.shape[1]
    with np.errstate(all="ignore"):
        out = a @ r
        mag = np.abs(a) @ np.abs(r)
        big = lambda m: np.abs(m[np.isfinite(m)]).max() if np.isfinite(m).any() else 0.0
        peak = 1.0 + big(a) + big(r)                   # of the finite factors: a NaN or infinite term is compared as such
        bound = gamma(k + 1) * mag + (k + 1) * TINY * peak
    return out, bound


# ----------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------
def poisoned(table, stride, offset):
    """A flat fp32 buffer holding ``table``'s rows ``stride`` floats apart from float ``offset`` on, NaN in every other float
    (the padding columns, the floats before the first row, 64 floats behind the last)."""
    rows, dim = table.shape
    flat = np.full(offset + rows * stride + 64, np.nan, dtype=np.float32)
    view = flat[offset:offset + rows * stride].reshape(rows, stride)
    view[:, :dim] = table
    return flat


SENTINEL = -7.25


def guarded_shape(rows, stride):
    """Floats of an output buffer with one guard row of ``stride`` floats before and behind ``rows`` rows."""
    return (rows + 2) * stride


def check_guarded(flat, rows, width, stride, name):
    """The [rows, width] block of a guarded buffer; every float around it must still hold the sentinel."""
    grid = np.asarray(flat).reshape(rows + 2, stride)
    assert (grid[0] == SENTINEL).all() and (grid[-1] == SENTINEL).all(), f"{name}: written before or behind the rows"
    assert (grid[1:-1, width:] == SENTINEL).all(), f"{name}: written past column {width}"
    return grid[1:-1, :width]


# ----------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------
N_USERS, N_ITEMS = 40, 300
N = N_USERS + N_ITEMS
LAYOUTS = {"dense": (0, 0), "padded": (7, 0), "misaligned": (3, 1)}      # (extra floats per row, floats before row 0)
IGN_FORMS = ("null", "empty", "long", "hits")


def case(name, n_rows, n_cand, dim, layout="dense", ign="null", bias=False, inv_tau=1.0, kind="random", seed=None):
    return SimpleNamespace(name=name, n_rows=n_rows, n_cand=n_cand, dim=dim, layout=layout, ign=ign, bias=bias, inv_tau=inv_tau,
                           kind=kind, seed=seed if seed is not None else 1000 + 7 * n_rows + 13 * n_cand + dim)


CASES = [
    case("r1_c1_d4", 1, 1, 4),
    case("r2_c2_d61_padded_empty", 2, 2, 61, "padded", "empty"),
    case("r63_c127_d64_hits", 63, 127, 64, "dense", "hits", inv_tau=4.0),
    case("r64_c128_d64_misaligned_hits_bias", 64, 128, 64, "misaligned", "hits", bias=True, inv_tau=2.5),
    case("r65_c129_d68_padded_long", 65, 129, 68, "padded", "long", inv_tau=3.0),
    case("r130_c260_d90_padded_hits_bias", 130, 260, 90, "padded", "hits", bias=True, inv_tau=5.0),
    case("r130_c129_d128_long", 130, 129, 128, "dense", "long", inv_tau=0.5),
    case("r65_c260_d256_misaligned_hits", 65, 260, 256, "misaligned", "hits"),
    case("r64_c64_d90", 64, 64, 90),
    case("r65_c65_d90_misaligned_empty_bias", 65, 65, 90, "misaligned", "empty", bias=True),
    case("r17_c63_d64_hits", 17, 63, 64, "dense", "hits"),
    case("r16_c2_d128_padded", 16, 2, 128, "padded"),
    case("r2_c260_d4_long", 2, 260, 4, "dense", "long", inv_tau=10.0),
    case("r130_c1_d64", 130, 1, 64),
    case("r1_c260_d90_hits", 1, 260, 90, "dense", "hits", inv_tau=7.0),
    case("r63_c127_d61_misaligned_long_bias", 63, 127, 61, "misaligned", "long", bias=True),
    # widths of one, two and three 16-column groups: one chunk, and two chunks whose second holds ONE group
    case("r65_c129_d16_hits", 65, 129, 16, "dense", "hits", inv_tau=2.0),
    case("r65_c129_d17_misaligned_long_bias", 65, 129, 17, "misaligned", "long", bias=True, inv_tau=3.0),
    case("r65_c129_d33_padded_hits", 65, 129, 33, "padded", "hits", inv_tau=1.5),
    case("r65_c129_d48_empty_bias", 65, 129, 48, "dense", "empty", bias=True),
    case("r65_c129_d49_padded_hits", 65, 129, 49, "padded", "hits", inv_tau=6.0),
    case("spread_r65_c129_d64_hits", 65, 129, 64, "dense", "hits", inv_tau=400.0, kind="spread"),
    case("bad_ids_r65_c129_d64_hits", 65, 129, 64, "padded", "hits", kind="bad"),
    case("nonfinite_r65_c129_d64", 65, 129, 64, "dense", "empty", bias=True, kind="nonfinite"),
]
CASE_NAMES = [c.name for c in CASES]
NONFINITE_USERS = {3: "nan", 5: "inf"}                     # user rows of the "nonfinite" case that hold a NaN / huge values
MINUS_INF_COLUMN = 7
BAD_USERS = [-1, N_USERS, 2 ** 40, -2 ** 40]
BAD_CANDS = [N_USERS - 1, N, -5, 2 ** 40, 0]
BAD_TARGETS = [-1, None]                                   # None: n_cand itself


def build(c):
    """The inputs of a case, in numpy: table [N, dim], users, cands, target, ign (ptr int32, items int64) or None, bias."""
    rng = np.random.default_rng(c.seed)
    table = f32(rng.standard_normal((N, c.dim)) * (0.35 if c.kind != "spread" else 0.5) / math.sqrt(c.dim / 16))
    users = rng.integers(0, N_USERS, c.n_rows)
    cands = N_USERS + rng.integers(0, N_ITEMS, c.n_cand)
    if c.n_cand >= 4:
        cands[c.n_cand // 2] = cands[1]                    # an item listed twice: the copy of a target is no negative
    target = rng.integers(0, c.n_cand, c.n_rows)
    if c.n_cand >= 4 and c.n_rows >= 2:
        target[1] = 1                                      # ... and row 1 has that item for its positive
    lo, hi = int(cands.min()), int(cands.max())
    ign = None
    if c.ign != "null":
        lists = {}
        for u in range(N_USERS):
            if c.ign == "empty":
                lists[u] = []
            elif c.ign == "hits":                          # first and last entry are candidates; some in between
                mid = rng.choice(np.arange(lo, hi + 1), size=min(hi - lo + 1, 1 + int(rng.integers(0, 40))), replace=False)
                lists[u] = sorted(set(mid.tolist()) | {lo, hi})
            else:                                          # "long": user of row 0 ignores the whole catalogue
                take = rng.choice(np.arange(N_USERS, N), size=int(rng.integers(0, 30)), replace=False)
                lists[u] = sorted(take.tolist())
        if c.ign == "long":
            lists[int(users[0])] = list(range(N_USERS, N))
        ptr = np.zeros(N_USERS + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(lists[u]) for u in range(N_USERS)])
        items = np.array([x for u in range(N_USERS) for x in lists[u]], dtype=np.int64)
        ign = (ptr, items)
    bias = f32(rng.standard_normal(c.n_cand)) if c.bias else None
    users, cands, target = users.astype(np.int64), cands.astype(np.int64), target.astype(np.int32)
    if c.kind == "bad":
        for k, u in enumerate(BAD_USERS):
            users[3 + 2 * k] = u
        for k, x in enumerate(BAD_CANDS):
            cands[5 + 3 * k] = x
        target[20] = -1
        target[21] = c.n_cand
        target[22] = 5                                     # a valid column that holds no item
        target[23] = 2 ** 31 - 1
    if c.kind == "nonfinite":
        for u, what in NONFINITE_USERS.items():
            if what == "nan":
                table[u, c.dim // 2] = np.nan
            else:
                table[u, 0] = 3e38
        table[N_USERS:, 0] = np.where(np.arange(N_ITEMS) % 2 == 0, 1e3, -1e3)   # the huge row scores +inf and -inf
        users[:8] = [3, 0, 5, 1, 3, 2, 5, 4]               # rows 0, 4: NaN; rows 2, 6: +-inf; neighbours finite
        bias[MINUS_INF_COLUMN] = -np.inf                   # a column at -inf contributes 0 to every row ...
        target[target == MINUS_INF_COLUMN] = 0
        users[8:10] = [7, 6]
        target[9] = MINUS_INF_COLUMN                       # ... and as a target beside finite logits gives loss +inf
    return SimpleNamespace(case=c, table=table, users=users, cands=cands, target=target, ign=ign, bias=bias, split=N_USERS, n=N)


def stride_of(c):
    return c.dim + LAYOUTS[c.layout][0]


def offset_of(c):
    return LAYOUTS[c.layout][1]
