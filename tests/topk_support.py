"""Reference, route rule and case table for the serving tail, lgc_mask_topk (tests/test_topk_host.py and
tests/test_topk_gpu.py).  Everything here is numpy; no project code is imported.

The order the kernel promises ("Top-k order"): every NaN first, then +inf, the finite values descending with
-0 and +0 equal, then -inf; equal elements by ascending index.  ``topk_ref`` states it as a partition and a stable sort.
``topk_route`` restates which of the kernel's three routes a row takes; only the host tests use it, to prove that the
case table reaches every route -- the device tests never branch on it."""
import numpy as np

BLOCK = 1024                 # threads of the one workgroup that owns a row; thread = column mod BLOCK
REGS_COLS = 64 * BLOCK       # widest row whose keys stay in registers
SHORT_MAX = 512              # longest candidate list the short cut ranks by counting
LIST_COLS_MAX = 983040       # widest row the list form of the mask takes (120 KiB of LDS, one bit per column)
K_MAX = 256


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def from_bits(words):
    """fp32 values from their bit patterns: NaNs of either sign and any payload, written without arithmetic."""
    return np.asarray(words, dtype=np.uint32).view(np.float32)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------
def masked_ref(scores, seen):
    """fp32 scores * (1 - seen): one subtract and one multiply, each rounded once.  ``seen`` None: the scores."""
    s = np.asarray(scores, dtype=np.float32)
    if seen is None:
        return np.array(s, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = np.float32(1.0) - np.asarray(seen, dtype=np.float32)
        return (s * keep).astype(np.float32)


def topk_ref(masked, k):
    """(indices int64 [rows, k], values fp32 [rows, k]) by (value descending, index ascending), every NaN ahead of +inf."""
    masked = np.asarray(masked, dtype=np.float32)
    one_row = masked.ndim == 1
    rows = masked.reshape(1, -1) if one_row else masked
    assert 1 <= k <= rows.shape[1]
    idx = np.empty((rows.shape[0], k), dtype=np.int64)
    for r, x in enumerate(rows):
        is_nan = np.isnan(x)
        if is_nan.any():
            nans, rest = np.flatnonzero(is_nan), np.flatnonzero(~is_nan)
            order = np.concatenate([nans, rest[np.argsort(-(x[rest] + np.float32(0.0)), kind="stable")]])
        else:
            order = np.argsort(-(x + np.float32(0.0)), kind="stable")
        idx[r] = order[:k]
    val = np.take_along_axis(rows, idx, axis=1)
    return (idx[0], val[0]) if one_row else (idx, val)


def values_match(got, want):
    """The same bit patterns, except that any NaN matches any NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(both_nan | (bits_of(got) == bits_of(want)).reshape(got.shape)))


# ----------------------------------------------------------------------------------------
# which route a row takes
# ----------------------------------------------------------------------------------------
def order_keys(row):
    """uint32 keys ascending with the order above: a NaN gets the top key, the rest the usual sign fold of x + 0; lifted to
    >= 1 (0 is the key of the padding past the row end)."""
    x = np.asarray(row, dtype=np.float32)
    with np.errstate(invalid="ignore"):                               # a signalling NaN in, a quiet one out
        u = bits_of(x + np.float32(0.0)).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    key = np.where(np.isnan(x), 0xFFFFFFFF, key)
    return np.maximum(key, 1).astype(np.uint32)


def topk_route(masked_row, k):
    """("short" | "regs_radix" | "stream", candidates).  Rows wider than REGS_COLS stream (no candidate list: None).
    Otherwise the k-th largest of the BLOCK per-thread maxima (thread = column mod BLOCK) names an 11-bit bin of the key;
    the candidates are the elements in or above that bin, and up to SHORT_MAX of them are ranked by counting."""
    x = np.asarray(masked_row, dtype=np.float32).reshape(-1)
    n = x.size
    assert 1 <= k <= n
    if n > REGS_COLS:
        return "stream", None
    keys = np.zeros(-(-n // BLOCK) * BLOCK, dtype=np.uint32)
    keys[:n] = order_keys(x)
    thread_max = keys.reshape(-1, BLOCK).max(axis=0)
    kth = np.sort(thread_max)[::-1][k - 1]
    low = max(int(kth >> 21) << 21, 1)
    count = int(np.count_nonzero(keys[:n] >= low))
    return ("short" if count <= SHORT_MAX else "regs_radix"), count


def tie_cut(masked_row, k):
    """(equal, need, slices): the elements equal to the k-th one (all NaNs count as equal), how many of them fit, and the
    number of BLOCK-column slices the ones that fit lie in.  A tie is cut when equal > need."""
    x = np.asarray(masked_row, dtype=np.float32).reshape(-1)
    idx, val = topk_ref(x, k)
    kth = val[-1]
    same = np.isnan(x) if np.isnan(kth) else (x == kth)
    n_above = int(np.count_nonzero(~same[idx]))
    need = k - n_above
    taken = np.flatnonzero(same)[:need]
    return int(same.sum()), need, int(np.unique(taken // BLOCK).size)


# ----------------------------------------------------------------------------------------
# masks
# ----------------------------------------------------------------------------------------
class Lists:
    """The list form of a mask: CSR over users (ptr int64 [n_users + 1], items int64), and the user of each row (None: row r
    is user r)."""

    def __init__(self, ptr, items, rows):
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        self.items = np.ascontiguousarray(items, dtype=np.int64)
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)

    def dense(self, n_rows, n_cols):
        """The 0 / 1 mask the lists stand for; entries outside [0, n_cols) are ignored, a repeated one counts once."""
        out = np.zeros((n_rows, n_cols), dtype=np.float32)
        for r in range(n_rows):
            u = r if self.rows is None else int(self.rows[r])
            it = self.items[self.ptr[u]:self.ptr[u + 1]]
            out[r, it[(it >= 0) & (it < n_cols)]] = 1.0
        return out


def lists_of(mask01, rng, with_rows, junk=False):
    """Lists of a 0 / 1 mask.  ``with_rows``: the rows are users 2 r + 1 of a table of 2 rows + 2 users (the others have
    lists of their own, which must not be read); otherwise row r is user r.  ``junk``: every list also gets its first
    entry a second time and three entries outside [0, n_cols) -- n_cols, -1 and 2^40 + 3, whose low 32 bits name a column."""
    n_rows, n_cols = mask01.shape
    per_row = []
    for r in range(n_rows):
        it = np.flatnonzero(mask01[r]).astype(np.int64)
        if junk:
            it = np.concatenate([[n_cols, -1], it, it[:1], [2 ** 40 + 3]]).astype(np.int64)
        per_row.append(it)
    if not with_rows:
        users = per_row
        rows = None
    else:
        users = []
        for it in per_row:
            users += [rng.integers(0, n_cols, size=5).astype(np.int64), it]
        users += [rng.integers(0, n_cols, size=3).astype(np.int64)] * 2
        rows = 2 * np.arange(n_rows, dtype=np.int64) + 1
    ptr = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum([len(u) for u in users], out=ptr[1:])
    items = np.concatenate(users) if ptr[-1] else np.zeros(1, dtype=np.int64)
    return Lists(ptr, items, rows)


def random_mask(rng, scores, share=0.1, top=3):
    """A 0 / 1 mask with ``share`` of the columns seen, among them the ``top`` best of each row: the mask changes the answer."""
    rows, cols = scores.shape
    mask = (rng.random((rows, cols)) < share).astype(np.float32)
    top = min(top, cols)
    if top:
        best, _ = topk_ref(scores, top)
        np.put_along_axis(mask, best, 1.0, axis=1)
    return mask


# ----------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------
class Case:
    """scores fp32 [rows, cols] (possibly a column slice of a wider table), the ks to ask for, and the masks to run it
    under: ``forms`` is a list of (name, dense mask or None, Lists or None).  ``claims`` is a list of
    (form name, row, k, route, candidates or None): what the case is in the table for; the host test checks each.
    ``tie_slices``: {(form name, row, k): least number of slices the cut tie must span}."""

    def __init__(self, scores, ks, forms, claims=(), tie_slices=None):
        self.scores, self.ks, self.forms = scores, tuple(ks), list(forms)
        self.claims, self.tie_slices = list(claims), dict(tie_slices or {})

    def masked(self, form):
        """The fp32 row values the kernel ranks under one of the case's forms."""
        for name, dense, lists in self.forms:
            if name == form:
                if lists is not None:
                    dense = lists.dense(*self.scores.shape)
                return masked_ref(self.scores, dense)
        raise KeyError(form)


def usual_forms(rng, scores, lists_with_rows=True):
    """No mask, a random 0 / 1 mask that hides each row's best columns, and the same mask as lists."""
    mask = random_mask(rng, scores)
    return [("none", None, None), ("dense", mask, None), ("lists", None, lists_of(mask, rng, lists_with_rows))]


def bulk(rng, rows, cols, hi=0.9):
    return f32(rng.random((rows, cols)) * hi)


def build_boundary(n):
    def build():
        rng = np.random.default_rng(n)
        s = bulk(rng, 2, 4096)
        for r in range(2):
            vals = f32(1.0 + rng.permutation(n) * 2.0 ** -12)           # distinct, all inside [1, 1.25)
            s[r, :min(n, 512)] = vals[:512]
            if n > 512:
                s[r, 1024] = vals[512]                                   # thread 0 again: a 513th candidate
        route = "short" if n <= SHORT_MAX else "regs_radix"
        return Case(s, (1, 20, 256), usual_forms(rng, s), [("none", r, k, route, n) for r in range(2) for k in (1, 20, 256)])
    return build


def cluster_rows(rng, rows, cols, div=1):
    return f32(np.stack([1.0 + (rng.permutation(cols) // div) * 2.0 ** -23 for _ in range(rows)]))


def build_cluster_low_bits():
    rng = np.random.default_rng(21)
    s = cluster_rows(rng, 2, 3000)
    return Case(s, (1, 20, 256), usual_forms(rng, s), [("none", r, k, "regs_radix", 3000) for r in range(2) for k in (1, 20, 256)])


def build_cluster_with_ties():
    rng = np.random.default_rng(22)
    s = cluster_rows(rng, 2, 3000, div=4)
    ks = (1, 22, 255)                                                    # 1, 2 and 3 of a tie of four fit
    return Case(s, ks, usual_forms(rng, s), [("none", r, k, "regs_radix", 3000) for r in range(2) for k in ks],
                {("none", r, k): 1 for r in range(2) for k in ks})


def build_narrow_band(cols, route):
    def build():
        rng = np.random.default_rng(cols)
        s = np.empty((2, cols), dtype=np.float32)
        s[0] = f32(rng.uniform(-1e-3, 1e-3, size=cols))
        s[0, 11::97] = from_bits([0x80000000])[0]                        # -0
        s[0, 12::97] = 0.0
        s[1] = f32(rng.uniform(-1e-3, -1e-6, size=cols))                 # all negative: the zeros lead, -0 and +0 tied
        s[1, 5::37] = from_bits([0x80000000])[0]
        s[1, 23::74] = 0.0
        zeros = int(np.count_nonzero(s[1] == 0))
        claims = [("none", 0, k, route, None) for k in (1, 20, 256)]
        ties = {}
        if zeros > SHORT_MAX:
            claims += [("none", 1, k, "regs_radix", zeros) for k in (1, 20, 256)]
            ties = {("none", 1, 256): 2}
        return Case(s, (1, 20, 256), usual_forms(rng, s), claims, ties)
    return build


def build_ties_carried():
    rng = np.random.default_rng(31)
    s = bulk(rng, 3, 4200)
    s[:, ::16] = 2.0                                                     # 263 ties, 64 per slice: 256 fill four slices
    s[1, 4097:4117:2] = f32(3.0 + rng.permutation(10))                   # row 1: 10 larger values, met after the ties
    s[2, 16] = 0.5                                                       # row 2: one tie fewer, the 256th is in the fifth slice
    return Case(s, (256,), usual_forms(rng, s)[:1] + [("dense", dense_keeping(rng, s, s >= 2.0), None)],
                [("none", r, 256, "regs_radix", None) for r in range(3)],
                {(f, r, 256): n for f in ("none", "dense") for r, n in ((0, 4), (1, 4), (2, 5))})


def dense_keeping(rng, scores, keep, share=0.1):
    """A random 0 / 1 mask that leaves the columns ``keep`` unseen: the case's structure survives the mask."""
    mask = (rng.random(scores.shape) < share).astype(np.float32)
    mask[keep] = 0.0
    return mask


def build_ties_carried_stream():
    rng = np.random.default_rng(32)
    s = bulk(rng, 2, 66000)
    s[:, ::512] = 2.0                                                    # 129 ties, two per slice
    s[1, 65990:66000] = f32(3.0 + rng.permutation(10))
    mask = dense_keeping(rng, s, s >= 2.0)
    forms = [("none", None, None), ("dense", mask, None), ("lists", None, lists_of(mask, rng, True))]
    return Case(s, (64,), forms, [(f, r, 64, "stream", None) for f in ("none", "dense", "lists") for r in range(2)],
                {(f, 0, 64): 32 for f in ("none", "dense", "lists")} | {(f, 1, 64): 27 for f in ("none", "dense", "lists")})


def build_short_ties():
    """The short cut with a tie at the cut: 40 equal candidates spread over all four slices, 20 of them fit."""
    rng = np.random.default_rng(33)
    s = bulk(rng, 2, 4096)
    for r in range(2):
        s[r, rng.permutation(1024)[:40] + 1024 * (np.arange(40) % 4)] = 1.5     # 40 different threads
    s[1, 4000] = 7.0
    return Case(s, (20,), [("none", None, None), ("dense", dense_keeping(rng, s, s >= 1.5), None)],
                [("none", 0, 20, "short", 40), ("none", 1, 20, "short", 41)], {("none", 0, 20): 2, ("none", 1, 20): 2})


def build_one_thread_owns_the_top():
    rng = np.random.default_rng(41)
    s = np.empty((2, 8192), dtype=np.float32)
    s[0] = bulk(rng, 1, 8192)[0]                                         # spread: few candidates
    s[1] = f32(0.5 + rng.random(8192) * 0.12)                            # one bin: every element is a candidate
    s[:, 7::1024] = f32(10.0 + rng.permutation(8))                       # the 8 largest, all of thread 7, not in index order
    claims = [("none", 0, k, "short", None) for k in (5, 8)] + [("none", 1, k, "regs_radix", 8192) for k in (5, 8)]
    return Case(s, (5, 8), usual_forms(rng, s), claims)


def build_k_edges():
    rng = np.random.default_rng(51)
    s = np.concatenate([cluster_rows(rng, 1, 2048), f32(rng.standard_normal((1, 2048)))])
    ks = (1, 2, 3, 127, 128, 129, 255, 256)
    return Case(s, ks, usual_forms(rng, s), [("none", 0, k, "regs_radix", 2048) for k in ks] + [("none", 1, k, "short", None) for k in ks])


def build_width(cols):
    def build():
        rng = np.random.default_rng(cols)
        s = np.concatenate([f32(rng.standard_normal((1, cols))), cluster_rows(rng, 1, cols)])
        ks = sorted({min(cols, 20)} | ({cols} if cols <= K_MAX else set()))
        if cols > REGS_COLS:
            claims = [("none", r, k, "stream", None) for r in range(2) for k in ks]
        else:
            claims = [("none", 1, k, "short" if cols <= SHORT_MAX else "regs_radix", cols) for k in ks]
        return Case(s, ks, usual_forms(rng, s), claims)
    return build


def build_list_mask(cols):
    def build():
        rng = np.random.default_rng(cols)
        s = f32(rng.standard_normal((2, cols)))
        mask = random_mask(rng, s, share=0.01, top=30)                   # the 30 best of each row are seen
        forms = [("none", None, None), ("dense", mask, None),
                 ("lists_rows", None, lists_of(mask, rng, True, junk=True)),
                 ("lists_null", None, lists_of(mask, rng, False, junk=True))]
        return Case(s, (20, 256), forms, [(f, r, k, "stream", None) for f, _, _ in forms for r in range(2) for k in (20, 256)])
    return build


def build_past_list_limit():
    """One column more than the list form takes: the dense mask and no mask still work (the device test adds the refusal)."""
    rng = np.random.default_rng(983041)
    s = f32(rng.standard_normal((2, LIST_COLS_MAX + 1)))
    return Case(s, (20,), [("none", None, None), ("dense", random_mask(rng, s, share=0.01, top=30), None)],
                [("none", 0, 20, "stream", None)])


def build_dense_values_and_strides():
    rng = np.random.default_rng(61)
    cols = 3000
    s = f32(rng.standard_normal((3, cols + 11)))[:, 3:3 + cols]          # rows 3,011 apart
    wide = np.zeros((3, cols + 37), dtype=np.float32)
    mask = wide[:, 5:5 + cols]                                           # rows 3,037 apart
    pick = rng.random((3, cols))
    mask[pick < 0.4] = 1.0
    mask[pick < 0.3] = 0.5
    mask[pick < 0.2] = 2.0                                               # 1 - seen = -1: the sign flips
    mask[pick < 0.1] = -1.0                                              # 1 - seen = 2
    wide[:, :5] = np.nan                                                 # what lies outside the slices must not be read as data
    wide[:, 5 + cols:] = np.nan
    return Case(s, (1, 20, 256), [("none", None, None), ("dense", mask, None)], [("dense", 0, 20, "short", None)])


def build_many_rows():
    rng = np.random.default_rng(71)
    s = f32(rng.integers(-2, 3, size=(70000, 8)))                        # small integers: ties in almost every row
    s[::9, 3] = from_bits([0x80000000])[0]
    mask = (rng.random(s.shape) < 0.3).astype(np.float32)
    return Case(s, (3,), [("none", None, None), ("dense", mask, None), ("lists", None, lists_of(mask, rng, False))],
                [("none", 0, 3, "short", None), ("none", 69999, 3, "short", None)])


NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFE00000, 0x7FA00000]


def plant_specials(rng, row):
    """Eight NaNs of both sign bits and several payloads, two +inf, two -inf, at random columns of ``row``."""
    cols = rng.permutation(row.size)[:12]
    row[cols[:8]] = from_bits(NANS)
    row[cols[8:10]] = np.inf
    row[cols[10:]] = -np.inf
    return cols


def build_nan(kind):
    def build():
        rng = np.random.default_rng({"short": 81, "regs_radix": 82, "stream": 83}[kind])
        if kind == "short":
            s = f32(rng.standard_normal((1, 3000)))
        elif kind == "regs_radix":
            s = cluster_rows(rng, 1, 3000)
        else:
            s = f32(rng.standard_normal((1, 66000)))
        plant_specials(rng, s[0])
        ks = (1, 3, 8, 9, 10, 11, 40)                                    # inside the NaNs, at their end, through +inf, beyond
        if kind == "short":
            claims = [("none", 0, k, "short", None) for k in ks]
        elif kind == "regs_radix":
            claims = ([("none", 0, k, "short", 8) for k in (1, 3, 8)] + [("none", 0, k, "short", 10) for k in (9, 10)]
                      + [("none", 0, k, "regs_radix", 2998) for k in (11, 40)])
        else:
            claims = [("none", 0, k, "stream", None) for k in ks]
        ties = {("none", 0, 3): 2} if kind == "stream" else {}
        return Case(s, ks, usual_forms(rng, s), claims, ties)
    return build


def build_nan_many():
    """600 NaNs, more than the short cut ranks: the radix passes order NaNs of both signs, the cut falls among them."""
    rng = np.random.default_rng(84)
    s = f32(rng.standard_normal((2, 3000)))
    for r in range(2):
        cols = rng.permutation(3000)[:600]
        s[r, cols] = from_bits(np.resize(NANS, 600))
    s[1, np.flatnonzero(~np.isnan(s[1]))[0]] = np.inf
    ks = (20, 256)
    return Case(s, ks, usual_forms(rng, s), [("none", r, k, "regs_radix", 600) for r in range(2) for k in ks],
                {("none", r, 256): 2 for r in range(2)})


def build_nan_from_mask():
    """A seen column holding +inf and one holding -inf: inf * 0 is a NaN whose sign the hardware chooses."""
    rng = np.random.default_rng(85)
    s = f32(rng.standard_normal((2, 3000)))
    s[0, 100], s[0, 2000], s[0, 50], s[0, 60] = np.inf, -np.inf, np.inf, -np.inf
    s[1, 2999], s[1, 0] = -np.inf, np.inf
    mask = (rng.random(s.shape) < 0.1).astype(np.float32)
    mask[0, [100, 2000]] = 1.0
    mask[0, [50, 60]] = 0.0
    mask[1, [0, 2999]] = 1.0
    forms = [("dense", mask, None), ("lists", None, lists_of(mask, rng, True))]
    return Case(s, (1, 2, 3, 20), forms, [("dense", 0, 3, "short", None)])


CASES = (
    [(f"boundary_{n}", build_boundary(n)) for n in (511, 512, 513)]
    + [("cluster_low_bits", build_cluster_low_bits), ("cluster_with_ties", build_cluster_with_ties),
       ("narrow_band_2500", build_narrow_band(2500, "short")), ("narrow_band_60000", build_narrow_band(60000, "regs_radix")),
       ("ties_carried", build_ties_carried), ("ties_carried_stream", build_ties_carried_stream), ("short_ties", build_short_ties),
       ("one_thread_owns_the_top", build_one_thread_owns_the_top), ("k_edges_2048", build_k_edges)]
    + [(f"width_{c}", build_width(c)) for c in (1, 2, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537)]
    + [(f"list_mask_{c}", build_list_mask(c)) for c in (131072, 131073, LIST_COLS_MAX)]
    + [("past_list_limit", build_past_list_limit), ("dense_values_and_strides", build_dense_values_and_strides),
       ("many_rows", build_many_rows)]
    + [(f"nan_{kind}", build_nan(kind)) for kind in ("short", "regs_radix", "stream")]
    + [("nan_many", build_nan_many), ("nan_from_mask", build_nan_from_mask)]
)
CASE_NAMES = [name for name, _ in CASES]
_built = {}


def case(name):
    """The case, built once and shared by every test that asks for it; nobody writes to it."""
    if name not in _built:
        _built[name] = dict(CASES)[name]()
    return _built[name]
