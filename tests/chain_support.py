"""The exact host reference of lgc_score_rows' chain, its mutants and the data that tells them apart
(tests/test_chain_host.py, tests/test_chain_gpu.py).  numpy only; no project code is imported.

``fma32`` is fp32 round(a * b + c), exact: the product of two fp32 values has at most 48 significant bits and is formed in
float64 without error; the float64 sum is taken with TwoSum, and where it is inexact the sum is moved to the neighbour whose
last mantissa bit is odd (round to odd).  A value rounded to odd at p + 2 or more bits rounds to p bits as the exact value
does, and 53 >= 24 + 2, so the cast to fp32 -- to a subnormal too, which keeps fewer bits still -- is the correctly rounded
fused multiply-add.  ``chain32`` runs it over d ascending from +0, ``rnorm32`` restates lgc_row_rnorm's rule with it.

The mutants are ``chain32`` with one plausible mistake each.  ``COINCIDES`` lists, per mutant, the widths up to which it is
the same computation as the chain; at every other width the data builders below must tell it apart, which
tests/test_chain_host.py proves on the very tables the device tests upload."""
import numpy as np

import fullrank_support as fs
from hardneg_support import poisoned
import similar_support as ss
import topk_support as ts

N_ROWS, N_ITEMS = 64, 160            # one full row tile; two item tiles, the second ragged
WIDTHS = list(range(1, 98)) + [112, 113, 127, 128, 129, 240, 241, 255, 256]
CLASS_WIDTHS = (5, 16, 17, 33, 48, 49, 64, 90, 256)      # one width of each class, for the other holders of the chain
KINDS = ("permuted", "random", "wide", "specials")
LAYOUTS = ("dense", "poisoned")
GROUP, CHUNK = 16, 32                # columns of an MFMA group (four instructions) and of a staged chunk (Tile::product)

F32 = np.float32


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ----------------------------------------------------------------------------------------
# the fused multiply-add and the chain
# ----------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 round(a * b + c), element-wise over broadcast fp32 arrays; NaN and the infinities as IEEE 754 has them."""
    with np.errstate(all="ignore"):                          # a signalling NaN may be cast, an infinity may be met
        a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
        p = a * b                                           # exact: 24 + 24 bits, exponents far inside float64's
        s = p + c
        t = s - p                                            # TwoSum: s + e == p + c exactly
        e = (p - (s - t)) + (c - t)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(np.float32)


def _steps(u, items, order, fused=True, acc=None):
    """The accumulator [n_u, n_items] after the steps d of ``order``, from ``acc`` (+0 by default)."""
    u, items = f32(u), f32(items)
    if acc is None:
        acc = np.zeros((u.shape[0], items.shape[0]), dtype=np.float32)
    for d in order:
        if fused:
            acc = fma32(u[:, d, None], items[None, :, d], acc)
        else:
            with np.errstate(all="ignore"):
                acc = (u[:, d, None] * items[None, :, d]).astype(np.float32) + acc
    return acc


def chain32(u, items):
    """fp32 [n_u, n_items]: acc = fma32(u[:, d], items[:, d], acc) over d ascending from +0, with zeros past dim up to the
    next multiple of 4 -- the extent include/lgconv_hip.h gives the chain (lgc_sample_hard_triples: "d = 0 .. round_up(dim, 4)
    - 1 ... with zeros past dim").  fma(0, 0, acc) changes nothing but a -0, which it makes +0: where dim % 4 != 0 a sum of
    -0 comes out as +0."""
    dim = np.shape(u)[1]
    acc = _steps(u, items, range(dim))
    if dim % 4:
        acc = fma32(F32(0), F32(0), acc)
    return acc


def rnorm32(table):
    """fp32 [n_rows]: lgc_row_rnorm's rule -- ss = fma32(x_d, x_d, ss) over d ascending from +0, the fp32 square root, the
    fp32 reciprocal (numpy rounds both correctly); an infinite result gives 0, NaN stays."""
    x = f32(table)
    ss_ = np.zeros(x.shape[0], dtype=np.float32)
    for d in range(x.shape[1]):
        ss_ = fma32(x[:, d], x[:, d], ss_)
    with np.errstate(all="ignore"):
        out = F32(1.0) / np.sqrt(ss_)
    return np.where(np.isinf(out), F32(0.0), out).astype(np.float32)


# ----------------------------------------------------------------------------------------
# mutants: chain32 with one mistake each
# ----------------------------------------------------------------------------------------
def _grouped(size):
    def run(u, items):
        dim = np.shape(u)[1]
        total = np.zeros((np.shape(u)[0], np.shape(items)[0]), dtype=np.float32)
        for lo in range(0, dim, size):
            with np.errstate(all="ignore"):
                total = total + _steps(u, items, range(lo, min(lo + size, dim)))
        return total
    return run


def _midswap_order(dim):
    order = list(range(dim))
    for g in range(0, dim, 4):
        if g + 2 < dim:                                      # a swap with a padded zero step is no change
            order[g + 1], order[g + 2] = order[g + 2], order[g + 1]
    return order


MUTANTS = {
    "descending": lambda u, items: _steps(u, items, range(np.shape(u)[1] - 1, -1, -1)),
    "unfused": lambda u, items: _steps(u, items, range(np.shape(u)[1]), fused=False),
    "midswap": lambda u, items: _steps(u, items, _midswap_order(np.shape(u)[1])),
    "groups4": _grouped(4),
    "groups16": _grouped(GROUP),
    "chunks32": _grouped(CHUNK),
}
# the widest dim at which the mutant is the chain itself: one step has no order and fma(a, b, +0) is the rounded product;
# columns 1 and 2 must both exist to be swapped; one group (or chunk) summed from +0 and added to +0 is the chain
COINCIDES = {"descending": 1, "unfused": 1, "midswap": 2, "groups4": 4, "groups16": GROUP, "chunks32": CHUNK}


def applicable(dim):
    """The mutants that are another computation than the chain at this width."""
    return [name for name in MUTANTS if dim > COINCIDES[name]]


# ----------------------------------------------------------------------------------------
# data, all seeded by (kind, dim) alone
# ----------------------------------------------------------------------------------------
def _rng(kind, dim):
    return np.random.default_rng([KINDS.index(kind) + 1, dim])


def permuted(dim, n=N_ITEMS):
    """(users [N_ROWS, dim], items [n, dim]).  Item rows are column permutations of one base vector of normal deviates times
    2^(-6 .. 6); every user row is the constant 1.1f, which is inexact, so fused and unfused differ.  The products of every
    (user, item) pair are the same multiset: scores differ only in their last bits, by the order of the steps, and tie in
    long runs.

    Not every base vector will do: four columns of very different size can sum to the same value in every order.  The
    builder therefore takes the first of its seeded draws whose REFERENCE ranking has the two properties the tests rest on
    (``tells_apart``); the code under test has no part in the choice, and tests/test_chain_host.py asserts both again."""
    users = np.full((N_ROWS, dim), 1.1, dtype=np.float32)
    for attempt in range(200):
        rng = np.random.default_rng([KINDS.index("permuted") + 1, dim, attempt])
        base = (rng.standard_normal(dim) * 2.0 ** rng.integers(-6, 7, size=dim)).astype(np.float32)
        items = f32(np.stack([base[rng.permutation(dim)] for _ in range(n)]))
        if dim < 3 or tells_apart(users, items):
            return users, items
    raise AssertionError(f"no base vector of width {dim} among 200 draws tells the mutants apart")


def tells_apart(users, items, places=20, long_tie=10):
    """Do the reference's scores of user row 0 tie in long runs -- a quarter of the items in runs of more than ``long_tie``
    -- and does every applicable mutant move one of the first ``places`` places AND one (rank, n_equal) pair?"""
    want = chain32(users[:1], items)[0]
    first, pairs = ranking(want, places), rank_pairs(want)
    if (pairs[1] > long_tie).sum() * 4 < want.size:
        return False
    for name in applicable(users.shape[1]):
        got = MUTANTS[name](users[:1], items)[0]
        other = rank_pairs(got)
        if (ranking(got, places) == first).all() or ((other[0] == pairs[0]) & (other[1] == pairs[1])).all():
            return False
    return True


def random(dim, n=N_ITEMS):
    rng = _rng("random", dim)
    return ss.random_table(rng, N_ROWS, dim), ss.random_table(rng, n, dim)


def wide(dim, n=N_ITEMS):
    """Rows scaled by 10^(0, 0, -20, -25) and one row of the smallest subnormal in either table: subnormal sums, products
    that underflow, sums of -0."""
    rng = _rng("wide", dim)
    return ss.subnormal_table(rng, N_ROWS, dim), ss.subnormal_table(rng, n, dim)


def specials(dim, n=N_ITEMS):
    """``similar_support.special_table`` for the items; user rows of zeros, of -0, with an infinity and with a NaN."""
    rng = _rng("specials", dim)
    users = ss.random_table(rng, N_ROWS, dim)
    users[0], users[1], users[2, 0], users[3, dim - 1] = 0.0, -0.0, np.inf, np.nan
    users[4, 0] = -np.inf
    return users, ss.special_table(rng, n, dim)[0]


BUILDERS = {"permuted": permuted, "random": random, "wide": wide, "specials": specials}
_tables, _panels = {}, {}


def tables(kind, dim):
    """(users, items) of a kind and width: built once, shared, never written to."""
    if (kind, dim) not in _tables:
        _tables[kind, dim] = BUILDERS[kind](dim)
    return _tables[kind, dim]


def panel(kind, dim, rows="users"):
    """``chain32`` of the user rows (``rows`` "users") or of all item rows ("items") against the items, cached."""
    if (kind, dim, rows) not in _panels:
        users, items = tables(kind, dim)
        if rows == "users" and kind == "permuted":           # one user row, N_ROWS times
            assert (users == users[0]).all()
            _panels[kind, dim, rows] = np.repeat(chain32(users[:1], items), users.shape[0], axis=0)
        else:
            _panels[kind, dim, rows] = chain32(users if rows == "users" else items, items)
    return _panels[kind, dim, rows]


def rank_case(dim):
    """(pair_users, pair_items, ptr, entries) of lgc_rank_positions' test at this width: N_ROWS pairs over N_ROWS users and
    N_ITEMS items, pairs and lists by ``fullrank_support.Case``'s rule (user u's list has LIST_LENGTHS[u % 5] entries,
    ascending, with repeats and entries on either side of the catalogue; every third pair's item is a seen one)."""
    case = fs.Case(f"chain_d{dim}", dim, "strided", N_ITEMS, N_ROWS, (0, 1, 3), n_users=N_ROWS, seed=dim)
    return case.build()[2:]


def query_ids(dim):
    """The N_ROWS query items of lgc_item_neighbors' test at this width: a permutation's prefix."""
    return np.random.default_rng([9, dim]).permutation(N_ITEMS)[:N_ROWS].astype(np.int64)


# ----------------------------------------------------------------------------------------
# layouts and comparisons
# ----------------------------------------------------------------------------------------
def laid_out(table, layout):
    """(flat fp32 buffer, first float of row 0, row stride).  "dense": the rows back to back; "poisoned": rows dim + 3
    floats apart from one float past the (16-byte aligned) buffer's start, NaN in every float that must not be read
    (``hardneg_support.poisoned``)."""
    dim = table.shape[1]
    if layout == "dense":
        return f32(table).reshape(-1).copy(), 0, dim
    return poisoned(table, dim + 3, 1), 1, dim + 3


def same_bits(got, want):
    """Raw bit equality (-0 is not +0), any NaN matching any NaN."""
    return ts.values_match(got, want)


def same_folded(got, want):
    """The same after x + 0: for the MFMA kernels, whose width is padded with zeros to 16 columns, so that a sum of -0 may
    come out as +0 (include/lgconv_hip.h says so for each of them)."""
    return ss.same_values(got, want)


def ranking(scores, places=20):
    """The first ``places`` columns of a row of scores in lgc_mask_topk's order."""
    return ts.topk_ref(scores, min(places, len(scores)))[0]


def rank_pairs(scores):
    """(rank, n_equal) of every column of a row of scores: how many columns precede it, how many others share its key."""
    keys = ts.order_keys(scores).astype(np.int64)
    idx = np.arange(keys.size)
    before = (keys[None, :] > keys[:, None]) | ((keys[None, :] == keys[:, None]) & (idx[None, :] < idx[:, None]))
    return before.sum(axis=1), (keys[None, :] == keys[:, None]).sum(axis=1) - 1


def width_class(dim):
    """(chunks: 1, 2 or 3 = three and more; groups in the last chunk; dim % 4; dim % 16 == 0) -- what Tile::product and the
    row loads branch on.  A chunk past the third is another middle one: staged, multiplied whole and replaced like the
    second."""
    dp = (dim + GROUP - 1) // GROUP * GROUP
    chunks = -(-dp // CHUNK)
    return min(chunks, 3), dp // GROUP - 2 * (chunks - 1), dim % 4, dim % GROUP == 0
