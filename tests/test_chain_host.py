"""CPU-only checks of tests/chain_support.py, the exact host reference the device tests of tests/test_chain_gpu.py hang on:
``fma32`` against rational arithmetic, ``chain32`` and ``rnorm32`` against what is already exact, and -- the condition that
keeps the device tests from passing a wrong kernel -- that the uploaded tables tell every mutant of the chain apart at every
width at which the mutant is another computation."""
import math
from fractions import Fraction

import numpy as np
import pytest

import chain_support as cs
import fullrank_support as fs
import similar_support as ss
import softmax_support as sm
import topk_support as ts

F32_MAX = Fraction(2) ** 128 - Fraction(2) ** 104            # the largest finite fp32


def round_f32(x):
    """A non-zero Fraction rounded to the nearest fp32, ties to even, subnormals kept, as a Python float."""
    sign, m = (-1.0 if x < 0 else 1.0), abs(x)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1                                               # 2^e <= m < 2^(e + 1)
    q = max(e, -126) - 23                                    # the exponent of one ulp
    n = m / Fraction(2) ** q
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r & 1):
        r += 1
    if Fraction(r) * Fraction(2) ** q >= Fraction(2) ** 128:
        return sign * math.inf
    return sign * math.ldexp(r, q)


def fma_exact(a, b, c):
    """fp32 fma of three finite fp32 values (Python floats) in rational arithmetic, the sign of a zero by IEEE 754's rules."""
    p = Fraction(a) * Fraction(b)
    x = p + Fraction(c)
    if x == 0:
        both_zero = p == 0 and c == 0
        negative = both_zero and math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0
        return -0.0 if negative else 0.0
    return round_f32(x)


def triples(kind, n, rng):
    if kind == "normal":
        return (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    if kind == "wide":                                       # exponents over the whole range, subnormal operands among them
        return ((rng.standard_normal(n) * 2.0 ** rng.integers(-149, 100, size=n)).astype(np.float32) for _ in range(3))
    if kind == "bits":
        w = rng.integers(0, 2 ** 32, size=(3, 2 * n), dtype=np.uint64).astype(np.uint32).view(np.float32)
        w = w[:, np.isfinite(w).all(axis=0)][:, :n]
        return w[0], w[1], w[2]
    a, b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, size=n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = -(a * b)                                             # "cancel": c within a few ulps of -a * b
    for _ in range(3):
        step = rng.integers(-1, 2, size=n)
        c = np.where(step == 0, c, np.nextafter(c, np.where(step > 0, np.inf, -np.inf).astype(np.float32)))
    return a, b, c.astype(np.float32)


@pytest.mark.parametrize("kind", ["normal", "wide", "bits", "cancel"])
def test_fma32_equals_rational_arithmetic(kind):
    rng = np.random.default_rng(["normal", "wide", "bits", "cancel"].index(kind))
    a, b, c = triples(kind, 3000, rng)
    assert a.size >= 2500
    got = cs.fma32(a, b, c)
    want = np.array([fma_exact(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float64).astype(np.float32)
    bad = np.flatnonzero(ts.bits_of(got) != ts.bits_of(want))
    assert bad.size == 0, (kind, bad.size, [(a[i], b[i], c[i], got[i], want[i]) for i in bad[:3]])
    if kind == "cancel":                                     # the premise: the sum cancels to a few ulps of the product
        with np.errstate(all="ignore"):
            assert np.median(np.abs(got) / np.abs(a * b)) < 2.0 ** -20
    if kind == "wide":
        tiny = np.abs(got) < 2.0 ** -126
        assert (tiny & (got != 0)).sum() > 20 and np.isinf(got).sum() > 20      # subnormal results and overflows


def test_fma32_gives_the_documented_corners():
    f = lambda a, b, c: cs.fma32(np.float32(a), np.float32(b), np.float32(c))
    bits = lambda x: int(ts.bits_of(x).reshape(-1)[0])
    tiny = 2.0 ** -149
    assert bits(f(0.0, 0.0, -0.0)) == 0x00000000             # +0 + -0
    assert bits(f(-0.0, 0.0, -0.0)) == 0x80000000
    assert bits(f(-tiny, tiny, 0.0)) == 0x80000000           # a product that underflows keeps its sign
    assert bits(f(1.0, -0.0, 0.0)) == 0x00000000
    assert bits(f(3e38, 2.0, 0.0)) == 0x7F800000 and bits(f(-3e38, 2.0, 0.0)) == 0xFF800000
    assert bits(f(3e38, 2.0, -3e38)) == bits(np.float32(3e38))                    # no overflow of the product alone
    assert np.isnan(f(np.inf, 0.0, 1.0)) and np.isnan(f(np.inf, 1.0, -np.inf)) and np.isnan(f(np.nan, 1.0, 1.0))
    assert bits(f(np.inf, -1.0, 5.0)) == 0xFF800000
    assert bits(f(2.0 ** -100, 2.0 ** -40, 0.0)) == 1 << 9                        # 2^-140, an exact subnormal
    assert bits(f(3.0 * 2.0 ** -75, 2.0 ** -75, 0.0)) == 2                        # 1.5 ulp: the tie goes to even
    assert bits(f(1.5 * 2.0 ** -75, 2.0 ** -75, 0.0)) == 1                        # 0.75 ulp
    assert bits(f(1.25 * 2.0 ** -75, 2.0 ** -75, tiny)) == 2                      # 0.625 + 1 ulp, seen whole
    # fused: the product's last bit survives the cancellation (the rounded product would leave 2^-11)
    x = np.float32(1.0 + 2.0 ** -12)
    assert bits(f(x, x, -1.0)) == bits(np.float32(2.0 ** -11 + 2.0 ** -24))
    # one rounding, not two: c + 2^36 - 2^-10 lies just below the fp32 tie c + 2^36; float64 alone would round it ONTO the
    # tie, which then goes to even -- upwards, since c's last bit is odd.  Round to odd keeps it below
    c = 2.0 ** 60 * (1.0 + 2.0 ** -23)
    assert bits(f(2.0 ** 36 * (1.0 + 2.0 ** -23), 1.0 - 2.0 ** -23, c)) == bits(np.float32(c))
    assert bits(f(2.0 ** 36 * (1.0 + 2.0 ** -23), 1.0, c)) == bits(np.float32(c)) + 1               # above the tie
    assert bits(f(2.0 ** -12, 2.0 ** -12, 1.0)) == bits(np.float32(1.0))          # a tie: to even
    assert bits(f(2.0 ** -12 + 2.0 ** -30, 2.0 ** -12, 1.0)) == bits(np.float32(1.0 + 2.0 ** -23))   # just above the tie


@pytest.mark.parametrize("dim", [1, 3, 4, 17, 90, 256])
def test_chain32_is_exact_on_integers_and_is_what_rnorm32_squares(dim):
    rng = np.random.default_rng(dim)
    a, b = ss.integer_table(rng, 9, dim, hi=3), ss.integer_table(rng, 21, dim, hi=3)
    assert np.array_equal(ts.bits_of(cs.chain32(a, b)), ts.bits_of(ss.dot_chain32(a, b)))
    for name, mutant in cs.MUTANTS.items():                  # on integers every order agrees: the gap the floats close
        assert np.array_equal(mutant(a, b), ss.dot_chain32(a, b)), name
    users, items = cs.tables("wide", dim)
    t = np.concatenate([cs.tables("random", dim)[1][:20], items[:40], np.zeros((1, dim), dtype=np.float32)])
    t[5, dim - 1] = np.nan
    ssq = np.diagonal(cs.chain32(t, t))
    with np.errstate(all="ignore"):
        want = np.float32(1.0) / np.sqrt(ssq)
    want = np.where(np.isinf(want), np.float32(0.0), want)
    got = cs.rnorm32(t)
    assert cs.same_bits(got, want) and got[-1] == 0.0 and np.isnan(got[5]) and (got == 0).sum() >= 2
    ref = ss.rnorm_ref(t)                                    # and inside the bound that held it until now
    ok = np.isfinite(ref) & (ref > 0) & (ssq >= 2.0 ** -100)
    assert ok.sum() >= 20 and (np.abs(got[ok] - ref[ok]) <= ss.rnorm_bound(dim) * ref[ok]).all()


def test_chain32_pads_with_zeros_to_four_columns_and_no_further():
    neg = np.float32(-2.0 ** -100)
    for dim in range(1, 9):
        u, i = np.full((1, dim), neg), np.full((1, dim), -neg)                    # every product underflows to -0
        want = 0x80000000 if dim % 4 == 0 else 0x00000000                         # fma(0, 0, -0) = +0 in the padded steps
        assert int(ts.bits_of(cs.chain32(u, i))[0, 0]) == want, dim


# ---------------------------------------------------------------------------------------------------------------
# the data tells the mutants apart
# ---------------------------------------------------------------------------------------------------------------
def test_exemption_table_is_what_the_arithmetic_says():
    assert cs.COINCIDES == {"descending": 1, "unfused": 1, "midswap": 2, "groups4": 4, "groups16": 16, "chunks32": 32}
    assert set(cs.COINCIDES) == set(cs.MUTANTS)
    assert cs.applicable(1) == [] and cs.applicable(2) == ["descending", "unfused"]
    assert cs.applicable(3) == ["descending", "unfused", "midswap"] and cs.applicable(16) == cs.applicable(5)
    assert cs.applicable(17)[-1] == "groups16" and cs.applicable(33) == list(cs.MUTANTS) and cs.applicable(32) == cs.applicable(17)


@pytest.mark.parametrize("dim", cs.WIDTHS)
def test_a_mutant_coincides_with_the_chain_exactly_at_its_exempt_widths(dim):
    """Asserted, not skipped: up to COINCIDES[name] columns the mutant IS the chain, bit for bit, on both kinds of data."""
    exempt = [name for name in cs.MUTANTS if name not in cs.applicable(dim)]
    for kind in ("permuted", "random"):
        users, items = cs.tables(kind, dim)
        want = cs.panel(kind, dim)[:8]
        for name in exempt:
            assert cs.same_bits(cs.MUTANTS[name](users[:8], items), want), (kind, name)
    assert len(exempt) == sum(dim <= w for w in cs.COINCIDES.values())


@pytest.mark.parametrize("dim", [d for d in cs.WIDTHS if d >= 3])
def test_permuted_rows_rank_differently_under_every_applicable_mutant(dim):
    users, items = cs.tables("permuted", dim)
    assert (users == users[0]).all()                         # one query row: one ranking
    want = cs.panel("permuted", dim)[0]
    places, pairs = cs.ranking(want), cs.rank_pairs(want)
    assert (pairs[1] > 10).sum() * 4 >= want.size            # the ties are long: a quarter of the items in runs above 10
    for name in cs.applicable(dim):
        got = cs.MUTANTS[name](users[:1], items)[0]
        moved = int((cs.ranking(got) != places).sum())
        other = cs.rank_pairs(got)
        changed = int(((other[0] != pairs[0]) | (other[1] != pairs[1])).sum())
        print(f"dim {dim} {name}: {moved} of the first 20 places moved, {changed} of {want.size} (rank, n_equal) pairs changed")
        assert moved >= 1 and changed >= 1, (dim, name)


@pytest.mark.parametrize("dim", [d for d in cs.WIDTHS if d >= 2])
def test_random_rows_change_bits_under_every_applicable_mutant(dim):
    users, items = cs.tables("random", dim)
    want = cs.panel("random", dim)[:8]
    for name in cs.applicable(dim):
        changed = int((ts.bits_of(cs.MUTANTS[name](users[:8], items)) != ts.bits_of(want)).sum())
        print(f"dim {dim} {name}: {changed} of {want.size} scores changed")
        assert changed >= 1, (dim, name)


def test_widths_reach_every_class_of_the_tile_and_of_the_row_loads():
    have = {cs.width_class(d) for d in cs.WIDTHS}
    exist = {cs.width_class(d) for d in range(1, 257)}
    # per (chunks, groups in the last one): dim % 4 = 1, 2, 3, a multiple of 4 that is none of 16, and the full width
    assert have == exist and len(exist) == 3 * 2 * 5
    assert set(cs.CLASS_WIDTHS) <= set(cs.WIDTHS) and {d % 4 for d in cs.CLASS_WIDTHS} == {0, 1, 2}
    # a lone last group -- the stale second half of Bs -- behind one, two and more full chunks; the widest width; D = 90
    lone = sorted(d for d in cs.WIDTHS if cs.width_class(d)[1] == 1 and d > 16)
    assert {-(-d // 32) for d in lone} >= {2, 3, 4, 5, 8} and 256 in cs.WIDTHS and 90 in cs.WIDTHS
    for m in (4, 16, 32):
        for chunks in (1, 2, 3):
            assert {d % m for d in cs.WIDTHS if cs.width_class(d)[0] == chunks} == set(range(m))


def test_pairs_of_the_rank_test_meet_the_long_ties():
    """lgc_rank_positions' device test counts over these pairs: on permuted rows some pair must sit in a run above 10."""
    for dim in cs.WIDTHS:
        pu, pi, ptr, entries = cs.rank_case(dim)
        assert pu.shape == pi.shape == (cs.N_ROWS,) and pu.max() < cs.N_ROWS and pi.max() < cs.N_ITEMS
        assert any(p in entries[ptr[u]:ptr[u + 1]] for u, p in zip(pu, pi))          # a seen p: -1 under "remove"
        if dim >= 3:
            _, n_equal, _, _ = fs.ranks_ref(cs.panel("permuted", dim)[pu], pi, None, "zero")
            assert n_equal.max() > 10, dim


def test_softmax_case_table_holds_the_narrow_widths():
    """lgc_softmax_batch's logits are no output; its widths of one, two and three 16-column groups are cases of the softmax
    suite, at r65 x c129: one chunk (d16), a misaligned second group (d17), and a lone group behind a full chunk (d33 .. d48)."""
    have = {(c.dim, c.layout) for c in sm.CASES if (c.n_rows, c.n_cand) == (65, 129)}
    assert have >= {(16, "dense"), (17, "misaligned"), (33, "padded"), (48, "dense"), (49, "padded")}
    assert len(set(sm.CASE_NAMES)) == len(sm.CASE_NAMES)


def test_layouts_keep_the_rows_and_poison_the_rest():
    t = cs.tables("random", 5)[1]
    flat, off, stride = cs.laid_out(t, "dense")
    assert (off, stride) == (0, 5) and np.array_equal(flat.reshape(-1, 5), t)
    flat, off, stride = cs.laid_out(t, "poisoned")
    assert (off, stride) == (1, 8) and np.isnan(flat[0]) and np.isnan(flat[off + stride * len(t):]).all()
    rows = flat[off:off + stride * len(t)].reshape(-1, stride)
    assert np.array_equal(rows[:, :5], t) and np.isnan(rows[:, 5:]).all()
    assert cs.same_bits(np.float32([np.nan, -0.0]), ts.from_bits([0xFFC00001, 0x80000000]))
    assert not cs.same_bits(np.float32([-0.0]), np.float32([0.0])) and cs.same_folded(np.float32([-0.0]), np.float32([0.0]))
    assert not cs.same_folded(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2.0)))
