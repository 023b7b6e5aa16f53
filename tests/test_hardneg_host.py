"""CPU-only checks of the hard-negative sampler: the entry point in the header (an addition to ABI 14), the ctypes table and
the library; its argument validation, which happens before any launch; the reference of tests/hardneg_support.py on lists
worked by hand with integer-valued scores (exact in any order); the device tests' case table against what its names
promise, from the reference alone; and the Python layer's own checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gnn_ecommerce_amd import _native
from gnn_ecommerce_amd.sampler import TripleSampler
import hardneg_support as hs
import sampler_support as ss

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_DIM, E_RANGE = -1, -2, -4
NAME = "lgc_sample_hard_triples"


def test_entry_point_is_declared_bound_and_exported_as_an_addition_to_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    assert "Hard negatives (an addition to ABI 14: exports only)" in header
    assert int(re.search(r"#define LGC_HARDNEG_MAX_CAND (\d+)", header).group(1)) == _native.HARDNEG_MAX_CAND == hs.MAX_CAND \
        == ss.MAX_ATTEMPTS
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"ptr": (ctypes.c_void_p,), "int64_t": (ctypes.c_int64,), "int32_t": (ctypes.c_int32,), "uint64_t": (ctypes.c_uint64,)}
    decl = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert decl and hasattr(lib, NAME)
    restype, argtypes = _native.SIGNATURES[NAME]
    assert restype is ctypes.c_int
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(argtypes) == 23
    for arg, have in zip(args, argtypes):
        kind = "ptr" if "*" in arg else re.match(r"(?:const\s+)?(\w+)", arg).group(1)
        assert have in kinds[kind], arg
    assert argtypes[:10] == _native.SIGNATURES["lgc_sample_triples"][1][:10]          # the stream's arguments, unchanged
    assert hasattr(TripleSampler, "sample_hard")
    makefile = open(os.path.join(ROOT, "gnn-ecommerce_amd", "csrc", "Makefile")).read()
    assert "lgconv_hardneg" in re.search(r"^UNITS\s*:=((?:.*\\\n)*.*)$", makefile, flags=re.M).group(1).split()


# addresses of host words: valid, 16-byte aligned, never read or written by a call that returns before its launch
_words = (ctypes.c_int64 * 8)()
ONE = ctypes.addressof(_words) + (-ctypes.addressof(_words)) % 16


def hard(**kw):
    a = dict(users=ONE, n=4, pos_ptr=ONE, pos_items=ONE, ign_ptr=ONE, ign_items=ONE, n_users=100, n_items=300, seed=1, step=2,
             n_cand=8, user_table=ONE, user_stride=64, item_table=ONE, item_stride=64, dim=64, pos_out=ONE, neg_out=ONE,
             neg_score=ONE, neg_attempt=ONE, n_admissible=ONE, status=ONE)
    assert set(kw) <= set(a)
    a.update(kw)
    return _native.load().lgc_sample_hard_triples(*a.values(), None)


def test_argument_errors_come_before_any_launch():
    for bad in (dict(users=None), dict(pos_ptr=None), dict(pos_items=None), dict(ign_ptr=None), dict(user_table=None),
                dict(item_table=None), dict(pos_out=None), dict(neg_out=None), dict(status=None), dict(n=-1), dict(n_users=-1),
                dict(n_items=0), dict(n_items=-5), dict(user_stride=63), dict(item_stride=63), dict(user_stride=0)):
        assert hard(**bad) == E_INVAL, bad
    for dim in (0, -1, 257):
        assert hard(dim=dim, user_stride=300, item_stride=300) == E_DIM
    assert hard(dim=0, users=None, n_cand=0) == E_DIM                                  # the width is judged first
    for bad in (dict(n_cand=0), dict(n_cand=-1), dict(n_cand=257), dict(n=2 ** 31), dict(n_users=2 ** 31), dict(n_items=2 ** 31),
                dict(n_users=2 ** 30, n_items=2 ** 30), dict(n_users=0, n_items=2 ** 31)):
        assert hard(**bad) == E_RANGE, bad
    # n == 0: validated, nothing launched; the optional pointers may be NULL
    assert hard(n=0) == 0 and hard(n=0, neg_score=None, neg_attempt=None, n_admissible=None, ign_items=None) == 0
    for ok in (dict(n_cand=1), dict(n_cand=256), dict(dim=1, user_stride=1, item_stride=1), dict(dim=256, user_stride=259,
               item_stride=256), dict(n_users=0), dict(n_items=1), dict(n_users=2 ** 30, n_items=2 ** 30 - 2),
               dict(seed=2 ** 64 - 1, step=2 ** 64 - 1), dict(user_stride=64, item_stride=67)):
        assert hard(n=0, **ok) == 0, ok
    assert hard(n=0, item_stride=63) == E_INVAL and hard(n=0, n_cand=257) == E_RANGE and hard(n=0, status=None) == E_INVAL


# ---------------------------------------------------------------------------------------------------------------
# the reference, on lists worked by hand: integer-valued scores
# ---------------------------------------------------------------------------------------------------------------
NU, NI = 3, 40
ALL = [NU + i for i in range(NI)]
POS = {0: [NU + 3, NU + 9], 1: [NU + 1], 2: [NU + 7]}
CSRS_OPEN = (ss.csr(NU, POS), ss.csr(NU, {}))


def key_with_distinct_draws(count, step=4):
    """(seed, draws): the smallest seed at which sample 0's first ``count`` draws are ``count`` different nodes."""
    for seed in range(1000):
        draws = ss.candidates(ss.sample_key(seed, step, 0), NU, NI, count)
        if len(set(draws)) == count:
            return seed, draws
    raise AssertionError("no such seed below 1000")


def by_node(values, default):
    """score(u, item) from {node: value}."""
    return lambda u, item: np.float32(values.get(NU + item, default))


def test_one_candidate_is_the_uniform_sampler_and_so_is_a_table_of_equal_scores():
    users = [0, 1, 2, 1, 0, 5, -1, 2]
    ign = ss.csr(NU, {0: ALL[::2], 1: [x for x in ALL if x != NU + 13], 2: ALL})
    csrs = (ss.csr(NU, POS), ign)
    integer_table = lambda u, item: np.float32((7 * u + 3 * item) % 11 - 5)
    for seed, step in ((0, 0), (5, 2 ** 32), (2 ** 64 - 1, 2 ** 64 - 1)):
        want = ss.sample_ref(users, *csrs[0], *csrs[1], NU, NI, seed, step)
        pos, neg, attempt, admissible, status = hs.hard_ref(users, csrs, NU, NI, seed, step, 1, integer_table)
        assert (pos, neg, status) == want
        for i, u in enumerate(users):
            if hs.bad_user(u, NU, csrs[0][0]):
                assert (pos[i], neg[i], attempt[i], admissible[i]) == (NU, NU, 0, 0)
            else:
                need = ss.attempts_needed(ss.sample_key(seed, step, i), NU, NI, set(ign[1][ign[0][u]:ign[0][u + 1]]))
                assert (attempt[i], admissible[i]) == ((need, 1) if need else (256, 0))
        assert status == ss.ST_INDEX_OOB | ss.ST_SAMPLER_EXHAUSTED
        for equal in (0.0, 3.0, -2.0):
            got = hs.hard_ref(users, csrs, NU, NI, seed, step, 8, lambda u, item: np.float32(equal))
            assert (got[0], got[1], got[4]) == want and got[2] == attempt


def test_a_tie_goes_to_the_earlier_attempt():
    seed, draws = key_with_distinct_draws(6)
    score = by_node({draws[1]: 5, draws[4]: 5}, 1)
    pos, neg, attempt, admissible, status = hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 6, score)
    assert (neg, attempt, admissible, status) == ([draws[1]], [2], [6], 0)
    # with four candidates only attempt 2 holds the 5; with one, attempt 1 is all there is
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 4, score)[1:3] == ([draws[1]], [2])
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 1, score)[1:3] == ([draws[0]], [1])
    # a higher score later beats both
    score = by_node({draws[1]: 5, draws[4]: 5, draws[5]: 6}, 1)
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 6, score)[1:3] == ([draws[5]], [6])


def test_minus_zero_ties_with_plus_zero_and_a_nan_beats_plus_infinity():
    seed, draws = key_with_distinct_draws(4)
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        score = by_node({draws[0]: first, draws[1]: second}, -1)
        assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 4, score)[1:3] == ([draws[0]], [1])     # a tie, not -0 < +0
    score = by_node({draws[0]: np.inf, draws[2]: np.nan, draws[3]: np.inf}, 9)
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 4, score)[1:3] == ([draws[2]], [3])
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 2, score)[1:3] == ([draws[0]], [1])
    negative_nan = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    score = by_node({draws[1]: negative_nan, draws[2]: np.nan}, np.inf)
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 4, score)[1:3] == ([draws[1]], [2])         # any NaN, the earlier one
    score = by_node({draws[3]: -1e30}, -np.inf)
    assert hs.hard_ref([0], CSRS_OPEN, NU, NI, seed, 4, 4, score)[1:3] == ([draws[3]], [4])         # -inf is last


def test_fewer_admissible_attempts_than_candidates_and_none_at_all():
    for seed in range(1000):
        key = ss.sample_key(seed, 1, 0)
        ign = hs.ignore_leaving(key, NU, NI, 4)
        draws = ss.candidates(key, NU, NI)
        if ign is not None and sum(node not in ign for node in draws) == 3:
            break
    else:
        raise AssertionError("no seed below 1000 leaves three admissible attempts")
    kept = [(a + 1, node) for a, node in enumerate(draws) if node not in ign]
    assert len(kept) == 3 and len({node for _, node in kept}) == 1 and len(ign) == NI - 1
    csrs = (ss.csr(NU, POS), ss.csr(NU, {0: ign, 1: ALL}))
    pos, neg, attempt, admissible, status = hs.hard_ref([0, 1], csrs, NU, NI, seed, 1, 8, lambda u, item: np.float32(item))
    assert admissible == [3, 0] and status == ss.ST_SAMPLER_EXHAUSTED
    assert (neg[0], attempt[0]) == (kept[0][1], kept[0][0])                                         # one node three times: a tie
    assert (neg[1], attempt[1]) == (ss.candidates(ss.sample_key(seed, 1, 1), NU, NI)[255], 256)
    assert hs.hard_ref([0, 1], csrs, NU, NI, seed, 1, 2, lambda u, item: np.float32(item))[3] == [2, 0]


# ---------------------------------------------------------------------------------------------------------------
# the device tests' cases, judged by the reference alone
# ---------------------------------------------------------------------------------------------------------------
def float64_scores(b):
    panel = b.user_table.astype(np.float64) @ b.item_table.astype(np.float64).T
    return lambda u, item: np.float32(panel[u, item])


@pytest.fixture(scope="module")
def built():
    out = {}
    for c in hs.CASES:
        b = hs.build(c)
        with np.errstate(all="ignore"):
            out[c.name] = (b, hs.walk(b.users, b.csrs, b.n_users, b.n_items, c.seed, c.step, c.n_cand, float64_scores(b)))
    return out


def test_constructed_ignore_sets_do_what_their_names_say(built):
    roles = set()
    for b, recs in built.values():
        c = b.case
        assert len(b.users) == c.n == len(recs)
        for u in range(b.n_users):
            row = b.csrs[1][1][b.csrs[1][0][u]:b.csrs[1][0][u + 1]]
            assert row == sorted(set(row)) and all(b.n_users <= x < b.n_users + b.n_items for x in row)
        for i, role in b.expect.items():
            r = recs[i]
            roles.add(role)
            if role == "short":
                assert 0 < r.admissible < c.n_cand and r.spent == 256 and r.status == 0, (c.name, i)
            else:
                assert r.admissible == c.n_cand and r.spent == r.taken[-1][0] == int(role[2:]), (c.name, i)
    assert roles >= {"at64", "at65", "at128", "at129", "at256", "short"}
    # an empty ignore set with 64 and 65 candidates ends at attempts 64 and 65 as well
    assert built["m64"][1][0].spent == 64 and built["m65"][1][0].spent == 65 and built["m256"][1][0].spent == 256


def test_case_table_reaches_every_path_and_every_listed_shape(built):
    seen = set()
    for b, recs in built.values():
        seen |= hs.paths(b, recs)
    assert seen >= hs.ALL_PATHS, hs.ALL_PATHS - seen
    cases = hs.CASES
    assert {c.dim for c in cases} >= {1, 3, 4, 5, 63, 64, 90, 256}
    assert {c.n for c in cases} >= {1, 3, 4, 5, 257}
    assert {c.n_cand for c in cases} >= {1, 2, 63, 64, 65, 128, 255, 256}
    assert {c.n_items for c in cases} >= {1, 2, 97}
    assert any(c.seed >= 2 ** 32 for c in cases) and any(c.step >= 2 ** 32 for c in cases) and any(c.step == 2 ** 64 - 1 for c in cases)
    assert any(c.us == 3 and c.is_ == 3 for c in cases) and any(c.us != c.is_ for c in cases) and any(c.uoff % 4 for c in cases)
    assert {hs.load_form(c) for c in cases if c.dim == 64} == {"vec", "dword"}                      # alignment alone decides it
    for name in ("dim64", "dim90", "m1", "zero_table"):                                             # bad users among good ones
        b, recs = built[name]
        kinds = {r.user for r in recs if r.bad}
        assert kinds >= {hs.U_NOPOS, b.n_users, -1, 2 ** 40, -2 ** 40} and sum(not r.bad for r in recs) > 200
        assert recs[-1].status == ss.ST_SAMPLER_EXHAUSTED
    # the last item of the catalogue is a candidate, and where its row is the hot one it wins
    b, recs = built["last_item_wins"]
    last = b.n_users + b.n_items - 1
    assert any(r.neg == last and r.attempt > 1 for r in recs)
    assert any(last in [node for _, node in r.taken] for r in built["dim64"][1])
    # ties exist where they are meant to: duplicate rows are drawn together
    b, recs = built["duplicate_rows"]
    assert any(len({(node - b.n_users) % 5 for _, node in r.taken}) < len({node for _, node in r.taken}) for r in recs)
    # the special rows produce NaN, +inf and -inf scores among the candidates
    b, recs = built["specials"]
    with np.errstate(all="ignore"):
        score = float64_scores(b)
        got = np.array([score(r.user, node - b.n_users) for r in recs for _, node in r.taken])
    assert np.isnan(got).any() and np.isposinf(got).any() and np.isneginf(got).any()


def test_poisoned_buffers_keep_the_rows_and_nothing_else():
    t = np.arange(12, dtype=np.float32).reshape(3, 4)
    flat = hs.poisoned(t, 7, 1)
    assert flat.size == 1 + 3 * 7 + 64 and np.isnan(flat[0]) and np.isnan(flat[-64:]).all()
    rows = flat[1:22].reshape(3, 7)
    assert (rows[:, :4] == t).all() and np.isnan(rows[:, 4:]).all()


# ---------------------------------------------------------------------------------------------------------------
# the Python layer's own checks: they come before anything touches a device
# ---------------------------------------------------------------------------------------------------------------
def bare_sampler(n_users=5, n_items=7):
    s = TripleSampler.__new__(TripleSampler)
    s.n_users, s.n_items, s.device = n_users, n_items, torch.device("cuda:0")
    return s


def test_sample_hard_rejects_tables_and_candidate_counts_it_cannot_take():
    s = bare_sampler()
    good = torch.zeros(12, 8)
    with pytest.raises(TypeError):
        s.sample_hard(2, good.numpy())
    with pytest.raises(TypeError):
        s.sample_hard(2, good.double())
    with pytest.raises(TypeError):
        s.sample_hard(2, good.half())
    with pytest.raises(TypeError):
        s.sample_hard(2, good, candidates=2.0)
    with pytest.raises(TypeError):
        s.sample_hard(2, good, candidates=True)
    for m in (0, -1, 257):
        with pytest.raises(ValueError, match="candidates"):
            s.sample_hard(2, good, candidates=m)
    with pytest.raises(ValueError, match="rows"):
        s.sample_hard(2, torch.zeros(11, 8))
    with pytest.raises(ValueError, match="rows"):
        s.sample_hard(2, torch.zeros(13, 8))
    for shape in ((12,), (12, 8, 1), (12, 0)):
        with pytest.raises(ValueError):
            s.sample_hard(2, torch.zeros(shape))
    with pytest.raises(ValueError, match="stride"):
        s.sample_hard(2, torch.zeros(8, 12).t())
    with pytest.raises(ValueError, match="stride"):
        s.sample_hard(2, torch.zeros(12, 16)[:, ::2])
    with pytest.raises(ValueError, match="is on cpu"):                                              # every other check passed
        s.sample_hard(2, good)
    with pytest.raises(ValueError, match="is on cpu"):
        s.sample_hard(2, torch.zeros(12, 11)[:, :8], candidates=256)
