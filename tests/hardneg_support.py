"""Reference and case table of the hard-negative sampler (lgc_sample_hard_triples): tests/test_hardneg_host.py and
tests/test_hardneg_gpu.py.  The stream is tests/sampler_support.py's and the order of the winner is tests/topk_support.py's;
neither is restated here.  Scores come in through a callback, so the reference itself does no floating-point arithmetic: the
device test hands it lgc_score_rows' panel, the host test integer-valued tables.  Every case is built from the reference
alone -- an ignore set "whose 2nd admissible attempt is attempt 64" is constructed from the candidates the stream gives that
sample, and the host test checks that it does what its name says."""
from types import SimpleNamespace

import numpy as np

import sampler_support as ss
import topk_support as ts

MAX_CAND = 256
ATTEMPTS = ss.MAX_ATTEMPTS
WAVE = 64


def bad_user(u, n_users, pos_ptr):
    return u < 0 or u >= n_users or int(pos_ptr[u + 1]) == int(pos_ptr[u])


def walk(users, csrs, n_users, n_items, seed, step, n_cand, score):
    """One record per sample: pos, neg, attempt, admissible, status bits, `taken` = [(attempt, node)] of its candidates, and
    `spent` = the attempts the walk needed (the n_cand-th admissible one, or all 256)."""
    (pos_ptr, pos_items), (ign_ptr, ign_items) = csrs
    assert 1 <= n_cand <= MAX_CAND
    out = []
    for i, u in enumerate(int(u) for u in users):
        if bad_user(u, n_users, pos_ptr):
            out.append(SimpleNamespace(pos=n_users, neg=n_users, attempt=0, admissible=0, status=ss.ST_INDEX_OOB, taken=[],
                                       spent=0, bad=True, user=u))
            continue
        key = ss.sample_key(seed, step, i)
        begin, count = int(pos_ptr[u]), int(pos_ptr[u + 1]) - int(pos_ptr[u])
        pos = int(pos_items[begin + ss.bounded(ss.mix64(key), count)])
        ignored = {int(x) for x in ign_items[int(ign_ptr[u]):int(ign_ptr[u + 1])]}
        draws = ss.candidates(key, n_users, n_items)
        taken = [(a + 1, node) for a, node in enumerate(draws) if node not in ignored][:n_cand]
        rec = SimpleNamespace(pos=pos, status=0, taken=taken, admissible=len(taken), bad=False, user=u,
                              spent=taken[-1][0] if len(taken) == n_cand else ATTEMPTS)
        if not taken:
            rec.neg, rec.attempt, rec.status = draws[ATTEMPTS - 1], ATTEMPTS, ss.ST_SAMPLER_EXHAUSTED
        else:
            scores = np.array([score(u, node - n_users) for _, node in taken], dtype=np.float32)
            best = int(np.argmax(ts.order_keys(scores)))           # the first of the largest keys: the earlier attempt
            rec.attempt, rec.neg = taken[best]
        out.append(rec)
    return out


def hard_ref(users, csrs, n_users, n_items, seed, step, n_cand, score):
    """(pos, neg, neg_attempt, n_admissible, status) of one launch: lists of Python ints and the OR of the status bits.
    ``score(u, item)`` is the score of user u and item index `item` (without the n_users offset) as an fp32 value."""
    recs = walk(users, csrs, n_users, n_items, seed, step, n_cand, score)
    status = 0
    for r in recs:
        status |= r.status
    return ([r.pos for r in recs], [r.neg for r in recs], [r.attempt for r in recs], [r.admissible for r in recs], status)


# ----------------------------------------------------------------------------------------
# ignore sets built from a sample's own draws
# ----------------------------------------------------------------------------------------
def ignore_mth_at(key, n_users, n_items, m, target):
    """A sorted ignore set under which the m-th admissible attempt of sample ``key`` is attempt ``target``; None where these
    draws allow none.  The target's item is free with all its occurrences; further items, latest first, are freed where their
    occurrences before ``target`` still fit into m."""
    draws = ss.candidates(key, n_users, n_items, target)
    last = draws[target - 1]
    need = m - draws.count(last)
    if need < 0:
        return None
    free = {last}
    for node in reversed(draws[:-1]):
        if node not in free and draws.count(node) <= need:
            free.add(node)
            need -= draws.count(node)
    if need:
        return None
    return sorted(set(draws) - free)


def ignore_leaving(key, n_users, n_items, below):
    """A sorted ignore set that leaves 1 .. below - 1 admissible attempts among all 256 (as many as can be had): every item
    but one is ignored.  None where no item is drawn that rarely."""
    draws = ss.candidates(key, n_users, n_items)
    counts = {node: draws.count(node) for node in set(draws)}
    fit = [(c, node) for node, c in counts.items() if 1 <= c < below]
    if not fit:
        return None
    keep = max(fit)[1]
    return [n_users + it for it in range(n_items) if n_users + it != keep]


# ----------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------
# users 0 .. 5 of every world; constructed users follow
U_NONE, U_FIRST, U_LAST, U_HALF, U_FULL, U_NOPOS = range(6)
ORDINARY = [U_NONE, U_FIRST, U_LAST, U_HALF]
OUTSIDE = [-1, 2 ** 40, -2 ** 40]             # plus n_users itself, appended where a case mixes bad users in

NAN_POS, NAN_NEG, INF_POS, INF_NEG = 0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000


def case(name, dim, n_cand, n=5, n_items=97, seed=7, step=3, kind="random", us=0, is_=0, uoff=0, ioff=0, roles=(), bad=False,
         full=False):
    return SimpleNamespace(name=name, dim=dim, n_cand=n_cand, n=n, n_items=n_items, seed=seed, step=step, kind=kind, us=us,
                           is_=is_, uoff=uoff, ioff=ioff, roles=tuple(roles), bad=bad, full=full)


BIG = 2 ** 32
CASES = (
    # widths and the two load forms; strides, poison and misaligned bases
    case("dim1", 1, 8), case("dim3", 3, 8, n=3), case("dim4", 4, 8, n=4), case("dim5", 5, 8),
    case("dim63", 63, 8), case("dim64", 64, 8, n=257, bad=True, full=True), case("dim90", 90, 8, n=257, bad=True, full=True),
    case("dim256", 256, 8), case("dim64_pad3", 64, 8, us=3, is_=3), case("dim90_pad3", 90, 4, us=3, is_=3, n=4),
    case("dim4_pad3", 4, 2, us=3, is_=3), case("dim64_strides_differ", 64, 8, us=4, is_=8),
    case("dim64_item_stride_4k", 64, 8, us=3, is_=4), case("dim64_user_base_off", 64, 8, uoff=1),
    case("dim64_both_bases_off", 64, 8, uoff=1, ioff=1), case("dim256_item_base_off", 256, 4, ioff=3, n=3),
    # how many candidates: one, two, and around the rounds of 64 attempts
    case("m1", 64, 1, n=257, bad=True, full=True), case("m2", 90, 2), case("m63", 64, 63), case("m64", 64, 64, n=4),
    case("m65", 90, 65), case("m128", 64, 128, n=3), case("m255", 5, 255), case("m256", 64, 256, n=4, full=True),
    case("m256_one_sample", 90, 256, n=1),
    # catalogues of one and two items
    case("one_item", 64, 8, n_items=1, full=True), case("two_items", 90, 64, n_items=2, full=True),
    case("two_items_m256", 4, 256, n_items=2, n=3),
    # seeds and steps past 32 bits
    case("seed_2_32", 64, 8, seed=BIG, step=BIG + 1), case("seed_top", 90, 8, seed=2 ** 64 - 1, step=2 ** 63),
    case("step_top", 64, 65, seed=BIG + 9, step=2 ** 64 - 1),
    # ignore sets built from the draws
    case("at64_m2", 64, 2, n=8, roles=("at64", "at65", "at64", "at65")), case("at64_m8", 90, 8, n=8, roles=("at64", "at65")),
    case("at128_m3", 64, 3, n=6, roles=("at128", "at129", "at192", "at193")),
    case("at256_m8", 90, 8, n=3, roles=("at256",)),
    case("short", 64, 8, n=8, roles=("short", "short", "short"), full=True),
    case("short_m2", 3, 2, n=5, roles=("short", "short")),
    # ties and special values
    case("zero_table", 64, 8, kind="zero", n=257, bad=True, full=True), case("zero_table_m256", 90, 256, kind="zero"),
    case("duplicate_rows", 64, 16, kind="dup"), case("duplicate_rows_d90", 90, 64, kind="dup", n=4),
    case("specials", 64, 8, kind="special", n=257), case("specials_d5_m64", 5, 64, kind="special", is_=3),
    case("specials_m256", 90, 256, kind="special", n=4, full=True),
    case("last_item_wins", 64, 64, kind="lasthot", n=5), case("bad_users_only", 64, 8, n=4, bad="only"),
)
CASE_NAMES = [c.name for c in CASES]


def build(c):
    """The inputs of a case: users, the two CSRs, the two tables as flat fp32 buffers with their views, and `expect`: what
    the constructed samples were built for, {sample: (role, attempt)}."""
    rng = np.random.default_rng(sum(map(ord, c.name)))
    nu0, ni = 6, c.n_items
    n_users = nu0 + len(c.roles)
    first, last = n_users, n_users + ni - 1
    every = list(range(first, last + 1))
    pos = {U_NONE: [first, last, first], U_FIRST: [last], U_LAST: [first], U_HALF: [every[len(every) // 2]], U_FULL: [first]}
    ign = {U_NONE: [], U_FIRST: [first], U_LAST: [last], U_HALF: every[1::2], U_FULL: every}
    users = [ORDINARY[i % 4] for i in range(c.n)]
    if c.bad == "only":
        users = ([n_users] + OUTSIDE + [U_NOPOS])[:c.n]
    expect = {}
    for j, role in enumerate(c.roles):                     # constructed users sit at samples 1, 2, ...: each its own user
        i, u = 1 + j, nu0 + j
        key = ss.sample_key(c.seed, c.step, i)
        if role == "short":
            ign_u = ignore_leaving(key, n_users, ni, c.n_cand)
        else:
            ign_u = ignore_mth_at(key, n_users, ni, c.n_cand, int(role[2:]))
        assert ign_u is not None, (c.name, role, i)
        users[i], pos[u], ign[u], expect[i] = u, [last], ign_u, role
    if c.full and c.n > len(c.roles) + 1:
        users[-1] = U_FULL
    if c.bad is True:
        for i, u in zip(range(len(c.roles) + 2, c.n, 9), [U_NOPOS, n_users] + OUTSIDE + [U_NOPOS]):
            users[i] = u
    csrs = (ss.csr(n_users, pos), ss.csr(n_users, {u: sorted(v) for u, v in ign.items()}))

    ut = rng.standard_normal((n_users, c.dim)).astype(np.float32)
    it = rng.standard_normal((ni, c.dim)).astype(np.float32)
    if c.kind == "zero":
        ut[:], it[:] = 0.0, 0.0
    elif c.kind == "dup":
        it = it[np.arange(ni) % 5]
    elif c.kind == "lasthot":
        ut, it[-1] = np.abs(ut) + np.float32(0.5), 10.0
    elif c.kind == "special":
        bits = it.view(np.uint32)
        for r in range(ni):
            col, k = r % c.dim, r % 8
            if k == 1:
                bits[r, col] = NAN_POS
            elif k == 2:
                bits[r, col] = NAN_NEG
            elif k == 3:
                bits[r, col] = INF_POS
            elif k == 4:
                bits[r, col] = INF_NEG
            elif k == 5:
                bits[r] = (bits[r] & 0x80000000) | (1 + (bits[r] & 0x3FF))      # a row of subnormals of both signs
            elif k == 6:
                it[r] *= np.float32(1e-30)                                      # products that underflow
        ut[U_LAST] *= np.float32(1e-12)
    return SimpleNamespace(case=c, users=users, csrs=csrs, n_users=n_users, n_items=ni, expect=expect,
                           user_table=ut, item_table=it, user_stride=c.dim + c.us, item_stride=c.dim + c.is_)


def poisoned(table, stride, offset):
    """(flat fp32 buffer, offset): the rows of ``table`` `stride` floats apart from float `offset` on, every other float of the
    buffer -- the padding columns, the floats before the first row and 64 floats behind the last row's last column -- a NaN."""
    rows, dim = table.shape
    flat = np.full(offset + rows * stride + 64, np.nan, dtype=np.float32)
    view = flat[offset:offset + rows * stride].reshape(rows, stride)
    view[:, :dim] = table
    return flat


def load_form(c):
    """Which load form the launch takes: 16-byte loads where the width is a multiple of 4 and every item row starts on 16
    bytes (the buffers themselves are 16-byte aligned), dword loads otherwise."""
    return "vec" if c.dim % 4 == 0 and (c.dim + c.is_) % 4 == 0 and c.ioff % 4 == 0 else "dword"


ALL_PATHS = {"vec", "dword", "rounds1", "rounds2", "rounds4", "early_stop", "short", "exhausted", "bad_user"}


def paths(b, recs):
    """The paths case ``b`` reaches, from the reference's records of its samples."""
    seen = {load_form(b.case)}
    for r in recs:
        if r.bad:
            seen.add("bad_user")
            continue
        rounds = -(-r.spent // WAVE)
        seen.add(f"rounds{rounds}")
        if r.admissible == b.case.n_cand and rounds < ATTEMPTS // WAVE:
            seen.add("early_stop")
        if 0 < r.admissible < b.case.n_cand:
            seen.add("short")
        if r.admissible == 0:
            seen.add("exhausted")
    return seen
