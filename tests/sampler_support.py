"""The mini-batch sampler's random stream, restated in Python integers (tests/test_sampler_stream.py).  The device
sampler is counter based and stateless -- draw(seed, step, sample, attempt) -- so every triple it returns is a pure function
of its arguments, and this module computes that function with unbounded integers masked to 64 bits.  No project code is
imported, and nothing here is vectorised: a truncation to 32 bits anywhere in the kernel shows as a different triple."""

M64 = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15          # splitmix64's increment
STEP_MUL = 0xD1B54A32D192ED03        # spreads the step over the counter: counter = step * STEP_MUL + sample
ATTEMPT_MUL = 0x632BE59BD9B4E019     # spreads the attempts of one sample
MAX_ATTEMPTS = 256
ST_INDEX_OOB, ST_SAMPLER_EXHAUSTED = 1, 2


def mix64(z):
    """splitmix64's output function of the state z + GOLDEN (mix64(0) is the first output of splitmix64 seeded with 0)."""
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def bounded(r, span):
    """An integer of [0, span) from a 64-bit draw: the high half of the 128-bit product."""
    assert 0 <= r <= M64 and 0 < span <= M64
    return (r * span) >> 64


def sample_key(seed, step, i):
    return mix64(mix64(seed & M64) ^ mix64(((step & M64) * STEP_MUL + i) & M64))


def candidates(key, n_users, n_items, count=MAX_ATTEMPTS):
    """The negatives sample ``key`` tries, in order (node ids: items are offset by n_users)."""
    return [n_users + bounded(mix64((key + ATTEMPT_MUL * (a + 1)) & M64), n_items) for a in range(count)]


def sample_ref(users, pos_ptr, pos_items, ign_ptr, ign_items, n_users, n_items, seed, step):
    """(pos, neg, status) of one launch: lists of Python ints and the OR of the status bits.  A user outside [0, n_users)
    or without positives gets pos = neg = n_users and raises ST_INDEX_OOB; a user whose first MAX_ATTEMPTS candidates are all
    ignored keeps the last one and raises ST_SAMPLER_EXHAUSTED."""
    pos, neg, status = [], [], 0
    for i, u in enumerate(int(u) for u in users):
        key = sample_key(seed, step, i)
        if u < 0 or u >= n_users or int(pos_ptr[u + 1]) == int(pos_ptr[u]):
            status |= ST_INDEX_OOB
            pos.append(n_users)
            neg.append(n_users)
            continue
        begin, count = int(pos_ptr[u]), int(pos_ptr[u + 1]) - int(pos_ptr[u])
        pos.append(int(pos_items[begin + bounded(mix64(key), count)]))
        ignored = [int(x) for x in ign_items[int(ign_ptr[u]):int(ign_ptr[u + 1])]]
        found = False
        for cand in candidates(key, n_users, n_items):
            if cand not in ignored:
                found = True
                break
        if not found:
            status |= ST_SAMPLER_EXHAUSTED
        neg.append(cand)
    return pos, neg, status


def attempts_needed(key, n_users, n_items, ignored):
    """1-based index of the first candidate outside ``ignored``, or None when all MAX_ATTEMPTS are ignored."""
    for a, cand in enumerate(candidates(key, n_users, n_items)):
        if cand not in ignored:
            return a + 1
    return None


def csr(n_users, lists):
    """{user: items} -> (ptr [n_users + 1], items) as Python lists, each user's items in the order given."""
    ptr, items = [0], []
    for u in range(n_users):
        items += [int(x) for x in lists.get(u, [])]
        ptr.append(len(items))
    return ptr, items
