"""Graphs and fp64 references for the middle-hop reduction tests (tests/test_eliminate_gpu.py, tests/eliminate_child.py).

Every graph is a directed edge list in the reference's layout (edge_index int64 [2, E], row 0 = source, row 1 = target;
users first), small enough that the fp64 references are dense matrices on the host.
"""
import numpy as np
import torch

from gnn_ecommerce_amd import synth


def _coo(n_users, pairs, drop_item_rows=(), extra=()):
    """Both directions of every (user, item) pair; ``drop_item_rows``: positions whose user -> item direction (an entry
    of the ITEM's row) is left out; ``extra``: (source, target) node pairs appended as they are."""
    u = np.array([p[0] for p in pairs], dtype=np.int64)
    i = np.array([p[1] for p in pairs], dtype=np.int64) + n_users
    keep = np.ones(len(pairs), dtype=bool)
    keep[list(drop_item_rows)] = False
    src = np.concatenate([i, u[keep], np.array([e[0] for e in extra], dtype=np.int64)])
    dst = np.concatenate([u, i[keep], np.array([e[1] for e in extra], dtype=np.int64)])
    ei = torch.from_numpy(np.stack([src, dst]))
    rng = np.random.default_rng(len(pairs))
    ew = torch.from_numpy(rng.uniform(0.5, 2.0, ei.size(1)).astype(np.float32))
    return ei, ew


def _lists(rng, n_users, n_items, degree_of, first_item=0):
    pairs = []
    for u in range(n_users):
        d = degree_of(u)
        for i in rng.choice(np.arange(first_item, n_items), size=d, replace=False):
            pairs.append((u, int(i)))
    return pairs


def graph_degrees_1_to_12():
    """(a) 300 users x 40 items, user degrees 1 .. 12; T = 3."""
    rng = np.random.default_rng(1)
    pairs = _lists(rng, 300, 40, lambda u: 1 + u % 12)
    return (*_coo(300, pairs), 300, 340, 3)


def graph_hub():
    """(b) 2,000 x 400, item 0 in every user's list; T = 4: the hub's G_L row has far more than 256 entries."""
    rng = np.random.default_rng(2)
    pairs = []
    for u in range(2000):
        pairs.append((u, 0))
        for i in rng.choice(np.arange(1, 400), size=u % 8, replace=False):
            pairs.append((u, int(i)))
    return (*_coo(2000, pairs), 2000, 2400, 4)


def graph_all_eliminated():
    """(c) every user has at most 3 entries; T = 3: n_h = 0, the kept half is empty."""
    rng = np.random.default_rng(3)
    pairs = _lists(rng, 200, 30, lambda u: 1 + u % 3)
    return (*_coo(200, pairs), 200, 230, 3)


def graph_none_eliminated():
    """(d) every user has at least 4 entries; T = 3: G_L is empty."""
    rng = np.random.default_rng(4)
    pairs = _lists(rng, 200, 30, lambda u: 4 + u % 5)
    return (*_coo(200, pairs), 200, 230, 3)


def graph_directed():
    """(e) as (a) with every seventh item-row entry removed (a user whose row says 3 items but whom only 2 item rows
    name, and the like) and one pair listed twice; T = 3."""
    rng = np.random.default_rng(5)
    pairs = _lists(rng, 300, 40, lambda u: 1 + u % 12)
    pairs.append(pairs[10])
    return (*_coo(300, pairs, drop_item_rows=range(0, len(pairs) - 1, 7)), 300, 340, 3)


def graph_item_extremes():
    """(f) item 0 is listed by users of 2 entries only (all eliminated at T = 3), item 1 by users of 6 only (none)."""
    rng = np.random.default_rng(6)
    pairs = []
    for u in range(240):
        if u < 60:
            own, d = [0], 1
        elif u < 120:
            own, d = [1], 5
        else:
            own, d = [], 1 + u % 9
        for i in own + [int(i) for i in rng.choice(np.arange(2, 50), size=d, replace=False)]:
            pairs.append((u, i))
    return (*_coo(240, pairs), 240, 290, 3)


def graph_nothing_left():
    """(g) 60 x 10, every user has at most 3 entries and no item row holds an entry (all of them dropped); T = 3: n_h = 0
    and G_L is empty -- the item step of a reduced layer has no operator at all and only zeroes / copies the block."""
    rng = np.random.default_rng(8)
    pairs = [(59, 0)] + _lists(rng, 59, 10, lambda u: 1 + u % 3)
    return (*_coo(60, pairs, drop_item_rows=range(len(pairs))), 60, 70, 3)


def graph_kept_but_unnamed():
    """(h) 80 x 12, even users have 1 .. 3 entries, odd users 4 .. 6 and no item row names them (their item-row entries
    are dropped); T = 3: kept users exist, the item part of the reduced CSR is empty, G_L is not."""
    rng = np.random.default_rng(9)
    pairs = [(0, 0)] + _lists(rng, 80, 12, lambda u: (4 + u % 3) if u % 2 else ((u // 2) % 3 + (u > 0)))
    return (*_coo(80, pairs, drop_item_rows=[k for k, p in enumerate(pairs) if p[0] % 2]), 80, 92, 3)


GRAPHS = {"degrees_1_to_12": graph_degrees_1_to_12, "hub": graph_hub, "all_eliminated": graph_all_eliminated,
          "none_eliminated": graph_none_eliminated, "directed": graph_directed, "item_extremes": graph_item_extremes,
          "nothing_left": graph_nothing_left, "kept_but_unnamed": graph_kept_but_unnamed}
# built without normalisation: a row without entries has degree zero, and the normalised values on it would be zeros --
# the point of these two is the path taken, with nonzero values
UNNORMALISED = ("nothing_left", "kept_but_unnamed")


def graph_sweep():
    """5,000 x 300 for the forced band sweep of the reduced item half (synth's skewed lists); T = 4."""
    g = synth.make_bipartite(5000, 300, 40000, seed=7)
    ei, ew = g.coo()
    return ei, ew, 5000, 5300, 4


def csr_host(op):
    """(rowptr int64, cols int64, vals fp64 from the fp32 bits, rows int64) of an operator's CSR on the host."""
    rowptr = op.rowptr.cpu().long()
    ent = op.entries.cpu()
    cols = ent[:, 0].long()
    vals = ent[:, 1].contiguous().view(torch.float32).double()
    rows = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])
    return rowptr, cols, vals, rows


def dense_fp64(op, n):
    """The operator as a dense fp64 matrix (duplicate entries add up, as the hop adds them)."""
    _, cols, vals, rows = csr_host(op)
    a = torch.zeros((n, n), dtype=torch.float64)
    a.index_put_((rows, cols), vals, accumulate=True)
    return a


def layer_sum_coo_fp64(rows, cols, vals, x0, alphas):
    """sum_l alpha_l A^l x0 in fp64 on the host for A[rows[e], cols[e]] += vals[e] (sparse product; no device)."""
    n = x0.size(0)
    a = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals.double(), (n, n)).coalesce()
    x = x0.cpu().double()
    out = alphas[0] * x
    for alpha in alphas[1:]:
        x = torch.sparse.mm(a, x)
        out = out + alpha * x
    return out


def layer_sum_fp64(op, x0, alphas):
    """sum_l alpha_l A^l x0 in fp64 on the host, A from the operator's own fp32 values (sparse product)."""
    _, cols, vals, rows = csr_host(op)
    return layer_sum_coo_fp64(rows, cols, vals, x0, alphas)


def alphas_for(k, equal):
    """K + 1 weights, K <= 7: the reference's 1 / (K + 1), or a falling sequence of all different values."""
    if equal:
        return tuple([1.0 / (k + 1)] * (k + 1))
    return tuple(float(v) for v in (0.5 ** np.arange(k + 1) * np.array([1.0, 0.9, 1.1, 0.7, 1.3, 0.8, 1.2, 0.6][:k + 1])))


def eliminated_users(op, split, max_deg):
    """The rule of lgc_reduce_count on the host: bool [split], True = eliminated."""
    rowptr, cols, _, rows = csr_host(op)
    deg = (rowptr[1:] - rowptr[:-1])[:split]
    in_item = rows >= split
    named = torch.bincount(cols[in_item & (cols < split)], minlength=split)[:split]
    return (deg <= max_deg) & (named <= max_deg)


def ulp32(v):
    """Spacing of fp32 at the (fp64) values v, rounded to fp32 first."""
    f = v.float()
    up = torch.nextafter(f.abs(), torch.full_like(f, float("inf")))
    return (up - f.abs()).double()
