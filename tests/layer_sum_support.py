"""One graph, two fp64 references and a path recorder for the tests of ``propagate.bipartite_sum`` over every path it
takes (tests/test_layer_sum_paths_host.py, tests/test_layer_sum_paths_gpu.py).

The graph: 700 users x 45 items as a directed edge list in the reference's layout (eliminate_support._coo).  45 items at
eight gaps give gap_rows = 6 and three unused rows in the last gap of the concatenated operator [R_H^T | G_L].

* item HUB is in every user's list but the isolated user's, item EMPTY in none, item SINGLE in one;
* the items of LIGHT are in 2, 5, 8 .. 23 lists;
* a user's list holds HUB and u % 12 of the other items: the degrees cycle through 1 .. 12, so that T = 3 and T = 4 both
  eliminate a quarter to a third of the users and keep the others;
* user ISOLATED has no edge at all;
* one (user, item) pair is listed twice;
* every seventh pair is missing from its ITEM's row (``drop_item_rows``), so that the two directions disagree.

The references are functions of (rows, cols, vals, x0, alphas) and run without a device:
``want`` = sum_l alpha_l A^l x0 and ``mag`` = sum_l |alpha_l| |A|^l |x0|, the size of the terms a row's fp32 sum handles --
the denominator for a row whose terms cancel.
"""
import numpy as np
import torch

from eliminate_support import _coo, csr_host, layer_sum_coo_fp64

N_USERS, N_ITEMS = 700, 45
N = N_USERS + N_ITEMS
HUB, EMPTY, SINGLE = 5, 17, 23
LIGHT = (30, 31, 32, 33, 34, 35, 36, 37)
ISOLATED = 333
SINGLE_USER = 7
DOUBLED = 10                               # position of the pair that is listed twice
N_GAPS = 8
# the planner configuration of test_mix_epilogue_gpu.SMALL_PLAN: pieces of at most 8 entries, the hub row beyond 32 slots
SMALL_PLAN = dict(waves_per_band_round=8, row_cap=20, piece_cap=8)
SWEPT = (62, 64, 68, 90, 96, 97, 128)      # both ends of 61..64 (four entries), 68..96 (two), 97..128 (two passes)
NOT_SWEPT = 20
LAYERS = (1, 2, 3, 4, 5, 7)                # 5: the reference's K; 7: the last K before the Horner fallback


def pairs():
    """The (user, item) pairs in list order, the doubled one last."""
    rng = np.random.default_rng(20261020)
    others = np.array([i for i in range(N_ITEMS) if i not in (HUB, EMPTY, SINGLE) + LIGHT])
    out = []
    for u in range(N_USERS):
        if u == ISOLATED:
            continue
        out.append((u, HUB))
        for i in rng.choice(others, size=u % 12, replace=False):
            out.append((u, int(i)))
    out.append((SINGLE_USER, SINGLE))
    connected = np.array([u for u in range(N_USERS) if u != ISOLATED])
    for j, i in enumerate(LIGHT):                                 # 2, 5, 8, ... 23 lists
        for u in rng.choice(connected, size=2 + 3 * j, replace=False):
            out.append((int(u), i))
    out.append(out[DOUBLED])
    return out


def dropped(n_pairs):
    """Positions whose item-row entry is left out: every seventh, never the doubled pair's second listing."""
    return range(0, n_pairs - 1, 7)


def edge_list():
    p = pairs()
    return _coo(N_USERS, p, drop_item_rows=dropped(len(p)))


def eliminated(ei, max_deg):
    """bool [N_USERS]: the users that leave the middle layers at T = max_deg (the rule of lgc_reduce_count: at most T
    entries in the user's row, and at most T item rows name the user)."""
    src, dst = ei[0].numpy(), ei[1].numpy()
    deg = np.bincount(dst[dst < N_USERS], minlength=N_USERS)
    named = np.bincount(src[(dst >= N_USERS) & (src < N_USERS)], minlength=N_USERS)
    return (deg <= max_deg) & (named <= max_deg)


def listed_rows(ei):
    """48 user ids and 48 item ids (node ids, int64 on the host): HUB, EMPTY, SINGLE, the isolated user, a user that
    T = 3 and T = 4 both eliminate, one that both keep, and a repeated id on either side."""
    gone3, gone4 = eliminated(ei, 3), eliminated(ei, 4)
    connected = np.arange(N_USERS) != ISOLATED
    gone_user = int(np.flatnonzero(gone3 & gone4 & connected)[0])
    kept_user = int(np.flatnonzero(~gone3 & ~gone4)[0])
    rng = np.random.default_rng(48)
    users = [ISOLATED, gone_user, kept_user, SINGLE_USER, kept_user]
    users += [int(u) for u in rng.choice(N_USERS, size=48 - len(users), replace=False)]
    items = [HUB, EMPTY, SINGLE, LIGHT[0], HUB]
    items += [int(i) for i in rng.choice(N_ITEMS, size=48 - len(items), replace=True)]
    return torch.tensor(users + [N_USERS + i for i in items], dtype=torch.int64), gone_user, kept_user


def want_fp64(rows, cols, vals, x0, alphas):
    """sum_l alpha_l A^l x0 in fp64 for A[rows[e], cols[e]] += vals[e]."""
    return layer_sum_coo_fp64(rows, cols, vals, x0, alphas)


def mag_fp64(rows, cols, vals, x0, alphas):
    """sum_l |alpha_l| |A|^l |x0|: the same recursion on absolute values."""
    return layer_sum_coo_fp64(rows, cols, vals.double().abs(), x0.cpu().double().abs(), [abs(a) for a in alphas])


def operator_coo(op):
    """(rows, cols, vals fp64 from the operator's own fp32 bits) of an operator's CSR, on the host."""
    _, cols, vals, rows = csr_host(op)
    return rows, cols, vals


def row_ratios(got, want, mag):
    """||got_r - want_r||_2 / ||mag_r||_2 per row, fp64 [rows]; a row of zero magnitude must match exactly."""
    num, den = (got.double() - want).norm(dim=1), mag.norm(dim=1)
    zero = den == 0
    assert (num[zero] == 0).all(), "a row whose terms are all exact zeros must be exactly zero"
    return torch.where(zero, torch.zeros_like(num), num / den.clamp_min(1e-300))


class Recorder:
    """Which operator objects ``Operator.apply`` and ``propagate.apply_rows`` were called on, in call order:
    ("apply", operator, has a second epilogue row) and ("rows", operator, split)."""

    def __init__(self, monkeypatch, graph_module, propagate_module):
        self.events = []
        real_apply, real_rows = graph_module.Operator.apply, propagate_module.apply_rows
        rec = self

        def apply(self, x, out, a=1.0, r=None, b=0.0, r2=None, b2=0.0):
            rec.events.append(("apply", self, r2 is not None))
            return real_apply(self, x, out, a=a, r=r, b=b, r2=r2, b2=b2)

        def apply_rows(op, rows, x, out, a=1.0, r=None, b=0.0, split=False, compact=False):
            rec.events.append(("rows", op, bool(split)))
            return real_rows(op, rows, x, out, a=a, r=r, b=b, split=split, compact=compact)
        monkeypatch.setattr(graph_module.Operator, "apply", apply)
        monkeypatch.setattr(propagate_module, "apply_rows", apply_rows)

    def clear(self):
        self.events = []

    def applies(self, op):
        return sum(1 for kind, o, _ in self.events if kind == "apply" and o is op)

    def rows_calls(self, op, split):
        return sum(1 for kind, o, s in self.events if kind == "rows" and o is op and s == split)

    def operators(self):
        seen = []
        for _, o, _ in self.events:
            if not any(o is s for s in seen):
                seen.append(o)
        return seen
