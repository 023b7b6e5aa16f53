"""What the two ranking-metric test modules share: a plain numpy fp64 restatement of lgc_rank_metrics written from the
definitions in include/lgconv_hip.h (a per-row Python loop with ``set``; every sum is taken afresh per cutoff, nothing
is shared with the kernel's running sums), the frame MARK_MAPK would build from it, and the synthetic cases."""
import functools

import numpy as np

PRECISION, RECALL, NDCG, AP, RR, HIT, COUNT = range(7)
N_ITEMS = 300


def discount(j):
    return 1.0 / np.log2(np.float64(j) + 2.0)


def reference(topk, ptr, items, users, cutoffs):
    """(hits int32 [n, C], metrics float64 [n, C, 6], bits uint64 [n, 4]) for ``topk`` [n, k] against the CSR ``ptr`` /
    ``items`` and the user of each row.  A user outside the CSR: the row is all zero.  An empty list: 0 / 0 = NaN."""
    topk, ptr, items = np.asarray(topk), np.asarray(ptr), np.asarray(items)
    n, k, n_users = topk.shape[0], topk.shape[1], len(ptr) - 1
    hits = np.zeros((n, len(cutoffs)), dtype=np.int32)
    metrics = np.zeros((n, len(cutoffs), COUNT), dtype=np.float64)
    bits = np.zeros((n, 4), dtype=np.uint64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(n):
            u = int(users[r])
            if not 0 <= u < n_users:
                continue
            listed = [int(x) for x in items[ptr[u]:ptr[u + 1]]]
            positives = set(listed)
            length, distinct = np.float64(len(listed)), len(positives)
            rel = [int(x) in positives for x in topk[r]]
            for j in range(k):
                if rel[j]:
                    bits[r, j // 64] |= np.uint64(1) << np.uint64(j % 64)
            for ci, c in enumerate(cutoffs):
                h = sum(rel[:c])
                dcg = sum(discount(j) for j in range(c) if rel[j])
                idcg = sum(discount(j) for j in range(min(c, distinct)))
                ap = sum(np.float64(sum(rel[:j + 1])) / np.float64(j + 1) for j in range(c) if rel[j])
                first = next((j for j in range(c) if rel[j]), None)
                hits[r, ci] = h
                metrics[r, ci, PRECISION] = np.float64(h) / np.float64(c)
                metrics[r, ci, RECALL] = np.float64(h) / length
                metrics[r, ci, NDCG] = np.float64(dcg) / np.float64(idcg)
                metrics[r, ci, AP] = np.float64(ap) / np.float64(min(c, distinct))
                metrics[r, ci, RR] = 0.0 if first is None else np.float64(1.0) / np.float64(first + 1)
                metrics[r, ci, HIT] = 1.0 if h > 0 else 0.0
    return hits, metrics, bits


def reference_frame(pos_list_df, users, topk, ptr, items, cutoff):
    """MARK_MAPK's third value restated on ``reference``: the left merge and its three derived columns, ``overlap_item``
    in the ranking's order."""
    import pandas as pd
    top = np.asarray(topk)[:, :cutoff]
    _, metrics, bits = reference(top, ptr, items, users, (cutoff,))
    overlap = [[int(x) for j, x in enumerate(row) if (int(b[j // 64]) >> (j % 64)) & 1] for row, b in zip(top, bits)]
    per_row = pd.DataFrame({"user_ID": np.asarray(users, dtype=np.int64), "top_rlvnt_itm": top.tolist(), "overlap_item": overlap,
                            "recall": metrics[:, 0, RECALL], "precision": metrics[:, 0, PRECISION]})
    per_row = per_row.drop_duplicates("user_ID", ignore_index=True)
    return pd.merge(pos_list_df, per_row, how="left", left_on="user_id_idx", right_on="user_ID")


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    items = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if lists else np.zeros(0, dtype=np.int64)
    return ptr, items.astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(n_rows, k, cutoffs, lengths, seed=0):
    """One synthetic case, built once and shared (treat as read-only): a dict with ``topk`` [n_rows, k] of random
    distinct item ids below N_ITEMS per row, positive lists of the given ``lengths`` (cycled over 11 users; every odd
    user's list of two or more repeats one of its items) as a CSR, ``users`` in no order with, from two rows on, one
    user on two rows, and ``want`` = ``reference`` of it."""
    rng = np.random.default_rng(1000 * seed + 17 * n_rows + k)
    n_users = 11
    lists = []
    for u in range(n_users):
        length = lengths[u % len(lengths)]
        lst = rng.permutation(N_ITEMS)[:min(length, N_ITEMS)]
        if length > N_ITEMS:
            lst = np.concatenate([lst, rng.integers(N_ITEMS, size=length - N_ITEMS)])
        if u % 2 == 1 and length > 1:
            lst[-1] = lst[0]                                              # a duplicate: len = distinct + 1
        lists.append(lst.astype(np.int64))
    ptr, items = csr(lists)
    topk = np.stack([rng.permutation(N_ITEMS)[:k] for _ in range(n_rows)]).astype(np.int64)
    users = rng.permutation(n_users)[np.arange(n_rows) % n_users].astype(np.int64)     # every user before any repeats
    if n_rows > 1:
        users[-1] = users[0]
    return dict(topk=topk, ptr=ptr, items=items, users=users, cutoffs=tuple(cutoffs), n_users=n_users,
                want=reference(topk, ptr, items, users, cutoffs))
