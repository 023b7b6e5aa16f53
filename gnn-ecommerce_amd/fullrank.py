"""Full-rank evaluation: the exact place of every held-out item among the whole catalogue, and what follows from it.

``recommend_topk`` says which held-out purchases land in the first k <= 256 places; ``lgc_rank_positions`` says where each
one landed, by counting the candidates that precede it on the fp32 matrix cores.  No score is
written to memory.  The scores have the bits of ``score_rows`` and the order is ``mask_topk``'s, so a rank is the column the
item has in ``recommend_topk``'s row wherever that row is long enough -- an integer, never within a tolerance.  From the
ranks: AUC (what BPR is a surrogate for), the mean percentile rank, the reciprocal rank and recall / hit rate at any K.

What this does NOT do: no ``item_ok`` filter, no mid-rank (ties = 1/2) AUC -- ``n_equal`` is reported so that a caller sees
degenerate ties --, and one device.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _native
from .propagate import (PositiveLists, SeenLists, _check_ids, _check_tables, _snapshot_status, _status, check_index_status,
                        column_sums)

__all__ = ["positive_ranks", "evaluate_full_rank", "PairRanks", "FullRankResult", "SEEN_MODES", "pair_metrics"]

SEEN_MODES = tuple(_native.RANK_SEEN_MODES)       # "zero": a seen item competes as score * 0; "remove": it is no candidate
MAX_KS = (_native.COLUMN_SUMS_MAX - 5) // 2       # cutoffs of one evaluate_full_rank: its means are ONE column_sums call


class PairRanks(NamedTuple):
    """Per pair, on the device: ``rank`` int32 (candidates that precede the item; -1 = no answer), ``n_equal`` int32
    (candidates with the item's key), ``n_cand`` int32 (candidates, the item counted) and ``value`` fp32 (its masked
    score)."""
    rank: Tensor
    n_equal: Tensor
    n_cand: Tensor
    value: Tensor


def _check_ascending(seen: SeenLists) -> None:
    """lgc_rank_positions binary-searches a user's list: once per object, one host sync, the verdict kept on it."""
    verdict = getattr(seen, "_ascending", None)
    if verdict is None:
        items, ptr = seen.items, seen.ptr
        if items.numel() < 2:
            verdict = True
        else:
            start = torch.zeros(items.numel() + 1, dtype=torch.bool, device=items.device)
            start[ptr.clamp(0, items.numel())] = True                       # where a list begins, order starts afresh
            verdict = bool(((items[1:] >= items[:-1]) | start[1:-1]).all().item())
        seen._ascending = verdict
    if not verdict:
        raise ValueError("seen lists must be ascending per user (ingest.seen_csr and SeenLists.from_dense produce them so)")


def positive_ranks(users: Tensor, items: Tensor, pair_users: Tensor, pair_items: Tensor, seen: Optional[SeenLists] = None,
                   seen_mode: str = "zero", slices: int = 0) -> PairRanks:
    """Where item ``pair_items[r]`` stands in the ranking of all ``items`` (fp32 ``[n_items, dim]``) for user row
    ``pair_users[r]`` of ``users`` (fp32 ``[n_user_rows, dim]``), in ``mask_topk``'s order: lgc_rank_positions.
    ``seen``: a ``SeenLists`` over all user rows or None.  ``seen_mode`` "zero": a seen item competes with score * 0, as in
    ``recommend_topk``; "remove": seen items are no candidates, and a pair whose item is seen gets rank -1.  ``slices``
    only moves work (0 = the library chooses).  A pair outside the tables gets -1 and raises at ``check_index_status()``."""
    if seen_mode not in _native.RANK_SEEN_MODES:
        raise ValueError(f"seen_mode must be one of {SEEN_MODES}, got {seen_mode!r}")
    if isinstance(slices, bool) or not isinstance(slices, int) or not 0 <= slices <= 64:
        raise ValueError("slices must be an integer in [0, 64]")
    _check_tables(users, items)
    if pair_users is None or pair_items is None:
        raise TypeError("pair_users and pair_items must be contiguous 1-D int64 tensors on the tables' device")
    _check_ids(pair_users, users, "pair_users")
    _check_ids(pair_items, users, "pair_items")
    if pair_users.numel() != pair_items.numel():
        raise ValueError(f"{pair_users.numel()} pair users for {pair_items.numel()} pair items")
    if seen is not None:
        if not isinstance(seen, SeenLists):
            raise TypeError("seen must be a SeenLists (SeenLists.from_dense converts the reference's dense mask) or None")
        _check_ids(seen.ptr, users, "seen.ptr")
        _check_ids(seen.items, users, "seen.items")
        if seen.ptr.numel() != users.size(0) + 1:
            raise ValueError(f"seen.ptr must have {users.size(0) + 1} entries, one list per user row; got {seen.ptr.numel()}")
        _check_ascending(seen)
    dev, n, n_items = users.device, pair_users.numel(), items.size(0)
    rank, n_equal, n_cand = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    value = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return PairRanks(rank, n_equal, n_cand, value)
    lib = _native.load()
    ws_bytes = lib.lgc_rank_positions_workspace_bytes(n, n_items, slices)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    seen_items = None
    if seen is not None:                                   # an empty tensor has no address; the kernels read no entry of it
        seen_items = seen.items if seen.items.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        code = lib.lgc_rank_positions(_native.ptr(users), users.stride(0), users.size(0), _native.ptr(items), items.stride(0),
                                      n_items, users.size(1), _native.ptr(pair_users), _native.ptr(pair_items), n,
                                      _native.ptr(seen.ptr) if seen is not None else None, _native.ptr(seen_items),
                                      _native.RANK_SEEN_MODES[seen_mode], slices, _native.ptr(rank), _native.ptr(n_equal),
                                      _native.ptr(n_cand), _native.ptr(value), _native.ptr(ws), ws_bytes,
                                      _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_rank_positions")
    _snapshot_status(dev)
    return PairRanks(rank, n_equal, n_cand, value)


def pair_metrics(rank: Tensor, n_cand: Tensor, owner: Tensor, length: Tensor, ks) -> dict:
    """The per-user metrics from per-pair ranks, with integer tensor ops up to the last division (any device).  ``rank``,
    ``n_cand``: int [n_pairs] (rank < 0 = the pair does not count); ``owner``: int64 [n_pairs], the user position of a
    pair; ``length``: int64 [n], a user's list length with duplicates.  Returns float64 [n] tensors ``auc``, ``mpr``,
    ``rr``, float64 [n, len(ks)] ``recall`` and ``hit``, and int64 [n] ``n_pos`` (P) and ``n_cand`` (n_c).
      auc = 1 - (sum rank - P (P - 1) / 2) / (P (n_c - P)), NaN when P = 0 or n_c = P
      mpr = mean(rank) / (n_c - 1), NaN when P = 0 or n_c = 1
      rr  = 1 / (min rank + 1), 0 when P = 0
      recall@K = #{rank < K} / len, hit@K = 1 if any rank < K"""
    n, dev = length.numel(), rank.device
    rank, owner = rank.to(torch.int64), owner.to(torch.int64)
    valid = rank >= 0
    zeros = lambda: torch.zeros(n, dtype=torch.int64, device=dev)
    n_pos = zeros().index_add_(0, owner, valid.to(torch.int64))
    total = zeros().index_add_(0, owner, torch.where(valid, rank, 0))
    n_c = zeros().scatter_reduce_(0, owner, torch.where(valid, n_cand.to(torch.int64), 0), "amax", include_self=True)
    big = torch.iinfo(torch.int64).max
    best = torch.full((n,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, owner, torch.where(valid, rank, big), "amin",
                                                                               include_self=True)
    nan = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    wrong = total - n_pos * (n_pos - 1) // 2                               # (candidate, positive) pairs in the wrong order
    space = n_pos * (n_c - n_pos)
    auc = torch.where(space > 0, 1.0 - wrong.to(torch.float64) / space.clamp_min(1).to(torch.float64), nan)
    room = n_pos * (n_c - 1)
    mpr = torch.where(room > 0, total.to(torch.float64) / room.clamp_min(1).to(torch.float64), nan)
    rr = torch.where(n_pos > 0, 1.0 / (best.clamp_max(big - 1) + 1).to(torch.float64), torch.zeros_like(nan))
    counts = torch.stack([zeros().index_add_(0, owner, (valid & (rank < int(k))).to(torch.int64)) for k in ks], dim=1)
    recall = counts.to(torch.float64) / length.to(torch.float64)[:, None]
    hit = (counts > 0).to(torch.float64)
    return {"auc": auc, "mpr": mpr, "rr": rr, "recall": recall, "hit": hit, "n_pos": n_pos, "n_cand": n_c}


class FullRankResult:
    """What ``evaluate_full_rank`` returns.  ``ks``: the cutoffs; ``mean``: a dict -- ``"auc"``, ``"mpr"``, ``"mrr"`` Python
    floats (auc and mpr over the users where they are defined), ``"recall"`` and ``"hit_rate"`` tuples with one float per
    cutoff; and, left on the device, per user ``users``, ``auc``, ``mpr``, ``rr``, ``recall`` [n, C], ``hit`` [n, C],
    ``n_pos``, ``n_cand``, and per pair ``pair_owner`` (the position in ``users``), ``pair_users``, ``pair_items`` and
    ``pairs`` (a ``PairRanks``)."""

    def __init__(self, ks, mean, users, per_user, pair_owner, pair_users, pair_items, pairs):
        self.ks, self.mean, self.users = tuple(ks), mean, users
        self.auc, self.mpr, self.rr = per_user["auc"], per_user["mpr"], per_user["rr"]
        self.recall, self.hit, self.n_pos, self.n_cand = per_user["recall"], per_user["hit"], per_user["n_pos"], per_user["n_cand"]
        self.pair_owner, self.pair_users, self.pair_items, self.pairs = pair_owner, pair_users, pair_items, pairs

    def __repr__(self) -> str:
        return f"FullRankResult(ks={self.ks}, mean={self.mean})"


def _pairs_of(positives: PositiveLists, users: Tensor):
    """(pair_owner, pair_users, pair_items, length): one pair per DISTINCT item of each listed user's list, by user position
    and then by item; ``length`` is the list length with duplicates.  Built from the sort ``PositiveLists.distinct`` keeps.
    The number of pairs is one size read from the device.  The last result is kept on the lists TOGETHER WITH its ``users``
    tensor: while the entry holds that tensor its memory cannot be handed out again, so the same address, length and
    device mean the same memory, and an unchanged version counter (views share it) means nothing wrote to it in place.  A
    caller that passes the same id tensor again pays no size read; a fresh tensor pays it again."""
    kept = positives.__dict__.get("_full_rank_pairs")
    if kept is not None:
        ids, version, pairs = kept
        if (ids.data_ptr() == users.data_ptr() and ids.shape == users.shape and ids.stride() == users.stride()
                and ids.dtype == users.dtype and ids.device == users.device and ids._version == version
                and users._version == version):
            return pairs
    n_lists = positives.ptr.numel() - 1
    _, entry_items = positives.distinct_entries()
    safe = users.clamp(0, max(n_lists - 1, 0))
    inside = (users >= 0) & (users < n_lists)
    counts = torch.where(inside, positives.distinct[safe], 0)
    first = torch.cumsum(positives.distinct, 0) - positives.distinct                      # a user's first distinct entry
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item()) if users.numel() else 0                                  # the size read
    owner = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), counts, output_size=total)
    within = torch.arange(total, device=users.device) - (ends - counts)[owner]
    pair_items = entry_items[first[safe][owner] + within] if total else entry_items[:0]
    length = torch.where(inside, positives.ptr[safe + 1] - positives.ptr[safe], 0)
    pairs = (owner.contiguous(), users[owner].contiguous(), pair_items.contiguous(), length)
    positives._full_rank_pairs = (users, users._version, pairs)
    return pairs


def evaluate_full_rank(users_table: Tensor, items: Tensor, seen: Optional[SeenLists], users: Tensor, positives: PositiveLists,
                       ks=(20,), seen_mode: str = "zero") -> FullRankResult:
    """AUC, mean percentile rank, MRR and recall / hit rate at every K of ``ks`` (any 1 <= K <= n_items, at most
    ``MAX_KS`` of them) for ``users`` against their ``positives``, from the exact rank of every distinct held-out item:
    ``positive_ranks``, integer reductions per user (``pair_metrics``) and ``column_sums`` for the means.  In mode "zero"
    ``recall`` and ``hit_rate`` at K <= 256 have the bits of ``evaluate_ranking``'s.  A user outside the table or the
    lists raises IndexError.  One host sync at the end, plus the read of the number of pairs (``_pairs_of``: paid on every
    call unless the same ``users`` tensor comes again) and the ascending check on a ``SeenLists``' first use."""
    cuts = [int(k) for k in ks]
    if not 1 <= len(cuts) <= MAX_KS or any(isinstance(k, bool) for k in ks):
        raise ValueError(f"1..{MAX_KS} cutoffs, got {len(cuts)}")
    _check_tables(users_table, items)
    n_items = items.size(0)
    if any(not 1 <= k <= n_items for k in cuts):
        raise ValueError(f"every cutoff must lie in [1, {n_items}], got {cuts}")
    _check_ids(users, users_table, "users")
    _check_ids(positives.ptr, users_table, "positives.ptr")
    _check_ids(positives.items, users_table, "positives.items")
    n, dev = users.numel(), users.device
    owner, pair_users, pair_items, length = _pairs_of(positives, users)
    pairs = positive_ranks(users_table, items, pair_users, pair_items, seen, seen_mode)
    per_user = pair_metrics(pairs.rank, pairs.n_cand, owner, length, cuts)
    nan = float("nan")
    if n == 0:
        mean = {"auc": nan, "mpr": nan, "mrr": nan, "recall": tuple(nan for _ in cuts), "hit_rate": tuple(nan for _ in cuts)}
        return FullRankResult(cuts, mean, users, per_user, owner, pair_users, pair_items, pairs)
    has_auc, has_mpr = ~per_user["auc"].isnan(), ~per_user["mpr"].isnan()
    table = torch.cat([torch.stack([per_user["auc"].nan_to_num(0.0), has_auc.to(torch.float64), per_user["mpr"].nan_to_num(0.0),
                                    has_mpr.to(torch.float64), per_user["rr"]], dim=1), per_user["recall"], per_user["hit"]], dim=1)
    bad_user = ((users < 0) | (users >= min(users_table.size(0), positives.ptr.numel() - 1))).any().to(torch.int64).reshape(1)
    host = torch.cat([column_sums(table.contiguous()).view(torch.int64), _status(dev)[:1].to(torch.int64), bad_user]).cpu()   # the one sync
    width = table.size(1)
    if int(host[width]) & _native.ST_INDEX_OOB or int(host[width + 1]):
        try:
            check_index_status(dev)                                      # clears the word and its host snapshot
        except IndexError:
            pass
        raise IndexError("evaluation: a user id lies outside the user table or the positive lists, or an item outside the catalogue")
    total = host[:width].view(torch.float64).tolist()
    c = len(cuts)
    mean = {"auc": total[0] / total[1] if total[1] else nan, "mpr": total[2] / total[3] if total[3] else nan, "mrr": total[4] / n,
            "recall": tuple(total[5 + i] / n for i in range(c)), "hit_rate": tuple(total[5 + c + i] / n for i in range(c))}
    return FullRankResult(cuts, mean, users, per_user, owner, pair_users, pair_items, pairs)
