"""The item-kNN recommender: rank items for a basket by the sum of their neighbour similarities to the basket's items.

``cooccur_topk`` (and ``similar_items``) return a ``[n_items, kn]`` neighbour table.  This module turns such a table into
ranked lists for users, carts and sessions -- the truncated-neighbourhood item-kNN people expect as the baseline of an
implicit-feedback model -- and evaluates them with the library's own metrics.  ``lgc_knn_recommend`` (DESIGN.md section
30) accumulates, per basket, the neighbour rows of the basket's items into candidate scores in LDS, in the basket's order
and without a float atomic, removes what must not be returned and selects the k best in the same launch: every output has
one right answer, bit for bit; the order is ``mask_topk``'s, equal scores by ascending index.

CPU tensors take a torch restatement (one step per basket position, a gather and a plain indexed store of ``acc + term``,
a stable sort by the total order's keys): the definition the host tests hold to the numpy reference, not a serving path.
What this does NOT do: exclusion lists beyond the basket, ``kn`` or ``k`` above 64, several devices, blending two tables.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native
from .cooccur import CoPurchase
from .foldin import SessionLists
from .propagate import PositiveLists, RankingResult, SeenLists, _snapshot_status, _status, ranking_result
from .retrieve import _key_values, _order_keys

__all__ = ["knn_recommend", "ItemKNN"]


def _baskets_of(baskets):
    """(ptr, items, weights or None) of anything with ``ptr`` / ``items`` / optional ``weights``, or of a tuple."""
    if isinstance(baskets, (tuple, list)):
        if len(baskets) not in (2, 3):
            raise TypeError("baskets must be (ptr, items) or (ptr, items, weights)")
        ptr, items, weights = tuple(baskets) + (None,) * (3 - len(baskets))
    else:
        ptr, items, weights = baskets.ptr, baskets.items, getattr(baskets, "weights", None)
    for t, what in ((ptr, "ptr"), (items, "items")):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise TypeError(f"baskets.{what} must be a contiguous 1-D int64 tensor")
    if ptr.numel() < 1 or ptr.device != items.device:
        raise TypeError("baskets.ptr must hold at least one entry on the device of baskets.items")
    if weights is not None and (not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.dim() != 1
                                or not weights.is_contiguous() or weights.numel() != items.numel() or weights.device != ptr.device):
        raise TypeError(f"baskets.weights must be a contiguous fp32 tensor of {items.numel()} entries on the lists' device")
    return ptr, items, weights


def _knn_host(nbr_index, nbr_value, n_items, ptr, items, weights, rows, k, exclude_basket, min_votes, item_ok):
    """The restatement in torch ops on CPU tensors; an entry or id that the kernel would flag sets the status word."""
    n_lists = ptr.numel() - 1
    lists = torch.arange(n_lists, dtype=torch.int64) if rows is None else rows
    n = lists.numel()
    void = (lists < 0) | (lists >= n_lists)
    safe = lists.clamp(0, max(n_lists - 1, 0))
    if n_lists:
        start = torch.where(void, torch.zeros_like(safe), ptr[safe])
        length = torch.where(void, torch.zeros_like(safe), ptr[safe + 1] - ptr[safe])
    else:
        start = length = torch.zeros_like(safe)
    row = torch.arange(n, dtype=torch.int64)
    acc = torch.zeros((n, n_items + 1), dtype=torch.float32)                 # column n_items takes what is skipped
    votes = torch.zeros((n, n_items + 1), dtype=torch.int64)
    listed = torch.zeros((n, n_items + 1), dtype=torch.bool)
    bad = bool(void.any())
    for t in range(int(length.max()) if n else 0):                           # the basket's order: entry t of every row
        live = length > t
        at = torch.where(live, start + t, torch.zeros_like(start))
        i = items[at]
        inside = live & (i >= 0) & (i < n_items)
        bad |= bool((live & ~inside).any())
        i = torch.where(inside, i, torch.zeros_like(i))
        j, term = nbr_index[i], nbr_value[i]                                 # [n, kn]: the t-th entry's neighbour row
        if weights is not None:
            term = weights[at][:, None] * term                               # rounded on its own
        there = inside[:, None] & (j != -1)
        valid = there & (j >= 0) & (j < n_items)
        bad |= bool((there & ~valid).any())
        col = torch.where(valid, j, torch.full_like(j, n_items))
        at_row = row[:, None].expand_as(col)
        acc[at_row, col] = acc[at_row, col] + term                           # the indices of a row are distinct: a plain store
        votes[at_row, col] = votes[at_row, col] + 1
        listed[row, torch.where(inside, i, torch.full_like(i, n_items))] = True
    if bad:
        _status(ptr.device)[0] |= _native.ST_INDEX_OOB
    acc, votes, listed = acc[:, :n_items], votes[:, :n_items], listed[:, :n_items]
    eligible = votes >= min_votes
    if item_ok is not None:
        eligible &= (item_ok != 0)[None, :]
    if exclude_basket:
        eligible &= ~listed
    key = torch.where(eligible, _order_keys(acc), torch.full((n, n_items), -1, dtype=torch.int64))
    top, index = torch.sort(key, dim=1, descending=True, stable=True)        # equal keys keep their ascending indices
    top, index = top[:, :k], index[:, :k]
    if n_items < k:
        pad = k - n_items
        top = torch.cat([top, torch.full((n, pad), -1, dtype=torch.int64)], dim=1)
        index = torch.cat([index, torch.zeros((n, pad), dtype=torch.int64)], dim=1)
    none = top < 0
    value = torch.where(none, torch.full((n, k), float("-inf")), _key_values(top.clamp(min=0)))
    count = torch.where(none, torch.zeros_like(index), torch.gather(votes, 1, index)).to(torch.int32)
    return torch.where(none, torch.full_like(index, -1), index), value, count


def knn_recommend(nbr_index: Tensor, nbr_value: Tensor, n_items: int, baskets, k: int, rows: Optional[Tensor] = None,
                  exclude_basket: bool = True, min_votes: int = 1, item_ok: Optional[Tensor] = None,
                  band: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """``(index int64 [n, k], value fp32 [n, k], votes int32 [n, k])``: per basket the k items with the best sum of
    neighbour similarities, best first: lgc_knn_recommend.

    ``nbr_index`` / ``nbr_value``: an int64 and an fp32 ``[n_items, kn]`` neighbour table (``cooccur_topk`` over the whole
    catalogue, ``similar_items``), ``kn <= 64``, -1 an empty place.  ``baskets``: a CSR of item indices, anything with
    ``ptr`` / ``items`` / optional fp32 ``weights`` (``SessionLists``, ``SeenLists``) or a tuple of them; entries in any
    order, repeats allowed.  ``rows`` (int64, None = basket r for query r) names the basket of each query.  The score of
    item j is the sum, in the basket's order, of ``weight * similarity`` over the basket entries whose neighbour row holds
    j, each product and each add rounded on its own in fp32; ``votes`` counts those entries.  j is a candidate iff it has
    at least ``min_votes`` (at least 1) votes, ``item_ok`` (bool or uint8 ``[n_items]``) is None or non-zero at j and, with
    ``exclude_basket``, j is no entry of the basket.  The order is ``mask_topk``'s, equal scores by ascending index.  With
    fewer than k candidates a row ends in -1 / -inf / 0.  ``band`` only moves work (0 = the library chooses); the result
    does not depend on it.  A basket number outside the CSR gives an empty row, an entry or neighbour outside the catalogue
    is skipped, and either raises at ``check_index_status()``."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.KNN_MAX_K:
        raise ValueError(f"k must be an integer in [1, {_native.KNN_MAX_K}]")
    if isinstance(min_votes, bool) or not isinstance(min_votes, int) or not 1 <= min_votes < 2 ** 31:
        raise ValueError("min_votes must be an integer of at least 1")
    if isinstance(band, bool) or not isinstance(band, int) or not (band == 0 or (64 <= band <= _native.KNN_MAX_BAND
                                                                                  and band % 64 == 0)):
        raise ValueError(f"band must be 0 or a multiple of 64 in [64, {_native.KNN_MAX_BAND}]")
    n_items = int(n_items)
    if n_items < 1:
        raise ValueError(f"n_items {n_items} does not name a catalogue")
    if not torch.is_tensor(nbr_index) or nbr_index.dtype != torch.int64 or nbr_index.dim() != 2 or nbr_index.size(0) != n_items \
            or not 1 <= nbr_index.size(1) <= _native.KNN_MAX_NEIGHBORS or nbr_index.stride(1) != 1:
        raise TypeError(f"nbr_index must be an int64 [{n_items}, kn] tensor with unit inner stride, kn in "
                        f"[1, {_native.KNN_MAX_NEIGHBORS}]")
    if not torch.is_tensor(nbr_value) or nbr_value.dtype != torch.float32 or nbr_value.shape != nbr_index.shape \
            or nbr_value.stride() != nbr_index.stride() or nbr_value.device != nbr_index.device:
        raise TypeError("nbr_value must be an fp32 tensor of nbr_index's shape, strides and device")
    ptr, items, weights = _baskets_of(baskets)
    dev = nbr_index.device
    if ptr.device != dev:
        raise TypeError("the baskets and the neighbour table must live on the same device")
    n_lists = ptr.numel() - 1
    n = n_lists
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous() \
                or rows.device != dev:
            raise TypeError("rows must be a contiguous 1-D int64 tensor on the table's device")
        n = rows.numel()
    if item_ok is not None:
        if torch.is_tensor(item_ok) and item_ok.dtype == torch.bool:
            item_ok = item_ok.to(torch.uint8)
        if not torch.is_tensor(item_ok) or item_ok.dtype != torch.uint8 or item_ok.dim() != 1 or item_ok.numel() != n_items \
                or not item_ok.is_contiguous() or item_ok.device != dev:
            raise TypeError(f"item_ok must be a contiguous bool or uint8 tensor of {n_items} entries on the table's device")
    if not nbr_index.is_cuda:
        return _knn_host(nbr_index, nbr_value, n_items, ptr, items, weights, rows, k, bool(exclude_basket), min_votes, item_ok)
    index = torch.empty((n, k), dtype=torch.int64, device=dev)
    value = torch.empty((n, k), dtype=torch.float32, device=dev)
    votes = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return index, value, votes
    lib = _native.load()
    if items.numel() == 0:                                   # an empty tensor has no address; the kernel reads no entry of it
        items = torch.zeros(1, dtype=torch.int64, device=dev)
        weights = None
    kn = nbr_index.size(1)
    ws_bytes = lib.lgc_knn_workspace_bytes(n, n_items, k, band, _native.stream_of(dev))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        code = lib.lgc_knn_recommend(_native.ptr(nbr_index), _native.ptr(nbr_value), nbr_index.stride(0) if n_items > 1 else kn,
                                     n_items, kn, _native.ptr(ptr), _native.ptr(items), _native.ptr(weights), n_lists,
                                     _native.ptr(rows), n, _native.ptr(item_ok), 1 if exclude_basket else 0, min_votes, k, band,
                                     _native.ptr(index), _native.ptr(value), _native.ptr(votes), _native.ptr(ws), ws_bytes,
                                     _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_knn_recommend")
    _snapshot_status(dev)
    return index, value, votes


class ItemKNN:
    """A neighbour table (``index`` int64 / ``value`` fp32 ``[n_items, kn]``) and, optionally, the purchase lists
    (``seen``, a ``SeenLists``) its users are addressed through: fitted or given once, asked many times."""

    def __init__(self, index: Tensor, value: Tensor, n_items: int, seen: Optional[SeenLists] = None):
        if seen is not None and not isinstance(seen, SeenLists):
            raise TypeError("seen must be a SeenLists or None")
        self.index, self.value, self.n_items, self.seen = index, value, int(n_items), seen

    @classmethod
    def fit(cls, copurchase: CoPurchase, kn: int = 64, measure: str = "cosine", min_count: int = 1, item_ok=None) -> "ItemKNN":
        """From purchase lists: ``cooccur_topk`` over the whole catalogue, ``kn`` neighbours an item; the lists stay with
        the result as its users' baskets."""
        if not isinstance(copurchase, CoPurchase):
            raise TypeError("copurchase must be a CoPurchase")
        index, value, _ = copurchase.neighbors(None, kn, measure, min_count, item_ok)
        return cls(index, value, copurchase.n_items, copurchase.seen)

    @classmethod
    def from_neighbors(cls, index: Tensor, value: Tensor, n_items: int, seen: Optional[SeenLists] = None) -> "ItemKNN":
        """From any table of the shape, for example ``LightGCN.similar_items(..., item_ids=None, k=kn)``: an embedding
        item-kNN."""
        return cls(index, value, n_items, seen)

    def _ok(self, item_ok):
        return None if item_ok is None else torch.as_tensor(item_ok).to(self.index.device).contiguous()

    def _users(self, users) -> Tensor:
        if self.seen is None:
            raise ValueError("this ItemKNN holds no purchase lists: give seen= when it is built, or ask recommend_sessions")
        users = users if torch.is_tensor(users) else torch.as_tensor(list(users), dtype=torch.int64)
        if users.dtype != torch.int64:
            raise TypeError("users must be int64 indices")
        return users.reshape(-1).to(self.index.device).contiguous()

    def recommend(self, users, k: int = 20, exclude_seen: bool = True, min_votes: int = 1, item_ok=None, band: int = 0):
        """``knn_recommend`` with the users' purchase lists as baskets: ``users`` a sequence or int64 tensor of user
        indices, addressed through the lists in place (the CSR is not copied)."""
        users = self._users(users)
        return knn_recommend(self.index, self.value, self.n_items, (self.seen.ptr, self.seen.items), k, users, exclude_seen,
                             min_votes, self._ok(item_ok), band)

    def recommend_sessions(self, sessions: SessionLists, k: int = 20, exclude_basket: bool = True, min_votes: int = 1,
                           item_ok=None, band: int = 0):
        """``knn_recommend`` with the sessions as baskets, one answer per session; the weights are the sessions'."""
        if not isinstance(sessions, SessionLists):
            raise TypeError("sessions must be a SessionLists")
        return knn_recommend(self.index, self.value, self.n_items, sessions, k, None, exclude_basket, min_votes,
                             self._ok(item_ok), band)

    def evaluate(self, users, positives: PositiveLists, ks=(5, 10, 20), coverage: bool = True) -> RankingResult:
        """What ``evaluate_ranking`` returns for a model, for this baseline: the users' purchased items removed, then
        precision, recall, NDCG, MAP, MRR, hit rate and coverage at every cutoff of ``ks`` from one ranking at ``max(ks)``
        (at most 64), by the same lgc_rank_metrics / lgc_column_sums / lgc_topk_coverage calls.  A user with fewer
        candidates than the cutoff keeps the empty places of its row: they hit nothing and cover nothing."""
        cuts = [int(c) for c in ks]
        if not cuts or cuts != sorted(set(cuts)) or cuts[0] < 1 or cuts[-1] > _native.KNN_MAX_K:
            raise ValueError(f"ks must be strictly ascending cutoffs in [1, {_native.KNN_MAX_K}]")
        users = self._users(users)
        top, _, _ = self.recommend(users, cuts[-1])
        return ranking_result(top, positives, users, cuts, self.n_items, coverage, short_rows=True)
