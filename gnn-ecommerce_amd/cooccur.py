"""Bought together: per item the k items that share most buyers with it.

"Customers who bought this also bought" is answered from the purchase lists alone -- no embedding, no training, valid on
day one -- and it is the item-kNN baseline a LightGCN result is compared against.  ``lgc_cooccur_topk`` (DESIGN.md section
29) takes the two CSRs the library already keeps on the device, item -> buyers (``BuyerLists``) and user -> items
(``SeenLists``), counts per query item how many buyers it shares with every other item in LDS, scores the counts (the raw
count, cosine ``c / sqrt(a b)`` or Jaccard ``c / (a + b - c)``, a and b the two items' buyer counts) and selects the k best
in the same launch.  Counts are integers and a score is a few correctly rounded fp32 operations on them, so every output
has one right answer, bit for bit; the order is ``mask_topk``'s, equal scores by ascending index.

CPU tensors take a torch restatement (a dense integer count panel for the asked rows, the three formulas in float32, a
stable sort by the total order's keys): the definition the host tests hold to the numpy reference, not a serving path.
What this does NOT do: weighted events, k above 64, several devices.  Basket queries (a sum of similarities over several
items, the item-kNN recommender) are ``itemknn.py``, which takes this module's result as its neighbour table.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native
from .propagate import SeenLists, _snapshot_status, _status
from .retrieve import BuyerLists, _csr_of_pairs, _key_values, _order_keys

__all__ = ["cooccur_topk", "CoPurchase", "MEASURES"]

MEASURES = {"count": 0, "cosine": 1, "jaccard": 2}           # LGC_COOCCUR_COUNT, _COSINE, _JACCARD


def _lists_of(lists, n_rows: int, name: str):
    ptr, items = lists if isinstance(lists, (tuple, list)) else (lists.ptr, lists.items)
    for t, what in ((ptr, "ptr"), (items, "items")):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise TypeError(f"{name}.{what} must be a contiguous 1-D int64 tensor")
    if ptr.numel() != n_rows + 1 or ptr.device != items.device:
        raise TypeError(f"{name}.ptr must hold {n_rows + 1} entries on the device of {name}.items")
    return ptr, items


def _entries(ptr: Tensor, items: Tensor, rows: Tensor):
    """(position in ``rows``, entry) of every entry of the lists ``rows`` names, in order."""
    counts = ptr[rows + 1] - ptr[rows]
    which = torch.repeat_interleave(torch.arange(rows.numel()), counts)
    first = torch.cumsum(counts, 0) - counts
    pos = torch.arange(int(counts.sum())) - first[which] + ptr[rows][which]
    return which, items[pos]


def _cooccur_host(bptr, busers, sptr, sitems, n_users, n_items, k, ids, measure, min_count, item_ok):
    """The restatement in torch ops on CPU tensors; an entry or id that the kernel would flag sets the status word."""
    n = n_items if ids is None else ids.numel()
    ids = torch.arange(n, dtype=torch.int64) if ids is None else ids
    void = (ids < 0) | (ids >= n_items)
    safe = ids.clamp(0, n_items - 1)
    length = bptr[1:] - bptr[:-1]
    a = torch.where(void, torch.zeros_like(safe), length[safe])
    row, user = _entries(bptr, busers, safe[~void])
    row = torch.nonzero(~void)[:, 0][row]
    bad_user = (user < 0) | (user >= n_users)
    row, user = row[~bad_user], user[~bad_user]
    which, item = _entries(sptr, sitems, user)
    row = row[which]
    bad_item = (item < 0) | (item >= n_items)
    c = torch.zeros((n, n_items), dtype=torch.int64)
    c.index_put_((row[~bad_item], item[~bad_item]), torch.ones(1, dtype=torch.int64), accumulate=True)
    if bool(void.any()) or bool(bad_user.any()) or bool(bad_item.any()):
        _status(bptr.device)[0] |= _native.ST_INDEX_OOB
    eligible = (c >= min_count) & (torch.arange(n_items)[None, :] != ids[:, None]) & ~void[:, None]
    if item_ok is not None:
        eligible &= (item_ok != 0)[None, :]
    s = c.to(torch.float32)
    if measure == "cosine":
        ra = 1.0 / torch.sqrt(a.to(torch.float32))
        rb = 1.0 / torch.sqrt(length.to(torch.float32))
        s = (s * ra[:, None]) * rb[None, :]
    elif measure == "jaccard":
        den = a[:, None] + length[None, :] - c
        eligible &= den > 0
        s = s / den.clamp(min=1).to(torch.float32)
    key = torch.where(eligible, _order_keys(s), torch.full((n, n_items), -1, dtype=torch.int64))
    top, index = torch.sort(key, dim=1, descending=True, stable=True)    # equal keys keep their ascending indices
    top, index = top[:, :k], index[:, :k]
    if n_items < k:
        pad = k - n_items
        top = torch.cat([top, torch.full((n, pad), -1, dtype=torch.int64)], dim=1)
        index = torch.cat([index, torch.zeros((n, pad), dtype=torch.int64)], dim=1)
    none = top < 0
    value = torch.where(none, torch.full((n, k), float("-inf")), _key_values(top.clamp(min=0)))
    count = torch.where(none, torch.zeros_like(index), torch.gather(c, 1, index)).to(torch.int32)
    return torch.where(none, torch.full_like(index, -1), index), value, count


def cooccur_topk(buyers, seen, n_users: int, n_items: int, k: int, item_ids: Optional[Tensor] = None, measure: str = "cosine",
                 min_count: int = 1, item_ok: Optional[Tensor] = None, band: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """``(index int64 [n, k], value fp32 [n, k], count int32 [n, k])``: per item of ``item_ids`` (int64, None = the whole
    catalogue in order) the k items bought together with it most, best first: lgc_cooccur_topk.

    ``buyers`` and ``seen``: the two purchase CSRs, anything with ``ptr`` / ``items`` or a ``(ptr, items)`` pair --
    ``BuyerLists`` (item -> ascending distinct users) and ``SeenLists`` (user -> ascending distinct items).  ``c(q, j)``
    counts the buyers q and j share; j is a candidate for q iff ``j != q``, ``c >= min_count`` (at least 1) and ``item_ok``
    (bool or uint8 ``[n_items]``) is None or non-zero at j.  ``measure``: "count" (``c``), "cosine" (``c / sqrt(a b)``) or
    "jaccard" (``c / (a + b - c)``), a and b the lengths of the two buyer lists, in fp32 as the header states them.  The
    order is ``mask_topk``'s, equal scores by ascending index; ``count`` is the raw c of each returned item.  With fewer
    than k candidates a row ends in -1 / -inf / 0.  ``band`` only moves work (0 = the library chooses); the result does
    not depend on it.  An id outside the catalogue gives an empty row, an entry outside its table is skipped, and either
    raises at ``check_index_status()``."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.COOCCUR_MAX_K:
        raise ValueError(f"k must be an integer in [1, {_native.COOCCUR_MAX_K}]")
    if not isinstance(measure, str) or measure not in MEASURES:
        raise ValueError(f"measure must be one of {list(MEASURES)}, got {measure!r}")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or not 1 <= min_count < 2 ** 31:
        raise ValueError("min_count must be an integer of at least 1")
    if isinstance(band, bool) or not isinstance(band, int) or not (band == 0 or (64 <= band <= _native.COOCCUR_MAX_BAND
                                                                                  and band % 64 == 0)):
        raise ValueError(f"band must be 0 or a multiple of 64 in [64, {_native.COOCCUR_MAX_BAND}]")
    n_users, n_items = int(n_users), int(n_items)
    if n_users < 0 or n_items < 1:
        raise ValueError(f"n_users {n_users} and n_items {n_items} do not name a catalogue")
    bptr, busers = _lists_of(buyers, n_items, "buyers")
    sptr, sitems = _lists_of(seen, n_users, "seen")
    dev = bptr.device
    if sptr.device != dev:
        raise TypeError("buyers and seen must live on the same device")
    n = n_items
    if item_ids is not None:
        if not torch.is_tensor(item_ids) or item_ids.dtype != torch.int64 or item_ids.dim() != 1 \
                or not item_ids.is_contiguous() or item_ids.device != dev:
            raise TypeError("item_ids must be a contiguous 1-D int64 tensor on the lists' device")
        n = item_ids.numel()
    if item_ok is not None:
        if torch.is_tensor(item_ok) and item_ok.dtype == torch.bool:
            item_ok = item_ok.to(torch.uint8)
        if not torch.is_tensor(item_ok) or item_ok.dtype != torch.uint8 or item_ok.dim() != 1 or item_ok.numel() != n_items \
                or not item_ok.is_contiguous() or item_ok.device != dev:
            raise TypeError(f"item_ok must be a contiguous bool or uint8 tensor of {n_items} entries on the lists' device")
    if not bptr.is_cuda:
        return _cooccur_host(bptr, busers, sptr, sitems, n_users, n_items, k, item_ids, measure, min_count, item_ok)
    index = torch.empty((n, k), dtype=torch.int64, device=dev)
    value = torch.empty((n, k), dtype=torch.float32, device=dev)
    count = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return index, value, count
    lib = _native.load()
    one = torch.zeros(1, dtype=torch.int64, device=dev)      # an empty tensor has no address; the kernel reads no entry of it
    busers = busers if busers.numel() else one
    sitems = sitems if sitems.numel() else one
    ws_bytes = lib.lgc_cooccur_workspace_bytes(n, n_items, k, band, _native.stream_of(dev))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        code = lib.lgc_cooccur_topk(_native.ptr(bptr), _native.ptr(busers), n_items, _native.ptr(sptr), _native.ptr(sitems),
                                    n_users, _native.ptr(item_ids), n, _native.ptr(item_ok), min_count, MEASURES[measure], k,
                                    band, _native.ptr(index), _native.ptr(value), _native.ptr(count), _native.ptr(ws),
                                    ws_bytes, _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_cooccur_topk")
    _snapshot_status(dev)
    return index, value, count


class CoPurchase:
    """The purchase lists in both directions, built once and asked many times: ``seen`` (a ``SeenLists``, user -> items)
    and ``buyers`` (its ``BuyerLists``, item -> users) of ``n_users`` users and ``n_items`` items."""

    def __init__(self, seen: SeenLists, buyers: BuyerLists, n_users: int, n_items: int):
        self.seen, self.buyers, self.n_users, self.n_items = seen, buyers, int(n_users), int(n_items)

    @classmethod
    def from_seen(cls, seen, n_users: int, n_items: int) -> "CoPurchase":
        """From the purchase lists; their transpose is built here."""
        if not isinstance(seen, SeenLists):
            raise TypeError("seen must be a SeenLists")
        return cls(seen, BuyerLists.from_seen(seen, n_users, n_items), n_users, n_items)

    @classmethod
    def from_edges(cls, edge_index: Tensor, n_users: int, n_items: int, device=None) -> "CoPurchase":
        """From the training graph's ``edge_index`` (int64 ``[2, E]`` node ids, users first, items offset by ``n_users``):
        every edge is a purchase, both directions and repeats are one; what ``BuyerLists.from_edges`` refuses is refused."""
        n_users, n_items = int(n_users), int(n_items)
        buyers = BuyerLists.from_edges(edge_index, n_users, n_items, device)
        counts = buyers.ptr[1:] - buyers.ptr[:-1]
        items = torch.repeat_interleave(torch.arange(n_items, dtype=torch.int64, device=buyers.ptr.device), counts)
        return cls(SeenLists(*_csr_of_pairs(buyers.users, items, max(n_users, 0), n_items)), buyers, n_users, n_items)

    def neighbors(self, item_ids, k: int = 10, measure: str = "cosine", min_count: int = 1, item_ok=None, band: int = 0):
        """``cooccur_topk`` over these lists: ``item_ids`` a sequence or int64 tensor of item indices, None = the whole
        catalogue; ``item_ok`` bool or uint8 ``[n_items]``.  Ids and mask are moved to the lists' device."""
        dev = self.buyers.ptr.device
        if item_ids is not None:
            item_ids = item_ids if torch.is_tensor(item_ids) else torch.as_tensor(list(item_ids), dtype=torch.int64)
            if item_ids.dtype != torch.int64:
                raise TypeError("item_ids must be int64 indices")
            item_ids = item_ids.reshape(-1).to(dev).contiguous()
        if item_ok is not None:
            item_ok = torch.as_tensor(item_ok).to(dev).contiguous()
        return cooccur_topk(self.buyers, self.seen, self.n_users, self.n_items, k, item_ids, measure, min_count, item_ok, band)
