"""Cross-table retrieval: per query row of one table the k best rows of another, filtered.

Three questions are one computation -- "recommend, but never what is out of stock and never what this user already bought"
(user rows against the item table), "which users should hear about this product?" (item rows against the user table, the
item's buyers left out) and "which users are like this one?" (the user table on both sides).  ``lgc_retrieve_topk`` scores
the asked-about rows against the whole candidate table on the fp32 matrix cores and selects the k best per row in the same
launch; a global eligibility mask, an ascending exclusion list per query and one skipped id per query
apply.  An excluded candidate is REMOVED: it never competes, unlike ``recommend_topk``'s seen items, which keep upstream's
``score * (1 - seen)``.  The scores have the bits of ``score_rows`` and the order is ``mask_topk``'s.

CPU tensors take a torch restatement (``mm``, a mask, a stable sort by the total order): the definition the host tests
check, not a serving path.  What this does NOT do: k above 64, per-query tag masks, upstream's ZERO rule, several devices.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _native
from .propagate import _snapshot_status, _status

__all__ = ["retrieve_topk", "BuyerLists", "request_lists"]


def _check_table(t: Tensor, name: str) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1) \
            or t.stride(0) < t.size(1):
        raise TypeError(f"{name} must be a 2-D fp32 table with unit inner stride")


def _check_vec(t: Optional[Tensor], dtype, n: int, dev, name: str) -> None:
    if t is None:
        return
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != dev or t.numel() != n:
        raise TypeError(f"{name} must be a contiguous 1-D {str(dtype).replace('torch.', '')} tensor of {n} entries on the "
                        "tables' device")


def _order_keys(v: Tensor) -> Tensor:
    """int64 keys of fp32 values, ascending with ``mask_topk``'s total order (order_key of csrc/lgconv_common.h)."""
    w = v + 0.0                                              # -0 -> +0
    u = w.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return torch.where(torch.isnan(w), torch.full_like(key, 0xFFFFFFFF), key)


def _key_values(key: Tensor) -> Tensor:
    """The fp32 value a key stands for (key_value): every NaN is 0x7FFFFFFF."""
    u = torch.where(key >= 0x80000000, key & 0x7FFFFFFF, ~key & 0xFFFFFFFF)
    u = torch.where(u >= 0x80000000, u - (1 << 32), u)
    return u.to(torch.int32).view(torch.float32)


def _retrieve_host(queries, cands, k, query_ids, query_scale, cand_scale, cand_ok, lists, n_lists, list_rows, skip_id):
    """The restatement in torch ops on the tables' (CPU) device; an id that the kernel would flag sets the status word."""
    n_rows, n_cand = queries.size(0), cands.size(0)
    n = n_rows if query_ids is None else query_ids.numel()
    ids = torch.arange(n, dtype=torch.int64) if query_ids is None else query_ids
    void = (ids < 0) | (ids >= n_rows)
    safe = ids.clamp(0, max(n_rows - 1, 0))
    panel = queries[safe] @ cands.t() if n_rows else torch.zeros((n, n_cand))
    if query_scale is not None:
        panel = (panel * query_scale[safe][:, None]) * cand_scale[None, :]
    eligible = torch.ones((n, n_cand), dtype=torch.bool)
    if cand_ok is not None:
        eligible &= (cand_ok != 0)[None, :]
    if skip_id is not None:
        hit = (skip_id >= 0) & (skip_id < n_cand)
        eligible[torch.nonzero(hit)[:, 0], skip_id[hit]] = False
    if lists is not None:
        ptr, items = lists
        which = safe if list_rows is None else list_rows
        found = (which >= 0) & (which < n_lists)
        void |= ~found & (which != -1)
        w = which.clamp(0, max(n_lists - 1, 0))
        counts = torch.where(found & ~void, ptr[w + 1] - ptr[w], torch.zeros_like(w)) if n_lists else torch.zeros_like(w)
        rows = torch.repeat_interleave(torch.arange(n), counts)
        first = torch.cumsum(counts, 0) - counts
        pos = torch.arange(int(counts.sum())) - first[rows] + ptr[w][rows] if n_lists else rows
        entry = items[pos]
        inside = (entry >= 0) & (entry < n_cand)
        eligible[rows[inside], entry[inside]] = False
    eligible[void] = False
    if bool(void.any()):
        _status(queries.device)[0] |= _native.ST_INDEX_OOB
    key = torch.where(eligible, _order_keys(panel), torch.full((n, n_cand), -1, dtype=torch.int64))
    top, index = torch.sort(key, dim=1, descending=True, stable=True)    # equal keys keep their ascending indices
    top, index = top[:, :k], index[:, :k]
    if n_cand < k:
        pad = k - n_cand
        top = torch.cat([top, torch.full((n, pad), -1, dtype=torch.int64)], dim=1)
        index = torch.cat([index, torch.full((n, pad), -1, dtype=torch.int64)], dim=1)
    none = top < 0
    value = torch.where(none, torch.full((n, k), float("-inf")), _key_values(top.clamp(min=0)))
    return torch.where(none, torch.full_like(index, -1), index), value


def retrieve_topk(queries: Tensor, cands: Tensor, k: int, query_ids: Optional[Tensor] = None,
                  query_scale: Optional[Tensor] = None, cand_scale: Optional[Tensor] = None, cand_ok: Optional[Tensor] = None,
                  lists=None, list_rows: Optional[Tensor] = None, skip_id: Optional[Tensor] = None,
                  slices: int = 0) -> Tuple[Tensor, Tensor]:
    """``(index int64 [n, k], value fp32 [n, k])``: per query the k best eligible rows of ``cands`` (fp32 ``[n_cand, dim]``)
    for the rows ``query_ids`` (int64, None = every row in order) of ``queries`` (fp32 ``[n_query_rows, dim]``), in
    ``mask_topk``'s order (NaN first, then descending, equal values by ascending index): lgc_retrieve_topk.

    ``query_scale`` / ``cand_scale``: fp32 per row of each table, both or neither; the score is ``(dot * query_scale[id]) *
    cand_scale[c]``.  ``cand_ok``: bool or uint8 ``[n_cand]``, a candidate whose entry is 0 is never returned.  ``lists``:
    the exclusion lists, a ``(ptr, items)`` pair or anything with these attributes (``SeenLists``, ``BuyerLists``) -- a CSR
    of ASCENDING candidate indices; ``list_rows`` (int64 ``[n]``) names the list of every query, -1 for none, None = the
    query's id.  ``skip_id`` (int64 ``[n]``): one more candidate the query leaves out, -1 for none.  A listed candidate is
    removed, not zeroed.  With fewer than k eligible candidates a row ends in -1 / -inf.  ``slices`` only moves work (0 =
    the library chooses); the result does not depend on it.  A query id outside the table, or a list number outside the
    lists, gives a row of -1 / -inf and raises at ``check_index_status()``."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.RETRIEVE_MAX_K:
        raise ValueError(f"k must be an integer in [1, {_native.RETRIEVE_MAX_K}]")
    if isinstance(slices, bool) or not isinstance(slices, int) or not 0 <= slices <= _native.RETRIEVE_MAX_SLICES:
        raise ValueError(f"slices must be an integer in [0, {_native.RETRIEVE_MAX_SLICES}]")
    _check_table(queries, "queries")
    _check_table(cands, "cands")
    if queries.size(1) != cands.size(1) or queries.device != cands.device:
        raise TypeError("queries and cands must have the same width and live on the same device")
    if cands.size(0) < 1:
        raise ValueError("no candidates to score")
    dev, n_rows, n_cand = queries.device, queries.size(0), cands.size(0)
    n = n_rows if query_ids is None else (query_ids.numel() if torch.is_tensor(query_ids) else -1)
    _check_vec(query_ids, torch.int64, n, dev, "query_ids")
    if (query_scale is None) != (cand_scale is None):
        raise ValueError("query_scale and cand_scale are given together or not at all")
    _check_vec(query_scale, torch.float32, n_rows, dev, "query_scale")
    _check_vec(cand_scale, torch.float32, n_cand, dev, "cand_scale")
    if cand_ok is not None and torch.is_tensor(cand_ok) and cand_ok.dtype == torch.bool:
        cand_ok = cand_ok.to(torch.uint8)
    _check_vec(cand_ok, torch.uint8, n_cand, dev, "cand_ok")
    n_lists = 0
    if lists is not None:
        ptr, items = lists if isinstance(lists, (tuple, list)) else (lists.ptr, lists.items)
        for t, name in ((ptr, "lists.ptr"), (items, "lists.items")):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
                raise TypeError(f"{name} must be a contiguous 1-D int64 tensor on the tables' device")
        if ptr.numel() < 1:
            raise ValueError("lists.ptr must hold at least one entry")
        lists, n_lists = (ptr, items), ptr.numel() - 1
        _check_vec(list_rows, torch.int64, n, dev, "list_rows")
    else:
        list_rows = None
    _check_vec(skip_id, torch.int64, n, dev, "skip_id")
    if not queries.is_cuda:
        return _retrieve_host(queries, cands, k, query_ids, query_scale, cand_scale, cand_ok, lists, n_lists, list_rows, skip_id)
    index = torch.empty((n, k), dtype=torch.int64, device=dev)
    value = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return index, value
    lib = _native.load()
    if lists is not None and lists[1].numel() == 0:          # an empty tensor has no address; the kernel reads no entry of it
        lists = (lists[0], torch.zeros(1, dtype=torch.int64, device=dev))
    ws_bytes = lib.lgc_retrieve_workspace_bytes(n, n_cand, k, slices)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        code = lib.lgc_retrieve_topk(_native.ptr(queries), queries.stride(0), n_rows, _native.ptr(cands), cands.stride(0), n_cand,
                                     queries.size(1), _native.ptr(query_ids), n, _native.ptr(query_scale),
                                     _native.ptr(cand_scale), _native.ptr(cand_ok),
                                     _native.ptr(lists[0]) if lists else None, _native.ptr(lists[1]) if lists else None,
                                     _native.ptr(list_rows), n_lists, _native.ptr(skip_id), k, slices, _native.ptr(index),
                                     _native.ptr(value), _native.ptr(ws), ws_bytes, _native.ptr(_status(dev)),
                                     _native.stream_of(dev))
    _native.check(code, "lgc_retrieve_topk")
    _snapshot_status(dev)
    return index, value


def _csr_of_pairs(row: Tensor, col: Tensor, n_rows: int, n_cols: int):
    """(ptr int64 [n_rows + 1], cols int64): the distinct (row, col) pairs as a CSR, columns ascending within a row."""
    key = torch.unique(row * n_cols + col)                   # sorted
    r = torch.div(key, n_cols, rounding_mode="floor")
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=key.device)
    torch.cumsum(torch.bincount(r, minlength=n_rows), 0, out=ptr[1:])
    return ptr, (key - r * n_cols).contiguous()


class BuyerLists:
    """The transpose of ``SeenLists``: per item the ascending distinct users connected to it, a device CSR (``ptr`` int64
    ``[n_items + 1]``, ``items`` int64 user indices -- the entries are called ``items`` as in every list ``retrieve_topk``
    takes; ``users`` is the same tensor)."""

    def __init__(self, ptr: Tensor, users: Tensor):
        self.ptr, self.items = ptr, users

    @property
    def users(self) -> Tensor:
        return self.items

    @classmethod
    def from_pairs(cls, users: Tensor, items: Tensor, n_users: int, n_items: int, device=None) -> "BuyerLists":
        """From (user index, item index) pairs, items WITHOUT the ``n_users`` offset; repeats are one entry."""
        users, items = users.reshape(-1).to(torch.int64), items.reshape(-1).to(torch.int64)
        if users.numel() != items.numel():
            raise ValueError(f"{users.numel()} users for {items.numel()} items")
        if users.numel() and (int(users.min()) < 0 or int(users.max()) >= n_users or int(items.min()) < 0
                              or int(items.max()) >= n_items):
            raise ValueError(f"pairs outside [0, {n_users}) x [0, {n_items})")
        if device is not None:
            users, items = users.to(device), items.to(device)
        return cls(*_csr_of_pairs(items, users, int(n_items), max(int(n_users), 1)))

    @classmethod
    def from_edges(cls, edge_index: Tensor, n_users: int, n_items: int, device=None) -> "BuyerLists":
        """From the training graph's ``edge_index`` (int64 ``[2, E]`` node ids, users first, items offset by ``n_users``):
        an edge counts in either direction, both directions and repeats are one entry; an edge between two users or two
        items, or a node outside the graph, is refused."""
        n_users, n_items = int(n_users), int(n_items)
        if not torch.is_tensor(edge_index) or edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise TypeError("edge_index must be an int64 [2, E] tensor")
        if device is not None:
            edge_index = edge_index.to(device)
        src, dst = edge_index[0], edge_index[1]
        lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
        if lo.numel() and (int(lo.min()) < 0 or int(lo.max()) >= n_users or int(hi.min()) < n_users
                           or int(hi.max()) >= n_users + n_items):
            raise ValueError(f"every edge must join a user in [0, {n_users}) and an item in [{n_users}, {n_users + n_items})")
        return cls.from_pairs(lo, hi - n_users, n_users, n_items)

    @classmethod
    def from_seen(cls, seen, n_users: int, n_items: int) -> "BuyerLists":
        """The transpose of a ``SeenLists`` over all ``n_users`` users."""
        counts = seen.ptr[1:] - seen.ptr[:-1]
        users = torch.repeat_interleave(torch.arange(int(n_users), dtype=torch.int64, device=seen.ptr.device), counts)
        return cls.from_pairs(users, seen.items, n_users, n_items)


def request_lists(seen, rows: Optional[Tensor], n: int, exclude: Optional[Sequence], n_cand: int, device):
    """``(ptr int64 [n + 1], items int64)`` on ``device``: per request row the ascending distinct union of list
    ``rows[r]`` of ``seen`` (anything with ``ptr`` / ``items``, or None; ``rows`` None = list r; a number outside the lists
    contributes nothing) and of ``exclude[r]`` (a sequence of candidate indices or None, per row).  Entries outside
    ``[0, n_cand)`` are dropped: the kernel would ignore them.  One host sync where ``seen`` is given."""
    device = torch.device(device)
    row_parts, col_parts = [], []
    if seen is not None:
        ptr, items = seen.ptr.to(device), seen.items.to(device)
        n_lists = ptr.numel() - 1
        which = torch.arange(n, dtype=torch.int64, device=device) if rows is None else rows.to(device)
        found = (which >= 0) & (which < n_lists)
        w = which.clamp(0, max(n_lists - 1, 0))
        counts = torch.where(found, ptr[w + 1] - ptr[w], torch.zeros_like(w)) if n_lists else torch.zeros_like(w)
        r = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=device), counts)
        first = torch.cumsum(counts, 0) - counts
        pos = torch.arange(r.numel(), dtype=torch.int64, device=device) - first[r] + ptr[w][r]
        row_parts.append(r)
        col_parts.append(items[pos])
    if exclude is not None:
        if len(exclude) != n:
            raise ValueError(f"exclude has {len(exclude)} rows for {n} requests")
        er, ec = [], []
        for r, extra in enumerate(exclude):
            for i in (extra or ()):
                if isinstance(i, bool) or not isinstance(i, int):
                    raise ValueError(f"exclude[{r}] must hold item indices")
                er.append(r)
                ec.append(i)
        row_parts.append(torch.tensor(er, dtype=torch.int64, device=device))
        col_parts.append(torch.tensor(ec, dtype=torch.int64, device=device))
    if not row_parts:
        return torch.zeros(n + 1, dtype=torch.int64, device=device), torch.zeros(0, dtype=torch.int64, device=device)
    row, col = torch.cat(row_parts), torch.cat(col_parts)
    inside = (col >= 0) & (col < n_cand)
    return _csr_of_pairs(row[inside], col[inside], n, int(n_cand))
