"""Similar items: the k nearest rows of the item table, by cosine or by dot product.

The question a product page asks of the same embeddings that answer ``recommendK``: "which items are like this one?"
``lgc_item_neighbors`` scores the asked-about rows against the whole catalogue on the fp32 matrix cores and selects the k
best per row in the same launch; the ``[n, n_items]`` score matrix never exists.  The scores have
the bits of ``score_rows`` (times the two norms for the cosine) and the order is ``mask_topk``'s, so the answer is the one
the composed route gives, bit for bit.

What this does NOT do: no approximate index (every item is scored), no user -> item ranking (that is ``recommendK``), and
at most 64 neighbours per item.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native
from .propagate import _check_ids, _check_tables, _snapshot_status, _status

__all__ = ["row_rnorm", "item_neighbors", "METRICS"]

METRICS = ("cosine", "dot")


def row_rnorm(table: Tensor) -> Tensor:
    """``1 / sqrt(sum_d table[r, d] ** 2)`` per row, fp32 ``[n_rows]`` (lgc_row_rnorm): one chain of fused multiply-adds
    over ascending d, square root and division correctly rounded.  A zero row gives 0, a NaN row NaN."""
    _check_tables(table, table)
    out = torch.empty(table.size(0), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        code = _native.load().lgc_row_rnorm(_native.ptr(table), table.stride(0), table.size(0), table.size(1),
                                            _native.ptr(out), _native.stream_of(table.device))
    _native.check(code, "lgc_row_rnorm")
    return out


def item_neighbors(items: Tensor, k: int, queries: Optional[Tensor] = None, metric: str = "cosine",
                   item_ok: Optional[Tensor] = None, exclude_self: bool = True, slices: int = 0) -> Tuple[Tensor, Tensor]:
    """``(index int64 [n, k], value fp32 [n, k])``: per asked-about item the k most similar items of ``items`` (fp32
    ``[n_items, dim]``) in ``mask_topk``'s order (NaN first, then descending, equal values by ascending index).
    ``queries``: int64 item indices, None = every item in order.  ``metric``: "cosine" or "dot".  ``item_ok``: bool or
    uint8 ``[n_items]``, an item whose entry is 0 is never returned.  ``exclude_self``: leave the asked-about item out of
    its own answer.  With fewer than k candidates a row ends in -1 / -inf.  ``slices`` only moves work (0 = the library
    chooses); the result does not depend on it.  A query outside the table gives a row of -1 / -inf and raises at
    ``check_index_status()``."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.NEIGHBORS_MAX_K:
        raise ValueError(f"k must be an integer in [1, {_native.NEIGHBORS_MAX_K}]")
    if isinstance(slices, bool) or not isinstance(slices, int) or not 0 <= slices <= 64:
        raise ValueError("slices must be an integer in [0, 64]")
    _check_tables(items, items)
    _check_ids(queries, items, "queries")
    dev, n_items = items.device, items.size(0)
    if item_ok is not None:
        if item_ok.dtype == torch.bool:
            item_ok = item_ok.to(torch.uint8)
        if item_ok.dtype != torch.uint8 or item_ok.dim() != 1 or not item_ok.is_contiguous() or item_ok.device != dev \
                or item_ok.numel() != n_items:
            raise TypeError(f"item_ok must be a contiguous bool or uint8 tensor of {n_items} entries on the table's device")
    n = n_items if queries is None else queries.numel()
    index = torch.empty((n, k), dtype=torch.int64, device=dev)
    value = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return index, value
    lib = _native.load()
    scale = row_rnorm(items) if metric == "cosine" else None
    ws_bytes = lib.lgc_item_neighbors_workspace_bytes(n, n_items, k, slices)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        code = lib.lgc_item_neighbors(_native.ptr(items), items.stride(0), n_items, items.size(1), _native.ptr(queries), n,
                                      _native.ptr(scale), _native.ptr(item_ok), int(bool(exclude_self)), k, slices,
                                      _native.ptr(index), _native.ptr(value), _native.ptr(ws), ws_bytes,
                                      _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_item_neighbors")
    _snapshot_status(dev)
    return index, value
