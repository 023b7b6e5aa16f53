"""Fold-in: embeddings and recommendations for nodes the model was not trained on.

A trained ``LightGCN`` can only answer for a row of its embedding table.  A new visitor -- or a known user whose basket
changed after the last training run -- has an interaction list instead.  Because the user side of the propagation is
linear in the item tables (``propagate.bipartite_sum``), such a node ``u`` with list ``(i_k, w_k)`` and layer-0 row
``z`` (zero for an unknown visitor) has the embedding

    e_u = alpha_0 * z + sum_k c_k * F[i_k],     F = sum_{l=0..K-1} alpha_{l+1} * x_l[items],
    c_k = dis_item[i_k] * w_k * d_u,            d_u = (sum_k w_k)^-1/2   (inf -> 0)

which is exactly ``get_embedding`` on the trained graph plus one node with one-way edges ``i_k -> u``: the existing
degrees and rows do not move.  ``F`` is one ``[n_items, D]`` table per model and graph
(``fold_table``: one ``propagate_sum`` with the coefficients shifted by one, cached beside the served table); a request
is one ``lgc_fold_in`` launch (``fold_in``) followed by the serving tail that known users take (``recommend_topk``).

What this does NOT model: the visitor's effect on the items' degrees and, through them, on every other row -- the
difference between one-way and two-way edges.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _native
from .graph import PropGraph
from .propagate import SeenLists, _check_ids, _check_tables, _snapshot_status, _status, propagate_sum

__all__ = ["SessionLists", "fold_table", "fold_in"]

MASK_RULES = ("purchased", "all", None)


class SessionLists:
    """The interaction lists of a request as a CSR: ``ptr`` int64 [n_rows + 1], ``items`` int64 item indices in
    ``[0, n_items)`` (no ``n_users`` offset: the convention of ``SeenLists``), ``weights`` fp32 per entry or None for all
    ones (the reference weighs view / cart / purchase 0.01 / 0.1 / 1.0)."""

    def __init__(self, ptr: Tensor, items: Tensor, weights: Optional[Tensor] = None):
        self.ptr, self.items, self.weights = ptr, items, weights
        self._host = None                 # (ptr, items, weights) on the host, when built there: validate() reads these
        self._valid_for = None            # the n_items a successful validate() has seen

    @property
    def n_rows(self) -> int:
        return self.ptr.numel() - 1

    @classmethod
    def from_lists(cls, lists: Sequence, device=None) -> "SessionLists":
        """From a sequence of ``(items, weights-or-None)`` pairs, one per request row.  A row without weights counts as
        all ones; when no row has any the result carries no weight array at all."""
        import numpy as np
        item_rows, weight_rows, any_weight = [], [], False
        for pos, pair in enumerate(lists):
            try:
                items, weights = pair
            except (TypeError, ValueError):
                raise ValueError(f"session {pos}: expected an (items, weights-or-None) pair") from None
            it = np.asarray(list(items))
            if it.size and it.dtype.kind not in "iu":
                raise ValueError(f"session {pos}: item indices must be integers")
            it = it.astype(np.int64).reshape(-1)
            if weights is None:
                w = np.ones(it.size, dtype=np.float32)
            else:
                any_weight = True
                try:
                    w = np.asarray(list(weights), dtype=np.float32).reshape(-1)
                except (TypeError, ValueError):
                    raise ValueError(f"session {pos}: weights must be numbers") from None
                if w.size != it.size:
                    raise ValueError(f"session {pos}: {it.size} items but {w.size} weights")
            item_rows.append(it)
            weight_rows.append(w)
        ptr = np.zeros(len(item_rows) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in item_rows], out=ptr[1:])
        items = np.concatenate(item_rows) if item_rows else np.zeros(0, dtype=np.int64)
        weights = (np.concatenate(weight_rows) if weight_rows else np.zeros(0, dtype=np.float32)) if any_weight else None
        host = (torch.from_numpy(ptr), torch.from_numpy(items), None if weights is None else torch.from_numpy(weights))
        got = cls(*(None if t is None else t.to(device) for t in host))
        got._host = host
        return got

    def validate(self, n_items: int, where: str = "session lists") -> "SessionLists":
        """lgc_fold_in and lgc_mask_topk read ``ptr`` on trust: a list that is not a monotone 0 .. len(items) sequence,
        an item outside ``[0, n_items)`` or a weight that is not a finite fp32 number ends here in a ValueError.  Runs
        on the host copy where the lists were built there (``from_lists``: before anything is uploaded is read), else
        on a copy fetched from the device (one sync)."""
        def bad(msg):
            raise ValueError(f"{where}: {msg}")
        if self._valid_for == int(n_items):
            return self
        for t, name in ((self.ptr, "ptr"), (self.items, "items")):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
                bad(f"{name} must be a contiguous 1-D int64 tensor")
        if self.ptr.numel() < 1:
            bad("ptr must hold at least one entry")
        w = self.weights
        if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous()
                              or w.numel() != self.items.numel()):
            bad(f"weights must be a contiguous fp32 tensor of {self.items.numel()} entries")
        if self.items.device != self.ptr.device or (w is not None and w.device != self.ptr.device):
            bad("ptr, items and weights must live on the same device")
        ptr, items, weights = self._host if self._host is not None else (self.ptr.cpu(), self.items.cpu(),
                                                                         None if w is None else w.cpu())
        if int(ptr[0]) != 0 or int(ptr[-1]) != items.numel() or bool((ptr[1:] < ptr[:-1]).any()):
            bad("ptr is not a non-decreasing 0 .. len(items) sequence")
        if items.numel() and (int(items.min()) < 0 or int(items.max()) >= n_items):
            bad(f"item indices must lie in [0, {n_items})")
        if weights is not None and not bool(torch.isfinite(weights).all()):
            bad("weights must be finite")
        self._valid_for = int(n_items)
        return self

    def mask(self, rule="purchased") -> Optional[SeenLists]:
        """The seen-mask of the request's score rows, row r = session r: ``"purchased"`` lists the entries of weight
        1.0 -- upstream's rule for its seen matrix (src/utils_v2.py:96) --, ``"all"`` every entry, None no mask."""
        if rule not in MASK_RULES:
            raise ValueError(f"mask rule must be one of {MASK_RULES}, got {rule!r}")
        if rule is None or self.items.numel() == 0:          # nothing listed: no mask (the kernels take no empty array)
            return None
        if rule == "all" or self.weights is None:
            return SeenLists(self.ptr, self.items)
        if self._host is not None:                           # built on the host: filter there, two small uploads, no sync
            ptr, items, weights = self._host
            keep = weights == 1.0
            if not bool(keep.any()):
                return None
            kept = torch.zeros(keep.numel() + 1, dtype=torch.int64)
            kept[1:] = torch.cumsum(keep, 0)
            return SeenLists(kept[ptr].to(self.ptr.device), items[keep].to(self.ptr.device))
        keep = self.weights == 1.0
        kept = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=keep.device)
        kept[1:] = torch.cumsum(keep, 0)
        items = self.items[keep].contiguous()
        return SeenLists(kept[self.ptr].contiguous(), items) if items.numel() else None


def fold_table(model, graph: PropGraph) -> Tensor:
    """``F = sum_{l=0..K-1} alpha_{l+1} x_l[items]`` (fp32 ``[n_items, D]``, detached): the item block of the layer sum
    with the coefficients shifted by one -- K - 1 hops, once per (graph, weights, alpha), kept on the model beside the
    served table and dropped with it (``LightGCN.invalidate``).  ``graph.split`` is ``n_users``."""
    if model.num_layers == 0:
        raise ValueError("a model without layers has nothing to fold a list through")
    if graph.split is None:
        raise ValueError("fold-in needs a user|item graph (every edge joining a node below the split with one above it)")
    w = model.embedding.weight
    _native.require_device(w, "LightGCN.embedding.weight")
    alphas = model._alphas()
    key = (id(graph), w.data_ptr(), w._version, w.device, alphas)
    got = getattr(model, "_fold", None)
    if got is None or got[0] != key:
        with torch.no_grad():
            table = propagate_sum(w.detach(), graph, alphas[1:])[graph.split:].detach()
        got = (key, graph, table)
        model._fold = got
        model.fold_tables_built = getattr(model, "fold_tables_built", 0) + 1
    return got[2]


def fold_in(fold: Tensor, item_dis: Optional[Tensor], sessions: SessionLists, init_table: Optional[Tensor] = None,
            init_rows: Optional[Tensor] = None, a0: float = 0.0, normalize: bool = True) -> Tensor:
    """fp32 ``[n_rows, D]``: row r = ``a0 * init_table[init_rows[r]] + sum_k c_k * fold[i_k]`` over session r's list
    (lgc_fold_in; the arithmetic contract is in include/lgconv_hip.h).  ``init_rows``: int64 ``[n_rows]``, -1 = no row.
    An item or an init id out of range contributes nothing and raises at ``check_index_status()``."""
    _check_tables(fold if init_table is None else init_table, fold)
    dev, n_items, dim = fold.device, fold.size(0), fold.size(1)
    _check_ids(sessions.ptr, fold, "sessions.ptr")
    _check_ids(sessions.items, fold, "sessions.items")
    if sessions.ptr.numel() < 1:
        raise ValueError("sessions.ptr must hold at least one entry")
    w = sessions.weights
    if w is not None and (w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous() or w.device != dev
                          or w.numel() != sessions.items.numel()):
        raise TypeError("sessions.weights must be a contiguous fp32 tensor with one entry per item, on the tables' device")
    if normalize:
        if item_dis is None:
            raise ValueError("normalize=True needs item_dis (the item slice of the graph's dis)")
        if (item_dis.dtype != torch.float32 or item_dis.dim() != 1 or not item_dis.is_contiguous() or item_dis.device != dev
                or item_dis.numel() != n_items):
            raise TypeError(f"item_dis must be a contiguous fp32 tensor of {n_items} entries on the tables' device")
    n_rows = sessions.n_rows
    if (init_rows is None) != (init_table is None):
        raise ValueError("init_table and init_rows come together")
    if init_rows is not None:
        _check_ids(init_rows, fold, "init_rows")
        if init_rows.numel() != n_rows:
            raise ValueError(f"{init_rows.numel()} init rows for {n_rows} sessions")
    out = torch.empty((n_rows, dim), dtype=torch.float32, device=dev)
    if n_rows == 0:
        return out
    # a request of empty lists only has no item array to point at: the kernel reads none of it, but wants a pointer
    items = sessions.items if sessions.items.numel() else sessions.items.new_zeros(1)
    with torch.cuda.device(dev):
        code = _native.load().lgc_fold_in(
            _native.ptr(sessions.ptr), _native.ptr(items), _native.ptr(w if items is sessions.items else None), n_rows,
            _native.ptr(item_dis) if normalize else None, _native.ptr(fold), fold.stride(0), n_items,
            _native.ptr(init_rows), _native.ptr(init_table), 0 if init_table is None else init_table.stride(0),
            0 if init_table is None else init_table.size(0), float(a0), int(bool(normalize)), dim, _native.ptr(out), dim,
            _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_fold_in")
    _snapshot_status(dev)
    return out
