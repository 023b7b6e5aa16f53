"""Score attribution: which of a visitor's own items produced a recommendation.

Fold-in (``foldin``) embeds a node from its list as ``e_u = alpha_0 * z_u + sum_k c_k * F[i_k]``.  The same line dotted with a
served item row ``E[t]`` splits every score additively over the list,

    score(u, t) = <e_u, E[t]> = alpha_0 <z_u, E[t]>  +  sum_k c_k <F[i_k], E[t]>  =  base[t] + sum_k contrib[k, t]

with ``c_k`` fold-in's coefficient for a session and, for a trained user, simply the value stored in the user's row of
the forward CSR.  No approximation, no gradients, no second model: "because you bought X (0.41),
Y (0.22), Z (0.08)", with contributions that sum to the score.  One ``lgc_attribute`` launch per group of 64 target columns
gives the full split (for the offline analysis of an evaluation run) and the m largest contributions per target (for the
handler).

What attribution does NOT say: it does not merge a repeated item into one contributor, it does not follow the visitor's
two-way effect on the items' degrees (fold-in's own caveat), and it is of the UNMASKED score -- ``recommendK`` zeroes a
seen item's score rather than removing it, so a seen item's explanation is of its raw score.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from . import _native
from .foldin import SessionLists
from .propagate import _check_ids, _check_tables, _snapshot_status, _status

__all__ = ["Attribution", "attribute"]


@dataclass
class Attribution:
    """``base`` / ``total`` fp32 ``[n_rows, k]``; ``top_pos`` int32, ``top_item`` int64, ``top_value`` fp32 ``[n_rows, k, m]``
    (unused places -1 / -1 / 0); with ``full=True`` ``contrib`` fp32 ``[n_entries, k]`` and ``contrib_ptr`` int64
    ``[n_rows + 1]``: the rows ``contrib_ptr[r] .. contrib_ptr[r + 1]`` are request row r's list in order."""
    base: Tensor
    total: Tensor
    top_pos: Tensor
    top_item: Tensor
    top_value: Tensor
    contrib: Optional[Tensor] = None
    contrib_ptr: Optional[Tensor] = None


def _check_vector(t: Tensor, like: Tensor, n: int, name: str) -> None:
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.device != like.device or t.numel() != n:
        raise TypeError(f"{name} must be a contiguous fp32 tensor of {n} entries on the tables' device")


def attribute(fold: Tensor, items: Tensor, targets: Tensor, *, sessions: Optional[SessionLists] = None,
              item_dis: Optional[Tensor] = None, normalize: bool = True, rowptr: Optional[Tensor] = None,
              entries: Optional[Tensor] = None, row_ids: Optional[Tensor] = None, col_base: int = 0,
              contrib_ptr: Optional[Tensor] = None, init_table: Optional[Tensor] = None, init_rows: Optional[Tensor] = None,
              a0: float = 0.0, m: int = 3, full: bool = False) -> Attribution:
    """Split ``<e_r, items[targets[r, j]]>`` over request row r's list (lgc_attribute; the contract is in
    include/lgconv_hip.h).  The lists come in exactly one form: ``sessions`` (+ ``item_dis`` with ``normalize``), or the rows
    ``row_ids`` of the CSR ``rowptr`` / ``entries`` whose columns are item nodes ``col_base + item``.  ``targets``: int64
    ``[n_rows, k]`` item indices (-1 = no target); more than 64 columns take one launch per group of 64.  ``full=True``
    also returns every contribution; the graph form then needs ``contrib_ptr`` (int64 ``[n_rows + 1]``, the prefix sum of
    the row lengths), the session form uses the lists' own ``ptr``.  The attribution is of the raw, unmasked score.  An
    index out of range contributes nothing and raises at ``check_index_status()``."""
    graph_form = rowptr is not None or entries is not None or row_ids is not None
    if (sessions is not None) == graph_form:
        raise ValueError("give the lists in exactly one form: sessions, or rowptr + entries + row_ids")
    if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= _native.ATTR_MAX_TOP:
        raise ValueError(f"m must be an integer in [0, {_native.ATTR_MAX_TOP}]")
    _check_tables(fold, items)
    if fold.size(0) != items.size(0):
        raise ValueError(f"fold has {fold.size(0)} rows, items {items.size(0)}")
    dev, n_items, dim = fold.device, fold.size(0), fold.size(1)
    if targets.dtype != torch.int64 or targets.dim() != 2 or targets.device != dev or (targets.size(1) > 1 and targets.stride(1) != 1):
        raise TypeError("targets must be a 2-D int64 tensor with unit inner stride on the tables' device")
    if targets.size(1) < 1:
        raise ValueError("no target columns")
    args = _native.AttrArgsC()
    keep = []                                                # what the raw pointers below point into
    if sessions is not None:
        _check_ids(sessions.ptr, fold, "sessions.ptr")
        _check_ids(sessions.items, fold, "sessions.items")
        if sessions.ptr.numel() < 1:
            raise ValueError("sessions.ptr must hold at least one entry")
        n_rows = sessions.n_rows
        w = sessions.weights
        if w is not None:
            _check_vector(w, fold, sessions.items.numel(), "sessions.weights")
        if normalize:
            if item_dis is None:
                raise ValueError("normalize=True needs item_dis (the item slice of the graph's dis)")
            _check_vector(item_dis, fold, n_items, "item_dis")
        # a request of empty lists only has no item array to point at: the kernel reads none of it, but wants a pointer
        list_items = sessions.items if sessions.items.numel() else sessions.items.new_zeros(1)
        keep.append(list_items)
        args.list_ptr, args.list_items = _native.ptr(sessions.ptr), _native.ptr(list_items)
        args.list_weight = _native.ptr(w if list_items is sessions.items else None)
        args.item_dis = _native.ptr(item_dis) if normalize else None
        args.normalize = int(bool(normalize))
        if full:
            contrib_ptr = sessions.ptr
    else:
        if rowptr is None or entries is None or row_ids is None:
            raise ValueError("the graph form needs rowptr, entries and row_ids")
        if rowptr.dtype != torch.int32 or rowptr.dim() != 1 or not rowptr.is_contiguous() or rowptr.device != dev or rowptr.numel() < 1:
            raise TypeError("rowptr must be a contiguous 1-D int32 tensor on the tables' device")
        if entries.dtype != torch.int32 or entries.dim() != 2 or entries.size(1) != 2 or not entries.is_contiguous() or entries.device != dev:
            raise TypeError("entries must be a contiguous int32 [n, 2] tensor (lgc_entry) on the tables' device")
        _check_ids(row_ids, fold, "row_ids")
        n_rows = row_ids.numel()
        rows_arg = row_ids if n_rows else row_ids.new_zeros(1)
        ent_arg = entries if entries.numel() else entries.new_zeros((1, 2))
        keep += [rows_arg, ent_arg]
        args.rowptr, args.entries, args.row_ids = _native.ptr(rowptr), _native.ptr(ent_arg), _native.ptr(rows_arg)
        args.n_graph_rows, args.col_base = rowptr.numel() - 1, int(col_base)
        if full:
            if contrib_ptr is None:
                raise ValueError("full=True in the graph form needs contrib_ptr (the prefix sum of the row lengths)")
            _check_ids(contrib_ptr, fold, "contrib_ptr")
            if contrib_ptr.numel() != n_rows + 1:
                raise ValueError(f"contrib_ptr has {contrib_ptr.numel()} entries for {n_rows} rows")
    if targets.size(0) != n_rows:
        raise ValueError(f"{targets.size(0)} target rows for {n_rows} request rows")
    if (init_rows is None) != (init_table is None):
        raise ValueError("init_table and init_rows come together")
    if init_rows is not None:
        _check_tables(init_table, fold)
        _check_ids(init_rows, fold, "init_rows")
        if init_rows.numel() != n_rows:
            raise ValueError(f"{init_rows.numel()} init rows for {n_rows} request rows")
        args.init_rows, args.init = _native.ptr(init_rows), _native.ptr(init_table)
        args.init_stride, args.n_init_rows = init_table.stride(0), init_table.size(0)
    k = targets.size(1)
    base = torch.empty((n_rows, k), dtype=torch.float32, device=dev)
    total = torch.empty((n_rows, k), dtype=torch.float32, device=dev)
    top_pos = torch.empty((n_rows, k, m), dtype=torch.int32, device=dev)
    top_item = torch.empty((n_rows, k, m), dtype=torch.int64, device=dev)
    top_value = torch.empty((n_rows, k, m), dtype=torch.float32, device=dev)
    got = Attribution(base, total, top_pos, top_item, top_value)
    n_entries = 0
    if full:
        n_entries = sessions.items.numel() if sessions is not None else None
        if n_entries is None:
            n_entries = int(contrib_ptr[-1].item()) if n_rows else 0        # the one size only the device knows
        # zeros: a slot of a span that is longer than its list is never written by the kernel
        got.contrib = torch.zeros((n_entries, k), dtype=torch.float32, device=dev)
        got.contrib_ptr = contrib_ptr
    if n_rows == 0:
        return got
    args.n_rows, args.fold, args.items = n_rows, _native.ptr(fold), _native.ptr(items)
    args.fold_stride, args.item_stride, args.n_items = fold.stride(0), items.stride(0), n_items
    args.a0, args.top_m, args.dim = float(a0), m, dim
    args.status = _native.ptr(_status(dev))
    args.target_stride = targets.stride(0) if n_rows > 1 else k
    lib = _native.load()
    cap = _native.ATTR_MAX_TARGETS
    with torch.cuda.device(dev):
        for c0 in range(0, k, cap):
            c1 = min(k, c0 + cap)
            whole = c0 == 0 and c1 == k                      # one group: the outputs are written in place
            part = [t if whole else t.new_empty((n_rows, c1 - c0) + tuple(t.shape[2:]))
                    for t in (base, total, top_pos, top_item, top_value)]
            part_c = None
            if full:
                part_c = got.contrib if whole else got.contrib.new_zeros((n_entries, c1 - c0))
                if not n_entries:                            # the kernel wants a pointer even where no row has an entry
                    keep.append(part_c.new_empty(1))
                args.contrib = _native.ptr(part_c if n_entries else keep[-1])
                args.contrib_ptr = _native.ptr(contrib_ptr)
            args.targets = targets.data_ptr() + 8 * c0
            args.n_targets = c1 - c0
            args.base, args.total = _native.ptr(part[0]), _native.ptr(part[1])
            if m:
                args.top_pos, args.top_item, args.top_value = (_native.ptr(t) for t in part[2:])
            code = lib.lgc_attribute(args, _native.stream_of(dev))
            _native.check(code, "lgc_attribute")
            if not whole:
                for t, p in zip((base, total, top_pos, top_item, top_value), part):
                    t[:, c0:c1] = p
                if full:
                    got.contrib[:, c0:c1] = part_c
    _snapshot_status(dev)
    return got
