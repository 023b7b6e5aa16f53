"""Diversified re-ranking: greedy maximal marginal relevance over a candidate list, and intra-list diversity.

The question a shop asks once it has ``recommendK`` and ``similar_items``: "give me k recommendations that are not twenty
shades of one lipstick."  ``lgc_rerank_mmr`` takes every row's candidates -- the ``N`` best of ``recommend_topk`` with
their masked scores -- and chooses k of them one at a time: the candidate with the best
``lam * relevance - (1 - lam) * max similarity to what is already chosen``.  One launch, one wavefront per row; a row's
``N x N`` similarity matrix is never formed.  The arithmetic is stated in include/lgconv_hip.h and
the order is ``mask_topk``'s, so the answer is a function of the inputs alone, bit for bit; with ``lam = 1`` it is
``recommend_topk(k)`` itself.  ``lgc_list_diversity`` is the metric that judges the result: the mean pairwise
``1 - similarity`` inside the first c places of a list, at several cutoffs.

What this does NOT do: no objective other than MMR (no determinantal point process, no category quotas), at most 256
candidates per row, no partitioned multi-GPU path, nothing at training time.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from . import _native
from .propagate import _check_tables, _host_cutoffs, _snapshot_status, _status
from .similar import METRICS, row_rnorm

__all__ = ["mmr_rerank", "list_diversity", "rerank_route", "check_lam"]


def rerank_route(n_cand: int, dim: int) -> str:
    """"lds" or "global": where ``lgc_rerank_mmr`` reads a row's candidates from at that shape (lgc_rerank_route)."""
    code = _native.load().lgc_rerank_route(int(n_cand), int(dim))
    _native.check(min(code, 0), "lgc_rerank_route")
    return _native.RERANK_ROUTES[code]


def check_lam(lam) -> float:
    """``lam`` as a Python float: any real number in [0, 1] -- a Python or numpy scalar, a 0-d floating tensor --, no bool."""
    if torch.is_tensor(lam) and lam.dim() == 0 and lam.is_floating_point():
        lam = lam.item()
    if isinstance(lam, (bool, np.bool_)) or not isinstance(lam, numbers.Real) or math.isnan(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam must be a real number in [0, 1], got {lam!r}")
    return float(lam)


def _check_lists(lists: Tensor, like: Tensor, name: str) -> None:
    if not torch.is_tensor(like):
        raise TypeError("items must be a 2-D fp32 tensor")
    if not torch.is_tensor(lists) or lists.dtype != torch.int64 or lists.dim() != 2 or lists.size(1) < 1 \
            or lists.stride(1) != 1 or (lists.size(0) > 1 and lists.stride(0) < lists.size(1)) or lists.device != like.device:
        raise TypeError(f"{name} must be a 2-D int64 tensor with unit inner stride on the table's device")
    if lists.size(1) > _native.RERANK_MAX_CAND:
        raise ValueError(f"{name}: at most {_native.RERANK_MAX_CAND} entries per row, got {lists.size(1)}")


def mmr_rerank(items: Tensor, cand: Tensor, rel: Tensor, k: int, lam: float = 0.7, metric: str = "cosine",
               return_values: bool = False):
    """``index`` int64 ``[n, k]`` -- or ``(index, pos int32 [n, k], value fp32 [n, k])`` with ``return_values`` --: out of
    the candidates ``cand`` (int64 ``[n, N]`` item indices into ``items``, fp32 ``[n_items, dim]``; -1 = an empty place)
    with relevance ``rel`` (fp32 ``[n, N]``), k per row in the order greedy MMR chooses them (lgc_rerank_mmr).  ``lam``
    in [0, 1]: 1 ranks by relevance alone, 0 by dissimilarity alone.  ``metric``: "cosine" (``similar.row_rnorm`` of the
    table scales the dot products) or "dot".  ``pos`` is the place in the candidate row, ``value`` the objective at the
    moment of choice.  Equal objectives go to the lower position; a row with fewer than k candidates ends in
    -1 / -1 / -inf.  An id outside the table is skipped and raises at ``check_index_status()``."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    lam = check_lam(lam)
    _check_lists(cand, items, "cand")
    n, n_cand, dev = cand.size(0), cand.size(1), items.device
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= n_cand:
        raise ValueError(f"k must be an integer in [1, {n_cand}] (the number of candidates)")
    _check_tables(items, items)
    if not torch.is_tensor(rel) or rel.dtype != torch.float32 or rel.shape != cand.shape or rel.stride(1) != 1 \
            or (n > 1 and rel.stride(0) < n_cand) or rel.device != dev:
        raise TypeError(f"rel must be fp32 {list(cand.shape)} with unit inner stride on the table's device")
    index = torch.empty((n, k), dtype=torch.int64, device=dev)
    pos = torch.empty((n, k), dtype=torch.int32, device=dev) if return_values else None
    value = torch.empty((n, k), dtype=torch.float32, device=dev) if return_values else None
    if n:
        scale = row_rnorm(items) if metric == "cosine" else None
        with torch.cuda.device(dev):
            code = _native.load().lgc_rerank_mmr(_native.ptr(items), items.stride(0), items.size(0), items.size(1),
                                                 _native.ptr(scale), _native.ptr(cand), cand.stride(0) if n > 1 else n_cand,
                                                 _native.ptr(rel), rel.stride(0) if n > 1 else n_cand, n, n_cand, k, lam,
                                                 _native.ptr(index), _native.ptr(pos), _native.ptr(value),
                                                 _native.ptr(_status(dev)), _native.stream_of(dev))
        _native.check(code, "lgc_rerank_mmr")
        _snapshot_status(dev)
    return (index, pos, value) if return_values else index


def list_diversity(items: Tensor, lists: Tensor, cutoffs, metric: str = "cosine") -> Tensor:
    """float64 ``[n, len(cutoffs)]`` on the device: per row of ``lists`` (int64 ``[n, k]`` item indices, -1 = an empty
    place) and cutoff c (ascending, 1 .. k) the mean of ``1 - similarity`` over the pairs among the valid entries of its
    first c places (lgc_list_diversity); NaN where fewer than two are valid.  ``metric`` as ``mmr_rerank``.  The sums
    run in a fixed order in float64: the same bits on every run."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    _check_lists(lists, items, "lists")
    n, k, dev = lists.size(0), lists.size(1), items.device
    cuts, cuts_c = _host_cutoffs(cutoffs, k)
    _check_tables(items, items)
    out = torch.empty((n, len(cuts)), dtype=torch.float64, device=dev)
    if n:
        scale = row_rnorm(items) if metric == "cosine" else None
        with torch.cuda.device(dev):
            code = _native.load().lgc_list_diversity(_native.ptr(items), items.stride(0), items.size(0), items.size(1),
                                                     _native.ptr(scale), _native.ptr(lists), lists.stride(0) if n > 1 else k,
                                                     n, k, cuts_c, len(cuts), _native.ptr(out), len(cuts),
                                                     _native.ptr(_status(dev)), _native.stream_of(dev))
        _native.check(code, "lgc_list_diversity")
        _snapshot_status(dev)
    return out
