"""Hop distances and shortest paths from users to their recommended items, on the device.

The second half of the reference's offline inference (``InferenceLightGCN.compute_paths``,
src/inference_lightgcn.py:85-119) asks, for every user with a hit, how many hops away each of the k recommended items
lies, whether any lies beyond 3 hops, and for one shortest path per pair -- three networkx searches per pair on the
host.  Here it is a level-synchronous breadth-first search over the forward CSR the propagation already holds
(``graph.forward_op``: row v lists the sources j of the edges j -> v, which is the pull direction of the search and the
predecessor list of the walk back), 64 sources per sweep: bit b of a node's 64-bit word belongs to source b
(lgc_bfs_init / _level / _resolve / _backtrack, csrc/lgconv_paths.hip).

Distances: the number of edges of a shortest walk along ``edge_index``'s source -> target direction (for upstream's
symmetric edge list: the undirected distance); -1 = no path (the source's frontier emptied), -2 = not reached within
``max_hops``.  Everything is integer arithmetic; the results are the same bits on every run.

The one deviation from upstream: ``compute_paths`` there raises ``NetworkXNoPath`` as soon as one recommended item is
unreachable (its ``path_len`` handles the case, its ``paths`` does not).  Here such a pair gives -1 and ``[]``.
"""
from __future__ import annotations

import time
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _native
from .graph import PropGraph
from .propagate import DEFAULT_WORKSPACE_BYTES, _snapshot_status, _status

__all__ = ["hop_distances", "shortest_paths", "paths_frame", "compute_paths"]

NO_PATH = -1           # the source's frontier emptied before it met the target
BEYOND_MAX_HOPS = -2   # max_hops levels ran and the source's frontier was still alive
_COUNTER_LEVELS = 64   # counter blocks (4 words per level) allocated at a time


def _check_pairs(graph: PropGraph, sources: Tensor, targets: Tensor) -> None:
    if not isinstance(graph, PropGraph):
        raise TypeError("graph must be a PropGraph (get_graph(...) or PropGraph.load(...))")
    for t, name, dim in ((sources, "sources", 1), (targets, "targets", 2)):
        _native.require_device(t, name)
        if t.dtype != torch.int64 or t.dim() != dim or not t.is_contiguous() or t.device != graph.device:
            raise TypeError(f"{name} must be a contiguous {dim}-D int64 tensor on the graph's device")
    if targets.size(0) != sources.numel():
        raise ValueError(f"{sources.numel()} sources for {targets.size(0)} rows of targets")
    plan = graph.forward_op.plan
    if plan.row_begin != 0 or plan.row_end != graph.num_nodes:
        raise ValueError("the forward operator's row plan must cover every row of the graph")


def _search(graph: PropGraph, sources: Tensor, targets: Tensor, max_hops: Optional[int], max_len: Optional[int],
            trace: Optional[list]) -> Tuple[Tensor, Optional[Tensor]]:
    """The BFS of both public functions.  ``max_len`` None: distances only (three [N] words of device memory per batch,
    whatever S is); else levels 0..max_len are kept ([max_len + 1, N] words) and walked back.  ``trace`` (a list)
    receives one ``(batch, level, nodes newly reached, pairs settled, seconds since the batch began)`` per level."""
    _check_pairs(graph, sources, targets)
    if max_hops is not None and max_hops < 0:
        raise ValueError("max_hops must be >= 0")
    lib = _native.load()
    op, dev, n_nodes = graph.forward_op, graph.device, graph.num_nodes
    plan = op.plan
    n_src, n_tgt = targets.shape
    keep = max_len is not None
    dist = torch.full((n_src, n_tgt), _native.BFS_UNSET, dtype=torch.int32, device=dev)
    paths = torch.full((n_src, n_tgt, max_len + 1), -1, dtype=torch.int64, device=dev) if keep else None
    if n_src == 0 or n_tgt == 0:
        return dist, paths
    if n_nodes == 0:                                     # every id is out of range
        dist.fill_(NO_PATH)
        with torch.cuda.device(dev):
            _status(dev)[0] |= _native.ST_INDEX_OOB
        return dist, paths
    words = dict(dtype=torch.int64, device=dev)
    seen = torch.empty(n_nodes, **words)
    levels = torch.empty((max_len + 1, n_nodes), **words) if keep else None
    spare = (torch.empty(n_nodes, **words), torch.empty(n_nodes, **words))

    def frontier(level: int) -> Tensor:                  # level l is written straight into row l while rows are kept
        return levels[level] if keep and level <= max_len else spare[level & 1]

    # a source outside the graph sets no bit anywhere: left in `active` it would keep every row "not yet reached by all"
    # and the skip in lgc_bfs_level from ever firing.  One host read per call, before any level.
    valid = ((sources >= 0) & (sources < n_nodes)).tolist()
    status = _native.ptr(_status(dev))
    rowptr, entries, chunks = _native.ptr(op.rowptr), _native.ptr(op.entries), _native.ptr(plan.chunks)
    with torch.cuda.device(dev):
        stream = _native.stream_of(dev)
        for batch, lo in enumerate(range(0, n_src, _native.BFS_MAX_SOURCES)):
            n = min(_native.BFS_MAX_SOURCES, n_src - lo)
            src, tgt, d = sources[lo:lo + n], targets[lo:lo + n], dist[lo:lo + n]
            active = sum(1 << b for b in range(n) if valid[lo + b])      # 0: level 0 settles every pair (-1)
            unset, dead, level, emptied = n * n_tgt, 0, 0, False
            t0 = time.perf_counter()
            _native.check(lib.lgc_bfs_init(_native.ptr(src), n, n_nodes, _native.ptr(seen), _native.ptr(frontier(0)),
                                           status, stream), "lgc_bfs_init")
            while True:
                if level % _COUNTER_LEVELS == 0:
                    block = torch.zeros((_COUNTER_LEVELS, 4), **words)
                counters = block[level % _COUNTER_LEVELS]
                if level > 0:
                    code = lib.lgc_bfs_level(rowptr, entries, plan.row_begin, plan.row_end, plan.short_max,
                                             chunks if plan.n_chunks else None, plan.n_chunks, active,
                                             _native.ptr(frontier(level - 1)), _native.ptr(frontier(level)),
                                             _native.ptr(seen), _native.ptr(counters), stream)
                    _native.check(code, "lgc_bfs_level")
                code = lib.lgc_bfs_resolve(_native.ptr(src), _native.ptr(tgt), n, n_tgt, n_nodes,
                                           _native.ptr(frontier(level)), level, _native.ptr(d), _native.ptr(counters),
                                           status, stream)
                _native.check(code, "lgc_bfs_resolve")
                new, settled, alive, _ = counters.tolist()            # the level's one host read
                unset -= settled
                if level > 0:
                    dead |= active & ~alive                           # a frontier that emptied stays empty
                if trace is not None:
                    trace.append((batch, level, new, settled, time.perf_counter() - t0))
                emptied = level > 0 and new == 0
                if unset == 0 or emptied or (max_hops is not None and level >= max_hops):
                    break
                level += 1
            if unset:
                rest = d == _native.BFS_UNSET
                if emptied:
                    d.masked_fill_(rest, NO_PATH)
                else:
                    gone = torch.tensor([bool((dead >> b) & 1) for b in range(n)], device=dev).unsqueeze(1)
                    d.masked_fill_(rest & gone, NO_PATH)
                    d.masked_fill_(rest & ~gone, BEYOND_MAX_HOPS)
            if keep:
                code = lib.lgc_bfs_backtrack(rowptr, entries, n_nodes, _native.ptr(levels), min(level, max_len) + 1,
                                             _native.ptr(tgt), _native.ptr(d), n, n_tgt, _native.ptr(paths[lo:lo + n]),
                                             max_len + 1, stream)
                _native.check(code, "lgc_bfs_backtrack")
    _snapshot_status(dev)
    return dist, paths


def hop_distances(graph: PropGraph, sources: Tensor, targets: Tensor, max_hops: Optional[int] = None,
                  trace: Optional[list] = None) -> Tensor:
    """int32 ``[S, T]`` on the device: the hop distance from ``sources[s]`` (int64 ``[S]``) to ``targets[s, t]`` (int64
    ``[S, T]``), any node ids (a user may be a target; source == target gives 0).  -1: no path; -2: not reached within
    ``max_hops`` levels.  Sources run in batches of 64 with one host read (a 32-byte counter block) per level; a batch
    ends when no node is new, no pair is unset or ``max_hops`` levels have run.  Device memory per batch: three words
    per node, whatever S is.  An id outside the graph gives -1 and raises at ``check_index_status()`` (the status word
    is the pair scoring's, and so is the IndexError's wording: it names ``edge_label_index``)."""
    return _search(graph, sources, targets, max_hops, None, trace)[0]


def shortest_paths(graph: PropGraph, sources: Tensor, targets: Tensor, max_len: int = 7, max_hops: Optional[int] = None,
                   workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, trace: Optional[list] = None) -> Tuple[Tensor, Tensor]:
    """``(dist, paths)``: ``hop_distances`` and one shortest path per pair, int64 ``[S, T, max_len + 1]`` on the device:
    ``paths[s, t, :d + 1]`` runs from the source to the target, the rest is -1.  The frontiers of levels 0..max_len are
    kept (``(max_len + 1) * N * 8`` bytes, refused beyond ``workspace_bytes``); a pair farther than ``max_len`` gets its
    distance and an all -1 row, and so does a pair without a path.  Among several shortest paths the walk back takes,
    at every node, the first predecessor in the row's stored entry order: the same path on every run."""
    if max_len < 0:
        raise ValueError("max_len must be >= 0")
    need = (max_len + 1) * graph.num_nodes * 8
    if need > workspace_bytes:
        raise ValueError(f"keeping levels 0..{max_len} of {graph.num_nodes} nodes takes {need} bytes, the workspace is "
                         f"{workspace_bytes} bytes: lower max_len or raise workspace_bytes")
    return _search(graph, sources, targets, max_hops, int(max_len), trace)


def paths_frame(hit_df, dist, paths):
    """The frame upstream's ``compute_paths`` returns, from ``hit_df`` (rows in the order of ``dist`` / ``paths``) and
    the two arrays (tensors or numpy; ``[S, k]`` and ``[S, k, L]``, -1 padded): columns ``path_lens`` (lists of int),
    ``longer_than_3`` (bool) and ``paths`` (lists of lists of node ids), rows sorted with upstream's own
    ``sort_values(by=['path_lens'], ascending=False)``.  Host only.  A pair without a path gives -1 and ``[]`` (upstream
    raises NetworkXNoPath there: the one deviation), and so does a pair whose path was not kept (longer than L - 1)."""
    import numpy as np
    d = dist.cpu().numpy() if torch.is_tensor(dist) else np.asarray(dist)
    p = paths.cpu().numpy() if torch.is_tensor(paths) else np.asarray(paths)
    if d.ndim != 2 or p.ndim != 3 or p.shape[:2] != d.shape or d.shape[0] != len(hit_df):
        raise ValueError(f"{len(hit_df)} rows, dist {d.shape}, paths {p.shape}")
    out = hit_df.copy()
    out['path_lens'] = [[int(x) for x in row] for row in d]
    out['longer_than_3'] = out.path_lens.apply(lambda x: any(i > 3 for i in x)).astype(bool)
    walks: List[list] = [[[int(v) for v in p[r, c, :n + 1]] if 0 <= n < p.shape[2] and p[r, c, n] >= 0 else []
                          for c, n in enumerate(row)] for r, row in enumerate(d)]
    out['paths'] = walks
    return out.sort_values(by=['path_lens'], ascending=False)


def compute_paths(hit_df, graph: PropGraph, workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
    """``InferenceLightGCN.compute_paths(hit_df, graph)`` with the device graph in place of the networkx one:
    ``hit_df`` is upstream's frame (``prepare_hit_df`` has already offset ``top_rlvnt_itm`` by ``n_users``; every row
    lists the same number of items).  Distances first, unbounded; then the paths with ``max_len`` = the largest
    distance found; then ``paths_frame``."""
    dev = graph.device
    sources = torch.tensor([int(u) for u in hit_df.user_id_idx], dtype=torch.int64).to(dev)
    rows = [list(r) for r in hit_df.top_rlvnt_itm]
    k = len(rows[0]) if rows else 0
    if any(len(r) != k for r in rows):
        raise ValueError("every row of top_rlvnt_itm must list the same number of items")
    targets = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), k).to(dev)
    dist = hop_distances(graph, sources, targets)
    max_len = max(int(dist.max().item()), 0) if dist.numel() else 0
    dist, paths = shortest_paths(graph, sources, targets, max_len=max_len, workspace_bytes=workspace_bytes)
    return paths_frame(hit_df, dist, paths)
