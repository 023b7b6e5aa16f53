"""One rank's training step on a partition as a fixed launch sequence -- and, optionally, as replayed HIP graphs.

The reference's loop body (src/train_lightgcn.py:130-147) is ``zero_grad -> forward -> bpr * size + reg -> backward ->
optimizer.step()`` through autograd.  ``partition.partitioned_bpr_loss`` + ``optim.Adam(row_ranges=...)`` keep that shape
on a partition.  At 8 ranks a step's kernels take about 1.3 ms while issuing its ~115 launches from Python takes 2 ms:
the step is bound by the host.  ``PartitionedTrainer`` runs the SAME launches (``partition.step_forward`` /
``step_backward``, ``lgc_adam_step_hp`` over the rows the rank owns) without autograd in between and with every shape
fixed, which makes the step capturable: with ``graphs=True`` the launch sequence is recorded once as HIP graphs --
one per stretch of work BETWEEN two collectives, never a collective inside a capture -- and every later step replays
them around the eager all-reduce calls (``partition.Comm`` is the seam).  What changes from step to step lives in device
buffers the host refreshes before the replay: the batch's ids (3 x B int64) and Adam's six scalars (24 bytes).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _native
from .partition import Comm, GraphCapture, PartitionedPropagator, check_batch, step_backward, step_forward


class _RecordingComm(Comm):
    """``Comm`` that records a step as segments cut at every collective: end the graph being captured, note the
    collective, run it eagerly, begin the next graph.  Handles are indices into ``self.handles`` so that a replay can wait
    for the work the REPLAYED start returned.  ``actions``: ("graph", g) | ("start", tensor, slot) | ("wait", slot) |
    ("reduce", tensor), in launch order."""

    def __init__(self, inner: Comm, device: torch.device):
        super().__init__(inner.world, inner.group)
        self.inner = inner
        self.actions, self.handles = [], []
        self.capture = GraphCapture(device, pool=torch.cuda.graph_pool_handle())

    def record(self, body) -> None:
        """``body()`` as segments; an exception inside it ends the open capture and leaves."""
        with self.capture:
            self.capture.begin()
            body()
            self.actions.append(("graph", self.capture.end()))

    def _cut(self, run, action):
        """Close the graph being captured, run the collective eagerly and note it, open the next graph."""
        self.actions.append(("graph", self.capture.end()))
        result = run()
        self.actions.append(action)
        self.capture.begin()
        return result

    def start(self, block: Tensor):
        slot = len(self.handles)
        self.handles.append(self._cut(lambda: self.inner.start(block), ("start", block, slot)))
        return ("slot", slot)

    def wait(self, handle) -> None:
        if handle is not None:
            self._cut(lambda: self.inner.wait(self.handles[handle[1]]), ("wait", handle[1]))

    def reduce_now(self, t: Tensor) -> None:
        self._cut(lambda: self.inner.reduce_now(t), ("reduce", t))


class PartitionedTrainer:
    """``step(users, pos, neg)`` = one training step of this rank for one GLOBAL batch (every rank is given the same
    ``users, pos, neg``: int64 ``[batch]`` device tensors): forward on the partition, BPR + regulariser of the triples this
    rank owns, seeded backward with the per-hop item-block exchange, Adam over ``pp.owned_row_ranges()``.  Returns a
    device tensor ``[bpr, reg, loss]`` (global values, summed over the ranks; no host sync).  ``weight`` is updated in
    place; its rows other ranks own are never read or written.  Every step bumps ``weight``'s version counter, as an
    in-place optimizer step does, so that caches keyed on it (``LightGCN.recommendK``'s table) see the update.

    ``graphs=True``: the first call records the step (after ``warmup`` eager steps that build every lazy plan and
    scratch buffer), later calls replay it.  Same launches, same order, same bits as the eager step.  ``graphs="full"``:
    the whole step as ONE graph with its collectives inside (RCCL's collectives are capturable; an eager collective costs a
    rank two cross-stream hand-offs, ~12-23 us each, and a step has a dozen) -- only over ``nccl``; if the capture fails on
    any rank, every rank falls back to the segmented recording together (one MIN all-reduce)."""

    def __init__(self, pp: PartitionedPropagator, weight: Tensor, alphas: Sequence[float], lr: float = 0.005,
                 decay: float = 1e-4, batch: int = 1024, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 graphs: bool = False, warmup: int = 2):
        if weight.dtype != torch.float32 or weight.dim() != 2 or not weight.is_contiguous():
            raise TypeError("weight must be a contiguous 2-D fp32 table")
        self.pp, self.w = pp, weight.detach()
        self._caller = weight                      # whose version counter a step bumps (the kernels write through self.w)
        self.alphas = tuple(float(a) for a in alphas)
        self.lr, self.decay, self.batch, self.betas, self.eps = float(lr), float(decay), int(batch), betas, float(eps)
        dev = self.w.device
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.t = 0
        self.ids = torch.zeros((3, self.batch), dtype=torch.int64, device=dev)       # users | pos | neg of the current batch
        self.hyper = torch.zeros(6, dtype=torch.float32, device=dev)                 # lgc_adam_step_hp's scalars
        # staged through a RING of pinned rows: the asynchronous copy of step t reads its row when the stream gets there, so
        # the host may not overwrite it before -- a row is reused only after the copy that read it has completed
        self._ring = 32
        self._hyper_host = torch.zeros((self._ring, 6), dtype=torch.float32)
        self._hyper_done = [None] * self._ring
        if dev.type == "cuda":
            self._hyper_host = self._hyper_host.pin_memory()
        # decided on the ranges every rank holds, not on this rank's own: the ranks refuse together, instead of one rank
        # raising while its peers construct and then wait for it in the first all-reduce
        if any(hi <= lo for lo, hi in pp.ranges):
            raise ValueError("this rank owns no user rows: a partition with more ranks than users cannot train")
        self.stats = torch.zeros(3, dtype=torch.float32, device=dev)
        self.use_graphs = bool(graphs) and dev.type == "cuda"
        self.full_graph = graphs == "full" and self.use_graphs
        self._full = None                          # the whole step as one graph (graphs="full"), once recorded
        self.full_error: Optional[str] = None
        self.warmup = int(warmup)
        self._actions: Optional[list] = None       # _RecordingComm.actions, once recorded
        self._steps_seen = 0

    # -- the step as straight-line code; collectives go through self.pp.comm -----------------------------------
    def _body(self) -> None:
        pp = self.pp
        users, pos, neg = self.ids[0], self.ids[1], self.ids[2]
        local, bpr_local, reg_users, reg_items, saved = step_forward(pp, self.w, self.alphas, users, pos, neg, self.decay)
        grad = step_backward(pp, saved, self.alphas, None, self.decay / self.batch, zero_foreign=False)
        self._adam(grad)
        part = torch.stack([bpr_local, reg_users])
        pp.comm.reduce_now(part)
        self.stats[0] = part[0]
        self.stats[1] = part[1] + reg_items
        self.stats[2] = self.stats[0] + self.stats[1]

    def _adam(self, grad: Tensor) -> None:
        ops = self.pp.ops
        width = self.w.size(1)
        for lo, hi in self.pp.owned_row_ranges():
            if hi > lo:
                ops.adam_rows(self.w, grad, self.m, self.v, lo * width, hi * width, self.hyper)

    def _refresh_hyper(self) -> None:
        self.t += 1
        b1, b2 = self.betas
        slot = self.t % self._ring
        if self._hyper_done[slot] is not None:
            self._hyper_done[slot].synchronize()       # the copy that last read this row (32 steps ago) has completed
        h = self._hyper_host[slot]
        h[0], h[1], h[2], h[3] = 1.0 - b1, b2, 1.0 - b2, self.eps
        h[4] = self.lr / (1.0 - b1 ** self.t)
        h[5] = math.sqrt(1.0 - b2 ** self.t)
        self.hyper.copy_(h, non_blocking=True)
        if self.hyper.is_cuda:
            ev = self._hyper_done[slot] or torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.hyper.device))
            self._hyper_done[slot] = ev

    # -- recording ------------------------------------------------------------------------------------------------
    def _record(self) -> None:
        inner = self.pp.comm
        rec = self.pp.comm = _RecordingComm(inner, self.w.device)
        try:
            rec.record(self._body)
        finally:
            self.pp.comm = inner
        self._actions, self._n_slots = rec.actions, len(rec.handles)

    def _record_full(self) -> bool:
        """The whole step, collectives included, as ONE graph.  Returns whether EVERY rank recorded it (else nothing is kept
        and the caller records the segmented form)."""
        comm = self.pp.comm
        self.full_error = comm.capture_refusal()
        graph = None
        if self.full_error is None:
            graph, _, self.full_error = GraphCapture.capture_one(self.w.device, self._body)
        if comm.agree(graph is not None, self.w.device):
            self._full = graph
        return self._full is not None

    def _replay(self) -> None:
        if self._full is not None:
            self._full.replay()
            return
        comm = self.pp.comm
        handles = [None] * self._n_slots
        for act in self._actions:
            kind = act[0]
            if kind == "graph":
                act[1].replay()
            elif kind == "start":
                handles[act[2]] = comm.start(act[1])
            elif kind == "wait":
                comm.wait(handles[act[1]])
            else:
                comm.reduce_now(act[1])

    # -- public ---------------------------------------------------------------------------------------------------
    def step(self, users: Tensor, pos: Tensor, neg: Tensor) -> Tensor:
        check_batch(self.w, users, pos, neg)
        if users.numel() != self.batch:
            raise ValueError(f"this trainer was built for batches of {self.batch} triples")
        self.ids[0].copy_(users, non_blocking=True)
        self.ids[1].copy_(pos, non_blocking=True)
        self.ids[2].copy_(neg, non_blocking=True)
        self._refresh_hyper()
        with torch.no_grad():
            if not self.use_graphs:
                self._body()
            elif self._actions is not None or self._full is not None:
                self._replay()
            elif self._steps_seen < self.warmup:
                self._body()                       # eager: builds every lazy work plan and scratch buffer first
            else:
                if not (self.full_graph and self._record_full()):
                    self._record()                 # the recording run IS this step (captured work does not execute ...
                self._replay()                     # ... so it is replayed once right away)
        # lgc_adam_step_hp writes the table where autograd's version counter cannot see it: bump it as optim.Adam does
        # (host bookkeeping only, after any capture has ended)
        torch.autograd.graph.increment_version(self._caller)
        self._steps_seen += 1
        return self.stats

    @property
    def graph_launches(self) -> int:
        if self._full is not None:
            return 1
        return 0 if self._actions is None else sum(1 for a in self._actions if a[0] == "graph")
