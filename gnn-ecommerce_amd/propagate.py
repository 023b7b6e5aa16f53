"""Differentiable propagation on the HIP kernels.

``propagate_sum`` computes what src/lightgcn.py:91-99 computes,

    out = sum_{l=0..K} alpha_l * A^l x0 ,

but in Horner form  h_K = alpha_K x0,  h_l = alpha_l x0 + A h_{l+1},  out = h_0 :
K sparse hops, each with the layer-sum folded into its epilogue (``y = a*(A x) + b*x0``).
Compared with "propagate, then axpy into a running sum" this removes the K read-modify-write
sweeps of the [N, D] accumulator -- per hop the only traffic beyond the SpMM
itself is one read of x0's row.  The value is the same polynomial in A; only the association of
the fp32 additions differs from the reference (covered by the norm-wise 1e-5 parity gate).

The operator is linear in x0, so the backward pass is the same routine on A^T and needs no
saved activations:  d out / d x0 = sum_l alpha_l (A^T)^l.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _native
from .graph import Operator, PropGraph, apply_rows


# bench.py sets this to a list to receive one (start, end) pair of events per hop, recorded on the
# stream the kernels are launched on; None (the default) records nothing.
HOP_EVENT_LOG: Optional[list] = None


def _timed_apply(op: Operator, x: Tensor, out: Tensor, **kw) -> None:
    if HOP_EVENT_LOG is None:
        op.apply(x, out, **kw)
        return
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    op.apply(x, out, **kw)
    end.record()
    HOP_EVENT_LOG.append((start, end))


def scratch_table(like: Tensor) -> Tensor:
    """An internal [N, D] table.  Rows are padded to a multiple of 32 floats (128 B, one cache line) when D
    is not one already (D = 90 -> stride 96), so that every gathered row covers whole lines: a 360-byte
    row at stride 360 straddles 3.8 lines on average, at stride 384 exactly 3.  Only the API-facing
    tables (embedding.weight in, the result out) keep the caller's dense layout."""
    n, d = like.shape
    if PAD_INTERNAL and d % 32 != 0:
        stride = (d + 31) // 32 * 32
        return torch.empty((n, stride), dtype=like.dtype, device=like.device)[:, :d]
    return torch.empty_like(like)


PAD_INTERNAL = os.environ.get("LGCN_PAD_INTERNAL", "1") == "1"


def horner_hops(op: Operator, x0: Tensor, alphas: Sequence[float]) -> Tensor:
    """sum_l alphas[l] * op^l x0 with len(alphas)-1 launches of ``op.apply``."""
    k = len(alphas) - 1
    if k == 0:
        return x0 * alphas[0]
    x0 = x0.contiguous()
    h = torch.empty_like(x0) if k == 1 else scratch_table(x0)
    # first hop reads x0 directly:  h_{K-1} = alpha_K * (A x0) + alpha_{K-1} * x0
    _timed_apply(op, x0, h, a=alphas[k], r=x0, b=alphas[k - 1])
    for layer in range(k - 2, -1, -1):
        nxt = torch.empty_like(x0) if layer == 0 else scratch_table(x0)
        _timed_apply(op, h, nxt, a=1.0, r=x0, b=alphas[layer])
        h = nxt
    return h


USE_BIPARTITE = os.environ.get("LGCN_BIPARTITE", "1") == "1"

class _HopSpan:
    """Events around one layer's launches (both halves), appended to HOP_EVENT_LOG when bench.py asks."""

    def __enter__(self):
        self.log = HOP_EVENT_LOG
        if self.log is not None:
            self.start, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.start.record()
        return self

    def __exit__(self, *exc):
        if self.log is not None:
            self.end.record()
            self.log.append((self.start, self.end))


def bipartite_sum(user_op: Operator, item_op: Operator, split: int, x0: Tensor, alphas: Sequence[float],
                  final_rows: Optional[Tensor] = None, reduced=None) -> Tensor:
    """sum_l alpha_l A^l x0 for A = [[0, R], [R^T, 0]] (users first), K = len(alphas) - 1 layers.

    With x_l = A^l x0:  x_l[items] = R^T x_{l-1}[users]  (item step, gathers user rows) and
    x_l[users] = R x_{l-1}[items]  (user step, gathers item rows).  Because the user side is linear in the
    item tables,
        out[users] = alpha_0 x0[users] + R ( sum_{l=1..K} alpha_l x_{l-1}[items] ),
    so the K-th user table is never materialised, only ONE user step (the last) reads an epilogue row,
    and the weighted sums over layers are taken on the small item tables only (``lgc_lincomb``, in the
    reference's own order: out = out + x * alpha).  Same K item steps + K user steps as K plain hops.

    With equal alphas, K = 2 or 3 and a band-sweep item step, that sum has no launch of its own either: the item step of
    layer K - 1 writes  mix = (alpha_{K-2} x_{K-3} + alpha_{K-1} x_{K-2}) + alpha_K x_{K-1}  over the item rows into the
    block where x_{K-1}[items] would go -- nothing else reads that block -- with the prior terms as epilogue rows
    (``Operator.apply(..., r2=, b2=)``, lgc_apply2), in lgc_lincomb's association: the same bits, one launch, one write
    and one read of the block less (``mix_in_item_step`` below; LGCN_MIX_IN_ITEM_STEP=0 keeps the lgc_lincomb).

    ``final_rows`` (int64 node ids on the device, users and items alike): the caller will only ever read these rows of the
    result -- a training step scores 2B label pairs (src/lightgcn.py:123-125).  The LAST user step, whose 1.6 M output rows
    nothing else consumes, is then computed for the listed user rows only (``lgc_spmm_rows``: a few thousand gathers, the
    same bits for rows of up to 32 entries), and the LAST item step -- otherwise a full sweep over the user table -- for the
    listed item rows only (``lgc_spmm_rows_split``; SCORED_ITEM_ROWS_ONLY); every other row of the result is left
    uninitialised.

    ``reduced`` (``PropGraph.reduced()``, K >= 2): the middle user tables x_1 .. x_{K-1}[users] are consumed by the next
    layer's item step only, so the users L with few entries never get a row there.  With H the kept users and
    G_L = R_L^T R_L,   x_l[items] = R_H^T x_{l-1}[H] + G_L x_{l-2}[items]   for l >= 2.  The tables stay allocated as
    without it and the reduced operators work on the views t[offset:] (kept user h = row h, item i = row n_h + i = row
    split + i of t), so full and reduced operators address the same item blocks and only the tail of a middle table is
    ever touched.  Layer 1's item step, the last user step and both listed-rows launches are the full operators,
    unchanged; with listed item rows the user step of layer K - 1 is the full one too, because that launch gathers every
    user row.

    Order of the additions of an item row, fixed from run to run.  With the concatenated operator
    (``reduced.concat_for``, LGCN_REDUCED_CONCAT) the item step of a reduced layer is ONE apply of
    [R_H^T | G_L]: the row is  a * (sum over its pieces, the entries of G_L among them, each at its gap column's place in
    the band walk) + r,  with r = ``mix`` in the last layer of the uniform-alpha shortcut and no epilogue row otherwise --
    one sweep and one combine.  The entries of G_L gather x_{l-2}[items] from the gaps of table l-1, which the user step
    of layer l-1 filled through its one-entry gap rows (bit-identical copies).  Without it (switch off, G_L empty, fewer
    eliminated users than gap rows, or a width "auto" leaves out):  (a * G_L x (+ mix)) + a * sweep sum -- the G_L launch
    writes the row, the kept users' item step adds its sum to it (r = the row itself, b = 1: each lane reads the elements
    it then writes).  The two orders differ in the last bits, both inside the 1e-5 gate.
    """
    k = len(alphas) - 1
    if k == 0:
        return x0 * alphas[0]
    x0 = x0.contiguous()
    n = x0.size(0)
    tables = [x0]                                     # x_0 .. x_K (x_K: item rows only)
    red = reduced if k >= 2 else None
    rows_items_only = final_rows is not None and SCORED_ITEM_ROWS_ONLY and item_op.listed_rows_pay(final_rows.numel()) \
        if red is not None else False

    # the scratch tables' geometry decides (as Operator.apply will): rows of the full table, row stride of scratch_table
    cc = red.concat_for(x0.size(1), n, x0.size(1) if (not PAD_INTERNAL or x0.size(1) % 32 == 0)
                        else (x0.size(1) + 31) // 32 * 32) if red is not None else None

    def user_step(layer: int, x: Tensor, out_t: Tensor) -> None:
        """x_layer[users] for a middle layer: the kept users only, unless the next launch reads every user row."""
        if red is None or (rows_items_only and layer == k - 1):
            user_op.apply(x, out_t)
        elif cc is not None:                              # ... and x_{layer-1}[items] into the gaps of out_t
            cc.user_op.apply(x[cc.offset:], out_t[cc.offset:])
        elif red.user_op_h is not None:
            red.user_op_h.apply(x[red.offset:], out_t[red.offset:])

    def item_step(layer: int, out_t: Tensor, a: float = 1.0, r: Optional[Tensor] = None) -> None:
        """out_t[items] = a * x_layer[items] (+ r[items]) for layer >= 2 on the reduced operators."""
        if cc is not None:
            o = cc.offset
            cc.item_op.apply(tables[layer - 1][o:], out_t[o:], a=a, r=None if r is None else r[o:], b=0.0 if r is None else 1.0)
            return
        o = red.offset
        y = out_t[o:]
        have = r is not None
        if red.gram_op is not None:
            red.gram_op.apply(tables[layer - 2][o:], y, a=a, r=r[o:] if have else None, b=1.0 if have else 0.0)
        elif have:
            _native.lincomb(out_t[split:], [(1.0, r[split:])])
        else:
            out_t[split:].zero_()
        if red.item_op_h is not None:
            red.item_op_h.apply(tables[layer - 1][o:], y, a=a, r=y, b=1.0)
    # The reference's alpha is 1 / (K + 1) for every layer (src/lightgcn.py:75-79).  Then sum_{l<K} alpha_l x_l[items] IS
    # the table the last user step gathers, so the last item step adds it as its epilogue row and writes the item block
    # of the result directly: one lgc_lincomb and the K-th item table less, the same sums in the same order
    # (((a x_0 + a x_1) + a x_2) + a x_3).
    # (only when a result row is whole cache lines: the combine's stores into 360-byte rows cost more than the lincomb saves,
    # 4.67 vs 4.65 ms per K=5, D=90 step; 1.607 vs 1.623 ms at K=3, D=64)
    uniform = UNIFORM_ALPHA_SHORTCUT and all(a == alphas[0] for a in alphas) and (UNIFORM_ALPHA_SHORTCUT == "force" or x0.size(1) % 32 == 0)

    def mix_in_item_step(out_t: Tensor) -> bool:
        """Layer K-1's item step writes mix = sum_{l=1..K} alpha_l x_{l-1}[items] where x_{K-1}[items] would go
        (LGCN_MIX_IN_ITEM_STEP): that block has no other reader -- the user step of layer K-1 gathers table K-2, layer K's
        item step gathers table K-1 below ``split`` only (user rows and gaps) and x_{K-2}[items] from the gaps or from
        table K-2 (gram_op) -- so the lgc_lincomb of the last layer, its write and its read of the block go away.  The
        prior terms ride as epilogue rows in lgc_lincomb's association, ((a_1 x_0 + a_2 x_1) + a_3 x_2): the same bits.
        One or two prior terms (K = 2, 3) and a band-sweep item step only; False = nothing launched, today's path."""
        if not (MIX_IN_ITEM_STEP and uniform and final_rows is None and k in (2, 3)):
            return False
        if red is None or k == 2:
            op, o = item_op, 0                                                  # layer 1 is always the full operator
        elif cc is not None:
            op, o = cc.item_op, cc.offset
        else:
            return False                                                        # G_L as a separate launch: unchanged
        x = tables[k - 2][o:]                               # x_{K-2}: its user rows are gathered, its item rows are r
        if not op.takes_second_row(x, out_t[o:], x):
            return False
        assert op.sweep_cols is not None and o + op.sweep_cols[1] <= split      # the item steps gather no item row
        if k == 2:
            op.apply(x, out_t[o:], a=alphas[2], r=x, b=alphas[1])
        else:
            op.apply(x, out_t[o:], a=alphas[3], r=x, b=alphas[2], r2=tables[0][o:], b2=alphas[1])
        return True

    mixed = False
    for layer in range(1, k + 1):
        with _HopSpan():
            nxt = None if mixed else scratch_table(x0)
            if layer < k:
                if layer == k - 1 and mix_in_item_step(nxt):
                    mixed = True                                                # nxt[items] = mix, not x_l[items]
                elif red is None or layer == 1:
                    item_op.apply(tables[-1], nxt)                              # x_l[items]
                else:
                    item_step(layer, nxt)
                user_step(layer, tables[-1], nxt)                               # x_l[users]
                tables.append(nxt)
            else:
                out = torch.empty_like(x0)
                rows_only = final_rows is not None
                if rows_only and SCORED_ITEM_ROWS_ONLY and item_op.listed_rows_pay(final_rows.numel()):
                    # the scores read the item block at the batch's item rows only: the last item step -- a full sweep over
                    # the 420 MB user table otherwise -- is computed for the listed rows (lgc_spmm_rows_split: the rows cut
                    # into chunks on the device), on top of rest = sum_{l<K} alpha_l x_l[items]
                    mix = nxt
                    _native.lincomb(mix[split:], [(alphas[l], tables[l - 1][split:]) for l in range(1, k + 1)])
                    if all(a == alphas[0] for a in alphas):
                        rest = mix                                              # the same table when the alphas are equal
                    else:
                        rest = scratch_table(x0)
                        _native.lincomb(rest[split:], [(alphas[l], tables[l][split:]) for l in range(0, k)])
                    apply_rows(item_op, final_rows, tables[-1], out, a=alphas[k], r=rest, b=1.0, split=True)
                elif uniform:
                    if mixed:
                        mix = tables[-1]                                        # written by layer K-1's item step
                    else:
                        mix = nxt                                               # item rows: sum_l alpha_l x_{l-1}
                        _native.lincomb(mix[split:], [(alphas[l], tables[l - 1][split:]) for l in range(1, k + 1)])
                    if red is None:
                        item_op.apply(tables[-1], out, a=alphas[k], r=mix, b=1.0)   # out[items] = mix + alpha_K x_K[items]
                    else:
                        item_step(k, out, a=alphas[k], r=mix)
                else:
                    if red is None:
                        item_op.apply(tables[-1], nxt)                          # x_K[items]
                    else:
                        item_step(k, nxt)
                    tables.append(nxt)
                    mix = scratch_table(x0)
                    _native.lincomb(mix[split:], [(alphas[l], tables[l - 1][split:]) for l in range(1, k + 1)])
                    _native.lincomb(out[split:], [(alphas[l], tables[l][split:]) for l in range(0, k + 1)])
                if not rows_only:
                    user_op.apply(mix, out, a=1.0, r=x0, b=alphas[0])            # out[users]
                else:
                    apply_rows(user_op, final_rows, mix, out, a=1.0, r=x0, b=alphas[0])
    return out


def _layer_sum(graph: PropGraph, x: Tensor, alphas: tuple, transpose: bool, final_rows: Optional[Tensor] = None) -> Tensor:
    if USE_BIPARTITE and graph.split is not None and len(alphas) - 1 <= _native.MAX_TERMS - 1:
        user_op, item_op = graph.halves(transpose)
        return bipartite_sum(user_op, item_op, graph.split, x, alphas, final_rows if SCORED_ROWS_ONLY else None,
                             reduced=graph.reduced(transpose) if len(alphas) > 2 else None)
    return horner_hops(graph.transpose_op if transpose else graph.forward_op, x, alphas)


# ... and the item step before it writes the layer sum the last user step gathers (bipartite_sum.mix_in_item_step,
# lgc_apply2); "0": that sum as a lgc_lincomb of its own in the last layer
MIX_IN_ITEM_STEP = os.environ.get("LGCN_MIX_IN_ITEM_STEP", "1") == "1"
# equal alphas: the last item step writes the result's item block itself (bipartite_sum); "0" keeps the two lincombs
UNIFORM_ALPHA_SHORTCUT ={"0": False, "force": "force"}.get(os.environ.get("LGCN_UNIFORM_ALPHA_SHORTCUT", "1"), True)
# the forward of a scoring step computes the last user step only for the rows its label pairs name (bipartite_sum)
SCORED_ROWS_ONLY = os.environ.get("LGCN_SCORED_ROWS_ONLY", "1") == "1"
# ... and the last ITEM step as well (lgc_spmm_rows_split); "0": the full item step, as get_embedding runs it
SCORED_ITEM_ROWS_ONLY = os.environ.get("LGCN_SCORED_ITEM_ROWS_ONLY", "1") == "1"


class _PropagateSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0: Tensor, graph: PropGraph, alphas: tuple) -> Tensor:
        ctx.graph, ctx.alphas = graph, alphas
        return _layer_sum(graph, x0.detach(), alphas, transpose=False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        return _layer_sum(ctx.graph, grad_out.contiguous(), ctx.alphas, transpose=True), None, None


class _Hop(torch.autograd.Function):
    """One LGConv hop y = A x (the operator surface of src/lightgcn.py:96)."""

    @staticmethod
    def forward(ctx, x: Tensor, graph: PropGraph) -> Tensor:
        ctx.graph = graph
        x = x.detach().contiguous()
        return graph.forward_op.apply(x, torch.empty_like(x))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        g = grad_out.contiguous()
        return ctx.graph.transpose_op.apply(g, torch.empty_like(g)), None


def propagate_sum(x0: Tensor, graph: PropGraph, alphas: Sequence[float]) -> Tensor:
    _native.require_device(x0, "embedding table")
    return _PropagateSum.apply(x0, graph, tuple(float(a) for a in alphas))


def hop(x: Tensor, graph: PropGraph) -> Tensor:
    _native.require_device(x, "x")
    return _Hop.apply(x, graph)


# ----------------------------------------------------------------------------------------
# pair scoring
# ----------------------------------------------------------------------------------------
_status_words = {}


def _status(device: torch.device) -> Tensor:
    t = _status_words.get(device)
    if t is None:
        t = torch.zeros(4, dtype=torch.int32, device=device)
        _status_words[device] = t
    return t


_status_snapshots = {}


def _snapshot_status(device: torch.device) -> None:
    """Enqueue an asynchronous copy of the status word to pinned host memory (after a scoring launch); the next
    scoring call looks at it without waiting.  Not while a HIP graph is being captured (trainer.PartitionedTrainer): the
    status word itself is still written by the replayed launches and read by ``check_index_status()``."""
    if torch.cuda.is_current_stream_capturing():
        return
    snap = _status_snapshots.get(device)
    if snap is None:
        snap = (torch.zeros(4, dtype=torch.int32).pin_memory(), torch.cuda.Event())
        _status_snapshots[device] = snap
    snap[0].copy_(_status(device), non_blocking=True)
    snap[1].record(torch.cuda.current_stream(device))


def raise_pending_index_error(device: torch.device) -> None:
    """Non-blocking: if an EARLIER scoring launch on this device has finished and flagged an out-of-range label
    index, raise IndexError now (the reference's gather raises at the faulty call; here the kernels never fault and
    the error surfaces at the next call, or at ``check_index_status()``)."""
    snap = _status_snapshots.get(device)
    if snap is not None and snap[1].query() and int(snap[0][0]) & _native.ST_INDEX_OOB:
        snap[0].zero_()
        _status(device).zero_()
        raise IndexError("edge_label_index of an earlier call contained node ids outside [0, num_nodes)")


def check_index_status(device: Optional[torch.device] = None) -> None:
    """Synchronising check: raise IndexError if any pair-scoring launch since the last check saw an
    out-of-range label index (the kernels skip such pairs and score them NaN instead of faulting)."""
    for dev, t in list(_status_words.items()):
        if device is not None and dev != device:
            continue
        if int(t[0].item()) & _native.ST_INDEX_OOB:
            t.zero_()
            snap = _status_snapshots.get(dev)
            if snap is not None:
                snap[1].synchronize()
                snap[0].zero_()
            raise IndexError("edge_label_index contains node ids outside [0, num_nodes)")


class _PairDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb: Tensor, idx0: Tensor, idx1: Tensor) -> Tensor:
        lib = _native.load()
        emb_c = emb.detach().contiguous()
        idx0, idx1 = idx0.contiguous(), idx1.contiguous()
        scores = torch.empty(idx0.numel(), dtype=torch.float32, device=emb.device)
        with torch.cuda.device(emb.device):
            code = lib.lgc_pair_dot(_native.ptr(emb_c), emb_c.stride(0), emb_c.size(1), emb_c.size(0),
                                    _native.ptr(idx0), _native.ptr(idx1), idx0.numel(), _native.ptr(scores),
                                    _native.ptr(_status(emb.device)), _native.stream_of(emb.device))
        _native.check(code, "lgc_pair_dot")
        _snapshot_status(emb.device)
        ctx.save_for_backward(emb_c, idx0, idx1)
        return scores

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores: Tensor):
        emb, idx0, idx1 = ctx.saved_tensors
        n = emb.size(0)
        ok = (idx0 >= 0) & (idx0 < n) & (idx1 >= 0) & (idx1 < n)       # invalid pairs scored NaN and carry no gradient
        i0, i1 = idx0.clamp(0, n - 1), idx1.clamp(0, n - 1)
        gs = torch.where(ok, grad_scores, torch.zeros_like(grad_scores)).unsqueeze(1)
        rows = torch.cat([i0, i1])
        vals = torch.cat([gs * emb[i1], gs * emb[i0]])                   # d score / d emb[i0] = emb[i1] and the reverse
        grad = torch.zeros_like(emb)
        rows_s, perm = torch.sort(rows, stable=True)                     # repeated nodes add up in position order
        segment_sum(rows_s, rows_s, vals[perm].contiguous(), grad)
        return grad, None, None


def segment_sum(key_sorted: Tensor, dest: Tensor, vals: Tensor, out: Tensor, scale: float = 1.0, accumulate: bool = False,
                vals_index: Optional[Tensor] = None) -> None:
    """out[dest[t]] (+)= scale * (sum of vals over the run of equal keys that starts at t), for every run head t with
    dest[t] >= 0: lgc_segment_sum -- one lane group per destination row, fixed order, no atomics.  ``vals_index`` (int32):
    the value row of sorted position t is vals[vals_index[t]] (the permutation of the sort; vals stays unsorted)."""
    lib = _native.load()
    _native.require_device(out, "segment_sum: out")
    if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1:
        raise TypeError("segment_sum: out must be a 2-D fp32 tensor with unit inner stride")
    m = key_sorted.numel()
    for name, t in (("key_sorted", key_sorted), ("dest", dest)):
        # raw pointers go to the kernel: a host tensor or int32 data read as int64 would be a GPU fault or garbage keys
        if t.dtype != torch.int64 or t.dim() != 1 or t.numel() != m or not t.is_contiguous() or t.device != out.device:
            raise TypeError(f"segment_sum: {name} must be a contiguous int64 vector of {m} entries on {out.device}, got "
                            f"{t.dtype} {tuple(t.shape)} on {t.device}")
    if (vals.dtype != torch.float32 or vals.dim() != 2 or vals.shape != (m, out.size(1)) or not vals.is_contiguous()
            or vals.device != out.device):
        raise TypeError(f"segment_sum: vals must be a contiguous fp32 [{m}, {out.size(1)}] tensor on {out.device}, got "
                        f"{vals.dtype} {tuple(vals.shape)} on {vals.device}")
    if vals_index is not None and (vals_index.dtype != torch.int32 or vals_index.shape != (m,) or not vals_index.is_contiguous()
                                   or vals_index.device != out.device):
        raise TypeError(f"segment_sum: vals_index must be a contiguous int32 vector of {m} entries on {out.device}")
    with torch.cuda.device(out.device):
        code = lib.lgc_segment_sum(_native.ptr(key_sorted), _native.ptr(dest), _native.ptr(vals), _native.ptr(vals_index),
                                   key_sorted.numel(), float(scale),
                                   _native.ptr(out), out.stride(0), out.size(0), out.size(1), int(accumulate),
                                   _native.stream_of(out.device))
    _native.check(code, "lgc_segment_sum")


# ----------------------------------------------------------------------------------------
# scores straight from the weight table: forward = propagate + pair scoring, backward seeded
# ----------------------------------------------------------------------------------------
SPARSE_BACKWARD = os.environ.get("LGCN_SPARSE_BACKWARD", "1") == "1"
# the seeded backward is used when the table has at least this many rows per possible seed row (2 per label pair)
SEED_ROWS_FACTOR = int(os.environ.get("LGCN_SEED_ROWS_FACTOR", "32"))


def _seed_pull(op: Operator, flag: Tensor, slot: Tensor, seed_vals: Tensor, out: Tensor, mark: Optional[Tensor] = None) -> None:
    """out[rows of op] = sum over the entries whose column carries a flag of val * seed_vals[slot[col]] (lgc_seed_pull):
    the rows of ``op`` through its row / chunk plan in lgc_spmm's fixed order; rows whose ``mark`` byte is 0 are written
    as zeros without being read."""
    lib = _native.load()
    p = op.plan
    stream = _native.stream_of(out.device)          # read once: the partial rows' owner and the launches' stream
    partials = op.partials(out.size(1), _native.scratch_owner(out.device, stream))
    with torch.cuda.device(out.device):
        code = lib.lgc_seed_pull(_native.ptr(op.rowptr), _native.ptr(op.entries), p.row_begin, p.row_end, p.short_max,
                                 _native.ptr(p.chunks) if p.n_chunks else None, p.n_chunks,
                                 _native.ptr(p.multi) if p.n_multi else None, p.n_multi, _native.ptr(partials),
                                 _native.ptr(flag), _native.ptr(slot), _native.ptr(mark), _native.ptr(seed_vals),
                                 seed_vals.stride(0), out.size(0), _native.ptr(out), out.stride(0), out.size(1), stream)
    _native.check(code, "lgc_seed_pull")


def _seed_mark(op: Operator, rows_sorted: Tensor, mark: Tensor, value: int) -> None:
    """mark[col] = value for every column of the rows of ``op`` listed in ``rows_sorted`` (lgc_seed_mark)."""
    lib = _native.load()
    p = op.plan
    with torch.cuda.device(mark.device):
        code = lib.lgc_seed_mark(_native.ptr(op.rowptr), _native.ptr(op.entries), p.row_begin, p.row_end, _native.ptr(rows_sorted),
                                 rows_sorted.numel(), _native.ptr(mark), mark.numel(), int(value), _native.stream_of(mark.device))
    _native.check(code, "lgc_seed_mark")


_seed_maps = {}


def _scratch_key(device: torch.device):
    """Scratch that must be all zero between uses is owned by one (device, stream, host thread) triple: the set / pull /
    clear sequence of a backward pass is ordered on ITS stream and issued by ITS thread only, so two backward passes on
    different streams or threads (two models, a DataParallel-style host loop, the thread-ranks of
    tests/test_partition_gpu.py) each get their own buffers instead of reading or clearing each other's flags.
    ``_native.scratch_owner``: the same key owns the hop's partial rows (graph.py) and the score panel."""
    return _native.scratch_owner(device)


def _seed_map_buffers(device: torch.device, n_cols: int):
    """Per (device, stream): a byte flag and an int32 slot per column, flags all zero between uses (the pull reads a
    slot only where the flag is set; the flags of a step's seeds are cleared again right after the pull)."""
    key = _scratch_key(device)
    got = _seed_maps.get(key)
    if got is None or got[0].numel() < n_cols + 1:
        got = (torch.zeros(n_cols + 1, dtype=torch.uint8, device=device), torch.empty(n_cols + 1, dtype=torch.int32, device=device))
        _seed_maps[key] = got
    return got


_seed_marks = {}
# item rows without a seed user among their columns are written as zeros unread (lgc_seed_mark); "0" reads every row
SEED_MARKS = os.environ.get("LGCN_SEED_MARKS", "1") == "1"


def _seed_mark_buffer(device: torch.device, n_rows: int) -> Tensor:
    """Per (device, stream): one byte per table row, all zero between uses."""
    key = _scratch_key(device)
    got = _seed_marks.get(key)
    if got is None or got.numel() < n_rows:
        got = torch.zeros(n_rows, dtype=torch.uint8, device=device)
        _seed_marks[key] = got
    return got


class DeviceOps:
    """The launches the seeded backward and the partitioned path are written against: one method = one (or a few)
    launches through the C ABI on the current stream.  ``partition.HipOps`` is this plus the graph builders; the CPU ranks
    of tests/test_partition_gloo.py substitute a test double with the same methods (tests/cpu_ops.py) -- the product
    ships this implementation only."""

    def apply(self, op: Operator, x: Tensor, out: Tensor, a: float = 1.0, r: Optional[Tensor] = None, b: float = 0.0) -> None:
        op.apply(x, out, a=a, r=r, b=b)

    def apply_rows(self, op: Operator, rows: Tensor, x: Tensor, out: Tensor, a: float = 1.0, r: Optional[Tensor] = None,
                   b: float = 0.0, split: bool = False, compact: bool = False) -> None:
        apply_rows(op, rows, x, out, a=a, r=r, b=b, split=split, compact=compact)

    def lincomb(self, y: Tensor, terms) -> None:
        _native.lincomb(y, terms)

    def segment_sum(self, key_sorted: Tensor, dest: Tensor, vals: Tensor, out: Tensor, scale: float = 1.0,
                    accumulate: bool = False, vals_index: Optional[Tensor] = None) -> None:
        segment_sum(key_sorted, dest, vals, out, scale=scale, accumulate=accumulate, vals_index=vals_index)

    def seed_pull(self, op: Operator, flag: Tensor, slot: Tensor, seed_vals: Tensor, out: Tensor, mark: Optional[Tensor]) -> None:
        _seed_pull(op, flag, slot, seed_vals, out, mark)

    def seed_prepare(self, rows: Tensor, split: int, n: int, flag: Optional[Tensor] = None, slot: Optional[Tensor] = None):
        """Sort the seed's row ids and derive the destination lists of its segment sums (lgc_seed_prepare, one launch):
        (rows_sorted, perm int32, dest_item, dest_slot, dest_user) -- see include/lgconv_hip.h.  With ``flag`` / ``slot``:
        the column map of the seeded pull is set for the user heads as well.  Seeds above LGC_SEED_MAX ids take the same
        steps as torch ops."""
        m = rows.numel()
        dev = rows.device
        if m > _native.SEED_MAX:
            return seed_prepare_reference(rows, split, n, flag, slot)
        rows = rows.contiguous()
        i64 = dict(dtype=torch.int64, device=dev)
        buf = torch.empty((5, max(m, 1)), **i64)               # four outputs + the sorted keys in between the two launches
        perm = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        lib = _native.load()
        with torch.cuda.device(dev):
            code = lib.lgc_seed_prepare(_native.ptr(rows), m, int(split), int(n), _native.ptr(buf[0]), _native.ptr(perm),
                                        _native.ptr(buf[1]), _native.ptr(buf[2]), _native.ptr(buf[3]), _native.ptr(flag),
                                        _native.ptr(slot), _native.ptr(buf[4]), _native.stream_of(dev))
        _native.check(code, "lgc_seed_prepare")
        return buf[0, :m], perm[:m], buf[1, :m], buf[2, :m], buf[3, :m]

    def seed_flags(self, rows_sorted: Tensor, split: int, flag: Tensor, value: int) -> None:
        lib = _native.load()
        with torch.cuda.device(flag.device):
            code = lib.lgc_seed_flags(_native.ptr(rows_sorted), rows_sorted.numel(), int(split), _native.ptr(flag), int(value),
                                      _native.stream_of(flag.device))
        _native.check(code, "lgc_seed_flags")

    def pair_scores_rows(self, emb: Tensor, idx0: Tensor, idx1: Tensor):
        """(scores [M], rows0 [M, D], rows1 [M, D], ok uint8 [M]): lgc_pair_dot_rows -- the scores of src/lightgcn.py:123-125
        and, in the same launch, the gathered rows and validity bytes its backward needs."""
        lib = _native.load()
        m, dim, dev = idx0.numel(), emb.size(1), emb.device
        scores = torch.empty(m, dtype=torch.float32, device=dev)
        rows = torch.empty((2, m, dim), dtype=torch.float32, device=dev)
        ok = torch.empty(m, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            code = lib.lgc_pair_dot_rows(_native.ptr(emb), emb.stride(0), dim, emb.size(0), _native.ptr(idx0), _native.ptr(idx1), m,
                                         _native.ptr(scores), _native.ptr(rows[0]), _native.ptr(rows[1]), _native.ptr(ok),
                                         _native.ptr(_status(dev)), _native.stream_of(dev))
        _native.check(code, "lgc_pair_dot_rows")
        _snapshot_status(dev)
        return scores, rows[0], rows[1], ok

    def pair_seed_vals(self, grad_scores: Tensor, mask: Optional[Tensor], grad_scale: Optional[Tensor], rows0: Tensor,
                       rows1: Tensor) -> Tensor:
        """vals [2M, D]: vals[m] = g_m rows1[m], vals[M + m] = g_m rows0[m], g_m = mask[m] ? grad_scores[m] * grad_scale : 0
        (lgc_pair_seed_vals; ``grad_scale`` a 0-dim device tensor or None)."""
        lib = _native.load()
        m, dim, dev = rows0.size(0), rows0.size(1), rows0.device
        grad_scores = grad_scores.contiguous()
        vals = torch.empty((2 * m, dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            code = lib.lgc_pair_seed_vals(_native.ptr(grad_scores), _native.ptr(mask), _native.ptr(grad_scale), _native.ptr(rows0),
                                          _native.ptr(rows1), m, dim, _native.ptr(vals), _native.stream_of(dev))
        _native.check(code, "lgc_pair_seed_vals")
        return vals

    def bpr_loss(self, scores: Tensor, mask: Optional[Tensor], size: int):
        """(loss 0-dim, grad [2B]): lgc_bpr_loss on scores = [pos | neg]."""
        lib = _native.load()
        dev = scores.device
        b = scores.numel() // 2
        out = torch.empty(1 + 2 * b, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            code = lib.lgc_bpr_loss(_native.ptr(scores), _native.ptr(mask), b, int(size), _native.ptr(out), _native.ptr(out[1:]),
                                    _native.stream_of(dev))
        _native.check(code, "lgc_bpr_loss")
        return out[0], out[1:]

    def reg_rows(self, w: Tensor, lists: Sequence[Tensor], scale: float):
        """(value 0-dim, rows int64 [sum of lengths]): lgc_reg_rows -- scale * sum over the three id lists of |w[ids]|_F^2 and
        the ids as row numbers (negative ids wrapped, out-of-range ones -1 and reported through the index status)."""
        lib = _native.load()
        dev = w.device
        a, b, c = lists
        value = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty(a.numel() + b.numel() + c.numel(), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            code = lib.lgc_reg_rows(_native.ptr(w), w.stride(0), w.size(1), w.size(0), _native.ptr(a), a.numel(), _native.ptr(b),
                                    b.numel(), _native.ptr(c), c.numel(), float(scale), _native.ptr(value), _native.ptr(rows),
                                    _native.ptr(_status(dev)), _native.stream_of(dev))
        _native.check(code, "lgc_reg_rows")
        return value[0], rows

    def seed_mark(self, op: Operator, rows_sorted: Tensor, mark: Tensor, value: int) -> None:
        _seed_mark(op, rows_sorted, mark, value)

    def pair_scores(self, emb: Tensor, idx0: Tensor, idx1: Tensor) -> Tensor:
        """scores[m] = <emb[idx0[m]], emb[idx1[m]]> (lgc_pair_dot; out-of-range pairs score NaN and raise later)."""
        lib = _native.load()
        scores = torch.empty(idx0.numel(), dtype=torch.float32, device=emb.device)
        with torch.cuda.device(emb.device):
            code = lib.lgc_pair_dot(_native.ptr(emb), emb.stride(0), emb.size(1), emb.size(0), _native.ptr(idx0),
                                    _native.ptr(idx1), idx0.numel(), _native.ptr(scores), _native.ptr(_status(emb.device)),
                                    _native.stream_of(emb.device))
        _native.check(code, "lgc_pair_dot")
        _snapshot_status(emb.device)
        return scores

    def scratch_table(self, like: Tensor) -> Tensor:
        return scratch_table(like)

    def adam_rows(self, w: Tensor, g: Tensor, m: Tensor, v: Tensor, lo: int, hi: int, hyper: Tensor) -> None:
        """One Adam step over the flat element range [lo, hi) of four same-shaped contiguous fp32 tables, the six scalars
        read from the device tensor ``hyper`` (lgc_adam_step_hp: capturable, see trainer.PartitionedTrainer)."""
        for t in (g, m, v):
            if t.shape != w.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != w.device:
                raise TypeError("adam_rows: parameter, gradient and moments must be contiguous fp32 tensors of one shape")
        if not 0 <= lo <= hi <= w.numel() or hyper.numel() != 6 or hyper.dtype != torch.float32 or hyper.device != w.device:
            raise ValueError("adam_rows: bad range or hyper-parameter tensor")
        lib = _native.load()
        with torch.cuda.device(w.device):
            code = lib.lgc_adam_step_hp(_native.ptr(w) + 4 * lo, _native.ptr(g) + 4 * lo, _native.ptr(m) + 4 * lo,
                                        _native.ptr(v) + 4 * lo, hi - lo, _native.ptr(hyper), _native.stream_of(w.device))
        _native.check(code, "lgc_adam_step_hp")


def seed_prepare_reference(rows: Tensor, split: int, n: int, flag: Optional[Tensor] = None, slot: Optional[Tensor] = None):
    """What lgc_seed_prepare computes, as torch ops on any device (seeds above LGC_SEED_MAX ids; the CPU test double)."""
    dev = rows.device
    m = rows.numel()
    rows = torch.where((rows >= 0) & (rows < n), rows, torch.full_like(rows, -1))
    rows_s, perm = torch.sort(rows, stable=True)
    pos = torch.arange(m, device=dev)
    head = torch.ones(m, dtype=torch.bool, device=dev)
    head[1:] = rows_s[1:] != rows_s[:-1]
    user = (rows_s >= 0) & (rows_s < split)
    none = torch.full_like(rows_s, -1)
    dest_item = torch.where(head & (rows_s >= split), rows_s, none)
    dest_slot = torch.where(head & user, pos, none)
    dest_user = torch.where(head & user, rows_s, none)
    if flag is not None:
        heads = rows_s[head & user]
        flag[heads] = 1
        slot[heads] = pos[head & user].to(torch.int32)
    return rows_s, perm.to(torch.int32), dest_item, dest_slot, dest_user


DEVICE_OPS = DeviceOps()


def seeded_transpose_sum(graph: PropGraph, rows: Tensor, vals: Tensor, alphas: Sequence[float], n: int,
                         extra: Optional[Sequence] = None) -> Tensor:
    """sum_l alpha_l (A^T)^l g for a gradient g given by its non-zero rows, on one device: ``seeded_sum`` with the
    graph's own operator halves and no exchange."""
    user_t, item_t = graph.halves(True)
    return seeded_sum(user_t, item_t, graph.halves(False)[0], graph.split, rows, vals, alphas, n, extra)


def seeded_sum(user_t, item_t, user_fwd, split: int, rows: Tensor, vals: Tensor, alphas: Sequence[float], n: int,
               extra: Optional[Sequence] = None, ops: Optional[DeviceOps] = None, exchange=None,
               zero_rows: Optional[Sequence] = None) -> Tensor:
    """sum_l alpha_l (A^T)^l g for a gradient g given by its non-zero rows (``rows`` int64, repeats add up; ``vals`` [len, D])
    on a user|item graph -- what ``_PropagateSum.backward`` computes from a dense g, without ever forming it:
      * the seed is sorted once; repeated rows are summed in position order by lgc_segment_sum (no float atomics anywhere:
        the gradient has the same bits on every run, like the reference's CPU path);
      * hop 1, item side: only edges between an item and a seed USER matter -> lgc_seed_pull over the item rows of A^T
        (an entry counts if its user carries a flag; it then reads that user's row of the compact seed table) instead of
        a dense item step gathering 10 M rows of zeros, and only over the item rows some seed user's own row names
        (lgc_seed_mark: ~6 per seed user of 54 k) -- the others are zeros without a look at their entries;
      * hop 1, user side: the dense user step, reading only the 14 MB item block of g (the rest of that table is never
        initialised, let alone zero-filled);
      * the alpha_0 g term of the user rows is added to the seed rows afterwards instead of being read as a dense
        epilogue table by the last user step.
    ``user_t`` / ``item_t``: the user-row and item-row halves of A^T; ``user_fwd``: the user-row half of A (its columns
    name the item rows of A^T that hold a seed user).  Negative row ids stand for "no row" (a rank of a partition parks
    the pairs other ranks own there: a run of equal ids is summed by ONE lane group, so a thousand pairs clamped onto one
    stand-in row cost 330 us).  ``extra``: (rows, vals, scale) triples added to the result's rows
    the same way -- the regulariser's gradient (LightGCN.regularization_loss), which upstream's autograd materialises as
    three dense [N, D] tables.
    On a rank of a partition (partition.py) the halves are the rank's LOCAL operators -- the user rows it owns, and the
    item rows restricted to its own users as columns -- and ``exchange(block)`` starts the sum of an item block over the
    ranks, returning a handle whose ``wait()`` completes it (None: nothing to wait for).  The item block of layer l is
    waited for right before the user step of layer l + 1 reads it, exactly like the forward pass.  ``zero_rows``: row
    ranges of the result to zero-fill (the user rows other ranks own); default none."""
    ops = ops or DEVICE_OPS
    k = len(alphas) - 1
    dim = vals.size(1)
    dev = vals.device
    m = rows.numel()
    vals = vals.contiguous()
    # one launch (lgc_seed_prepare): the sorted ids, the permutation, the three destination lists and -- for k > 0 -- the
    # column map of the seeded pull (flag = 1, slot = position of the run's head, for every seed user)
    flag, slot = _seed_map_buffers(dev, split) if k > 0 else (None, None)
    rows_s, perm, dest_item, dest_slot, dest_user = ops.seed_prepare(rows, split, n, flag, slot)
    g_tab = torch.empty((n, dim), dtype=torch.float32, device=dev)         # only the item block is ever read
    g_tab[split:].zero_()
    ops.segment_sum(rows_s, dest_item, vals, g_tab, vals_index=perm)                        # g[items]

    def wait(work) -> None:
        if work is not None:
            work.wait()

    def finish(out: Tensor) -> Tensor:
        for e_rows, e_vals, e_scale in (extra or ()):
            e_s, e_perm, e_item, _, e_user = ops.seed_prepare(e_rows, split, n)
            ops.segment_sum(e_s, torch.maximum(e_item, e_user), e_vals.contiguous(), out, scale=e_scale, accumulate=True,
                            vals_index=e_perm)
        return out

    def new_result() -> Tensor:
        out = torch.empty((n, dim), dtype=torch.float32, device=dev)
        for lo, hi in (zero_rows or ()):
            if hi > lo:
                out[lo:hi].zero_()
        return out

    if k == 0:
        out = torch.zeros((n, dim), dtype=torch.float32, device=dev)
        ops.segment_sum(rows_s, torch.maximum(dest_item, dest_user), vals, out, scale=alphas[0], vals_index=perm)
        return finish(out)
    # compact table of the seed users: slot = position of the run's head
    gu = torch.empty((m, dim), dtype=torch.float32, device=dev)
    ops.segment_sum(rows_s, dest_slot, vals, gu, vals_index=perm)
    # Which item rows of A^T hold a seed user among their columns: row i of A^T has the columns {u : A[u, i] != 0}, so
    # the rows to read are the columns of the seed users' rows of the FORWARD operator A (not of A^T, whose user row u
    # lists {i : A[i, u] != 0} -- the same set only on a structurally symmetric edge list, which is never assumed).
    tables = [g_tab]
    pending = [None] * (k + 1)                                             # exchange of x_l[items]
    out = None
    for layer in range(1, k + 1):
        with _HopSpan():
            # an exchanged item block is reduced in place by a collective, which takes one dense run of memory: with an
            # exchange the tables keep the dense layout instead of scratch_table's padded rows (D=90: stride 96)
            nxt = ops.scratch_table(g_tab) if exchange is None else torch.empty_like(g_tab)
            if layer == 1:
                mark = _seed_mark_buffer(dev, n) if SEED_MARKS else None
                try:
                    if mark is not None:                                        # the item rows next to a seed user: the only
                        ops.seed_mark(user_fwd, rows_s, mark, 1)                # rows the pull has to read
                    ops.seed_pull(item_t, flag, slot, gu, nxt, mark)            # x_1[items] from the seed users
                finally:
                    ops.seed_flags(rows_s, split, flag, 0)                      # flags and marks are all zero between steps
                    if mark is not None:
                        ops.seed_mark(user_fwd, rows_s, mark, 0)
            else:
                ops.apply(item_t, tables[-1], nxt)
            if exchange is not None:
                pending[layer] = exchange(nxt[split:])
            wait(pending[layer - 1])                                            # x_{l-1}[items] is read from here on
            if layer < k:
                ops.apply(user_t, tables[-1], nxt)
                tables.append(nxt)
            else:
                tables.append(nxt)
                out = new_result()
                mix = ops.scratch_table(g_tab)
                ops.lincomb(mix[split:], [(alphas[l], tables[l - 1][split:]) for l in range(1, k + 1)])
                ops.apply(user_t, mix, out, a=1.0)
                wait(pending[k])
                if all(a == alphas[0] for a in alphas):     # equal alphas: mix + a x_K is the same chain of adds
                    ops.lincomb(out[split:], [(1.0, mix[split:]), (alphas[k], tables[k][split:])])
                else:
                    ops.lincomb(out[split:], [(alphas[l], tables[l][split:]) for l in range(0, k + 1)])
                # + alpha_0 g on the seed users (each such row is owned by one lane group: read, add, write)
                ops.segment_sum(rows_s, dest_user, vals, out, scale=alphas[0], accumulate=True, vals_index=perm)
    return finish(out)


class RegHook:
    """Where a regulariser on the layer-0 rows of the SAME weight table hands its gradient to the scoring node of one
    forward (``LightGCN.regularization_loss``): ``terms`` collects (rows, scale) pairs; the scoring node's backward adds
    ``grad_of_the_hook * scale * w[rows]`` to the <= 3B rows of the dense gradient it already writes."""

    def __init__(self, weight: Tensor):
        self.weight, self.token, self.terms, self.spent = weight, None, [], False


class _ScoresFromTable(torch.autograd.Function):
    """scores[m] = <out[i0_m], out[i1_m]> with out = sum_l alpha_l A^l w (src/lightgcn.py:121-125) as ONE autograd node:
    keeps the 2M gathered rows instead of the [N, D] table, and runs the backward pass from the sparse seed.  Its second
    output is a zero-valued scalar ``token``: a loss term that depends on ``w`` only through a few of its rows can route
    its gradient through it (RegHook) instead of through a dense [N, D] tensor of its own."""

    @staticmethod
    def forward(ctx, w: Tensor, graph: PropGraph, alphas: tuple, idx0: Tensor, idx1: Tensor, hook: Optional[RegHook]):
        idx0, idx1 = idx0.contiguous(), idx1.contiguous()
        n_nodes = w.size(0)
        # only the rows the pairs name are read below (clamped like the gathers that follow, so that every row that is
        # gathered has been computed): the last user step is restricted to them
        # (ids outside the table are skipped by the listed-rows launches and scored NaN below: no clamp; the two rows of one
        # contiguous [2, M] label tensor are one vector already: no cat)
        m = idx0.numel()
        if (idx1.data_ptr() == idx0.data_ptr() + 8 * m and idx0.untyped_storage().data_ptr() == idx1.untyped_storage().data_ptr()):
            rows = idx0.as_strided((2 * m,), (1,))
        else:
            rows = torch.cat([idx0, idx1])
        emb = _layer_sum(graph, w.detach(), alphas, transpose=False, final_rows=rows)
        # one launch: the scores, the two gathered rows of every pair and a validity byte (an invalid pair scores NaN,
        # keeps zero rows and carries no gradient)
        scores, e0, e1, ok = DEVICE_OPS.pair_scores_rows(emb, idx0, idx1)
        ctx.save_for_backward(e0, e1, rows, ok)
        ctx.graph, ctx.alphas, ctx.n, ctx.hook, ctx.width = graph, alphas, emb.size(0), hook, emb.size(1)
        ctx.set_materialize_grads(False)                                # an unused output arrives as None, not as zeros
        return scores, torch.zeros((), dtype=torch.float32, device=emb.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores: Tensor, grad_token: Optional[Tensor]):
        e0, e1, rows, ok = ctx.saved_tensors
        hook = ctx.hook
        extra = []
        if hook is not None:
            hook.spent = True                                           # later regularisers take the plain torch path
            if grad_token is not None:
                w = hook.weight.detach()
                extra = [(r, w[r] * grad_token, scale) for r, scale in hook.terms]
        if grad_scores is None:                                          # only the regulariser was differentiated
            out = torch.zeros((ctx.n, ctx.width), dtype=torch.float32, device=e0.device)
            for r, v, scale in extra:
                r_s, perm = torch.sort(r, stable=True)
                segment_sum(r_s, r_s, v.contiguous(), out, scale=scale, accumulate=True, vals_index=perm.to(torch.int32))
            return out, None, None, None, None, None
        # pairs that share a node simply add up; d score / d out[i0] = e1, d / d out[i1] = e0; an invalid pair's id is
        # outside the table: "no row" for the seed
        vals = DEVICE_OPS.pair_seed_vals(grad_scores, ok, None, e0, e1)
        return seeded_transpose_sum(ctx.graph, rows, vals, ctx.alphas, ctx.n, extra), None, None, None, None, None


class _RegThroughHook(torch.autograd.Function):
    """value = decay/2 * (|w[u]|^2 + |w[p]|^2 + |w[n]|^2) / size (src/utils_v2.py:193-211), differentiable through the
    scoring node's token: d value / d w[r] = decay / size * w[r] per occurrence of r, added by that node's backward."""

    @staticmethod
    def forward(ctx, token: Tensor, value: Tensor) -> Tensor:
        return value + token

    @staticmethod
    def backward(ctx, grad: Tensor):
        return grad, None


def regularization_through(hook: RegHook, size: int, users: Tensor, pos: Tensor, neg: Tensor, decay: float) -> Tensor:
    """The regulariser of src/utils_v2.py:193-211 on ``hook.weight``, its gradient routed into the scoring node.  Value and
    row list in ONE launch (lgc_reg_rows) when the table qualifies (fp32, unit inner stride): upstream's expression is 13
    small launches plus nine that normalise the ids -- 0.13 ms of a 3.4 ms step."""
    w = hook.weight.detach()
    # upstream's gathers take CPU or int32 index tensors and negative (wrapping) ids on a CUDA table; the kernels take raw
    # int64 device pointers, so the lists are normalised here (no launch when they already are int64 on the device)
    lists = [t.reshape(-1).to(device=w.device, dtype=torch.int64).contiguous() for t in (users, pos, neg)]
    if FUSED_GLUE and w.dtype == torch.float32 and w.dim() == 2 and w.stride(1) == 1:
        value, rows = DEVICE_OPS.reg_rows(w, lists, 0.5 * float(decay) / float(size))
    else:
        value = (1 / 2) * (w[users].norm().pow(2) + w[pos].norm().pow(2) + w[neg].norm().pow(2)) / size * decay
        rows = torch.cat([torch.where(r < 0, r + w.size(0), r) for r in lists])
    hook.terms.append((rows, float(decay) / float(size)))
    return _RegThroughHook.apply(hook.token, value)


# the step's glue around the scoring node as single launches (lgc_reg_rows, lgc_bpr_loss); "0": upstream's torch expressions
FUSED_GLUE = os.environ.get("LGCN_FUSED_GLUE", "1") == "1"


class _BprLoss(torch.autograd.Function):
    """-mean(log sigmoid(pos - neg)) / n_pairs (src/lightgcn.py:262-286 with lambda_reg = 0) and its gradient in one launch
    (lgc_bpr_loss) instead of five forward and six backward launches of elementwise torch kernels."""

    @staticmethod
    def forward(ctx, positives: Tensor, negatives: Tensor) -> Tensor:
        n = positives.numel()
        pos, neg = positives.reshape(-1), negatives.reshape(-1)
        if (pos.is_contiguous() and neg.is_contiguous() and neg.data_ptr() == pos.data_ptr() + 4 * n
                and pos.untyped_storage().data_ptr() == neg.untyped_storage().data_ptr()):
            scores = pos.as_strided((2 * n,), (1,))            # out[:B], out[B:] of one score vector: no copy
        else:
            scores = torch.cat([pos, neg])
        loss, grad = DEVICE_OPS.bpr_loss(scores, None, n * n)   # -sum log sigmoid / n^2
        ctx.save_for_backward(grad)
        ctx.shapes = (positives.shape, negatives.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        (grad,) = ctx.saved_tensors
        g = grad * grad_out
        n = g.numel() // 2
        return g[:n].reshape(ctx.shapes[0]), g[n:].reshape(ctx.shapes[1])


def bpr_loss_fused(positives: Tensor, negatives: Tensor) -> Optional[Tensor]:
    """``BPRLoss(0)(positives, negatives)`` through lgc_bpr_loss, or None when the inputs do not qualify (then the caller
    evaluates upstream's expression on torch ops)."""
    if (FUSED_GLUE and positives.is_cuda and negatives.is_cuda and positives.dtype == torch.float32
            and negatives.dtype == torch.float32 and positives.shape == negatives.shape and positives.numel() > 0
            and positives.device == negatives.device and positives.numel() <= 1 << 20):
        return _BprLoss.apply(positives, negatives)
    return None


def routable_index(t) -> bool:
    """An index argument the routed regulariser can take: an integer (not bool) tensor -- anything else upstream's
    ``init_embed[idx]`` accepts (masks, lists, slices) goes through upstream's expression on plain torch ops."""
    return torch.is_tensor(t) and t.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def regularizer_rows(t: Tensor, w: Tensor) -> Tensor:
    """Row ids of ``w[t]`` as a flat int64 vector on ``w``'s device, negative ids wrapped like torch's indexing."""
    r = t.reshape(-1).to(device=w.device, dtype=torch.int64)
    return torch.where(r < 0, r + w.size(0), r)


def scores_from_table(w: Tensor, graph: PropGraph, alphas: Sequence[float], edge_label_index: Tensor,
                      hook: Optional[RegHook] = None) -> Tensor:
    """``pair_dot(propagate_sum(w, graph, alphas), edge_label_index)``; with gradients on, a user|item graph and few
    label pairs it runs as one node whose backward pass starts from the sparse seed.  ``hook``: filled
    in (``hook.token``) when that node is used, so that a regulariser can hand it its gradient."""
    _native.require_device(w, "embedding table")
    _native.require_device(edge_label_index, "edge_label_index")
    if edge_label_index.dtype != torch.int64 or edge_label_index.dim() != 2 or edge_label_index.size(0) != 2:
        raise TypeError("edge_label_index must be an int64 tensor of shape [2, M]")
    raise_pending_index_error(w.device)
    alphas = tuple(float(a) for a in alphas)
    sparse_ok = (SPARSE_BACKWARD and torch.is_grad_enabled() and w.requires_grad and graph.split is not None
                 and USE_BIPARTITE and len(alphas) - 1 <= _native.MAX_TERMS - 1
                 and 2 * edge_label_index.size(1) * SEED_ROWS_FACTOR <= w.size(0))   # a seed far smaller than the table
    if not sparse_ok:
        few = (SCORED_ROWS_ONLY and graph.split is not None and USE_BIPARTITE and len(alphas) - 1 <= _native.MAX_TERMS - 1
               and len(alphas) > 1 and 2 * edge_label_index.size(1) * SEED_ROWS_FACTOR <= w.size(0))
        if few and not (torch.is_grad_enabled() and w.requires_grad):
            # scoring a few pairs without gradients (an evaluation batch under no_grad): the last user step and the last
            # item step for the rows the pairs name only, like the training forward
            rows = edge_label_index.reshape(-1).clamp(0, w.size(0) - 1)
            return pair_dot(_layer_sum(graph, w.detach().contiguous(), alphas, transpose=False, final_rows=rows), edge_label_index)
        return pair_dot(propagate_sum(w, graph, alphas), edge_label_index)
    scores, token = _ScoresFromTable.apply(w, graph, alphas, edge_label_index[0], edge_label_index[1], hook)
    if hook is not None:
        hook.token = token
    return scores


def pair_dot(emb: Tensor, edge_label_index: Tensor) -> Tensor:
    """scores[m] = <emb[idx[0, m]], emb[idx[1, m]]>  (src/lightgcn.py:123-125)."""
    _native.require_device(emb, "embeddings")
    _native.require_device(edge_label_index, "edge_label_index")
    if edge_label_index.dtype != torch.int64 or edge_label_index.dim() != 2 or edge_label_index.size(0) != 2:
        raise TypeError("edge_label_index must be an int64 tensor of shape [2, M]")
    if emb.dtype != torch.float32 or emb.dim() != 2:
        raise TypeError("embeddings must be a 2-D fp32 tensor")
    return _PairDot.apply(emb, edge_label_index[0], edge_label_index[1])


# ----------------------------------------------------------------------------------------
# serving tail: seen-mask + top-k on the device
# ----------------------------------------------------------------------------------------
TOPK_MAX = 256


class SeenLists:
    """The purchase matrix as a device CSR (``ptr`` int64 [n_users + 1], ``items`` int64) plus the users of a
    request: the list form of ``recommendK``'s ``interactions_t`` (seen = 1 for listed items)."""

    def __init__(self, ptr: Tensor, items: Tensor, users: Optional[Tensor] = None):
        self.ptr, self.items, self.users = ptr, items, users

    def validate(self, n_users: int, where: str = "purchase lists") -> "SeenLists":
        """lgc_mask_topk reads ptr[u], ptr[u + 1] and items[ptr[u] .. ptr[u + 1]) on trust: a truncated or stale list
        (ptr shorter than n_users + 1, not monotone, pointing past ``items``) must end here in a ValueError, not in an
        out-of-range read on the device.  One host sync; called once per loaded file, not per request."""
        def bad(msg):
            raise ValueError(f"{where}: {msg}")
        if self.ptr.dtype != torch.int64 or self.ptr.dim() != 1 or self.ptr.numel() != n_users + 1:
            bad(f"ptr must be int64 [{n_users + 1}], got {self.ptr.dtype} {tuple(self.ptr.shape)}")
        if self.items.dtype != torch.int64 or self.items.dim() != 1:
            bad(f"items must be a 1-D int64 tensor, got {self.items.dtype} {tuple(self.items.shape)}")
        if not self.ptr.is_contiguous() or not self.items.is_contiguous():
            bad("ptr and items must be contiguous")
        checks = torch.stack([(self.ptr[0] == 0).reshape(()), (self.ptr[-1] == self.items.numel()).reshape(()),
                              (self.ptr[1:] >= self.ptr[:-1]).all().reshape(())])
        if not bool(checks.all().item()):
            bad("ptr is not a non-decreasing 0 .. len(items) sequence")
        return self

    def for_users(self, users: Tensor) -> "SeenLists":
        return SeenLists(self.ptr, self.items, users)

    dense_builds = 0          # CSRs built by from_dense so far (cache hits do not count)
    _dense_cache: list = []   # [(key, mask, SeenLists)], most recent last

    @classmethod
    def from_dense(cls, interactions_t: Tensor, user_id_list, n_users: int, device=None) -> "SeenLists":
        """The CSR of the reference's dense mask (``[n_sel, n_items]``, row r = the seen items of ``user_id_list[r]``;
        src/utils_v2.py:92-106 + :136-137), on ``device`` (default: where the mask lives).  Users outside the list get
        empty rows.  The list form can only say "seen": a mask with any entry other than 0 or 1 is refused (upstream's
        matrix sums a repeated purchase to 2, where ``1 - seen`` is -1), and so is a user listed twice with different
        rows.  Upstream passes the same mask object every epoch: the result is kept per tensor identity + version."""
        m = interactions_t
        if not torch.is_tensor(m) or m.dim() != 2:
            raise TypeError("the dense mask must be a 2-D tensor")
        ids = torch.as_tensor(user_id_list).reshape(-1).to(dtype=torch.int64, device="cpu")
        device = torch.device(m.device if device is None else device)
        key = (id(m), m._version, m.data_ptr(), tuple(m.shape), int(n_users), str(device), ids.numpy().tobytes())
        for k_, m_, got in cls._dense_cache:
            if k_ == key and m_ is m:
                return got
        if ids.numel() != m.size(0):
            raise ValueError(f"the dense mask has {m.size(0)} rows for {ids.numel()} users")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_users):
            raise ValueError(f"user ids must lie in [0, {n_users})")
        nonzero = m != 0
        if bool((nonzero & (m != 1)).any()):
            raise ValueError("the dense mask has entries other than 0 and 1 (a purchase counted twice?): "
                             "the list form cannot express them")
        ids_m = ids.to(m.device)
        order = torch.argsort(ids_m, stable=True)                      # rows by user, first occurrence first
        sorted_ids = ids_m[order]
        first = torch.ones_like(sorted_ids, dtype=torch.bool)
        first[1:] = sorted_ids[1:] != sorted_ids[:-1]
        if not bool(first.all()):                                      # a user listed twice: its rows must agree
            lead = order[torch.cummax(torch.where(first, torch.arange(len(order), device=m.device), 0), 0).values]
            if not bool((nonzero[order] == nonzero[lead]).all()):
                raise ValueError("a user appears twice in user_id_list with different mask rows")
        rows = order[first]                                            # one mask row per distinct user, ascending by user
        r, c = nonzero[rows].nonzero(as_tuple=True)                    # row-major: by user, items ascending
        counts = torch.zeros(n_users, dtype=torch.int64, device=m.device)
        counts[sorted_ids[first]] = nonzero[rows].sum(dim=1)
        ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=m.device)
        torch.cumsum(counts, 0, out=ptr[1:])
        got = cls(ptr.to(device), c.to(dtype=torch.int64).contiguous().to(device))
        cls.dense_builds += 1
        cls._dense_cache.append((key, m, got))
        del cls._dense_cache[:-4]
        return got

    def to_dense(self, user_id_list, n_items: int) -> Tensor:
        """The fp32 ``[n_sel, n_items]`` mask these lists stand for (host side; tests and small requests)."""
        ptr, items = self.ptr.cpu(), self.items.cpu()
        ids = torch.as_tensor(user_id_list).reshape(-1).long().cpu()
        out = torch.zeros((ids.numel(), n_items), dtype=torch.float32)
        for r, u in enumerate(ids.tolist()):
            out[r, items[ptr[u]:ptr[u + 1]]] = 1.0
        return out


class PositiveLists:
    """A ``*_pos_list_df`` of the reference (columns ``user_id_idx``, ``item_id_idx_list``; src/utils_v2.py:109-113) as a
    device CSR over all users -- ``ptr`` int64 [n_users + 1], ``items`` int64, duplicates kept -- plus ``users``, the
    listed users in the frame's order (int64): what ``MARK_MAPK`` intersects the recommendations with."""

    def __init__(self, ptr: Tensor, items: Tensor, users: Tensor):
        self.ptr, self.items, self.users = ptr, items, users
        self._distinct: Optional[Tensor] = None
        self._entries = None

    def _sorted_entries(self):
        """(owner, items, head) of all entries ordered by (user, item) -- two stable sorts -- with ``head`` marking the
        first entry of every run of equal (user, item).  Temporaries: the callers keep what they derive, not these."""
        dev, n_users = self.ptr.device, self.ptr.numel() - 1
        owner = torch.repeat_interleave(torch.arange(n_users, device=dev), self.ptr[1:] - self.ptr[:-1],
                                        output_size=self.items.numel())
        items, order = torch.sort(self.items, stable=True)
        owner, order = torch.sort(owner[order], stable=True)
        items = items[order]
        head = torch.ones_like(items, dtype=torch.bool)
        head[1:] = (owner[1:] != owner[:-1]) | (items[1:] != items[:-1])
        return owner, items, head

    @property
    def distinct(self) -> Tensor:
        """int64 [n_users]: the number of DISTINCT items of each user's list (0 for a user without one) -- what NDCG's
        ideal ranking and AP's denominator can at most reach, where recall divides by the length with duplicates.
        Computed once, on the lists' device (two stable sorts order the entries by (user, item); a run's head counts),
        and kept; only the counts are."""
        if self._distinct is None:
            if self._entries is not None:
                heads = self._entries[0]
            else:
                owner, _, head = self._sorted_entries()
                heads = owner[head]
            self._distinct = torch.bincount(heads, minlength=self.ptr.numel() - 1).to(torch.int64).contiguous()
        return self._distinct

    def distinct_entries(self):
        """(owner int64 [E], items int64 [E]): every distinct (user, item) of the lists, by user and then by item -- the
        same sort ``distinct`` counts; user u's entries are [cumsum(distinct)[u - 1], cumsum(distinct)[u]).  Kept once
        asked for (full-rank evaluation asks); ``distinct`` alone keeps no entry."""
        if self._entries is None:
            owner, items, head = self._sorted_entries()
            self._entries = (owner[head].contiguous(), items[head].contiguous())
        return self._entries

    @classmethod
    def from_lists(cls, user_id_idx, item_id_idx_list, n_users: int, device=None) -> "PositiveLists":
        """From the two columns: user ids and, per user, a sequence of item indices (0-based columns of the scores)."""
        import numpy as np
        users = np.asarray(list(user_id_idx), dtype=np.int64).reshape(-1)
        lists = [np.asarray(list(x), dtype=np.int64).reshape(-1) for x in item_id_idx_list]
        if len(lists) != len(users):
            raise ValueError(f"{len(users)} users but {len(lists)} item lists")
        if len(users) and (users.min() < 0 or users.max() >= n_users):
            raise ValueError(f"user ids must lie in [0, {n_users})")
        by_user = {}
        for u, lst in zip(users.tolist(), lists):
            if u in by_user and not np.array_equal(by_user[u], lst):
                raise ValueError(f"user {u} is listed twice with different item lists")
            by_user[u] = lst
        counts = np.zeros(n_users, dtype=np.int64)
        for u, lst in by_user.items():
            counts[u] = len(lst)
        ptr = np.zeros(n_users + 1, dtype=np.int64)
        np.cumsum(counts, out=ptr[1:])
        order = sorted(by_user)
        items = np.concatenate([by_user[u] for u in order]) if order else np.zeros(0, dtype=np.int64)
        return cls.from_arrays(ptr, items, users, device)

    @classmethod
    def from_frame(cls, pos_list_df, n_users: int, device=None) -> "PositiveLists":
        return cls.from_lists(pos_list_df["user_id_idx"], pos_list_df["item_id_idx_list"], n_users, device)

    @classmethod
    def from_arrays(cls, ptr, items, users, device=None) -> "PositiveLists":
        """From a ready CSR (anything ``torch.as_tensor`` takes)."""
        conv = lambda a: torch.as_tensor(a).to(dtype=torch.int64, device=device).contiguous()
        return cls(conv(ptr), conv(items), conv(users))

    def validate(self, n_users: int, n_items: Optional[int] = None, where: str = "positive lists") -> "PositiveLists":
        """The kernels read the CSR on trust (as ``SeenLists.validate``), and every listed user needs at least one
        positive: upstream's recall divides by the list's length.  One host sync; once per frame, not per epoch."""
        SeenLists(self.ptr, self.items).validate(n_users, where)
        if self.users.dtype != torch.int64 or self.users.dim() != 1:
            raise ValueError(f"{where}: users must be a 1-D int64 tensor")
        if self.users.numel():
            if int(self.users.min()) < 0 or int(self.users.max()) >= n_users:
                raise ValueError(f"{where}: user ids must lie in [0, {n_users})")
            if bool((self.ptr[self.users + 1] == self.ptr[self.users]).any()):
                raise ValueError(f"{where}: a listed user has an empty item list (recall would divide by zero)")
        if n_items is not None and self.items.numel() and (int(self.items.min()) < 0 or int(self.items.max()) >= n_items):
            raise ValueError(f"{where}: item indices must lie in [0, {n_items})")
        return self

    def to(self, device) -> "PositiveLists":
        moved = PositiveLists(self.ptr.to(device), self.items.to(device), self.users.to(device))
        if self._distinct is not None:
            moved._distinct = self._distinct.to(device)
        return moved


def mask_topk(scores: Tensor, seen, k: int) -> Tensor:
    """Indices [rows, k] (int64, on the device) of the k largest ``scores * (1 - seen)`` per row, ties by lower index
    (src/lightgcn.py:175-177).  The order: every NaN first (either sign bit, as torch.topk ranks them), then +inf, the
    finite values with -0 equal to +0, then -inf; equal elements, NaNs among them, by ascending index.
    ``seen``: a dense fp32 tensor, a ``SeenLists``, or None.  k <= 256."""
    lists = seen if isinstance(seen, SeenLists) else None
    if lists is not None:
        seen = None
    _native.require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise TypeError("scores must be a 2-D fp32 tensor with unit inner stride")
    if seen is not None:
        _native.require_device(seen, "seen mask")
        if seen.dtype != torch.float32 or seen.shape != scores.shape or seen.stride(1) != 1:
            raise TypeError("the seen mask must be fp32 of the scores' shape")
    rows, cols = scores.shape
    if not 1 <= k <= cols:
        raise RuntimeError(f"selected index k out of range: k={k}, {cols} columns")      # torch.topk's error class
    out = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    lib = _native.load()
    with torch.cuda.device(scores.device):
        code = lib.lgc_mask_topk(_native.ptr(scores), scores.stride(0), _native.ptr(seen), 0 if seen is None else seen.stride(0),
                                 _native.ptr(lists.ptr) if lists else None, _native.ptr(lists.items) if lists else None,
                                 _native.ptr(lists.users) if lists else None, rows, cols, k, _native.ptr(out), None,
                                 _native.stream_of(scores.device))
    _native.check(code, "lgc_mask_topk")
    return out


# ----------------------------------------------------------------------------------------
# epoch evaluation: score panels -> top-k -> hits, in bounded device memory
# ----------------------------------------------------------------------------------------
DEFAULT_WORKSPACE_BYTES = 64 << 20


def panel_rows(n_items: int, workspace_bytes: int = DEFAULT_WORKSPACE_BYTES) -> int:
    """Rows of one score panel: as many fp32 rows of ``n_items`` scores as fit the workspace, at least one."""
    return max(1, int(workspace_bytes) // (4 * int(n_items)))


def _check_tables(users: Tensor, items: Tensor) -> None:
    for t, name in ((users, "users"), (items, "items")):
        _native.require_device(t, name)
        if t.dtype != torch.float32 or t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1) or t.stride(0) < t.size(1):
            raise TypeError(f"{name} must be a 2-D fp32 table with unit inner stride")
    if users.size(1) != items.size(1) or users.device != items.device:
        raise TypeError("users and items must have the same width and live on the same device")
    if items.size(0) < 1:
        raise ValueError("no items to score")


def _check_ids(ids: Optional[Tensor], like: Tensor, name: str) -> None:
    if ids is None:
        return
    if ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous() or ids.device != like.device:
        raise TypeError(f"{name} must be a contiguous 1-D int64 tensor on the tables' device")


def _score_panel(lib, users: Tensor, ids_ptr: Optional[int], n_rows: int, items: Tensor, out_ptr: int, out_stride: int) -> None:
    dev = users.device
    code = lib.lgc_score_rows(_native.ptr(users), users.stride(0), users.size(0), ids_ptr, n_rows, _native.ptr(items),
                              items.stride(0), items.size(0), users.size(1), out_ptr, out_stride, _native.ptr(_status(dev)),
                              _native.stream_of(dev))
    _native.check(code, "lgc_score_rows")


def score_rows(users: Tensor, row_ids: Optional[Tensor], items: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``out[r, i] = <users[row_ids[r]], items[i]>`` (fp32 ``[n_rows, n_items]``; ``row_ids`` None = every user row in
    order): lgc_score_rows.  The bits of an entry depend only on its two rows, not on where it sits or on the panel it
    is computed in.  An id outside the table zero-fills its row and raises at ``check_index_status()``."""
    _check_tables(users, items)
    _check_ids(row_ids, users, "row_ids")
    n_rows, n_items = users.size(0) if row_ids is None else row_ids.numel(), items.size(0)
    if out is None:
        out = torch.empty((n_rows, n_items), dtype=torch.float32, device=users.device)
    elif (out.dtype != torch.float32 or out.shape != (n_rows, n_items) or out.device != users.device
          or (n_items > 1 and out.stride(1) != 1) or (n_rows > 1 and out.stride(0) < n_items)):
        raise TypeError(f"out must be fp32 [{n_rows}, {n_items}] with unit inner stride on the tables' device")
    with torch.cuda.device(users.device):
        _score_panel(_native.load(), users, _native.ptr(row_ids), n_rows, items, _native.ptr(out),
                     out.stride(0) if n_rows > 1 else n_items)
    _snapshot_status(users.device)
    return out


_score_workspaces = {}


def _score_workspace(device: torch.device, n_floats: int) -> Tensor:
    """Per (device, stream, host thread): the score panel, allocated once and reused (grown when a request needs more).
    lgc_score_rows fills it and lgc_mask_topk ranks it in a later launch: two threads on one stream (the default stream
    of every thread) would otherwise rank each other's scores."""
    key = _scratch_key(device)
    got = _score_workspaces.get(key)
    if got is None or got.numel() < n_floats:
        _score_workspaces.pop(key, None)
        got = None                                   # let go of the old one before asking for the new one
        got = torch.empty(n_floats, dtype=torch.float32, device=device)
        _score_workspaces[key] = got
    return got


def recommend_topk(users: Tensor, sel: Tensor, items: Tensor, seen: Optional[SeenLists], k: int,
                   workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, return_values: bool = False):
    """Indices int64 ``[n_sel, k]`` (on the device) of the k largest ``<users[sel[r]], items[i]> * (1 - seen)`` per row,
    ties by lower index -- what ``recommendK`` ranks, without ever holding more than one panel of
    ``panel_rows(n_items, workspace_bytes)`` score rows: per panel one lgc_score_rows and one lgc_mask_topk (list form
    of the mask; None = no mask).  The result does not depend on the panel size, bit for bit.  With
    ``return_values`` also the masked scores fp32 ``[n_sel, k]``."""
    _check_tables(users, items)
    _check_ids(sel, users, "sel")
    n_sel, n_items, dev = sel.numel(), items.size(0), users.device
    if k > TOPK_MAX:
        raise ValueError(f"the list form of the mask supports k <= {TOPK_MAX}")
    if not 1 <= k <= n_items:
        raise RuntimeError(f"selected index k out of range: k={k}, {n_items} columns")      # torch.topk's error class
    if seen is not None:
        if not isinstance(seen, SeenLists):
            raise TypeError("seen must be a SeenLists (SeenLists.from_dense converts the reference's dense mask) or None")
        _check_ids(seen.ptr, users, "seen.ptr")
        _check_ids(seen.items, users, "seen.items")
    index = torch.empty((n_sel, k), dtype=torch.int64, device=dev)
    value = torch.empty((n_sel, k), dtype=torch.float32, device=dev) if return_values else None
    if n_sel:
        rows = min(n_sel, panel_rows(n_items, workspace_bytes))
        panel = _score_workspace(dev, rows * n_items)
        lib = _native.load()
        # lgc_mask_topk reads the lists of a row's user on trust: an id outside them is clamped for that read (its score
        # row is zero-filled and the id reported through the index status by lgc_score_rows)
        list_rows = sel.clamp(0, seen.ptr.numel() - 2) if seen else None
        with torch.cuda.device(dev):
            stream = _native.stream_of(dev)
            for lo in range(0, n_sel, rows):
                n = min(rows, n_sel - lo)
                _score_panel(lib, users, sel.data_ptr() + 8 * lo, n, items, panel.data_ptr(), n_items)
                code = lib.lgc_mask_topk(panel.data_ptr(), n_items, None, 0, _native.ptr(seen.ptr) if seen else None,
                                         _native.ptr(seen.items) if seen else None,
                                         list_rows.data_ptr() + 8 * lo if seen else None, n, n_items, k,
                                         index.data_ptr() + 8 * k * lo, value.data_ptr() + 4 * k * lo if return_values else None,
                                         stream)
                _native.check(code, "lgc_mask_topk")
        _snapshot_status(dev)
    return (index, value) if return_values else index


def topk_hits(topk: Tensor, positives: PositiveLists, users: Tensor):
    """(hits int32 [n], recall float64 [n]) on the device: per row the number of its top-k items among the positives of
    ``users[r]`` and that number over the list's length (lgc_topk_hits)."""
    _native.require_device(topk, "topk")
    if topk.dtype != torch.int64 or topk.dim() != 2 or topk.size(1) < 1 or topk.stride(1) != 1:
        raise TypeError("topk must be a 2-D int64 tensor with unit inner stride")
    _check_ids(users, topk, "users")
    _check_ids(positives.ptr, topk, "positives.ptr")
    _check_ids(positives.items, topk, "positives.items")
    n, k, dev = topk.size(0), topk.size(1), topk.device
    if users.numel() != n:
        raise ValueError(f"{n} rows of recommendations for {users.numel()} users")
    hits = torch.empty(n, dtype=torch.int32, device=dev)
    recall = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        code = _native.load().lgc_topk_hits(_native.ptr(topk), topk.stride(0) if n > 1 else k, k, _native.ptr(positives.ptr),
                                            _native.ptr(positives.items), _native.ptr(users), n, positives.ptr.numel() - 1,
                                            _native.ptr(hits), _native.ptr(recall), _native.ptr(_status(dev)),
                                            _native.stream_of(dev))
    _native.check(code, "lgc_topk_hits")
    return hits, recall


def metric_sums(hits: Tensor, recall: Tensor) -> Tensor:
    """int64 [2] on the device: the sum of ``hits`` and the BITS of the fp64 sum of ``recall`` (``.view(torch.float64)``),
    added in a fixed order by one workgroup (lgc_metric_sums): the same bits on every run."""
    dev = hits.device
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        code = _native.load().lgc_metric_sums(_native.ptr(hits), _native.ptr(recall), hits.numel(), _native.ptr(out),
                                              _native.ptr(out[1:]), _native.stream_of(dev))
    _native.check(code, "lgc_metric_sums")
    return out


def evaluate_topk(users_table: Tensor, items: Tensor, seen: Optional[SeenLists], users: Tensor, positives: PositiveLists,
                  k: int, workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
    """(precision, recall, hits): MARK_MAPK's two means (src/lightgcn.py:184-190) over ``users`` as Python floats and the
    per-user hit counts (int32, left on the device).  One host sync, at the end: two sums and the index status."""
    top = recommend_topk(users_table, users, items, seen, k, workspace_bytes)
    hits, recall = topk_hits(top, positives, users)
    n, dev = users.numel(), users.device
    if n == 0:
        return float("nan"), float("nan"), hits                          # upstream: the mean of an empty column
    sums = metric_sums(hits, recall)
    host = torch.cat([sums, _status(dev)[:1].to(torch.int64)]).cpu()     # the one sync
    if int(host[2]) & _native.ST_INDEX_OOB:
        try:
            check_index_status(dev)                                      # clears the word and its host snapshot
        except IndexError:
            pass
        raise IndexError("evaluation: a user id lies outside the user table or the positive lists")
    return int(host[0]) / (k * n), float(host[1:2].view(torch.float64)[0]) / n, hits


# ----------------------------------------------------------------------------------------
# ranking metrics at several cutoffs from one ranking pass
# ----------------------------------------------------------------------------------------
METRIC_NAMES = ("precision", "recall", "ndcg", "map", "mrr", "hit_rate")      # the LGC_RM_* columns, in order


def _host_cutoffs(cutoffs, k: int):
    """(list of ints, ctypes int32 array): 1..8 cutoffs, each >= 1, strictly ascending, the last <= k."""
    import ctypes
    cuts = [int(c) for c in cutoffs]
    if not 1 <= len(cuts) <= _native.RM_MAX_CUTOFFS:
        raise ValueError(f"1..{_native.RM_MAX_CUTOFFS} cutoffs, got {len(cuts)}")
    if cuts[0] < 1 or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"cutoffs must be >= 1 and strictly ascending, got {cuts}")
    if cuts[-1] > k:
        raise ValueError(f"the largest cutoff {cuts[-1]} exceeds k = {k}")
    return cuts, (ctypes.c_int32 * len(cuts))(*cuts)


def _check_topk(topk: Tensor) -> None:
    _native.require_device(topk, "topk")
    if topk.dtype != torch.int64 or topk.dim() != 2 or topk.size(1) < 1 or topk.stride(1) != 1:
        raise TypeError("topk must be a 2-D int64 tensor with unit inner stride")
    if topk.size(1) > TOPK_MAX:
        raise ValueError(f"k <= {TOPK_MAX}")


def rank_metrics(topk: Tensor, positives: PositiveLists, users: Tensor, cutoffs, return_bits: bool = False):
    """(hits int32 [n, C], metrics float64 [n, C, 6]) on the device, per row and per cutoff c of ``cutoffs`` (ascending,
    the last <= topk.size(1)): the hits among the first c entries and precision, recall, NDCG, AP, RR and hit
    (``METRIC_NAMES``; include/lgconv_hip.h: lgc_rank_metrics) against the positives of ``users[r]``.  The rows of
    ``topk`` must be ranked and distinct (``recommend_topk``'s are).  With ``return_bits`` also ``hit_bits`` [n, 4]:
    bit j of a row = topk[r, j] is a positive (uint64 words, held in an int64 tensor)."""
    _check_topk(topk)
    _check_ids(users, topk, "users")
    _check_ids(positives.ptr, topk, "positives.ptr")
    _check_ids(positives.items, topk, "positives.items")
    n, k, dev = topk.size(0), topk.size(1), topk.device
    if users.numel() != n:
        raise ValueError(f"{n} rows of recommendations for {users.numel()} users")
    cuts, cuts_c = _host_cutoffs(cutoffs, k)
    hits = torch.empty((n, len(cuts)), dtype=torch.int32, device=dev)
    metrics = torch.empty((n, len(cuts), _native.RM_COUNT), dtype=torch.float64, device=dev)
    bits = torch.empty((n, TOPK_MAX // 64), dtype=torch.int64, device=dev) if return_bits else None
    if n == 0:                                       # empty tensors have no address to hand over; nothing to compute
        return (hits, metrics, bits) if return_bits else (hits, metrics)
    distinct = positives.distinct
    with torch.cuda.device(dev):
        code = _native.load().lgc_rank_metrics(_native.ptr(topk), topk.stride(0) if n > 1 else k, k, _native.ptr(positives.ptr),
                                               _native.ptr(positives.items), _native.ptr(distinct), _native.ptr(users), n,
                                               positives.ptr.numel() - 1, cuts_c, len(cuts), _native.ptr(bits),
                                               _native.ptr(hits), _native.ptr(metrics), _native.ptr(_status(dev)),
                                               _native.stream_of(dev))
    _native.check(code, "lgc_rank_metrics")
    return (hits, metrics, bits) if return_bits else (hits, metrics)


def column_sums(table: Tensor) -> Tensor:
    """float64 [n_cols] on the device: the sum of every column of a 2-D float64 tensor (at most 64 columns, unit inner
    stride), each added in ``metric_sums``' fixed order (lgc_column_sums): the same bits on every run.  No rows: zeros."""
    _native.require_device(table, "table")
    if table.dtype != torch.float64 or table.dim() != 2 or table.size(1) < 1 or (table.size(1) > 1 and table.stride(1) != 1):
        raise TypeError("column_sums takes a 2-D float64 tensor with unit inner stride")
    n, cols, dev = table.size(0), table.size(1), table.device
    if cols > _native.COLUMN_SUMS_MAX:
        raise ValueError(f"at most {_native.COLUMN_SUMS_MAX} columns")
    out = torch.zeros(cols, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        code = _native.load().lgc_column_sums(_native.ptr(table), table.stride(0) if n > 1 else cols, n, cols, _native.ptr(out),
                                              _native.stream_of(dev))
    _native.check(code, "lgc_column_sums")
    return out


def topk_coverage(topk: Tensor, cutoffs, n_items: int, bitmap: Optional[Tensor] = None):
    """(counts int64 [C], bitmap int32 [C, ceil(n_items / 32)]) on the device: per cutoff c the number of distinct items
    among the first c entries of all rows seen so far (lgc_topk_coverage).  Pass the returned ``bitmap`` to the next
    call to accumulate over requests; None starts from an empty catalogue.  An entry outside [0, n_items) marks nothing
    and raises at ``check_index_status()``."""
    _check_topk(topk)
    n, k, dev = topk.size(0), topk.size(1), topk.device
    cuts, cuts_c = _host_cutoffs(cutoffs, k)
    words = (int(n_items) + 31) // 32
    if n_items < 1:
        raise ValueError("no items to cover")
    if bitmap is None:
        bitmap = torch.zeros((len(cuts), words), dtype=torch.int32, device=dev)
    elif bitmap.dtype != torch.int32 or bitmap.shape != (len(cuts), words) or not bitmap.is_contiguous() or bitmap.device != dev:
        raise TypeError(f"bitmap must be a contiguous int32 [{len(cuts)}, {words}] tensor on {dev}")
    counts = torch.empty(len(cuts), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        code = _native.load().lgc_topk_coverage(_native.ptr(topk), topk.stride(0) if n > 1 else k, k, n, cuts_c, len(cuts),
                                                int(n_items), _native.ptr(bitmap), _native.ptr(counts),
                                                _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_topk_coverage")
    return counts, bitmap


class RankingResult:
    """What ``evaluate_ranking`` returns.  ``cutoffs``: the tuple of cutoffs; ``mean``: a dict from ``"precision"``,
    ``"recall"``, ``"ndcg"``, ``"map"``, ``"mrr"``, ``"hit_rate"``, ``"coverage"`` to a tuple with one Python float per
    cutoff (coverage = distinct recommended items / n_items); and, left on the device, ``users`` int64 [n], ``topk``
    int64 [n, max(cutoffs)], ``hits`` int32 [n, C], ``metrics`` float64 [n, C, 6] (``METRIC_NAMES``) and ``hit_bits``
    [n, 4] (see ``rank_metrics``)."""

    def __init__(self, cutoffs, mean, users, topk, hits, metrics, hit_bits):
        self.cutoffs, self.mean, self.users = tuple(cutoffs), mean, users
        self.topk, self.hits, self.metrics, self.hit_bits = topk, hits, metrics, hit_bits

    def __repr__(self) -> str:
        return f"RankingResult(cutoffs={self.cutoffs}, mean={self.mean})"


def evaluate_ranking(users_table: Tensor, items: Tensor, seen: Optional[SeenLists], users: Tensor, positives: PositiveLists,
                     cutoffs, workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, coverage: bool = True) -> RankingResult:
    """Precision, recall, NDCG, MAP, MRR, hit rate and catalogue coverage at every cutoff from ONE ranking pass at
    k = max(cutoffs): ``recommend_topk``, then lgc_rank_metrics, lgc_column_sums and (``coverage``) lgc_topk_coverage.
    The first c entries of a ranked row are its top-c row, so a smaller cutoff costs no second pass.  One host sync, at
    the end: the sums, the counts and the index status.  Precision and recall at a cutoff are the floats
    ``evaluate_topk(k=cutoff)`` returns.  Without users the means are NaN; without ``coverage`` that entry is NaN."""
    cuts = [int(c) for c in cutoffs]
    _host_cutoffs(cuts, TOPK_MAX)
    top = recommend_topk(users_table, users, items, seen, cuts[-1], workspace_bytes)
    return ranking_result(top, positives, users, cuts, items.size(0), coverage)


def ranking_result(top: Tensor, positives: PositiveLists, users: Tensor, cuts, n_items: int, coverage: bool = True,
                   short_rows: bool = False) -> RankingResult:
    """The metrics half of ``evaluate_ranking`` for ranked rows from ANY source (``top`` int64 [n, max(cuts)], ``cuts`` a
    list of ascending ints): lgc_rank_metrics, lgc_column_sums and (``coverage``) lgc_topk_coverage, one host sync.
    ``short_rows``: rows may end in -1, the empty places of a source with fewer than k candidates; they hit nothing (an
    entry is only compared), and what lgc_topk_coverage reports about them -- they mark nothing -- is dropped: the status
    word is put back to what it was before that launch."""
    n, dev, n_cut = users.numel(), users.device, len(cuts)
    hits, metrics, bits = rank_metrics(top, positives, users, cuts, return_bits=True)
    nan = tuple(float("nan") for _ in cuts)
    if n == 0:
        mean = {name: nan for name in METRIC_NAMES}
        mean["coverage"] = tuple(0.0 for _ in cuts) if coverage else nan
        return RankingResult(cuts, mean, users, top, hits, metrics, bits)
    # the hit counts ride along as exact doubles: precision's mean is then the integer sum over c * n, as evaluate_topk's
    sums = column_sums(torch.cat([metrics.view(n, n_cut * _native.RM_COUNT), hits.to(torch.float64)], dim=1))
    parts = [sums.view(torch.int64), _status(dev)[:1].to(torch.int64)]
    if coverage:
        before = _status(dev).clone() if short_rows else None
        parts.append(topk_coverage(top, cuts, n_items)[0])
        if short_rows:
            _status(dev).copy_(before)
    host = torch.cat(parts).cpu()                                        # the one sync
    width = n_cut * (_native.RM_COUNT + 1)
    if int(host[width]) & _native.ST_INDEX_OOB:
        try:
            check_index_status(dev)                                      # clears the word and its host snapshot
        except IndexError:
            pass
        raise IndexError("evaluation: a user id lies outside the user table or the positive lists")
    total = host[:width].view(torch.float64).tolist()
    mean = {name: tuple(total[ci * _native.RM_COUNT + m] / n for ci in range(n_cut)) for m, name in enumerate(METRIC_NAMES)}
    mean["precision"] = tuple(int(total[n_cut * _native.RM_COUNT + ci]) / (c * n) for ci, c in enumerate(cuts))
    mean["coverage"] = tuple(int(v) / n_items for v in host[width + 1:].tolist()) if coverage else nan
    return RankingResult(cuts, mean, users, top, hits, metrics, bits)


def overlap_items(topk: Tensor, hit_bits: Tensor, cutoff: Optional[int] = None) -> list:
    """Per row the entries of ``topk[r, :cutoff]`` whose bit is set in ``hit_bits``, in the ranking's order, as a Python
    list of lists: what upstream's ``list(set(a).intersection(b))`` holds.  One copy to the host."""
    import numpy as np
    n, k = topk.size(0), topk.size(1) if cutoff is None else int(cutoff)
    if hit_bits.shape != (n, TOPK_MAX // 64) or hit_bits.dtype != torch.int64 or not 1 <= k <= topk.size(1):
        raise ValueError(f"hit_bits must be int64 [{n}, {TOPK_MAX // 64}] and 1 <= cutoff <= {topk.size(1)}")
    host = torch.cat([topk[:, :k], hit_bits.to(topk.device)], dim=1).cpu().numpy()   # the one copy
    top, words = host[:, :k], np.ascontiguousarray(host[:, k:])
    flags = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :k].astype(bool)
    return [row[f].tolist() for row, f in zip(top, flags)]


def metrics_frame(pos_list_df, result: RankingResult, cutoff: Optional[int] = None):
    """The frame ``MARK_MAPK`` returns as its third value (src/lightgcn.py:184-190) at one cutoff of ``result`` (default:
    the largest): ``pos_list_df`` left-merged on ``user_id_idx`` with the columns ``user_ID``, ``top_rlvnt_itm`` (the
    first ``cutoff`` entries of the ranking), ``overlap_item``, ``recall`` and ``precision`` -- the same columns, dtypes
    and values, built from ``result.topk``, ``result.hit_bits`` and the two metric columns instead of a per-user set
    intersection.  ``overlap_item`` holds the same items as upstream's, in the RANKING's order: upstream's order is
    whatever iterating a Python ``set`` gives, which nothing should rely on."""
    import pandas as pd
    cutoff = result.cutoffs[-1] if cutoff is None else int(cutoff)
    if cutoff not in result.cutoffs:
        raise ValueError(f"cutoff {cutoff} is not one of {result.cutoffs}")
    ci = result.cutoffs.index(cutoff)
    cols = result.metrics[:, ci, [_native.RM_RECALL, _native.RM_PRECISION]].cpu().numpy()
    per_row = pd.DataFrame({"user_ID": result.users.cpu().numpy(),
                            "top_rlvnt_itm": result.topk[:, :cutoff].cpu().numpy().tolist(),
                            "overlap_item": overlap_items(result.topk, result.hit_bits, cutoff),
                            "recall": cols[:, 0], "precision": cols[:, 1]})
    per_row = per_row.drop_duplicates("user_ID", ignore_index=True)      # a user evaluated twice has two equal rows
    return pd.merge(pos_list_df, per_row, how="left", left_on="user_id_idx", right_on="user_ID")
