"""In-batch softmax loss: every user of a batch against every item the batch lists, many negatives per positive.

BPR trains each triple against one negative.  A batch, though, has already propagated the rows of ``B`` users, ``B``
positives and ``B`` negatives, and the sparse backward (``propagate.seeded_sum``) starts from any list of rows.  So a softmax
(InfoNCE / sampled-softmax) objective that scores each user against all ``C = 2B`` listed items needs the same forward rows
and a seed of ``3B`` ids against BPR's ``4B``; what it adds is ``lgc_softmax_batch``: the ``B x C``
logits on the fp32 matrix cores, a masked log-sum-exp per row and two small products for the gradient.  A user's own other
positives are no negatives: the mask is a lookup in the ignore lists ``TripleSampler`` keeps on the device.

Three parts: ``softmax_batch`` (the entry, with its workspace and status word), ``softmax_loss_reference`` (the same formula
in torch ops, differentiable, any dtype or device: the fallback and the tests' restatement) and ``softmax_from_table`` (the
autograd node ``LightGCN.softmax_loss`` runs, modelled on ``propagate.scores_from_table``).

What this does NOT do: the partitioned trainer and the multi-GPU step, seeds above ``LGC_SEED_MAX`` through the fused seed
kernels (they take ``seed_prepare``'s torch route), per-row candidate lists, cosine-normalised logits.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _native
from . import propagate as _prop          # its switches (SEED_ROWS_FACTOR ...) are read where they are used, as it reads them
from .graph import PropGraph
from .propagate import (RegHook, _layer_sum, _snapshot_status, _status, propagate_sum, raise_pending_index_error,
                        seeded_transpose_sum, segment_sum)

__all__ = ["softmax_batch", "softmax_loss_reference", "softmax_from_table", "SoftmaxBatch", "ignore_lists"]


class SoftmaxBatch(NamedTuple):
    """What ``softmax_batch`` returns, on the device: ``loss`` fp32 0-dim, ``row_loss`` fp32 [B], ``n_adm`` int32 [B] (the
    negatives a row admits), ``grad_users`` fp32 [B, D], ``grad_cands`` fp32 [C, D] and ``grad_logits`` fp32 [B, C] or None."""
    loss: Tensor
    row_loss: Tensor
    n_adm: Tensor
    grad_users: Tensor
    grad_cands: Tensor
    grad_logits: Optional[Tensor]


def ignore_lists(ignore) -> Optional[Tuple[Tensor, Tensor]]:
    """``(ign_ptr int32, ign_items int64)`` from a ``TripleSampler``, such a pair, or None."""
    if ignore is None:
        return None
    if hasattr(ignore, "ign_ptr") and hasattr(ignore, "ign_items"):
        ignore = (ignore.ign_ptr, ignore.ign_items)
    if not isinstance(ignore, (tuple, list)) or len(ignore) != 2 or not all(torch.is_tensor(t) for t in ignore):
        raise TypeError("ignore must be a TripleSampler, an (ign_ptr, ign_items) pair of tensors, or None")
    ptr, items = ignore
    if ptr.dtype != torch.int32 or ptr.dim() != 1 or ptr.numel() < 1:
        raise TypeError("ign_ptr must be a 1-D int32 tensor with one entry per user and one more")
    if items.dtype != torch.int64 or items.dim() != 1:
        raise TypeError("ign_items must be a 1-D int64 tensor of node ids")
    return ptr, items


def _check_inv_tau(inv_tau) -> float:
    if isinstance(inv_tau, bool) or not isinstance(inv_tau, (int, float)) or not math.isfinite(inv_tau) or not inv_tau > 0:
        raise ValueError(f"inv_tau must be a finite number > 0, got {inv_tau!r}")
    return float(inv_tau)


def _check_list(t, dtype, name: str) -> None:
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1:
        raise TypeError(f"{name} must be a 1-D {dtype} tensor")


def softmax_batch(table: Tensor, split: int, users: Tensor, cands: Tensor, target: Tensor, ign=None, inv_tau: float = 1.0,
                  size: Optional[int] = None, bias: Optional[Tensor] = None, return_logits_grad: bool = False) -> SoftmaxBatch:
    """``lgc_softmax_batch`` on the rows ``users`` (int64 node ids below ``split``) and ``cands`` (int64 node ids from
    ``split`` on) of ``table`` (fp32 ``[N, D]``, unit inner stride): the loss ``(1 / size) sum_i log sum_{j in J_i}
    exp(z_ij - z_it)`` with ``z = <e_u, e_c> * inv_tau + bias``, ``t = target[i]`` (int32) and ``J_i`` the columns row i
    admits -- its target, and every other candidate that is a valid item, not the target's item and not in the user's list
    of ``ign`` (``(ign_ptr, ign_items)`` or None) -- and the gradient with respect to the gathered rows.  ``size`` defaults
    to the number of rows.  A bad id gives a zero row and raises at ``check_index_status()``."""
    if not torch.is_tensor(table) or table.dtype != torch.float32 or table.dim() != 2:
        raise TypeError("table must be a 2-D float32 tensor")
    _native.require_device(table, "table")
    if table.size(1) < 1 or (table.size(0) > 1 and (table.stride(1) != 1 or table.stride(0) < table.size(1))):
        raise ValueError("table needs unit inner stride and a row stride >= dim")
    _check_list(users, torch.int64, "users")
    _check_list(cands, torch.int64, "cands")
    _check_list(target, torch.int32, "target")
    if target.numel() != users.numel():
        raise ValueError(f"{target.numel()} targets for {users.numel()} rows")
    n, dim, dev = table.size(0), table.size(1), table.device
    split = int(split)
    if not 0 <= split <= n:
        raise ValueError(f"split {split} outside [0, {n}]")
    inv_tau = _check_inv_tau(inv_tau)
    b, c = users.numel(), cands.numel()
    size = b if size is None else int(size)
    if size < 1:
        raise ValueError("size must be >= 1 (an empty batch has no loss)")
    ign = ignore_lists(ign)
    if ign is not None and ign[0].numel() != split + 1:
        raise ValueError(f"ign_ptr must have {split + 1} entries, one list per user; got {ign[0].numel()}")
    if bias is not None:
        _check_list(bias, torch.float32, "bias")
        if bias.numel() != c:
            raise ValueError(f"{bias.numel()} bias values for {c} candidates")
    for name, t in (("users", users), ("cands", cands), ("target", target), ("bias", bias),
                    ("ign_ptr", ign[0] if ign else None), ("ign_items", ign[1] if ign else None)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the table on {dev}")
    users, cands, target = users.contiguous(), cands.contiguous(), target.contiguous()
    ign_ptr = ign_items = None
    if ign is not None:                                    # an empty tensor has no address; the kernels read no entry of it
        ign_ptr = ign[0].contiguous()
        ign_items = ign[1].contiguous() if ign[1].numel() else torch.zeros(1, dtype=torch.int64, device=dev)
    if bias is not None:
        bias = bias.contiguous()
    lib = _native.load()
    f32 = dict(dtype=torch.float32, device=dev)
    head = torch.empty(1 + b, **f32)                       # [loss | row_loss]
    n_adm = torch.empty(b, dtype=torch.int32, device=dev)
    grads = torch.empty((b + c, dim), **f32)               # [grad_users | grad_cands]: the seed's value table as it stands
    logits_grad = torch.empty((b, c), **f32) if return_logits_grad else None
    if b == 0 or c == 0:                                   # nothing to score (an empty tensor has no address to pass): the
        for t in (head, n_adm, grads, logits_grad):        # entry's answer, a zero loss, and zeros in every other output
            if t is not None:
                t.zero_()
        return SoftmaxBatch(head[0], head[1:], n_adm, grads[:b], grads[b:], logits_grad)
    ws_bytes = lib.lgc_softmax_workspace_bytes(b, c)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    stride = table.stride(0) if n > 1 else dim
    with torch.cuda.device(dev):
        code = lib.lgc_softmax_batch(_native.ptr(table), stride, n, split, dim, _native.ptr(users), b, _native.ptr(cands), c,
                                     _native.ptr(target), _native.ptr(ign_ptr), _native.ptr(ign_items), _native.ptr(bias),
                                     inv_tau, size, head.data_ptr(), head.data_ptr() + 4, n_adm.data_ptr(),
                                     _native.ptr(logits_grad), c, grads.data_ptr(), grads.data_ptr() + 4 * b * dim, dim,
                                     _native.ptr(ws), ws_bytes, _native.ptr(_status(dev)), _native.stream_of(dev))
    _native.check(code, "lgc_softmax_batch")
    _snapshot_status(dev)
    return SoftmaxBatch(head[0], head[1:], n_adm, grads[:b], grads[b:], logits_grad)


def admissible_mask(users: Tensor, cands: Tensor, target: Tensor, ign, n: int, split: Optional[int] = None):
    """``(adm bool [B, C], valid_row bool [B])``: the admissible set of every row, in torch ops on the lists' device.  With
    ``split`` None an id is valid when it lies in ``[0, n)``."""
    b, c, dev = users.numel(), cands.numel(), users.device
    lo = 0 if split is None else int(split)
    target = target.to(torch.int64)
    cand_ok = (cands >= lo) & (cands < n)
    t_safe = target.clamp(0, max(c - 1, 0))
    t_item = cands[t_safe] if c else torch.zeros(b, dtype=torch.int64, device=dev)
    valid = (users >= 0) & (users < (n if split is None else lo)) & (target >= 0) & (target < c)
    if c:
        valid = valid & cand_ok[t_safe]
    cols = torch.arange(c, device=dev)
    is_t = cols[None, :] == target[:, None]
    adm = cand_ok[None, :] & (cands[None, :] != t_item[:, None])
    ign = ignore_lists(ign)
    if ign is not None and ign[1].numel():
        ptr, items = ign[0].to(torch.int64), ign[1]
        owner = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=dev), ptr[1:] - ptr[:-1])
        base = max(int(n), 1)
        keys = owner * base + items                        # ascending: the lists are, and so are their users
        u_safe = users.clamp(0, max(ptr.numel() - 2, 0))
        q = u_safe[:, None] * base + cands.clamp(0, base - 1)[None, :]
        pos = torch.searchsorted(keys, q).clamp(max=keys.numel() - 1)
        adm = adm & ~(keys[pos] == q)
    adm = (adm | is_t) & valid[:, None]
    return adm, valid


def softmax_loss_reference(emb: Tensor, users: Tensor, cands: Tensor, target: Tensor, ign=None, inv_tau: float = 1.0,
                           size: Optional[int] = None, bias: Optional[Tensor] = None, split: Optional[int] = None) -> Tensor:
    """``softmax_batch``'s loss in torch ops -- gather, ``mm``, a mask by ``searchsorted``, ``logsumexp`` -- differentiable
    by autograd with respect to ``emb`` (any float dtype, any device).  The fallback of ``softmax_from_table`` and the
    tests' restatement."""
    n = emb.size(0)
    adm, valid = admissible_mask(users, cands, target, ign, n, split)
    b = users.numel()
    size = b if size is None else int(size)
    if b == 0 or cands.numel() == 0:
        return emb.sum() * 0
    e_u = emb[users.clamp(0, n - 1)]
    e_c = emb[cands.clamp(0, n - 1)]
    z = (e_u @ e_c.t()) * inv_tau
    if bias is not None:
        z = z + bias.to(z.dtype)[None, :]
    t = target.to(torch.int64).clamp(0, cands.numel() - 1)
    neg_inf = torch.full((), float("-inf"), dtype=z.dtype, device=z.device)
    keep = adm | ~valid[:, None]                           # an invalid row keeps its logits so that no NaN enters autograd
    lse = torch.logsumexp(torch.where(keep, z, neg_inf), dim=1)
    row = lse - z.gather(1, t[:, None])[:, 0]
    return torch.where(valid, row, torch.zeros_like(row)).sum() / size


class _SoftmaxFromTable(torch.autograd.Function):
    """loss = softmax_batch(out, users, cands, ...) with out = sum_l alpha_l A^l w as ONE autograd node, modelled on
    ``propagate._ScoresFromTable``: the forward's last steps run for the listed rows only, one ``lgc_softmax_batch`` gives
    the loss and the gradient with respect to those rows, and the backward runs from that sparse seed.  The second output is
    the zero-valued ``token`` of the ``RegHook`` protocol."""

    @staticmethod
    def forward(ctx, w: Tensor, graph: PropGraph, alphas: tuple, users: Tensor, cands: Tensor, target: Tensor, ign, inv_tau: float,
                size: int, bias: Optional[Tensor], hook: Optional[RegHook]):
        rows = torch.cat([users, cands])
        emb = _layer_sum(graph, w.detach(), alphas, transpose=False, final_rows=rows)
        out = softmax_batch(emb, graph.split, users, cands, target, ign, inv_tau, size, bias)
        ctx.save_for_backward(rows, out.grad_users, out.grad_cands)
        ctx.graph, ctx.alphas, ctx.n, ctx.hook, ctx.width = graph, alphas, emb.size(0), hook, emb.size(1)
        ctx.set_materialize_grads(False)                                # an unused output arrives as None, not as zeros
        return out.loss.clone(), torch.zeros((), dtype=torch.float32, device=emb.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss: Optional[Tensor], grad_token: Optional[Tensor]):
        rows, grad_users, grad_cands = ctx.saved_tensors
        none = (None,) * 10
        hook = ctx.hook
        extra = []
        if hook is not None:
            hook.spent = True                                           # later regularisers take the plain torch path
            if grad_token is not None:
                w = hook.weight.detach()
                extra = [(r, w[r] * grad_token, scale) for r, scale in hook.terms]
        if grad_loss is None:                                            # only the regulariser was differentiated
            out = torch.zeros((ctx.n, ctx.width), dtype=torch.float32, device=rows.device)
            for r, v, scale in extra:
                r_s, perm = torch.sort(r, stable=True)
                segment_sum(r_s, r_s, v.contiguous(), out, scale=scale, accumulate=True, vals_index=perm.to(torch.int32))
            return (out, *none)
        # grad_users and grad_cands are one [B + C, D] block in the order of `rows`; an invalid id's row is zeros and its
        # id, outside the table, is "no row" for the seed
        vals = grad_users.as_strided((rows.numel(), ctx.width), (ctx.width, 1)) if _adjacent(grad_users, grad_cands) \
            else torch.cat([grad_users, grad_cands])
        return (seeded_transpose_sum(ctx.graph, rows, vals * grad_loss, ctx.alphas, ctx.n, extra), *none)


def _adjacent(a: Tensor, b: Tensor) -> bool:
    """Do the dense 2-D blocks ``a`` and ``b`` lie back to back in one storage (``softmax_batch`` allocates them so)?"""
    return (a.is_contiguous() and b.is_contiguous() and a.size(1) == b.size(1)
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.data_ptr() == a.data_ptr() + 4 * a.numel())


def softmax_from_table(w: Tensor, graph: PropGraph, alphas: Sequence[float], users: Tensor, cands: Tensor, target: Tensor,
                       ign=None, inv_tau: float = 1.0, size: Optional[int] = None, bias: Optional[Tensor] = None,
                       hook: Optional[RegHook] = None) -> Tensor:
    """The softmax loss of ``softmax_batch`` on ``propagate_sum(w, graph, alphas)``.  With gradients on, a user|item graph
    and a seed far smaller than the table (``scores_from_table``'s conditions) it runs as one node whose backward starts
    from the sparse seed; ``hook.token`` is filled in then.  Anything else is ``propagate_sum`` (or, without gradients, the
    listed-rows forward) followed by ``softmax_loss_reference``."""
    _native.require_device(w, "embedding table")
    for name, t in (("users", users), ("cands", cands), ("target", target)):
        _native.require_device(t, name)
    raise_pending_index_error(w.device)
    alphas = tuple(float(a) for a in alphas)
    inv_tau = _check_inv_tau(inv_tau)
    size = users.numel() if size is None else int(size)
    seed = users.numel() + cands.numel()
    bipartite = graph.split is not None and _prop.USE_BIPARTITE and len(alphas) - 1 <= _native.MAX_TERMS - 1
    small = seed * _prop.SEED_ROWS_FACTOR <= w.size(0)
    grads = torch.is_grad_enabled() and w.requires_grad
    if (_prop.SPARSE_BACKWARD and grads and bipartite and small and seed > 0 and size >= 1 and w.dtype == torch.float32):
        loss, token = _SoftmaxFromTable.apply(w, graph, alphas, users.contiguous(), cands.contiguous(), target.contiguous(),
                                              ign, inv_tau, size, bias, hook)
        if hook is not None:
            hook.token = token
        return loss
    if not grads and bipartite and small and _prop.SCORED_ROWS_ONLY and len(alphas) > 1 and seed > 0:
        rows = torch.cat([users, cands]).clamp(0, w.size(0) - 1)
        emb = _layer_sum(graph, w.detach().contiguous(), alphas, transpose=False, final_rows=rows)
    else:
        emb = propagate_sum(w, graph, alphas)
    return softmax_loss_reference(emb, users, cands, target, ign, inv_tau, size, bias, graph.split)
