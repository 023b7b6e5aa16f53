"""Drop-in ``LightGCN`` / ``BPRLoss`` for src/lightgcn.py (and its copy torchserve/lightgcn.py).

Public surface kept identical to the reference so that src/train_lightgcn.py,
src/inference_lightgcn.py and torchserve/lightgcn_handler.py run unchanged
(SURVEY.md section 8b): constructor arguments, the attributes callers read
(``embedding.weight``, ``alpha``, ``convs``, ``num_nodes`` ...), ``state_dict`` keys
(``alpha``, ``embedding.weight``), and the methods ``get_embedding``, ``forward``,
``predict_link``, ``recommend``, ``recommendK``, ``MARK_MAPK``, ``link_pred_loss``,
``recommendation_loss``.  ``recommend_topk`` and ``evaluateK`` are additions: the epoch's evaluation
(``recommendK`` over all validation users, then ``MARK_MAPK``) in bounded device memory; ``evaluate_metrics`` adds NDCG, MAP, MRR,
hit rate and coverage at several cutoffs from the same single ranking pass; ``recommendation_paths`` is one too: hop
distances and shortest paths from users to their recommended items (src/inference_lightgcn.py:85-119); ``embed_sessions`` and
``recommend_sessions`` answer for nodes outside the table -- new visitors, known users with a fresh list -- from their
interaction lists (``foldin``); ``explain_topk`` and ``explain_sessions`` split every recommended item's score over the user's
own items (``explain``); ``similar_items`` answers "which items are like this one?" (``similar``); ``recommend_diverse``,
``rerank_diverse`` and ``list_diversity`` re-rank a candidate list by greedy maximal marginal relevance and measure the
intra-list diversity of the result (``rerank``); ``recommend_filtered``, ``item_audience`` and ``similar_users`` retrieve across
two tables with a catalogue filter and per-request exclusion lists that REMOVE what they list (``retrieve``); ``bought_together`` answers "customers who bought this also bought" from the
purchase lists alone, without the embedding (``cooccur``), and ``recommend_itemknn`` ranks items for users and sessions from
those neighbour lists, the item-kNN baseline (``itemknn``).  What changes is underneath: propagation is the HIP CSR-SpMM with
the layer sum fused (``propagate.propagate_sum``) and pair scoring is one gather-dot kernel.
"""
from __future__ import annotations

import math
from typing import Optional, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn.modules.loss import _Loss

from . import _native
from .explain import Attribution, attribute
from .foldin import SessionLists, fold_in, fold_table
from .graph import get_graph
from .lgconv import LGConv
from .paths import shortest_paths
from .similar import METRICS, item_neighbors, row_rnorm
from .retrieve import BuyerLists, request_lists, retrieve_topk
from .cooccur import MEASURES, CoPurchase
from .itemknn import ItemKNN
from .fullrank import evaluate_full_rank
from .propagate import (DEFAULT_WORKSPACE_BYTES, TOPK_MAX, PositiveLists, RegHook, SeenLists, bpr_loss_fused, column_sums,
                        evaluate_ranking, evaluate_topk, mask_topk, pair_dot, propagate_sum, recommend_topk,
                        regularization_through, routable_index, scores_from_table)
from .rerank import check_lam, list_diversity, mmr_rerank
from .softmax import ignore_lists, softmax_from_table

RERANK_MAX_CAND = _native.RERANK_MAX_CAND

__all__ = ["LightGCN", "BPRLoss", "LGConv", "regularization_loss"]


def _is_sparse_tensor(obj) -> bool:
    # torch_sparse is optional; only used to mirror the isinstance branch of src/lightgcn.py:116
    return type(obj).__name__ == "SparseTensor" and hasattr(obj, "coo")


class LightGCN(torch.nn.Module):
    """x_i = sum_l alpha_l x_i^(l),  x^(l+1) = D^-1/2 A D^-1/2 x^(l)   (He et al., 2020).

    Args mirror src/lightgcn.py:58-65: ``num_nodes``, ``embedding_dim``, ``num_layers``,
    ``alpha`` (None -> uniform 1/(K+1); float -> repeated; Tensor of K+1 entries), and
    ``**kwargs`` forwarded to every ``LGConv``.
    """

    def __init__(self, num_nodes: int, embedding_dim: int, num_layers: int,
                 alpha: Optional[Union[float, Tensor]] = None, **kwargs):
        super().__init__()
        self.num_nodes, self.embedding_dim, self.num_layers = num_nodes, embedding_dim, num_layers
        if alpha is None:
            alpha = 1. / (num_layers + 1)
        if isinstance(alpha, Tensor):
            assert alpha.size(0) == num_layers + 1
        else:
            alpha = torch.tensor([alpha] * (num_layers + 1))
        self.register_buffer('alpha', alpha)
        self.embedding = torch.nn.Embedding(num_nodes, embedding_dim)
        self.convs = torch.nn.ModuleList(LGConv(**kwargs) for _ in range(num_layers))
        self._alpha_host = None
        # serving: recommendK reuses the propagated table while neither the graph, the
        # weights nor alpha changed; set to False to recompute on every request like the reference
        self.cache_recommend_embeddings = True
        self._served = None
        self._fold = None                 # foldin.fold_table's table, kept under the same key as _served
        self.fold_tables_built = 0        # how often it was computed (cache hits do not count)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.embedding.weight)
        for conv in self.convs:
            conv.reset_parameters()

    # -- hot path ------------------------------------------------------------------------
    def _alphas(self) -> tuple:
        """Host copy of the alpha buffer (kernel arguments), refreshed when the buffer changes."""
        a = self.alpha
        tag = (a.data_ptr(), a._version, a.device)
        if self._alpha_host is None or self._alpha_host[0] != tag:
            self._alpha_host = (tag, tuple(float(v) for v in a.detach().cpu().tolist()))
        return self._alpha_host[1]

    def get_embedding(self, edge_index, edge_weight) -> Tensor:
        """All K hops and the weighted layer sum in K kernel sequences (src/lightgcn.py:91-99)."""
        x0 = self.embedding.weight
        _native.require_device(x0, "LightGCN.embedding.weight")
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        return propagate_sum(x0, graph, self._alphas())

    def _serving_embedding(self, edge_index, edge_weight) -> Tensor:
        """The propagated table for read-only use by ``recommendK``.

        Upstream recomputes all K layers for every request (torchserve/lightgcn_handler.py:91 ->
        src/lightgcn.py:171) although, with gradients off, the result depends only on the graph, the weight
        table and alpha.  It is kept here until one of them changes (tensor identity + version counter; an
        optimizer step or load_state_dict bumps the weight's version)."""
        w = self.embedding.weight
        if torch.is_grad_enabled() or not self.cache_recommend_embeddings:
            return self.get_embedding(edge_index, edge_weight)
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        key = (id(graph), w.data_ptr(), w._version, w.device, self._alphas())
        if self._served is None or self._served[0] != key:
            self._served = (key, graph, self.get_embedding(edge_index, edge_weight))
        return self._served[2]

    def invalidate(self) -> None:
        """Forget every derived table: the cached graphs of this process and the propagated table ``recommendK``
        reuses and the fold-in table beside it.  The caches key on tensor identity + version counter, which in-place torch ops bump; call this after
        writes that do not (``weight.data.copy_``, a DLPack/numpy alias, a foreign kernel).  The reference re-derives
        everything on every call."""
        from .graph import clear_cache
        clear_cache()
        self._served = None
        self._fold = None
        self._alpha_host = None

    def forward(self, edge_index, edge_label_index: Optional[Tensor] = None,
                edge_weight: Optional[Tensor] = None) -> Tensor:
        """Scores of the node pairs in ``edge_label_index`` (default: the graph's own edges)."""
        if edge_label_index is None:
            if _is_sparse_tensor(edge_index):
                edge_label_index = torch.stack(edge_index.coo()[:2], dim=0)
            else:
                edge_label_index = edge_index
        x0 = self.embedding.weight
        _native.require_device(x0, "LightGCN.embedding.weight")
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        hook = RegHook(x0) if (torch.is_grad_enabled() and x0.requires_grad) else None
        scores = scores_from_table(x0, graph, self._alphas(), edge_label_index, hook)
        # a regulariser on the layer-0 rows of this step (regularization_loss below) routes its gradient through the
        # scoring node of THIS forward; None when the scores took the dense two-node path
        x0._lgcn_reg_hook = hook if (hook is not None and hook.token is not None) else None
        return scores

    # -- heads built on it -----------------------------------------------------------------
    def predict_link(self, edge_index, edge_label_index: Optional[Tensor] = None, prob: bool = False) -> Tensor:
        pred = self(edge_index, edge_label_index).sigmoid()
        return pred if prob else pred.round()

    def recommend(self, edge_index, src_index: Optional[Tensor] = None, dst_index: Optional[Tensor] = None,
                  k: int = 1) -> Tensor:
        # Upstream calls get_embedding(edge_index) here without the edge_weight its own signature
        # requires (src/lightgcn.py:153 vs :91) and so raises TypeError; kept bug-for-bug.
        out_src = out_dst = self.get_embedding(edge_index)
        if src_index is not None:
            out_src = out_src[src_index]
        if dst_index is not None:
            out_dst = out_dst[dst_index]
        top_index = (out_src @ out_dst.t()).topk(k, dim=-1).indices
        if dst_index is not None:
            top_index = dst_index[top_index.view(-1)].view(*top_index.size())
        return top_index

    def recommendK(self, edge_index, edge_weight, n_users, n_items, interactions_t, user_id_list, k: int = 5):
        """Top-k unseen items per user as the DataFrame src/lightgcn.py:169-182 returns
        (columns ``user_ID``, ``top_rlvnt_itm``); seen items are zeroed, not removed, as upstream."""
        import pandas as pd
        embeds = self._serving_embedding(edge_index, edge_weight)
        users, items = torch.split(embeds, [n_users, n_items])
        # Scores, the multiplicative seen-mask and the top-k all stay on the device: only the [n_sel, k] indices
        # come back (upstream ships the whole [n_sel, n_items] score matrix to the host first, :174).  Same fp32
        # products as ``torch.mul(pred.cpu(), 1 - interactions_t)``; the mask may already live on the device.
        sel = torch.as_tensor(user_id_list, device=embeds.device) if not torch.is_tensor(user_id_list) \
            else user_id_list.to(embeds.device)
        sel = sel.reshape(-1).long()
        pred = users.index_select(0, sel) @ items.t()
        if isinstance(interactions_t, SeenLists):                    # purchase lists on the device: no dense mask at all
            if k > TOPK_MAX:
                raise ValueError(f"the list form of the mask supports k <= {TOPK_MAX}")
            top_index = mask_topk(pred, interactions_t.for_users(sel), k).cpu()
            return pd.DataFrame({'user_ID': list(user_id_list), 'top_rlvnt_itm': top_index.numpy().tolist()})
        seen = interactions_t.to(device=embeds.device, dtype=pred.dtype, non_blocking=True)
        if k <= TOPK_MAX:
            top_index = mask_topk(pred, seen.expand_as(pred).contiguous(), k).cpu()       # one launch: lgc_mask_topk
        else:
            top_index = torch.mul(pred, (1 - seen)).topk(k, dim=-1).indices.cpu()
        if isinstance(user_id_list, (list, tuple)):
            # the frame upstream builds in three steps (:178-182), built directly: same columns, dtypes, index, values
            return pd.DataFrame({'user_ID': list(user_id_list), 'top_rlvnt_itm': top_index.numpy().tolist()})
        frame = pd.DataFrame(top_index.numpy())           # anything index-carrying (a Series): upstream's own steps
        frame['top_rlvnt_itm'] = frame.values.tolist()
        frame['user_ID'] = user_id_list
        return frame[['user_ID', 'top_rlvnt_itm']]

    def MARK_MAPK(self, test_pos_list_df, top_index_df, k):
        import pandas as pd
        m = pd.merge(test_pos_list_df, top_index_df, how='left', left_on='user_id_idx', right_on='user_ID')
        m['overlap_item'] = [list(set(a).intersection(b)) for a, b in zip(m.item_id_idx_list, m.top_rlvnt_itm)]
        m['recall'] = m.apply(lambda x: len(x['overlap_item']) / len(x['item_id_idx_list']), axis=1)
        m['precision'] = m.apply(lambda x: len(x['overlap_item']) / k, axis=1)
        return m['precision'].mean(), m['recall'].mean(), m

    def _eval_tables(self, edge_index, edge_weight, n_users, n_items, seen, users):
        """(user table, item table, SeenLists or None, user ids int64 on the device) for the two methods below."""
        embeds = self._serving_embedding(edge_index, edge_weight).detach()
        user_t, item_t = torch.split(embeds, [n_users, n_items])
        ids = users if torch.is_tensor(users) else torch.as_tensor(list(users), dtype=torch.int64)
        ids = ids.reshape(-1).to(device=embeds.device, dtype=torch.int64).contiguous()
        if seen is not None and not isinstance(seen, SeenLists):         # the reference's dense mask, rows positional in users
            seen = SeenLists.from_dense(seen, ids if torch.is_tensor(users) else users, n_users, device=embeds.device)
        return user_t, item_t, seen, ids

    def recommend_topk(self, edge_index, edge_weight, n_users, n_items, seen, users, k: int = 5,
                       workspace_bytes: int = DEFAULT_WORKSPACE_BYTES) -> Tensor:
        """``recommendK``'s ranking as int64 ``[len(users), k]`` item indices on the device, no DataFrame, in bounded
        memory: scores exist one panel of ``workspace_bytes`` at a time (``propagate.recommend_topk``).  ``seen``: a
        ``SeenLists``, the reference's dense 0/1 mask (converted once, ``SeenLists.from_dense``) or None."""
        user_t, item_t, seen, ids = self._eval_tables(edge_index, edge_weight, n_users, n_items, seen, users)
        return recommend_topk(user_t, ids, item_t, seen, k, workspace_bytes)

    def evaluateK(self, edge_index, edge_weight, n_users, n_items, seen, users, positives, k: int = 20,
                  workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        """``(precision, recall, hits)``: what ``recommendK`` + ``MARK_MAPK`` report for ``users`` (None: the users of
        ``positives``, in its order) -- the two means as Python floats, the per-user hit counts as an int32 tensor left
        on the device.  ``positives``: a ``PositiveLists`` or a ``*_pos_list_df``.  Scores, ranking, hits and the two
        sums stay on the device; there is one host sync, at the end."""
        if not isinstance(positives, PositiveLists):
            positives = PositiveLists.from_frame(positives, n_users)
        if users is None:
            users = positives.users
        user_t, item_t, seen, ids = self._eval_tables(edge_index, edge_weight, n_users, n_items, seen, users)
        if positives.ptr.device != ids.device:
            positives = positives.to(ids.device)
        return evaluate_topk(user_t, item_t, seen, ids, positives, k, workspace_bytes)

    def evaluate_metrics(self, edge_index, edge_weight, n_users, n_items, seen, users, positives, ks=(5, 10, 20),
                         workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, coverage: bool = True):
        """Precision, recall, NDCG, MAP, MRR, hit rate and catalogue coverage at every cutoff of ``ks`` (ascending) from
        ONE ranking pass at ``max(ks)``; arguments as ``evaluateK``.  Returns a ``propagate.RankingResult``: ``mean``
        (a dict of tuples, one Python float per cutoff) and the per-user device tensors ``topk``, ``hits``, ``metrics``
        and ``hit_bits``.  Precision and recall at a cutoff are ``evaluateK``'s floats at that k.  One host sync."""
        if not isinstance(positives, PositiveLists):
            positives = PositiveLists.from_frame(positives, n_users)
        if users is None:
            users = positives.users
        user_t, item_t, seen, ids = self._eval_tables(edge_index, edge_weight, n_users, n_items, seen, users)
        if positives.ptr.device != ids.device:
            positives = positives.to(ids.device)
        return evaluate_ranking(user_t, item_t, seen, ids, positives, ks, workspace_bytes, coverage)

    def evaluate_full_rank(self, edge_index, edge_weight, n_users, n_items, seen, users, positives, ks=(20,),
                           seen_mode: str = "zero"):
        """AUC, mean percentile rank, MRR and recall / hit rate at every K of ``ks`` (any K up to ``n_items``) from the exact
        catalogue rank of every distinct held-out item; arguments as ``evaluate_metrics``.  ``seen_mode`` "zero" ranks as
        ``recommendK`` does (a seen item competes with score * 0), "remove" takes the seen items out of the candidates.
        Returns a ``fullrank.FullRankResult``.  One host sync at the end, plus the read of the number of pairs wherever
        ``users`` is not the device tensor of the previous call (``fullrank.evaluate_full_rank``)."""
        if not isinstance(positives, PositiveLists):
            positives = PositiveLists.from_frame(positives, n_users)
        if users is None:
            users = positives.users
        user_t, item_t, seen, ids = self._eval_tables(edge_index, edge_weight, n_users, n_items, seen, users)
        if positives.ptr.device != ids.device:
            positives = positives.to(ids.device)
        return evaluate_full_rank(user_t, item_t, seen, ids, positives, ks, seen_mode)

    def recommendation_paths(self, edge_index, edge_weight, n_users, users, top_items, max_len: int = 7,
                             workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, trace: Optional[list] = None):
        """``(path_lens int32 [S, k], longer_than_3 bool [S], paths int64 [S, k, max_len + 1])`` on the device: what
        ``InferenceLightGCN.compute_paths`` (src/inference_lightgcn.py:85-119) derives per user from ``top_items`` --
        ``recommend_topk``'s item indices, without offset -- in graph node ids (items offset by ``n_users``).  See
        ``paths.shortest_paths``: -1 and an all -1 row for an item without a path, the distance and an all -1 row for
        one farther than ``max_len``."""
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        ids = users if torch.is_tensor(users) else torch.as_tensor(list(users), dtype=torch.int64)
        ids = ids.reshape(-1).to(device=graph.device, dtype=torch.int64).contiguous()
        targets = (top_items.to(device=graph.device, dtype=torch.int64) + int(n_users)).contiguous()
        dist, paths = shortest_paths(graph, ids, targets, max_len=max_len, workspace_bytes=workspace_bytes, trace=trace)
        return dist, (dist > 3).any(dim=1), paths

    # -- nodes outside the table: fold-in -------------------------------------------------------
    def embed_sessions(self, edge_index, edge_weight, n_users, n_items, sessions: SessionLists, init_users=None) -> Tensor:
        """fp32 ``[n_rows, D]``: for every interaction list of ``sessions`` the embedding ``get_embedding`` would give a
        node appended to the graph with one-way edges from the listed items (``foldin``) -- a visitor the model was not
        trained on.  ``init_users`` (int64 tensor or list, one id per session): the trained user whose layer-0 row the
        node starts from -- a known user with a fresh list; with its own edge list the result is its served row --,
        -1 for an unknown visitor (a zero row); None = all unknown."""
        w = self.embedding.weight
        _native.require_device(w, "LightGCN.embedding.weight")
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        n_users, n_items = int(n_users), int(n_items)
        if graph.split != n_users or n_users + n_items != self.num_nodes:
            raise ValueError(f"fold-in needs the user|item graph split at n_users: split {graph.split}, n_users {n_users}, "
                             f"n_items {n_items}, {self.num_nodes} nodes")
        fold = fold_table(self, graph)
        sessions.validate(n_items)
        init_table = init_rows = None
        if init_users is not None:
            if not torch.is_tensor(init_users):
                ids = [int(u) for u in init_users]
                if any(u < -1 or u >= n_users for u in ids):
                    raise ValueError(f"init_users must be -1 or lie in [0, {n_users})")
                init_users = torch.tensor(ids, dtype=torch.int64)
            init_rows = init_users.reshape(-1).to(device=w.device, dtype=torch.int64).contiguous()
            init_table = w.detach()[:n_users]
        return fold_in(fold, graph.dis[n_users:] if graph.normalize else None, sessions, init_table, init_rows,
                       self._alphas()[0], graph.normalize)

    def recommend_sessions(self, edge_index, edge_weight, n_users, n_items, sessions: SessionLists, init_users=None,
                           k: int = 20, mask="purchased", return_values: bool = False,
                           workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        """int64 ``[n_rows, k]`` item indices on the device: ``recommend_topk`` with the folded rows of
        ``embed_sessions`` as the user table.  ``mask``: which of a session's own items are zeroed like seen items --
        ``"purchased"`` (weight 1.0, upstream's rule for the seen matrix), ``"all"`` or None.  The score matrix exists
        one panel of ``workspace_bytes`` at a time; with ``return_values`` also the masked scores."""
        rows = self.embed_sessions(edge_index, edge_weight, n_users, n_items, sessions, init_users)
        item_t = self._serving_embedding(edge_index, edge_weight).detach()[int(n_users):]
        sel = torch.arange(rows.size(0), dtype=torch.int64, device=rows.device)
        return recommend_topk(rows, sel, item_t, sessions.mask(mask), k, workspace_bytes, return_values)

    # -- which of the user's own items produced a recommendation ---------------------------------
    def _explain_tables(self, edge_index, edge_weight, n_users, n_items, top_items):
        """(graph, fold table, served item rows, targets int64 [rows, k] on the device) for the two methods below."""
        w = self.embedding.weight
        _native.require_device(w, "LightGCN.embedding.weight")
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        n_users, n_items = int(n_users), int(n_items)
        if graph.split != n_users or n_users + n_items != self.num_nodes:
            raise ValueError(f"fold-in needs the user|item graph split at n_users: split {graph.split}, n_users {n_users}, "
                             f"n_items {n_items}, {self.num_nodes} nodes")
        fold = fold_table(self, graph)
        item_t = self._serving_embedding(edge_index, edge_weight).detach()[n_users:]
        targets = top_items if torch.is_tensor(top_items) else torch.as_tensor(top_items, dtype=torch.int64)
        if targets.dim() != 2:
            raise ValueError("top_items must be [rows, k] item indices")
        targets = targets.to(device=w.device, dtype=torch.int64).contiguous()
        return graph, fold, item_t, targets

    def explain_topk(self, edge_index, edge_weight, n_users, n_items, users, top_items, m: int = 3,
                     full: bool = False) -> Attribution:
        """For trained ``users`` and their recommended ``top_items`` (``recommend_topk``'s item indices, int64
        ``[len(users), k]``): every score ``<e_u, E[t]>`` split over the user's own edge list -- ``base`` (the share of
        the user's layer-0 row), ``total`` (base + all contributions = the score, to rounding) and per recommended item
        the ``m`` items of the user's list that contributed most (``top_pos`` the position in the user's CSR row,
        ``top_item``, ``top_value``); with ``full`` every contribution (``contrib``, ``contrib_ptr``; sizing it is the one
        host sync).  The attribution is of the raw, UNMASKED score: ``recommendK`` zeroes a seen item's score rather than
        removing it, so a seen item's explanation is of the score before the mask.  See ``explain.attribute``."""
        graph, fold, item_t, targets = self._explain_tables(edge_index, edge_weight, n_users, n_items, top_items)
        n_users = int(n_users)
        ids = users if torch.is_tensor(users) else torch.as_tensor(list(users), dtype=torch.int64)
        ids = ids.reshape(-1).to(device=fold.device, dtype=torch.int64).contiguous()
        op = graph.forward_op
        contrib_ptr = None
        if full:                                             # row lengths -> first entry slot of every row, on the device
            safe = ids.clamp(0, n_users - 1)
            counts = (op.rowptr[safe + 1] - op.rowptr[safe]).to(torch.int64)
            counts = torch.where((ids >= 0) & (ids < n_users), counts, torch.zeros_like(counts))
            contrib_ptr = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=ids.device)
            contrib_ptr[1:] = torch.cumsum(counts, 0)
        return attribute(fold, item_t, targets, rowptr=op.rowptr[:n_users + 1], entries=op.entries, row_ids=ids,
                         col_base=n_users, contrib_ptr=contrib_ptr, init_table=self.embedding.weight.detach()[:n_users],
                         init_rows=ids, a0=self._alphas()[0], m=m, full=full)

    def explain_sessions(self, edge_index, edge_weight, n_users, n_items, sessions: SessionLists, top_items, init_users=None,
                         m: int = 3, full: bool = False) -> Attribution:
        """The same for interaction lists (``embed_sessions``' arguments): the scores of ``recommend_sessions``' rows
        split over each session's own list, with fold-in's coefficients.  The attribution is of the raw, UNMASKED
        score: a session item zeroed by the mask is explained by its score before the mask."""
        graph, fold, item_t, targets = self._explain_tables(edge_index, edge_weight, n_users, n_items, top_items)
        n_users = int(n_users)
        sessions.validate(int(n_items))
        init_table = init_rows = None
        if init_users is not None:
            if not torch.is_tensor(init_users):
                ids = [int(u) for u in init_users]
                if any(u < -1 or u >= n_users for u in ids):
                    raise ValueError(f"init_users must be -1 or lie in [0, {n_users})")
                init_users = torch.tensor(ids, dtype=torch.int64)
            init_rows = init_users.reshape(-1).to(device=fold.device, dtype=torch.int64).contiguous()
            init_table = self.embedding.weight.detach()[:n_users]
        return attribute(fold, item_t, targets, sessions=sessions, item_dis=graph.dis[n_users:] if graph.normalize else None,
                         normalize=graph.normalize, init_table=init_table, init_rows=init_rows, a0=self._alphas()[0], m=m,
                         full=full)

    # -- which items are like this one ------------------------------------------------------------
    def similar_items(self, edge_index, edge_weight, n_users, n_items, item_ids=None, k: int = 10, metric: str = "cosine",
                      item_ok=None):
        """``(index int64 [n, k], value fp32 [n, k])`` on the device: per item of ``item_ids`` (item indices WITHOUT the
        ``n_users`` offset, as in fold-in; None = the whole catalogue in order) the ``k`` most similar other items by
        ``metric`` ("cosine" or "dot") over the item rows of the cached serving embedding -- the table ``recommendK``
        scores against.  ``item_ok``: bool or uint8 ``[n_items]``, items that may be returned (None = all).  The order is
        ``recommend_topk``'s (descending, equal values by ascending index); with fewer than k other items a row ends
        in -1 / -inf.  An id outside ``[0, n_items)`` gives such a row and raises at ``check_index_status()``.  See
        ``similar.item_neighbors``."""
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 0 or n_items < 1 or n_users + n_items != self.num_nodes:
            raise ValueError(f"n_users {n_users} + n_items {n_items} != {self.num_nodes} nodes")
        _native.require_device(self.embedding.weight, "LightGCN.embedding.weight")
        with torch.no_grad():                                # read-only: the table recommendK keeps between requests
            item_t = self._serving_embedding(edge_index, edge_weight).detach()[n_users:]
        ids = None
        if item_ids is not None:
            ids = item_ids if torch.is_tensor(item_ids) else torch.as_tensor(list(item_ids), dtype=torch.int64)
            ids = ids.reshape(-1).to(device=item_t.device, dtype=torch.int64).contiguous()
        if item_ok is not None:
            item_ok = torch.as_tensor(item_ok).to(device=item_t.device).contiguous()
        return item_neighbors(item_t, k, ids, metric, item_ok, True, 0)

    # -- filtered retrieval across two tables ------------------------------------------------------
    def _retrieve_tables(self, edge_index, edge_weight, n_users, n_items, k):
        """(user rows, item rows) of the cached serving embedding, after the checks the three methods below share."""
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 1 or n_items < 1 or n_users + n_items != self.num_nodes:
            raise ValueError(f"n_users {n_users} + n_items {n_items} != {self.num_nodes} nodes")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.RETRIEVE_MAX_K:
            raise ValueError(f"k must be an integer in [1, {_native.RETRIEVE_MAX_K}]")
        _native.require_device(self.embedding.weight, "LightGCN.embedding.weight")
        with torch.no_grad():                                # read-only: the table recommendK keeps between requests
            return torch.split(self._serving_embedding(edge_index, edge_weight).detach(), [n_users, n_items])

    @staticmethod
    def _ok_mask(ok, n: int, name: str):
        if ok is None:
            return None
        ok = torch.as_tensor(ok)
        if ok.dtype not in (torch.bool, torch.uint8) or ok.dim() != 1 or ok.numel() != n:
            raise TypeError(f"{name} must be a bool or uint8 tensor of {n} entries")
        return ok

    @staticmethod
    def _id_tensor(ids, name: str) -> Tensor:
        t = ids if torch.is_tensor(ids) else torch.as_tensor(list(ids), dtype=torch.int64)
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be int64 indices")
        return t.reshape(-1)

    def recommend_filtered(self, edge_index, edge_weight, n_users, n_items, seen, users, k: int = 20, item_ok=None,
                           exclude=None, queries: Optional[Tensor] = None):
        """``(index int64 [n, k], value fp32 [n, k])`` on the device: per user of ``users`` the k best items that are in
        stock and new to the user.  ``seen``: a ``SeenLists`` (or None) whose items are REMOVED -- they never compete,
        unlike in ``recommend_topk``, where a seen item keeps upstream's score 0.  ``item_ok``: bool or uint8
        ``[n_items]``, an item whose entry is 0 is returned to nobody.  ``exclude``: per request row a list of further item
        indices (what is in the cart) or None, merged into the row's list.  With fewer than k eligible items a row ends in
        -1 / -inf.  Session form: ``queries`` = the folded rows of ``embed_sessions`` (fp32 ``[n, D]``), ``users`` None and
        ``seen`` = ``SessionLists.mask()``, whose list r belongs to row r.  See ``retrieve.retrieve_topk``."""
        if seen is not None and not isinstance(seen, SeenLists):
            raise TypeError("seen must be a SeenLists or None (SeenLists.from_dense converts the dense mask)")
        item_ok = self._ok_mask(item_ok, int(n_items), "item_ok")
        if (queries is None) == (users is None):
            raise ValueError("give users (trained rows) or queries (folded rows), not both")
        ids = None if users is None else self._id_tensor(users, "users")
        user_t, item_t = self._retrieve_tables(edge_index, edge_weight, n_users, n_items, k)
        dev = item_t.device
        if queries is not None:
            if not torch.is_tensor(queries) or queries.dim() != 2 or queries.size(1) != item_t.size(1):
                raise TypeError(f"queries must be fp32 [n, {item_t.size(1)}] rows")
            table, n = queries.to(device=dev, dtype=torch.float32), queries.size(0)
        else:
            ids = ids.to(dev).contiguous()
            table, n = user_t, ids.numel()
        if item_ok is not None:
            item_ok = item_ok.to(dev).contiguous()
        lists = list_rows = None
        if exclude is not None or (queries is not None and seen is not None):
            # the row's own ascending list: the union with `exclude`; a session's list comes in the visitor's order
            lists = request_lists(seen, ids, n, exclude, int(n_items), dev)
            list_rows = torch.arange(n, dtype=torch.int64, device=dev)
        elif seen is not None:
            lists = (seen.ptr.to(dev), seen.items.to(dev))    # list = the user's id
        return retrieve_topk(table, item_t, k, ids, cand_ok=item_ok, lists=lists, list_rows=list_rows)

    def item_audience(self, edge_index, edge_weight, n_users, n_items, item_ids, k: int = 20, buyers=None, user_ok=None):
        """``(index int64 [n, k], value fp32 [n, k])`` on the device: per item of ``item_ids`` (item indices WITHOUT the
        ``n_users`` offset) the k users whose rows score it best -- the audience of a product.  ``buyers``: a
        ``BuyerLists`` whose users are removed from their items' answers; None builds it from ``edge_index`` (an int64
        ``[2, E]`` tensor; anything else needs ``buyers``).  ``user_ok``: bool or uint8 ``[n_users]``, a user whose entry is
        0 (opted out) is returned for nothing.  One pass over the user table; see ``retrieve.retrieve_topk``."""
        user_ok = self._ok_mask(user_ok, int(n_users), "user_ok")
        ids = self._id_tensor(item_ids, "item_ids")
        if buyers is not None and not isinstance(buyers, BuyerLists):
            raise TypeError("buyers must be a BuyerLists or None")
        user_t, item_t = self._retrieve_tables(edge_index, edge_weight, n_users, n_items, k)
        dev = user_t.device
        if buyers is None:
            if not (torch.is_tensor(edge_index) and edge_index.dim() == 2):
                raise ValueError("buyers=None needs edge_index as an int64 [2, E] tensor (BuyerLists.from_edges)")
            buyers = BuyerLists.from_edges(edge_index, int(n_users), int(n_items), dev)
        if user_ok is not None:
            user_ok = user_ok.to(dev).contiguous()
        return retrieve_topk(item_t, user_t, k, ids.to(dev).contiguous(), cand_ok=user_ok,
                             lists=(buyers.ptr.to(dev), buyers.items.to(dev)))

    def similar_users(self, edge_index, edge_weight, n_users, n_items, user_ids, k: int = 10, metric: str = "cosine",
                      user_ok=None):
        """``(index int64 [n, k], value fp32 [n, k])`` on the device: per user of ``user_ids`` the k most similar OTHER
        users by ``metric`` ("cosine" or "dot") over the user rows of the serving embedding -- lookalike users.
        ``user_ok`` as in ``item_audience``.  The order and the tail of a short row are ``similar_items``'."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        user_ok = self._ok_mask(user_ok, int(n_users), "user_ok")
        ids = self._id_tensor(user_ids, "user_ids")
        user_t, _ = self._retrieve_tables(edge_index, edge_weight, n_users, n_items, k)
        dev = user_t.device
        ids = ids.to(dev).contiguous()
        scale = row_rnorm(user_t) if metric == "cosine" else None
        if user_ok is not None:
            user_ok = user_ok.to(dev).contiguous()
        return retrieve_topk(user_t, user_t, k, ids, scale, scale, user_ok, skip_id=ids)

    # -- customers who bought this also bought -----------------------------------------------------
    def bought_together(self, edge_index, edge_weight, n_users, n_items, item_ids=None, k: int = 10, measure: str = "cosine",
                        min_count: int = 1, item_ok=None, seen=None):
        """``(index int64 [n, k], value fp32 [n, k], count int32 [n, k])`` on the device: per item of ``item_ids`` (item
        indices WITHOUT the ``n_users`` offset; None = the whole catalogue in order) the k items that share most buyers with
        it, by ``measure`` ("count", "cosine" or "jaccard" over the buyer counts), and the number of shared buyers of each.
        With ``seen`` (a ``SeenLists``) those purchase lists are used; without it every edge of ``edge_index`` (an int64
        ``[2, E]`` tensor) is a purchase.  An item that shares fewer than ``min_count`` buyers, or whose ``item_ok`` entry
        (bool or uint8 ``[n_items]``) is 0, is never returned; short rows end in -1 / -inf / 0.  It reads no embedding and
        triggers no propagation: ``edge_weight`` is unused, and the answer is the same before the first training step.
        The lists are transposed on every call; hold a ``cooccur.CoPurchase`` to ask many times.  See
        ``cooccur.cooccur_topk``."""
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 1 or n_items < 1 or n_users + n_items != self.num_nodes:
            raise ValueError(f"n_users {n_users} + n_items {n_items} != {self.num_nodes} nodes")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.COOCCUR_MAX_K:
            raise ValueError(f"k must be an integer in [1, {_native.COOCCUR_MAX_K}]")
        if not isinstance(measure, str) or measure not in MEASURES:
            raise ValueError(f"measure must be one of {list(MEASURES)}, got {measure!r}")
        if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
            raise ValueError("min_count must be an integer of at least 1")
        item_ok = self._ok_mask(item_ok, n_items, "item_ok")
        ids = None if item_ids is None else self._id_tensor(item_ids, "item_ids")
        if seen is not None:
            if not isinstance(seen, SeenLists):
                raise TypeError("seen must be a SeenLists or None")
            _native.require_device(seen.ptr, "seen.ptr")
            lists = CoPurchase.from_seen(seen, n_users, n_items)
        else:
            if not (torch.is_tensor(edge_index) and edge_index.dim() == 2):
                raise ValueError("seen=None needs edge_index as an int64 [2, E] tensor (CoPurchase.from_edges)")
            _native.require_device(edge_index, "edge_index")
            lists = CoPurchase.from_edges(edge_index, n_users, n_items)
        return lists.neighbors(ids, k, measure, min_count, item_ok)

    # -- the item-kNN baseline: recommendations from the neighbour table alone ----------------------
    def recommend_itemknn(self, edge_index, edge_weight, n_users, n_items, users=None, sessions=None, k: int = 20, knn=None,
                          kn: int = 64, measure: str = "cosine", seen=None, item_ok=None):
        """``(index int64 [n, k], value fp32 [n, k], votes int32 [n, k])`` on the device: item-kNN recommendations, per
        user of ``users`` (their purchase lists are the baskets, the purchased items removed) or per session of
        ``sessions`` (a ``SessionLists``, its weights applied, its own items removed); exactly one of the two is given.
        A prebuilt ``itemknn.ItemKNN`` is taken as ``knn``; otherwise one is fitted here with ``kn`` neighbours an item by
        ``measure``, from ``seen`` (a ``SeenLists``) or, without it, from every edge of ``edge_index`` as
        ``bought_together`` does.  ``item_ok``: bool or uint8 ``[n_items]``, items that may be returned.  It reads no
        embedding and triggers no propagation.  See ``itemknn.knn_recommend``."""
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 1 or n_items < 1 or n_users + n_items != self.num_nodes:
            raise ValueError(f"n_users {n_users} + n_items {n_items} != {self.num_nodes} nodes")
        if (users is None) == (sessions is None):
            raise ValueError("exactly one of users and sessions must be given")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.KNN_MAX_K:
            raise ValueError(f"k must be an integer in [1, {_native.KNN_MAX_K}]")
        if isinstance(kn, bool) or not isinstance(kn, int) or not 1 <= kn <= _native.KNN_MAX_NEIGHBORS:
            raise ValueError(f"kn must be an integer in [1, {_native.KNN_MAX_NEIGHBORS}]")
        if not isinstance(measure, str) or measure not in MEASURES:
            raise ValueError(f"measure must be one of {list(MEASURES)}, got {measure!r}")
        item_ok = self._ok_mask(item_ok, n_items, "item_ok")
        if sessions is not None and not isinstance(sessions, SessionLists):
            raise TypeError("sessions must be a SessionLists")
        ids = None if users is None else self._id_tensor(users, "users")
        if knn is None:
            if seen is not None:
                if not isinstance(seen, SeenLists):
                    raise TypeError("seen must be a SeenLists or None")
                _native.require_device(seen.ptr, "seen.ptr")
                lists = CoPurchase.from_seen(seen, n_users, n_items)
            else:
                if not (torch.is_tensor(edge_index) and edge_index.dim() == 2):
                    raise ValueError("seen=None needs edge_index as an int64 [2, E] tensor (CoPurchase.from_edges)")
                _native.require_device(edge_index, "edge_index")
                lists = CoPurchase.from_edges(edge_index, n_users, n_items)
            knn = ItemKNN.fit(lists, kn, measure)
        elif not isinstance(knn, ItemKNN) or knn.n_items != n_items:
            raise TypeError(f"knn must be an ItemKNN over {n_items} items or None")
        if sessions is not None:
            return knn.recommend_sessions(sessions, k, item_ok=item_ok)
        return knn.recommend(ids, k, item_ok=item_ok)

    # -- k recommendations that are not k variants of one product ---------------------------------
    def _item_table(self, edge_index, edge_weight, n_users, n_items) -> Tensor:
        """The item rows of the cached serving embedding, the table the three methods below measure similarity on."""
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 0 or n_items < 1 or n_users + n_items != self.num_nodes:
            raise ValueError(f"n_users {n_users} + n_items {n_items} != {self.num_nodes} nodes")
        _native.require_device(self.embedding.weight, "LightGCN.embedding.weight")
        with torch.no_grad():
            return self._serving_embedding(edge_index, edge_weight).detach()[n_users:]

    def recommend_diverse(self, edge_index, edge_weight, n_users, n_items, seen, users, k: int = 20, candidates: int = 100,
                          lam: float = 0.7, metric: str = "cosine", workspace_bytes: int = DEFAULT_WORKSPACE_BYTES) -> Tensor:
        """int64 ``[len(users), k]`` item indices on the device: the ``min(candidates, n_items)`` best of
        ``recommend_topk`` with their masked scores, re-ranked by greedy maximal marginal relevance
        (``rerank.mmr_rerank``): every place goes to the candidate with the best ``lam * score - (1 - lam) * (largest
        similarity to an item already chosen)``, similarity by ``metric`` over the item rows of the serving embedding.
        ``k <= candidates <= 256``.  With ``lam = 1`` the answer is ``recommend_topk(k)``, index for index."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError("k must be a positive integer")
        if isinstance(candidates, bool) or not isinstance(candidates, int) or not k <= candidates <= RERANK_MAX_CAND:
            raise ValueError(f"candidates must be an integer in [k, {RERANK_MAX_CAND}], got {candidates!r} with k = {k}")
        check_lam(lam)
        user_t, item_t, seen, ids = self._eval_tables(edge_index, edge_weight, n_users, n_items, seen, users)
        top, value = recommend_topk(user_t, ids, item_t, seen, min(candidates, int(n_items)), workspace_bytes, True)
        return mmr_rerank(item_t, top, value, k, lam, metric)

    def rerank_diverse(self, edge_index, edge_weight, n_users, n_items, top_items, top_values, k: int, lam: float = 0.7,
                       metric: str = "cosine") -> Tensor:
        """The same for any candidate list: ``top_items`` int64 ``[rows, N]`` item indices (-1 = an empty place) and
        ``top_values`` fp32 ``[rows, N]`` their relevance -- ``recommend_topk(..., return_values=True)``'s answer or
        ``recommend_sessions(..., return_values=True)``'s.  int64 ``[rows, k]`` on the device."""
        item_t = self._item_table(edge_index, edge_weight, n_users, n_items)
        cand = top_items if torch.is_tensor(top_items) else torch.as_tensor(top_items, dtype=torch.int64)
        rel = top_values if torch.is_tensor(top_values) else torch.as_tensor(top_values, dtype=torch.float32)
        if cand.dim() != 2 or rel.shape != cand.shape:
            raise ValueError("top_items and top_values must be [rows, N] of the same shape")
        cand = cand.to(device=item_t.device, dtype=torch.int64).contiguous()
        rel = rel.to(device=item_t.device, dtype=torch.float32).contiguous()
        return mmr_rerank(item_t, cand, rel, k, lam, metric)

    def list_diversity(self, edge_index, edge_weight, n_users, n_items, top_items, ks=(5, 10, 20), metric: str = "cosine"):
        """``(values, mean)``: the intra-list diversity of the lists ``top_items`` (int64 ``[rows, k]`` item indices) at
        every cutoff of ``ks`` (ascending, the last <= k) -- the mean of ``1 - similarity`` over the pairs among a list's
        first c items, float64 ``[rows, len(ks)]`` on the device (``rerank.list_diversity``) -- and its mean over the rows,
        a tuple of Python floats (NaN where a row's is).  One host sync."""
        item_t = self._item_table(edge_index, edge_weight, n_users, n_items)
        lists = top_items if torch.is_tensor(top_items) else torch.as_tensor(top_items, dtype=torch.int64)
        if lists.dim() != 2:
            raise ValueError("top_items must be [rows, k] item indices")
        lists = lists.to(device=item_t.device, dtype=torch.int64).contiguous()
        values = list_diversity(item_t, lists, ks, metric)
        n = values.size(0)
        if n == 0:
            return values, tuple(float("nan") for _ in range(values.size(1)))
        sums = column_sums(values).cpu().tolist()            # the one sync
        return values, tuple(s / n for s in sums)

    def link_pred_loss(self, pred: Tensor, edge_label: Tensor, **kwargs) -> Tensor:
        return torch.nn.BCEWithLogitsLoss(**kwargs)(pred, edge_label.to(pred.dtype))

    def recommendation_loss(self, pos_edge_rank: Tensor, neg_edge_rank: Tensor,
                            lambda_reg: float = 1e-4, **kwargs) -> Tensor:
        return BPRLoss(lambda_reg, **kwargs)(pos_edge_rank, neg_edge_rank, self.embedding.weight)

    def softmax_loss(self, edge_index, edge_weight, users: Tensor, pos_items: Tensor, neg_items: Optional[Tensor] = None, *,
                     temperature: float = 1.0, ignore=None, cand_bias: Optional[Tensor] = None) -> Tensor:
        """In-batch softmax (InfoNCE / sampled-softmax) loss of a batch, an addition to the reference's BPR: every user
        of ``users`` is scored against ALL candidates ``cat[pos_items, neg_items]`` (or ``pos_items`` alone) and
        ``loss = (1 / B) sum_i log sum_{j in J_i} exp((s_ij - s_ii) / temperature)``, where ``J_i`` holds the user's own
        positive (column i) and every other candidate that is not the same item and not in the user's ignore list.  With
        ``neg_items`` that is up to ``2B - 1`` negatives per positive from the rows the BPR step propagates anyway.

        ``users``, ``pos_items``, ``neg_items``: int64 ``[B]`` node ids as ``TripleSampler.sample()`` returns them (items
        already offset by ``n_users``).  ``ignore``: a ``TripleSampler`` or its ``(ign_ptr, ign_items)`` pair -- a user's
        other positives among the candidates are then no negatives; None admits every other item.  ``cand_bias``: fp32
        ``[C]`` added to the logits of a column (``-log q_j`` corrects for the sampling distribution).  ``temperature``
        must be finite and > 0.  For ``B = 1, C = 2, temperature = 1`` the value is BPR's ``softplus(neg - pos)``.

        With gradients on this is one autograd node with a sparse backward (``softmax.softmax_from_table``), and
        ``regularization_loss(users, pos, neg, decay)`` after it routes its gradient into that node exactly as after
        ``forward``.  Single device; ``PartitionedTrainer`` keeps BPR."""
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) \
                or not temperature > 0:
            raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
        lists = [users, pos_items] + ([neg_items] if neg_items is not None else [])
        for name, t in zip(("users", "pos_items", "neg_items"), lists):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
                raise TypeError(f"{name} must be a 1-D int64 tensor of node ids")
            if t.numel() != users.numel():
                raise ValueError(f"{name} has {t.numel()} entries, users {users.numel()}")
        if users.numel() == 0:
            raise ValueError("an empty batch has no loss")
        ignore = ignore_lists(ignore)
        if cand_bias is not None and (not torch.is_tensor(cand_bias) or cand_bias.dtype != torch.float32 or cand_bias.dim() != 1
                                      or cand_bias.numel() != len(lists[1:]) * users.numel()):
            raise TypeError("cand_bias must be a 1-D float32 tensor with one value per candidate")
        x0 = self.embedding.weight
        _native.require_device(x0, "LightGCN.embedding.weight")
        normalize = self.convs[0].normalize if self.num_layers > 0 else True
        graph = get_graph(edge_index, edge_weight, self.num_nodes, normalize)
        if graph.split is None:
            raise ValueError("softmax_loss needs a user|item (bipartite) graph with the users first")
        b = users.numel()
        cands = pos_items if neg_items is None else torch.cat([pos_items, neg_items])
        target = torch.arange(b, dtype=torch.int32, device=users.device)
        hook = RegHook(x0) if (torch.is_grad_enabled() and x0.requires_grad) else None
        loss = softmax_from_table(x0, graph, self._alphas(), users, cands, target, ignore, 1.0 / float(temperature), b,
                                  cand_bias, hook)
        x0._lgcn_reg_hook = hook if (hook is not None and hook.token is not None) else None
        return loss

    def regularization_loss(self, users: Tensor, pos_items: Tensor, neg_items: Tensor, decay: float,
                            batch_size: Optional[int] = None) -> Tensor:
        """``regularization_loss(model.embedding.weight, size, users, pos, neg, decay)`` of src/utils_v2.py:193-211 (the
        call at src/train_lightgcn.py:142): same value, same gradient -- see the module function below."""
        return regularization_loss(self.embedding.weight, len(users) if batch_size is None else batch_size, users,
                                   pos_items, neg_items, decay)

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}({self.num_nodes}, {self.embedding_dim}, num_layers={self.num_layers})'


def regularization_loss(init_embed: Tensor, batch_size: int, batch_usr: Tensor, batch_pos: Tensor, batch_neg: Tensor,
                        decay: float) -> Tensor:
    """src/utils_v2.py:193-211 with the reference's signature:  decay / 2 * (|E0[u]|^2 + |E0[p]|^2 + |E0[n]|^2) / size.

    Upstream's autograd turns the three row gathers into three dense, zero-filled [N, D] gradients and adds them to the
    dense gradient of the scores (0.9 ms of a 5.2 ms step at 1.7 M x 64).  When ``init_embed`` is the weight a
    ``LightGCN.forward`` of this step has just scored from, the value is computed the same way but its gradient --
    ``decay / size * E0[r]`` on the <= 3B rows -- is handed to that forward's scoring node, whose backward adds it to
    the rows of the dense gradient it writes anyway.  In every other situation (no forward yet, gradients off, the
    dense two-node path, the graph already consumed) this is upstream's expression on plain torch ops."""
    hook = getattr(init_embed, "_lgcn_reg_hook", None)
    if (hook is not None and not hook.spent and hook.token is not None and hook.weight is init_embed
            and torch.is_grad_enabled() and init_embed.is_cuda and batch_size > 0       # (size 0: upstream's inf / nan)
            and all(routable_index(t) for t in (batch_usr, batch_pos, batch_neg))):
        return regularization_through(hook, batch_size, batch_usr, batch_pos, batch_neg, decay)
    reg_loss = (1 / 2) * (init_embed[batch_usr].norm().pow(2) + init_embed[batch_pos].norm().pow(2)
                          + init_embed[batch_neg].norm().pow(2)) / batch_size
    return reg_loss * decay


class BPRLoss(_Loss):
    """(-mean(log sigmoid(pos - neg)) + lambda_reg * ||parameters||^2) / n_pairs  (src/lightgcn.py:262-286)."""
    __constants__ = ['lambda_reg']
    lambda_reg: float

    def __init__(self, lambda_reg: float = 0, **kwargs) -> None:
        super().__init__(None, None, "sum", **kwargs)
        self.lambda_reg = lambda_reg

    def forward(self, positives: Tensor, negatives: Tensor, parameters: Tensor = None) -> Tensor:
        n_pairs = positives.size(0)
        if self.lambda_reg == 0 and positives.dim() == 1:
            fused = bpr_loss_fused(positives, negatives)      # the same value and gradient in one launch each way
            if fused is not None:
                return fused
        loss = -F.logsigmoid(positives - negatives).mean()
        if self.lambda_reg != 0:
            loss = loss + self.lambda_reg * parameters.norm(p=2).pow(2)
        return loss / n_pairs
