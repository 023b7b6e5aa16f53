"""MI355X-native LightGCN propagation (the hot path of happykygo/GNN-eCommerce).

``LightGCN`` / ``BPRLoss`` / ``LGConv`` are drop-ins for the reference's ``src/lightgcn.py``
surface; the arithmetic runs in ``csrc/liblgconv_hip.so`` (hand-written HIP for gfx950) behind the
C ABI of ``include/lgconv_hip.h``.  There is no CPU fallback.

The directory is called ``gnn-ecommerce_amd`` (not an importable name); ``import gnn_ecommerce_amd``
resolves to it through the shim package of that name at the repository root.
"""
from . import _native
from .explain import Attribution, attribute
from .foldin import SessionLists, fold_in, fold_table
from .graph import PropGraph, build_row_plan, clear_cache, get_graph
from .lgconv import LGConv
from .lightgcn import BPRLoss, LightGCN, regularization_loss
from .paths import compute_paths, hop_distances, paths_frame, shortest_paths
from .propagate import (PositiveLists, RankingResult, SeenLists, check_index_status, evaluate_ranking, hop, metrics_frame,
                        overlap_items, pair_dot, propagate_sum, rank_metrics, recommend_topk, score_rows)
from .sampler import TripleSampler
from .similar import item_neighbors, row_rnorm
from .retrieve import BuyerLists, retrieve_topk
from .cooccur import CoPurchase, cooccur_topk
from .itemknn import ItemKNN, knn_recommend
from .fullrank import FullRankResult, PairRanks, evaluate_full_rank, positive_ranks
from .rerank import list_diversity, mmr_rerank
from .softmax import SoftmaxBatch, softmax_batch, softmax_from_table, softmax_loss_reference
from . import ingest, serving
from .trainer import PartitionedTrainer

__all__ = ["LightGCN", "BPRLoss", "LGConv", "PropGraph", "get_graph", "clear_cache", "build_row_plan",
           "propagate_sum", "hop", "pair_dot", "check_index_status", "TripleSampler", "regularization_loss", "PartitionedTrainer", "_native",
           "SeenLists", "PositiveLists", "score_rows", "recommend_topk", "hop_distances", "shortest_paths", "paths_frame", "compute_paths",
           "rank_metrics", "evaluate_ranking", "overlap_items", "metrics_frame", "RankingResult",
           "SessionLists", "fold_table", "fold_in", "Attribution", "attribute",
           "item_neighbors", "row_rnorm", "retrieve_topk", "BuyerLists", "cooccur_topk", "CoPurchase", "knn_recommend", "ItemKNN", "mmr_rerank", "list_diversity",
           "positive_ranks", "evaluate_full_rank", "PairRanks", "FullRankResult",
           "softmax_batch", "softmax_loss_reference", "softmax_from_table", "SoftmaxBatch"]
