"""ctypes binding of ``csrc/liblgconv_hip.so`` (C ABI: ``include/lgconv_hip.h``).

There is no fallback: if the library is missing or fails to load, every operator in this
package raises ``NativeLibraryError``.  The library is opened only AFTER ``import torch`` so
that its ``NEEDED libamdhip64.so.7`` binds to the HIP runtime torch has already mapped (one
runtime per process); ``runtime_libraries()`` lets tests assert that.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import CFUNCTYPE, POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p
from typing import Optional

import torch

LIB_NAME = "liblgconv_hip.so"
# LGCN_LIB_PATH selects another build of the SAME library (A/B kernel experiments); never a fallback.
LIB_PATH = os.environ.get("LGCN_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", LIB_NAME)
ABI_VERSION = 14

# status bits (include/lgconv_hip.h)
ST_INDEX_OOB = 1
ST_SAMPLER_EXHAUSTED = 2

class SweepCfg(Structure):
    """lgc_sweep_cfg"""
    _fields_ = [("n_bands", c_int32), ("waves_per_band_round", c_int32), ("row_cap", c_int32), ("piece_cap", c_int32),
                ("lookahead", c_int32), ("groups", c_int32), ("round_order", c_int32), ("light_len", c_int32)]


class SweepDims(Structure):
    """lgc_sweep_dims"""
    _fields_ = [("n_bands", c_int32), ("rounds", c_int32), ("row_cap", c_int32), ("piece_cap", c_int32),
                ("n_rows", c_int32), ("groups", c_int32),
                ("n_waves", c_int64), ("n_slabs", c_int64), ("n_slots", c_int64), ("n_entries", c_int64),
                ("n_steps", c_int64), ("n_padding", c_int64), ("light_len", c_int32), ("reserved", c_int32)]


class TileClassC(Structure):
    """lgc_tile_class"""
    _fields_ = [("order", c_void_p), ("meta", c_void_p), ("slab", c_void_p), ("n_tiles", c_int32), ("width", c_int32)]


class SweepArraysC(Structure):
    """lgc_sweep_arrays"""
    _fields_ = [("slabs", c_void_p), ("wave_slab_ptr", c_void_p), ("wave_npieces", c_void_p), ("piece_slot", c_void_p),
                ("multi", c_void_p), ("multi_wide", c_void_p), ("partials", c_void_p), ("n_waves", c_int64),
                ("row_cap", c_int32), ("n_rows", c_int32), ("n_wide", c_int32), ("groups", c_int32)]


class OperatorC(Structure):
    """lgc_operator"""
    _fields_ = [("rowptr", c_void_p), ("entries", c_void_p), ("chunks", c_void_p), ("multi", c_void_p),
                ("partials", c_void_p), ("sweep", POINTER(SweepArraysC)), ("tiles", TileClassC * 3),
                ("row_begin", c_int32), ("row_end", c_int32), ("short_max", c_int32), ("n_chunks", c_int32),
                ("n_multi", c_int32), ("n_tile_classes", c_int32), ("tiles_per_wave", c_int32), ("reserved", c_int32)]


# lgc_apply_route's codes (LGC_ROUTE_*; LGC_ROUTE_WT_STORE is the bit 0x100, spelt "+wt" by route_name)
ROUTES = {1: "rows", 2: "sweep", 3: "sweep_wide", 4: "sweep_two_pass", 5: "fused_dpp", 6: "fused_generic", 7: "split_dpp",
          8: "split_generic"}
ROUTE_WT_STORE = 0x100


def route_name(code: int) -> str:
    """"fused_dpp+wt" for LGC_ROUTE_FUSED_DPP | LGC_ROUTE_WT_STORE, "fused_dpp" without the bit."""
    return ROUTES[code & ~ROUTE_WT_STORE] + ("+wt" if code & ROUTE_WT_STORE else "")


class AttrArgsC(Structure):
    """lgc_attr_args"""
    _fields_ = [("list_ptr", c_void_p), ("list_items", c_void_p), ("list_weight", c_void_p), ("item_dis", c_void_p),
                ("rowptr", c_void_p), ("entries", c_void_p), ("row_ids", c_void_p), ("n_graph_rows", c_int64),
                ("col_base", c_int64), ("n_rows", c_int64), ("fold", c_void_p), ("items", c_void_p), ("fold_stride", c_int64),
                ("item_stride", c_int64), ("n_items", c_int64), ("init_rows", c_void_p), ("init", c_void_p),
                ("init_stride", c_int64), ("n_init_rows", c_int64), ("targets", c_void_p), ("target_stride", c_int64),
                ("contrib_ptr", c_void_p), ("contrib", c_void_p), ("base", c_void_p), ("total", c_void_p),
                ("top_pos", c_void_p), ("top_item", c_void_p), ("top_value", c_void_p), ("status", c_void_p),
                ("a0", c_float), ("normalize", c_int32), ("n_targets", c_int32), ("top_m", c_int32), ("dim", c_int32)]


EXCHANGE_FN = CFUNCTYPE(c_int, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p)   # lgc_exchange_fn


# symbol -> (restype, argtypes); tests check every name against the header and the .so
SIGNATURES = {
    "lgc_abi_version": (c_int, []),
    "lgc_error_string": (c_char_p, [c_int]),
    "lgc_dim_ok": (c_int, [c_int32]),
    "lgc_build_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "lgc_build_csr": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lgc_spmm": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                         c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_float, c_float,
                         c_int32, c_void_p]),
    "lgc_spmm_rows": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                              c_void_p, c_int64, c_float, c_float, c_int32, c_void_p]),
    "lgc_spmm_rows_split": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                    c_int64, c_int64, c_void_p, c_int64, c_float, c_float, c_int32, c_int32, c_void_p, c_void_p,
                                    c_int64, c_void_p]),
    "lgc_bipartite_split": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "lgc_row_plan_workspace_bytes": (c_size_t, [c_int64]),
    "lgc_row_plan_count": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lgc_row_plan_fill": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_tile_classes_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "lgc_tile_classes": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_void_p, c_size_t, c_void_p,
                                 c_void_p, c_void_p]),
    "lgc_tile_pack": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "lgc_build_tiles": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "lgc_spmm_tiles": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p, c_int64,
                               c_void_p, c_int64, c_void_p, c_int64, c_float, c_float, c_int32, c_void_p]),
    "lgc_sweep_plan_create": (c_void_p, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(SweepCfg),
                                         POINTER(c_int)]),
    "lgc_sweep_plan_dims": (c_int, [c_void_p, POINTER(SweepDims)]),
    "lgc_sweep_plan_export": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_sweep_plan_upload": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_sweep_plan_export_multi": (c_int, [c_void_p, c_void_p]),
    "lgc_sweep_plan_free": (None, [c_void_p]),
    "lgc_sweep_dplan_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, POINTER(SweepCfg)]),
    "lgc_sweep_dplan_create": (c_void_p, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32,
                                          POINTER(SweepCfg), c_void_p, c_size_t, c_void_p, POINTER(c_int)]),
    "lgc_sweep_dplan_dims": (c_int, [c_void_p, POINTER(SweepDims)]),
    "lgc_sweep_dplan_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_sweep_dplan_export_multi": (c_int, [c_void_p, c_void_p]),
    "lgc_sweep_dplan_free": (None, [c_void_p]),
    "lgc_sweep_ok": (c_int, [c_int32, c_int64, c_int64]),
    "lgc_spmm_sweep": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p,
                               c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_float, c_float,
                               c_int32, c_void_p]),
    "lgc_apply_route": (c_int, [POINTER(OperatorC), c_int64, c_int64, c_int64, c_int64, c_int32]),
    "lgc_apply": (c_int, [POINTER(OperatorC), c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_float, c_float,
                          c_int32, c_void_p]),
    "lgc_apply2": (c_int, [POINTER(OperatorC), c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                           c_float, c_float, c_float, c_int32, c_void_p]),
    "lgc_hop_exchange": (c_int, [POINTER(OperatorC), POINTER(OperatorC), c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                 c_int64, c_float, c_float, c_int32, c_int32, c_int32, c_int32, EXCHANGE_FN, c_void_p, c_void_p]),
    "lgc_segment_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p, c_int64, c_int64, c_int32,
                                c_int32, c_void_p]),
    "lgc_pair_dot_rows": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "lgc_reg_rows": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_float,
                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_bpr_loss": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "lgc_pair_seed_vals": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "lgc_seed_prepare": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "lgc_seed_flags": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int32, c_void_p]),
    "lgc_seed_pull": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    "lgc_seed_mark": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    "lgc_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                              c_float, c_void_p]),
    "lgc_adam_step_hp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "lgc_lincomb": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p]),
    "lgc_mask_topk": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                              c_void_p, c_void_p, c_void_p]),
    "lgc_fold_in": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                            c_int64, c_int64, c_float, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "lgc_score_rows": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                               c_int64, c_void_p, c_void_p]),
    "lgc_topk_hits": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                              c_void_p, c_void_p]),
    "lgc_metric_sums": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "lgc_rank_metrics": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                 POINTER(c_int32), c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_column_sums": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    "lgc_topk_coverage": (c_int, [c_void_p, c_int64, c_int32, c_int64, POINTER(c_int32), c_int32, c_int64, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "lgc_bfs_init": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_bfs_level": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_uint64, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p]),
    "lgc_bfs_resolve": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "lgc_bfs_backtrack": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int64,
                                  c_void_p, c_int32, c_void_p]),
    "lgc_sample_triples": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_uint64,
                                   c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_pair_dot": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                             c_void_p, c_void_p]),
    "lgc_reduce_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "lgc_reduce_count": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_size_t, c_void_p, c_void_p,
                                 c_void_p]),
    "lgc_reduce_fill": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                c_void_p, c_void_p]),
    "lgc_reduce_gram_workspace_bytes": (c_size_t, [c_int64]),
    "lgc_reduce_gram_count": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_size_t,
                                      c_void_p, c_void_p]),
    "lgc_reduce_gram_fill": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "lgc_reduce_concat_rows": (c_int64, [c_int64, c_int64, c_int32]),
    "lgc_reduce_concat": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "lgc_reduce_concat_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
    "lgc_attribute": (c_int, [POINTER(AttrArgsC), c_void_p]),
    "lgc_row_rnorm": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    "lgc_item_neighbors_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "lgc_item_neighbors": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32,
                                   c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lgc_rerank_route": (c_int, [c_int32, c_int32]),
    "lgc_rerank_mmr": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                               c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_list_diversity": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int32,
                                   POINTER(c_int32), c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "lgc_sample_hard_triples": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_uint64,
                                        c_uint64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lgc_rank_positions_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32]),
    "lgc_rank_positions": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p, c_void_p]),
    "lgc_softmax_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "lgc_softmax_batch": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lgc_retrieve_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "lgc_retrieve_topk": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                                  c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lgc_cooccur_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_void_p]),
    "lgc_cooccur_topk": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32,
                                 c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lgc_knn_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_void_p]),
    "lgc_knn_recommend": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                  c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p, c_void_p]),
}


class NativeLibraryError(RuntimeError):
    """The HIP library is missing, stale, or a call into it failed."""


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: the MI355X propagation library has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C gnn-ecommerce_amd/csrc`). "
            "There is no CPU or PyTorch fallback for this path.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from exc
        fn.restype, fn.argtypes = restype, argtypes
    if lib.lgc_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"{LIB_PATH} has ABI {lib.lgc_abi_version()}, expected {ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        text = load().lgc_error_string(code).decode()
        raise NativeLibraryError(f"{what} failed: {text} (code {code})")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Raw device pointer, or None (-> NULL)."""
    return None if t is None else t.data_ptr()


def stream_of(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def scratch_owner(device: torch.device, stream: Optional[int] = None) -> tuple:
    """(device, stream handle, host thread id): the one owner of a scratch buffer that lives across launches -- the partial
    rows one launch of a hop writes and a later one reads, the flags a backward sets, pulls through and clears, a score
    panel between its scoring and its ranking launch.  Work on such a buffer is ordered on ITS stream and issued by ITS
    thread only, so two streams, or two threads on one stream (every thread's default), never share one.  ``stream``: the
    handle the launches will get, when the caller has it already (None: the device's current stream is looked up; 0 for
    a CPU device).  A stream that is being captured is an owner like any other."""
    if stream is None:
        stream = stream_of(device) if device.type == "cuda" else 0
    return (device, stream, threading.get_ident())


def require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise NativeLibraryError(
            f"{name} is on {t.device}: the LightGCN propagation path runs only on a ROCm device "
            "(MI355X); move the model and graph tensors to 'cuda'. No CPU fallback is provided.")


MAX_TERMS = 8
BFS_MAX_SOURCES = 64   # LGC_BFS_MAX_SOURCES: sources one batch of the BFS carries
BFS_UNSET = -3         # LGC_BFS_UNSET
SEED_MAX = 8192        # LGC_SEED_MAX: ids one lgc_seed_prepare launch sorts
# lgc_rank_metrics: the columns of its metrics output (LGC_RM_*), the most cutoffs of one call, lgc_column_sums' widest input
RM_PRECISION, RM_RECALL, RM_NDCG, RM_AP, RM_RR, RM_HIT, RM_COUNT = range(7)
RM_MAX_CUTOFFS = 8
COLUMN_SUMS_MAX = 64
ATTR_MAX_TARGETS = 64  # LGC_ATTR_MAX_TARGETS: target columns of one lgc_attribute launch
ATTR_MAX_TOP = 8       # LGC_ATTR_MAX_TOP
NEIGHBORS_MAX_K = 64   # LGC_NEIGHBORS_MAX_K
RETRIEVE_MAX_K = 64    # LGC_RETRIEVE_MAX_K
RETRIEVE_MAX_SLICES = 1024   # LGC_RETRIEVE_MAX_SLICES
COOCCUR_MAX_K = 64     # LGC_COOCCUR_MAX_K
COOCCUR_MAX_BAND = 32768   # LGC_COOCCUR_MAX_BAND: item counters of one workgroup
KNN_MAX_K = 64         # LGC_KNN_MAX_K
KNN_MAX_NEIGHBORS = 64 # LGC_KNN_MAX_NEIGHBORS: the widest neighbour table lgc_knn_recommend takes
KNN_MAX_BAND = 16384   # LGC_KNN_MAX_BAND: items (accumulator and votes) of one workgroup
RERANK_MAX_CAND = 256  # LGC_RERANK_MAX_CAND
HARDNEG_MAX_CAND = 256 # LGC_HARDNEG_MAX_CAND
RANK_SEEN_MODES = {"zero": 0, "remove": 1}   # LGC_RANK_SEEN_ZERO, LGC_RANK_SEEN_REMOVE
RERANK_ROUTES = {1: "lds", 2: "global"}   # lgc_rerank_route's codes (LGC_RERANK_ROUTE_*)


def lincomb(y: torch.Tensor, terms) -> torch.Tensor:
    """y = sum_t coef_t * src_t over 2-D fp32 views of equal shape (``terms``: list of (coef, tensor))."""
    lib = load()
    n = len(terms)
    if not 1 <= n <= MAX_TERMS:
        raise ValueError(f"1..{MAX_TERMS} terms")
    ptrs = (c_void_p * n)(*[t.data_ptr() for _, t in terms])
    strides = (c_int64 * n)(*[t.stride(0) for _, t in terms])
    coefs = (c_float * n)(*[float(c) for c, _ in terms])
    with torch.cuda.device(y.device):
        code = lib.lgc_lincomb(y.data_ptr(), y.stride(0), ptrs, strides, coefs, n, y.size(0), y.size(1),
                               stream_of(y.device))
    check(code, "lgc_lincomb")
    return y


def runtime_libraries() -> list:
    """Paths of every libamdhip64 / libhsa-runtime64 mapped into this process."""
    seen = set()
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64" in path or "libhsa-runtime64" in path:
                seen.add(path)
    return sorted(seen)
