"""ctypes binding of ``libnpi_gnn.so`` (the C ABI of ``include/npi_gnn.h``).

There is NO CPU fallback: every wrapper raises if the library is missing or if a tensor is not
on an AMD GPU.  PyTorch only lends device memory and the current HIP stream.  The link-prediction entry points in the
order of a run: ``npi_split_*`` (train / val / test parts and folds of the edge list), ``npi_sample_*`` (batches), ``npi_negative_*`` (negatives), ``npi_random_walk`` / ``npi_walk_pairs`` (node2vec
walks and their skip-gram pair list), ``npi_pair_score`` (scores and loss), ``npi_group_score`` (ranking losses of every
positive against its own corrupted targets), ``npi_gauss_*`` (the variational
sample and its KL term), ``npi_rank_metrics`` (ROC-AUC, average precision and
the score curve of an evaluation), ``npi_topk_links`` (the k most likely new links of every query row), ``npi_link_ranks`` (the
filtered rank of every held-out link among the targets its source has no known edge to), ``npi_softmax_link_*`` (the listwise
loss over all those targets, forward and backward).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

import torch  # noqa: F401  (must be imported first: the .so binds to torch's libamdhip64.so.7)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NPI_GNN_LIB") or os.path.join(HERE, "libnpi_gnn.so")   # env override: kernel A/B experiments

NPI_F32 = 0
NPI_BF16 = 1
NPI_GEMM_EXACT_F32 = 1      # flags of the npi_linear_*_ex entry points
NPI_GEMM_SPLIT_BF16 = 2
NPI_GEMM_A_ZERO_PADDED = 4   # A stored with zero pad columns up to a multiple of 128 (include/npi_gnn.h)
NPI_GEMM_WORKSPACE_PREPARED = 8   # the workspace already holds npi_linear_prepare's copy of this weight matrix
NPI_GEMM_SPLIT_F16X2 = 16         # two fp16 pieces per operand, three matrix products per tile pair (needs the row scales of A)
NPI_PREPARE_F16X2 = 4             # npi_linear_prepare(which | this): the fp16 x 2 planes of the weight matrix
NPI_STATUS_BAD_ROW_ID = 8         # status bit of npi_rows_gather: a row id outside the source table
NPI_STATUS_BAD_TARGET_ID = 16     # status bit of npi_sample_counts / npi_sample_union: a target (batch) id outside [0, N)
NPI_STATUS_BAD_SAMPLE_SIZES = 32  # status bit of npi_sample_select / _relabel / _union: offsets / counts / capacity of another call
NPI_STATUS_NO_NEGATIVE = 64       # status bit of npi_negative_targets: a slot whose tries all hit edges (it holds -1)
NPI_STATUS_BAD_SOURCE_ID = 128    # status bit of npi_negative_targets: a source id outside [0, n_src) (its slot holds -1)
NPI_STATUS_BAD_PAIR_ID = 256      # status bit of npi_pair_score: a pair with an id outside its table (logit, coefficient and loss term 0);
                                  # of npi_split_permute / npi_split_undirected: a column with an id out of range (it was dropped)
NPI_SPLIT_UPPER = 1               # flag of npi_split_permute: keep src < dst only (one id space; PyG's row < col)
NPI_STATUS_WALK_TRIES = 512       # status bit of npi_random_walk: a step whose tries were all rejected (it took the last candidate)
NPI_STATUS_BAD_SCORE = 1024      # status bit of npi_rank_metrics: a NaN score (the metrics are undefined)
NPI_STATUS_BAD_LABEL = 2048      # status bit of npi_rank_metrics: a label other than 0 / 1 (it counted as 0)
NPI_STATUS_BAD_ENCLOSE_KEY = 4096     # status bit of npi_enclose_sizes: a key with u == v or an id out of range (its sample is empty)
NPI_STATUS_BAD_ENCLOSE_TOTALS = 8192  # status bit of npi_enclose_fill: totals of other keys (the batch holds placeholders only)
NPI_ENCLOSE_ADD_TARGET_EDGE = 1   # flag of npi_enclose_sizes / _fill: both target columns in front of rows 0 and 1, e_id -1
NPI_ENCLOSE_LABEL_NONE = 0        # label column of npi_enclose_features
NPI_ENCLOSE_LABEL_DRNL = 1
NPI_ENCLOSE_LABEL_TARGETS = 2
NPI_PAIR_LOGITS = 0               # modes of npi_pair_score
NPI_PAIR_LOSS_GAE = 1
NPI_PAIR_LOSS_BCE = 2
NPI_GROUP_LOGITS = 0              # modes of npi_group_score
NPI_GROUP_LOSS_BPR = 1
NPI_GROUP_LOSS_MARGIN = 2
NPI_GROUP_LOSS_SOFTMAX = 3
NPI_GAUSS_SAMPLE = 1              # flags of npi_gauss_sample_kl / _bwd: the reparametrised sample z ...
NPI_GAUSS_KL = 2                  # ... and the KL term
NPI_TOPK_MAX = 128               # largest k of npi_topk_links
NPI_TOPK_NO_LOOPS = 1            # flag of npi_topk_links: one id space, (v, v) is no candidate
NPI_LINK_RANK_NO_LOOPS = 1       # flag of npi_link_ranks: one id space, (v, v) is no competitor
NPI_SOFTMAX_LINK_NO_LOOPS = 1    # flag of npi_softmax_link_*: one id space, (v, v) is no candidate (unless it is the target)
NPI_DROP_UNDIRECTED = 1         # flag of npi_csr_drop_side / npi_drop_edge_*: Rule E keyed on the column's unordered pair of ends
NPI_HUB_MAX = 128              # hubs per plan (npi_hub_plan; mask words of NPI_HUB_MAX / 32 per source row)


def NPI_GEMM_RESERVE_CUS(n: int) -> int:
    """flag bits of npi_linear_fwd_ex / npi_linear_bwd_data_ex: leave ``n`` CUs (a multiple of 8, at most 128) to a kernel running
    beside the GEMM"""
    n = int(n)
    if n < 0 or n > 128 or n % 8:
        raise ValueError(f"NPI_GEMM_RESERVE_CUS: a multiple of 8 in [0, 128], got {n}")
    return (n // 8) << 8

_P = c_void_p
_I = c_int64

# name -> (restype, argtypes); mirrors include/npi_gnn.h one to one
PROTOTYPES = {
    "npi_last_error": (c_char_p, []),
    "npi_abi_version": (c_int, []),
    "npi_csr_workspace_bytes": (_I, [_I, _I]),
    "npi_item_edges": (_I, [_I]),
    "npi_num_items": (_I, [_I, _I]),
    "npi_csr_build_ex": (c_int, [_P, _P, _I, _I, _I, c_int, _I, c_int, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P]),
    "npi_edge_positions": (c_int, [_P, _P, _I, _I, _I, _P, _P]),
    "npi_segsum_carry_elems": (_I, [_I, _I, _I]),
    "npi_segsum_ex": (c_int, [_P, _P, _P, _I, _P, _I, _I, _P, _I, _P, _I, _P, _I, _I, c_int, c_int, _P, _P, _P, _P]),
    "npi_segsum_scales_supported": (c_int, [_I, c_int]),
    "npi_hub_plan_workspace_elems": (_I, []),
    "npi_hub_plan": (c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "npi_hub_light_side": (c_int, [_P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "npi_segsum_hub_slabs": (_I, [_I]),
    "npi_segsum_hub_partial_elems": (_I, [_I]),
    "npi_segsum_hub": (c_int, [_P, _I, _P, _P, _I, _I, _P, _P, _I, _P, _I, _I, c_int, _P, _P, _P]),
    "npi_row_weight_sum": (c_int, [_P, _P, _I, _P, _P]),
    "npi_gcn_norm": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "npi_row_inv_count": (c_int, [_P, _I, _P, _P]),
    "npi_entry_col_scale": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "npi_entry_weights": (c_int, [_P, _P, _P, _P, _P, c_float, _I, _I, _P, _P]),
    "npi_edge_dot": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "npi_gcn_norm_bwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "npi_relu_backward": (c_int, [_P, _I, _P, _I, _I, _I, _P, _I, _P]),
    "npi_rows_gather": (c_int, [_P, _I, _I, _P, _I, _I, _P, _I, c_int, _P, _P]),
    "npi_l2_normalize_rows": (c_int, [_P, _I, _I, _I, c_float, _P, _I, _P, _P]),
    "npi_l2_normalize_rows_bwd": (c_int, [_P, _I, _P, _I, _P, _I, _I, c_float, _P, _I, _P]),
    "npi_colsum_workspace_elems": (_I, [_I, _I]),
    "npi_colsum": (c_int, [_P, _I, _I, _I, _P, _P, _I, _P]),
    "npi_linear_bwd_weight_workspace_elems": (_I, [_I, _I, _I]),
    "npi_linear_workspace_bytes": (_I, [_I, _I]),
    "npi_row_scales": (c_int, [_P, _I, _I, _I, _P, _P]),
    "npi_linear_fwd_ex": (c_int, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, c_int, c_int, c_int, _P, _I, _P, _P]),
    "npi_linear_bwd_data_ex": (c_int, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, c_int, c_int, _P, _I, _P, _P]),
    "npi_linear_prepare": (c_int, [_P, _I, _I, _I, c_int, c_int, _P, _I, _P]),
    "npi_hold_cus": (c_int, [c_int, _I, _P, _P]),
    "npi_linear_fwd_scores_supported": (c_int, [_I, _I, _I]),
    "npi_linear_fwd_scores": (c_int, [_P, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "npi_linear_bwd_data_rank2_supported": (c_int, [_I, _I, _I]),
    "npi_linear_bwd_data_rank2": (c_int, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "npi_gat_rank2_cols": (c_int, [_P, _I, _P, _I, _I, _P, _P]),
    "npi_gat_rank2_tail": (c_int, [_P, _P, _I, _P, _I, _I, _P, _I, _P, _P]),
    "npi_linear_bwd_weight_ex": (c_int, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _I, c_int, c_int, c_int, _P, _P, _P]),
    "npi_col_scales_workspace_elems": (_I, [_I, _I]),
    "npi_col_scales": (c_int, [_P, _I, _I, _I, _P, _P, _P, _I, _P]),
    "npi_conv_fwd": (c_int, [_P, _P, _P, _I, _P, _I, _I, _P, _I, _I, c_int, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, c_int, c_int, c_int,
                             c_int, _P, _I, _P]),
    "npi_conv_bwd": (c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _I, c_int, c_int, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _P, _I,
                             c_int, _P, _P, _P, _I, _P, _I, _P, _I, _P, _P]),
    "npi_gat_aggregate_fused": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _P, _P, c_float, _P, c_int, _P, _P, _P, _P,
                                            _P]),
    "npi_gat_aggregate_fused_heads": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, c_float, _P, c_int, _P, _P,
                                               _P, _P, _P]),
    # the three launches with attention dropout under Rule D: the sibling's arguments, then eid, key, threshold (the uint64's bits), scale
    "npi_gat_aggregate_fused_heads_dropout": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, c_float, _P, c_int,
                                                       _P, _P, _P, _P, _P, _P, _I, _I, c_float]),
    "npi_gat_backward_fused_heads_dropout": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, c_float, _P,
                                                      _P, _P, _P, _P, _I, _P, _P, _I, _I, c_float]),
    "npi_gat_edge_grad_dropout": (c_int, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, c_float,
                                          c_int, _P, _P, _P, _P, _I, _I, c_float]),
    "npi_gat_dropout_keep": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, c_float, _P, _P]),
    "npi_gat_scores": (c_int, [_P, _I, _P, _I, _I, _I, _P, _P, _P]),
    "npi_gat_aggregate_ex": (c_int, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, c_float, c_int,
                                     _P, _P, _P, _P, _P, _P, _P, _P]),
    "npi_gat_pack_targets": (c_int, [_P, _P, _P, _P, _I, _P, _P]),
    "npi_gat_backward_fused_heads": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, c_float, _P,
                                                 _P, _P, _P, _P, _I, _P]),
    "npi_gat_rank1_add": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "npi_gat_rowdot": (c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _P, _P]),
    "npi_gat_edge_grad_ex": (c_int, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, c_float,
                                     c_int, _P, _P, _P]),
    "npi_seg_scan_workspace_elems": (_I, [_I, _I]),
    "npi_seg_rowsum_ex": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "npi_gat_softmax_stats_ex": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, c_float, _P, _P, _P, _P, _I, _P]),
    "npi_gat_aggregate_scores": (c_int, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, c_int, _P, _P]),
    "npi_gat_rowdot_colsum_workspace_elems": (_I, [_I, _I, _I]),
    "npi_gat_rowdot_colsum_relu": (c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P]),
    "npi_entry_transpose_map": (c_int, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "npi_gat_att_grad_workspace_elems": (_I, [_I, _I, _I]),
    "npi_gat_att_grad": (c_int, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "npi_topk_score": (c_int, [_P, _I, _P, _I, _I, _P, _P]),
    "npi_graph_bounds": (c_int, [_P, _I, _I, _P, _P]),
    "npi_topk_select": (c_int, [_P, _P, _I, _I, c_float, _P, _P, _P, _P, _I, _P]),
    "npi_topk_sorted_workspace_bytes": (_I, [_I]),
    "npi_topk_select_sorted": (c_int, [_P, _P, _P, _I, _I, c_float, _P, _P, _P, _P, _I, _P]),
    "npi_topk_gather": (c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    "npi_filter_adj_workspace_elems": (_I, [_I]),
    "npi_filter_adj": (c_int, [_P, _P, _I, _P, _P, _P, _P, _P, c_int, _P]),
    "npi_filter_adj_newpos_offset": (_I, [_I]),
    "npi_csr_filter_max_rows": (_I, []),
    "npi_csr_filter_workspace_elems": (_I, [_I]),
    "npi_csr_filter": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "npi_readout_max_mean": (c_int, [_P, _I, _P, _I, _I, _P, _P]),
    "npi_topk_gather_bwd": (c_int, [_P, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P]),
    "npi_topk_gather_bwd_ex": (c_int, [_P, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P]),
    "npi_topk_weight_grad_workspace_elems": (_I, [_I, _I]),
    "npi_topk_weight_grad": (c_int, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P]),
    "npi_readout_max_mean_bwd": (c_int, [_P, _I, _P, _I, _I, _P, _P, _P, _I, _P]),
    "npi_readout_max_mean_bwd_ex": (c_int, [_P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P]),
    "npi_confusion_update": (c_int, [_P, _I, _I, _P, _I, _P, _P]),
    "npi_mlp_head_fwd": (c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, c_float, c_int,
                                 _P, _P, _P, _P, _P]),
    "npi_mlp_head_workspace_elems": (_I, [_I, _I, _I, _I]),
    "npi_mlp_head_bwd": (c_int, [_I, _I, _I, _I, _I, _P, _P, _P, _P, c_float, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                 _P, _I, _P]),
    "npi_subgraph_sizes": (c_int, [_P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "npi_subgraph_fill": (c_int, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "npi_subgraph_features": (c_int, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _P]),
    # enclosing subgraphs under Rule H: the parent's by-target CSR (rowptr, col, eid), mask, N, keys, B | ... | the label kernel alone
    "npi_enclose_workspace_bytes": (_I, [_I, _I]),
    "npi_enclose_sizes": (c_int, [_P, _P, _P, _P, _I, _P, _I, _I, c_int, _P, _P, _P, _P, _I, _P, _P]),
    "npi_enclose_fill": (c_int, [_P, _P, _P, _P, _I, _P, _I, c_int, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "npi_drnl_label": (c_int, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P]),
    "npi_enclose_features": (c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, c_int, _P, _I, _P]),
    "npi_sample_counts": (c_int, [_P, _I, _P, _I, _I, c_float, _P, _P, _P]),
    "npi_sample_select": (c_int, [_P, _P, _P, _I, _P, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P]),
    "npi_sample_workspace_elems": (_I, [_I]),
    "npi_sample_relabel_count": (c_int, [_P, _P, _I, _I, _P, c_int, _P, _I, _P, _P, _P]),
    "npi_sample_relabel": (c_int, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "npi_sample_union": (c_int, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "npi_sample_coalesce_workspace_bytes": (_I, [_I]),
    "npi_sample_coalesce": (c_int, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "npi_negative_candidates": (c_int, [_P, _P, _I, _I, _I, _I, _I, c_int, _P, _P, _P]),
    "npi_negative_targets": (c_int, [_P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P]),
    "npi_negative_distinct_workspace_bytes": (_I, [_I]),
    "npi_negative_distinct": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "npi_random_walk": (c_int, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "npi_walk_pairs": (c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "npi_pair_score_workspace_bytes": (_I, [_I]),
    "npi_pair_score": (c_int, [_P, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, c_int, _P, _P, _P, _P, _I, _P, _P]),
    "npi_group_score_workspace_bytes": (_I, [_I, _I]),
    "npi_group_score": (c_int, [_P, _P, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, c_int, c_float, c_float, _P, _P, _P, _P, _I, _P, _P]),
    "npi_gauss_workspace_bytes": (_I, [_I, _I]),
    "npi_gauss_sample_kl": (c_int, [_P, _I, _P, _I, _I, _I, _I, c_float, _I, _P, c_int, c_int, _P, _I, _P, _P, _I, _P]),
    "npi_gauss_sample_kl_bwd": (c_int, [_P, _I, _P, _I, _I, _I, _I, c_float, _I, _P, c_int, c_int, _P, _I, _P, _P, _I, _P, _I, _P]),
    "npi_gauss_noise": (c_int, [_I, _I, _I, _P, c_int, _P, _I, _P]),
    "npi_rank_workspace_bytes": (_I, [_I]),
    "npi_rank_metrics": (c_int, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "npi_split_workspace_bytes": (_I, [_I]),
    "npi_split_permute": (c_int, [_P, _P, _I, _I, _I, _I, c_int, _P, _P, _P, _P, _P, _P, _I, _P]),
    "npi_split_canonical": (c_int, [_P, _P, _I, _P]),
    "npi_split_undirected_workspace_bytes": (_I, [_I]),
    "npi_split_undirected": (c_int, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "npi_topk_links_workspace_bytes": (_I, [_I, _I, _I, _I]),
    "npi_topk_links": (c_int, [_P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, c_int, _I, _P, _P, _P, _I, _P, _P]),
    "npi_link_ranks_workspace_bytes": (_I, [_I, _I, _I]),
    "npi_link_ranks": (c_int, [_P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P, c_int, _I, _P, _P, _P, _I, _P, _P]),
    "npi_softmax_link_workspace_bytes": (_I, [_I, _I, _I, _I, _I]),
    "npi_softmax_link_fwd": (c_int, [_P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P, c_int, c_float, _I, _P, _P, _P, _P, _I, _P, _P]),
    "npi_softmax_link_bwd_src": (c_int, [_P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P, c_int, c_float, _I, _P, _P, _P, _P, _I, _P]),
    "npi_softmax_link_bwd_dst": (c_int, [_P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P, c_int, c_float, _I, _P, _P, _P, _P, _I, _P]),
    "npi_segmax_workspace_bytes": (_I, [_I, _I, _I]),
    "npi_segmax": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _P, _I, _P, _I, _P]),
    "npi_segmax_bwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _I, _P, _I, _P]),
    # readouts under Rule O: x, ldx, graph_ptr, N, B, F, out, ldo, workspace, bytes | ... m, s ... | order / remap, k
    "npi_readout_add_workspace_bytes": (_I, [_I, _I, _I]),
    "npi_readout_add": (c_int, [_P, _I, _P, _I, _I, _I, _P, _I, _P, _I, _P]),
    "npi_readout_add_bwd": (c_int, [_P, _I, _P, _I, _I, _I, _P, _I, _P]),
    "npi_readout_attention_workspace_bytes": (_I, [_I, _I, _I]),
    "npi_readout_attention": (c_int, [_P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _I, _P]),
    "npi_readout_attention_bwd": (c_int, [_P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "npi_sort_pool_keys": (c_int, [_P, _I, _I, _I, _P, _P]),
    "npi_sort_pool_gather": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "npi_sort_pool_bwd": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _P]),
    # DropEdge under Rule E: key, tick (device word or NULL), threshold (the uint64's bits), flags
    "npi_drop_edges_workspace_elems": (_I, [_I]),
    "npi_csr_drop_side": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, c_int, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "npi_drop_edge_list": (c_int, [_P, _P, _I, _I, _P, _I, c_int, _P, _P, _P, _P, c_int, _P, _I, _P]),
    "npi_drop_edge_keep": (c_int, [_P, _P, _I, _I, _P, _I, c_int, _P, _P]),
}

_lib = None


class NpiError(RuntimeError):
    pass


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """dlopen the C-ABI library and attach prototypes.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NpiError(
            f"{path} is missing: the HIP extension has not been built "
            "(run `python -m npi_gnn_amd.build`).  npi_gnn_amd has no CPU fallback.")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().npi_last_error()
        raise NpiError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def require_gpu(*tensors) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NpiError("npi_gnn_amd kernels run on MI355X (HIP) tensors only; got a "
                           f"{t.device} tensor.  There is no CPU fallback.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise NpiError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device) -> int:
    """hipStream_t of torch's current stream on ``device`` (the raw-handle call is ~20x cheaper than building a
    ``torch.cuda.Stream`` object; the small-batch step makes some 20 of these)"""
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream
