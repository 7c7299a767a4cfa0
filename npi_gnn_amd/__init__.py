"""npi_gnn_amd -- MI355X-native message-passing engine for NPI-GNN's conv hot path.

Only what the path needs: ``csrc/`` (hand-written gfx950 kernels + the C ABI of
``include/npi_gnn.h``), ``graph`` (device CSR build), ``functional`` / ``nn`` (the PyG
``nn.Conv`` interface the reference calls at ``src/classes.py:48-52,62-70``) and ``dist``
(row sharding over RCCL).  The package directory is ``npi_gnn_amd`` because a hyphen cannot
be imported.
"""
from ._lib import LIB_PATH, NpiError, load  # noqa: F401
from .graph import BipartiteGraph, CSRGraph, GraphBatch, as_graph, set_debug  # noqa: F401
from .functional import (GCNNorm, GaussianNoise, gat_conv, gat_conv_bipartite, gaussian_noise, gcn_conv, group_scores,  # noqa: F401
                         link_loss, pair_scores, ranking_loss, reparametrize_kl, sage_conv, sage_conv_bipartite, segmax, segsum)
from .nn import GATConv, GCNConv, SAGEConv  # noqa: F401
from .schedule import Schedule  # noqa: F401
from .graphed import GraphedStack  # noqa: F401
from .sampler import Block, DataFlow, NeighborSampler, SubgraphBatch  # noqa: F401
from .negative import NegativeSampler, negative_sampling, structured_negative_sampling  # noqa: F401
from .autoencoder import ARGA, ARGVA, GAE, VGAE, InnerProductDecoder  # noqa: F401
from .walk import Node2Vec, RandomWalker, random_walk  # noqa: F401
from .rank import average_precision_score, precision_recall_curve, rank_metrics, roc_auc_score, roc_curve  # noqa: F401
from .split import EdgeSplitter, to_undirected, train_test_split_edges  # noqa: F401
from .topk import KnownLinks, topk_links  # noqa: F401
from .link_rank import LinkRanks, link_ranks, ranking_metrics  # noqa: F401
from .softmax_link import link_log_softmax, listwise_loss  # noqa: F401
from .dropedge import DropEdge, drop_edge_mask, dropout_adj  # noqa: F401
from .enclose import EnclosingBatch, EnclosingSubgraphs, drnl_node_labeling  # noqa: F401

__all__ = ["CSRGraph", "GraphBatch", "as_graph", "set_debug", "GCNNorm", "gat_conv", "gcn_conv", "sage_conv", "segmax", "segsum",
           "GATConv", "GCNConv", "SAGEConv", "Schedule", "GraphedStack", "NeighborSampler", "DataFlow", "Block", "SubgraphBatch", "NegativeSampler", "negative_sampling",
           "structured_negative_sampling", "InnerProductDecoder", "GAE", "VGAE", "ARGA", "ARGVA", "GaussianNoise", "gaussian_noise", "reparametrize_kl", "RandomWalker", "random_walk", "Node2Vec", "pair_scores", "link_loss", "group_scores", "ranking_loss", "rank_metrics",
           "roc_auc_score", "average_precision_score", "roc_curve", "precision_recall_curve", "EdgeSplitter",
           "train_test_split_edges", "to_undirected", "KnownLinks", "topk_links", "LinkRanks", "link_ranks", "ranking_metrics", "link_log_softmax", "listwise_loss", "DropEdge", "drop_edge_mask", "dropout_adj", "EnclosingSubgraphs", "EnclosingBatch", "drnl_node_labeling",
           "NpiError", "load", "LIB_PATH"]
