"""numpy restatement of the one-id-space data flow of ``include/npi_gnn.h`` (PyG 1.4.2 ``NeighborSampler.__produce_subgraph__`` with
the orders this project fixes), on top of ``_sampler_ref.data_flow(..., add_self_loops=False)``.  Pure numpy: it shares no code with
the package."""
import numpy as np

import _sampler_ref as ref


def hop_entries(csr, b_id, sizes, seed):
    """the sampled entries of all hops, concatenated, with GLOBAL ids: (src_g, dst_g, eid), and the hops' source sets T_1 .. T_L"""
    targets = np.asarray(b_id, dtype=np.int64)
    src_g, dst_g, eid, sets = [], [], [], []
    for n_id, _, e_id, lei in ref.data_flow(csr, targets, sizes, seed, add_self_loops=False):
        src_g.append(n_id[lei[0]])
        dst_g.append(targets[lei[1]])
        eid.append(e_id)
        sets.append(n_id)
        targets = n_id
    return np.concatenate(src_g), np.concatenate(dst_g), np.concatenate(eid), sets


def subgraph_flow(csr, b_id, sizes, seed):
    """(n_id, sub_b_id, edge_index [2, E_u], e_id, num_nodes): n_id ascending, columns in ascending (src_local, dst_local) order,
    e_id the smallest merged column"""
    b_id = np.asarray(b_id, dtype=np.int64)
    src_g, dst_g, eid, sets = hop_entries(csr, b_id, sizes, seed)
    n_id = np.unique(np.concatenate([b_id] + sets))
    U = len(n_id)
    idx = np.searchsorted(n_id, src_g) * U + np.searchsorted(n_id, dst_g)
    order = np.lexsort((eid, idx))                          # by pair, then by column: the first of a run carries the smallest
    uniq, first = np.unique(idx[order], return_index=True)
    edge_index = np.stack([uniq // U, uniq % U]) if U else np.zeros((2, 0), dtype=np.int64)
    return n_id, np.searchsorted(n_id, b_id), edge_index.astype(np.int64), eid[order][first].astype(np.int64), U
