"""The one-id-space data flow of the neighbour sampler without a GPU: the numpy restatement ``tests/_subgraph_flow_ref.py`` against
a literal torch-CPU transcription of PyG 1.4.2 ``NeighborSampler.__produce_subgraph__`` fed the same per-hop samples, the
restatement's own order and minimum-``e_id`` rule, the new C-ABI symbols and their argument errors, and the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import sampler as S
import _sampler_ref as ref
import _subgraph_flow_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_sample_union", "npi_sample_coalesce_workspace_bytes", "npi_sample_coalesce")

#: columns (source -> target): 3->0 twice (parallel), a (1, 1) column, nothing into 2 (which is in the batch), 1 a target of both
#: hops through its own loop, 6->4 twice
EI = np.array([[3, 4, 3, 1, 5, 0, 6, 7, 6, 2],
               [0, 0, 0, 1, 1, 3, 4, 5, 4, 6]])
NODES = 8
BATCH = [0, 2, 0, 1]                                        # a repeated id, and the node without an in-edge


def pyg_produce_subgraph(edge_index, num_nodes, b_id, e_ids_per_hop):
    """``__produce_subgraph__`` of PyG 1.4.2 line by line, the ``neighbor_sampler`` call replaced by the given samples (columns
    of ``edge_index`` per hop)"""
    edge_index = torch.as_tensor(edge_index)
    tmp = torch.empty(num_nodes, dtype=torch.long)
    b_id = torch.as_tensor(b_id)
    n_ids, e_ids, edge_indices = [b_id], [], []
    for e_id in e_ids_per_hop:
        e_id = torch.as_tensor(e_id)
        n_id = edge_index[0].index_select(0, e_id)
        n_id = n_id.unique(sorted=False)
        n_ids.append(n_id)
        e_ids.append(e_id)
        edge_indices.append(edge_index.index_select(1, e_id))
    n_id = torch.unique(torch.cat(n_ids, dim=0), sorted=False)
    tmp[n_id] = torch.arange(n_id.size(0))
    e_id = torch.cat(e_ids, dim=0)
    edge_index = tmp[torch.cat(edge_indices, dim=1)]
    num_nodes = n_id.size(0)
    idx = edge_index[0] * num_nodes + edge_index[1]
    idx, inv = idx.unique(sorted=False, return_inverse=True)
    edge_index = torch.stack([idx // num_nodes, idx % num_nodes], dim=0)
    e_id = e_id.new_zeros(edge_index.size(1)).scatter_(0, inv, e_id)
    return edge_index, e_id, n_id, tmp[b_id], num_nodes


@pytest.mark.parametrize("sizes", [[10, 10], [1, 2], [2, 1, 2], [0.5, 1.0]])
def test_restatement_equals_the_pyg_transcription(sizes):
    csr = ref.by_target_csr(EI, NODES)
    seed = ref.epoch_seed(5, 0)
    n_id, sub_b_id, ei, e_id, U = sref.subgraph_flow(csr, BATCH, sizes, seed)
    blocks = ref.data_flow(csr, np.array(BATCH), sizes, seed, add_self_loops=False)
    p_ei, p_e_id, p_n_id, p_sub, p_U = pyg_produce_subgraph(EI, NODES, BATCH, [b[2] for b in blocks])
    assert U == p_U == len(n_id) and set(n_id.tolist()) == set(p_n_id.tolist())
    assert p_n_id[p_sub].tolist() == BATCH == n_id[sub_b_id].tolist()
    pairs = set(zip(n_id[ei[0]].tolist(), n_id[ei[1]].tolist()))
    p_pairs = set(zip(p_n_id[p_ei[0]].tolist(), p_n_id[p_ei[1]].tolist()))
    assert pairs == p_pairs and len(pairs) == ei.shape[1] == p_ei.size(1)
    # the restatement's own rules: ascending ids, ascending pairs, the smallest column of each pair among ALL sampled entries
    assert (np.diff(n_id) > 0).all() and {0, 1, 2} <= set(n_id.tolist())
    assert (np.diff(ei[0] * U + ei[1]) > 0).all()
    src_g, dst_g, eid, _ = sref.hop_entries(csr, BATCH, sizes, seed)
    for c in range(ei.shape[1]):
        s, d = n_id[ei[0, c]], n_id[ei[1, c]]
        merged = eid[(src_g == s) & (dst_g == d)]
        assert e_id[c] == merged.min() and EI[0, e_id[c]] == s and EI[1, e_id[c]] == d
        p_c = [k for k in range(p_ei.size(1)) if (p_n_id[p_ei[0, k]], p_n_id[p_ei[1, k]]) == (s, d)]
        assert len(p_c) == 1 and int(p_e_id[p_c[0]]) in merged.tolist()           # PyG keeps ONE of them, whichever
    assert 2 not in n_id[ei[1]].tolist()                                          # node 2: in the batch, isolated as a target


def test_take_all_case_by_hand():
    """budget above every degree, two hops from [0, 2, 0, 1]: T_1 = {1, 3, 4, 5}, T_2 = {0, 1, 5, 6, 7}; every edge except 2->6"""
    n_id, sub_b_id, ei, e_id, U = sref.subgraph_flow(ref.by_target_csr(EI, NODES), BATCH, [10, 10], 1)
    assert n_id.tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and sub_b_id.tolist() == [0, 2, 0, 1] and U == 8
    assert ei.tolist() == [[0, 1, 3, 4, 5, 6, 7], [3, 1, 0, 0, 1, 4, 5]]
    assert e_id.tolist() == [5, 3, 0, 1, 4, 6, 7]                                 # 3->0: columns 0 and 2; 6->4: columns 6 and 8
    none = sref.subgraph_flow(ref.by_target_csr(EI, NODES), [2], [10, 10], 1)
    assert none[0].tolist() == [2] and none[1].tolist() == [0] and none[2].shape == (2, 0) and none[3].shape == (0,)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert "__produce_subgraph__" in header                                         # the call replaced
    assert _lib.load().npi_abi_version() == 4
    import test_boundary_cpu as B
    B.test_every_declared_symbol_is_exported_and_bound()
    B.test_ctypes_prototypes_have_the_headers_argument_lists()
    B.test_the_library_allocates_nothing_and_keeps_no_state()


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N = None
    calls = {
        "npi_sample_union (negative count)": lambda: lib.npi_sample_union(8, 8, -1, 8, 4, 16, 4, 8, 4, 8, 8, 8, 8, 8, N, N),
        "npi_sample_union (negative batch)": lambda: lib.npi_sample_union(8, 8, 4, 8, -4, 16, 4, 8, 4, 8, 8, 8, 8, 8, N, N),
        "npi_sample_union (more ids than nodes)": lambda: lib.npi_sample_union(8, 8, 4, 8, 4, 16, 4, 8, 5, 8, 8, 8, 8, 8, N, N),
        "npi_sample_union (null)": lambda: lib.npi_sample_union(N, N, 4, N, 4, N, 4, N, 4, N, N, N, N, N, N, N),
        "npi_sample_union (alignment)": lambda: lib.npi_sample_union(8, 8, 4, 8, 4, 20, 4, 8, 4, 8, 8, 8, 8, 8, N, N),
        "npi_sample_coalesce (negative count)": lambda: lib.npi_sample_coalesce(8, 8, 8, -1, 4, 8, 8, 8, 8, 16, 1 << 20, N),
        "npi_sample_coalesce (negative ids)": lambda: lib.npi_sample_coalesce(8, 8, 8, 4, -1, 8, 8, 8, 8, 16, 1 << 20, N),
        "npi_sample_coalesce (null)": lambda: lib.npi_sample_coalesce(N, N, N, 4, 4, N, N, N, N, N, 0, N),
        "npi_sample_coalesce (alignment)": lambda: lib.npi_sample_coalesce(8, 8, 8, 4, 4, 8, 8, 8, 8, 20, 1 << 20, N),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.split()[0].encode() in lib.npi_last_error(), (name, lib.npi_last_error())
    # a workspace that is too small: refused before anything is launched, sized by the query
    assert lib.npi_sample_coalesce_workspace_bytes(-1) == -1 and lib.npi_sample_coalesce_workspace_bytes(1000) >= 16 * 1000
    assert lib.npi_sample_coalesce(8, 8, 8, 4, 4, 8, 8, 8, 8, 16, 10, N) == -3 and b"npi_sample_coalesce" in lib.npi_last_error()
    # nothing to do: no launch, no error
    assert lib.npi_sample_union(N, N, 0, N, 0, N, 4, N, 0, N, N, N, N, N, N, N) == 0
    assert lib.npi_sample_coalesce(N, N, N, 0, 0, N, N, N, N, N, 0, N) == 0


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def test_subgraph_batch_and_sampler_surface():
    assert npi.SubgraphBatch is S.SubgraphBatch and "SubgraphBatch" in npi.__all__
    assert set(S.SubgraphBatch.__slots__) >= {"edge_index", "e_id", "n_id", "b_id", "sub_b_id", "num_nodes"}
    sub = npi.SubgraphBatch(torch.zeros((2, 3), dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.arange(4), torch.tensor([2, 2]),
                            torch.tensor([2, 2]), 4)
    assert sub.num_nodes == 4 and sub.to("cpu") is sub and "num_nodes=4" in repr(sub) and "edges=3" in repr(sub)
    with pytest.raises(npi.NpiError):
        sub.graph()                                                                  # no CPU fallback
    assert callable(npi.NeighborSampler.sample_subgraph) and callable(npi.NeighborSampler.subgraphs)
    with pytest.raises(ValueError, match="bipartite"):
        npi.NeighborSampler(torch.tensor([[0, 1], [1, 0]]), 2, size=2, bipartite=False)


def test_subgraphs_and_call_run_over_the_same_batches():
    """with the device part out of reach: same (seed, epoch) -> the same id lists in both flows, and both count ``epoch`` up"""
    def make():
        s = object.__new__(npi.NeighborSampler)
        s.device, s.num_nodes, s.batch_size, s.shuffle, s.drop_last, s.seed, s.epoch = torch.device("cpu"), 300, 64, True, False, 5, 0
        s.sample = lambda targets, seed=None: (targets, seed)
        s.sample_subgraph = lambda targets, seed=None: (targets, seed)
        return s
    a, b = make(), make()
    for _ in range(2):
        fa, fb = list(a(None)), list(b.subgraphs(None))
        assert len(fa) == len(fb) == 5 and a.epoch == b.epoch
        assert all(torch.equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(fa, fb))
    assert a.epoch == 2
