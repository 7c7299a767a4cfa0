"""``NeighborSampler.sample_subgraph`` / ``subgraphs`` on the GPU: every field of the ``SubgraphBatch`` against the numpy restatement
``tests/_subgraph_flow_ref.py`` element for element, the union property against the bipartite flow of the same sampler without the
restatement, both paths of the radix sort, the edge cases, reproducibility, and one subgraph through the square layers against
``oracle.ref_conv`` in fp64 with the bars of ``tests/test_gpu_sampler.py`` (out / dX 1e-4 per row scale, parameter gradients
``GRAD_REL`` by ``rel_max``).  The graph is the hand-made one of ``tests/test_gpu_sampler.py``."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from oracle import ref_conv as R
from _util import GRAD_REL, rel_max
import _subgraph_flow_ref as sref
from test_gpu_sampler import DEGREES, HUB, HUB_DEG, N, SEED, _graph, _row_scaled, _sampler

pytestmark = pytest.mark.gpu

SMALL_SORT_KEYS = 64 * 4096          # up to this many entries the radix sort derives its offsets per workgroup; above, it scans


def _batch(which):
    if which == "all":
        return torch.arange(N)
    g = torch.Generator().manual_seed(6)
    return torch.cat([torch.tensor([0, HUB, 15, 15]), torch.randperm(N, generator=g)[:296]])    # no in-edge, the hub, an id twice


def _equal(sub, want, b_id):
    n_id, sub_b_id, ei, e_id, U = want
    assert sub.num_nodes == U
    assert torch.equal(sub.n_id.cpu(), torch.from_numpy(n_id))
    assert torch.equal(sub.sub_b_id.cpu(), torch.from_numpy(sub_b_id))
    assert torch.equal(sub.edge_index.cpu(), torch.from_numpy(ei))
    assert torch.equal(sub.e_id.cpu(), torch.from_numpy(e_id))
    assert torch.equal(sub.b_id.cpu(), b_id)
    for t in (sub.n_id, sub.sub_b_id, sub.edge_index, sub.e_id):
        assert t.dtype == torch.int64
    assert sub.edge_index.is_contiguous() and tuple(sub.edge_index.shape) == (2, ei.shape[1])


# ---- 1. equality with the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "some"])
@pytest.mark.parametrize("size", [[5, 3], [25, 10], [0.5, 0.5]])
def test_subgraph_equals_the_restatement(dev, size, which):
    b_id = _batch(which)
    sub = _sampler(dev, size, num_hops=2).sample_subgraph(b_id.to(dev), SEED)
    _equal(sub, sref.subgraph_flow(_graph()[1], b_id.numpy(), size, SEED), b_id)
    npi.graph.check_pending()


# ---- 2. the union of the bipartite flow's blocks, without the restatement -------------------------------------------------------------------
def _block_edges(flow):
    """(src, dst, e_id) with global ids of every sampled entry of a DataFlow"""
    src, dst, eid = [], [], []
    targets = flow.n_id
    for block in flow.blocks:                                    # in the order they were produced: hop 0 first
        src.append(block.n_id[block.edge_index[0]])
        dst.append(targets[block.edge_index[1]])
        eid.append(block.e_id)
        targets = block.n_id
    return torch.cat(src).cpu(), torch.cat(dst).cpu(), torch.cat(eid).cpu()


@pytest.mark.parametrize("size", [[5, 3], [25, 10], [0.5, 0.5]])
def test_subgraph_is_the_union_of_the_blocks(dev, size):
    ei = _graph()[0]
    b_id = _batch("some")
    sampler = _sampler(dev, size, num_hops=2, add_self_loops=True)            # the switch plays no part in this flow
    sub = sampler.sample_subgraph(b_id.to(dev), SEED)
    flow = _sampler(dev, size, num_hops=2, add_self_loops=False).sample(b_id.to(dev), SEED)
    src, dst, eid = _block_edges(flow)
    n_id, lei, e_id, U = sub.n_id.cpu(), sub.edge_index.cpu(), sub.e_id.cpu(), sub.num_nodes
    key = src * N + dst
    got = n_id[lei[0]] * N + n_id[lei[1]]
    assert torch.equal(torch.unique(key), torch.unique(got)) and got.numel() == torch.unique(got).numel()
    assert torch.equal(ei[0][e_id], n_id[lei[0]]) and torch.equal(ei[1][e_id], n_id[lei[1]])       # a column with exactly that pair
    order = torch.argsort(key * ei.size(1) + eid)                           # by pair, then by column
    first = torch.ones(key.numel(), dtype=torch.bool)
    first[1:] = key[order][1:] != key[order][:-1]
    want_min = dict(zip(key[order][first].tolist(), eid[order][first].tolist()))
    assert [want_min[k] for k in got.tolist()] == e_id.tolist()            # the minimum over the blocks' e_ids with that pair
    idx = lei[0] * U + lei[1]
    assert bool((idx[1:] > idx[:-1]).all())                                 # strictly ascending: no pair twice
    assert bool((n_id[1:] > n_id[:-1]).all()) and U == n_id.numel()
    assert torch.equal(n_id[sub.sub_b_id.cpu()], b_id)
    want_ids = torch.unique(torch.cat([b_id] + [b.n_id.cpu() for b in flow.blocks]))
    assert torch.equal(n_id, want_ids)
    npi.graph.check_pending()


# ---- 3. both paths of the radix sort ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops,above", [(2, False), (4, True)])
def test_take_all_budget_on_both_sort_paths(dev, hops, above):
    ei, csr = _graph()
    b_id = torch.arange(N)
    size = [HUB_DEG + 5] * hops
    sampler = _sampler(dev, size, num_hops=hops)
    flow = sampler.sample(b_id.to(dev), SEED)
    total = sum(int(b.e_id.numel()) for b in flow)
    print("concatenated sampled entries:", total)
    assert (total > SMALL_SORT_KEYS) == above, total
    sub = sampler.sample_subgraph(b_id.to(dev), SEED)
    # every node is a target of hop 0 and every in-edge is taken: the distinct pairs of the whole edge list
    pairs = torch.unique(ei[0] * N + ei[1])
    assert sub.edge_index.size(1) == pairs.numel() and sub.num_nodes == N
    assert torch.equal(sub.edge_index[0].cpu() * N + sub.edge_index[1].cpu(), pairs)            # n_id = arange: local ids are global
    _equal(sub, sref.subgraph_flow(csr, b_id.numpy(), size, SEED), b_id)
    npi.graph.check_pending()


# ---- 4. edge cases -----------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_one_node_without_in_edges(dev):
    sub = _sampler(dev, [5, 3], num_hops=2).sample_subgraph(torch.tensor([0], device=dev), SEED)
    assert sub.n_id.tolist() == [0] and tuple(sub.edge_index.shape) == (2, 0) and sub.sub_b_id.tolist() == [0]
    assert sub.num_nodes == 1 and sub.e_id.numel() == 0 and sub.edge_index.dtype == torch.int64
    npi.graph.check_pending()


def test_a_one_hop_sampler(dev):
    b_id = _batch("some")
    sub = _sampler(dev, 5).sample_subgraph(b_id.to(dev), SEED)
    _equal(sub, sref.subgraph_flow(_graph()[1], b_id.numpy(), [5], SEED), b_id)
    k = np.minimum(np.array(DEGREES), 5)
    assert int((sub.n_id[sub.edge_index[1]] == 15).sum()) <= k[15]


def test_out_of_range_batch_ids_are_reported(dev):
    sampler = _sampler(dev, [5, 3], num_hops=2)
    npi.graph.check_pending()
    with pytest.raises(IndexError):
        sampler.sample_subgraph(torch.tensor([3, N + 4, -1, 15], device=dev), SEED)
    assert int(sampler._scratch.abs().max()) == 0                                   # the scratch is clean after the error too
    sub = sampler.sample_subgraph(torch.tensor([3, 15], device=dev), SEED)          # and the sampler still works
    assert torch.equal(sub.n_id[sub.sub_b_id].cpu(), torch.tensor([3, 15]))
    npi.graph.check_pending()


def test_scratch_is_zero_after_twenty_batches(dev):
    sampler = _sampler(dev, [25, 10], num_hops=2, batch_size=150, shuffle=True)
    subs = list(sampler.subgraphs(None))
    assert len(subs) == 20 and sampler.epoch == 1
    assert sampler._scratch.numel() == N and int(sampler._scratch.abs().max()) == 0
    npi.graph.check_pending()


def test_sampling_a_subgraph_inside_a_capture_raises(dev):
    sampler = _sampler(dev, 5)
    targets = torch.arange(10, device=dev)
    sampler.sample_subgraph(targets, SEED)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        with pytest.raises(npi.NpiError, match="capture"):
            sampler.sample_subgraph(targets, SEED)
    torch.cuda.synchronize()
    assert int(sampler._scratch.abs().max()) == 0


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------------
def test_same_seed_and_epoch_give_the_same_subgraphs(dev):
    def epoch(seed, epoch_no, flow=False):
        s = _sampler(dev, [5, 3], num_hops=2, batch_size=700, shuffle=True, seed=seed)
        s.epoch = epoch_no
        return list(s(None)) if flow else list(s.subgraphs(None))
    a, b, c = epoch(9, 2), epoch(9, 2), epoch(9, 3)
    assert len(a) == len(b) == 5
    for sa, sb in zip(a, b):
        for name in ("edge_index", "e_id", "n_id", "b_id", "sub_b_id"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), name
        assert sa.num_nodes == sb.num_nodes
    assert not torch.equal(a[0].b_id, c[0].b_id)
    flows = epoch(9, 2, flow=True)
    assert len(flows) == 5 and all(torch.equal(f.n_id, s.b_id) for f, s in zip(flows, a))       # the batches of __call__
    assert torch.equal(torch.cat([s.b_id for s in a]).sort().values.cpu(), torch.arange(N))


# ---- 6. through the square layers ----------------------------------------------------------------------------------------------------------
def _check(got, want, names, bars):
    for g_, w_, name, bar in zip(got, want, names, bars):
        err = _row_scaled(g_, w_) if bar == "row" else rel_max(g_, w_)
        print(f"   {name}: {err:.2e}")
        assert err < (1e-4 if bar == "row" else GRAD_REL), (name, err)


_SUB = {}


def _sub_for_layers(dev):
    if "sub" not in _SUB:
        _SUB["sub"] = _sampler(dev, [5, 3], num_hops=2).sample_subgraph(_batch("some").to(dev), SEED)
    return _SUB["sub"]


def _loss_grad(sub, out_dim, seed):
    """the gradient of a loss taken on out[sub_b_id] only: one row per batch id (a repeated id takes two), fp64 on the host"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sub.sub_b_id.numel(), out_dim, generator=g).double()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_two_layers_over_the_subgraph(dev, kind):
    sub = _sub_for_layers(dev)
    ei, U = sub.edge_index.cpu(), sub.num_nodes
    g = torch.Generator().manual_seed(7)
    x = torch.randn(U, 32, generator=g).double()
    W1, b1 = (torch.randn(32, 16, generator=g) / 6).double(), torch.randn(16, generator=g).double()
    W2, b2 = (torch.randn(16, 8, generator=g) / 4).double(), torch.randn(8, generator=g).double()
    go = _loss_grad(sub, 8, 9)
    layer = R.gcn_conv if kind == "gcn" else R.sage_conv
    xr, W1r, b1r, W2r, b2r = (t.clone().requires_grad_(True) for t in (x, W1, b1, W2, b2))
    want = layer(layer(xr, ei, W1r, b1r).relu(), ei, W2r, b2r)
    want[sub.sub_b_id.cpu()].backward(go)
    Conv = npi.GCNConv if kind == "gcn" else npi.SAGEConv
    conv1, conv2 = Conv(32, 16).to(dev), Conv(16, 8).to(dev)
    with torch.no_grad():
        conv1.weight.copy_(W1)
        conv1.bias.copy_(b1)
        conv2.weight.copy_(W2)
        conv2.bias.copy_(b2)
    xg = x.float().to(dev).requires_grad_(True)
    graph = sub.graph()
    assert graph is sub.graph() and graph.num_nodes == U
    out = conv2(conv1(xg, graph).relu(), graph)
    out[sub.sub_b_id].backward(go.float().to(dev))
    _check([out, xg.grad, conv1.weight.grad, conv1.bias.grad, conv2.weight.grad, conv2.bias.grad],
           [want, xr.grad, W1r.grad, b1r.grad, W2r.grad, b2r.grad], ["out", "dX", "dW1", "db1", "dW2", "db2"],
           ["row", "row", "rel", "rel", "rel", "rel"])
    npi.graph.check_pending()


def test_gat_over_the_subgraph(dev):
    sub = _sub_for_layers(dev)
    ei, U = sub.edge_index.cpu(), sub.num_nodes
    heads, C, Fin = 2, 8, 32
    g = torch.Generator().manual_seed(8)
    x = torch.randn(U, Fin, generator=g).double()
    W = (torch.randn(Fin, heads * C, generator=g) / Fin ** 0.5).double()
    att = (torch.randn(1, heads, 2 * C, generator=g) / C ** 0.5).double()
    b = torch.randn(heads * C, generator=g).double()
    go = _loss_grad(sub, heads * C, 10)
    xr, Wr, ar, br = (t.clone().requires_grad_(True) for t in (x, W, att, b))
    want = R.gat_conv(xr, ei, Wr, ar, br, heads=heads)
    want[sub.sub_b_id.cpu()].backward(go)
    conv = npi.GATConv(Fin, C, heads=heads).to(dev)
    with torch.no_grad():
        conv.weight.copy_(W)
        conv.att.copy_(att)
        conv.bias.copy_(b)
    xg = x.float().to(dev).requires_grad_(True)
    out = conv(xg, sub.graph())
    out[sub.sub_b_id].backward(go.float().to(dev))
    _check([out, xg.grad, conv.weight.grad, conv.att.grad, conv.bias.grad], [want, xr.grad, Wr.grad, ar.grad, br.grad],
           ["out", "dX", "dW", "d att", "db"], ["row", "row", "rel", "rel", "rel"])


def test_a_graph_batch_of_the_subgraph_through_sage(dev):
    """the one-id-space plumbing takes the subgraph: GraphBatch needs no ``batch`` vector (one graph)"""
    sub = _sub_for_layers(dev)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(sub.num_nodes, 32, generator=g)
    conv = npi.SAGEConv(32, 8).to(dev)
    gb = npi.GraphBatch(x.to(dev), sub.edge_index, csr=sub.graph())
    out = conv(gb)
    assert isinstance(out, npi.GraphBatch) and out.num_graphs == 1 and out.peek_graph() is sub.graph()
    want = R.sage_conv(x.double(), sub.edge_index.cpu(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu())
    assert _row_scaled(out.x, want) < 1e-4
