"""``npi.NeighborSampler`` on the GPU: every block against the numpy restatement of the sampling rule (``tests/_sampler_ref.py``,
checked by ``tests/test_sampler_cpu.py``) element for element, structural properties checked independently of it, and the blocks
through the bipartite layers against the fp64 restatement ``tests/_bipartite_ref.py`` with the bars of ``tests/test_gpu_bipartite.py``
(out / dX 1e-4 per row scale, parameter gradients ``GRAD_REL`` by ``rel_max``)."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from _util import GRAD_REL, rel_max
import _bipartite_ref as bref
import _sampler_ref as ref
from test_sampler_cpu import HUB_STAT_SEED, STAT_SEED

pytestmark = pytest.mark.gpu

N = 3000
HUB, HUB_DEG = 16, 70_000
#: in-degrees of nodes 0 .. 16: the empty row, take-all rows, k - 1 / k / k + 1 for k = 5 and 25 (and 1: degrees 0, 1, 2), both sides
#: of a wavefront (64) and of a workgroup (256), a row kept whole in LDS (1,025) and the hub, which is filtered by a threshold
DEGREES = [0, 1, 2, 4, 5, 6, 24, 25, 26, 63, 64, 65, 255, 256, 257, 1025, HUB_DEG]
SEED = ref.epoch_seed(3, 0)


def _row_scaled(got, ref_):
    got, ref_ = got.detach().double().cpu(), ref_.detach().double().cpu()
    return float(((got - ref_).abs() / (1.0 + ref_.abs().amax(1, keepdim=True))).max())


_CACHE = {}


def _graph():
    """the hand-made graph (host LongTensor [2, E], shuffled columns) and its by-target CSR in numpy; built once"""
    if "graph" not in _CACHE:
        g = torch.Generator().manual_seed(1)
        deg = torch.randint(0, 9, (N,), generator=g)
        deg[: len(DEGREES)] = torch.tensor(DEGREES)
        dst = torch.repeat_interleave(torch.arange(N), deg)
        src = torch.randint(0, N, (dst.numel(),), generator=g)                      # sources repeat: a multigraph
        loops = torch.tensor([3, 15, HUB, 40, 41])
        for v in loops.tolist():                                                    # a few (v, v) columns: ordinary entries
            src[int((dst == v).nonzero()[0])] = v
        ei = torch.stack([src, dst])[:, torch.randperm(dst.numel(), generator=g)]
        _CACHE["graph"] = (ei, ref.by_target_csr(ei.numpy(), N))
    return _CACHE["graph"]


def _want(size, loops):
    """the restatement's block for every node as a target, computed once per (size, add_self_loops)"""
    key = ("want", size, loops)
    if key not in _CACHE:
        _CACHE[key] = ref.sample_hop(_graph()[1], np.arange(N), size, 0, SEED, loops)
    return _CACHE[key]


def _sampler(dev, size, **kw):
    return npi.NeighborSampler(_graph()[0].to(dev), N, size=size, **kw)


def _equal(block, want):
    n_id, res, e_id, ei = want
    assert torch.equal(block.n_id.cpu(), torch.from_numpy(n_id))
    assert torch.equal(block.e_id.cpu(), torch.from_numpy(e_id))
    assert torch.equal(block.edge_index.cpu(), torch.from_numpy(ei))
    if res is None:
        assert block.res_n_id is None
    else:
        assert torch.equal(block.res_n_id.cpu(), torch.from_numpy(res))


# ---- one hop, exact --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 5, 25, 0.5])
def test_one_hop_equals_the_restatement(dev, size):
    ei, (rowptr, _, _) = _graph()
    sampler = _sampler(dev, size)
    targets = torch.arange(N, device=dev)
    flow = sampler.sample(targets, SEED)
    assert len(flow) == 1 and flow.n_id is not None and torch.equal(flow.n_id, targets)
    block = flow[0]
    _equal(block, _want(size, False))
    assert block.res_n_id is None
    # the same properties without the restatement
    e_id, lei, n_id = block.e_id.cpu(), block.edge_index.cpu(), block.n_id.cpu()
    assert block.edge_index.dtype == block.e_id.dtype == block.n_id.dtype == torch.int64
    assert int(e_id.min()) >= 0 and int(e_id.max()) < ei.size(1)
    assert torch.equal(ei[1][e_id], lei[1])                                         # a column whose target is the block's target
    assert torch.equal(n_id[lei[0]], ei[0][e_id])
    deg = np.diff(rowptr)
    k = np.array([ref.budget(int(d), size) for d in deg]) if isinstance(size, float) else np.minimum(deg, size)
    assert np.array_equal(np.bincount(lei[1].numpy(), minlength=N), k)
    assert torch.unique(e_id).numel() == e_id.numel()                               # no edge twice (so none twice within a target)
    assert bool((n_id[1:] > n_id[:-1]).all())
    assert block.size == (n_id.numel(), N)
    assert bool((lei[1][1:] >= lei[1][:-1]).all())                                  # targets in list order
    npi.graph.check_pending()


def test_budget_above_every_degree_takes_every_in_edge(dev):
    ei, _ = _graph()
    sampler = _sampler(dev, HUB_DEG + 5)
    targets = torch.tensor([HUB, 0, 15, 2, 2999, 12, 9], device=dev)
    block = sampler.sample(targets, SEED)[0]
    e_id, lei, n_id = block.e_id.cpu(), block.edge_index.cpu(), block.n_id.cpu()
    t = targets.cpu()
    want = torch.cat([(ei[1] == v).nonzero().view(-1) for v in t.tolist()])        # in-edges of each target, list order
    assert torch.equal(e_id, want)
    assert torch.equal(n_id[lei[0]], ei[0][e_id]) and torch.equal(t[lei[1]], ei[1][e_id])
    assert torch.equal(n_id, torch.unique(ei[0][e_id]))


def test_self_loops_give_res_n_id(dev):
    sampler = _sampler(dev, 5, add_self_loops=True)
    targets = torch.arange(N, device=dev)
    block = sampler.sample(targets, SEED)[0]
    _equal(block, _want(5, True))
    assert torch.equal(block.n_id[block.res_n_id], targets)
    some = torch.tensor([0, HUB, 7, 0, 2999], device=dev)                           # node 0 has no in-edge; a repeated target
    block = sampler.sample(some, SEED)[0]
    assert torch.equal(block.n_id[block.res_n_id], some) and block.size == (block.n_id.numel(), 5)
    assert _sampler(dev, 5).sample(some, SEED)[0].res_n_id is None


# ---- independence, reproducibility -------------------------------------------------------------------------------------------------------
def test_a_nodes_sample_does_not_depend_on_its_batch(dev):
    sampler = _sampler(dev, 25)
    g = torch.Generator().manual_seed(4)
    others = torch.randperm(N, generator=g)[:999]

    def sample_of(v, batch):
        block = sampler.sample(batch.to(dev), SEED)[0]
        t = int((batch == v).nonzero()[0])
        return block.e_id[block.edge_index[1] == t].cpu()
    for v in (15, HUB, 11, 7):
        rest = others[others != v][:999]
        alone = sample_of(v, torch.tensor([v]))
        assert alone.numel() == min(DEGREES[v], 25)
        assert torch.equal(alone, sample_of(v, torch.cat([torch.tensor([v]), rest])))       # first of 1,000
        assert torch.equal(alone, sample_of(v, torch.cat([rest, torch.tensor([v])])))       # last
        assert torch.equal(alone, sample_of(v, torch.cat([rest.flip(0)[:500], torch.tensor([v]), rest[:300]])))
    big = sample_of(15, torch.tensor([15]))
    other_seed = sampler.sample(torch.tensor([15], device=dev), ref.epoch_seed(4, 0))[0].e_id.cpu()
    assert other_seed.numel() == 25 and not torch.equal(big, other_seed)            # another seed: another sample of the 1,025 row


def test_same_seed_and_epoch_give_the_same_data_flows(dev):
    def epoch(seed, epoch_no):
        s = _sampler(dev, [5, 3], num_hops=2, batch_size=700, shuffle=True, add_self_loops=True, seed=seed)
        s.epoch = epoch_no
        return list(s(None))
    a, b, c = epoch(9, 2), epoch(9, 2), epoch(9, 3)
    assert len(a) == len(b) == 5
    for fa, fb in zip(a, b):
        assert torch.equal(fa.n_id, fb.n_id) and len(fa) == len(fb) == 2
        for ba, bb in zip(fa, fb):
            assert ba.size == bb.size and torch.equal(ba.n_id, bb.n_id) and torch.equal(ba.e_id, bb.e_id)
            assert torch.equal(ba.edge_index, bb.edge_index) and torch.equal(ba.res_n_id, bb.res_n_id)
    assert not torch.equal(a[0].n_id, c[0].n_id)
    assert torch.equal(torch.cat([f.n_id for f in a]).sort().values.cpu(), torch.arange(N))
    # against the restatement, both hops (hop 0 next to the batch, produced first; flow[0] is the outermost)
    seed = ref.epoch_seed(9, 2)
    flow = a[0]
    want = ref.data_flow(_graph()[1], flow.n_id.cpu().numpy(), [5, 3], seed, True)
    _equal(flow[1], want[0])
    _equal(flow[0], want[1])
    assert flow[1].size[0] == flow[0].size[1] and flow[1].size[1] == 700


# ---- the distribution ----------------------------------------------------------------------------------------------------------------------
def _shared_row_counts(dev, n_targets, d, k, seed):
    """n_targets nodes with the same d in-neighbours each (the sources are the d nodes after them); inclusion count per position"""
    src = torch.arange(n_targets, n_targets + d).repeat(n_targets)
    dst = torch.repeat_interleave(torch.arange(n_targets), d)
    sampler = npi.NeighborSampler(torch.stack([src, dst]).to(dev), n_targets + d, size=k)
    block = sampler.sample(torch.arange(n_targets, device=dev), seed)[0]
    assert block.e_id.numel() == n_targets * k
    pos = (block.e_id % d).cpu().numpy()                                            # the list is row-major: column = v * d + p
    per_target = torch.unique(block.e_id).numel()
    assert per_target == n_targets * k                                              # k distinct positions per target
    return np.bincount(pos, minlength=d)


def test_inclusion_counts_on_the_device(dev):
    """Binomial(4096, 1/4) per position of the 64-entry row: mean 1024, sigma 27.7, all 64 within 6 sigma = 166"""
    counts = _shared_row_counts(dev, 4096, 64, 16, STAT_SEED)
    print("min / max inclusion count:", counts.min(), counts.max())
    assert (np.abs(counts - 1024) <= 166).all(), counts
    assert np.array_equal(counts, ref.inclusion_counts(STAT_SEED, 0, 4096, 64, 16)[0])


def test_inclusion_counts_on_the_hub_path(dev):
    """Binomial(256, 1/4) per position of the 4,096-entry row, k = 1024: mean 64, sigma 6.9, all 4,096 within 7 sigma = 49"""
    counts = _shared_row_counts(dev, 256, 4096, 1024, HUB_STAT_SEED)
    print("min / max inclusion count:", counts.min(), counts.max())
    assert (np.abs(counts - 64) <= 49).all()
    assert np.array_equal(counts, ref.inclusion_counts(HUB_STAT_SEED, 0, 256, 4096, 1024)[0])


# ---- through the layers --------------------------------------------------------------------------------------------------------------------
def _check(got, want, names, bars):
    for g_, w_, name, bar in zip(got, want, names, bars):
        err = _row_scaled(g_, w_) if bar == "row" else rel_max(g_, w_)
        print(f"   {name}: {err:.2e}")
        assert err < (1e-4 if bar == "row" else GRAD_REL), (name, err)


def _flow_for_layers(dev):
    sampler = _sampler(dev, [5, 3], num_hops=2, add_self_loops=True)
    g = torch.Generator().manual_seed(6)
    targets = torch.cat([torch.tensor([0, HUB, 15]), torch.randperm(N, generator=g)[:297]])
    return sampler.sample(targets.to(dev), SEED)


def test_two_hops_through_sage_layers(dev):
    flow = _flow_for_layers(dev)
    outer, inner = flow[0], flow[1]
    assert inner.size[1] == 300 and outer.size[1] == inner.size[0]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(outer.size[0], 32, generator=g).double()
    W1 = (torch.randn(64, 16, generator=g) / 8).double()
    b1 = torch.randn(16, generator=g).double()
    W2 = (torch.randn(16, 8, generator=g) / 4).double()
    b2 = torch.randn(8, generator=g).double()
    go = torch.randn(300, 8, generator=g).double()
    xr, W1r, b1r, W2r, b2r = (t.clone().requires_grad_(True) for t in (x, W1, b1, W2, b2))
    h = bref.sage_bipartite(xr, outer.edge_index.cpu(), W1r, b1r, n_dst=outer.size[1], res_n_id=outer.res_n_id.cpu(), concat=True)
    want = bref.sage_bipartite(h, inner.edge_index.cpu(), W2r, b2r, n_dst=inner.size[1])
    want.backward(go)
    conv1, conv2 = npi.SAGEConv(32, 16, concat=True).to(dev), npi.SAGEConv(16, 8).to(dev)
    with torch.no_grad():
        conv1.weight.copy_(W1)
        conv1.bias.copy_(b1)
        conv2.weight.copy_(W2)
        conv2.bias.copy_(b2)
    xg = x.float().to(dev).requires_grad_(True)
    h_g = conv1((xg, None), outer.graph(), size=outer.size, res_n_id=outer.res_n_id)
    out = conv2((h_g, None), inner.graph(), size=inner.size)
    assert outer.graph() is outer.graph() and tuple(out.shape) == (300, 8)
    out.backward(go.float().to(dev))
    _check([out, xg.grad, conv1.weight.grad, conv1.bias.grad, conv2.weight.grad, conv2.bias.grad],
           [want, xr.grad, W1r.grad, b1r.grad, W2r.grad, b2r.grad], ["out", "dX", "dW1", "db1", "dW2", "db2"],
           ["row", "row", "rel", "rel", "rel", "rel"])
    npi.graph.check_pending()


def test_a_block_through_gat_with_x_dst_from_res_n_id(dev):
    block = _flow_for_layers(dev)[1]
    heads, C, Fin = 2, 8, 32
    g = torch.Generator().manual_seed(8)
    x = torch.randn(block.size[0], Fin, generator=g).double()
    W = (torch.randn(Fin, heads * C, generator=g) / Fin ** 0.5).double()
    att = (torch.randn(1, heads, 2 * C, generator=g) / C ** 0.5).double()
    b = torch.randn(heads * C, generator=g).double()
    go = torch.randn(block.size[1], heads * C, generator=g).double()
    xr, Wr, ar, br = (t.clone().requires_grad_(True) for t in (x, W, att, b))
    want = bref.gat_bipartite(xr, xr[block.res_n_id.cpu()], block.edge_index.cpu(), Wr, ar, br, n_dst=block.size[1], heads=heads)
    want.backward(go)
    conv = npi.GATConv(Fin, C, heads=heads).to(dev)
    with torch.no_grad():
        conv.weight.copy_(W)
        conv.att.copy_(att)
        conv.bias.copy_(b)
    xg = x.float().to(dev).requires_grad_(True)
    out = conv((xg, xg[block.res_n_id]), block.graph(), size=block.size)
    out.backward(go.float().to(dev))
    _check([out, xg.grad, conv.weight.grad, conv.att.grad, conv.bias.grad], [want, xr.grad, Wr.grad, ar.grad, br.grad],
           ["out", "dX", "dW", "d att", "db"], ["row", "row", "rel", "rel", "rel"])


# ---- housekeeping ----------------------------------------------------------------------------------------------------------------------------
def test_scratch_is_zero_after_twenty_batches(dev):
    sampler = _sampler(dev, [25, 10], num_hops=2, batch_size=150, shuffle=True, add_self_loops=True)
    flows = list(sampler(None))
    assert len(flows) == 20
    assert sampler._scratch.numel() == N and int(sampler._scratch.abs().max()) == 0
    assert sampler.epoch == 1


def test_mask_and_id_list_subsets_are_the_same_epoch(dev):
    mask = torch.zeros(N, dtype=torch.bool)
    mask[::7] = True
    mask[HUB] = True
    ids = mask.nonzero().view(-1)
    flows = []
    for subset in (mask.to(dev), ids.to(dev), ids):
        s = _sampler(dev, [5, 3], num_hops=2, batch_size=128, shuffle=True, drop_last=True, seed=2)
        flows.append(list(s(subset)))
    assert len(flows[0]) == ids.numel() // 128
    for other in flows[1:]:
        assert len(other) == len(flows[0])
        for fa, fb in zip(flows[0], other):
            assert torch.equal(fa.n_id, fb.n_id)
            for ba, bb in zip(fa, fb):
                assert torch.equal(ba.n_id, bb.n_id) and torch.equal(ba.e_id, bb.e_id) and torch.equal(ba.edge_index, bb.edge_index)
                assert ba.res_n_id is None and bb.res_n_id is None


def test_out_of_range_targets_are_dropped_and_reported(dev):
    sampler = _sampler(dev, 5, add_self_loops=True)
    npi.graph.check_pending()
    with pytest.raises(IndexError):
        sampler.sample(torch.tensor([3, N + 4, -1, 15], device=dev), SEED)
    assert int(sampler._scratch.abs().max()) == 0                                   # the scratch is clean after the error too
    block = sampler.sample(torch.tensor([3, 15], device=dev), SEED)[0]               # and the sampler still works
    assert block.edge_index.size(1) == 4 + 5
    npi.graph.check_pending()


def test_sampling_inside_a_capture_raises(dev):
    sampler = _sampler(dev, 5)
    targets = torch.arange(10, device=dev)
    sampler.sample(targets, SEED)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        with pytest.raises(npi.NpiError, match="capture"):
            sampler.sample(targets, SEED)
    torch.cuda.synchronize()
