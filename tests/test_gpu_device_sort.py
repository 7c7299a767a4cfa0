"""The shared device sort and scans (csrc/sort.h) through their public callers, at the smallest sizes where each piece takes
another path.  Every comparison is integer-exact against a torch restatement on the host.

  PairSort (radix sort, both launch regimes)   CSRGraph, plain and with sorted columns; TopKPooling's large-graph selection (and
                                               npi_topk_select_sorted itself, for the scores the layer never produces)
  exclusive_scan_i32                           inside the sort above 64 tiles; NeighborSampler.sample_subgraph's coalesce
  block_exclusive_scan<1024, long long>        InteractionGraph.batch (subgraph_scan_kernel), NeighborSampler (relabel_scan_kernel)
  block_exclusive_scan<256, int>               every sort pass up to 64 tiles; topk_kept_offsets_kernel; scan_small_kernel

scan_small_kernel (npi_filter_adj above 2,048 tiles) is run at 2,051 tiles -- just above the switch -- by
test_gpu_pool.py::test_filter_adj_keeps_the_edge_order_on_both_tile_paths[4199304] and is not repeated here.
"""
import math

import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import pool as NP
from npi_gnn_amd.sampler import NeighborSampler
from npi_gnn_amd.subgraph import InteractionGraph

pytestmark = pytest.mark.gpu

SORT_TILE = 4096            # pairs per workgroup of the radix sort
SMALL_SORT_TILES = 64       # up to here every workgroup derives its own offsets; above, the histograms are scanned


# ---- CSR build ------------------------------------------------------------------------------------------------------------------------
def _edge_list(E, N, seed):
    """E columns: random pairs with repeated columns and self loops, the last E // 8 of them (-1, -1) padding"""
    g = torch.Generator().manual_seed(seed)
    pad = E // 8
    body = E - pad
    ei = torch.randint(0, N, (2, body), generator=g)
    q = body // 4
    ei[:, :q] = ei[:, q:2 * q]                                # every column of the second quarter a second time
    ei[0, 3::7] = ei[1, 3::7]                                 # self loops
    return torch.cat([ei, torch.full((2, pad), -1, dtype=torch.int64)], dim=1)


def _csr_reference(ei, N, sort_columns):
    """by-target CSR with the self loop last in every row: the padding and the (i, i) columns dropped, the rest in a stable order"""
    key, val = ei[1], ei[0]
    idx = ((key != val) & (key >= 0)).nonzero().flatten()
    k, v = key[idx], val[idx]
    if sort_columns:                                          # by (row, column), equal pairs in list order
        o = torch.sort(v, stable=True).indices
        o = o[torch.sort(k[o], stable=True).indices]
    else:
        o = torch.sort(k, stable=True).indices
    k, v, e = k[o], v[o], idx[o]
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(k, minlength=N) + 1, 0)
    nnz = int(rowptr[-1])
    col = torch.empty(nnz, dtype=torch.int64)
    eid = torch.full((nnz,), -1, dtype=torch.int64)
    at = torch.arange(k.numel()) + k                          # k loops lie in front of an entry of row k
    col[at], eid[at] = v, e
    col[rowptr[1:] - 1] = torch.arange(N)
    return rowptr.int(), col.int(), eid.int()


# one tile, the tile boundary, both sides of the switch between the two launch regimes; 1, 2 and 3 radix passes
@pytest.mark.parametrize("N", [3, 300, 70_000])
@pytest.mark.parametrize("E", [1, 255, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, SMALL_SORT_TILES * SORT_TILE,
                               SMALL_SORT_TILES * SORT_TILE + 1])
def test_csr_build_equals_a_stable_sort(dev, E, N):
    ei = _edge_list(E, N, seed=E + N)
    for sort_columns in (False, True):
        side = npi.CSRGraph(ei.to(dev), N, sort_columns=sort_columns).by_dst
        rowptr, col, eid = _csr_reference(ei, N, sort_columns)
        nnz = int(rowptr[-1])
        assert torch.equal(side.rowptr.cpu(), rowptr)
        assert torch.equal(side.col[:nnz].cpu(), col)
        assert torch.equal(side.eid[:nnz].cpu(), eid)
        assert int(side.status.item()) == 0                   # padding is not an out-of-range id


# ---- TopKPooling's radix selection ----------------------------------------------------------------------------------------------------
def _topk_reference(x, sizes, ratio, ei):
    """per graph: the ceil(ratio n) highest scores, descending, equal scores by index; filter_adj over the kept nodes"""
    score = torch.tanh(x[:, 0])                               # w = [1]: score = tanh(x . w / |w|)
    perm, a = [], 0
    for n in sizes:
        order = torch.sort(score[a:a + n], descending=True, stable=True).indices
        perm.append(order[:math.ceil(ratio * n)] + a)
        a += n
    perm = torch.cat(perm)
    remap = torch.full((x.size(0),), -1, dtype=torch.int64)
    remap[perm] = torch.arange(perm.numel())
    s, d = remap[ei[0]], remap[ei[1]]
    keep = (s >= 0) & (d >= 0)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return perm, batch[perm], torch.stack([s[keep], d[keep]])


def _topk_check(dev, x, sizes, ratio):
    g = torch.Generator().manual_seed(len(sizes))
    n = sum(sizes)
    ei = torch.randint(0, n, (2, 2000), generator=g)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    w = torch.ones(1, 1)
    perm, bo, eo = _topk_reference(x, sizes, ratio, ei)
    # the tensor form knows no graph sizes: the LDS selection reports the graph it cannot hold and the radix selection
    # (npi_topk_select_sorted) runs in its place
    got = NP.topk_pool(x.to(dev), ei.to(dev), batch.to(dev), w.to(dev), ratio)
    assert torch.equal(got[4].cpu(), perm)
    assert torch.equal(got[3].cpu(), bo)
    assert torch.equal(got[1].cpu(), eo)


def _grid_scores(n, seed):
    """a 65-value grid (many ties; neighbours 1/16 apart, far more than a rounding of tanh)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-32, 33, (n, 1), generator=g).float() / 16)


BIG_AND_SMALL = [SMALL_SORT_TILES * SORT_TILE + 1, 5]        # 65 tiles: the scanned regime; 32-bit keys: 4 passes


def _special_values(n, seed):
    """the grid with -0.0 / 0.0, +-inf and one NaN in the large graph, and a small graph that the zeros' order decides"""
    v = _grid_scores(n, seed)
    v[10:14, 0] = torch.tensor([-0.0, 0.0, float("inf"), float("-inf")])
    v[5000, 0] = float("inf")                                 # a tie with v[12]
    v[70_000, 0] = float("nan")                               # sorts first, as in torch.sort
    v[n - 5:, 0] = torch.tensor([0.5, -0.0, 0.5, 0.0, float("-inf")])
    return v


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_radix_selection_equals_a_stable_descending_sort(dev, ratio):
    """Through TopKPooling.  The special values are FEATURES here, and npi_topk_score stands between them and the selection:
    score = tanh(fma(x, w, +0) / |w|) turns -0.0 into +0.0 and +-inf into +-1, so what reaches npi_topk_select_sorted on this
    path is the ties (thousands per grid value, the two zeros, the two +1), the NaN and the saturated +-1 -- never a -0.0 or an
    infinite score.  Those two are given to the entry point itself by the test below."""
    sizes = BIG_AND_SMALL
    assert NP.LDS_SORT_MAX_NODES < sizes[0]
    _topk_check(dev, _special_values(sum(sizes), seed=3), sizes, ratio)


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_radix_selection_on_raw_scores(dev, ratio):
    """npi_topk_select_sorted itself (called as pool.py's select_sorted calls it) on scores that hold -0.0 / 0.0, +-inf, ties
    and one NaN.  The reference is torch.sort(descending=True, stable=True) per graph with ONE order made explicit: the kernel
    sorts the scores' bit patterns, which puts 0.0 strictly ahead of -0.0, where torch.sort calls them equal and lets the index
    decide (the 5-node graph [0.5, -0.0, 0.5, 0.0, -inf] keeps nodes 0, 2, 3 at ratio 0.5; index order would keep 0, 2, 1).
    A score from npi_topk_score is never -0.0 (above), so the layer cannot show the difference."""
    from npi_gnn_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    sizes = BIG_AND_SMALL
    n, B = sum(sizes), len(sizes)
    score = _special_values(n, seed=4)[:, 0].contiguous()
    key = score.double()
    key[(score == 0) & torch.signbit(score)] = -1e-300       # -0.0 behind 0.0, ahead of every negative score
    perm, a = [], 0
    for m in sizes:
        order = torch.sort(key[a:a + m], descending=True, stable=True).indices
        perm.append(order[:math.ceil(ratio * m)] + a)
        a += m
    kept = torch.tensor([0] + [p.numel() for p in perm]).cumsum(0)
    perm = torch.cat(perm)
    remap = torch.full((n,), -1, dtype=torch.int64)
    remap[perm] = torch.arange(perm.numel())
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(dev)
    gp = NP.graph_ptr(batch, B)
    i32 = dict(dtype=torch.int32, device=dev)
    out_ptr, got_perm, got_remap = torch.empty(B + 1, **i32), torch.empty(n, **i32), torch.empty(n, **i32)
    n_ws = int(lib.npi_topk_sorted_workspace_bytes(n))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    sd = score.to(dev)
    check(lib.npi_topk_select_sorted(ptr(sd), ptr(batch), ptr(gp), n, B, float(ratio), ptr(out_ptr), ptr(got_perm), ptr(got_remap),
                                     ptr(ws), n_ws, stream_ptr(dev)), "npi_topk_select_sorted")
    assert torch.equal(out_ptr.cpu().long(), kept)
    assert torch.equal(got_perm[: perm.numel()].cpu().long(), perm)
    assert torch.equal(got_remap.cpu().long(), remap)


@pytest.mark.parametrize("B", [1, 256, 257])                 # topk_kept_offsets_kernel: one block of graphs, a full one, one more
def test_kept_offsets_across_the_scan_block(dev, B):
    sizes = [NP.LDS_SORT_MAX_NODES + 1] + [1 + i % 5 for i in range(B - 1)]
    _topk_check(dev, _grid_scores(sum(sizes), seed=B), sizes, 0.5)


# ---- the 1024-thread scans ------------------------------------------------------------------------------------------------------------
SCAN_COUNTS = [1, 1023, 1024, 1025, 2049]                    # one entry per thread or fewer, one more, two per thread + 1


@pytest.fixture(scope="module")
def interactions(dev):
    """40 RNAs x 30 proteins, a fifth of the pairs present, a fifth of those not usable"""
    g = torch.Generator().manual_seed(11)
    R, P = 40, 30
    present = torch.rand(R, P, generator=g) < 0.2
    pairs = present.nonzero() + torch.tensor([0, R])
    usable = torch.rand(pairs.size(0), generator=g) < 0.8
    U = torch.zeros(R, P, dtype=torch.int64)
    U[pairs[:, 0], pairs[:, 1] - R] = usable.long()
    ig = InteractionGraph(pairs.to(dev), usable.to(dev), torch.zeros(R + P, 1, device=dev))
    return ig, U, R, P


@pytest.mark.parametrize("B", SCAN_COUNTS)
def test_subgraph_offsets_across_the_scan_block(dev, interactions, B):
    """subgraph_scan_kernel: sample g starts at row sum_{h<g} nodes_h and at pair sum_{h<g} pairs_h"""
    ig, U, R, P = interactions
    g = torch.Generator().manual_seed(B)
    l, p = torch.randint(0, R, (B,), generator=g), torch.randint(0, P, (B,), generator=g)
    partners = U[l].sum(1) + U[:, p].sum(0) - 2 * U[l, p]    # usable partners of l other than p, and of p other than l
    nodes, pairs = 2 + partners, 1 + partners
    gb, node_id = ig.batch(torch.stack([l, p + R], dim=1), return_node_id=True)
    which = torch.repeat_interleave(torch.arange(B), nodes)
    bvec = gb.batch_vector().cpu()
    assert torch.equal(bvec, which)
    start = torch.cumsum(nodes, 0) - nodes
    assert torch.equal(node_id.cpu()[start].long(), l) and torch.equal(node_id.cpu()[start + 1].long(), p + R)
    assert torch.equal(bvec[gb.edge_index[0].cpu()], torch.repeat_interleave(torch.arange(B), 2 * pairs))


@pytest.mark.parametrize("chunks", SCAN_COUNTS)
def test_relabelling_across_the_scan_block(dev, chunks):
    """relabel_scan_kernel scans one count per 1,024 node ids: a hop that takes every in-edge, and the subgraph of the same
    entries (npi_sample_union scans again; npi_sample_coalesce sorts and scans the pairs)"""
    N = 700 if chunks == 1 else (chunks - 1) * 1024 + 7
    T, E = 16, 6000
    g = torch.Generator().manual_seed(chunks)
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, T, (E,), generator=g)
    src[:2] = torch.tensor([0, N - 1])
    src[-100:], dst[-100:] = src[:100], dst[:100]             # parallel edges
    sampler = NeighborSampler(torch.stack([src, dst]).to(dev), N, size=E)
    targets = torch.arange(T)
    order = torch.sort(dst, stable=True).indices              # a block's entries: target by target, in list order
    n_id = torch.unique(src)
    blk = sampler.sample(targets.to(dev), seed=5)[0]
    assert torch.equal(blk.n_id.cpu(), n_id)
    assert torch.equal(blk.e_id.cpu(), order)
    assert torch.equal(blk.edge_index.cpu(), torch.stack([torch.searchsorted(n_id, src[order]), dst[order]]))
    # the one-id-space flow over the same entries: ascending union of both ends, equal pairs merged under their smallest edge id
    sub = sampler.sample_subgraph(targets.to(dev), seed=5)
    ids = torch.unique(torch.cat([src, targets]))
    U = ids.numel()
    code, inv = torch.unique(torch.searchsorted(ids, src) * U + torch.searchsorted(ids, dst), return_inverse=True)
    e_id = torch.full((code.numel(),), E, dtype=torch.int64).scatter_reduce(0, inv, torch.arange(E), "amin")
    assert torch.equal(sub.n_id.cpu(), ids)
    assert torch.equal(sub.edge_index.cpu(), torch.stack([code // U, code % U]))
    assert torch.equal(sub.e_id.cpu(), e_id)
    assert torch.equal(sub.sub_b_id.cpu(), torch.searchsorted(ids, targets))
