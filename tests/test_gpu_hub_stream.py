"""The streaming path for the heaviest rows of a side (``CSRSide.hub_plan`` / ``npi_segsum_hub``, ``CSRGraph.hub_stream``).

  * plan construction against numpy on a small graph: hub choice, mask bits, the light side's rowptr and col
  * SAGEConv forward, dX, dW, db through the hub path against the plain path (``graph.hub_stream = False``) and against fp64 torch ops, at the bars
    of the existing suite: 1e-4 per row scale for out and dX, 1e-5 against fp64 on the heaviest rows (tests/test_gpu_fullsize.py),
    GRAD_REL = 1e-5 for dW and db (tests/_util.py) -- on the C4 graph, a mid-size Zipf graph, a graph with fewer qualifying rows
    than NPI_HUB_MAX, one with a duplicate pair on a heavy row and one whose heaviest row has an explicit self loop
  * a graph with uniform sources has no plan, and its result is bit-identical to the plain path
  * two launches are bitwise equal; the hub rows' power-of-two scales equal those of a pass over the finished rows; a captured
    replay equals the eager launch
"""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import functional as NF
from npi_gnn_amd import graph as G
from npi_gnn_amd._lib import NPI_HUB_MAX
from npi_gnn_amd.synth import bipartite_edge_index, bipartite_edge_index_device
from _util import GRAD_REL

pytestmark = pytest.mark.gpu

F = 256


# ---- plan construction ------------------------------------------------------------------------------------------------------------
def _small_edges(n=3000, heavy=((5, 900), (17, 700), (2999, 700), (40, 300), (41, 120)), seed=0):
    """random light edges plus rows of chosen in-degree (distinct sources per heavy row); directed, no duplicates"""
    rng = np.random.default_rng(seed)
    pairs = {(int(s), int(d)) for s, d in zip(rng.integers(0, n, 6000), rng.integers(100, 2900, 6000)) if s != d}
    for row, deg in heavy:
        for s in rng.permutation(n)[:deg]:
            if int(s) != row:
                pairs.add((int(s), row))
    e = np.array(sorted(pairs), dtype=np.int64)
    return torch.from_numpy(e[rng.permutation(len(e))].T.copy())


def test_plan_against_numpy(dev):
    n = 3000
    ei = _small_edges(n)
    graph = npi.CSRGraph(ei.to(dev), n)
    side = graph.by_dst
    rowptr, col = side.rowptr.cpu().numpy().astype(np.int64), side.col.cpu().numpy().astype(np.int64)
    deg = rowptr[1:] - rowptr[:-1]
    for h_max, min_degree in ((NPI_HUB_MAX, 200), (2, 200), (NPI_HUB_MAX, 100)):
        plan = G.build_hub_plan(side, h_max=h_max, min_degree=min_degree, min_entries=1)
        cand = np.flatnonzero(deg >= min_degree)
        want = cand[np.lexsort((cand, -deg[cand]))][:h_max]                    # by degree, ties: the lower row
        assert plan is not None and plan.H == len(want)
        hub_rows = plan.hub_rows.cpu().numpy()
        assert np.array_equal(hub_rows[: plan.H], want) and (hub_rows[plan.H:] == -1).all()
        assert plan.n_entries == int(deg[want].sum())
        mask = np.zeros((n, NPI_HUB_MAX // 32), dtype=np.uint32)
        for j, r in enumerate(want):
            mask[col[rowptr[r]:rowptr[r + 1]], j // 32] |= np.uint32(1 << (j % 32))
        assert np.array_equal(plan.mask.cpu().numpy().view(np.uint32), mask)
        keep = np.ones(rowptr[-1], dtype=bool)
        for r in want:
            keep[rowptr[r]:rowptr[r + 1]] = False
        ldeg = deg.copy()
        ldeg[want] = 0
        light = plan.light
        assert np.array_equal(light.rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(ldeg)]))
        nnz_l = int(ldeg.sum())
        assert light.nnz_max == side.nnz_max - plan.n_entries and light.nnz_max >= nnz_l
        assert np.array_equal(light.col.cpu().numpy()[:nnz_l], col[: rowptr[-1]][keep])
        assert np.array_equal(light.eid.cpu().numpy()[:nnz_l], side.eid.cpu().numpy()[: rowptr[-1]][keep])
        lrow = np.repeat(np.arange(n), ldeg)
        assert np.array_equal(light.rowidx.cpu().numpy()[:nnz_l], lrow)
        starts = np.arange(0, nnz_l, light.item)
        assert np.array_equal(light.item_row.cpu().numpy()[: len(starts)][1:], lrow[starts][1:])
    # thresholds: too few hub entries for the rows that would be streamed -> no plan
    assert G.build_hub_plan(side, min_degree=200, min_entries=int(deg[deg >= 200].sum()) + 1) is None
    assert G.build_hub_plan(side, min_degree=200, min_entries=int(deg[deg >= 200].sum())) is not None
    assert G.build_hub_plan(side, min_degree=5000, min_entries=1) is None


def test_plan_drops_a_row_with_a_duplicate_pair(dev):
    n = 3000
    ei = _small_edges(n)
    src17 = int(ei[0][ei[1] == 17][0])
    ei = torch.cat([ei, torch.tensor([[src17], [17]])], 1)                     # the pair (src17 -> 17) a second time
    side = npi.CSRGraph(ei.to(dev), n).by_dst
    plan = G.build_hub_plan(side, min_degree=200, min_entries=1)
    rows = plan.hub_rows.cpu().tolist()[: plan.H]
    assert rows == [5, 2999, 40]                                               # 17 (701 entries) is out, the others move up
    rowptr, col = side.rowptr.cpu().numpy(), side.col.cpu().numpy()
    mask = np.zeros((n, NPI_HUB_MAX // 32), dtype=np.uint32)
    for j, r in enumerate(rows):
        mask[col[rowptr[r]:rowptr[r + 1]], 0] |= np.uint32(1 << j)
    assert np.array_equal(plan.mask.cpu().numpy().view(np.uint32), mask)


# ---- the layer through both paths -------------------------------------------------------------------------------------------------
def _heavy_extra(ei, n, rows, deg, seed):
    g = torch.Generator().manual_seed(seed)
    extra = [torch.stack([torch.randperm(n, generator=g)[:deg], torch.full((deg,), r)]) for r in rows]
    extra = extra + [e.flip(0) for e in extra]                                 # both directions: heavy rows on both sides
    return torch.cat([ei] + extra, 1)


def _graphs(name, dev):
    """(edge_index on the device, N, expected number of hubs by target, by source)"""
    if name == "c4":
        return bipartite_edge_index(1_000_000, 20_000_000, seed=20260310).to(dev), 1_000_000, NPI_HUB_MAX, NPI_HUB_MAX
    n = 300_000
    if name == "zipf":
        return bipartite_edge_index_device(n, 6_000_000, dev, seed=3), n, NPI_HUB_MAX, NPI_HUB_MAX
    g = torch.Generator().manual_seed(1)
    ei = torch.randint(0, n, (2, 1_500_000), generator=g)
    ei = ei[:, ei[0] != ei[1]]
    heavy = [7, 150_000, 299_999, 12_345, 200_001]                             # five rows of 160k in- and out-edges: fewer than NPI_HUB_MAX
    if name == "few":
        ei = _heavy_extra(ei, n, heavy, 160_000, 2)
        ei = torch.unique(ei[:, ei[0] != ei[1]], dim=1)
        return ei.to(dev), n, 5, 5
    if name == "duplicate":
        ei = _heavy_extra(ei, n, heavy, 160_000, 2)
        ei = torch.unique(ei[:, ei[0] != ei[1]], dim=1)
        first = int(torch.nonzero(ei[1] == 150_000)[0])
        ei = torch.cat([ei, ei[:, first:first + 1]], 1)                        # one pair of row 150000 twice: that row is no hub
        return ei.to(dev), n, 4, 5
    if name == "self_loop":
        ei = _heavy_extra(ei, n, heavy, 160_000, 2)
        ei = torch.unique(ei[:, ei[0] != ei[1]], dim=1)
        ei = torch.cat([ei, torch.tensor([[7, 12_345], [7, 12_345]])], 1)      # explicit (i, i) columns on two hub rows
        return ei.to(dev), n, 5, 5
    raise KeyError(name)


def _row_scaled(got, ref):
    return float(((got - ref).abs() / (1.0 + ref.abs().amax(1, keepdim=True))).max())


@pytest.mark.parametrize("name", ["zipf", "few", "duplicate", "self_loop", "c4"])
def test_layer_hub_path_against_plain_path_and_fp64(dev, name):
    ei, n, want_d, want_s = _graphs(name, dev)
    graph = npi.CSRGraph(ei, n)
    for side, want_h in ((graph.by_dst, want_d), (graph.by_src, want_s)):
        plan = side.hub_plan()
        assert plan is not None and plan.H == want_h, (name, plan and plan.H)
    if name == "duplicate":
        assert 150_000 not in graph.by_dst.hub_plan().hub_rows.cpu().tolist()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, F, generator=g).to(dev)
    W = (torch.randn(F, F, generator=g) / 16).to(dev)
    b = torch.randn(F, generator=g).to(dev)
    go = torch.randn(n, F, generator=g).to(dev)
    res = {}
    for key, on in (("hub", True), ("plain", False)):
        graph.hub_stream = on                                                  # the same graph through both paths
        xg, Wg, bg = (t.clone().requires_grad_(True) for t in (x, W, b))
        out = npi.sage_conv(xg, graph, Wg, bg)
        out.backward(go)
        res[key] = (out.detach(), xg.grad, Wg.grad, bg.grad)
    out, dx, dw, db = res["hub"]
    # against the plain path: out and dX per row scale, the parameter gradients relative
    e_out, e_dx = _row_scaled(out, res["plain"][0]), _row_scaled(dx, res["plain"][1])
    e_dw = float((dw - res["plain"][2]).abs().max() / res["plain"][2].abs().max())
    e_db = float((db - res["plain"][3]).abs().max() / res["plain"][3].abs().max())
    print(f"{name}: hub vs plain  out {e_out:.2e}  dX {e_dx:.2e}  dW {e_dw:.2e}  db {e_db:.2e}")
    assert e_out < 1e-4 and e_dx < 1e-4 and e_dw < GRAD_REL and e_db < GRAD_REL
    # against fp64: dW = agg^T dOut with agg from fp64 segment sums, db; the heaviest rows of out and dX by their formulas
    side, tside = graph.by_dst, graph.by_src
    cnt = (side.rowptr[1:] - side.rowptr[:-1]).double()
    Wd = W.double()
    dagg = go.double() @ Wd.t()
    worst_out = worst_dx = 0.0
    hubs_d = side.hub_plan().hub_rows[: min(want_d, 8)].tolist()
    hubs_s = tside.hub_plan().hub_rows[: min(want_s, 8)].tolist()
    for i in hubs_d:
        nb = side.col[int(side.rowptr[i]):int(side.rowptr[i + 1])].long()
        truth = (x[nb].double().sum(0) / cnt[i]) @ Wd + b.double()
        worst_out = max(worst_out, float((out[i].double() - truth).abs().max() / truth.abs().max()))
    for j in hubs_s:
        nb = tside.col[int(tside.rowptr[j]):int(tside.rowptr[j + 1])].long()
        truth = (dagg[nb] / cnt[nb, None]).sum(0)
        worst_dx = max(worst_dx, float((dx[j].double() - truth).abs().max() / truth.abs().max()))
    del dagg
    agg64 = torch.zeros(n, F, dtype=torch.float64, device=dev)
    nnz = int(side.rowptr[-1])
    CH = 4_000_000
    for p0 in range(0, nnz, CH):
        sl = slice(p0, min(p0 + CH, nnz))
        agg64.index_add_(0, side.rowidx[sl].long(), x[side.col[sl].long()].double())
    agg64 /= cnt[:, None]
    dw64 = agg64.t() @ go.double()
    e_dw64 = float((dw.double() - dw64).abs().max() / dw64.abs().max())
    e_db64 = float((db.double() - go.double().sum(0)).abs().max() / go.double().sum(0).abs().max())
    out64 = agg64 @ Wd + b.double()
    e_out64 = _row_scaled(out.double(), out64)
    print(f"{name}: hub vs fp64   heaviest rows out {worst_out:.2e} dX {worst_dx:.2e}  all rows out {e_out64:.2e}  dW {e_dw64:.2e}  db {e_db64:.2e}")
    assert worst_out < 1e-5 and worst_dx < 1e-5
    assert e_out64 < 1e-4 and e_dw64 < GRAD_REL and e_db64 < GRAD_REL


def test_uniform_sources_have_no_plan_and_the_same_bits(dev):
    n = 300_000
    g = torch.Generator().manual_seed(5)
    ei = torch.randint(0, n, (2, 3_000_000), generator=g).to(dev)
    graph = npi.CSRGraph(ei, n)
    assert graph.by_dst.hub_plan() is None and graph.by_src.hub_plan() is None
    x = torch.randn(n, F, generator=g).to(dev)
    W = (torch.randn(F, F, generator=g) / 16).to(dev)
    go = torch.randn(n, F, generator=g).to(dev)
    res = []
    for on in (True, False):
        graph.hub_stream = on
        xg, Wg = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
        out = npi.sage_conv(xg, graph, Wg, None)
        out.backward(go)
        res.append((out.detach(), xg.grad, Wg.grad))
    for a, c in zip(*res):
        assert torch.equal(a, c)
    # small graphs never ask: no device work, no plan
    small = npi.CSRGraph(_small_edges().to(dev), 3000)
    assert small.by_dst.hub_plan() is None and small.by_dst._hub_asked


def test_reproducible_scales_and_captured_replay(dev):
    ei, n, _, _ = _graphs("zipf", dev)
    graph = npi.CSRGraph(ei, n)
    side = graph.by_dst
    plan = side.hub_plan()
    assert plan is not None
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, F, generator=g).to(dev)
    cs = (torch.rand(n, generator=g) + 0.5).to(dev)
    rows = plan.hub_rows[: plan.H].long()
    for mean, col_scale in ((True, None), (False, cs)):
        w_light = None if col_scale is None else cs[plan.light.col.long().clamp_(0, n - 1)]
        outs, scales = [], []
        for _ in range(2):
            o, s = torch.empty(n, F, device=dev), torch.empty(n, device=dev)
            NF.segsum(graph, side, x, w=w_light, mean=mean, out=o, scales_out=s, hub=plan, col_scale=col_scale)
            outs.append(o)
            scales.append(s)
        assert torch.equal(outs[0], outs[1]) and torch.equal(scales[0], scales[1])          # launch to launch: the same bits
        # the scale of every hub row is the one the plain launch writes for the same row values (a pass over them: npi_row_scales)
        assert torch.equal(scales[0][rows], NF.row_scales(outs[0][rows].contiguous()))
        assert torch.equal(scales[0], NF.row_scales(outs[0]))
        w_full = None if col_scale is None else cs[side.col.long().clamp_(0, n - 1)]
        ref = NF.segsum(graph, side, x, w=w_full, mean=mean)
        assert _row_scaled(outs[0], ref) < 1e-5
    # a captured replay equals the eager launch
    o_cap, s_cap = torch.empty(n, F, device=dev), torch.empty(n, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        NF.segsum(graph, side, x, mean=True, out=o_cap, scales_out=s_cap, hub=plan)         # warm-up on the capture stream
    torch.cuda.current_stream(dev).wait_stream(stream)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        NF.segsum(graph, side, x, mean=True, out=o_cap, scales_out=s_cap, hub=plan)
    o_eager = torch.empty(n, F, device=dev)
    NF.segsum(graph, side, x, mean=True, out=o_eager, hub=plan)
    for _ in range(2):
        o_cap.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_cap, o_eager)
