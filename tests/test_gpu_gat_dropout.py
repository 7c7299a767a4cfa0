"""Seeded attention dropout (Rule D) inside GATConv's fused kernels: the mask on the device against the numpy rule bit for bit, the
square form against the fp64 oracle under that mask (served shapes: the fused kernels; unserved ones: the composed variant under the
same mask), rows that stress the aggregation (a row of > 4096 entries, cut rows, empty rows, rows that lose every entry), the
bipartite form against its fp64 restatement, determinism and the module's ``seed=`` / ``.draw``.  Tolerances are the layer's own bars
(``tests/test_gpu_gat.py``): forward 1e-4 / 1e-4, dX 2e-4 / 1e-3, parameters ``GRAD_REL``."""
import numpy as np
import pytest
import torch

import _gat_dropout_ref as D
import npi_gnn_amd as npi
from _util import GRAD_REL, rel_max
from npi_gnn_amd import functional as NF
from npi_gnn_amd.schedule import DEFAULT
from oracle import ref_conv as R

pytestmark = pytest.mark.gpu


def _case(N, E, Fi, H, C, seed, hub=True):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    if hub:
        ei[1, : E // 3] = 3                    # one target with ~E/3 entries: a row cut over many items / workgroups
        ei[0, E // 3: E // 2] = 5              # one heavy source row for the backward
    x = torch.randn(N, Fi, generator=g)
    W = (torch.rand(Fi, H * C, generator=g) * 2 - 1) * (6.0 / (Fi + H * C)) ** 0.5
    att = (torch.rand(1, H, 2 * C, generator=g) * 2 - 1) * (6.0 / (H + 2 * C)) ** 0.5 * 3.0
    b = torch.randn(H * C, generator=g) * 0.1
    go = torch.randn(N, H * C, generator=g)
    return ei, x, W, att, b, go


def _rule_keep(side, H, p, seed, draw):
    """Rule D in numpy over the entries of one side: ``[nnz, H]`` float32 (the host's copy of the CSR arrays; padding cut off)"""
    nnz = int(side.rowptr[-1])
    return torch.from_numpy(D.keep_np(seed, draw, p, D.slots(side.eid[:nnz].cpu().numpy(), side.col[:nnz].cpu().numpy()), H)), nnz


# ---- the mask on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,p,seed,draw", [(1, 0.6, 0, 0), (4, 0.4, 12345, 7), (3, 0.9, 1, 3)])
def test_mask_on_the_device_is_the_numpy_rule(dev, H, p, seed, draw):
    g = torch.Generator().manual_seed(H)
    N, E = 700, 5000
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1, :40] = ei[0, :40]                                    # self loops in the list (dropped by the build; their eids stay unused)
    ei[:, 100:160] = ei[:, 200:260]                            # parallel edges: equal pairs with different eids
    square = npi.CSRGraph(ei.to(dev), N)
    n_src, n_dst = 500, 300
    eb = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    pair = npi.BipartiteGraph(eb.to(dev), (n_src, n_dst))
    for graph, n_loops in ((square, N), (pair, 0)):
        per_edge = {}
        for which in ("by_dst", "by_src"):
            side = getattr(graph, which)
            got = NF.gat_dropout_keep(graph, H, p, seed=seed, draw=draw, side=which)
            want, nnz = _rule_keep(side, H, p, seed, draw)
            assert got.shape == (side.nnz_max, H) and got.dtype == torch.float32
            assert torch.equal(got[:nnz].cpu(), want), which
            assert float(got[nnz:].abs().sum()) == 0.0
            assert set(want.unique().tolist()) <= {0.0, float(D.scale(p))}
            # the value of every edge, keyed by its slot: eid, or 2^32 + node for an appended loop
            k = D.slots(side.eid[:nnz].cpu().numpy(), side.col[:nnz].cpu().numpy())
            order = np.argsort(k, kind="stable")
            per_edge[which] = (k[order], want.numpy()[order])
            assert int((side.eid[:nnz] < 0).sum()) == n_loops
        assert np.array_equal(per_edge["by_dst"][0], per_edge["by_src"][0])            # the same edges on both sides ...
        assert np.array_equal(per_edge["by_dst"][1], per_edge["by_src"][1])            # ... and the same decision for each
    assert torch.equal(NF.gat_dropout_keep(square, H, p, seed=seed, draw=draw), NF.gat_dropout_keep(square, H, p, seed=seed, draw=draw))
    assert not torch.equal(NF.gat_dropout_keep(square, H, p, seed=seed, draw=draw), NF.gat_dropout_keep(square, H, p, seed=seed, draw=draw + 1))
    assert NF.gat_dropout_keep(square, H, p).shape == (square.by_dst.nnz_max, H)       # without a seed: torch's generator, as before


# ---- the square form against the oracle under the Rule D mask --------------------------------------------------------------------
def _square_parity(dev, N, E, Fi, H, C, p=0.4, item=64, concat=True, relu=False, schedule=DEFAULT, scales=False, hub=True, seed=11, draw=2):
    ei, x, W, att, b, go = _case(N, E, Fi, H, C, seed=N + H + C, hub=hub)
    if not concat:
        b, go = b[:C].clone(), go[:, :C].clone()
    graph = npi.CSRGraph(ei.to(dev), N, item=item)
    d = graph.by_dst
    keep, nnz = _rule_keep(d, H, p, seed, draw)
    ks = R.keep_scale_from_entries(ei, N, d.eid[:nnz].cpu(), d.rowidx[:nnz].cpu(), keep)
    xr, Wr, ar, br = (t.clone().double().requires_grad_(True) for t in (x, W, att, b))
    pre = R.gat_conv(xr, ei, Wr, ar, br, heads=H, concat=concat, keep_scale=ks)
    if relu:
        go = torch.where(pre.detach().abs() < 1e-4, torch.zeros(()), go)      # away from the ReLU's kink: fp32 may take the other side
    ref = torch.relu(pre) if relu else pre
    ref.backward(go.double())
    xd, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x, W, att, b))
    rule = NF.AttentionDropout(p, seed, draw)
    res = npi.gat_conv(xd, graph, Wd, ad, bd, heads=H, concat=concat, relu=relu, schedule=schedule, dropout=rule, return_scales=scales)
    out, sc = res if scales else (res, None)
    out.backward(go.to(dev))
    print(f"N={N} H={H} C={C} item={item}: out {float((out.detach().cpu().double() - ref.detach()).abs().max()):.3g} "
          f"dX {float((xd.grad.cpu().double() - xr.grad).abs().max()):.3g} "
          f"dW {rel_max(Wd.grad, Wr.grad):.3g} datt {rel_max(ad.grad, ar.grad):.3g} db {rel_max(bd.grad, br.grad):.3g}")
    assert torch.allclose(out.detach().cpu(), ref.detach().float(), atol=1e-4, rtol=1e-4)
    assert torch.allclose(xd.grad.cpu(), xr.grad.float(), atol=2e-4, rtol=1e-3)
    for got, want in ((Wd.grad, Wr.grad), (ad.grad, ar.grad), (bd.grad, br.grad)):
        assert rel_max(got, want) <= GRAD_REL, rel_max(got, want)
    return graph, (xd, Wd, ad, bd), out.detach(), sc, ref.detach()


@pytest.mark.parametrize("N,E,Fi,H,C", [(60, 300, 16, 1, 8), (1500, 12000, 48, 2, 32), (1500, 12000, 32, 4, 64), (800, 6000, 32, 8, 32),
                                        (3000, 40000, 64, 1, 256), (800, 6000, 32, 1, 100),
                                        (800, 6000, 32, 3, 16), (60, 300, 16, 1, 6)])       # the last two: the composed variant
@pytest.mark.parametrize("item", [64, 256])
def test_square_form_matches_the_oracle_under_the_rule_d_mask(dev, N, E, Fi, H, C, item):
    graph, (xd, Wd, ad, bd), out, _, _ = _square_parity(dev, N, E, Fi, H, C, item=item)
    # the mask matters: the layer without dropout is somewhere else (the oracle's: the plain kernels do not serve C % 4 != 0)
    ei = _case(N, E, Fi, H, C, seed=N + H + C)[0]
    plain = R.gat_conv(xd.detach().cpu(), ei, Wd.detach().cpu(), ad.detach().cpu(), bd.detach().cpu(), heads=H)
    assert not torch.allclose(out.cpu(), plain, atol=1e-3)


@pytest.mark.parametrize("N,E,Fi,H,C", [(1500, 12000, 32, 4, 64), (800, 6000, 32, 1, 100), (800, 6000, 32, 3, 16)])
def test_square_form_head_average(dev, N, E, Fi, H, C):
    _square_parity(dev, N, E, Fi, H, C, concat=False, p=0.6)


def test_square_form_options_keep_working(dev):
    # the ReLU in the row epilogue, with the row scales of the output written by the same launch (one head of 256 channels)
    _, _, out, sc, _ = _square_parity(dev, 3000, 40000, 64, 1, 256, relu=True, scales=True)
    assert sc is not None and torch.equal(sc, NF.row_scales(out))
    assert bool((out >= 0).all()) and float((out == 0).float().mean()) > 0.2
    _square_parity(dev, 1500, 12000, 48, 2, 32, relu=True)
    # the rank-2 backward (dX's attention terms in its GEMM's store epilogue), which the product takes from 100,000 rows on
    _square_parity(dev, 3000, 40000, 128, 1, 256, schedule=DEFAULT.but(gat_rank2_min_rows=0))
    _square_parity(dev, 800, 6000, 128, 1, 64, schedule=DEFAULT.but(gat_rank2_min_rows=0), item=256)
    # g_src by its own pass instead of out of the fused launch; the statistics pass in front (the composed variant)
    _square_parity(dev, 800, 6000, 32, 1, 100, schedule=DEFAULT.but(gat_src_rowsum_fused=False))
    _square_parity(dev, 3000, 40000, 64, 1, 256, schedule=DEFAULT.but(gat_src_rowsum_fused=False, gat_rank2_min_rows=0))
    _square_parity(dev, 1500, 12000, 32, 4, 64, schedule=DEFAULT.but(gat_fused_stats=False))


@pytest.mark.parametrize("H,C,item", [(1, 64, 64), (1, 64, 256), (4, 32, 64), (2, 128, 256)])
def test_rows_that_stress_the_aggregation(dev, H, C, item):
    """one row of > 4096 entries (the shape of test_gat_heavy_row_softmax: cut over items and workgroups, the chain in `carry`), rows
    straddling item and workgroup boundaries, and p = 0.9: most short rows lose every entry and come out as the bias"""
    N, E, Fi = 9000, 30000, 32
    graph, (xd, Wd, ad, bd), out, _, ref = _square_parity(dev, N, E, Fi, H, C, p=0.9, item=item, seed=5, draw=0)
    d = graph.by_dst
    assert int((d.rowptr[1:] - d.rowptr[:-1]).max()) > 4096
    keep, nnz = _rule_keep(d, H, 0.9, 5, 0)
    alive = torch.zeros(N, H).index_add_(0, d.rowidx[:nnz].cpu().long(), keep)
    dead = (alive == 0).all(dim=1)
    assert int(dead.sum()) > N // 10                            # (0.9 ** (3.2 entries x H heads) of the short rows: 26 % at four heads)
    assert torch.equal(out[dead.to(dev)], bd.detach().expand(int(dead.sum()), H * C))      # every entry dropped: exactly the bias


def test_empty_rows_and_the_edge_list_as_it_is(dev):
    """targets without any in-edge (no self loop is added in the pair form): the bias; against the fp64 restatement"""
    _bipartite_parity(dev, "size", 1, 64, empty=True)
    _bipartite_parity(dev, "size", 4, 32, empty=True)


# ---- the same mask on both paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,Fi,H,C", [(1500, 12000, 32, 4, 64), (3000, 40000, 64, 1, 256), (60, 300, 16, 1, 8)])
def test_fused_and_composed_paths_share_the_mask(dev, N, E, Fi, H, C):
    ei, x, W, att, b, go = _case(N, E, Fi, H, C, seed=N)
    graph = npi.CSRGraph(ei.to(dev), N)
    rule = NF.AttentionDropout(0.4, 3, 1)
    runs = []
    for kw in (dict(dropout=rule), dict(keep=NF.gat_dropout_keep(graph, H, 0.4, seed=3, draw=1))):
        xd, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x, W, att, b))
        out = npi.gat_conv(xd, graph, Wd, ad, bd, heads=H, **kw)
        out.backward(go.to(dev))
        runs.append((out.detach(), xd.grad, Wd.grad, ad.grad, bd.grad))
    f, c = runs
    assert torch.allclose(f[0], c[0], atol=1e-4, rtol=1e-4)
    assert torch.allclose(f[1], c[1], atol=2e-4, rtol=1e-3)
    for got, want in zip(f[2:], c[2:]):
        assert rel_max(got, want) <= GRAD_REL, rel_max(got, want)
    plain = npi.gat_conv(x.to(dev), graph, W.to(dev), att.to(dev), b.to(dev), heads=H)
    assert not torch.allclose(f[0], plain, atol=1e-3)
    zero = npi.gat_conv(x.to(dev), graph, W.to(dev), att.to(dev), b.to(dev), heads=H, dropout=NF.AttentionDropout(0.0, 3, 1))
    print(f"H={H} C={C}: p = 0 bitwise equal to the plain layer: {torch.equal(zero, plain)}")
    assert torch.allclose(zero, plain, atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError, match="keep"):
        npi.gat_conv(x.to(dev), graph, W.to(dev), att.to(dev), b.to(dev), heads=H, dropout=rule, keep=torch.ones(1, H, device=dev))


# ---- bipartite ---------------------------------------------------------------------------------------------------------------------
def _bipartite_parity(dev, form, H, C, concat=True, relu=False, empty=False, p=0.5, seed=9, draw=4):
    n_src, n_dst, E, Fi = 700, 500, 6000, 32
    if form == "size":
        n_dst = n_src
    g = torch.Generator().manual_seed(H * 10 + C + len(form))
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst - (40 if empty else 0), (E,), generator=g)])
    ei[1, :1500] = 2                                           # a heavy target
    x_src = torch.randn(n_src, Fi, generator=g)
    x_dst = torch.randn(n_dst, Fi, generator=g) if form == "pair" else None
    W = torch.randn(Fi, H * C, generator=g) / Fi ** 0.5
    att = torch.randn(1, H, 2 * C, generator=g) / C ** 0.5
    b = torch.randn(H * C if concat else C, generator=g)
    go = torch.randn(n_dst, H * C if concat else C, generator=g)
    ks = torch.from_numpy(D.keep_np(seed, draw, p, np.arange(E), H)).double()          # an edge's slot is its column: no loops here
    xr, Wr, ar, br = (t.clone().double().requires_grad_(True) for t in (x_src, W, att, b))
    xdr = x_dst.clone().double().requires_grad_(True) if form == "pair" else None
    ref = D.gat_bipartite(xr, xr if form == "size" else xdr, ei, Wr, ar, br, n_dst=n_dst, heads=H, concat=concat, keep_scale=ks)
    ref.backward(go.double())
    xs, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x_src, W, att, b))
    xd = x_dst.to(dev).requires_grad_(True) if form == "pair" else None
    rule = NF.AttentionDropout(p, seed, draw)
    if form == "size":
        out = npi.gat_conv_bipartite((xs, None), ei.to(dev), Wd, ad, bd, size=(n_src, n_dst), heads=H, concat=concat, shared=True, dropout=rule)
    else:
        out = npi.gat_conv_bipartite((xs, xd), ei.to(dev), Wd, ad, bd, size=(n_src, n_dst), heads=H, concat=concat, dropout=rule)
    out.backward(go.to(dev))
    assert torch.allclose(out.detach().cpu(), ref.detach().float(), atol=1e-4, rtol=1e-4)
    assert torch.allclose(xs.grad.cpu(), xr.grad.float(), atol=2e-4, rtol=1e-3)
    if form == "pair":
        assert torch.allclose(xd.grad.cpu(), xdr.grad.float(), atol=2e-4, rtol=1e-3)
    for got, want in ((Wd.grad, Wr.grad), (ad.grad, ar.grad), (bd.grad, br.grad)):
        assert rel_max(got, want) <= GRAD_REL, rel_max(got, want)
    if form == "src_only":
        assert float(ad.grad[..., :C].abs().max()) == 0.0                             # no target term: a zero gradient
    if empty:
        assert torch.equal(out.detach()[n_dst - 40:], bd.detach().expand(40, -1))
    plain = npi.gat_conv_bipartite((xs.detach(), xd.detach() if xd is not None else None), ei.to(dev), Wd.detach(), ad.detach(), bd.detach(),
                                   size=(n_src, n_dst), heads=H, concat=concat, shared=form == "size")
    assert not torch.allclose(out.detach(), plain, atol=1e-3)


@pytest.mark.parametrize("H,C", [(1, 64), (4, 32)])
@pytest.mark.parametrize("form", ["pair", "src_only", "size"])
def test_bipartite_form_matches_the_fp64_restatement(dev, form, H, C):
    _bipartite_parity(dev, form, H, C)
    if form == "pair" and H == 4:
        _bipartite_parity(dev, form, H, C, concat=False)


def test_bipartite_unserved_shape_and_sampler_block(dev):
    g = torch.Generator().manual_seed(0)
    N, E, Fi = 2000, 16000, 32
    ei = torch.randint(0, N, (2, E), generator=g).to(dev)
    feat = torch.randn(N, Fi, generator=g).to(dev)
    with pytest.raises(NotImplementedError, match="heads"):
        npi.gat_conv_bipartite((feat, None), ei, torch.zeros(Fi, 48, device=dev), torch.zeros(1, 3, 32, device=dev), size=(N, N), heads=3,
                               dropout=NF.AttentionDropout(0.5, 0, 0))
    conv3 = npi.GATConv(Fi, 16, heads=3, dropout=0.5, seed=0).to(dev).train()
    with pytest.raises(NotImplementedError, match="heads"):
        conv3((feat, None), ei, size=(N, N))
    # one NeighborSampler block through a seeded module in training mode: trains, and replays from (seed, draw)
    sampler = npi.NeighborSampler(ei, N, size=[8], num_hops=1, batch_size=256, shuffle=False, seed=0)
    flow = next(iter(sampler(None)))
    block = flow[0]
    conv = npi.GATConv(Fi, 32, heads=4, dropout=0.5, seed=0).to(dev).train()
    x = feat[block.n_id].clone().requires_grad_(True)
    out = conv((x, None), block.graph(), size=block.size)
    assert out.shape == (block.size[1], 128) and conv.draw == 1
    out.sum().backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in conv.parameters()) and bool(torch.isfinite(x.grad).all())
    conv.draw = 0
    assert torch.equal(conv((x, None), block.graph(), size=block.size), out)
    assert not torch.equal(conv((x, None), block.graph(), size=block.size), out)       # draw 1
    conv.eval()
    plain = npi.GATConv(Fi, 32, heads=4).to(dev)
    plain.load_state_dict(conv.state_dict())
    assert torch.equal(conv((x, None), block.graph(), size=block.size), plain((x, None), block.graph(), size=block.size))


# ---- determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", [(1, 256), (4, 64), (8, 32)])
def test_a_step_is_reproducible_from_seed_and_draw(dev, H, C):
    N, E, Fi = 4000, 60000, 64
    ei, x, W, att, b, go = _case(N, E, Fi, H, C, seed=4)

    def run(graph, draw):
        xd, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x, W, att, b))
        out = npi.gat_conv(xd, graph, Wd, ad, bd, heads=H, dropout=NF.AttentionDropout(0.6, 21, draw))
        out.backward(go.to(dev))
        return out.detach(), xd.grad, Wd.grad, ad.grad, bd.grad
    graph = npi.CSRGraph(ei.to(dev), N)
    a, c, nxt = run(graph, 0), run(graph, 0), run(graph, 1)
    for p, q in zip(a, c):
        assert torch.equal(p, q)
    assert not torch.equal(a[0], nxt[0]) and not torch.equal(a[1], nxt[1])
    # the mask follows the EDGE, not the entry's position: another entry order of the same edge list, the same layer
    s = run(npi.CSRGraph(ei.to(dev), N, sort_columns=True), 0)
    assert not torch.equal(graph.by_dst.col, npi.CSRGraph(ei.to(dev), N, sort_columns=True).by_dst.col)
    assert torch.allclose(a[0], s[0], atol=1e-4, rtol=1e-4)
    assert torch.allclose(a[1], s[1], atol=2e-4, rtol=1e-3)
    for got, want in zip(a[2:], s[2:]):
        assert rel_max(got, want) <= GRAD_REL, rel_max(got, want)


# ---- the module ----------------------------------------------------------------------------------------------------------------------
def test_module_seed_and_draw(dev):
    g = torch.Generator().manual_seed(3)
    ei = torch.randint(0, 300, (2, 2000), generator=g).to(dev)
    x = torch.randn(300, 32, generator=g).to(dev)
    for heads, C in ((2, 16), (2, 32)):                       # the composed variant under Rule D; the fused kernels
        a, b = npi.GATConv(32, C, heads=heads, dropout=0.6, seed=7).to(dev), npi.GATConv(32, C, heads=heads).to(dev)
        b.load_state_dict(a.state_dict())
        a.eval()
        assert torch.equal(a(x, ei), b(x, ei)) and a.draw == 0             # evaluation: the identity, and no draw is taken
        a.train()
        o0, o1 = a(x, ei), a(x, ei)
        assert a.draw == 2 and o0.shape == (300, heads * C) and not torch.equal(o0, o1)
        a.draw = 0
        assert torch.equal(a(x, ei), o0) and torch.equal(a(x, ei), o1) and a.draw == 2      # set back: the steps replay
        o1.sum().backward()
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in a.parameters())
        other = npi.GATConv(32, C, heads=heads, dropout=0.6, seed=8).to(dev)
        other.load_state_dict(a.state_dict())
        assert not torch.equal(other(x, ei), o0)
        mean = torch.stack([a(x, ei).detach() for _ in range(400)]).mean(0)               # E[alpha kappa] = alpha
        ref = b(x, ei).detach()
        assert float((mean - ref).abs().mean()) <= 0.12 * float(ref.abs().mean())
