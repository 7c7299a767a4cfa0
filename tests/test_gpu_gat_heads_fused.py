"""The fused GATConv forward for 2 / 4 / 8 heads (``npi_gat_aggregate_fused_heads``: aggregation, per-head scores and per-head softmax
statistics in one launch) against the two-launch path, the fp64 definition and the oracle."""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import functional as NF
from npi_gnn_amd.schedule import DEFAULT
from _util import GRAD_REL, rel_max
from oracle import ref_conv as R
import _bipartite_ref as bref

pytestmark = pytest.mark.gpu

SHAPES = [(2, 32), (2, 128), (4, 64), (8, 32), (4, 32)]          # (4, 32): 128 of 256 columns, half the lanes inactive
HEAD_SCALE = [0.5, 2.0, 6.0, 1.0, 3.0, 0.25, 4.0, 1.5]           # att per head: heads reach new maxima at different entries
HUB = 7
_graphs = {}


def _hub_graph(dev, item):
    """N = 2,000: one hub target (40,000 in-edges at 64-entry items = 156 workgroups: the two-level chain; 70,000 at 256-entry
    items), 20,000 random edges, no in-edge at all from node 1,500 on, and the hub row padded to end exactly on an item boundary"""
    if item not in _graphs:
        N = 2000
        g = torch.Generator().manual_seed(item)
        hub_n = 40_000 if item == 64 else 70_000
        rnd = torch.stack([torch.randint(0, N, (20_000,), generator=g), torch.randint(0, 1500, (20_000,), generator=g)])
        hub = torch.stack([torch.randint(0, N, (hub_n,), generator=g), torch.full((hub_n,), HUB)])
        ei = torch.cat([hub, rnd], 1)
        pad = (-int((ei[1] <= HUB).sum())) % item
        ei = torch.cat([ei, torch.stack([torch.randint(0, N, (pad,), generator=g), torch.full((pad,), HUB)])], 1)
        graph = npi.CSRGraph(ei.to(dev), N, self_loops=False, keep_equal=True, item=item)
        assert graph.by_dst.item == item and int(graph.by_dst.rowptr[HUB + 1]) % item == 0
        _graphs[item] = (ei, graph)
    return _graphs[item]


def _lrelu(z):
    return torch.where(z > 0, z, 0.2 * z)


@pytest.mark.parametrize("item", [64, 256])
@pytest.mark.parametrize("H,C", SHAPES)
def test_fused_heads_forward_equals_the_two_launch_path(dev, H, C, item):
    ei, graph = _hub_graph(dev, item)
    d = graph.by_dst
    N = graph.num_nodes
    g = torch.Generator().manual_seed(100 * H + C)
    h = torch.randn(N, H * C, generator=g).to(dev)
    att = (torch.randn(H, 2 * C, generator=g) * (torch.tensor(HEAD_SCALE[:H]).view(H, 1) / C ** 0.5)).to(dev)
    bias = torch.randn(H * C, generator=g).to(dev)
    a_dst, a_src = NF.gat_scores(h, att, H, C)
    m0, s0 = NF.gat_softmax_stats(d, a_dst, a_src, H, 0.2)
    ref = torch.relu(NF._gat_aggregate(graph, d, h, H, C, a_dst, a_src, m0, s0, 0.2, False) + bias)
    out, m, s = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, 0.2, bias=bias, relu=True, H=H)
    torch.cuda.synchronize()
    assert out.shape == (N, H * C) and m.shape == (N, H) and s.shape == (N, H)
    nnz = int(d.rowptr[-1])
    sc = _lrelu(a_dst[d.rowidx[:nnz].long()] + a_src[d.col[:nnz].long()])              # [nnz, H]: every entry's score
    for hd in range(H):
        tol = 4e-6 * max(1.0, float(sc[:, hd].abs().max()))
        e_m = float((m[:, hd] - m0[:, hd]).abs().max())
        e_s = float(((s[:, hd] - s0[:, hd]).abs() / s0[:, hd].abs().clamp(min=1e-30)).max())
        r_h, o_h = ref[:, hd * C:(hd + 1) * C], out[:, hd * C:(hd + 1) * C]
        e_o = float((o_h - r_h).abs().max())
        print(f"H={H} C={C} item={item} head {hd}: m {e_m:.2e} (tol {tol:.2e})  s {e_s:.2e}  out {e_o:.2e}")
        assert e_m <= tol
        assert e_s <= 10 * tol + 2e-5
        assert e_o <= 5e-5 * max(1.0, float(r_h.abs().max()))
        # the hub row of this head against the definition in fp64
        src = ei[0][ei[1] == HUB].to(dev)
        e = _lrelu((a_dst[HUB, hd] + a_src[src, hd]).double())
        w = torch.softmax(e, 0)
        want = torch.relu((w.view(-1, 1) * h[src, hd * C:(hd + 1) * C].double()).sum(0) + bias[hd * C:(hd + 1) * C].double())
        assert float((o_h[HUB].double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
        assert abs(float(m[HUB, hd]) - float(e.max())) <= tol
        s_def = float((e - e.max()).exp().sum())
        assert abs(float(s[HUB, hd]) - s_def) <= (10 * tol + 2e-5) * s_def
    # rows without an entry: m = s = 0 exactly, out = bias (the ReLU off), as the statistics pass leaves them
    empty = torch.bincount(ei[1], minlength=N).to(dev) == 0
    assert int(empty.sum()) >= 500
    plain, m1, s1 = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, 0.2, bias=bias, H=H)
    assert torch.equal(plain[empty], bias.expand(int(empty.sum()), H * C))
    assert torch.equal(out[empty], torch.relu(bias).expand(int(empty.sum()), H * C))
    assert float(m[empty].abs().max()) == 0.0 and float(s[empty].abs().max()) == 0.0
    assert torch.equal(m1, m) and torch.equal(s1, s) and torch.equal(torch.relu(plain), out)
    for _ in range(3):
        o2, m2, s2 = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, 0.2, bias=bias, relu=True, H=H)
        assert torch.equal(o2, out) and torch.equal(m2, m) and torch.equal(s2, s)


def test_fused_heads_two_part_table_is_bit_equal(dev):
    N, E, H, C, k = 600, 8000, 4, 64, 250
    g = torch.Generator().manual_seed(3)
    graph = npi.CSRGraph(torch.randint(0, N, (2, E), generator=g).to(dev), N)
    d = graph.by_dst
    h = torch.randn(N, H * C, generator=g).to(dev)
    att = (torch.randn(H, 2 * C, generator=g) * (torch.tensor(HEAD_SCALE[:H]).view(H, 1) / C ** 0.5)).to(dev)
    bias = torch.randn(H * C, generator=g).to(dev)
    a_dst, _ = NF.gat_scores(h, att, H, C)
    one = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, 0.2, bias=bias, relu=True, H=H)
    two = NF.gat_aggregate_fused(d, h[:k], h[k:], C, a_dst, att, 0.2, bias=bias, relu=True, H=H)
    for a, b in zip(one, two):
        assert torch.equal(a, b)


def test_two_part_table_is_bit_equal_in_the_other_wrappers(dev):
    """The second part of the table through the wrappers the fused launches above do not cover: ``_gat_aggregate`` by target and by
    source, ``gat_aggregate_scores`` and ``gat_edge_grad`` in both orientations.  The same kernel adds the same entries in the same
    order -- only the address of a gathered row differs -- so the result is bit equal to the call with the whole table."""
    N, E, k = 600, 8000, 250
    g = torch.Generator().manual_seed(3)
    graph = npi.CSRGraph(torch.randint(0, N, (2, E), generator=g).to(dev), N)
    d, sr = graph.by_dst, graph.by_src

    def operands(H, C):
        h, dout = torch.randn(N, H * C, generator=g).to(dev), torch.randn(N, H * C, generator=g).to(dev)
        att = (torch.randn(H, 2 * C, generator=g) / C ** 0.5).to(dev)
        a_dst, a_src = NF.gat_scores(h, att, H, C)
        return h, dout, a_dst, a_src

    H, C = 3, 16
    h, dout, a_dst, a_src = operands(H, C)
    m, s = NF.gat_softmax_stats(d, a_dst, a_src, H, 0.2)
    for side, table, by_source in ((d, h, False), (sr, dout, True)):
        one = NF._gat_aggregate(graph, side, table, H, C, a_dst, a_src, m, s, 0.2, by_source)
        two = NF._gat_aggregate(graph, side, table[:k], H, C, a_dst, a_src, m, s, 0.2, by_source, x2=table[k:])
        assert torch.equal(one, two), by_source

    H, C = 1, 64
    h, _, a_dst, a_src = operands(H, C)
    bias = torch.randn(C, generator=g).to(dev)
    m, s, sc = NF.gat_softmax_stats(d, a_dst, a_src, H, 0.2, want_scores=True)
    one = NF.gat_aggregate_scores(d, h, None, C, sc, m, s, bias=bias, relu=True)
    two = NF.gat_aggregate_scores(d, h[:k], h[k:], C, sc, m, s, bias=bias, relu=True)
    assert torch.equal(one, two)

    H, C = 2, 32
    h, dout, a_dst, a_src = operands(H, C)
    m, s = NF.gat_softmax_stats(d, a_dst, a_src, H, 0.2)
    D = torch.randn(N, H, generator=g).to(dev)
    for side, table, rows, swap in ((d, h, dout, 0), (sr, dout, h, 1)):
        nnz = int(side.rowptr[-1])
        one = NF.gat_edge_grad(side, table, None, rows, H, C, a_dst, a_src, m, s, D, 0.2, swap)
        two = NF.gat_edge_grad(side, table[:k], table[k:], rows, H, C, a_dst, a_src, m, s, D, 0.2, swap)
        assert nnz > 0 and torch.equal(one[:nnz], two[:nnz]), swap


def test_four_heads_take_the_fused_launch(dev, monkeypatch):
    """With the statistics pass made to raise, the 4 x 64 layer still runs its forward (one-id-space and pair form); with
    Schedule(gat_fused_stats=False) the statistics pass is reached."""
    def boom(*a, **k):
        raise RuntimeError("statistics pass reached")
    monkeypatch.setattr(NF, "gat_softmax_stats", boom)
    N, E, Fi, H, C = 500, 5000, 64, 4, 64
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, N, (2, E), generator=g).to(dev)
    x = torch.randn(N, Fi, generator=g).to(dev)
    W = (torch.randn(Fi, H * C, generator=g) / Fi ** 0.5).to(dev)
    att = (torch.randn(1, H, 2 * C, generator=g) / C ** 0.5).to(dev)
    b = torch.randn(H * C, generator=g).to(dev)
    out = npi.gat_conv(x, ei, W, att, b, heads=H)
    assert out.shape == (N, H * C) and bool(torch.isfinite(out).all())
    conv = npi.GATConv(Fi, C, heads=H).to(dev)
    bg = npi.BipartiteGraph(ei, (N, N))
    out2 = conv((x, x), bg)
    assert out2.shape == (N, H * C) and bool(torch.isfinite(out2).all())
    off = DEFAULT.but(gat_fused_stats=False)
    with pytest.raises(RuntimeError, match="statistics pass reached"):
        npi.gat_conv(x, ei, W, att, b, heads=H, schedule=off)
    with pytest.raises(RuntimeError, match="statistics pass reached"):
        npi.GATConv(Fi, C, heads=H, schedule=off).to(dev)((x, x), bg)


_oracle = {}


def _inputs(H, C):
    """N = 3,000, E = 40,000 with one heavy target and one heavy source, as tests/test_gpu_gat.py builds its cases"""
    N, E, Fi = 3000, 40_000, 64
    g = torch.Generator().manual_seed(H * 100 + C)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1, : E // 3] = 3
    ei[0, E // 3: E // 2] = 5
    x = torch.randn(N, Fi, generator=g)
    W = (torch.rand(Fi, H * C, generator=g) * 2 - 1) * (6.0 / (Fi + H * C)) ** 0.5
    att = (torch.rand(1, H, 2 * C, generator=g) * 2 - 1) * (6.0 / (H + 2 * C)) ** 0.5 * 3.0
    b = torch.randn(H * C, generator=g) * 0.1
    go = torch.randn(N, H * C, generator=g)
    return ei, x, W, att, b, go


def _layer_case(H, C):
    """inputs and the oracle's forward / gradients (fp32 for the activations' bars, fp64 for the parameter gradients), once per shape"""
    if (H, C) not in _oracle:
        ei, x, W, att, b, go = _inputs(H, C)
        xr, Wr, ar, br = (t.clone().requires_grad_(True) for t in (x, W, att, b))
        ref = R.gat_conv(xr, ei, Wr, ar, br, heads=H)
        ref.backward(go)
        x6, W6, a6, b6 = (t.clone().double().requires_grad_(True) for t in (x, W, att, b))
        R.gat_conv(x6, ei, W6, a6, b6, heads=H).backward(go.double())
        _oracle[(H, C)] = ((ei, x, W, att, b, go), (ref.detach(), xr.grad), (W6.grad, a6.grad, b6.grad))
    return _oracle[(H, C)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("H,C", [(2, 32), (4, 64), (8, 32)])
def test_gat_conv_heads_fwd_bwd_matches_oracle(dev, H, C, fused):
    (ei, x, W, att, b, go), (ref, dx), grads64 = _layer_case(H, C)
    xd, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x, W, att, b))
    out = npi.gat_conv(xd, ei.to(dev), Wd, ad, bd, heads=H, schedule=DEFAULT.but(gat_fused_stats=fused))
    out.backward(go.to(dev))
    assert torch.allclose(out.detach().cpu(), ref.float(), atol=1e-4, rtol=1e-4)
    assert torch.allclose(xd.grad.cpu(), dx.float(), atol=2e-4, rtol=1e-3)
    for got, want in zip((Wd.grad, ad.grad, bd.grad), grads64):
        assert rel_max(got, want) <= GRAD_REL, rel_max(got, want)


def _row_scaled(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(((got - want).abs() / (1.0 + want.abs().amax(1, keepdim=True))).max())


def test_pair_form_four_heads_matches_the_fp64_restatement(dev):
    n_src, n_dst, Fin, H, C = 1500, 400, 48, 4, 32
    g = torch.Generator().manual_seed(29)
    ei = torch.stack([torch.randint(0, n_src, (6200,), generator=g), torch.randint(0, n_dst - 15, (6200,), generator=g)])
    ei[1, :1200] = 2                                                     # one heavy target; the last 15 targets stay empty
    x_src = torch.randn(n_src, Fin, generator=g).double()
    x_dst = torch.randn(n_dst, Fin, generator=g).double()
    W = (torch.randn(Fin, H * C, generator=g) / Fin ** 0.5).double()
    att = (torch.randn(1, H, 2 * C, generator=g) / C ** 0.5).double()
    b = torch.randn(H * C, generator=g).double()
    go = torch.randn(n_dst, H * C, generator=g).double()
    xr, xdr, Wr, ar, br = (t.clone().requires_grad_(True) for t in (x_src, x_dst, W, att, b))
    want = bref.gat_bipartite(xr, xdr, ei, Wr, ar, br, n_dst=n_dst, heads=H)
    want.backward(go)
    conv = npi.GATConv(Fin, C, heads=H).to(dev)
    with torch.no_grad():
        conv.weight.copy_(W)
        conv.att.copy_(att)
        conv.bias.copy_(b)
    xg, xdg = (t.to(dev).float().requires_grad_(True) for t in (x_src, x_dst))
    out = conv((xg, xdg), ei.to(dev))
    out.backward(go.float().to(dev))
    for name, got, ref in (("out", out, want), ("dX_src", xg.grad, xr.grad), ("dX_dst", xdg.grad, xdr.grad)):
        assert _row_scaled(got, ref) < 1e-4, name
    for name, got, ref in (("dW", conv.weight.grad, Wr.grad), ("d att", conv.att.grad, ar.grad), ("db", conv.bias.grad, br.grad)):
        assert rel_max(got, ref) < GRAD_REL, name
    assert _row_scaled(out[n_dst - 15:], b.expand(15, -1)) < 1e-6         # empty targets: the bias


@pytest.mark.parametrize("H,C", [(4, 64), (8, 32)])
def test_fused_relu_heads_equals_relu_behind_the_layer(dev, H, C):
    ei, x, W, att, b, go = _inputs(H, C)
    res = []
    for fused in (False, True):
        xd, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x, W, att, b))
        out = npi.gat_conv(xd, ei.to(dev), Wd, ad, bd, heads=H, relu=fused)
        if not fused:
            out = torch.relu(out)
        out.backward(go.to(dev))
        res.append((out.detach(), xd.grad, Wd.grad, ad.grad, bd.grad))
    assert bool((res[1][0] >= 0).all()) and float((res[1][0] == 0).float().mean()) > 0.2      # a real ReLU
    assert torch.equal(res[0][0], res[1][0])
    for a, c in zip(res[0][1:], res[1][1:]):
        assert torch.allclose(a, c, rtol=1e-5, atol=1e-6 * float(a.abs().max()))



def test_fused_heads_take_a_bias_that_is_not_16_byte_aligned(dev):
    """the row epilogue reads the bias one scalar at a time: a view at a 4-byte offset gives the bits of an aligned copy"""
    N, E, H, C = 600, 8000, 4, 64
    g = torch.Generator().manual_seed(4)
    d = npi.CSRGraph(torch.randint(0, N, (2, E), generator=g).to(dev), N).by_dst
    h = torch.randn(N, H * C, generator=g).to(dev)
    att = (torch.randn(H, 2 * C, generator=g) / C ** 0.5).to(dev)
    buf = torch.randn(H * C + 1, generator=g).to(dev)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    a_dst, _ = NF.gat_scores(h, att, H, C)
    want = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, 0.2, bias=view.clone(), relu=True, H=H)
    got = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, 0.2, bias=view, relu=True, H=H)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
