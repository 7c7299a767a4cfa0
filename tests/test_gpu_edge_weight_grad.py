"""Gradients w.r.t. ``edge_weight`` of SAGEConv and GCNConv (``functional._EdgeWeightGradFn``: ``npi_edge_dot``, ``npi_gcn_norm_bwd``).

The reference is autograd over ``oracle.ref_conv`` on the host in fp64 (``edge_weight.requires_grad_()``, ``out.backward(grad_out)``),
the metric ``_util.rel_max``, the bar ``_util.GRAD_REL`` (1e-5) -- the project's bar for parameter gradients; the same oracle run in
f32 against itself in fp64 gives 1.5e-7 .. 1.8e-6 on inputs of this kind (``randn`` features and ``grad_out``, weights in
[0.5, 1.5)), so the bar leaves a factor of at least 5 over plain f32 arithmetic.  In the same backward dW and db keep GRAD_REL and
out / dX the 1e-4 of their scale the parity tests ask (tests/test_gpu_parity.py).

  * every layer form: ``sage_conv`` plain / relu / normalize / concat, ``gcn_conv`` aggregate-first and project-first, improved,
    normalize=False, through ``nn.SAGEConv`` / ``nn.GCNConv`` and through a ``GraphBatch``
  * widths 1, 3, 64, 178, 256, 300, 1100; graphs with empty rows and isolated nodes, a hub row holding more than half of the
    entries, no edge at all, existing self loops (fill 1 and 2), ``(-1, -1)`` padding columns, a prebuilt ``CSRGraph``, more
    entries than one 256-entry item
  * one case where the fp16 x 2 projection is taken (asserted), two runs bit-identical, the interface (shape, ``[E, 1]`` and
    non-contiguous weights, the constant path bit-identical to ``edge_weight.detach()``, ``norm=`` and bf16 refused)
  * C4 at full size: the closed form in fp64 on 100 000 random edges and on every entry of the 8 heaviest rows
"""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import functional as NF
from npi_gnn_amd.schedule import DEFAULT
from npi_gnn_amd.synth import bipartite_edge_index
from oracle import ref_conv as R
from _util import GRAD_REL, rel_max

pytestmark = pytest.mark.gpu

ATOL = 1e-4          # out and dX, times max(1, max |reference|): the parity tests' bar


def _edges(N, E, seed, hubs=0, loops=0, pad=0, live=None, hub_share=0.5):
    """``E`` random directed edges without self loops among the first ``live`` nodes (the others stay isolated; many of the live
    ones have no in-edge: empty rows but for the loop), ``hub_share`` of them onto ``hubs`` hub targets; then ``loops`` existing self loops
    on distinct nodes and ``pad`` padding columns ``(-1, -1)``, all shuffled."""
    g = torch.Generator().manual_seed(seed)
    live = N if live is None else live
    src = torch.randint(0, live, (E,), generator=g)
    dst = torch.randint(0, live, (E,), generator=g)
    if hubs:
        n_hub = int(E * hub_share)
        dst[:n_hub] = torch.randint(0, hubs, (n_hub,), generator=g)
    if live > 1:
        same = src == dst
        src[same] = (dst[same] + 1) % live
    cols = [torch.stack([src, dst])]
    if loops:
        k = torch.randperm(live, generator=g)[:loops]
        cols.append(torch.stack([k, k]))
    if pad:
        cols.append(torch.full((2, pad), -1, dtype=torch.long))
    ei = torch.cat(cols, 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


def _inputs(N, ei, Fi, Fo, seed, concat=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Fi, generator=g)
    W = torch.randn((2 if concat else 1) * Fi, Fo, generator=g) / max(Fi, 1) ** 0.5
    b = torch.randn(Fo, generator=g)
    ew = torch.rand(ei.size(1), generator=g) + 0.5
    go = torch.randn(N, Fo, generator=g)
    return x, W, b, ew, go


def _reference(layer, x, ei, W, b, ew, go, **kw):
    """fp64 autograd over the oracle on the host.  Padding columns are not part of the oracle's edge list: they are cut out
    and, through the indexing, their weights get the gradient 0."""
    x6, W6, b6 = (t.detach().cpu().double().clone().requires_grad_(True) for t in (x, W, b))
    w6 = ew.detach().cpu().double().reshape(-1).clone().requires_grad_(True)
    ei = ei.cpu()
    keep = ei[0] >= 0
    eik, wk = ei[:, keep], w6[keep]
    if layer == "sage":
        out = R.sage_conv(x6, eik, W6, b6, edge_weight=wk, normalize=kw.get("normalize", False))
        if kw.get("relu"):
            out = torch.relu(out)
    elif layer == "concat":
        out = R.sage_conv_concat(x6, eik, W6, b6, edge_weight=wk)
    else:
        out = R.gcn_conv(x6, eik, W6, b6, edge_weight=wk, improved=kw.get("improved", False), normalize=kw.get("normalize", True))
    out.backward(go.detach().cpu().double())
    return out.detach(), x6.grad, W6.grad, b6.grad, w6.grad


def _run(layer, dev, x, edges, W, b, ew, go, **kw):
    xd, Wd, bd, wd = (t.to(dev).clone().requires_grad_(True) for t in (x, W, b, ew))
    if layer == "sage":
        out = npi.sage_conv(xd, edges, Wd, bd, edge_weight=wd, **kw)
    elif layer == "concat":
        out = npi.sage_conv(xd, edges, Wd, bd, edge_weight=wd, concat=True, **kw)
    else:
        out = npi.gcn_conv(xd, edges, Wd, bd, edge_weight=wd, **kw)
    out.backward(go.to(dev))
    return out.detach(), xd.grad, Wd.grad, bd.grad, wd.grad


def _compare(got, ref, what=""):
    out, dx, dw, db, dwe = got
    out6, dx6, dw6, db6, dwe6 = ref
    assert dwe.shape == dwe6.shape or dwe.numel() == dwe6.numel()
    assert float((out.cpu().double() - out6).abs().max()) <= ATOL * max(1.0, float(out6.abs().max())), what
    assert float((dx.cpu().double() - dx6).abs().max()) <= ATOL * max(1.0, float(dx6.abs().max())), what
    assert rel_max(dw, dw6) <= GRAD_REL and rel_max(db, db6) <= GRAD_REL, (what, rel_max(dw, dw6), rel_max(db, db6))
    if dwe6.numel():
        err = rel_max(dwe.reshape(-1), dwe6)
        print(f"d edge_weight {what}: rel_max {err:.3e} (max |ref| {float(dwe6.abs().max()):.3g})")
        assert err <= GRAD_REL, (what, err)
    else:
        assert dwe.numel() == 0


def _case(dev, layer, N, E, Fi, Fo, seed=0, hubs=0, loops=0, pad=0, live=None, prebuilt=False, hub_share=0.5, **kw):
    ei = _edges(N, E, seed, hubs=hubs, loops=loops, pad=pad, live=live, hub_share=hub_share)
    x, W, b, ew, go = _inputs(N, ei, Fi, Fo, seed + 1, concat=layer == "concat")
    edges = ei.to(dev)
    if prebuilt:
        plain = layer == "concat" or kw.get("normalize") is False
        edges = npi.CSRGraph(edges, N, self_loops=False, keep_equal=True) if plain else npi.CSRGraph(edges, N)
    got = _run(layer, dev, x, edges, W, b, ew, go, **kw)
    _compare(got, _reference(layer, x, ei, W, b, ew, go, **kw), f"{layer} {N}/{E}/{Fi}/{Fo} {kw}")
    assert got[4].shape == ew.shape and got[4].dtype == torch.float32
    return got


# ---- every layer form ---------------------------------------------------------------------------------------------------------------
FORMS = [
    ("sage", 64, 128, {}),
    ("sage", 64, 128, {"relu": True}),
    ("sage", 64, 128, {"normalize": True}),
    ("concat", 64, 128, {}),
    ("gcn", 64, 128, {}),                           # F_in <= F_out: aggregate first
    ("gcn", 178, 64, {}),                           # F_in > F_out: project first
    ("gcn", 64, 128, {"improved": True}),
    ("gcn", 178, 64, {"improved": True}),
    ("gcn", 64, 128, {"normalize": False}),
    ("gcn", 178, 64, {"normalize": False}),
]


@pytest.mark.parametrize("layer,Fi,Fo,kw", FORMS, ids=[f"{f[0]}-{f[1]}x{f[2]}-{'-'.join(f'{k}={v}' for k, v in f[3].items()) or 'plain'}"
                                                      for f in FORMS])
def test_layer_forms(dev, layer, Fi, Fo, kw):
    """5k nodes (500 of them isolated), 100k edges, half of them on 32 hub targets, 50 existing self loops, 37 padding columns"""
    _case(dev, layer, 5000, 100_000, Fi, Fo, seed=10, hubs=32, loops=50, pad=37, live=4500, **kw)


@pytest.mark.parametrize("Fi", [1, 3, 64, 178, 256, 300, 1100])
@pytest.mark.parametrize("layer", ["sage", "gcn"])
def test_widths(dev, layer, Fi):
    """the dot at every kind of width: below a lane quad, unaligned rows (178), one full chunk (256), several chunks"""
    _case(dev, layer, 3000, 60_000, Fi, max(Fi, 8), seed=20 + Fi, hubs=32, loops=50)


@pytest.mark.parametrize("Fo", [1, 3, 300])
def test_widths_project_first(dev, Fo):
    """``_GcnConvFn``: the dot runs at F_out, against the recomputed xW"""
    _case(dev, "gcn", 3000, 60_000, 320, Fo, seed=40 + Fo, hubs=32, loops=50)


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,kw", [("sage", {}), ("concat", {}), ("gcn", {}), ("gcn", {"improved": True}), ("gcn", {"normalize": False})],
                         ids=["sage", "concat", "gcn", "gcn-improved", "gcn-plain"])
def test_hub_row_with_more_than_half_of_the_entries(dev, layer, kw):
    """one target holds 80 % of the 70k edges: 56k of the 73k entries (loops included) are one row, cut over many items"""
    _case(dev, layer, 3000, 70_000, 64, 64, seed=50, hubs=1, loops=20, hub_share=0.8, **kw)


@pytest.mark.parametrize("layer,kw", [("sage", {}), ("concat", {}), ("gcn", {}), ("gcn", {"normalize": False})],
                         ids=["sage", "concat", "gcn", "gcn-plain"])
def test_no_edges(dev, layer, kw):
    got = _case(dev, layer, 100, 0, 16, 16, seed=60, **kw)
    assert got[4].shape == (0,)


@pytest.mark.parametrize("layer,kw", [("sage", {}), ("gcn", {}), ("gcn", {"improved": True})], ids=["sage", "gcn-fill1", "gcn-fill2"])
def test_existing_self_loops(dev, layer, kw):
    """every third node has one existing self loop (at most one per node): its weight is the loop entry's, its gradient that
    entry's; the other nodes' loops carry the constant fill (1, or 2 under ``improved``)"""
    N = 900
    ei = _edges(N, 8000, 70, loops=300)
    x, W, b, ew, go = _inputs(N, ei, 32, 48, 71)
    got = _run(layer, dev, x, ei.to(dev), W, b, ew, go, **kw)
    ref = _reference(layer, x, ei, W, b, ew, go, **kw)
    _compare(got, ref, f"{layer} self loops {kw}")
    loop = ei[0] == ei[1]
    assert int(loop.sum()) == 300 and rel_max(got[4][loop.to(dev)], ref[4][loop]) <= GRAD_REL


@pytest.mark.parametrize("layer,kw", [("sage", {}), ("concat", {}), ("gcn", {}), ("gcn", {"normalize": False})],
                         ids=["sage", "concat", "gcn", "gcn-plain"])
def test_padding_columns_get_zero(dev, layer, kw):
    N = 2000
    ei = _edges(N, 30_000, 80, loops=10, pad=500)
    x, W, b, ew, go = _inputs(N, ei, 64, 64, 81, concat=layer == "concat")
    got = _run(layer, dev, x, ei.to(dev), W, b, ew, go, **kw)
    _compare(got, _reference(layer, x, ei, W, b, ew, go, **kw), f"{layer} padding")
    assert float(got[4][(ei[0] < 0).to(dev)].abs().max()) == 0.0


@pytest.mark.parametrize("layer,kw", [("sage", {}), ("concat", {}), ("gcn", {}), ("gcn", {"normalize": False})],
                         ids=["sage", "concat", "gcn", "gcn-plain"])
def test_prebuilt_graph(dev, layer, kw):
    _case(dev, layer, 3000, 60_000, 64, 64, seed=90, hubs=32, loops=50, prebuilt=True, **kw)


def test_a_graph_of_256_entry_items(dev):
    """``CSRGraph(item=256)`` (what graphs above 2^22 entries get) and more entries than one item"""
    N, E = 3000, 60_000
    ei = _edges(N, E, 100, hubs=8, loops=50)
    x, W, b, ew, go = _inputs(N, ei, 256, 256, 101)
    for layer in ("sage", "gcn"):
        graph = npi.CSRGraph(ei.to(dev), N, item=256)
        assert graph.by_dst.item == 256 and graph.by_dst.nnz_max > 256
        got = _run(layer, dev, x, graph, W, b, ew, go)
        _compare(got, _reference(layer, x, ei, W, b, ew, go), f"{layer} item=256")


# ---- modules ------------------------------------------------------------------------------------------------------------------------
def _module_case(dev, conv, ref_layer, N, ei, Fi, through_batch=False, **ref_kw):
    x, _, _, ew, go = _inputs(N, ei, Fi, conv.weight.size(1), 111)
    conv = conv.to(dev)
    xd, wd = x.to(dev).requires_grad_(True), ew.to(dev).requires_grad_(True)
    if through_batch:
        gb = npi.GraphBatch(xd, ei.to(dev), torch.zeros(N, dtype=torch.long, device=dev))
        out = conv(gb, edge_weight=wd).x
    else:
        out = conv(xd, ei.to(dev), edge_weight=wd)
    out.backward(go.to(dev))
    ref = _reference(ref_layer, x, ei, conv.weight, conv.bias, ew, go, **ref_kw)
    _compare((out.detach(), xd.grad, conv.weight.grad, conv.bias.grad, wd.grad), ref, f"{type(conv).__name__} batch={through_batch}")


@pytest.mark.parametrize("through_batch", [False, True], ids=["tensor", "GraphBatch"])
def test_through_the_modules(dev, through_batch):
    N = 2500
    ei = _edges(N, 40_000, 110, hubs=16, loops=30)
    torch.manual_seed(5)
    _module_case(dev, npi.SAGEConv(64, 96), "sage", N, ei, 64, through_batch)
    _module_case(dev, npi.GCNConv(64, 96), "gcn", N, ei, 64, through_batch)
    _module_case(dev, npi.GCNConv(96, 32, improved=True), "gcn", N, ei, 96, through_batch, improved=True)
    _module_case(dev, npi.GCNConv(64, 96, normalize=False), "gcn", N, ei, 64, through_batch, normalize=False)
    _module_case(dev, npi.SAGEConv(64, 96, concat=True), "concat", N, ei, 64, through_batch)


def test_cached_gcn_refuses_a_differentiable_weight(dev):
    ei = _edges(50, 200, 120).to(dev)
    conv = npi.GCNConv(8, 8, cached=True).to(dev)
    with pytest.raises(ValueError, match="cached"):
        conv(torch.randn(50, 8, device=dev), ei, edge_weight=torch.rand(200, device=dev).requires_grad_(True))


# ---- fp16 x 2 projection, reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", ["sage", "gcn"])
def test_with_the_fp16x2_projection(dev, monkeypatch, layer):
    """20k nodes, 400k edges, 256 -> 256 under a schedule that takes the fp16 x 2 projection at this size: the forward GEMM ran
    on row scales (asserted), and the weight gradient -- dAgg from a GEMM of its own -- keeps the bar"""
    N, E, F = 20_000, 400_000, 256
    ei = _edges(N, E, 130, hubs=32, loops=50)
    x, W, b, ew, go = _inputs(N, ei, F, F, 131)
    calls = []
    real = NF.linear_fwd

    def spy(a, weight, *args, **kw):
        calls.append(kw.get("a_scales") is not None)
        return real(a, weight, *args, **kw)
    monkeypatch.setattr(NF, "linear_fwd", spy)
    got = _run(layer, dev, x, ei.to(dev), W, b, ew, go, schedule=DEFAULT.but(f16x2_min_rows=0))
    assert calls == [True], calls
    _compare(got, _reference(layer, x, ei, W, b, ew, go), f"{layer} fp16x2")


@pytest.mark.parametrize("layer,Fi,Fo,kw", [("sage", 256, 256, {}), ("concat", 64, 64, {}), ("gcn", 64, 128, {}), ("gcn", 178, 64, {}),
                                            ("gcn", 64, 64, {"normalize": False})],
                         ids=["sage", "concat", "gcn", "gcn-project-first", "gcn-plain"])
def test_two_runs_are_bit_identical(dev, layer, Fi, Fo, kw):
    N = 5000
    ei = _edges(N, 100_000, 140, hubs=32, loops=50, pad=11)
    x, W, b, ew, go = _inputs(N, ei, Fi, Fo, 141, concat=layer == "concat")
    first = _run(layer, dev, x, ei.to(dev), W, b, ew, go, **kw)[4]
    second = _run(layer, dev, x, ei.to(dev), W, b, ew, go, **kw)[4]
    assert torch.equal(first, second)


# ---- interface ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", ["sage", "gcn"])
def test_weight_views_keep_their_shape(dev, layer):
    """an ``[E, 1]`` view and a non-contiguous weight work in the forward (it flattens / copies them): so does the gradient, in
    the weight's own shape"""
    N, E = 1500, 20_000
    ei = _edges(N, E, 150, loops=10)
    x, W, b, ew, go = _inputs(N, ei, 32, 32, 151)
    flat = _run(layer, dev, x, ei.to(dev), W, b, ew, go)[4]
    col = _run(layer, dev, x, ei.to(dev), W, b, ew.view(-1, 1), go)[4]
    assert col.shape == (ew.numel(), 1) and torch.equal(col.view(-1), flat)
    wide = torch.stack([ew, torch.zeros_like(ew)], 1).to(dev).requires_grad_(True)         # [E', 2]: column 0 is not contiguous
    fn = npi.sage_conv if layer == "sage" else npi.gcn_conv
    out = fn(x.to(dev), ei.to(dev), W.to(dev), b.to(dev), edge_weight=wide[:, 0])
    out.backward(go.to(dev))
    assert wide.grad.shape == wide.shape and torch.equal(wide.grad[:, 0], flat) and float(wide.grad[:, 1].abs().max()) == 0.0


@pytest.mark.parametrize("layer,Fi,Fo", [("sage", 256, 256), ("sage", 178, 64), ("concat", 64, 64), ("gcn", 64, 128), ("gcn", 178, 64)])
def test_constant_weight_path_is_untouched(dev, layer, Fi, Fo):
    """``requires_grad=False``: out, dX, dW bit-identical to the call with ``edge_weight.detach()`` of a weight that does"""
    N = 5000
    ei = _edges(N, 100_000, 160, hubs=32, loops=50)
    x, W, b, ew, go = _inputs(N, ei, Fi, Fo, 161, concat=layer == "concat")
    fn = npi.gcn_conv if layer == "gcn" else npi.sage_conv
    kw = {"concat": True} if layer == "concat" else {}
    res = []
    for w in (ew.to(dev), ew.to(dev).requires_grad_(True).detach(), ew.to(dev).requires_grad_(True)):
        xd, Wd, bd = (t.to(dev).clone().requires_grad_(True) for t in (x, W, b))
        out = fn(xd, ei.to(dev), Wd, bd, edge_weight=w, **kw)
        out.backward(go.to(dev))
        res.append((out.detach(), xd.grad, Wd.grad, bd.grad))
    for k in range(4):
        assert torch.equal(res[0][k], res[1][k])
        assert torch.equal(res[0][k], res[2][k])          # and asking for the weight gradient changes none of the others


def test_precomputed_norm_with_a_differentiable_weight_is_refused(dev):
    N = 100
    ei = _edges(N, 500, 170).to(dev)
    graph = npi.CSRGraph(ei, N)
    w = torch.rand(500, device=dev)
    norm = NF.GCNNorm(graph, w)
    x, W = torch.randn(N, 8, device=dev), torch.randn(8, 8, device=dev)
    npi.gcn_conv(x, graph, W, norm=norm, edge_weight=w)                                        # constants: as before
    with pytest.raises(ValueError, match="norm="):
        npi.gcn_conv(x, graph, W, norm=norm, edge_weight=w.clone().requires_grad_(True))


@pytest.mark.parametrize("layer", ["sage", "gcn"])
def test_bf16_features_with_a_differentiable_weight_are_refused(dev, layer):
    N = 100
    ei = _edges(N, 500, 180).to(dev)
    x, W = torch.randn(N, 128, device=dev).bfloat16(), torch.randn(128, 128, device=dev).bfloat16()
    fn = npi.sage_conv if layer == "sage" else npi.gcn_conv
    with pytest.raises(NotImplementedError, match="edge_weight"):
        fn(x, ei, W, edge_weight=torch.rand(500, device=dev).requires_grad_(True))


# ---- C4 at full size ---------------------------------------------------------------------------------------------------------------
def test_c4_sage_closed_form_in_fp64(dev):
    """N = 1M, E = 20M, 256 -> 256, SAGEConv.  The host cannot hold fp64 autograd over 20M gathered rows, so the closed form
    ``g_e = <dAgg[i, :], x[j, :]> / cnt[i]``, ``dAgg = dOut W^T`` is evaluated in fp64 on the host for 100 000 random edges and
    for every entry of the 8 heaviest target rows; the bar is the same GRAD_REL on each of the two sets."""
    N, E, F = 1_000_000, 20_000_000, 256
    ei = bipartite_edge_index(N, E, seed=20260310)
    assert not bool((ei[0] == ei[1]).any())
    g = torch.Generator().manual_seed(3)
    W = torch.randn(F, F, generator=g) / 16
    b = torch.randn(F, generator=g)
    x = torch.randn(N, F, generator=g)
    go = torch.randn(N, F, generator=g)
    ew = torch.rand(E, generator=g) + 0.5
    graph = npi.CSRGraph(ei.to(dev), N)
    wd = ew.to(dev).requires_grad_(True)
    xd, Wd, bd = (t.to(dev).requires_grad_(True) for t in (x, W, b))
    out = npi.sage_conv(xd, graph, Wd, bd, edge_weight=wd)
    out.backward(go.to(dev))
    got = wd.grad.cpu().double()
    assert got.shape == (E,)
    del out, xd, graph
    torch.cuda.empty_cache()
    cnt = (torch.bincount(ei[1], minlength=N) + 1).double()
    W6 = W.double()

    def closed_form(idx):
        res = torch.empty(idx.numel(), dtype=torch.float64)
        for k in range(0, idx.numel(), 50_000):
            e = idx[k:k + 50_000]
            i, j = ei[1][e], ei[0][e]
            dagg = go[i].double() @ W6.t()
            res[k:k + 50_000] = (dagg * x[j].double()).sum(1) / cnt[i]
        return res

    sample = torch.randperm(E, generator=g)[:100_000]
    truth = closed_form(sample)
    err = float((got[sample] - truth).abs().max() / truth.abs().max())
    print(f"C4 d edge_weight, 100k random edges: rel_max {err:.3e} (max |ref| {float(truth.abs().max()):.3g})")
    assert err <= GRAD_REL, err
    deg = torch.bincount(ei[1], minlength=N)
    worst = 0.0
    for row in torch.topk(deg, 8).indices.tolist():
        idx = (ei[1] == row).nonzero().view(-1)
        truth = closed_form(idx)
        e_row = float((got[idx] - truth).abs().max() / truth.abs().max())
        print(f"C4 d edge_weight, row {row} ({idx.numel()} entries): rel_max {e_row:.3e}")
        worst = max(worst, e_row)
    assert worst <= GRAD_REL, worst
