"""Max aggregation on the GPU: ``npi.segmax`` (Rule X, ``include/npi_gnn.h``) bit for bit against the host reference on the stress
graph of ``_segmax_ref`` -- every build variant (self loops, item size, column order) gives the same bits --, its backward exact on
integer-valued inputs and at the project's bar on real ones, special values, pitched and misaligned views, ``SAGEConv(aggr="max")``
in all its forms against the fp64 composition, and one forward + backward under stream capture."""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG

import _segmax_ref as ref
from _util import GRAD_REL, rel_max

pytestmark = pytest.mark.gpu

N = ref.N_STRESS
VARIANTS = [(item, sort) for item in (64, 256) for sort in (False, True)]
WIDTHS = (1, 7, 64, 100, 256, 260, 516)
_GRAPHS = {}


def _graph(dev, self_loops, item, sort):
    k = (self_loops, item, sort)
    if k not in _GRAPHS:
        _GRAPHS[k] = npi.CSRGraph(ref.stress_edges().to(dev), N, self_loops=self_loops, item=item, sort_columns=sort)
        assert _GRAPHS[k].by_dst.item == item and _GRAPHS[k].by_src.item == item
    return _GRAPHS[k]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _fwd_bwd(g, x, dout):
    xg = x.clone().requires_grad_(True)
    out, arg = npi.segmax(g, xg)
    assert not arg.requires_grad and arg.dtype == torch.int32
    out.backward(dout)
    return out.detach(), arg, xg.grad


# ---- 1, 2: exact forward and backward on integer-valued tables -----------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("F", WIDTHS)
def test_forward_and_backward_are_exact_on_every_build_variant(dev, F, self_loops):
    x, dout, out_ref, arg_ref, dx64 = ref.stress_reference(F, self_loops)
    ei = ref.stress_edges()
    frac = ref.tied_fraction(x, ei[0].numpy(), ei[1].numpy(), N, self_loops)
    print(f"F={F} self_loops={self_loops}: tied maxima {frac:.3f}")
    assert frac >= 0.30                                            # the inputs really exercise the tie rule
    dx_ref = dx64.float()
    assert torch.equal(dx_ref.double(), dx64)                     # small integers: every sum is exact in f32, in any order
    xg, dg = x.to(dev), dout.to(dev)
    first = None
    for item, sort in VARIANTS:
        out, arg, dx = _fwd_bwd(_graph(dev, self_loops, item, sort), xg, dg)
        what = (F, self_loops, item, sort)
        assert torch.equal(_bits(out), _bits(out_ref)), what
        assert torch.equal(arg.cpu(), arg_ref), what
        assert torch.equal(_bits(dx), _bits(dx_ref)), what
        if first is None:
            first = (out, arg)
        assert torch.equal(_bits(out), _bits(first[0])) and torch.equal(arg, first[1]), what
    NG.check_pending()


# ---- 3: real-valued tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [7, 256, 260])
def test_backward_on_real_values_meets_the_bar_and_repeats_bitwise(dev, F):
    x, dout, out_ref, arg_ref, dx64 = ref.stress_reference(F, True, integer=False)
    xg, dg = x.to(dev), dout.to(dev)
    for item, sort in VARIANTS:
        g = _graph(dev, True, item, sort)
        out, arg, dx = _fwd_bwd(g, xg, dg)
        assert torch.equal(_bits(out), _bits(out_ref)) and torch.equal(arg.cpu(), arg_ref), (F, item, sort)
        err = rel_max(dx, dx64)
        print(f"F={F} item={item} sort_columns={sort}: rel_max(dX) = {err:.3e}")
        assert err <= GRAD_REL, (F, item, sort, err)
        again = _fwd_bwd(g, xg, dg)[2]
        assert torch.equal(_bits(dx), _bits(again)), (F, item, sort)
    NG.check_pending()


# ---- 4: special values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
def test_special_values_follow_the_rule(dev, self_loops):
    F = 8
    x = ref.randn_table(N, F, 31).clone()
    x[40, 0], x[41, 0], x[ref.HUB_SRC, 0] = float("nan"), -float("nan"), float("nan")       # NaNs in one column (the hub source: many rows)
    x[:, 1] = -0.0                                                 # every row's maximum is -0.0 -> +0.0
    x[:, 2] = -float("inf")
    x[:, 3] = torch.where(ref.randn_table(N, 1, 32)[:, 0] > 0, 0.0, -0.0)
    x[:, 4] = float("inf")
    x[::3, 4] = float("nan")
    ei = ref.stress_edges()
    dout = ref.int_table(N, F, -3, 3, 33)
    out_ref, arg_ref = ref.rule_x(x, ei[0].numpy(), ei[1].numpy(), N, self_loops)
    dx_ref = ref.rule_x_bwd(dout, arg_ref, ei[0].numpy(), N)
    assert bool(torch.isnan(out_ref[:, 0]).any()) and bool((_bits(out_ref)[torch.isnan(out_ref)] == 0x7FC00000).all())
    for r in ref.EMPTY_ROWS:                                       # no entry, or the loop alone
        assert bool((arg_ref[r] == (-1 if self_loops else -2)).all())
    for item, sort in VARIANTS:
        out, arg, dx = _fwd_bwd(_graph(dev, self_loops, item, sort), x.to(dev), dout.to(dev))
        assert torch.equal(_bits(out), _bits(out_ref)), (item, sort)
        assert torch.equal(arg.cpu(), arg_ref), (item, sort)
        assert torch.equal(dx.cpu().double(), dx_ref), (item, sort)       # the gradient goes to the rule's winner (integer sums: exact)
    NG.check_pending()


# ---- 5: views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [64, 100])
def test_pitched_and_misaligned_views(dev, F):
    x, dout, out_ref, arg_ref, dx64 = ref.stress_reference(F, True)
    g = _graph(dev, True, 64, False)
    dg = dout.to(dev)
    wide = torch.zeros((N, F + 12), device=dev).requires_grad_(True)
    flat = torch.zeros(N * F + 1, device=dev).requires_grad_(True)
    with torch.no_grad():
        wide[:, :F] = x.to(dev)
        flat[1:] = x.to(dev).reshape(-1)
    pitched = wide[:, :F]
    shifted = flat[1:].view(N, F)
    assert pitched.stride(0) == F + 12 and shifted.data_ptr() % 16 == 4             # the second one forces one float per lane
    for leaf, view, grad_of in ((wide, pitched, lambda t: t[:, :F]), (flat, shifted, lambda t: t[1:].view(N, F))):
        out, arg = npi.segmax(g, view)
        out.backward(dg[:, :F])
        assert torch.equal(_bits(out), _bits(out_ref)) and torch.equal(arg.cpu(), arg_ref)
        assert torch.equal(grad_of(leaf.grad).cpu().double(), dx64)
    # a pitched gradient as well
    xg = x.to(dev).requires_grad_(True)
    out, _ = npi.segmax(g, xg)
    dwide = torch.zeros((N, F + 4), device=dev)
    dwide[:, :F] = dg
    out.backward(dwide[:, :F])
    assert torch.equal(xg.grad.cpu().double(), dx64)
    NG.check_pending()


# ---- 6: the layer --------------------------------------------------------------------------------------------------------------
def _compose(x, ei, n_dst, self_loops, W, b, root=None, relu=False, normalize=False):
    """the reference composition in fp64 on the host (randn inputs: no ties, autograd's amax is the rule's)"""
    agg = ref.torch_amax(x, ei[0].numpy(), ei[1].numpy(), n_dst, self_loops)
    a = agg if root is None else torch.cat([root, agg], dim=1)
    out = a @ W + b
    if relu:
        out = torch.relu(out)
    return torch.nn.functional.normalize(out, p=2.0, dim=-1) if normalize else out


def _compare(dev, conv, call, x, ref_out, what):
    """``call(conv, x_on_device)`` against the fp64 composition ``ref_out(x64, W64, b64)``: out, dX, dW, db"""
    x64 = x.double().requires_grad_(True)
    W64, b64 = conv.weight.detach().cpu().double().requires_grad_(True), conv.bias.detach().cpu().double().requires_grad_(True)
    want = ref_out(x64, W64, b64)
    dout = ref.randn_table(want.size(0), want.size(1), 77)
    want.backward(dout.double())
    xg = x.to(dev).requires_grad_(True)
    conv.zero_grad()
    got = call(conv, xg)
    got.backward(dout.to(dev))
    for name, a, b in (("out", got, want), ("dX", xg.grad, x64.grad), ("dW", conv.weight.grad, W64.grad), ("db", conv.bias.grad, b64.grad)):
        err = rel_max(a, b)
        print(f"{what} {name}: rel_max = {err:.3e}")
        assert err <= GRAD_REL, (what, name, err)


@pytest.mark.parametrize("fin,fout", [(64, 32), (100, 48)])
def test_sage_conv_max_against_the_fp64_composition(dev, fin, fout):
    torch.manual_seed(fin)
    ei = ref.stress_edges()
    eig = ei.to(dev)
    x = ref.randn_table(N, fin, 5)
    conv = npi.SAGEConv(fin, fout, aggr="max").to(dev)
    _compare(dev, conv, lambda m, xg: m(xg, eig), x, lambda x64, W, b: _compose(x64, ei, N, True, W, b), "default")
    _compare(dev, conv, lambda m, xg: m(xg, npi.CSRGraph(eig, N)), x, lambda x64, W, b: _compose(x64, ei, N, True, W, b), "CSRGraph")
    _compare(dev, conv, lambda m, xg: m(xg, eig, relu=True), x, lambda x64, W, b: _compose(x64, ei, N, True, W, b, relu=True), "relu")
    _compare(dev, conv, lambda m, xg: m(npi.GraphBatch(xg, eig)).x, x, lambda x64, W, b: _compose(x64, ei, N, True, W, b), "GraphBatch")
    norm = npi.SAGEConv(fin, fout, normalize=True, aggr="max").to(dev)
    _compare(dev, norm, lambda m, xg: m(xg, eig), x, lambda x64, W, b: _compose(x64, ei, N, True, W, b, normalize=True), "normalize")
    cat = npi.SAGEConv(fin, fout, concat=True, aggr="max").to(dev)
    _compare(dev, cat, lambda m, xg: m(xg, eig), x, lambda x64, W, b: _compose(x64, ei, N, False, W, b, root=x64), "concat")
    # the pair form: 150 sources, 90 targets, a target without an in-edge, repeated roots
    g = torch.Generator().manual_seed(9)
    n_src, n_dst = 150, 90
    bei = torch.stack([torch.randint(0, n_src, (800,), generator=g), torch.randint(0, n_dst - 1, (800,), generator=g)])
    res = torch.randint(0, n_src, (n_dst,), generator=g)
    xs = ref.randn_table(n_src, fin, 6)
    beig, resg = bei.to(dev), res.to(dev)
    _compare(dev, conv, lambda m, xg: m((xg, None), beig, size=(n_src, n_dst)), xs,
             lambda x64, W, b: _compose(x64, bei, n_dst, False, W, b), "pair")
    _compare(dev, conv, lambda m, xg: m((xg, None), npi.BipartiteGraph(beig, (n_src, n_dst))), xs,
             lambda x64, W, b: _compose(x64, bei, n_dst, False, W, b), "pair, BipartiteGraph")
    _compare(dev, cat, lambda m, xg: m((xg, None), beig, size=(n_src, n_dst), res_n_id=resg), xs,
             lambda x64, W, b: _compose(x64, bei, n_dst, False, W, b, root=x64[res]), "pair, concat")
    NG.check_pending()


def test_sage_conv_max_is_not_the_mean_and_mean_is_unchanged(dev):
    """fails on a layer that swallows ``aggr``: the maximum over the stress graph is nowhere near the mean"""
    torch.manual_seed(3)
    eig = ref.stress_edges().to(dev)
    x = ref.randn_table(N, 64, 5).to(dev)
    plain, mean, mx = npi.SAGEConv(64, 32).to(dev), npi.SAGEConv(64, 32, aggr="mean").to(dev), npi.SAGEConv(64, 32, aggr="max").to(dev)
    mean.load_state_dict(plain.state_dict())
    mx.load_state_dict(plain.state_dict())
    a, b, c = plain(x, eig), mean(x, eig), mx(x, eig)
    assert torch.equal(_bits(a), _bits(b))
    assert rel_max(c, a) > 0.1
    agg, arg = npi.segmax(eig, x)                                  # the [2, E] tensor: self loops appended, as the layer does
    want = agg.double().cpu() @ mx.weight.detach().double().cpu() + mx.bias.detach().double().cpu()
    assert rel_max(c, want) <= GRAD_REL
    assert int(arg.min()) >= -1                                    # every row has its loop
    NG.check_pending()


# ---- 7: capture ----------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_under_capture(dev):
    """``segmax`` forward + backward inside ONE ``torch.cuda.graph`` on one stream (both sides built before), replayed with new x"""
    NG.check_pending()
    F = 100
    g = _graph(dev, True, 64, False)
    assert g.by_src is not None
    xs = [ref.randn_table(N, F, 40 + k).to(dev) for k in range(3)]
    dout = ref.randn_table(N, F, 50).to(dev)
    eager = [_fwd_bwd(g, x, dout) for x in xs]
    torch.cuda.synchronize()
    sx = xs[0].clone().requires_grad_(True)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        out, arg = npi.segmax(g, sx)
        (dx,) = torch.autograd.grad(out, sx, dout)
    for k in (1, 2):
        with torch.no_grad():
            sx.copy_(xs[k])
        out.detach().fill_(7.0)
        arg.fill_(7)
        dx.fill_(7.0)
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager[k][0])) and torch.equal(arg, eager[k][1]) and torch.equal(_bits(dx), _bits(eager[k][2])), k
    NG.check_pending()


# ---- edges of the interface ----------------------------------------------------------------------------------------------------
def test_empty_graphs_sides_and_shapes(dev):
    x = ref.randn_table(5, 6, 1).to(dev)
    none = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    out, arg = npi.segmax(npi.CSRGraph(none, 5, self_loops=False), x.clone().requires_grad_(True))      # no entry at all
    assert bool((out == 0).all()) and bool((arg == -2).all())
    out.sum().backward()
    out, arg = npi.segmax(none, x)                                 # the loops alone
    assert torch.equal(out, x) and bool((arg == -1).all())
    g = _graph(dev, False, 64, False)
    xs = ref.stress_reference(7, False)[0].to(dev)
    a = npi.segmax(g.by_dst, xs)                                   # one side: forward only
    b = npi.segmax(g, xs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="by-source"):
        npi.segmax(g.by_dst, xs.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="rows"):
        npi.segmax(g, xs[:100])
    NG.check_pending()
