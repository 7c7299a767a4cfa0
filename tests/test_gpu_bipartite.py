"""The bipartite ``(x_src, x_dst)`` / ``size=`` form of SAGEConv and GATConv on the GPU, every case against the fp64 restatement
``tests/_bipartite_ref.py`` (pinned to the oracle by ``tests/test_bipartite_cpu.py``).

Bars, taken from the existing suite: out, dX_src, dX_dst 1e-4 per row scale (``tests/test_gpu_hub_stream.py::_row_scaled``; 1e-5
against fp64 on the heaviest rows of the streamed sides), dW / db / d att ``GRAD_REL`` (``tests/_util.py``), d edge_weight
``GRAD_REL`` by ``rel_max`` (``tests/test_gpu_edge_weight_grad.py``)."""
import ctypes

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import functional as NF
from npi_gnn_amd import graph as G
from npi_gnn_amd._lib import NPI_HUB_MAX
from _util import GRAD_REL, rel_max
import _bipartite_ref as ref

pytestmark = pytest.mark.gpu


def _row_scaled(got, ref_):
    got, ref_ = got.detach().double().cpu(), ref_.detach().double().cpu()
    return float(((got - ref_).abs() / (1.0 + ref_.abs().amax(1, keepdim=True))).max())


def _edges(n_src, n_dst, e, seed, heavy=None, empty_from=None):
    """random edges src -> dst with duplicates, some (k, k) columns, one heavy target, empty targets from ``empty_from`` on,
    and (-1, -1) padding at the end"""
    g = torch.Generator().manual_seed(seed)
    hi = n_dst if empty_from is None else empty_from
    ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, hi, (e,), generator=g)])
    parts = [ei, ei[:, :50]]                                                        # duplicates
    k = torch.arange(min(n_src, hi, 40))
    parts.append(torch.stack([k, k]))                                              # (k, k): ordinary edges
    if heavy is not None:
        t, deg = heavy
        parts.append(torch.stack([torch.randint(0, n_src, (deg,), generator=g), torch.full((deg,), t)]))
    parts.append(torch.full((2, 7), -1))
    ei = torch.cat(parts, 1)
    return ei


RELU_MARGIN = 1e-4


def _away_from_the_kink(go, pre):
    """``relu=True`` against an fp64 reference: the derivative of the ReLU jumps at 0, so where the fp64 pre-activation lies within
    f32 rounding of 0 the f32 layer may legitimately take the other branch, and the whole of dOut[i, c] (not a rounding error's
    worth) moves between the two gradients -- among the ~10^5..10^6 outputs of a case a few such elements are to be expected.
    The upstream gradient is therefore set to ZERO at the elements with ``|pre| < RELU_MARGIN`` (1e-4: a hundred times the f32
    error of a pre-activation of size 1, a 1e-4 share of the elements), for the reference and the layer alike; every other
    element is held to the unchanged bars."""
    go = go.clone()
    go[pre.detach().abs() < RELU_MARGIN] = 0.0
    return go


def _leaves(dev, *ts):
    return [None if t is None else t.to(dev).float().requires_grad_(True) for t in ts]


def _check(got, want, names, bars):
    for g_, w_, name, bar in zip(got, want, names, bars):
        if w_ is None:
            assert g_ is None, name
            continue
        err = _row_scaled(g_, w_) if bar == "row" else rel_max(g_, w_)
        print(f"   {name}: {err:.2e}")
        assert err < (1e-4 if bar == "row" else GRAD_REL), (name, err)


# ---- SAGEConv ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,n_dst", [(3001, 517), (517, 3001)])
@pytest.mark.parametrize("F", [1, 64, 178, 256])
def test_sage_rectangular(dev, n_src, n_dst, F):
    Fo = 128
    g = torch.Generator().manual_seed(F + n_src)
    ei = _edges(n_src, n_dst, 9000, seed=F, heavy=(3, 4000), empty_from=n_dst - 20)
    x_src = torch.randn(n_src, F, generator=g).double()
    x_dst = torch.randn(n_dst, F, generator=g).double()
    W = (torch.randn(F, Fo, generator=g) / max(F, 4) ** 0.5).double()
    b = torch.randn(Fo, generator=g).double()
    go = torch.randn(n_dst, Fo, generator=g).double()
    ew = (torch.rand(ei.size(1), generator=g) + 0.5).double()
    eid = ei.to(dev)
    variants = [dict(bias=True), dict(bias=False, x_dst=True), dict(bias=True, normalize=True), dict(bias=True, relu=True),
                dict(bias=True, ew="const"), dict(bias=True, ew="grad", relu=True), dict(bias=True, prebuilt=True)]
    for v in variants:
        print(f"sage {n_src}x{n_dst} F={F} {v}")
        bias = b if v.get("bias") else None
        xr, Wr = x_src.clone().requires_grad_(True), W.clone().requires_grad_(True)
        br = bias.clone().requires_grad_(True) if bias is not None else None
        er = ew.clone().requires_grad_(v.get("ew") == "grad") if v.get("ew") else None
        go_v = go
        if v.get("relu"):
            go_v = _away_from_the_kink(go, ref.sage_bipartite(x_src, ei, W, bias, n_dst=n_dst, edge_weight=er))
        want = ref.sage_bipartite(xr, ei, Wr, br, n_dst=n_dst, edge_weight=er, normalize=v.get("normalize", False), relu=v.get("relu", False))
        want.backward(go_v)
        conv = npi.SAGEConv(F, Fo, normalize=v.get("normalize", False), bias=bias is not None).to(dev)
        with torch.no_grad():
            conv.weight.copy_(W)
            if bias is not None:
                conv.bias.copy_(b)
        xg, xdg = _leaves(dev, x_src, x_dst if v.get("x_dst") else None)
        eg = None
        if v.get("ew"):
            eg = ew.float().to(dev).requires_grad_(v["ew"] == "grad")
        graph = npi.BipartiteGraph(eid, (n_src, n_dst)) if v.get("prebuilt") else eid
        # (N_dst: from x_dst, from size, or -- neither given -- from the prebuilt graph)
        out = conv((xg, xdg), graph, eg, None if (xdg is not None or v.get("prebuilt")) else (n_src, n_dst), relu=v.get("relu", False))
        assert tuple(out.shape) == (n_dst, Fo)
        out.backward(go_v.float().to(dev))
        _check([out, xg.grad, conv.weight.grad, conv.bias.grad if bias is not None else None],
               [want, xr.grad, Wr.grad, br.grad if br is not None else None], ["out", "dX_src", "dW", "db"], ["row", "row", "rel", "rel"])
        if xdg is not None:
            assert xdg.grad is None                                                 # x_dst is not read
        if v.get("ew") == "grad":
            pad = ei[0] < 0
            err = rel_max(eg.grad, er.grad)
            print(f"   d edge_weight: {err:.2e}")
            assert err < GRAD_REL and float(eg.grad[pad.to(dev)].abs().max()) == 0.0
        if bias is not None and not v.get("normalize") and not v.get("relu"):
            assert torch.equal(out[n_dst - 20:].detach(), conv.bias.detach().expand(20, Fo))      # empty targets: the bias
    npi.graph.check_pending()                                                        # padding is dropped silently


def test_out_of_range_edges_are_dropped_and_reported(dev):
    ei = torch.tensor([[0, 1, 9, 2], [0, 1, 1, 5]]).to(dev)                         # source 9 of 5, target 5 of 3
    conv = npi.SAGEConv(4, 4).to(dev)
    x = torch.randn(5, 4, device=dev)
    npi.graph.check_pending()
    out = conv((x, None), ei, size=(5, 3))
    with pytest.raises(IndexError):
        npi.graph.check_pending()
    want = ref.sage_bipartite(x.cpu().double(), ei.cpu(), conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double(), n_dst=3)
    assert _row_scaled(out, want) < 1e-4


@pytest.mark.parametrize("F", [64, 178])
@pytest.mark.parametrize("ids", ["perm", "dup", "bad"])
def test_sage_concat(dev, F, ids):
    n_src, n_dst, Fo = 2000, 700, 96
    g = torch.Generator().manual_seed(F)
    ei = _edges(n_src, n_dst, 6000, seed=11, heavy=(5, 2500), empty_from=n_dst - 10)
    res = torch.randperm(n_src, generator=g)[:n_dst] if ids == "perm" else torch.randint(0, 50, (n_dst,), generator=g)
    x = torch.randn(n_src, F, generator=g).double()
    W = (torch.randn(2 * F, Fo, generator=g) / F ** 0.5).double()
    b = torch.randn(Fo, generator=g).double()
    go = torch.randn(n_dst, Fo, generator=g).double()
    ew = (torch.rand(ei.size(1), generator=g) + 0.5).double()
    res_ref, x_ref = res, x
    if ids == "bad":
        res = res.clone()
        res[3] = n_src + 5                                                          # out of range: a ZERO root row, reported
        res_ref = res.clone()
        res_ref[3] = n_src
        x_ref = torch.cat([x, torch.zeros(1, F, dtype=torch.float64)])              # (the reference gathers an appended zero row)
    for use_ew in (False, True):
        xr, Wr, br = (t.clone().requires_grad_(True) for t in (x_ref, W, b))
        er = ew.clone().requires_grad_(True) if use_ew else None
        want = ref.sage_bipartite(xr, ei, Wr, br, n_dst=n_dst, res_n_id=res_ref, concat=True, edge_weight=er)
        want.backward(go)
        conv = npi.SAGEConv(F, Fo, concat=True).to(dev)
        with torch.no_grad():
            conv.weight.copy_(W)
            conv.bias.copy_(b)
        graph = npi.BipartiteGraph(ei.to(dev), (n_src, n_dst))
        res_d = res.to(dev)
        npi.graph.check_pending()
        grads = []
        for _ in range(2):
            conv.zero_grad()
            xg, = _leaves(dev, x)
            eg = ew.float().to(dev).requires_grad_(True) if use_ew else None
            out = conv((xg, None), graph, eg, (n_src, n_dst), res_d)
            out.backward(go.float().to(dev))
            grads.append((out.detach().clone(), xg.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()))
        for a, c in zip(*grads):
            assert torch.equal(a, c)                                                # two runs: the same bits
        out, dx, dw, db = grads[0]
        print(f"concat F={F} {ids} ew={use_ew}")
        _check([out, dx, dw, db], [want, xr.grad[:n_src], Wr.grad, br.grad], ["out", "dX_src", "dW", "db"], ["row", "row", "rel", "rel"])
        if use_ew:
            assert rel_max(eg.grad, er.grad) < GRAD_REL
        if ids == "bad":
            with pytest.raises(IndexError):
                npi.graph.check_pending()
        else:
            npi.graph.check_pending()


# ---- npi_rows_gather through ctypes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F", [256, 64, 178, 3, 1])
def test_rows_gather_bit_exact(dev, dtype, F):
    lib = _lib.load()
    n_src, n = 1237, 2001
    g = torch.Generator().manual_seed(F)
    x = torch.randn(n_src, F, generator=g).to(dev).to(dtype)
    idx = torch.randint(0, n_src, (n,), generator=g).to(dev)
    code = _lib.NPI_BF16 if dtype == torch.bfloat16 else _lib.NPI_F32
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    s = _lib.stream_ptr(x.device)
    for off in (0, F, 1):                                                           # left half, right half, an unaligned column block
        buf = torch.full((n, 2 * F + 8), 7.0, dtype=dtype, device=dev)            # (a 16-byte pitch: off 0 / F aligned when F is)
        out = buf[:, off:off + F]
        assert lib.npi_rows_gather(x.data_ptr(), x.stride(0), n_src, idx.data_ptr(), n, F, out.data_ptr(), buf.stride(0), code,
                                   st.data_ptr(), s) == 0
        assert torch.equal(out, x.index_select(0, idx))
        rest = torch.ones(2 * F + 8, dtype=torch.bool)
        rest[off:off + F] = False
        assert bool((buf[:, rest.to(dev)] == 7.0).all())                            # nothing outside the block was written
    # idx == NULL: the identity, from a pitched source
    wide = torch.randn(n_src, F + 8, generator=g).to(dev).to(dtype)
    out = torch.empty(n_src, F, dtype=dtype, device=dev)
    assert lib.npi_rows_gather(wide.data_ptr(), wide.stride(0), n_src, None, n_src, F, out.data_ptr(), F, code, st.data_ptr(), s) == 0
    assert torch.equal(out, wide[:, :F])
    assert int(st.item()) == 0
    # an id out of range: a zero row, the status bit, the other rows as before
    bad = idx.clone()
    bad[5], bad[77] = n_src, -1
    out = torch.full((n, F), 7.0, dtype=dtype, device=dev)
    assert lib.npi_rows_gather(x.data_ptr(), x.stride(0), n_src, bad.data_ptr(), n, F, out.data_ptr(), F, code, st.data_ptr(), s) == 0
    want = x.index_select(0, idx)
    want[5], want[77] = 0, 0
    assert torch.equal(out, want) and int(st.item()) == _lib.NPI_STATUS_BAD_ROW_ID
    # the wrapper
    out = torch.empty(n, F, dtype=dtype, device=dev)
    assert torch.equal(NF.rows_gather(x, idx, out), x.index_select(0, idx))


# ---- rectangular hub streaming, item sizes ----------------------------------------------------------------------------------------------
def _hub_edges(n_big, n_small, seed):
    """big table of n_big sources, n_small targets with Zipf in-degrees on the first 48 of them (distinct sources per heavy target)"""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k in range(48):
        deg = int(150_000 / (k + 1) ** 0.7)
        parts.append(torch.stack([torch.randperm(n_big, generator=g)[:deg], torch.full((deg,), k)]))
    parts.append(torch.stack([torch.randint(0, n_big, (1_000_000,), generator=g), torch.randint(48, n_small - 100, (1_000_000,), generator=g)]))
    ei = torch.cat(parts, 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)]


@pytest.mark.parametrize("direction,item", [("fwd", 256), ("bwd", 64)])
def test_rectangular_hub_streaming(dev, direction, item):
    n_big, n_small, F = 300_000, 20_000, 256
    assert n_big >= G.HUB_MIN_COLS
    ei = _hub_edges(n_big, n_small, seed=21)
    assert ei.size(1) > (1 << 20)
    if direction == "bwd":
        ei = ei.flip(0)                                                             # the big id space is the TARGET side: the plan is by_src's
    size = (n_big, n_small) if direction == "fwd" else (n_small, n_big)
    n_src, n_dst = size
    graph = npi.BipartiteGraph(ei.to(dev), size, item=item)
    side = graph.by_dst if direction == "fwd" else graph.by_src
    other = graph.by_src if direction == "fwd" else graph.by_dst
    assert side.item == item and other.item == item and side.n_cols == n_big and side.n_rows == n_small
    plan = side.hub_plan()
    assert plan is not None and plan.H > 0
    assert other.hub_plan() is None                                                 # its table is the small one
    # the plan against numpy, as tests/test_gpu_hub_stream.py::test_plan_against_numpy
    rowptr, col = side.rowptr.cpu().numpy().astype(np.int64), side.col.cpu().numpy().astype(np.int64)
    deg = rowptr[1:] - rowptr[:-1]
    min_degree = max(-(-n_big // G.HUB_DEGREE_DIV), 2)
    cand = np.flatnonzero(deg >= min_degree)
    want = cand[np.lexsort((cand, -deg[cand]))][:NPI_HUB_MAX]
    hub_rows = plan.hub_rows.cpu().numpy()
    assert plan.H == len(want) and np.array_equal(hub_rows[: plan.H], want) and (hub_rows[plan.H:] == -1).all()
    assert plan.n_entries == int(deg[want].sum()) and plan.n_entries >= G.HUB_ENTRIES_PER_STREAMED_ROW * n_big
    mask = np.zeros((n_big, NPI_HUB_MAX // 32), dtype=np.uint32)
    for j, r in enumerate(want):
        mask[col[rowptr[r]:rowptr[r + 1]], j // 32] |= np.uint32(1 << (j % 32))
    assert np.array_equal(plan.mask.cpu().numpy().view(np.uint32), mask)
    ldeg = deg.copy()
    ldeg[want] = 0
    assert np.array_equal(plan.light.rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(ldeg)]))
    # the layer through both paths
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n_src, F, generator=g).to(dev)
    W = (torch.randn(F, F, generator=g) / 16).to(dev)
    b = torch.randn(F, generator=g).to(dev)
    go = torch.randn(n_dst, F, generator=g).to(dev)
    res = {}
    for key, on in (("hub", True), ("hub2", True), ("plain", False)):
        graph.hub_stream = on
        xg, Wg, bg = (t.clone().requires_grad_(True) for t in (x, W, b))
        out = npi.sage_conv_bipartite((xg, None), graph, Wg, bg, size=size)
        out.backward(go)
        res[key] = (out.detach(), xg.grad, Wg.grad, bg.grad)
    for a, c in zip(res["hub"], res["hub2"]):
        assert torch.equal(a, c)                                                    # two launches: the same bits
    out, dx, dw, db = res["hub"]
    e_out, e_dx = _row_scaled(out, res["plain"][0]), _row_scaled(dx, res["plain"][1])
    e_dw, e_db = rel_max(dw, res["plain"][2]), rel_max(db, res["plain"][3])
    print(f"{direction}: hub vs plain  out {e_out:.2e}  dX {e_dx:.2e}  dW {e_dw:.2e}  db {e_db:.2e}")
    assert e_out < 1e-4 and e_dx < 1e-4 and e_dw < GRAD_REL and e_db < GRAD_REL
    # fp64 on the heaviest rows, by their formulas
    d, t = graph.by_dst, graph.by_src
    cnt = (d.rowptr[1:] - d.rowptr[:-1]).double().clamp(min=1)
    worst = 0.0
    if direction == "fwd":
        for i in plan.hub_rows[:8].tolist():
            nb = d.col[int(d.rowptr[i]):int(d.rowptr[i + 1])].long()
            truth = (x[nb].double().sum(0) / cnt[i]) @ W.double() + b.double()
            worst = max(worst, float((out[i].double() - truth).abs().max() / truth.abs().max()))
    else:
        dagg = go.double() @ W.double().t()
        for j in plan.hub_rows[:8].tolist():
            nb = t.col[int(t.rowptr[j]):int(t.rowptr[j + 1])].long()
            truth = (dagg[nb] / cnt[nb, None]).sum(0)
            worst = max(worst, float((dx[j].double() - truth).abs().max() / truth.abs().max()))
    print(f"{direction}: heaviest rows against fp64 {worst:.2e}")
    assert worst < 1e-5
    # dW and db against fp64 segment sums
    nnz = int(d.rowptr[-1])
    agg64 = torch.zeros(n_dst, F, dtype=torch.float64, device=dev)
    agg64.index_add_(0, d.rowidx[:nnz].long(), x[d.col[:nnz].long()].double())
    agg64 /= cnt[:, None]
    assert rel_max(dw, agg64.t() @ go.double()) < GRAD_REL and rel_max(db, go.double().sum(0)) < GRAD_REL
    assert _row_scaled(out, agg64 @ W.double() + b.double()) < 1e-4
    # a captured replay of the streamed aggregation equals the eager launch
    graph.hub_stream = True
    tab = x if direction == "fwd" else go
    o_cap = torch.empty(side.n_rows, F, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        NF.segsum(graph, side, tab, mean=True, out=o_cap, hub=plan)
    torch.cuda.current_stream(dev).wait_stream(stream)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        NF.segsum(graph, side, tab, mean=True, out=o_cap, hub=plan)
    o_eager = torch.empty(side.n_rows, F, device=dev)
    NF.segsum(graph, side, tab, mean=True, out=o_eager, hub=plan)
    o_cap.zero_()
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(o_cap, o_eager)
    assert _row_scaled(o_eager, NF.segsum(graph, side, tab, mean=True)) < 1e-5


# ---- GATConv ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,concat", [(1, True), (4, True), (4, False)])
@pytest.mark.parametrize("with_dst", [True, False])
def test_gat_rectangular(dev, heads, concat, with_dst):
    n_src, n_dst, Fin, C = 1500, 400, 48, 32
    g = torch.Generator().manual_seed(heads * 7 + with_dst)
    ei = _edges(n_src, n_dst, 5000, seed=5, heavy=(2, 1200), empty_from=n_dst - 15)
    x_src = torch.randn(n_src, Fin, generator=g).double()
    x_dst = torch.randn(n_dst, Fin, generator=g).double() if with_dst else None
    W = (torch.randn(Fin, heads * C, generator=g) / Fin ** 0.5).double()
    att = (torch.randn(1, heads, 2 * C, generator=g) / C ** 0.5).double()
    b = torch.randn(heads * C if concat else C, generator=g).double()
    go = torch.randn(n_dst, heads * C if concat else C, generator=g).double()
    for relu in (False, True):
        print(f"gat H={heads} concat={concat} x_dst={with_dst} relu={relu}")
        xr, Wr, ar, br = (t.clone().requires_grad_(True) for t in (x_src, W, att, b))
        xdr = x_dst.clone().requires_grad_(True) if with_dst else None
        go_v = go
        if relu:
            go_v = _away_from_the_kink(go, ref.gat_bipartite(x_src, x_dst, ei, W, att, b, n_dst=n_dst, heads=heads, concat=concat))
        want = ref.gat_bipartite(xr, xdr, ei, Wr, ar, br, n_dst=n_dst, heads=heads, concat=concat, relu=relu)
        want.backward(go_v)
        conv = npi.GATConv(Fin, C, heads=heads, concat=concat, dropout=0.3).to(dev).eval()       # eval(): dropout is the identity
        with torch.no_grad():
            conv.weight.copy_(W)
            conv.att.copy_(att)
            conv.bias.copy_(b)
        xg, xdg = _leaves(dev, x_src, x_dst)
        out = conv((xg, xdg), ei.to(dev), None if with_dst else (n_src, n_dst), relu=relu)
        out.backward(go_v.float().to(dev))
        _check([out, xg.grad, xdg.grad if with_dst else None, conv.weight.grad, conv.att.grad, conv.bias.grad],
               [want, xr.grad, xdr.grad if with_dst else None, Wr.grad, ar.grad, br.grad],
               ["out", "dX_src", "dX_dst", "dW", "d att", "db"], ["row", "row", "row", "rel", "rel", "rel"])
        if not with_dst:
            assert float(conv.att.grad[..., :C].abs().max()) == 0.0                 # no target term: a zero gradient
        if not relu:
            assert _row_scaled(out[n_dst - 15:], b.expand(15, -1)) < 1e-6           # empty targets: the bias
        conv.train()
        with pytest.raises(NotImplementedError, match="dropout"):
            conv((xg, xdg), ei.to(dev), None if with_dst else (n_src, n_dst))


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_tensor_with_size_is_the_pair_form(dev, heads):
    n, Fin, C = 900, 32, 16
    g = torch.Generator().manual_seed(heads)
    ei = _edges(n, n, 4000, seed=8)
    x = torch.randn(n, Fin, generator=g).double()
    conv = npi.GATConv(Fin, C, heads=heads).to(dev)
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
    W, att, b = (t.detach().cpu().double().requires_grad_(True) for t in (conv.weight, conv.att, conv.bias))
    xr = x.clone().requires_grad_(True)
    go = torch.randn(n, heads * C, generator=g).double()
    want = ref.gat_bipartite(xr, xr, ei, W, att, b, heads=heads)
    want.backward(go)
    res = []
    for form in ("size", "pair", "graph"):
        conv.zero_grad()
        xg, = _leaves(dev, x)
        if form == "size":
            out = conv(xg, ei.to(dev), size=(n, n))
        elif form == "pair":
            out = conv((xg, xg), ei.to(dev))
        else:
            out = conv(xg, npi.BipartiteGraph(ei.to(dev), (n, n)), size=(n, n))
        out.backward(go.float().to(dev))
        _check([out, xg.grad, conv.weight.grad, conv.att.grad, conv.bias.grad], [want, xr.grad, W.grad, att.grad, b.grad],
               ["out", "dX", "dW", "d att", "db"], ["row", "row", "rel", "rel", "rel"])
        res.append((out.detach().clone(), xg.grad.clone(), conv.weight.grad.clone()))
    for a, c in zip(res[0], res[1]):
        assert torch.equal(a, c)


# ---- the square paths are untouched -------------------------------------------------------------------------------------------------
def test_square_calls_keep_their_bits(dev):
    n, F = 2000, 64
    g = torch.Generator().manual_seed(0)
    ei = torch.randint(0, n, (2, 12000), generator=g).to(dev)
    x = torch.randn(n, F, generator=g).to(dev)
    go = torch.randn(n, 32, generator=g).to(dev)
    sage, gat = npi.SAGEConv(F, 32).to(dev), npi.GATConv(F, 32).to(dev)

    def run(conv, **kw):
        conv.zero_grad()
        xg = x.clone().requires_grad_(True)
        out = conv(xg, ei, **kw)
        out.backward(go)
        return out.detach().clone(), xg.grad.clone(), conv.weight.grad.clone()
    a, c = run(sage), run(sage, size=(n, n))
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    a, c = run(sage), run(sage, size=None)
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    a, c = run(gat), run(gat, size=None)
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    graph = npi.CSRGraph(ei, n)
    with pytest.raises(TypeError):
        sage((x, x), graph)
    with pytest.raises(TypeError):
        gat((x, x), graph)


# ---- square and rectangular layers are one code path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["64to32", "256-f16x2-overlap", "256-f16x2-overlap-edge-weight"])
@pytest.mark.parametrize("relu", [False, True])
def test_square_graph_and_pair_form_give_the_same_bits(dev, case, relu):
    """``sage_conv`` over the edge list as it is (``CSRGraph(self_loops=False, keep_equal=True)``) and ``sage_conv_bipartite`` over
    the same list with ``size = (n, n)`` run one function (``functional._AggProjectFn``) over the same two sorted sides.  The square
    call may take the whole-layer entry points (the 64 -> 32 case does), which the pair form never takes; those issue the same
    launches as the per-op calls, and every kernel is deterministic -- so out, dX, dW and db are the same bits.  The 256 -> 256
    cases run the fp16 x 2 forward, the aggregate-first backward and the two-stream fork."""
    n, E = 2000, 12000
    Fi, Fo = (64, 32) if case == "64to32" else (256, 256)
    sch = npi.Schedule() if case == "64to32" else npi.Schedule(f16x2_min_rows=128, overlap_min_rows=0)
    g = torch.Generator().manual_seed(17)
    ei = torch.randint(0, n, (2, E), generator=g).to(dev)
    x = torch.randn(n, Fi, generator=g).to(dev)
    W = (torch.randn(Fi, Fo, generator=g) / Fi ** 0.5).to(dev)
    b = torch.randn(Fo, generator=g).to(dev)
    go = torch.randn(n, Fo, generator=g).to(dev)
    ew = (torch.rand(E, generator=g) + 0.5).to(dev) if case.endswith("edge-weight") else None
    res = []
    for form in ("square", "pair"):
        xg, Wg, bg = (t.clone().requires_grad_(True) for t in (x, W, b))
        if form == "square":
            out = npi.sage_conv(xg, npi.CSRGraph(ei, n, self_loops=False, keep_equal=True), Wg, bg, edge_weight=ew, relu=relu, schedule=sch)
        else:
            out = npi.sage_conv_bipartite((xg, None), npi.BipartiteGraph(ei, (n, n)), Wg, bg, edge_weight=ew, relu=relu, schedule=sch)
        out.backward(go)
        res.append((out.detach(), xg.grad, Wg.grad, bg.grad))
    for name, a, c in zip(("out", "dX", "dW", "db"), *res):
        print(f"   {case} relu={relu} {name}: max |diff| {float((a - c).abs().max()):.2e}")
        assert torch.equal(a, c), name
