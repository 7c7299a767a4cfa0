"""The fused readouts of Rule O on the MI355X -- global_add_pool, global_sort_pool, GlobalAttention -- against the torch reference
(tests/_readout_ref.py): every graph size around a wave and a chunk, every vector width through F, the pitch and the base alignment,
the invariances the rule promises, stream capture, and a Net_1-shaped model trained on each of them."""
import copy
import functools
import os

import pytest
import torch
import torch.nn.functional as F_

from npi_gnn_amd import graph as NG
from npi_gnn_amd import pool as NP

import _readout_ref as ref
from _util import GRAD_REL, rel_max

pytestmark = pytest.mark.gpu
C = ref.CHUNK
LAYOUTS = ["contiguous", "pitched", "misaligned"]
BIG = [0, 1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3, 0, 5000, 20000, 0]       # attention: long sums as well


def _place(x, layout, dev):
    """x on the device as itself, as a column block of a wider tensor (16-byte aligned base, another pitch), or as a view whose
    base is 4-byte but not 16-byte aligned"""
    n, F = x.shape
    if layout == "contiguous":
        return x.to(dev)
    lead, width = (4, F + 8) if layout == "pitched" else (1, F + 3)
    wide = torch.full((n, width), 7.0, device=dev)
    wide[:, lead:lead + F] = x.to(dev)
    view = wide[:, lead:lead + F]
    assert view.data_ptr() % 16 == (0 if layout == "pitched" else 4) and (n < 2 or view.stride(0) == width)
    return view


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@functools.lru_cache(maxsize=None)
def _add_case(F):
    gp = ref.graph_ptr(ref.SIZES, first=3)                     # three rows in front of the first graph, five behind the last
    N = int(gp[-1]) + 5
    xi, xr = ref.int_table(N, F, -8, 8, F), ref.randn_table(N, F, F + 1)
    dout = ref.randn_table(len(ref.SIZES), F, F + 2)
    return gp, xi, ref.add(xi, gp), xr, ref.add(xr.double(), gp), dout, ref.add_bwd(dout, gp, N)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F", ref.WIDTHS)
def test_add(dev, F, layout):
    gp, xi, want_i, xr, want_r, dout, want_dx = _add_case(F)
    gpd = gp.to(dev)
    got = NP.global_add_pool(_place(xi, layout, dev), gpd)
    assert torch.equal(got.cpu(), want_i)                      # integer sums are exact in f32 in any order
    xg = _place(xr, layout, dev).requires_grad_(True)
    out = NP.global_add_pool(xg, gpd)
    assert rel_max(out, want_r) <= GRAD_REL
    (dx,) = torch.autograd.grad(out, xg, dout.to(dev))
    assert torch.equal(dx.cpu(), want_dx)
    assert float(dx[:3].abs().sum()) == 0.0 and float(dx[-5:].abs().sum()) == 0.0          # rows outside every graph
    # the batch-vector form of the same rows
    batch = ref.batch_of(ref.SIZES).to(dev)
    assert torch.equal(NP.global_add_pool(xg.detach()[3:-5], batch, len(ref.SIZES)), out.detach())


@functools.lru_cache(maxsize=None)
def _sort_case(F):
    gp = ref.graph_ptr(ref.SIZES)
    N = int(gp[-1])
    x = ref.randn_table(N, F, F + 3)
    x[:, -1] = ref.tied_keys(N, F + 4)
    return gp, x


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F", ref.WIDTHS)
def test_sort_pool(dev, F, layout):
    gp, x = _sort_case(F)
    gpd, batch = gp.to(dev), ref.batch_of(ref.SIZES).to(dev)
    B = len(ref.SIZES)
    for k in (1, 64, 65, 66, 2 * C + 10):                     # n - 1, n, n + 1 of the 65-row graph; more rows than any graph has
        xg = _place(x, layout, dev).requires_grad_(True)
        out = NP.global_sort_pool(xg, batch, k, B)
        assert out.shape == (B, k * F)
        assert torch.equal(_bits(out), _bits(ref.sort_pool(x, gp, k))), k          # (bits: NaN keys travel with their rows)
        dout = ref.randn_table(B, k * F, k)
        (dx,) = torch.autograd.grad(out, xg, dout.to(dev))
        want = ref.sort_pool_bwd(dout, x, gp, k)
        assert torch.equal(dx.cpu(), want), k
        rank, _ = ref.ranks(x, gp)
        assert float(dx.cpu()[rank >= k].abs().sum()) == 0.0
    gb = NG.GraphBatch(_place(x, layout, dev), torch.zeros((2, 0), dtype=torch.int64, device=dev), batch, B,
                       sizes=torch.tensor(ref.SIZES))
    assert torch.equal(_bits(NP.global_sort_pool(gb, k=3)), _bits(ref.sort_pool(x, gp, 3)))


def test_sort_pool_selection_paths_agree_and_a_graph_beyond_the_lds_sort(dev):
    """after the NaN canonicalisation the LDS selection and the radix selection give the same order (they differ on raw NaNs with
    the sign bit set); a graph of 16,385 rows takes the radix path"""
    gp, x = _sort_case(6)
    xd, gpd, batch = x.to(dev), gp.to(dev), ref.batch_of(ref.SIZES).to(dev)
    lds, radix = (NP._sort_order(xd, gpd, batch, None, selection=s) for s in ("lds", "radix"))
    rank, _ = ref.ranks(x, gp)
    assert torch.equal(lds[0], radix[0]) and torch.equal(lds[1], radix[1])
    assert torch.equal(lds[1].cpu().long() - gp.long()[ref.batch_of(ref.SIZES)], rank)
    sizes = [5, 16385, 0, 300]
    gp, batch = ref.graph_ptr(sizes), ref.batch_of(sizes)
    x = ref.randn_table(batch.numel(), 6, 9)
    x[:, -1] = ref.tied_keys(batch.numel(), 10)
    for known in (None, torch.tensor(sizes)):                # sizes unknown and N > 16,384; sizes known on the host
        xg = x.to(dev).requires_grad_(True)
        src = xg if known is None else NG.GraphBatch(xg, torch.zeros((2, 0), dtype=torch.int64, device=dev), batch.to(dev), 4, sizes=known)
        out = NP.global_sort_pool(src, batch.to(dev) if known is None else None, 70, 4)
        assert torch.equal(_bits(out), _bits(ref.sort_pool(x, gp, 70)))
        dout = ref.randn_table(4, 70 * 6, 11)
        (dx,) = torch.autograd.grad(out, xg, dout.to(dev))
        assert torch.equal(dx.cpu(), ref.sort_pool_bwd(dout, x, gp, 70))


@functools.lru_cache(maxsize=None)
def _att_case(F, big):
    sizes = BIG if big else ref.SIZES
    gp = ref.graph_ptr(sizes, first=3)
    N = int(gp[-1]) + 5
    gate, x, dout = 3 * ref.randn_table(N, 1, F + 5).view(-1), ref.randn_table(N, F, F + 6), ref.randn_table(len(sizes), F, F + 7)
    want = ref.attention(gate.double(), x.double(), gp)
    dx, dgate = ref.attention_bwd(gate.double(), x.double(), gp, dout.double())
    return gp, gate, x, dout, want, dx, dgate


def _att_run(dev, gp, gate, x, dout, layout="contiguous"):
    gg, xg = gate.to(dev).requires_grad_(True), _place(x, layout, dev).requires_grad_(True)
    out = NP.attention_readout(gg, xg, gp.to(dev))
    dx, dgate = torch.autograd.grad(out, (xg, gg), dout.to(dev))
    return out.detach(), dx, dgate


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F", ref.WIDTHS)
def test_attention(dev, F, layout):
    gp, gate, x, dout, want, want_dx, want_dgate = _att_case(F, False)
    out, dx, dgate = _att_run(dev, gp, gate, x, dout, layout)
    errs = rel_max(out, want), rel_max(dx, want_dx), rel_max(dgate, want_dgate)
    print(f"attention F={F} {layout}: out {errs[0]:.2e} dx {errs[1]:.2e} dgate {errs[2]:.2e}")
    assert max(errs) <= GRAD_REL
    empty = torch.tensor(ref.SIZES) == 0
    assert float(out.cpu()[empty].abs().sum()) == 0.0
    assert float(dx[:3].abs().sum()) == 0.0 and float(dx[-5:].abs().sum()) == 0.0 and float(dgate[:3].abs().sum()) == 0.0


@pytest.mark.parametrize("F", [64, 100])
def test_attention_long_graphs_against_fp64(dev, F):
    """gate = 3 randn, x = randn, graphs of 5,000 and 20,000 rows among the others: the three errors against the fp64 reference"""
    gp, gate, x, dout, want, want_dx, want_dgate = _att_case(F, True)
    out, dx, dgate = _att_run(dev, gp, gate, x, dout)
    errs = rel_max(out, want), rel_max(dx, want_dx), rel_max(dgate, want_dgate)
    print(f"attention, long graphs, F={F}: rel_max out {errs[0]:.2e} dx {errs[1]:.2e} dgate {errs[2]:.2e}")
    assert max(errs) <= GRAD_REL


def test_attention_constant_and_dominant_gates(dev):
    gp = ref.graph_ptr(ref.SIZES)
    N = int(gp[-1])
    x = ref.randn_table(N, 100, 21)
    full = torch.tensor(ref.SIZES) > 0
    out = NP.attention_readout(torch.full((N,), 1.25, device=dev), x.to(dev), gp.to(dev))
    mean = ref.add(x.double(), gp)[full] / torch.tensor(ref.SIZES)[full, None]
    assert rel_max(out[full.to(dev)], mean) <= GRAD_REL        # a constant gate: the mean
    gate = ref.randn_table(N, 1, 22).view(-1)
    chosen = (gp[:-1].long() + torch.tensor(ref.SIZES) // 2)[full]
    gate[chosen] = gate.max() + 80.0                           # one gate 80 above the rest: that row
    out = NP.attention_readout(gate.to(dev), x.to(dev), gp.to(dev)).cpu()
    assert float(((out[full] - x[chosen]).abs() / x[chosen].abs().clamp(min=1e-30)).max()) <= 1e-6


@pytest.mark.parametrize("F", [6, 100, 256])
def test_invariances(dev, F):
    """the bits of a graph's result depend on its own rows alone: not on the batch around it (at an offset that is no multiple of
    the chunk or of a vector), not on the pitch, not on the run"""
    n = 2 * C + 3
    x1, g1, d1 = ref.randn_table(n, F, 31), 3 * ref.randn_table(n, 1, 32).view(-1), ref.randn_table(1, F, 33)
    sizes = [C + 7, n, 5]
    lo = sizes[0]
    xb, gb_ = ref.randn_table(sum(sizes), F, 34), 3 * ref.randn_table(sum(sizes), 1, 35).view(-1)
    xb[lo:lo + n], gb_[lo:lo + n] = x1, g1
    db = ref.randn_table(3, F, 36)
    db[1] = d1[0]
    gp1, gpb = ref.graph_ptr([n]), ref.graph_ptr(sizes)

    def add(x, gp, dout, layout="contiguous"):
        xg = _place(x, layout, dev).requires_grad_(True)
        out = NP.global_add_pool(xg, gp.to(dev))
        return out.detach(), torch.autograd.grad(out, xg, dout.to(dev))[0]
    a_alone, a_batch = add(x1, gp1, d1), add(xb, gpb, db)
    assert torch.equal(a_alone[0][0], a_batch[0][1]) and torch.equal(a_alone[1], a_batch[1][lo:lo + n])
    t_alone, t_batch = _att_run(dev, gp1, g1, x1, d1), _att_run(dev, gpb, gb_, xb, db)
    assert torch.equal(t_alone[0][0], t_batch[0][1])
    assert torch.equal(t_alone[1], t_batch[1][lo:lo + n]) and torch.equal(t_alone[2], t_batch[2][lo:lo + n])
    for layout in LAYOUTS[1:] + LAYOUTS[:1]:                  # the other pitches and alignments; then the same call again
        again = add(xb, gpb, db, layout)
        assert torch.equal(again[0], a_batch[0]) and torch.equal(again[1], a_batch[1]), layout
        again = _att_run(dev, gpb, gb_, xb, db, layout)
        assert all(torch.equal(p, q) for p, q in zip(again, t_batch)), layout


def test_empty_batches(dev):
    x0, gp0 = torch.zeros((0, 6), device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    x, batch = ref.randn_table(9, 6, 41).to(dev), torch.zeros(9, dtype=torch.int64, device=dev)
    gp_empty = torch.zeros(4, dtype=torch.int32, device=dev)   # three graphs, no row in any
    for fn in (lambda t, p: NP.global_add_pool(t, p), lambda t, p: NP.global_sort_pool(t, p, 2),
               lambda t, p: NP.attention_readout(t[:, 0].contiguous(), t, p)):
        assert fn(x0, gp0).shape[0] == 0                       # B = 0, N = 0
        out = fn(x0, gp_empty)                                 # N = 0
        assert out.shape[0] == 3 and float(out.abs().sum()) == 0.0
        xg = x.clone().requires_grad_(True)
        out = fn(xg, gp0)                                      # B = 0 over nine rows: nothing to read out, no gradient
        assert out.shape[0] == 0
        assert float(torch.autograd.grad(out.sum() + 0.0 * xg.sum(), xg)[0].abs().sum()) == 0.0
    assert NP.global_add_pool(x, batch, 1).shape == (1, 6)


def test_capture(dev):
    """forward and backward of each readout inside torch.cuda.graph (num_graphs given: nothing is read back), replayed twice"""
    B = len(ref.SIZES)
    gp = ref.graph_ptr(ref.SIZES)
    N = int(gp[-1])
    batch = ref.batch_of(ref.SIZES).to(dev)
    x = ref.randn_table(N, 100, 51)
    x[:, -1] = ref.tied_keys(N, 52)
    x[:, -1] = torch.nan_to_num(x[:, -1], nan=3.0, posinf=4.0)                         # (finite: the results are compared as values)
    gate = ref.randn_table(N, 1, 53).view(-1)
    douts = {1: ref.randn_table(B, 100, 54).to(dev), 5: ref.randn_table(B, 500, 55).to(dev)}
    steps = {"add": (lambda xg, gg: NP.global_add_pool(xg, batch, B), 1),
             "sort": (lambda xg, gg: NP.global_sort_pool(xg, batch, 5, B), 5),
             "attention": (lambda xg, gg: NP.attention_readout(gg, xg, batch, B), 1)}
    for name, (fn, k) in steps.items():
        def step(leaves):
            """forward and backward as a training step runs them; the output leaves WITHOUT its autograd graph (a graph kept alive
            binds its accumulation nodes to the stream of their first use, as npi_gnn_amd/graphed.py explains)"""
            for t in leaves:
                t.grad = None
            out = fn(*leaves)
            out.backward(douts[k])
            return out.detach()
        used = (0, 1) if name == "attention" else (0,)
        leaves = [x.to(dev).requires_grad_(True), gate.to(dev).requires_grad_(True)]
        eager = [step(leaves).clone()] + [leaves[i].grad.clone() for i in used]
        # leaves of their own, and the warm-up on the stream that is captured
        leaves = [x.to(dev).requires_grad_(True), gate.to(dev).requires_grad_(True)]
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            for _ in range(2):
                step(leaves)
            torch.cuda.synchronize(dev)
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg, stream=stream):
                out = step(leaves)
        torch.cuda.current_stream(dev).wait_stream(stream)
        held = [out] + [leaves[i].grad for i in used]
        for _ in range(2):
            for t in held:
                t.zero_()
            cg.replay()
            torch.cuda.synchronize(dev)
            assert all(torch.equal(a, b) for a, b in zip(held, eager)), name


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _torch_readout(kind, att, k):
    """the reference readout composed in torch on the device"""
    def readout(x, batch, B):
        gp = torch.searchsorted(batch, torch.arange(B + 1, device=batch.device)).to(torch.int32)
        if kind == "add":
            return ref.add(x, gp)
        if kind == "sort":
            return ref.sort_pool(x, gp, k)
        return ref.attention(att.gate_nn(x).view(-1), x, gp)
    return readout


def _fused_readout(kind, att, k):
    def readout(x, batch, B):
        if kind == "add":
            return NP.global_add_pool(x, batch, B)
        if kind == "sort":
            return NP.global_sort_pool(x, batch, k, B)
        return att(x, batch, B)
    return readout


@pytest.mark.parametrize("kind", ["add", "sort", "attention"])
def test_net1_shaped_model_trains_on_each_readout(dev, kind):
    from test_gpu_pool import Net1, load

    class Net1R(Net1):
        def __init__(self, nf, width):
            super().__init__(nf)
            self.lin1 = torch.nn.Linear(width, 128)
            self.att = NP.GlobalAttention(torch.nn.Linear(128, 1))
            self.dropout_p = 0.0
            self.readout = None

        def forward(self, x, edge_index, batch, B):
            acc = None
            for conv, pool in ((self.conv1, self.pool1), (self.conv2, self.pool2), (self.conv3, self.pool3)):
                x = F_.relu(conv(x, edge_index))
                x, edge_index, _, batch, _, _ = pool(x, edge_index, None, batch)
                r = self.readout(x, batch, B)
                acc = r if acc is None else acc + r
            x = F_.relu(self.lin2(F_.relu(self.lin1(acc))))
            return F_.log_softmax(self.lin3(x), dim=-1)

    fx = load("rpi369_fold0.pt")
    x, ei, batch, y = (fx[n].to(dev) for n in ("x", "edge_index", "batch", "y"))
    y, B, k = y.long(), fx["y"].numel(), 4
    torch.manual_seed(0)
    fused = Net1R(x.size(1), 128 * k if kind == "sort" else 128).to(dev)
    plain = copy.deepcopy(fused)
    fused.readout, plain.readout = _fused_readout(kind, fused.att, k), _torch_readout(kind, plain.att, k)
    losses = []
    for model in (fused, plain):
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=0.01)
        trace = []
        for _ in range(3):
            opt.zero_grad()
            loss = F_.nll_loss(model(x, ei, batch, B), y)
            loss.backward()
            opt.step()
            trace.append(loss.detach().double().cpu())
        losses.append(torch.stack(trace))
    print(f"{kind}: losses {losses[0].tolist()} against {losses[1].tolist()}")
    if kind == "sort":
        assert torch.equal(losses[0][0], losses[1][0])         # the forward copies rows: bit for bit
    assert float(((losses[0] - losses[1]).abs() / losses[1].abs()).max()) <= GRAD_REL
    if kind == "attention":
        assert fused.att.gate_nn.weight.grad is not None and float(fused.att.gate_nn.weight.grad.abs().sum()) > 0.0
