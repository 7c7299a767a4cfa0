"""The readouts of Rule O without a GPU: the torch reference against the literal PyG 1.4.2 compositions, the rule's order on special
values, the new symbols, every argument the entry points refuse (on the host, before any launch; no pointer is followed), and the
Python surface."""
import ctypes

import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import pool as NP

import _readout_ref as ref

NPI_ERR_ARG = -1
A = 0x10000                      # a 16-byte aligned stand-in for every pointer: never dereferenced by a refused call
SIZES = [5, 0, 1, 9, 0, 17, 2]


# ---- PyG 1.4.2, restated ---------------------------------------------------------------------------------------------------------
def _pyg_to_dense_batch(x, batch, fill_value):
    B = int(batch[-1]) + 1
    num_nodes = torch.zeros(B, dtype=torch.long).index_add_(0, batch, torch.ones_like(batch))
    cum = torch.cat([num_nodes.new_zeros(1), num_nodes.cumsum(0)])
    n_max = int(num_nodes.max())
    idx = torch.arange(batch.size(0)) - cum[batch] + batch * n_max
    out = x.new_full((B * n_max, x.size(1)), fill_value)
    out[idx] = x
    return out.view(B, n_max, x.size(1))


def _pyg_global_sort_pool(x, batch, k):
    fill_value = x.min().item() - 1
    batch_x = _pyg_to_dense_batch(x, batch, fill_value)
    B, N, D = batch_x.size()
    _, perm = batch_x[:, :, -1].sort(dim=-1, descending=True)
    arange = torch.arange(B, dtype=torch.long) * N
    perm = perm + arange.view(-1, 1)
    batch_x = batch_x.view(B * N, D)[perm.view(-1)].view(B, N, D)
    if N >= k:
        batch_x = batch_x[:, :k].contiguous()
    else:
        batch_x = torch.cat([batch_x, batch_x.new_full((B, k - N, D), fill_value)], dim=1)
    batch_x[batch_x == fill_value] = 0
    return batch_x.view(B, k * D)


def _pyg_softmax(src, index, num_nodes):
    mx = torch.full((num_nodes,), -float("inf"), dtype=src.dtype).scatter_reduce(0, index, src, "amax")
    out = (src - mx[index]).exp()
    return out / (torch.zeros(num_nodes, dtype=src.dtype).index_add(0, index, out)[index] + 1e-16)


def _pyg_global_attention(gate, x, batch, size):
    gate = _pyg_softmax(gate.view(-1), batch, size).view(-1, 1)
    return torch.zeros((size, x.size(1)), dtype=x.dtype).index_add(0, batch, gate * x)


def _case(F, seed):
    sizes = [n for n in SIZES]
    batch = ref.batch_of(sizes)
    return ref.randn_table(batch.numel(), F, seed).double(), batch, ref.graph_ptr(sizes), len(sizes)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5])
def test_reference_add_and_attention_are_the_pyg_compositions(F):
    x, batch, gp, B = _case(F, 1)
    want = torch.zeros(B, F, dtype=torch.float64).index_add(0, batch, x)                  # scatter_add
    assert float((ref.add(x, gp) - want).abs().max()) <= 1e-12
    dout = ref.randn_table(B, F, 2).double()
    xr = x.clone().requires_grad_(True)
    torch.zeros(B, F, dtype=torch.float64).index_add(0, batch, xr).backward(dout)
    assert torch.equal(ref.add_bwd(dout, gp, x.size(0)), xr.grad)
    gate = (3 * ref.randn_table(x.size(0), 1, 3)).double().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    want = _pyg_global_attention(gate, xr, batch, B)
    got = ref.attention(gate.detach(), x, gp)
    assert float((got - want.detach()).abs().max()) <= 1e-12
    assert float(got[1].abs().max()) == 0.0 and float(got[4].abs().max()) == 0.0          # empty graphs
    want.backward(dout)
    dx, dgate = ref.attention_bwd(gate.detach().view(-1), x, gp, dout)
    assert float((dx - xr.grad).abs().max()) <= 1e-12
    assert float((dgate - gate.grad.view(-1)).abs().max()) <= 1e-12


@pytest.mark.parametrize("k", [1, 4, 16, 17, 18, 40])
def test_reference_sort_pool_is_the_pyg_composition_on_tie_free_input(k):
    sizes = [5, 1, 9, 17, 2]                                  # (PyG's dense batch has no row for a trailing empty graph)
    batch, gp = ref.batch_of(sizes), ref.graph_ptr(sizes)
    x = ref.randn_table(batch.numel(), 3, 4).double()
    assert torch.equal(ref.sort_pool(x, gp, k), _pyg_global_sort_pool(x, batch, k))
    xr = x.clone().requires_grad_(True)
    dout = ref.randn_table(len(sizes), k * 3, 5).double()
    _pyg_global_sort_pool(xr, batch, k).backward(dout)
    assert float((ref.sort_pool_bwd(dout, x, gp, k) - xr.grad).abs().max()) <= 1e-12


def test_reference_order_on_special_values():
    """NaN keys of both signs rank first, +0.0 above -0.0, equal keys by index"""
    nan = float("nan")
    keys = torch.tensor([1.0, -0.0, nan, 0.0, float("inf"), -nan, 0.0, -0.0, 1.0, -float("inf")])
    bits = keys.view(torch.int32).clone()
    bits[5] |= -0x80000000                                    # a NaN with the sign bit set, whatever the parser made of -nan
    keys = bits.view(torch.float32)
    x = torch.stack([torch.arange(10.0), keys], dim=1)
    gp = ref.graph_ptr([10])
    rank, _ = ref.ranks(x, gp)
    order = torch.argsort(rank)
    assert order.tolist() == [2, 5, 4, 0, 8, 3, 6, 1, 7, 9]
    out = ref.sort_pool(x, gp, 12)
    assert out.view(12, 2)[:10, 0].tolist() == [2.0, 5.0, 4.0, 0.0, 8.0, 3.0, 6.0, 1.0, 7.0, 9.0]
    assert torch.equal(out.view(12, 2)[:10, 1].view(torch.int32), keys[order].view(torch.int32))      # copied bit for bit
    assert float(out.view(12, 2)[10:].abs().sum()) == 0.0     # only the padding is zero
    # two graphs, rows outside both: rank -1
    rank, g = ref.ranks(x, ref.graph_ptr([3, 4], first=2))
    assert rank.tolist() == [-1, -1, 0, 2, 1, 0, 2, 3, 1, -1] and g.tolist() == [-1, -1, 0, 0, 0, 1, 1, 1, 1, -1]
    t = ref.tied_keys(4000, 3)
    assert bool(torch.isnan(t).any()) and bool(((t == 0) & torch.signbit(t)).any()) and bool(((t == 0) & ~torch.signbit(t)).any())
    assert bool((t[torch.isnan(t)].view(torch.int32) < 0).any()) and bool((t[torch.isnan(t)].view(torch.int32) > 0).any())


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
NAMES = ("npi_readout_add_workspace_bytes", "npi_readout_add", "npi_readout_add_bwd", "npi_readout_attention_workspace_bytes",
         "npi_readout_attention", "npi_readout_attention_bwd", "npi_sort_pool_keys", "npi_sort_pool_gather", "npi_sort_pool_bwd")


def test_symbols_and_abi_version():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert lib.npi_abi_version() == 4                              # an additive change
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "readout.hip" in SOURCES and "readout.hip" not in HOST_ONLY
    assert NP.READOUT_CHUNK == ref.CHUNK == 1024


def test_workspace_queries():
    lib = _lib.load()
    for query, extra in ((lib.npi_readout_add_workspace_bytes, 0), (lib.npi_readout_attention_workspace_bytes, 2)):
        W = 5000 // 1024 + 7                                   # workgroups: N / chunk + B
        got = query(5000, 7, 100)
        assert got >= 8 * 4 + W * (100 + extra) * 4 and got % 16 == 0
        assert query(0, 0, 1) >= 0
        assert query(-1, 7, 100) == -1 and query(5000, -1, 100) == -1 and query(5000, 7, 0) == -1
    assert lib.npi_readout_attention_workspace_bytes(5000, 7, 100) > lib.npi_readout_add_workspace_bytes(5000, 7, 100)


def _add(lib, x=A, ldx=8, gp=A, N=100, B=3, F=8, out=A, ldo=8, ws=A, ws_bytes=1 << 20):
    return lib.npi_readout_add(x, ldx, gp, N, B, F, out, ldo, ws, ws_bytes, None)


def _add_bwd(lib, dout=A, ldd=8, gp=A, N=100, B=3, F=8, dx=A, lddx=8):
    return lib.npi_readout_add_bwd(dout, ldd, gp, N, B, F, dx, lddx, None)


def _att(lib, gate=A, x=A, ldx=8, gp=A, N=100, B=3, F=8, out=A, ldo=8, m=A, s=A, ws=A, ws_bytes=1 << 20):
    return lib.npi_readout_attention(gate, x, ldx, gp, N, B, F, out, ldo, m, s, ws, ws_bytes, None)


def _att_bwd(lib, gate=A, x=A, ldx=8, gp=A, N=100, B=3, F=8, out=A, ldo=8, m=A, s=A, dout=A, ldd=8, dx=A, lddx=8, dgate=A):
    return lib.npi_readout_attention_bwd(gate, x, ldx, gp, N, B, F, out, ldo, m, s, dout, ldd, dx, lddx, dgate, None)


def _keys(lib, x=A, ldx=8, N=100, F=8, keys=A):
    return lib.npi_sort_pool_keys(x, ldx, N, F, keys, None)


def _gather(lib, x=A, ldx=8, order=A, gp=A, N=100, B=3, F=8, k=4, out=A, ldo=32):
    return lib.npi_sort_pool_gather(x, ldx, order, gp, N, B, F, k, out, ldo, None)


def _sort_bwd(lib, dout=A, ldd=32, remap=A, gp=A, N=100, B=3, F=8, k=4, dx=A, lddx=8):
    return lib.npi_sort_pool_bwd(dout, ldd, remap, gp, N, B, F, k, dx, lddx, None)


SIZES_BAD = {"F = 0": dict(F=0), "F < 0": dict(F=-4), "negative N": dict(N=-1)}
GRAPHS_BAD = {"negative B": dict(B=-1), "null graph_ptr": dict(gp=None)}
REFUSED = [
    (_add, "npi_readout_add", dict(SIZES_BAD, **GRAPHS_BAD, **{
        "null table": dict(x=None), "null output": dict(out=None), "table pitch": dict(ldx=7), "output pitch": dict(ldo=7),
        "null workspace": dict(ws=None), "misaligned workspace": dict(ws=A + 4), "short workspace": "add", "negative workspace": dict(ws_bytes=-1)})),
    (_add_bwd, "npi_readout_add_bwd", dict(SIZES_BAD, **GRAPHS_BAD, **{
        "null dout": dict(dout=None), "null dx": dict(dx=None), "dout pitch": dict(ldd=7), "dx pitch": dict(lddx=7)})),
    (_att, "npi_readout_attention", dict(SIZES_BAD, **GRAPHS_BAD, **{
        "null gate": dict(gate=None), "null table": dict(x=None), "null output": dict(out=None), "null m": dict(m=None), "null s": dict(s=None),
        "table pitch": dict(ldx=7), "output pitch": dict(ldo=7), "null workspace": dict(ws=None), "misaligned workspace": dict(ws=A + 8),
        "short workspace": "attention", "negative workspace": dict(ws_bytes=-1)})),
    (_att_bwd, "npi_readout_attention_bwd", dict(SIZES_BAD, **GRAPHS_BAD, **{
        "null gate": dict(gate=None), "null table": dict(x=None), "null out": dict(out=None), "null m": dict(m=None), "null s": dict(s=None),
        "null dout": dict(dout=None), "null dx": dict(dx=None), "null dgate": dict(dgate=None), "table pitch": dict(ldx=7),
        "out pitch": dict(ldo=7), "dout pitch": dict(ldd=7), "dx pitch": dict(lddx=7)})),
    (_keys, "npi_sort_pool_keys", dict(SIZES_BAD, **{"null table": dict(x=None), "null keys": dict(keys=None), "table pitch": dict(ldx=7)})),
    (_gather, "npi_sort_pool_gather", dict(SIZES_BAD, **GRAPHS_BAD, **{
        "k = 0": dict(k=0), "k < 0": dict(k=-2), "null table": dict(x=None), "null order": dict(order=None), "null output": dict(out=None),
        "table pitch": dict(ldx=7), "output pitch": dict(ldo=31)})),
    (_sort_bwd, "npi_sort_pool_bwd", dict(SIZES_BAD, **GRAPHS_BAD, **{
        "k = 0": dict(k=0), "k < 0": dict(k=-2), "null dout": dict(dout=None), "null remap": dict(remap=None), "null dx": dict(dx=None),
        "dout pitch": dict(ldd=31), "dx pitch": dict(lddx=7)})),
]


@pytest.mark.parametrize("call,name,cases", REFUSED, ids=[r[1] for r in REFUSED])
def test_bad_arguments_are_refused_before_a_launch(call, name, cases):
    lib = _lib.load()
    for what, kw in cases.items():
        if kw == "add":
            kw = dict(ws_bytes=lib.npi_readout_add_workspace_bytes(100, 3, 8) - 1)
        elif kw == "attention":
            kw = dict(ws_bytes=lib.npi_readout_attention_workspace_bytes(100, 3, 8) - 1)
        assert call(lib, **kw) == NPI_ERR_ARG, what
        msg = lib.npi_last_error().decode()
        assert msg.startswith(name + ":"), (what, msg)
    # nothing to write: no launch, and no pointer is looked at
    names = call.__code__.co_varnames[1:call.__code__.co_argcount]
    nothing = {n: None for n, default in zip(names, call.__defaults__) if default == A}       # every pointer of the call
    assert call(lib, **dict(nothing, N=0)) == 0
    if "B" in names:
        assert call(lib, **dict(nothing, B=0)) == 0


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_global_attention_module_is_pygs():
    torch.manual_seed(0)
    gate_nn = torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.ReLU(), torch.nn.Linear(4, 1))
    att = NP.GlobalAttention(gate_nn, torch.nn.Linear(8, 6))
    assert list(att.state_dict()) == ["gate_nn.0.weight", "gate_nn.0.bias", "gate_nn.2.weight", "gate_nn.2.bias", "nn.weight", "nn.bias"]
    assert list(NP.GlobalAttention(torch.nn.Linear(8, 1)).state_dict()) == ["gate_nn.weight", "gate_nn.bias"]
    assert NP.GlobalAttention(torch.nn.Linear(8, 1)).nn is None
    before = att.nn.weight.detach().clone()
    att.reset_parameters()                                         # reaches the leaves of both modules
    assert not torch.equal(before, att.nn.weight.detach())
    assert repr(att).startswith("GlobalAttention(gate_nn=Sequential(") and "nn=Linear(" in repr(att)
    import inspect
    assert list(inspect.signature(att.forward).parameters) == ["x", "batch", "size"]
    assert list(inspect.signature(NP.global_add_pool).parameters) == ["x", "batch", "size"]
    assert list(inspect.signature(NP.global_sort_pool).parameters)[:3] == ["x", "batch", "k"]
    assert list(inspect.signature(NP.attention_readout).parameters) == ["gate", "x", "batch_or_graph_ptr", "num_graphs"]


def test_readouts_refuse_bf16_and_cpu_tensors_by_name():
    x, batch, gate = torch.randn(5, 8), torch.tensor([0, 0, 1, 1, 1]), torch.randn(5)
    with pytest.raises(NotImplementedError, match="global_add_pool.*bf"):
        NP.global_add_pool(x.bfloat16(), batch, 2)
    with pytest.raises(NotImplementedError, match="global_sort_pool.*bf"):
        NP.global_sort_pool(x.bfloat16(), batch, 3, 2)
    with pytest.raises(NotImplementedError, match="attention_readout.*x.*bf"):
        NP.attention_readout(gate, x.bfloat16(), batch, 2)
    with pytest.raises(NotImplementedError, match="attention_readout.*gate.*bf"):
        NP.attention_readout(gate.bfloat16(), x, batch, 2)
    with pytest.raises(NotImplementedError, match="attention_readout.*bf"):
        NP.GlobalAttention(torch.nn.Linear(8, 1).bfloat16())(x.bfloat16(), batch, 2)
    with pytest.raises(ValueError, match="global_sort_pool.*k"):
        NP.global_sort_pool(x, batch, 0, 2)
    with pytest.raises(npi.NpiError):
        NP.global_add_pool(x, batch, 2)
    with pytest.raises(npi.NpiError):
        NP.global_sort_pool(x, batch, 3, 2)
    with pytest.raises(npi.NpiError):
        NP.attention_readout(gate, x, batch, 2)
    with pytest.raises(npi.NpiError):
        NP.GlobalAttention(torch.nn.Linear(8, 1))(x, batch, 2)
