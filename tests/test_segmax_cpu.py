"""Max aggregation without a GPU: the host reference of Rule X against the literal torch composition, the new symbols, every
argument the entry points refuse (checked on the host before any launch; no pointer is followed), and the layer's keyword."""
import ctypes

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import functional as NF

import _segmax_ref as ref

NPI_ERR_ARG = -1
A = 0x10000                      # a 16-byte aligned stand-in for every pointer: never dereferenced by a refused call


def _small_graph(seed=3, n=40, e=300):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(1, n - 1, (e,), generator=g)              # rows 0 and n-1 stay empty
    pairs = torch.unique(torch.stack([src, dst])[:, src != dst], dim=1)          # no repeated column: no tie on randn values
    pairs = pairs[:, torch.randperm(pairs.size(1), generator=g)]
    return pairs[0].numpy(), pairs[1].numpy(), n


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
def test_reference_is_the_torch_composition_on_randn(self_loops):
    src, dst, n = _small_graph()
    x = ref.randn_table(n, 9, 1).double().requires_grad_(True)    # (f32 values, the composition's sums in fp64 like the reference's)
    out, arg = ref.rule_x(x, src, dst, n, self_loops)
    want = ref.torch_amax(x, src, dst, n, self_loops)
    assert torch.equal(out.double(), want.detach())
    dout = ref.randn_table(n, 9, 2)
    want.backward(dout.double())                                   # no ties on randn: autograd sends each cell to its one winner
    got = ref.rule_x_bwd(dout, arg, src, n)
    assert float((got - x.grad).abs().max()) <= 1e-12
    empty = (arg == -2)
    assert bool(empty.any()) == (not self_loops) and bool((out[empty] == 0).all())
    if self_loops:
        assert bool((arg[0] == -1).all()) and torch.equal(out[0].double(), x[0].detach())      # a row whose only entry is the loop


def test_vectorised_reference_is_the_literal_loop():
    src, dst, n = _small_graph(seed=5, n=24, e=200)
    x = ref.int_table(n, 5, -1, 1, 7).clone()
    x[3, 0], x[4, 1], x[5, 1] = float("nan"), float("nan"), -float("nan")
    x[6] = -0.0
    for loops in (False, True):
        a, b = ref.rule_x(x, src, dst, n, loops), ref.rule_x_loop(x, src, dst, n, loops)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_reference_special_values_against_torch():
    """NaN, +-0.0, -inf and empty rows: the same VALUES as ``scatter_reduce('amax')`` (NaN where it has NaN), and the rule's bits"""
    src = np.array([1, 2, 3, 1, 2, 4, 4, 5])
    dst = np.array([0, 0, 0, 1, 1, 2, 3, 3])
    n = 7                                                          # rows 4, 5, 6 are empty
    x = torch.tensor([[0.0, 0.0], [float("nan"), -0.0], [1.0, 0.0], [float("nan"), -0.0], [-0.0, -float("inf")],
                      [-0.0, -float("inf")], [9.0, 9.0]])
    out, arg = ref.rule_x(x, src, dst, n, False)
    want = ref.torch_amax(x, src, dst, n, False)
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(out, nan=7.0), torch.nan_to_num(want, nan=7.0))           # (-0.0 == 0.0 as values)
    bits = out.view(torch.int32)
    assert bits[0, 0] == 0x7FC00000 and arg[0, 0] == 0            # two NaNs: the smaller eid
    assert bits[0, 1] == 0 and arg[0, 1] == 0                     # -0.0, 0.0, -0.0: a tie, written as +0.0
    assert bits[2, 0] == 0 and arg[2, 0] == 5                     # a row of only -0.0 -> +0.0
    assert out[3, 1] == -float("inf") and arg[3, 1] == 6          # -inf everywhere: the smaller eid
    assert bool((arg[4:] == -2).all()) and bool((bits[4:] == 0).all())


def test_stress_inputs_exercise_the_tie_rule():
    ei = ref.stress_edges()
    deg = torch.bincount(ei[1], minlength=ref.N_STRESS)
    assert all(int(deg[r]) == 0 for r in ref.EMPTY_ROWS)
    assert all(int(deg[r]) == k for r, k in ref.SIZED_ROWS.items())
    assert int(deg[ref.HUB_ROW]) == ref.HUB and int(torch.bincount(ei[0], minlength=ref.N_STRESS)[ref.HUB_SRC]) >= ref.HUB
    assert not bool((ei[0] == ei[1]).any())
    for loops in (False, True):
        x = ref.stress_reference(64, loops)[0]
        frac = ref.tied_fraction(x, ei[0].numpy(), ei[1].numpy(), ref.N_STRESS, loops)
        print(f"tied maxima, self_loops={loops}: {frac:.3f}")
        assert frac >= 0.30


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("npi_segmax_workspace_bytes", "npi_segmax", "npi_segmax_bwd"):
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert lib.npi_abi_version() == 4                              # an additive change
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "segmax.hip" in SOURCES and "segmax.hip" not in HOST_ONLY


def test_workspace_query():
    lib = _lib.load()
    for item in (64, 256):
        items = -(-1000 // item)
        got = lib.npi_segmax_workspace_bytes(1000, item, 100)
        assert got >= items * (2 * 100 * 8 + 4) and got % 16 == 0   # a (value, eid) head and tail per item and column, the tails' rows
    assert lib.npi_segmax_workspace_bytes(0, 64, 100) == 0
    assert lib.npi_segmax_workspace_bytes(1000, 100, 100) == -1     # no such item size
    assert lib.npi_segmax_workspace_bytes(1000, 64, 0) == -1
    assert lib.npi_segmax_workspace_bytes(-1, 64, 8) == -1


def _fwd(lib, rowptr=A, col=A, eid=A, rowidx=A, item=64, N=100, nnz_max=1000, x=A, ldx=8, F=8, out=A, ldo=8, arg=A, lda=8, ws=A,
         ws_bytes=1 << 20):
    return lib.npi_segmax(rowptr, col, eid, rowidx, item, N, 100, nnz_max, x, ldx, F, out, ldo, arg, lda, ws, ws_bytes, None)


def _bwd(lib, rowptr=A, col=A, eid=A, rowidx=A, item=64, N=100, nnz_max=1000, x=A, ldx=8, F=8, out=A, ldo=8, arg=A, lda=8, ws=A,
         ws_bytes=1 << 20):
    return lib.npi_segmax_bwd(rowptr, col, eid, rowidx, item, N, 100, nnz_max, x, ldx, arg, lda, F, out, ldo, ws, ws_bytes, None)


@pytest.mark.parametrize("call,name", [(_fwd, "npi_segmax"), (_bwd, "npi_segmax_bwd")])
def test_bad_arguments_are_refused_before_a_launch(call, name):
    lib = _lib.load()
    cases = {"null rowptr": dict(rowptr=None), "null col": dict(col=None), "null eid": dict(eid=None), "null rowidx": dict(rowidx=None),
             "null table": dict(x=None), "null output": dict(out=None), "null arg": dict(arg=None),
             "F = 0": dict(F=0), "F < 0": dict(F=-4), "table pitch": dict(ldx=7), "output pitch": dict(ldo=7), "arg pitch": dict(lda=7),
             "item 100": dict(item=100), "item 0": dict(item=0), "null workspace": dict(ws=None), "misaligned workspace": dict(ws=A + 4),
             "short workspace": dict(ws_bytes=lib.npi_segmax_workspace_bytes(1000, 64, 8) - 1), "negative N": dict(N=-1),
             "negative nnz_max": dict(nnz_max=-1)}
    for what, kw in cases.items():
        assert call(lib, **kw) == NPI_ERR_ARG, what
        msg = lib.npi_last_error().decode()
        assert msg.startswith(name + ":"), (what, msg)
    assert call(lib, N=0, nnz_max=0, ws=None, ws_bytes=0) == 0          # nothing to write: no launch


# ---- the layer ---------------------------------------------------------------------------------------------------------------
def test_module_keyword_and_checkpoints():
    torch.manual_seed(0)
    mx, mean = npi.SAGEConv(8, 8, aggr="max"), npi.SAGEConv(8, 8)
    assert mx.aggr == "max" and mean.aggr == "mean"
    assert repr(mean) == "SAGEConv(8, 8)" and repr(mx) == "SAGEConv(8, 8, aggr='max')"
    assert list(mx.state_dict()) == list(mean.state_dict()) == ["weight", "bias"]
    assert mx.weight.shape == mean.weight.shape and float(mx.weight.detach().abs().max()) <= 1.0 / 8 ** 0.5
    mean.load_state_dict(mx.state_dict())
    assert torch.equal(mean.weight, mx.weight)
    mx.load_state_dict(npi.SAGEConv(8, 8).state_dict())
    assert npi.SAGEConv(8, 4, concat=True, aggr="max").weight.shape == (16, 4)
    for bad in ("add", "min", "sum", None):
        with pytest.raises(ValueError, match="'mean' or 'max'"):
            npi.SAGEConv(8, 8, aggr=bad)
    with pytest.raises(ValueError, match="'mean' or 'max'"):
        NF.sage_conv(torch.zeros(3, 8), torch.zeros((2, 0), dtype=torch.int64), torch.zeros(8, 8), aggr="add")
    with pytest.raises(ValueError, match="'mean' or 'max'"):
        NF.sage_conv_bipartite((torch.zeros(3, 8), None), torch.zeros((2, 0), dtype=torch.int64), torch.zeros(8, 8), aggr="add")


def test_max_refuses_bf16_edge_weight_and_cpu_tensors_by_name():
    x, ei, w = torch.randn(5, 8), torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.randn(8, 4)
    conv = npi.SAGEConv(8, 4, aggr="max")
    with pytest.raises(NotImplementedError, match="sage_conv.*bf"):
        NF.sage_conv(x.bfloat16(), ei, w.bfloat16(), aggr="max")
    with pytest.raises(NotImplementedError, match="sage_conv.*bf"):
        NF.sage_conv(x, ei, w.bfloat16(), aggr="max")
    with pytest.raises(NotImplementedError, match="sage_conv.*edge_weight"):
        conv(x, ei, edge_weight=torch.ones(3))
    with pytest.raises(NotImplementedError, match="sage_conv_bipartite.*edge_weight"):
        conv((x, None), ei, edge_weight=torch.ones(3))
    with pytest.raises(NotImplementedError, match="sage_conv_bipartite.*bf"):
        NF.sage_conv_bipartite((x.bfloat16(), None), ei, w.bfloat16(), aggr="max")
    with pytest.raises(NotImplementedError, match="segmax.*bf"):
        npi.segmax(ei, x.bfloat16())
    with pytest.raises(npi.NpiError):
        conv(x, ei)
    with pytest.raises(npi.NpiError):
        conv((x, None), ei)
    with pytest.raises(npi.NpiError):
        npi.segmax(ei, x)
