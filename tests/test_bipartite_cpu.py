"""The bipartite ``(x_src, x_dst)`` / ``size=`` form without a GPU: the fp64 restatement the GPU tests compare with
(``tests/_bipartite_ref.py``) is pinned to ``oracle/ref_conv.py``, every argument error of the new signatures is raised before
anything touches the device, and the new C-ABI symbol is declared, bound and exported."""
import ctypes
import os
import re

import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from oracle import ref_conv as oracle
import _bipartite_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(n=40, e=300, seed=0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    return ei[:, ei[0] != ei[1]]


def _with_loops(ei, n):
    return torch.cat([ei, torch.arange(n).unsqueeze(0).repeat(2, 1)], 1)


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------
def test_sage_restatement_equals_the_oracle_on_a_square_graph():
    n, F, Fo = 40, 7, 5
    g = torch.Generator().manual_seed(1)
    x, W, b = torch.randn(n, F, generator=g).double(), torch.randn(F, Fo, generator=g).double(), torch.randn(Fo, generator=g).double()
    ei = _graph(n)
    got = ref.sage_bipartite(x, _with_loops(ei, n), W, b, n_dst=n)
    want = oracle.sage_conv(x, ei, W, b)
    assert float((got - want).abs().max()) < 1e-12
    w = torch.rand(ei.size(1), generator=g).double() + 0.5
    got = ref.sage_bipartite(x, _with_loops(ei, n), W, b, n_dst=n, edge_weight=torch.cat([w, torch.ones(n).double()]), normalize=True)
    want = oracle.sage_conv(x, ei, W, b, edge_weight=w, normalize=True)
    assert float((got - want).abs().max()) < 1e-12


def test_sage_concat_restatement_equals_the_oracle():
    n, F, Fo = 40, 7, 5
    g = torch.Generator().manual_seed(2)
    x, W, b = torch.randn(n, F, generator=g).double(), torch.randn(2 * F, Fo, generator=g).double(), torch.randn(Fo, generator=g).double()
    ei = _graph(n, seed=3)
    got = ref.sage_bipartite(x, ei, W, b, n_dst=n, res_n_id=torch.arange(n), concat=True)
    want = oracle.sage_conv_concat(x, ei, W, b)
    assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("heads,concat", [(1, True), (4, True), (4, False)])
def test_gat_restatement_equals_the_oracle_on_a_square_graph(heads, concat):
    n, F, C = 40, 6, 4
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, F, generator=g).double()
    W = torch.randn(F, heads * C, generator=g).double()
    att = torch.randn(1, heads, 2 * C, generator=g).double()
    b = torch.randn(heads * C if concat else C, generator=g).double()
    ei = _graph(n, seed=5)
    got = ref.gat_bipartite(x, x, _with_loops(ei, n), W, att, b, heads=heads, concat=concat)
    want = oracle.gat_conv(x, ei, W, att, b, heads=heads, concat=concat)
    assert float((got - want).abs().max()) < 1e-12


def test_rectangular_case_by_hand():
    """5 sources, 3 targets, target 1 without an in-edge; edges (source -> target): 0->0, 1->0, 4->0, 2->2, 2->2 (a duplicate)"""
    x = torch.tensor([[1., 2.], [3., 4.], [5., 6.], [7., 8.], [9., 10.]], dtype=torch.float64)
    ei = torch.tensor([[0, 1, 4, 2, 2], [0, 0, 0, 2, 2]])
    W = torch.tensor([[1., 0., 2.], [0., 1., -1.]], dtype=torch.float64)
    b = torch.tensor([0.5, -0.5, 1.0], dtype=torch.float64)
    mean = torch.tensor([[13. / 3, 16. / 3], [0., 0.], [5., 6.]], dtype=torch.float64)
    want = torch.stack([torch.stack([m[0], m[1], 2 * m[0] - m[1]]) for m in mean]) + b
    got = ref.sage_bipartite(x, ei, W, b, n_dst=3)
    assert float((got - want).abs().max()) < 1e-12
    assert torch.equal(got[1], b)                                                   # the empty target: bias
    # concat with res_n_id = (4, 4, 0): [root | mean] @ W2
    W2 = torch.cat([W, 2 * W])
    root = x[[4, 4, 0]]
    want2 = root @ W + mean @ (2 * W) + b
    got2 = ref.sage_bipartite(x, ei, W2, b, n_dst=3, res_n_id=torch.tensor([4, 4, 0]), concat=True)
    assert float((got2 - want2).abs().max()) < 1e-12
    # GAT, one head, no x_dst: scores from the sources alone; target 0: softmax over sources 0, 1, 4; target 2: two equal entries
    Wg = torch.tensor([[1., 0.], [0., 1.]], dtype=torch.float64)
    att = torch.tensor([[[9., 9., 0.1, -0.1]]], dtype=torch.float64)               # the target half must not matter
    e = torch.nn.functional.leaky_relu(x @ torch.tensor([0.1, -0.1], dtype=torch.float64), 0.2)
    a0 = torch.softmax(e[[0, 1, 4]], 0)
    want3 = torch.stack([a0 @ x[[0, 1, 4]], torch.zeros(2, dtype=torch.float64), x[2]])
    got3 = ref.gat_bipartite(x, None, ei, Wg, att, None, n_dst=3)
    assert float((got3 - want3).abs().max()) < 1e-12
    # (-1, -1) padding and out-of-range columns are dropped
    ei_pad = torch.cat([ei, torch.tensor([[-1, 7], [-1, 0]])], 1)
    assert torch.equal(ref.sage_bipartite(x, ei_pad, W, b, n_dst=3), got)


# ---- validation: nothing below needs a GPU ------------------------------------------------------------------------------------------
def test_argument_errors_of_the_bipartite_signatures():
    sage, sagec, gat = npi.SAGEConv(8, 4), npi.SAGEConv(8, 4, concat=True), npi.GATConv(8, 4, heads=2)
    xs, xd = torch.randn(7, 8), torch.randn(5, 8)
    ei = torch.tensor([[0, 1, 6], [1, 2, 3]])
    for conv in (sage, gat):
        with pytest.raises(ValueError):
            conv((xs, xd), ei, size=(6, 5))                                        # size[0] != x_src rows
        with pytest.raises(ValueError):
            conv((xs, xd), ei, size=(7, 4))                                        # size[1] != x_dst rows
        with pytest.raises(ValueError):
            conv((None, xd), ei)                                                   # x_src is required
        with pytest.raises(ValueError):
            conv(xd, ei, size=(5, 4))                                              # a tensor with two id spaces
        with pytest.raises(ValueError):
            conv(xd, ei, size=(7, 7))
        with pytest.raises(TypeError):
            conv(npi.GraphBatch(xd, ei), None, size=(5, 5))                        # a GraphBatch together with size
    with pytest.raises(ValueError, match="tuple form"):
        sage(xd, ei, None, (5, 4))
    with pytest.raises(ValueError, match="res_n_id"):
        sagec((xs, xd), ei)                                                        # concat=True without res_n_id
    with pytest.raises(ValueError):
        sagec((xs, xd), ei, None, None, torch.zeros(4, dtype=torch.long))          # res_n_id of the wrong length
    with pytest.raises(ValueError):
        gat((xs, xd), ei, x_scales=torch.ones(7))
    with pytest.raises(ValueError):
        gat((xs, xd), ei, return_scales=True)
    drop = npi.GATConv(8, 4, dropout=0.5)
    with pytest.raises(NotImplementedError, match="dropout"):
        drop((xs, xd), ei)
    with pytest.raises(NotImplementedError, match="dropout"):
        drop(xd, ei, size=(5, 5))
    # a CSRGraph together with a tuple x: a TypeError (a CSRGraph cannot be built here; the check looks at the type only)
    fake = object.__new__(npi.CSRGraph)
    for conv in (sage, gat):
        with pytest.raises(TypeError):
            conv((xs, xd), fake)
    with pytest.raises(ValueError):
        npi.BipartiteGraph(ei, (7,))
    with pytest.raises(ValueError):
        npi.BipartiteGraph(ei.float(), (7, 5))


def test_valid_bipartite_calls_raise_the_no_gpu_error_on_cpu_tensors():
    """no CPU fall-back and no NotImplementedError left on the new signatures"""
    sage, sagec, gat = npi.SAGEConv(8, 4), npi.SAGEConv(8, 4, concat=True), npi.GATConv(8, 4, heads=2)
    xs, xd = torch.randn(7, 8), torch.randn(5, 8)
    ei = torch.tensor([[0, 1, 6], [1, 2, 3]])
    calls = [lambda: sage((xs, xd), ei), lambda: sage((xs, None), ei, size=(7, 5)), lambda: sage((xs, None), ei, None, (None, 5)),
             lambda: sage(xd, ei, size=(5, 5)), lambda: sagec((xs, xd), ei, None, None, torch.tensor([0, 1, 2, 3, 6])),
             lambda: gat((xs, xd), ei), lambda: gat((xs, None), ei, size=(7, 5)), lambda: gat(xd, ei, size=(5, 5)),
             lambda: npi.GATConv(8, 4, dropout=0.5).eval()((xs, xd), ei), lambda: npi.BipartiteGraph(ei, (7, 5))]
    for call in calls:
        with pytest.raises(npi.NpiError):
            call()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_rows_gather_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+npi_rows_gather\s*\(", text)
    assert "torch.cat([x[0][res_n_id], aggr_out], dim=-1)" in header              # the PyG line it replaces
    assert "npi_rows_gather" in _lib.PROTOTYPES
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "npi_rows_gather")
    assert lib.npi_abi_version() == 4
    # argument errors come back before anything is launched
    assert lib.npi_rows_gather(None, 4, 4, None, 4, 8, None, 8, 0, None, None) == -1      # ldx < F
    assert b"npi_rows_gather" in lib.npi_last_error()
    assert lib.npi_rows_gather(None, 8, 4, None, 4, 8, None, 8, 7, None, None) == -1      # no such dtype
    assert lib.npi_rows_gather(None, 8, 4, None, 0, 8, None, 8, 0, None, None) == 0       # n == 0: nothing to do


def test_boundary_consistency_checks_hold_with_the_new_symbol():
    import test_boundary_cpu as B
    B.test_every_declared_symbol_is_exported_and_bound()
    B.test_ctypes_prototypes_have_the_headers_argument_lists()
    B.test_the_library_allocates_nothing_and_keeps_no_state()
    B.test_product_package_never_imports_the_oracle()
    B.test_no_module_level_switch_on_the_layer_path()
