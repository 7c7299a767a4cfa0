"""Seeded attention dropout (Rule D) without a GPU: the rule's known answers and dropped fraction from the reference alone, the four
new symbols, the unchanged ABI version, every new entry point refusing arguments outside its contract with ``NPI_ERR_ARG`` before
anything is launched (the arguments are checked on the host; no pointer is followed), and the Python-side argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _gat_dropout_ref as D
from npi_gnn_amd import _lib
from npi_gnn_amd import functional as NF
from npi_gnn_amd import nn as NN

NPI_ERR_ARG = -1
A = 0x10000                      # a 16-byte aligned stand-in for every pointer: never dereferenced by a refused call
KEY, T, SCALE = 12345, D.threshold(0.5) - (1 << 64), 2.0        # T travels as the int64 with its bits (2^63 -> -2^63)
NEW = ("npi_gat_aggregate_fused_heads_dropout", "npi_gat_backward_fused_heads_dropout", "npi_gat_edge_grad_dropout",
       "npi_gat_dropout_keep")


def test_known_answers():
    assert D.root(0, 0) == 0x6F163EDB947C9E05
    assert D.threshold(0.6) == 11068046444225730560
    want = {0: (0x16487DC5AE5A7950, 0x36D77E7754A4D63D, True), 1: (0xEDEFF920902A8EC7, 0xB36D8FB43721E4F1, False),
            1 << 32: (0x219C474DE52E9ABD, 0x269B94D91227E886, True)}
    rt, thr = D.root(0, 0), D.threshold(0.6)
    for k, (w0, w1, dropped) in want.items():
        assert (D.word(rt, k, 0), D.word(rt, k, 1)) == (w0, w1), k
        assert (D.word(rt, k, 0) < thr, D.word(rt, k, 1) < thr) == (dropped, dropped), k
    # the numpy form is the same function
    ks = [0, 1, 1 << 32]
    assert D.words_np(0, 0, ks, 2).tolist() == [[want[k][0], want[k][1]] for k in ks]
    keep = D.keep_np(0, 0, 0.6, ks, 2)
    assert keep.dtype == np.float32 and keep.tolist() == [[0.0, 0.0], [float(np.float32(2.5)), float(np.float32(2.5))], [0.0, 0.0]]
    # a self loop's slot, and the host side of the package says the same key / threshold / scale
    assert D.slots([5, -1], [9, 7]).tolist() == [5, (1 << 32) + 7]
    rule = NF.AttentionDropout(0.6, 0, 0)
    assert rule.key & D.M64 == D.epoch_seed(0, 0) and rule.threshold == D.threshold(0.6) and rule.scale == float(D.scale(0.6))
    assert NF.AttentionDropout(0.0, 3, 1).threshold == 0 and NF.AttentionDropout(0.0, 3, 1).scale == 1.0


@pytest.mark.parametrize("seed,draw", [(0, 0), (1, 3), (12345, 7)])
@pytest.mark.parametrize("n,H,p", [(360, 1, 0.4), (13500, 2, 0.4), (43000, 1, 0.6), (2000, 8, 0.6)])
def test_dropped_fraction(n, H, p, seed, draw):
    """over the slots k < n and H heads the dropped fraction lies within 4 binomial standard deviations of p"""
    dropped = D.keep_np(seed, draw, p, np.arange(n), H) == 0
    z = (float(dropped.mean()) - p) / math.sqrt(p * (1 - p) / (n * H))
    assert abs(z) <= 4.0, z


def test_symbols_and_abi_version():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    assert lib.npi_abi_version() == 4                                   # an additive change


def _fwd(lib, H, C, eid=A, att=A, row_scales=None, item=64):
    return lib.npi_gat_aggregate_fused_heads_dropout(A, A, A, A, item, 100, 1000, A, H * C, None, 0, A, H * C, H, C, A, att, 0.2, A, 0,
                                                     A, A, A, row_scales, None, eid, KEY, T, SCALE)


def _bwd(lib, H, C, eid=A, item=64, g_src=None):
    return lib.npi_gat_backward_fused_heads_dropout(A, A, A, A, item, 100, 1000, A, H * C, None, 0, A, H * C, A, H * C, H, C, A, A, 0.2,
                                                    A, A, None, g_src, None, 0, None, eid, KEY, T, SCALE)


def _edge(lib, H, C, eid=A, ldh=None):
    return lib.npi_gat_edge_grad_dropout(A, A, A, 100, 1000, A, H * C if ldh is None else ldh, None, 0, A, H * C, H, C, A, A, A, A, A,
                                         0.2, 0, A, None, None, eid, KEY, T, SCALE)


def test_arguments_outside_the_contract_are_refused_before_a_launch():
    lib = _lib.load()
    cases = {
        "forward": (_fwd, "npi_gat_aggregate_fused", {
            "three heads": dict(H=3, C=32), "48 channels": dict(H=2, C=48), "H C = 512": dict(H=4, C=128),
            "one head of 300": dict(H=1, C=300), "row scales with two heads": dict(H=2, C=128, row_scales=A),
            "misaligned att": dict(H=4, C=64, att=A + 4), "bad item size": dict(H=4, C=64, item=100),
            "null eid": dict(H=4, C=64, eid=None), "null eid, one head": dict(H=1, C=64, eid=None)}),
        "backward": (_bwd, "npi_gat_backward_fused_heads", {
            "three heads": dict(H=3, C=32), "48 channels": dict(H=2, C=48), "H C = 512": dict(H=4, C=128),
            "C % 4": dict(H=1, C=30), "bad item size": dict(H=4, C=64, item=100), "row sums with two heads": dict(H=2, C=64, g_src=A),
            "null eid": dict(H=4, C=64, eid=None), "null eid, one head": dict(H=1, C=256, eid=None)}),
        "edge grad": (_edge, "npi_gat_edge_grad", {
            "C % 4": dict(H=1, C=30), "H C > 1024": dict(H=8, C=256), "pitch % 4": dict(H=1, C=64, ldh=66),
            "null eid": dict(H=3, C=16, eid=None)}),
    }
    for which, (call, who, shapes) in cases.items():
        for name, kw in shapes.items():
            assert call(lib, **kw) == NPI_ERR_ARG, (which, name)
            msg = lib.npi_last_error().decode()
            assert who in msg, (which, name, msg)
    # the mask itself
    keep = lib.npi_gat_dropout_keep
    assert keep(A, A, A, 100, 1000, 0, KEY, T, SCALE, A, None) == NPI_ERR_ARG            # no heads
    assert keep(A, A, A, 100, 1000, 65, KEY, T, SCALE, A, None) == NPI_ERR_ARG           # more heads than the rule's words per slot here
    assert keep(A, A, None, 100, 1000, 2, KEY, T, SCALE, A, None) == NPI_ERR_ARG         # null eid
    assert keep(A, A, A, 100, 1000, 2, KEY, T, SCALE, None, None) == NPI_ERR_ARG         # null output
    assert "npi_gat_dropout_keep" in lib.npi_last_error().decode()
    assert keep(A, A, A, -1, 1000, 2, KEY, T, SCALE, A, None) == NPI_ERR_ARG


def test_python_argument_checks():
    with pytest.raises(ValueError):
        NN.GATConv(8, 4, dropout=0.5, seed="x")
    with pytest.raises(ValueError):
        NN.GATConv(8, 4, dropout=0.5, seed=True)
    with pytest.raises(ValueError):
        NF.AttentionDropout(p=1.0, seed=0, draw=0)
    with pytest.raises(ValueError):
        NF.AttentionDropout(p=-0.1, seed=0)
    with pytest.raises(ValueError):
        NF.AttentionDropout(p=0.5, seed=0.5)
    with pytest.raises(ValueError):
        NF.AttentionDropout(p=0.5, seed=0, draw=-1)
    with pytest.raises(Exception):                      # frozen
        NF.AttentionDropout(0.5, 0).p = 0.1
    conv = NN.GATConv(8, 4, dropout=0.5, seed=3)
    assert conv.draw == 0 and conv.seed == 3
    conv.draw = 5
    assert conv.draw == 5
    assert "seed" not in conv.state_dict() and "draw" not in conv.state_dict()
    assert sorted(conv.state_dict()) == ["att", "bias", "weight"]
    assert repr(conv) == repr(NN.GATConv(8, 4, dropout=0.5)) == "GATConv(8, 4, heads=1)"
    assert not hasattr(NN.GATConv(8, 4, dropout=0.5), "draw")


def test_unseeded_module_still_refuses_the_bipartite_form_in_training():
    conv = NN.GATConv(8, 4, dropout=0.5).train()
    x = (torch.zeros(5, 8), torch.zeros(3, 8))
    ei = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        conv(x, ei)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        conv(torch.zeros(5, 8), ei, size=(5, 5))
