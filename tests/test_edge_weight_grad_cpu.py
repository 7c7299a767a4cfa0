"""No GPU: the entry points behind ``d edge_weight`` (``npi_edge_dot``, ``npi_gcn_norm_bwd``, csrc/edge_dot.hip) refuse bad sizes
and null pointers before anything is launched -- status -1, the message names the entry point -- and the layers' refusals that
need no device.  Header / prototype sync is covered by tests/test_boundary_cpu.py once the declarations exist."""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib

N = None


def _dot(lib, rowptr=8, col=8, rowidx=8, eid=8, n=4, n_cols=4, nnz=16, e=12, a=8, lda=4, b=8, ldb=4, f=4, rs=N, mul=N, g=8, gm=N, de=N,
         dl=N):
    return lib.npi_edge_dot(rowptr, col, rowidx, eid, n, n_cols, nnz, e, a, lda, b, ldb, f, rs, mul, g, gm, de, dl, N)


def _nbwd(lib, rowptr=8, col=8, rowidx=8, eid=8, n=4, nnz=16, e=12, g=8, deg=8, sa=8, sb=N, de=8, dl=N):
    return lib.npi_gcn_norm_bwd(rowptr, col, rowidx, eid, n, nnz, e, g, deg, sa, sb, de, dl, N)


@pytest.mark.parametrize("kw", [{"n": -1}, {"n_cols": -1}, {"nnz": -1}, {"e": -1}, {"f": 0}, {"f": -4}, {"lda": 3}, {"ldb": 3},
                                {"n": 1 << 31}, {"nnz": 1 << 31}, {"e": 1 << 31},
                                {"rowptr": N}, {"col": N}, {"rowidx": N}, {"a": N}, {"b": N}, {"g": N},      # (g: then no output at all)
                                {"eid": N, "de": 8}, {"eid": N, "dl": 8}, {"mul": 8}, {"gm": 8}],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_edge_dot_rejects_bad_arguments(kw):
    lib = _lib.load()
    assert _dot(lib, **kw) == -1, kw
    assert b"npi_edge_dot" in lib.npi_last_error()


def test_edge_dot_with_nothing_to_do_returns_ok():
    lib = _lib.load()
    assert _dot(lib, nnz=0, rowptr=N, col=N, rowidx=N, a=N, b=N, g=N) == 0
    assert _dot(lib, n=0, rowptr=N, col=N, rowidx=N, a=N, b=N, g=N) == 0


@pytest.mark.parametrize("kw", [{"n": -1}, {"nnz": -1}, {"e": -1}, {"n": 1 << 31}, {"e": 1 << 31},
                                {"rowptr": N}, {"col": N}, {"rowidx": N}, {"eid": N}, {"g": N}, {"deg": N}, {"sa": N}, {"de": N}],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_gcn_norm_bwd_rejects_bad_arguments(kw):
    lib = _lib.load()
    assert _nbwd(lib, **kw) == -1, kw
    assert b"npi_gcn_norm_bwd" in lib.npi_last_error()
    assert _nbwd(lib, nnz=0, rowptr=N) == 0


def test_abi_version_is_unchanged():
    assert _lib.load().npi_abi_version() == 4          # additive: two new entry points, no existing one changed


def test_differentiable_weight_still_needs_the_gpu():
    """no CPU fallback for the new path either, and the refusal is no longer NotImplementedError"""
    x, W = torch.randn(5, 8), torch.randn(8, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    w = torch.rand(3, requires_grad=True)
    for fn in (npi.sage_conv, npi.gcn_conv):
        with pytest.raises(npi.NpiError):
            fn(x, ei, W, edge_weight=w)
