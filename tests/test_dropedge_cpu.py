"""DropEdge (Rule E) without a GPU: the rule's known answers from two independent restatements, the thresholds as exact integers, the
kept share and the independence of draws / ticks / modes from the reference alone, the undirected mode's symmetry, the new symbols
with the unchanged ABI version, the entry points refusing arguments outside their contract before anything is launched (checked on
the host; no pointer is followed), and the Python-side argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _dropedge_ref as R
import npi_gnn_amd as npi
from npi_gnn_amd import _lib, dropedge
from npi_gnn_amd.graph import BipartiteGraph, CSRGraph

NPI_ERR_ARG = -1
A = 0x10000                      # an aligned stand-in for every pointer: never dereferenced by a refused call
NEW = ("npi_csr_drop_side", "npi_drop_edge_list", "npi_drop_edge_keep", "npi_drop_edges_workspace_elems")
E_SHARE = 200_000


def _edges(E, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, E), rng.integers(0, n, E)


def test_known_answers():
    K = R.KNOWN
    assert (R.key_of(0, 0), R.root_of(0, 0), R.root_t_of(0, 0, 0), R.root_t_of(0, 0, 1)) == \
        (K["key"], K["root"], K["root_t0"], K["root_t1"])
    assert R.roots_int(0, 0) == (K["key"], K["root"], K["root_t0"], K["root_t1"])          # the restatement in Python ints
    # slots 0 and 1: directed columns 0, 1; undirected the pairs (0, 0), (0, 1) -- and (1, 0), the same pair
    assert tuple(int(w) for w in R.words([0, 0], [0, 1])) == K["directed"]
    assert tuple(int(w) for w in R.words([0, 0, 1], [0, 1, 0], undirected=True)) == K["undirected"] + K["undirected"][1:]
    assert tuple(R.word_int(k) for k in (0, 1)) == K["directed"]
    assert tuple(R.word_int(k, undirected=True) for k in (0, 1)) == K["undirected"]
    # the two restatements agree away from the pinned point as well
    src, dst = _edges(64, 1000, 1)
    for und in (False, True):
        ks = R.slots(src, dst, und)
        assert [int(w) for w in R.words(src, dst, 7, 3, 5, und)] == [R.word_int(int(k), 7, 3, 5, und) for k in ks]
    assert int(R.slots([5], [3], True)[0]) == (3 << 32) + 5


def test_thresholds_exact():
    assert R.threshold(0.5) == 1 << 63 == R.KNOWN["T"][0.5]
    assert R.threshold(0.3) == 5534023222112865280 == (5404319552844595 << 64) >> 54      # 0.3 = 5404319552844595 / 2^54
    assert R.threshold(1 - 2.0 ** -53) == (1 << 64) - (1 << 11) == 18446744073709549568
    assert R.threshold(0.0) == 0
    for p in (0.5, 0.3, 1 - 2.0 ** -53, 0.0):
        assert dropedge.threshold(p) == R.threshold(p)                  # the host side of the package says the same


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_kept_share(p, seed):
    """E = 200,000: the kept share lies within 5 binomial standard deviations of 1 - p (about 0.0034 / 0.0056 / 0.0034)"""
    src, dst = _edges(E_SHARE, 50_000, seed)
    sigma = math.sqrt(p * (1 - p) / E_SHARE)
    for und in (False, True):
        share = float(R.keep_mask(src, dst, p, seed, 0, 0, und).mean())
        # (undirected: the pairs are the trials; 200,000 draws over 1.25e9 pairs repeat a pair a handful of times at most)
        assert abs(share - (1 - p)) <= 5 * sigma, (und, share)


def test_undirected_pairs_agree():
    src, dst = _edges(5000, 300, 2)                                       # 5000 columns over 45,000 pairs: parallel duplicates occur
    s = np.concatenate([src, dst, src])
    d = np.concatenate([dst, src, dst])
    m = R.keep_mask(s, d, 0.5, 3, 1, 2, True)
    assert (m[:5000] == m[5000:10000]).all() and (m[:5000] == m[10000:]).all()
    slot = R.slots(src, dst, True)
    _, first, inv = np.unique(slot, return_index=True, return_inverse=True)
    assert len(first) < 5000 and (m[:5000] == m[:5000][first][inv]).all()
    # directed mode is keyed on the column, not on the ends
    md = R.keep_mask(s, d, 0.5, 3, 1, 2, False)
    assert (md[:5000] != md[5000:10000]).any()


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_draws_ticks_modes_are_independent(p):
    """masks of another draw / tick / mode / seed agree on a share within 5 sigma of p^2 + (1 - p)^2"""
    src, dst = _edges(E_SHARE, 50_000, 4)
    base = R.keep_mask(src, dst, p, 0, 0, 0, False)
    q = p * p + (1 - p) * (1 - p)
    sigma = math.sqrt(q * (1 - q) / E_SHARE)
    for name, other in (("draw", R.keep_mask(src, dst, p, 0, 1, 0, False)), ("tick", R.keep_mask(src, dst, p, 0, 0, 1, False)),
                        ("mode", R.keep_mask(src, dst, p, 0, 0, 0, True)), ("seed", R.keep_mask(src, dst, p, 1, 0, 0, False))):
        agree = float((base == other).mean())
        assert abs(agree - q) <= 5 * sigma, (name, agree)


def test_symbols_and_abi_version():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    assert lib.npi_abi_version() == 4                                   # an additive change
    assert _lib.NPI_DROP_UNDIRECTED == 1
    for name in ("DropEdge", "dropout_adj", "drop_edge_mask"):
        assert name in npi.__all__ and hasattr(npi, name)
    assert hasattr(CSRGraph, "drop_edges") and hasattr(BipartiteGraph, "drop_edges")
    assert lib.npi_drop_edges_workspace_elems(-1) == -1
    assert lib.npi_drop_edges_workspace_elems(0) == 2                   # the total word and one word of the scan
    assert lib.npi_drop_edges_workspace_elems(257) == 3 + 1


def side_args(**kw):
    a = dict(rowptr=A, col=A, eid=A, rowidx=A, N=10, nnz_max=100, n_edges=90, key=1, tick=0, T=1 << 62, flags=0, nnz_max_out=100, item=64,
             rowptr_o=A + 0x1000, col_o=A + 0x2000, eid_o=A + 0x3000, rowidx_o=A + 0x4000, item_row_o=A + 0x5000, ws=A + 0x6000, ws_n=None)
    a.update(kw)
    if a["ws_n"] is None:
        a["ws_n"] = int(_lib.load().npi_drop_edges_workspace_elems(max(a["nnz_max"], 0)))
    return [a[k] for k in ("rowptr", "col", "eid", "rowidx", "N", "nnz_max", "n_edges", "key", "tick", "T", "flags", "nnz_max_out", "item",
                           "rowptr_o", "col_o", "eid_o", "rowidx_o", "item_row_o", "ws", "ws_n")] + [0]


def list_args(**kw):
    a = dict(src=A, dst=A + 0x1000, E=100, key=1, tick=0, T=1 << 62, flags=0, out_src=A + 0x2000, out_dst=A + 0x3000, newpos=0,
             count=A + 0x4000, pad=0, ws=A + 0x5000, ws_n=None)
    a.update(kw)
    if a["ws_n"] is None:
        a["ws_n"] = int(_lib.load().npi_drop_edges_workspace_elems(max(a["E"], 0)))
    return [a[k] for k in ("src", "dst", "E", "key", "tick", "T", "flags", "out_src", "out_dst", "newpos", "count", "pad", "ws", "ws_n")] + [0]


SIDE_REFUSALS = [dict(rowptr=0), dict(col=0), dict(eid=0), dict(rowidx=0), dict(rowptr_o=0), dict(col_o=0), dict(eid_o=0),
                 dict(rowidx_o=0), dict(item_row_o=0), dict(ws=0), dict(N=-1), dict(nnz_max=-1), dict(n_edges=-1), dict(nnz_max=2 ** 31),
                 dict(nnz_max_out=99), dict(item=128), dict(item=0), dict(flags=2), dict(ws=A + 0x6002), dict(ws=A + 0x6001), dict(ws_n=1),
                 dict(col_o=A)]
LIST_REFUSALS = [dict(src=0), dict(dst=0), dict(out_src=0), dict(out_dst=0), dict(count=0), dict(ws=0), dict(E=-1), dict(E=2 ** 31),
                 dict(flags=4), dict(ws=A + 0x5002), dict(ws_n=1), dict(out_src=A)]


@pytest.mark.parametrize("bad", SIDE_REFUSALS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_drop_side_refuses(bad):
    lib = _lib.load()
    assert lib.npi_csr_drop_side(*side_args(**bad)) == NPI_ERR_ARG
    assert b"npi_csr_drop_side" in lib.npi_last_error()


@pytest.mark.parametrize("bad", LIST_REFUSALS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_drop_list_refuses(bad):
    lib = _lib.load()
    assert lib.npi_drop_edge_list(*list_args(**bad)) == NPI_ERR_ARG
    assert b"npi_drop_edge_list" in lib.npi_last_error()


def test_drop_keep_refuses():
    lib = _lib.load()
    assert lib.npi_drop_edge_keep(A, A, 10, 1, 0, 1, 0, 0, 0) == NPI_ERR_ARG                       # keep NULL
    assert lib.npi_drop_edge_keep(0, A, 10, 1, 0, 1, 1, A, 0) == NPI_ERR_ARG                       # undirected needs the ends
    assert lib.npi_drop_edge_keep(A, A, -1, 1, 0, 1, 0, A, 0) == NPI_ERR_ARG
    assert lib.npi_drop_edge_keep(A, A, 10, 1, 0, 1, 8, A, 0) == NPI_ERR_ARG
    assert lib.npi_drop_edge_keep(0, 0, 0, 1, 0, 1, 0, 0, 0) == 0                                  # no columns: nothing to do


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan"), True, "0.5", None])
def test_p_refused(p):
    ei = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError):
        npi.dropout_adj(ei, p=p)
    with pytest.raises(ValueError):
        npi.drop_edge_mask(ei, p)
    with pytest.raises(ValueError):
        npi.DropEdge(p)
    for cls in (CSRGraph, BipartiteGraph):                                # (refused before the graph is looked at)
        with pytest.raises(ValueError):
            object.__new__(cls).drop_edges(p)


def test_python_argument_checks():
    with pytest.raises(ValueError, match="undirected"):
        object.__new__(BipartiteGraph).drop_edges(0.5, undirected=True)
    ei = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError):
        npi.dropout_adj(ei.to(torch.int32), p=0.5)
    with pytest.raises(ValueError):
        npi.dropout_adj(ei, p=0.5, seed=1.5)
    with pytest.raises(ValueError):
        npi.dropout_adj(ei, p=0.5, draw=-1)
    with pytest.raises(ValueError):
        npi.dropout_adj(ei, p=0.5, tick=torch.zeros(1, dtype=torch.int64))            # a host tensor is no device word
    with pytest.raises(_lib.NpiError):
        npi.dropout_adj(ei, p=0.5)                                                    # no CPU fallback
    # eval and p = 0 are the identity and need no device
    assert npi.dropout_adj(ei, p=0.5, training=False)[0] is ei
    m = npi.DropEdge(0.5, seed=3).eval()
    assert m.draw == 0 and "p=0.5" in repr(m)
