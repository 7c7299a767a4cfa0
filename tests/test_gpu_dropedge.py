"""DropEdge (Rule E) on the device: the mask against the numpy rule bit for bit, both sides of ``drop_edges`` against a FRESH build
over the reference-filtered edge list (shapes at the compaction's edges: a tile is 256 entries), ``dropout_adj`` over the list, the
layers on a dropped graph bitwise equal to the same layers on the freshly built filtered graph, reproducibility, ``out=`` reuse, a
captured step that draws a new mask per replay from the tick word, and the refusals of the C ABI."""
import numpy as np
import pytest
import torch

import _dropedge_ref as R
import _gat_dropout_ref as D
import npi_gnn_amd as npi
from _util import GRAD_REL, rel_max
from npi_gnn_amd import _lib, dropedge
from npi_gnn_amd import functional as NF
from npi_gnn_amd import graph as NG
from npi_gnn_amd._draw import epoch_seed
from npi_gnn_amd._lib import ptr, stream_ptr
from oracle import ref_conv as O

pytestmark = pytest.mark.gpu

TILE = 256                       # entries one wavefront compacts (csrc/dropedge.hip)
NPI_ERR_ARG = -1
SEED, DRAW = 5, 2


def _np(t):
    return t.detach().cpu().numpy()


def _ref_mask(ei, p, undirected=False, tick=0, seed=SEED, draw=DRAW):
    a = ei.numpy()
    return R.keep_mask(a[0], a[1], p, seed, draw, tick, undirected)


def _same_side(got, want, kept_idx, E, what):
    """``got``: a side drop_edges made (the parent's capacity, the parent's column numbers); ``want``: the fresh build's"""
    N, E_kept = want.n_rows, len(kept_idx)
    assert got.n_rows == N and got.n_cols == want.n_cols and got.item == want.item, what
    rp = _np(want.rowptr)
    nnz = int(rp[-1])
    assert np.array_equal(_np(got.rowptr), rp), what
    assert np.array_equal(_np(got.col)[:nnz], _np(want.col)[:nnz]), what
    assert np.array_equal(_np(got.rowidx)[:nnz], _np(want.rowidx)[:nnz]), what
    fe = _np(want.eid)[:nnz].astype(np.int64)
    edge = (fe >= 0) & (fe < E_kept)
    parent_eid = np.where(edge, np.asarray(kept_idx, dtype=np.int64)[np.clip(fe, 0, max(E_kept - 1, 0))] if E_kept else fe,
                          np.where(fe >= E_kept, fe - E_kept + E, fe))             # loops stay -1, root entries E_kept + i -> E + i
    assert np.array_equal(_np(got.eid)[:nnz].astype(np.int64), parent_eid), what
    # item_row: the fresh side's on the items that hold entries; behind them what write_item_rows gives this capacity (N; item 0: 0)
    gi, wi = _np(got.item_row), _np(want.item_row)
    hold = -(-nnz // got.item)
    assert gi.shape[0] == got.n_items + 1 and got.n_items == int(_lib.load().npi_num_items(got.nnz_max, got.item))
    assert np.array_equal(gi[:hold], wi[:hold]), what
    assert gi[0] == 0 and (gi[max(hold, 1):] == N).all(), what
    return nnz


def _check_graph(dev, ei, make, p, undirected=False, tick=None):
    """``make(edge_index)`` builds the graph; both sides of its drop against the fresh build over the reference-filtered list"""
    parent = make(ei.to(dev))
    tk = None if tick is None else torch.tensor([tick], dtype=torch.int64, device=dev)
    g = parent.drop_edges(p, seed=SEED, draw=DRAW, tick=tk, undirected=undirected)
    mask = _ref_mask(ei, p, undirected, tick or 0)
    if p == 0:
        assert g is parent
        return parent, g, mask
    assert g is not parent and g.dropped_from is parent and g.num_edges == parent.num_edges and g._src is parent._src
    kept_idx = np.nonzero(mask)[0]
    fresh = make(ei[:, torch.from_numpy(mask)].to(dev))
    E = ei.size(1)
    for which in ("by_dst", "by_src"):
        got, want = getattr(g, which), getattr(fresh, which)
        assert got.nnz_max == getattr(parent, which).nnz_max and got._hub_asked and got.hub_plan() is None
        _same_side(got, want, kept_idx, E, (which, p, undirected))
    NG.pending_status()                                   # (lists with out-of-range ids: their status words are not this test's subject)
    return parent, g, mask


def _rand_ei(E, n_src, n_dst, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])


# ---- 1. the mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("undirected", [False, True])
def test_mask_on_the_device_is_the_numpy_rule(dev, undirected):
    ei = _rand_ei(3 * TILE + 5, 40, 40, 1)
    ei[:, 100:140] = ei[:, 200:240].flip(0)               # mirrored columns
    ei[:, 300:320] = ei[:, 400:420]                       # parallel duplicates
    ei[1, :20] = ei[0, :20]                               # (i, i) columns
    ei[:, 50:55] = -1                                     # padding
    ei[0, 60:63] = 1 << 33                                # out of range: the rule is over the columns, whatever they hold
    for p in (0.3, 0.999, 0.0):
        for tick in (0, 5):
            tk = torch.tensor([tick], dtype=torch.int64, device=dev)
            got = npi.drop_edge_mask(ei.to(dev), p, seed=SEED, draw=DRAW, tick=tk, undirected=undirected)
            assert got.dtype == torch.bool and np.array_equal(_np(got), _ref_mask(ei, p, undirected, tick)), (p, tick)
        assert torch.equal(npi.drop_edge_mask(ei.to(dev), p, seed=SEED, draw=DRAW, undirected=undirected),
                           npi.drop_edge_mask(ei.to(dev), p, seed=SEED, draw=DRAW, tick=torch.zeros(1, dtype=torch.int64, device=dev),
                                              undirected=undirected))
    m = _ref_mask(ei, 0.3, undirected)
    if undirected:
        assert np.array_equal(m[100:140], m[200:240]) and np.array_equal(m[300:320], m[400:420])
    assert npi.drop_edge_mask(ei[:, :0].to(dev), 0.3).shape == (0,)


# ---- 2. the sides ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", [64, 256])
@pytest.mark.parametrize("nnz", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_sides_at_the_tile_edges(dev, nnz, item):
    """the list as it is (no loop appended, nothing dropped by the build): nnz entries exactly, over 1, 7 and 300 rows"""
    for N in (1, 7, 300):
        ei = _rand_ei(nnz, N, N, nnz + N)
        for p in (0.3, 0.999):
            _check_graph(dev, ei, lambda e: npi.CSRGraph(e, N, self_loops=False, keep_equal=True, item=item), p, undirected=(N == 7))


@pytest.mark.parametrize("p", [0.0, 0.3, 0.999])
@pytest.mark.parametrize("item", [64, 256])
def test_sides_hub_row_among_short_rows(dev, p, item):
    """(a) one row of 5,000 entries: a row cut by ~20 tile boundaries; with the appended self loops, both modes, a tick word"""
    N = 600
    ei = _rand_ei(7000, N, N, 7)
    ei[1, 1000:6000] = 3
    ei[0, 1000:6000][ei[0, 1000:6000] == 3] = 4           # (none of them an (i, i) column, which the build drops)
    for undirected, tick in ((False, None), (True, 5)):
        parent, g, _ = _check_graph(dev, ei, lambda e: npi.CSRGraph(e, N, item=item), p, undirected, tick)
    assert int((parent.by_dst.rowptr[1:] - parent.by_dst.rowptr[:-1]).max()) > 5000


@pytest.mark.parametrize("p", [0.3, 0.999])
def test_sides_bipartite_long_runs_of_empty_rows(dev, p):
    """(b) 3,000 targets of which 3 have edges: runs of empty rows far longer than a tile, and the root side (its root entries stay)"""
    n_src, n_dst = 50, 3000
    ei = _rand_ei(900, n_src, n_dst, 3)
    ei[1] = torch.tensor([10, 1500, 2990])[torch.arange(900) % 3]
    for item in (64, 256):
        parent, g, mask = _check_graph(dev, ei, lambda e: npi.BipartiteGraph(e, (n_src, n_dst), item=item), p)
        res = torch.randint(0, n_src, (n_dst,), generator=torch.Generator().manual_seed(1)).to(dev)
        fresh = npi.BipartiteGraph(ei[:, torch.from_numpy(mask)].to(dev), (n_src, n_dst), item=item)
        nnz = _same_side(g.root_side(res), fresh.root_side(res), np.nonzero(mask)[0], 900, "root_side")
        assert nnz == int(mask.sum()) + n_dst and g.root_side(res) is g.root_side(res)
        with pytest.raises(ValueError, match="pair_side"):
            g.pair_side()
    with pytest.raises(ValueError, match="undirected"):
        parent.drop_edges(p, undirected=True)


@pytest.mark.parametrize("sort_columns", [False, True])
@pytest.mark.parametrize("p", [0.3, 0.999])
def test_sides_messy_list_and_sorted_columns(dev, p, sort_columns):
    """(c) parallel duplicates, (i, i) columns, out-of-range and (-1, -1) columns; (d) sort_columns=True"""
    N = 90
    ei = _rand_ei(3 * TILE + 5, N, N, 11)
    ei[:, 300:360] = ei[:, 400:460]
    ei[:, 500:540] = ei[:, 600:640].flip(0)
    ei[1, :30] = ei[0, :30]
    ei[:, 70:80] = -1
    ei[0, 90:95] = N + 3
    ei[1, 95:99] = 1 << 31
    for undirected in (False, True):
        _check_graph(dev, ei, lambda e: npi.CSRGraph(e, N, sort_columns=sort_columns, item=64), p, undirected)
    NG.pending_status()


def test_threshold_zero_reproduces_the_parent(dev):
    """a direct ABI call with T = 0: the parent's arrays bit for bit (and entries behind nnz are not touched)"""
    lib = _lib.load()
    N = 300
    ei = _rand_ei(3 * TILE + 5, N, N, 2)
    ei[:, 40:60] = -1                                    # dropped by the build: nnz < nnz_max
    side = npi.CSRGraph(ei.to(dev), N, item=64).by_src
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr, item_row = torch.full((N + 1,), -7, **i32), torch.full((side.n_items + 1,), -7, **i32)
    col, eid, rowidx = (torch.full((side.nnz_max,), -7, **i32) for _ in range(3))
    ws_n = int(lib.npi_drop_edges_workspace_elems(side.nnz_max))
    ws = torch.empty(ws_n, **i32)
    for flags in (0, 1):
        rc = lib.npi_csr_drop_side(ptr(side.rowptr), ptr(side.col), ptr(side.eid), ptr(side.rowidx), N, side.nnz_max, ei.size(1),
                                   epoch_seed(SEED, DRAW), 0, 0, flags, side.nnz_max, 64, ptr(rowptr), ptr(col), ptr(eid), ptr(rowidx),
                                   ptr(item_row), ptr(ws), ws_n, stream_ptr(dev))
        assert rc == 0
        nnz = int(side.rowptr[-1])
        assert nnz <= side.nnz_max - 20                      # (the padding columns and the list's (i, i) columns have no entry)
        assert torch.equal(rowptr, side.rowptr) and torch.equal(item_row, side.item_row)
        for got, want in ((col, side.col), (eid, side.eid), (rowidx, side.rowidx)):
            assert torch.equal(got[:nnz], want[:nnz]) and bool((got[nnz:] == -7).all())
    NG.pending_status()


# ---- 3. the list -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("undirected", [False, True])
@pytest.mark.parametrize("E", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_dropout_adj(dev, E, undirected):
    ei = _rand_ei(E, 30, 30, E)
    if E > 300:
        ei[:, 100:140] = ei[:, 200:240].flip(0)
        ei[1, :20] = ei[0, :20]                           # (i, i) columns take part here, as in PyG
        ei[:, 50:55] = -1
    attr = torch.arange(E * 3, dtype=torch.float32).view(E, 3) + 1
    for p in (0.3, 0.999):
        want, mask = R.filtered(ei.numpy(), p, SEED, DRAW, 0, undirected)
        out, oattr = npi.dropout_adj(ei.to(dev), attr.to(dev), p=p, force_undirected=undirected, seed=SEED, draw=DRAW)
        assert out.dtype == torch.int64 and np.array_equal(_np(out), want)
        assert torch.equal(oattr.cpu(), attr[torch.from_numpy(mask)])
        assert npi.dropout_adj(ei.to(dev), p=p, force_undirected=undirected, seed=SEED, draw=DRAW)[1] is None
        # pad=True: the length stays E, the same prefix, (-1, -1) behind it, nothing read back
        pout, pattr = npi.dropout_adj(ei.to(dev), attr.to(dev), p=p, force_undirected=undirected, seed=SEED, draw=DRAW, pad=True)
        n = int(mask.sum())
        assert pout.shape == (2, E) and np.array_equal(_np(pout)[:, :n], want) and bool((pout[:, n:] == -1).all())
        assert torch.equal(pattr[:n].cpu(), attr[torch.from_numpy(mask)]) and float(pattr[n:].abs().sum()) == 0.0
    dei = ei.to(dev)
    assert npi.dropout_adj(dei, p=0.5, training=False)[0] is dei and npi.dropout_adj(dei, p=0.0)[0] is dei


def test_drop_edge_list_count_and_newpos(dev):
    """the ABI call itself: count, newpos (-1 for a dropped column), with a tick word"""
    lib = _lib.load()
    E = 3 * TILE + 5
    ei = _rand_ei(E, 30, 30, 4).to(dev)
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    out = torch.full((2, E), -9, dtype=torch.int64, device=dev)
    newpos, count = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    tick = torch.tensor([5], dtype=torch.int64, device=dev)
    ws_n = int(lib.npi_drop_edges_workspace_elems(E))
    ws = torch.empty(ws_n, dtype=torch.int32, device=dev)
    for pad in (0, 1):
        assert lib.npi_drop_edge_list(ptr(src), ptr(dst), E, epoch_seed(SEED, DRAW), ptr(tick), dropedge.threshold(0.3), 0, ptr(out[0]),
                                      ptr(out[1]), ptr(newpos), ptr(count), pad, ptr(ws), ws_n, stream_ptr(dev)) == 0
        mask = _ref_mask(ei.cpu(), 0.3, False, 5)
        n = int(mask.sum())
        assert int(count) == n
        want_pos = np.where(mask, np.cumsum(mask) - 1, -1)
        assert np.array_equal(_np(newpos), want_pos)
        assert bool((out[:, n:] == (-1 if pad else -9)).all())


# ---- 4. the layers -----------------------------------------------------------------------------------------------------------------
N_L, E_L, F_L = 700, 9000, 32


def _layer_case(seed=0):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N_L, (E_L,), generator=g)
    src[: E_L // 3] = (4 + torch.arange(E_L // 3)) % N_L
    src[src == 3] = 5
    dst = (src + 1 + torch.randint(0, N_L - 1, (E_L,), generator=g)) % N_L            # no (i, i) column: see CSRGraph.drop_edges
    dst[: E_L // 3] = 3                                                               # a row of ~3,000 entries
    ei = torch.stack([src, dst])
    assert not bool((ei[0] == ei[1]).any())
    return ei, torch.randn(N_L, F_L, generator=g), torch.rand(E_L, generator=g) + 0.5, g


def _run(dev, fn, tensors, go):
    """forward + backward of ``fn(*leaves)``: the output and every gradient"""
    leaves = [t.to(dev).requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    out.backward(go.to(dev))
    return [out.detach()] + [t.grad for t in leaves]


def _pair(dev, p=0.3, undirected=False, **kw):
    ei, x, ew, gen = _layer_case()
    parent = npi.CSRGraph(ei.to(dev), N_L, **kw)
    g = parent.drop_edges(p, seed=SEED, draw=DRAW, undirected=undirected)
    mask = torch.from_numpy(_ref_mask(ei, p, undirected))
    fresh = npi.CSRGraph(ei[:, mask].to(dev), N_L, item=parent.by_dst.item, **kw)
    return ei, x, ew, gen, g, fresh, mask


def _bitwise(a, b, mask, names):
    for name, p, q in zip(names, a, b):
        if name == "d_edge_weight":                        # the fresh graph's [E_kept] gradient scattered to the parent's columns
            full = torch.zeros_like(p)
            full[mask.to(p.device)] = q
            assert float(p[~mask.to(p.device)].abs().max()) == 0.0          # a dropped edge's weight: exactly 0
            q = full
        assert torch.equal(p, q), name


@pytest.mark.parametrize("layer", ["sage_mean", "sage_mean_w", "sage_max", "gcn_w", "gcn_wide_w", "gat1"])
@pytest.mark.parametrize("undirected", [False, True])
def test_layers_bitwise_equal_to_the_fresh_filtered_graph(dev, layer, undirected):
    """the entry order and the item cuts are the same, so the kernels do the same arithmetic: forward, dX, dW, db (, d att,
    d edge_weight) bit for bit"""
    ei, x, ew, gen, g, fresh, mask = _pair(dev, undirected=undirected)
    Fo = 16 if layer == "gcn_wide_w" else 48               # (GCNConv projects first when the input is wider than the output)
    W, b = torch.randn(F_L, Fo, generator=gen) / F_L ** 0.5, torch.randn(Fo, generator=gen)
    go = torch.randn(N_L, Fo, generator=gen)
    if layer in ("sage_mean", "sage_max"):
        aggr = "max" if layer == "sage_max" else "mean"
        fn = lambda graph: (lambda x_, W_, b_: npi.sage_conv(x_, graph, W_, b_, aggr=aggr))                     # noqa: E731
        a, c = _run(dev, fn(g), (x, W, b), go), _run(dev, fn(fresh), (x, W, b), go)
        _bitwise(a, c, mask, ("out", "dX", "dW", "db"))
    elif layer in ("sage_mean_w", "gcn_w", "gcn_wide_w"):
        conv = npi.sage_conv if layer == "sage_mean_w" else npi.gcn_conv
        fn = lambda graph: (lambda x_, W_, b_, w_: conv(x_, graph, W_, b_, edge_weight=w_))                     # noqa: E731
        a, c = _run(dev, fn(g), (x, W, b, ew), go), _run(dev, fn(fresh), (x, W, b, ew[mask]), go)
        _bitwise(a, c, mask, ("out", "dX", "dW", "db", "d_edge_weight"))
        assert float(a[4].abs().max()) > 0.0
    else:
        att = torch.randn(1, 1, 2 * Fo, generator=gen) / Fo ** 0.5
        fn = lambda graph: (lambda x_, W_, a_, b_: npi.gat_conv(x_, graph, W_, a_, b_, heads=1))                # noqa: E731
        a, c = _run(dev, fn(g), (x, W, att, b), go), _run(dev, fn(fresh), (x, W, att, b), go)
        _bitwise(a, c, mask, ("out", "dX", "dW", "datt", "db"))
    # the drop matters: the parent's layer output is somewhere else
    assert int(mask.sum()) < E_L


def test_gat_with_rule_d_dropout_against_the_oracle(dev):
    """four heads, ``dropout=0.6, seed=0``: Rule D is keyed on the PARENT's column numbers, which the fresh graph renumbers, so the two
    graphs' masks differ by construction -- the dropped graph is compared against the fp64 oracle over the kept edges with the
    Rule D mask of their parent columns (the layer's own bars, tests/test_gpu_gat_dropout.py)."""
    ei, x, ew, gen, g, fresh, mask = _pair(dev)
    H, C, p_att = 4, 32, 0.6
    W = torch.randn(F_L, H * C, generator=gen) / F_L ** 0.5
    att, b = torch.randn(1, H, 2 * C, generator=gen) / C ** 0.5, torch.randn(H * C, generator=gen) * 0.1
    go = torch.randn(N_L, H * C, generator=gen)
    kept = ei[:, mask]
    slots = np.concatenate([np.nonzero(mask.numpy())[0].astype(np.uint64), (1 << 32) + np.arange(N_L, dtype=np.uint64)])
    ks = torch.from_numpy(D.keep_np(0, 0, p_att, slots, H)).double()               # the kept columns (none is a loop), then the N loops
    xr, Wr, ar, br = (t.clone().double().requires_grad_(True) for t in (x, W, att, b))
    ref = O.gat_conv(xr, kept, Wr, ar, br, heads=H, keep_scale=ks)
    ref.backward(go.double())
    rule = NF.AttentionDropout(p_att, 0, 0)
    got = _run(dev, lambda x_, W_, a_, b_: npi.gat_conv(x_, g, W_, a_, b_, heads=H, dropout=rule), (x, W, att, b), go)
    assert torch.allclose(got[0].cpu(), ref.detach().float(), atol=1e-4, rtol=1e-4)
    assert torch.allclose(got[1].cpu(), xr.grad.float(), atol=2e-4, rtol=1e-3)
    for have, want in zip(got[2:], (Wr.grad, ar.grad, br.grad)):
        assert rel_max(have, want) <= GRAD_REL, rel_max(have, want)
    # and the module: a seeded GATConv in training mode over a DropEdge'd graph runs the same call
    conv = npi.GATConv(F_L, C, heads=H, dropout=p_att, seed=0).to(dev).train()
    with torch.no_grad():
        conv.weight.copy_(W.to(dev)), conv.att.copy_(att.to(dev)), conv.bias.copy_(b.to(dev))
    assert torch.equal(conv(x.to(dev), g), got[0])


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_pair_form_sage_concat_bitwise(dev, aggr):
    """SAGEConv(concat=True) in the pair form with res_n_id: the backward walks root_side, the drop of the parent's"""
    n_src, n_dst, E, p = 500, 300, 5000, 0.3
    gen = torch.Generator().manual_seed(8)
    ei = _rand_ei(E, n_src, n_dst, 8)
    ei[1, :1500] = 2
    res = torch.randint(0, n_src, (n_dst,), generator=gen).to(dev)
    x, ew = torch.randn(n_src, F_L, generator=gen), torch.rand(E, generator=gen) + 0.5
    W, b = torch.randn(2 * F_L, 48, generator=gen) / 8, torch.randn(48, generator=gen)
    go = torch.randn(n_dst, 48, generator=gen)
    parent = npi.BipartiteGraph(ei.to(dev), (n_src, n_dst))
    g = parent.drop_edges(p, seed=SEED, draw=DRAW)
    mask = torch.from_numpy(_ref_mask(ei, p))
    fresh = npi.BipartiteGraph(ei[:, mask].to(dev), (n_src, n_dst), item=parent.by_dst.item)
    if aggr == "max":
        fn = lambda graph: (lambda x_, W_, b_: npi.sage_conv_bipartite((x_, None), graph, W_, b_, res_n_id=res, concat=True,   # noqa: E731
                                                                       aggr="max"))
        a, c = _run(dev, fn(g), (x, W, b), go), _run(dev, fn(fresh), (x, W, b), go)
        _bitwise(a, c, mask, ("out", "dX", "dW", "db"))
    else:
        fn = lambda graph: (lambda x_, W_, b_, w_: npi.sage_conv_bipartite((x_, None), graph, W_, b_, res_n_id=res, concat=True,   # noqa: E731
                                                                           edge_weight=w_))
        a, c = _run(dev, fn(g), (x, W, b, ew), go), _run(dev, fn(fresh), (x, W, b, ew[mask]), go)
        _bitwise(a, c, mask, ("out", "dX", "dW", "db", "d_edge_weight"))


def test_dropout_adj_and_drop_edges_give_the_same_layer(dev):
    ei, x, ew, gen = _layer_case(1)
    W, b = torch.randn(F_L, 48, generator=gen) / F_L ** 0.5, torch.randn(48, generator=gen)
    go = torch.randn(N_L, 48, generator=gen)
    dei = ei.to(dev)
    for undirected in (False, True):
        kw = dict(seed=SEED, draw=DRAW)
        g = npi.CSRGraph(dei, N_L, item=64).drop_edges(0.5, undirected=undirected, **kw)
        lst = npi.dropout_adj(dei, p=0.5, force_undirected=undirected, **kw)[0]
        padded = npi.dropout_adj(dei, p=0.5, force_undirected=undirected, pad=True, **kw)[0]
        fn = lambda graph: (lambda x_, W_, b_: npi.sage_conv(x_, graph, W_, b_))                                # noqa: E731
        a = _run(dev, fn(g), (x, W, b), go)
        for other in (npi.CSRGraph(lst, N_L, item=64), npi.CSRGraph(padded, N_L, item=64)):
            for p_, q_ in zip(a, _run(dev, fn(other), (x, W, b), go)):
                assert torch.equal(p_, q_)


# ---- 5. reproducibility, out=, capture, the module ------------------------------------------------------------------------------------
def _arrays(g):
    out = []
    for side in (g.by_dst, g.by_src):
        nnz = int(side.rowptr[-1])
        out += [side.rowptr.clone(), side.col[:nnz].clone(), side.eid[:nnz].clone(), side.rowidx[:nnz].clone(), side.item_row.clone()]
    return out


def test_reproducible_and_out_reuse(dev):
    ei, x, ew, gen = _layer_case(2)
    parent = npi.CSRGraph(ei.to(dev), N_L)
    tick = torch.tensor([3], dtype=torch.int64, device=dev)
    kw = dict(seed=SEED, draw=DRAW, tick=tick)
    a = parent.drop_edges(0.5, **kw)
    b = parent.drop_edges(0.5, **kw)
    assert all(torch.equal(p, q) for p, q in zip(_arrays(a), _arrays(b)))
    for other in (dict(kw, draw=DRAW + 1), dict(kw, seed=SEED + 1), dict(kw, tick=tick + 1), dict(kw, undirected=True)):
        assert not torch.equal(parent.drop_edges(0.5, **other).by_dst.rowptr, a.by_dst.rowptr)
    # out=: the arrays are reused, what was derived from the old sides is gone, the result is the fresh allocation's
    W, bias = torch.randn(F_L, 48, generator=gen).to(dev), torch.randn(48, generator=gen).to(dev)
    xd = x.to(dev).requires_grad_(True)
    npi.sage_conv(xd, a, W, bias).sum().backward()
    NF.mean_bwd_weights(a, a.by_src), NF._inverse_transpose_map(a), a.by_dst.inv_count()        # the per-graph caches of `a`
    assert a.__dict__.get("_mean_t_w") and all(k in a.__dict__ for k in ("_tmap", "_tmap_inv")) and a.by_dst._inv_cnt is not None
    ptrs = [t.data_ptr() for t in (a.by_dst.rowptr, a.by_dst.col, a.by_src.col)]
    want = parent.drop_edges(0.5, seed=SEED, draw=DRAW + 7)
    again = parent.drop_edges(0.5, seed=SEED, draw=DRAW + 7, out=a)
    assert again is a and ptrs == [t.data_ptr() for t in (a.by_dst.rowptr, a.by_dst.col, a.by_src.col)]
    assert all(torch.equal(p, q) for p, q in zip(_arrays(again), _arrays(want)))
    assert not any(k in a.__dict__ for k in ("_mean_t_w", "_tmap", "_tmap_inv")) and a.by_dst._inv_cnt is None
    assert torch.equal(npi.sage_conv(x.to(dev), again, W, bias), npi.sage_conv(x.to(dev), want, W, bias))
    with pytest.raises(ValueError, match="out="):
        parent.drop_edges(0.5, out=parent)
    with pytest.raises(ValueError, match="out="):
        npi.CSRGraph(ei.to(dev), N_L).drop_edges(0.5, out=a)
    with pytest.raises(ValueError, match="cached"):
        npi.GCNConv(F_L, 48, cached=True).to(dev)(x.to(dev), a)
    assert npi.GCNConv(F_L, 48).to(dev)(x.to(dev), a).shape == (N_L, 48)
    assert parent.drop_edges(0.5, training=False) is parent and parent.drop_edges(0.0) is parent


def test_captured_step_draws_a_new_mask_per_tick(dev):
    """drop_edges(tick=t) + one SAGEConv forward inside torch.cuda.graph: each replay equals the eager result for that tick"""
    ei, x, ew, gen = _layer_case(3)
    parent = npi.CSRGraph(ei.to(dev), N_L)
    parent.by_src                                                          # (built outside the capture)
    W, b = torch.randn(F_L, 48, generator=gen).to(dev), torch.randn(48, generator=gen).to(dev)
    xd = x.to(dev)
    tick = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.no_grad():
        eager = []
        for t in (0, 1):
            tick.fill_(t)
            eager.append(npi.sage_conv(xd, parent.drop_edges(0.5, seed=SEED, draw=DRAW, tick=tick), W, b).clone())
        assert not torch.equal(eager[0], eager[1])
        NG.check_pending()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=stream):
            out = npi.sage_conv(xd, parent.drop_edges(0.5, seed=SEED, draw=DRAW, tick=tick), W, b)
        for t in (0, 1):
            tick.fill_(t)
            out.fill_(7.0)
            cg.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager[t]), t


def test_module_counts_draws(dev):
    ei, x, ew, gen = _layer_case(4)
    parent = npi.CSRGraph(ei.to(dev), N_L)
    m = npi.DropEdge(0.5, seed=SEED)
    g0, g1 = m(parent), m(parent)
    assert m.draw == 2 and g0.dropped_from is parent and not torch.equal(g0.by_dst.rowptr, g1.by_dst.rowptr)
    assert torch.equal(g0.by_dst.rowptr, parent.drop_edges(0.5, seed=SEED, draw=0).by_dst.rowptr)
    assert torch.equal(g1.by_dst.rowptr, parent.drop_edges(0.5, seed=SEED, draw=1).by_dst.rowptr)
    m.draw = 0
    assert all(torch.equal(p, q) for p, q in zip(_arrays(m(parent)), _arrays(g0)))          # set back: the step replays
    m.eval()
    assert m(parent) is parent and m.draw == 1
    m.train()
    gb = npi.GraphBatch(x.to(dev), ei.to(dev))
    assert m(gb).dropped_from is gb.graph()
    bp = npi.BipartiteGraph(ei.to(dev), (N_L, N_L))
    assert m(bp).dropped_from is bp
    with pytest.raises(ValueError, match="undirected"):
        npi.DropEdge(0.5, undirected=True)(bp)
    with pytest.raises(TypeError):
        m(ei.to(dev))
    assert npi.DropEdge(0.0)(parent) is parent


# ---- 6. refusals through the ABI ---------------------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing(dev):
    lib = _lib.load()
    N = 40
    side = npi.CSRGraph(_rand_ei(500, N, N, 6).to(dev), N, item=64).by_dst
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr, item_row = torch.full((N + 1,), -7, **i32), torch.full((side.n_items + 1,), -7, **i32)
    col, eid, rowidx = (torch.full((side.nnz_max,), -7, **i32) for _ in range(3))
    ws_n = int(lib.npi_drop_edges_workspace_elems(side.nnz_max))
    ws = torch.full((ws_n + 1,), -7, **i32)
    good = dict(rowptr=ptr(side.rowptr), col=ptr(side.col), eid=ptr(side.eid), rowidx=ptr(side.rowidx), N=N, nnz_max=side.nnz_max, E=500,
                key=1, tick=0, T=1 << 62, flags=0, cap=side.nnz_max, item=64, rowptr_o=ptr(rowptr), col_o=ptr(col), eid_o=ptr(eid),
                rowidx_o=ptr(rowidx), item_row_o=ptr(item_row), ws=ptr(ws), ws_n=ws_n)
    bad = [dict(rowptr=0), dict(eid=0), dict(rowidx_o=0), dict(item_row_o=0), dict(ws=0), dict(cap=side.nnz_max - 1), dict(item=128),
           dict(ws=ptr(ws) + 2), dict(ws_n=ws_n - 1), dict(flags=2), dict(N=-1)]
    for b in bad:
        a = dict(good, **b)
        assert lib.npi_csr_drop_side(*a.values(), stream_ptr(dev)) == NPI_ERR_ARG, b
        assert b"npi_csr_drop_side" in lib.npi_last_error()
    ei = _rand_ei(500, N, N, 6).to(dev)
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    out = torch.full((2, 500), -7, dtype=torch.int64, device=dev)
    count = torch.full((1,), -7, **i32)
    lgood = dict(src=ptr(src), dst=ptr(dst), E=500, key=1, tick=0, T=1 << 62, flags=0, o0=ptr(out[0]), o1=ptr(out[1]), newpos=0,
                 count=ptr(count), pad=1, ws=ptr(ws), ws_n=ws_n)
    for b in (dict(src=0), dict(o1=0), dict(count=0), dict(ws=0), dict(ws=ptr(ws) + 1), dict(ws_n=1), dict(o0=ptr(src)), dict(E=-1)):
        assert lib.npi_drop_edge_list(*dict(lgood, **b).values(), stream_ptr(dev)) == NPI_ERR_ARG, b
    keep = torch.full((500,), 7, dtype=torch.uint8, device=dev)
    assert lib.npi_drop_edge_keep(0, ptr(dst), 500, 1, 0, 1 << 62, 1, ptr(keep), stream_ptr(dev)) == NPI_ERR_ARG
    assert lib.npi_drop_edge_keep(ptr(src), ptr(dst), 500, 1, 0, 1 << 62, 0, 0, stream_ptr(dev)) == NPI_ERR_ARG
    torch.cuda.synchronize()
    for t in (rowptr, item_row, col, eid, rowidx, ws, count):                # nothing was launched: every output still holds its fill
        assert bool((t == -7).all())
    assert bool((out == -7).all()) and bool((keep == 7).all())
