"""``npi.EnclosingSubgraphs`` on the GPU, bit for bit against Rule H restated in Python (``_enclose_ref.py``): every integer array
with ``torch.equal``, ``x`` bitwise against ``cat([label, feat[node_id]])``.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
from npi_gnn_amd import net1 as N1
from npi_gnn_amd import pool as NP

import _enclose_ref as ref

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = [("remove", "drnl"), ("add", "targets")]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _feat(n, F, seed):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed))


def _check(b, want, feat=None, label="drnl", B=None):
    """the EnclosingBatch `b` is exactly the reference's dict `want`"""
    gb = b.graph_batch
    for name in ("node_id", "z", "dist", "e_id", "graph_ptr", "edge_ptr"):
        got = getattr(b, name).cpu()
        exp = torch.from_numpy(want[name])
        assert got.dtype == exp.dtype and torch.equal(got, exp), name
    assert torch.equal(gb.batch.cpu(), torch.from_numpy(want["batch"]))
    assert gb.edge_index.dtype == torch.int64 and torch.equal(gb.edge_index.cpu(), torch.from_numpy(want["edge_index"]))
    assert torch.equal(gb.graph_ptr.cpu(), torch.from_numpy(want["graph_ptr"])) and gb.symmetric
    if B is not None:
        assert gb.num_graphs == B
    z = torch.from_numpy(want["z"])
    if label == "drnl":
        col = [z.float().view(-1, 1)]
    elif label == "targets":
        first = torch.from_numpy(want["graph_ptr"].astype(np.int64))[torch.from_numpy(want["batch"])]
        col = [((torch.arange(z.numel()) - first) >= 2).float().view(-1, 1)]
    else:
        col = []
    rows = [feat[torch.from_numpy(want["node_id"])]] if feat is not None else []
    exp = torch.cat(col + rows, dim=1) if col + rows else torch.zeros(z.numel(), 0)
    x = gb.x.cpu()
    assert x.shape == exp.shape and torch.equal(x.view(torch.int32), exp.view(torch.int32))
    if gb.pad_base is not None:
        assert gb.pad_base.size(1) % 128 == 0 and float(gb.pad_base[:, exp.size(1):].abs().sum()) == 0.0


def _run(dev, ei, n, keys, h, mask=None, feat=None, target_edge="remove", label="drnl", **kw):
    enc = npi.EnclosingSubgraphs(_t(ei, dev), n, num_hops=h, feat=None if feat is None else feat.to(dev),
                                 edge_mask=None if mask is None else _t(mask, dev), target_edge=target_edge, label=label)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    b = enc.batch(torch.from_numpy(keys), **kw)
    want = ref.extract(ei, n, keys, h, mask, target_edge)
    _check(b, want, feat, label, B=len(keys))
    return enc, b, want


# ---- boundaries ------------------------------------------------------------------------------------------------------------------------
def _boundary_graph(n, seed):
    """Mean degree 3 and a hub (node 0).  From 2,049 nodes on the hub is joined to 300 ordinary nodes and the nodes 1 .. 5 have exactly
    0, 1, 63, 64 and 65 neighbours; below, the hub is joined to all n - 1 others (a row of 63 / 64 entries at n = 64 / 65) and whether
    an isolated node exists is up to the mask."""
    rng = np.random.default_rng(seed)
    if n >= 2049:
        pairs = ref.random_pairs(n - 6, 3.0, seed) + 6
        stars = [(0, 300), (2, 1), (3, 63), (4, 64), (5, 65)]
        extra = [np.stack([np.full(d, c), 6 + rng.choice(n - 6, size=d, replace=False)], axis=1) for c, d in stars]
        pairs = np.concatenate([pairs] + extra)
    else:
        pairs = np.concatenate([ref.random_pairs(n, 3.0, seed), np.stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)], axis=1)])
        pairs = np.unique(np.sort(pairs, axis=1), axis=0)
    return ref.symmetric(pairs)


def _boundary_keys(ei, n, mask, seed):
    rng = np.random.default_rng(seed)
    live = np.ones(ei.shape[1], dtype=bool) if mask is None else mask
    adj = set(zip(ei[0][live].tolist(), ei[1][live].tolist()))
    deg = np.bincount(ei[1][live], minlength=n)
    nb = int(ei[1][(ei[0] == 0)][0])
    keys = [(0, nb), (nb, 0)]                                                     # (hub, neighbour) and (neighbour, hub)
    for _ in range(200):                                                           # a non-adjacent pair
        a, c = (int(v) for v in rng.integers(0, n, size=2))
        if a != c and (a, c) not in adj:
            keys.append((a, c))
            break
    iso = np.flatnonzero(deg == 0)
    if iso.size:                                                                   # an isolated node and another node
        keys.append((int(iso[0]), int((iso[0] + 1) % n)))
    if n >= 2049:
        keys += [(3, 4), (5, 2), (4, int(ei[1][ei[0] == 4][0]))]                    # the rows of 63, 64, 65 entries and of one
    while len(keys) < 15:
        if rng.random() < 0.5:
            c = int(rng.integers(ei.shape[1]))
            keys.append((int(ei[0][c]), int(ei[1][c])))
        else:
            a, c = (int(v) for v in rng.integers(0, n, size=2))
            keys.append((a, c) if a != c else (a, (a + 1) % n))
    keys.append(keys[2])                                                           # a repeated key
    return keys[:16]


@pytest.mark.parametrize("h", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 3, 33, 64, 65, 2049, 8200])
def test_boundaries(dev, n, h):
    ei = _boundary_graph(n, 100 + n)
    if n >= 2049:
        deg = np.bincount(ei[1], minlength=n)
        assert deg[:6].tolist() == [300, 0, 1, 63, 64, 65]
    else:
        assert np.bincount(ei[1], minlength=n)[0] == n - 1
    feat = _feat(n, 5, n)
    for mask in (None, ref.symmetric_mask(ei, 0.3, n + h)):
        keys = _boundary_keys(ei, n, mask, n + 7)
        assert len(keys) == 16
        for target_edge, label in MODES:
            _run(dev, ei, n, keys, h, mask, feat, target_edge, label)


# ---- structures ------------------------------------------------------------------------------------------------------------------------
def _path(n):
    return ref.symmetric([(i, i + 1) for i in range(n - 1)])


STRUCTURES = {
    # a BFS deeper than a wavefront is wide; large labels, and zeros behind a removed target link
    "path": (_path(70), 70, 40, [(0, 69), (0, 35), (10, 11), (34, 36), (69, 0), (20, 60)]),
    "cycle": (ref.symmetric([(i, (i + 1) % 9) for i in range(9)]), 9, 3, [(0, 1), (0, 4), (2, 7), (8, 0), (3, 5)]),
    "two components": (ref.symmetric([(0, 1), (1, 2), (2, 0), (2, 3), (4, 5), (5, 6), (6, 7), (7, 4)]), 9, 3,
                       [(0, 4), (3, 6), (0, 1), (4, 6), (8, 0), (8, 5)]),
    "K_3_70": (ref.symmetric([(a, 3 + c) for a in range(3) for c in range(70)]), 73, 2, [(0, 3), (0, 1), (3, 4), (72, 2), (1, 40)]),
    "triangles": (ref.symmetric(ref.random_pairs(40, 9.0, 5)), 40, 2, [(0, 1), (5, 30), (17, 3), (39, 38), (2, 20), (8, 9)]),
}


@pytest.mark.parametrize("name", list(STRUCTURES))
def test_structures(dev, name):
    ei, n, h, keys = STRUCTURES[name]
    for hops in sorted({1, 2, h}):
        for target_edge, label in MODES:
            _, b, want = _run(dev, ei, n, keys, hops, None, _feat(n, 3, 1), target_edge, label)
    if name == "path":
        assert int(want["z"].max()) > 300 and int((want["z"] == 0).sum()) > 0 and int(want["dist"].max()) > 64


def test_parallel_duplicates_and_loop_columns(dev):
    pairs = ref.random_pairs(30, 4.0, 9)
    base = ref.symmetric(pairs)
    dup = ref.symmetric(pairs[::3])                                # every third pair once more, in both directions ...
    loops = np.array([[4, 9, 4], [4, 9, 4]])                       # ... and (i, i) columns, one of them twice
    ei = np.concatenate([base[:, :7], loops, dup, base[:, 7:], dup[:, :10], dup[:, dup.shape[1] // 2: dup.shape[1] // 2 + 10]], axis=1)
    keys = [tuple(pairs[0]), tuple(pairs[3]), tuple(pairs[3][::-1]), (4, 9), (0, 29), (11, 12)]
    for mask in (None, ref.symmetric_mask(ei, 0.3, 2)):
        for target_edge, label in MODES:
            _, b, want = _run(dev, ei, 30, keys, 2, mask, _feat(30, 4, 2), target_edge, label)
    first = want["e_id"][: want["edge_ptr"][1]]
    assert len(set(first[first >= 0].tolist())) == int((first >= 0).sum())                              # each column at most once a sample ...
    assert want["edge_index"].shape[1] > len({tuple(c) for c in want["edge_index"].T.tolist()})          # ... and duplicates are emitted


# ---- batch sizes, widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 1030])
def test_batch_sizes(dev, B):
    ei = ref.symmetric(ref.random_pairs(12, 3.0, 4))
    rng = np.random.default_rng(B)
    keys = np.stack([rng.integers(0, 12, size=B), rng.integers(0, 11, size=B)], axis=1)
    keys[:, 1] = (keys[:, 0] + 1 + keys[:, 1]) % 12                # u != v
    enc, b, want = _run(dev, ei, 12, keys, 2, None, _feat(12, 2, 3), "add", "drnl")
    nodes, edges = enc.sizes(torch.from_numpy(keys))
    assert nodes.dtype == torch.int64 and not nodes.is_cuda
    assert torch.equal(nodes, torch.from_numpy(np.diff(want["graph_ptr"]).astype(np.int64)))
    assert torch.equal(edges, torch.from_numpy(np.diff(want["edge_ptr"]).astype(np.int64)))


def test_feature_widths_padding_and_no_features(dev):
    ei = ref.symmetric(ref.random_pairs(50, 3.0, 6))
    keys = [(0, 1), (7, 30), (49, 2)]
    _, b, _ = _run(dev, ei, 50, keys, 2, None, _feat(50, 100, 1), "remove", "drnl")             # 101 -> a pitch of 128
    assert b.graph_batch.pad_base is not None and b.graph_batch.pad_base.size(1) == 128
    _, b, _ = _run(dev, ei, 50, keys, 2, None, _feat(50, 100, 1), "remove", "drnl", pad_features=False)
    assert b.graph_batch.pad_base is None
    _, b, _ = _run(dev, ei, 50, keys, 2, None, _feat(50, 100, 1), "remove", None)               # 100 columns, no label
    _, b, _ = _run(dev, ei, 50, keys, 2, None, None, "add", "drnl")                             # the label alone
    _, b, _ = _run(dev, ei, 50, keys, 2, None, None, "remove", None)                            # only the structure
    assert tuple(b.graph_batch.x.shape) == (b.node_id.numel(), 0)


def test_check_input(dev):
    ei = ref.symmetric(ref.random_pairs(20, 3.0, 1))
    with pytest.raises(ValueError, match="symmetric"):
        npi.EnclosingSubgraphs(_t(ei[:, :-1], dev), 20)
    mask = ref.symmetric_mask(ei, 0.3, 1)
    mask[0] = not mask[0]
    with pytest.raises(ValueError, match="edge_mask"):
        npi.EnclosingSubgraphs(_t(ei, dev), 20, edge_mask=_t(mask, dev))
    with pytest.raises(ValueError, match="outside"):
        npi.EnclosingSubgraphs(_t(ei, dev), int(ei.max()))
    npi.EnclosingSubgraphs(_t(ei[:, :-1], dev), 20, check_input=False)


# ---- totals ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def totals_case(dev):
    ei = ref.symmetric(ref.random_pairs(200, 3.0, 8))
    rng = np.random.default_rng(5)
    keys = np.stack([rng.integers(0, 100, size=40), rng.integers(100, 200, size=40)], axis=1)
    feat = _feat(200, 7, 4)
    enc = npi.EnclosingSubgraphs(_t(ei, dev), 200, num_hops=2, feat=feat.to(dev), target_edge="add")
    want = ref.extract(ei, 200, keys, 2, None, "add")
    NG.check_pending()
    return enc, keys, feat, want, ei


def test_right_totals_and_stream_capture(dev, totals_case):
    enc, keys, feat, want, _ = totals_case
    n, e = int(want["graph_ptr"][-1]), int(want["edge_ptr"][-1])
    _check(enc.batch(torch.from_numpy(keys), n_nodes=n, n_edges=e), want, feat, "drnl", 40)
    nodes, edges = enc.sizes(torch.from_numpy(keys))
    b = enc.batch(torch.from_numpy(keys), n_nodes=nodes, n_edges=edges)
    _check(b, want, feat, "drnl", 40)
    assert torch.equal(b.graph_batch.sizes, nodes)
    dkeys = torch.from_numpy(keys).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.batch(dkeys, n_nodes=n, n_edges=e)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = enc.batch(dkeys, n_nodes=n, n_edges=e)
    graph.replay()
    torch.cuda.synchronize()
    _check(cap, want, feat, "drnl", 40)
    dkeys.copy_(torch.from_numpy(keys[::-1].copy()))                # the same multiset of samples in another order: same totals
    graph.replay()
    torch.cuda.synchronize()
    _check(cap, ref.extract(totals_case[4], 200, keys[::-1], 2, None, "add"), feat, "drnl", 40)
    NG.check_pending()


def test_wrong_totals_are_an_error_and_write_placeholders(dev, totals_case):
    enc, keys, feat, want, _ = totals_case
    n, e = int(want["graph_ptr"][-1]), int(want["edge_ptr"][-1])
    for dn, de in ((3, 0), (0, -2), (-1, 5)):
        b = enc.batch(torch.from_numpy(keys), n_nodes=n + dn, n_edges=e + de)
        gb = b.graph_batch
        assert b.node_id.numel() == n + dn and gb.edge_index.size(1) == e + de
        assert int(b.node_id.abs().max()) == 0 and int(gb.batch.abs().max()) == 0
        assert bool((gb.edge_index == -1).all()) and bool((b.e_id == -1).all())
        assert float(gb.x.abs().max()) == 0.0
        assert b.graph_ptr.tolist() == [0] + [n + dn] * 40 and b.edge_ptr.tolist() == [0] + [e + de] * 40
        with pytest.raises(ValueError, match="n_nodes / n_edges"):
            NG.check_pending()
    NG.set_debug(True)
    try:
        with pytest.raises(ValueError, match="n_nodes / n_edges"):
            enc.batch(torch.from_numpy(keys), n_nodes=n + 1, n_edges=e)
    finally:
        NG.set_debug(False)
    NG.check_pending()


def test_bad_keys_are_an_error_and_give_empty_samples(dev, totals_case):
    enc, keys, feat, _, ei = totals_case
    keys = keys[:6].copy()
    keys[1] = (5, 5)
    keys[4] = (3, 200)
    keys[5] = (-1, 7)
    want = ref.extract(ei, 200, keys, 2, None, "add")
    assert np.diff(want["graph_ptr"])[[1, 4, 5]].tolist() == [0, 0, 0] and np.diff(want["edge_ptr"])[[1, 4, 5]].tolist() == [0, 0, 0]
    b = enc.batch(torch.from_numpy(keys), n_nodes=int(want["graph_ptr"][-1]), n_edges=int(want["edge_ptr"][-1]))
    _check(b, want, feat, "drnl", 6)
    with pytest.raises(ValueError, match="u == v"):
        NG.check_pending()
    with pytest.raises(ValueError, match="u == v"):
        enc.batch(torch.from_numpy(keys))
    with pytest.raises(ValueError, match="u == v"):
        enc.sizes(torch.from_numpy(keys))
    NG.check_pending()


# ---- invariances ------------------------------------------------------------------------------------------------------------------------
def test_invariances(dev):
    pairs = ref.random_pairs(300, 3.0, 12)
    ei = ref.symmetric(pairs)
    rng = np.random.default_rng(1)
    keys = np.concatenate([pairs[rng.integers(0, len(pairs), size=10)], np.stack([rng.integers(0, 150, size=10), rng.integers(150, 300, size=10)], 1)])
    feat = _feat(300, 6, 1)
    enc, b, want = _run(dev, ei, 300, keys, 2, None, feat, "add", "drnl")
    again = enc.batch(torch.from_numpy(keys))
    for name in ("node_id", "z", "dist", "e_id", "graph_ptr", "edge_ptr"):
        assert torch.equal(getattr(b, name), getattr(again, name)), name
    assert torch.equal(b.graph_batch.edge_index, again.graph_batch.edge_index)
    assert torch.equal(b.graph_batch.x.view(torch.int32), again.graph_batch.x.view(torch.int32))
    for g in (0, 7, 19):                                           # a sample alone = the sample inside the batch, offsets subtracted
        one = enc.batch(torch.from_numpy(keys[g:g + 1]))
        nb, ne = int(b.graph_ptr[g]), int(b.graph_ptr[g + 1])
        eb, ee = int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        assert torch.equal(one.node_id, b.node_id[nb:ne]) and torch.equal(one.z, b.z[nb:ne]) and torch.equal(one.dist, b.dist[nb:ne])
        assert torch.equal(one.graph_batch.edge_index, b.graph_batch.edge_index[:, eb:ee] - nb) and torch.equal(one.e_id, b.e_id[eb:ee])
        assert torch.equal(one.graph_batch.x.view(torch.int32), b.graph_batch.x[nb:ne].view(torch.int32))
    perm = np.random.default_rng(2).permutation(ei.shape[1])       # column c of the permuted list is the old column perm[c]
    _, p, _ = _run(dev, ei[:, perm], 300, keys, 2, None, feat, "add", "drnl")
    assert torch.equal(p.node_id, b.node_id) and torch.equal(p.z, b.z) and torch.equal(p.dist, b.dist)
    assert torch.equal(p.graph_batch.edge_index, b.graph_batch.edge_index)
    real = (b.e_id >= 0).cpu()
    assert torch.equal((p.e_id < 0).cpu(), ~real)
    assert torch.equal(torch.from_numpy(perm)[p.e_id.cpu()[real]], b.e_id.cpu()[real])


# ---- the label kernel alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target_edge", ["remove", "add"])
def test_drnl_node_labeling(dev, target_edge):
    ei = ref.symmetric(ref.random_pairs(300, 3.0, 21))
    rng = np.random.default_rng(3)
    keys = np.stack([rng.integers(0, 150, size=12), rng.integers(150, 300, size=12)], 1)
    enc, b, want = _run(dev, ei, 300, keys, 3, None, None, target_edge, "drnl")
    gp = b.graph_ptr
    src, dst = gp[:-1], gp[:-1] + 1
    n = int(b.node_id.numel())
    for g in (b, npi.CSRGraph(b.graph_batch.edge_index, n), npi.CSRGraph(b.graph_batch.edge_index, n, self_loops=False),
              b.graph_batch.edge_index):
        z, dist = npi.drnl_node_labeling(g, src, dst, gp)
        assert z.dtype == torch.int64 and dist.dtype == torch.int32
        assert torch.equal(z, b.z) and torch.equal(dist, b.dist)
    # other targets than the first two rows, and graphs that do not cover every row: against the reference's BFS, graph by graph
    src2, dst2 = gp[1:-1] + 2, gp[1:-1].clone()
    z, dist = npi.drnl_node_labeling(b, src2, dst2, gp[1:])
    z, dist = z.cpu(), dist.cpu()
    first = int(gp[1])
    assert int(z[:first].abs().max()) == 0 and bool((dist[:first] == -1).all())
    eis = want["edge_index"]
    for g in range(1, 12):
        nb, ne = int(want["graph_ptr"][g]), int(want["graph_ptr"][g + 1])
        eb, ee = int(want["edge_ptr"][g]), int(want["edge_ptr"][g + 1])
        if ne - nb < 3:                                            # the source lies outside the graph: no label at all
            assert z[nb:ne].tolist() == [0, 0] and dist[nb:ne].tolist() == [[-1, -1], [-1, -1]]
            continue
        zz, dd = ref.label_graph(ne - nb, (eis[:, eb:ee] - nb).T.tolist(), s=2, d=0)
        assert z[nb:ne].tolist() == zz and dist[nb:ne].tolist() == dd, g


# ---- downstream ----------------------------------------------------------------------------------------------------------------------------
def test_downstream_models_train_on_the_batch(dev):
    pairs = ref.random_pairs(300, 4.0, 31, bipartite=True)
    ei = ref.symmetric(pairs)
    feat = _feat(300, 16, 5)
    rng = np.random.default_rng(4)
    keys = np.concatenate([pairs[rng.integers(0, len(pairs), size=12)], np.stack([rng.integers(0, 150, size=12), rng.integers(150, 300, size=12)], 1)])
    y = torch.cat([torch.ones(12), torch.zeros(12)]).long().to(dev)
    enc = npi.EnclosingSubgraphs(_t(ei, dev), 300, num_hops=2, feat=feat.to(dev), target_edge="add")
    torch.manual_seed(0)
    # SEAL's shape: conv -> sort pool -> linear
    conv, lin = npi.GCNConv(17, 8).to(dev), torch.nn.Linear(10 * 8, 2).to(dev)
    b = enc.batch(torch.from_numpy(keys))
    gb = conv(b.graph_batch)
    out = lin(NP.global_sort_pool(torch.relu(gb.x), gb.batch, 10, 24))
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for p in list(conv.parameters()) + list(lin.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    # Net_1 through the loader: host sizes, no read-back per batch
    model = N1.Net_1(17).to(dev).train()
    loader = N1.KeyLoader(enc, torch.from_numpy(keys).to(dev), y, batch_size=16)
    assert len(loader) == 2
    for data in loader:
        assert isinstance(data, npi.GraphBatch) and data.sizes is not None and data.x.size(1) == 17
        loss = torch.nn.functional.nll_loss(model(data), data.y)
        loss.backward()
        assert bool(torch.isfinite(loss))
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    NG.check_pending()


# ---- the real graph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 2])
def test_npinter2_graph(dev, h):
    fx = torch.load(os.path.join(G, "npinter2_graph.pt"), map_location="cpu", weights_only=False)
    ei = fx["edge_index"].long().numpy()
    n = int(fx["x"].size(0))
    deg = np.bincount(ei[1], minlength=n)
    hub = int(deg.argmax())
    assert deg[hub] == 1121
    cols = np.random.default_rng(0).choice(ei.shape[1], size=23, replace=False)
    keys = np.concatenate([ei[:, cols].T, ei[:, np.flatnonzero(ei[1] == hub)[:1]].T])            # 24 positive columns, one of the hub's
    feat = fx["x"].float()
    for target_edge, label in MODES:
        _, b, want = _run(dev, ei, n, keys, h, None, feat, target_edge, label)
    assert b.graph_batch.pad_base is not None and b.graph_batch.pad_base.size(1) == 256           # 179 columns on a pitch of 256
    assert int(np.diff(want["graph_ptr"]).max()) > 1121
