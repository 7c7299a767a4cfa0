"""Rule H without a GPU: the Python reference against an independent restatement through networkx / scipy, hand-worked labels, the new
symbols, every argument the entry points refuse (on the host, before any launch; no pointer is followed) and the ``ValueError``s of
the Python layer that are decided before the device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import enclose as NE

import _enclose_ref as ref

NPI_ERR_ARG = -1
A = 0x10000                      # an aligned stand-in for every pointer: never dereferenced by a refused call


# ---- the reference against networkx / scipy ------------------------------------------------------------------------------------------
def _independent(pairs, n, u, v, h):
    """(node_id, set of directed (global source, global target), z) through ego graphs, the induced subgraph and scipy's shortest paths"""
    nx = pytest.importorskip("networkx")
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import shortest_path
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(map(tuple, pairs.tolist()))
    if G.has_edge(u, v):
        G.remove_edge(u, v)
    S = set(nx.ego_graph(G, u, radius=h).nodes) | set(nx.ego_graph(G, v, radius=h).nodes)
    node_id = [u, v] + sorted(S - {u, v})
    local = {w: a for a, w in enumerate(node_id)}
    sub = G.subgraph(S)
    directed = {(a, b) for a, b in sub.edges} | {(b, a) for a, b in sub.edges}
    m = len(node_id)
    rows = [local[a] for a, b in directed]
    cols = [local[b] for a, b in directed]
    adj = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, m))
    keep0 = [0] + list(range(2, m))                          # the other target deleted, as PyG's drnl_node_labeling does
    keep1 = list(range(1, m))
    d0 = shortest_path(adj[keep0][:, keep0], directed=False, unweighted=True, indices=0)
    d1 = shortest_path(adj[keep1][:, keep1], directed=False, unweighted=True, indices=0)
    z = [1, 1]
    for w in range(2, m):
        du, dv = d0[w - 1], d1[w - 1]
        if not (np.isfinite(du) and np.isfinite(dv)):
            z.append(0)
            continue
        du, dv = int(du), int(dv)
        d = du + dv
        z.append(1 + min(du, dv) + (d // 2) * (d // 2 + d % 2 - 1))
    return node_id, directed, z


@pytest.mark.parametrize("bipartite", [False, True])
@pytest.mark.parametrize("h", [1, 2, 3])
def test_reference_is_the_induced_ego_union_with_scipy_distances(h, bipartite):
    for n, deg, seed in ((12, 2.0, 1), (31, 2.5, 2), (60, 3.0, 3)):
        pairs = ref.random_pairs(n, deg, seed, bipartite)
        ei = ref.symmetric(pairs)
        rng = np.random.default_rng(seed + 10)
        keys = [tuple(pairs[int(rng.integers(len(pairs)))]) for _ in range(4)]            # links of the graph
        keys += [tuple(int(x) for x in rng.choice(n, size=2, replace=False)) for _ in range(4)]   # and arbitrary pairs
        out = ref.extract(ei, n, keys, h)
        for g, (u, v) in enumerate(keys):
            node_id, directed, z = _independent(pairs, n, int(u), int(v), h)
            b, e = out["graph_ptr"][g], out["graph_ptr"][g + 1]
            assert out["node_id"][b:e].tolist() == node_id
            eb, ee = out["edge_ptr"][g], out["edge_ptr"][g + 1]
            got = [(int(out["node_id"][s]), int(out["node_id"][t])) for s, t in out["edge_index"][:, eb:ee].T]
            assert len(got) == len(set(got)) and set(got) == directed
            assert out["z"][b:e].tolist() == z
            assert bool((np.diff(out["edge_index"][1, eb:ee]) >= 0).all())


def test_hand_worked_labels():
    # a path 0-1-2-3-4, targets (0, 4), h = 2: local order u, v, 1, 2, 3
    ei = ref.symmetric([(0, 1), (1, 2), (2, 3), (3, 4)])
    out = ref.extract(ei, 5, [(0, 4)], 2)
    assert out["node_id"].tolist() == [0, 4, 1, 2, 3] and out["z"].tolist() == [1, 1, 4, 5, 4]
    assert out["dist"].tolist() == [[0, -1], [-1, 0], [1, 3], [2, 2], [3, 1]]
    # a common neighbour of both targets: z = 2; the target link itself is never emitted
    ei = ref.symmetric([(0, 1), (0, 2), (1, 2)])
    out = ref.extract(ei, 3, [(0, 1)], 1)
    assert out["z"].tolist() == [1, 1, 2] and out["e_id"].tolist() == [4, 5, 1, 2]
    out = ref.extract(ei, 3, [(0, 1)], 1, target_edge="add")
    assert out["e_id"].tolist() == [-1, 4, -1, 5, 1, 2] and out["edge_index"].tolist() == [[1, 2, 0, 2, 0, 1], [0, 0, 1, 1, 2, 2]]
    assert out["z"].tolist() == [1, 1, 2]
    # node 3 hangs off target 1 alone: it is reachable from 0 only through the other target -> z = 0
    ei = ref.symmetric([(0, 2), (1, 2), (1, 3)])
    out = ref.extract(ei, 4, [(0, 1)], 2)
    assert out["node_id"].tolist() == [0, 1, 2, 3] and out["z"].tolist() == [1, 1, 2, 0]
    assert out["dist"].tolist() == [[0, -1], [-1, 0], [1, 1], [-1, 1]]
    # a bad key is an empty sample
    out = ref.extract(ei, 4, [(2, 2), (0, 1), (0, 7)], 2)
    assert out["graph_ptr"].tolist() == [0, 0, 4, 4] and out["edge_ptr"].tolist() == [0, 0, 6, 6]
    assert [ref.drnl(1, 1), ref.drnl(1, 2), ref.drnl(2, 2), ref.drnl(1, 3), ref.drnl(2, 3), ref.drnl(-1, 1)] == [2, 3, 5, 4, 7, 0]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
NAMES = ("npi_enclose_workspace_bytes", "npi_enclose_sizes", "npi_enclose_fill", "npi_drnl_label", "npi_enclose_features")


def test_symbols_and_abi_version():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert lib.npi_abi_version() == 4                              # an additive change
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "enclose.hip" in SOURCES and "enclose.hip" not in HOST_ONLY
    for name in ("EnclosingSubgraphs", "EnclosingBatch", "drnl_node_labeling"):
        assert hasattr(npi, name) and name in npi.__all__


def test_workspace_query():
    lib = _lib.load()
    assert lib.npi_enclose_workspace_bytes(5085, 200) == NE.workspace_bytes(5085, 200) == 200 * 4 * 159 * 4
    assert lib.npi_enclose_workspace_bytes(1_000_000, 200) == NE.workspace_bytes(1_000_000, 200) == 100_000_000     # four bitmaps a sample
    assert lib.npi_enclose_workspace_bytes(33, 1) == 32 and lib.npi_enclose_workspace_bytes(7, 0) == 0
    assert lib.npi_enclose_workspace_bytes(0, 1) == -1 and lib.npi_enclose_workspace_bytes(5, -1) == -1
    assert lib.npi_enclose_workspace_bytes(2 ** 31 - 1, 1) == -1


def _sizes(lib, rowptr=A, col=A, eid=A, mask=None, N=100, keys=A, B=3, hops=2, flags=0, counts=A, node_off=A, edge_off=A, ws=A,
           ws_bytes=1 << 20, status=None):
    return lib.npi_enclose_sizes(rowptr, col, eid, mask, N, keys, B, hops, flags, counts, node_off, edge_off, ws, ws_bytes, status, None)


def _fill(lib, rowptr=A, col=A, eid=A, mask=None, N=100, keys=A, B=3, flags=0, node_off=A, edge_off=A, ws=A, ws_bytes=1 << 20, node_id=A,
          batch=A, esrc=A, edst=A, e_id=A, lrowptr=A, lcol=A, graph_ptr=A, edge_ptr=A, n_nodes=10, n_edges=20, status=None):
    return lib.npi_enclose_fill(rowptr, col, eid, mask, N, keys, B, flags, node_off, edge_off, ws, ws_bytes, node_id, batch, esrc, edst,
                                e_id, lrowptr, lcol, graph_ptr, edge_ptr, n_nodes, n_edges, status, None)


def _label(lib, rowptr=A, col=A, n=10, nnz=20, src=A, dst=A, graph_ptr=A, B=3, z=A, dist=A):
    return lib.npi_drnl_label(rowptr, col, n, nnz, src, dst, graph_ptr, B, z, dist, None)


def _features(lib, feat=A, ldf=8, Ff=8, node_id=A, z=A, batch=A, node_off=A, edge_off=A, B=3, n=10, e=20, label=1, x=A, ldx=9):
    return lib.npi_enclose_features(feat, ldf, Ff, node_id, z, batch, node_off, edge_off, B, n, e, label, x, ldx, None)


PARENT_BAD = {"N = 0": dict(N=0), "negative N": dict(N=-5), "N too large": dict(N=2 ** 31 - 1), "negative B": dict(B=-1),
              "null rowptr": dict(rowptr=None), "null col": dict(col=None), "null eid": dict(eid=None), "null keys": dict(keys=None),
              "unknown flag": dict(flags=2), "null workspace": dict(ws=None), "misaligned workspace": dict(ws=A + 2),
              "short workspace": dict(ws_bytes=3 * 4 * 4 * 4 - 1), "negative workspace": dict(ws_bytes=-1),
              "null node_off": dict(node_off=None), "null edge_off": dict(edge_off=None)}
REFUSED = [
    (_sizes, "npi_enclose_sizes", dict(PARENT_BAD, **{"hops = 0": dict(hops=0), "negative hops": dict(hops=-1), "null counts": dict(counts=None)})),
    (_fill, "npi_enclose_fill", dict(PARENT_BAD, **{
        "negative nodes": dict(n_nodes=-1), "negative edges": dict(n_edges=-1), "nodes too many": dict(n_nodes=2 ** 31 - 1),
        "edges too many": dict(n_edges=2 ** 31 - 1), "null node_id": dict(node_id=None), "null batch": dict(batch=None),
        "null edge_src": dict(esrc=None), "null edge_dst": dict(edst=None), "null e_id": dict(e_id=None), "null local_rowptr": dict(lrowptr=None),
        "null local_col": dict(lcol=None), "null graph_ptr": dict(graph_ptr=None), "null edge_ptr": dict(edge_ptr=None)})),
    (_label, "npi_drnl_label", {
        "negative n": dict(n=-1), "negative nnz": dict(nnz=-1), "negative B": dict(B=-1), "n too large": dict(n=2 ** 31 - 1),
        "null rowptr": dict(rowptr=None), "null col": dict(col=None), "null graph_ptr": dict(graph_ptr=None), "null z": dict(z=None),
        "null dist": dict(dist=None), "src without dst": dict(dst=None), "dst without src": dict(src=None)}),
    (_features, "npi_enclose_features", {
        "negative n": dict(n=-1), "negative e": dict(e=-1), "negative B": dict(B=-1), "negative F": dict(Ff=-1), "no column at all": dict(Ff=0, label=0, ldx=4),
        "feature pitch": dict(ldf=7), "output pitch": dict(ldx=8), "unknown label": dict(label=3), "null feat": dict(feat=None),
        "null node_id": dict(node_id=None), "null z": dict(z=None), "null batch": dict(batch=None), "null node_off": dict(node_off=None),
        "null edge_off": dict(edge_off=None), "null x": dict(x=None)}),
]


@pytest.mark.parametrize("call,name,cases", REFUSED, ids=[r[1] for r in REFUSED])
def test_bad_arguments_are_refused_before_a_launch(call, name, cases):
    lib = _lib.load()
    for what, kw in cases.items():
        assert call(lib, **kw) == NPI_ERR_ARG, what
        msg = lib.npi_last_error().decode()
        assert msg.startswith(name + ":"), (what, msg)


def test_nothing_to_label_or_to_write_is_no_launch():
    lib = _lib.load()
    assert _label(lib, rowptr=None, col=None, src=None, dst=None, graph_ptr=None, z=None, dist=None, n=0) == 0
    assert _label(lib, rowptr=None, col=None, src=None, dst=None, graph_ptr=None, z=None, dist=None, B=0) == 0
    assert _features(lib, feat=None, node_id=None, z=None, batch=None, node_off=None, edge_off=None, x=None, n=0) == 0


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_value_errors_decided_before_the_device_is_touched():
    ei = torch.from_numpy(ref.symmetric([(0, 1), (1, 2)]))
    with pytest.raises(ValueError, match="target_edge"):
        npi.EnclosingSubgraphs(ei, 3, target_edge="keep")
    with pytest.raises(ValueError, match="label"):
        npi.EnclosingSubgraphs(ei, 3, label="de")
    with pytest.raises(ValueError, match="num_hops"):
        npi.EnclosingSubgraphs(ei, 3, num_hops=0)
    with pytest.raises(ValueError, match="num_nodes"):
        npi.EnclosingSubgraphs(ei, 0)
    with pytest.raises(ValueError, match="edge_mask"):
        npi.EnclosingSubgraphs(ei, 3, edge_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="edge_index"):
        npi.EnclosingSubgraphs(ei.to(torch.int32), 3)
    with pytest.raises(TypeError, match="float32"):
        npi.EnclosingSubgraphs(ei, 3, feat=torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(npi.NpiError):                              # valid arguments, host tensors: there is no CPU path
        npi.EnclosingSubgraphs(ei, 3)


def test_workspace_cap():
    assert NE.WORKSPACE_CAP == 1 << 30
    assert NE.check_workspace(1_000_000, 200) == 100_000_000
    assert NE.check_workspace(1_000_000, NE.max_keys(1_000_000)) <= NE.WORKSPACE_CAP
    with pytest.raises(ValueError, match="fewer keys"):
        NE.check_workspace(1_000_000, NE.max_keys(1_000_000) + 1)
    with pytest.raises(ValueError, match="fewer keys"):
        NE.check_workspace(5085, 500_000)
    import inspect
    assert list(inspect.signature(npi.EnclosingSubgraphs.__init__).parameters)[1:] == [
        "edge_index", "num_nodes", "num_hops", "feat", "edge_mask", "target_edge", "label", "check_input"]
    assert list(inspect.signature(npi.EnclosingSubgraphs.batch).parameters)[1:] == ["keys", "n_nodes", "n_edges", "pad_features"]
    assert list(inspect.signature(npi.drnl_node_labeling).parameters)[:4] == ["graph_or_edge_index", "src", "dst", "graph_ptr"]
