"""Rule H of ``include/npi_gnn.h`` (h-hop enclosing subgraphs with DRNL labels) restated in plain Python / numpy: sets, a BFS and
the formula.  What ``npi.EnclosingSubgraphs`` is tested against, bit for bit; ``test_enclose_cpu.py`` checks this file itself against
an independent restatement through scipy / networkx."""
import numpy as np


def drnl(du: int, dv: int) -> int:
    """SEAL's label of a non-target node from its two distances (-1: unreachable)"""
    if du < 0 or dv < 0:
        return 0
    d = du + dv
    return 1 + min(du, dv) + (d // 2) * (d // 2 + d % 2 - 1)


def rows_by_target(edge_index, num_nodes, mask=None):
    """rows[i] = [(j, e), ...]: the columns e = (j -> i) with j != i that the mask allows, in ascending (source id, column) order"""
    src, dst = np.asarray(edge_index[0]).tolist(), np.asarray(edge_index[1]).tolist()
    rows = [[] for _ in range(num_nodes)]
    for e, (j, i) in enumerate(zip(src, dst)):
        if j != i and (mask is None or bool(mask[e])):
            rows[i].append((j, e))
    for r in rows:
        r.sort()
    return rows


def _bfs(start, removed, n, out_edges):
    dist = [-1] * n
    dist[start] = 0
    level = [start]
    while level:
        nxt = []
        for x in level:
            for a in out_edges[x]:
                if a != removed and dist[a] < 0:
                    dist[a] = dist[x] + 1
                    nxt.append(a)
        level = nxt
    return dist


def label_graph(n, entries, s=0, d=1):
    """(z, dist) of one graph of n nodes: entries = [(source, target), ...] local; s / d: its two targets"""
    out_edges = [[] for _ in range(n)]
    for j, a in entries:
        if j != a:
            out_edges[j].append(a)
    du, dv = _bfs(s, d, n, out_edges), _bfs(d, s, n, out_edges)
    du[d], dv[s] = -1, -1
    z = [1 if w in (s, d) else drnl(du[w], dv[w]) for w in range(n)]
    return z, [[du[w], dv[w]] for w in range(n)]


def sample(rows, num_nodes, u, v, h, add=False):
    """one sample: (node_id, [(local source, local target, e_id), ...], z, dist); a bad key: all empty"""
    if u == v or not (0 <= u < num_nodes) or not (0 <= v < num_nodes):
        return [], [], [], []
    walk = lambda i, j: {i, j} != {u, v}                                        # noqa: E731
    S, level = {u, v}, {u, v}
    for _ in range(h):
        level = {j for i in level for j, _e in rows[i] if walk(i, j)} - S
        if not level:
            break
        S |= level
    node_id = [u, v] + sorted(S - {u, v})
    local = {w: a for a, w in enumerate(node_id)}
    entries = []
    for a, w in enumerate(node_id):
        if add and a < 2:
            entries.append((1 - a, a, -1))
        entries += [(local[j], a, e) for j, e in rows[w] if walk(w, j) and j in S]
    z, dist = label_graph(len(node_id), [(j, a) for j, a, e in entries if e >= 0])
    return node_id, entries, z, dist


def extract(edge_index, num_nodes, keys, h, mask=None, target_edge="remove"):
    """the whole batch, as numpy arrays under the names of ``EnclosingBatch``"""
    rows = rows_by_target(edge_index, num_nodes, mask)
    node_id, batch, src, dst, e_id, z, dist, gp, ep = [], [], [], [], [], [], [], [0], [0]
    for g, (u, v) in enumerate(np.asarray(keys).reshape(-1, 2).tolist()):
        ids, entries, zz, dd = sample(rows, num_nodes, int(u), int(v), h, add=target_edge == "add")
        off = gp[-1]
        node_id += ids
        batch += [g] * len(ids)
        src += [off + j for j, _a, _e in entries]
        dst += [off + a for _j, a, _e in entries]
        e_id += [e for _j, _a, e in entries]
        z += zz
        dist += dd
        gp.append(off + len(ids))
        ep.append(ep[-1] + len(entries))
    i64 = lambda v: np.asarray(v, dtype=np.int64)                               # noqa: E731
    return dict(node_id=i64(node_id), batch=i64(batch), edge_index=np.stack([i64(src), i64(dst)]), e_id=i64(e_id), z=i64(z),
                dist=np.asarray(dist, dtype=np.int32).reshape(-1, 2), graph_ptr=np.asarray(gp, dtype=np.int32),
                edge_ptr=np.asarray(ep, dtype=np.int32))


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------------
def symmetric(pairs):
    """[2, 2 P] int64: every undirected pair in both directions, (a, b) columns first, then (b, a)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([p.T, p.T[::-1]], axis=1)


def random_pairs(n, mean_degree, seed, bipartite=False):
    """distinct undirected pairs a < b (bipartite: a in the lower half, b in the upper), about n * mean_degree / 2 of them"""
    rng = np.random.default_rng(seed)
    m = max(1, int(n * mean_degree / 2))
    if bipartite:
        a, b = rng.integers(0, n // 2, size=m), rng.integers(n // 2, n, size=m)
    else:
        a, b = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo != hi
    return np.unique(np.stack([lo[keep], hi[keep]], axis=1), axis=0).reshape(-1, 2)


def symmetric_mask(edge_index, drop, seed):
    """bool [E], equal on every copy and direction of an undirected pair; about `drop` of the pairs False"""
    src, dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    code = lo * (int(max(src.max(initial=0), dst.max(initial=0))) + 1) + hi
    uniq, inv = np.unique(code, return_inverse=True)
    keep = np.random.default_rng(seed).random(uniq.size) >= drop
    return keep[inv]
