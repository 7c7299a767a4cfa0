"""numpy restatement of Rule S of ``include/npi_gnn.h`` (the random order of the kept columns of an edge list, its parts, the
undirected form and the held-out negatives of one id space).  Pure numpy: it shares no code with the package."""
import math

import numpy as np

from _sampler_ref import GAMMA, U64, _u64, epoch_seed, mix64  # noqa: F401
from _negative_ref import candidates, edge_codes


def keep_mask(edge_index, n_src, n_dst, upper):
    """Rule S 1: (kept [E] bool, any id out of range)"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    in_range = (ei[0] >= 0) & (ei[0] < n_src) & (ei[1] >= 0) & (ei[1] < n_dst)
    kept = in_range & (ei[0] < ei[1]) if upper else in_range
    return kept, bool((~in_range).any())


def words(key, E):
    """``r_e`` of columns ``0 .. E - 1``: a function of the key and of ``e`` alone"""
    with np.errstate(over="ignore"):
        base = mix64(mix64(mix64(_u64(key)) + U64(5) * GAMMA))
        return mix64(base + GAMMA * (np.arange(E, dtype=U64) + U64(1)))


def permutation(key, edge_index, n_src, n_dst, upper):
    """Rule S 1-2: (edges [2, K], e_id [K]) in ascending ``(r_e, e)``"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    kept, _ = keep_mask(ei, n_src, n_dst, upper)
    e = np.nonzero(kept)[0]
    r = words(key, ei.shape[1])[e]
    e_id = e[np.lexsort((e, r))].astype(np.int64)
    return ei[:, e_id], e_id


def part_sizes(K, val_ratio, test_ratio):
    """Rule S 3: (n_v, n_t); val = [0, n_v), test = [n_v, n_v + n_t), train = the rest"""
    return int(math.floor(val_ratio * K)), int(math.floor(test_ratio * K))


def fold_bounds(K, k):
    return [f * K // k for f in range(k + 1)]


def to_undirected(edge_index, N):
    """Rule S 5: both orientations of the in-range columns, sorted by (row, col), equal pairs once"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ei = ei[:, keep_mask(ei, N, N, False)[0]]
    codes = np.unique(np.concatenate([ei[0] * N + ei[1], ei[1] * N + ei[0]]))
    return np.stack([codes // N, codes % N])


def num_upper_non_edges(edge_index, N):
    u = to_undirected(edge_index, N)
    return N * (N - 1) // 2 - int((u[0] < u[1]).sum())


def upper_negatives(key, edge_index, N, M, chunk=4096):
    """Rule S 4: ``[2, min(M, upper non-edges)]`` distinct ``a < b`` non-edges in candidate order"""
    M = min(int(M), num_upper_non_edges(edge_index, N))
    codes = edge_codes(to_undirected(edge_index, N), N)
    seen, out, first = set(), [], 0
    while len(out) < M:
        s, d = candidates(key, first, chunk, N, N)
        ok = ~np.isin(s * N + d, codes) & (s != d)
        a, b = np.minimum(s, d), np.maximum(s, d)
        for j in np.nonzero(ok)[0]:
            c = (int(a[j]), int(b[j]))
            if c not in seen:
                seen.add(c)
                out.append(c)
                if len(out) == M:
                    break
        first += chunk
    return np.array(out, dtype=np.int64).reshape(-1, 2).T
