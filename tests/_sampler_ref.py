"""numpy restatement of the neighbour-sampling rule of ``include/npi_gnn.h`` and of the block construction of PyG 1.4.2's bipartite
``NeighborSampler`` (ascending ``n_id``).  Pure numpy: it shares no code with the package.

Rule: over the by-target CSR of the edge list as it is (stable by target; ``eid`` = the edge's column), position ``p`` of the row of
target ``v`` gets the key ``(h32(seed, hop, v, p) << 32) | p``; the sample is the ``k`` smallest keys, in ascending ``p``."""
import math

import numpy as np

U64 = np.uint64
GAMMA = U64(0x9E3779B97F4A7C15)


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def _u64(i):
    return np.array([int(i) & ((1 << 64) - 1)], dtype=U64)


def epoch_seed(seed, epoch):
    """the key seed of one epoch (signed 64-bit), from the sampler's ``seed`` and its epoch count"""
    with np.errstate(over="ignore"):
        z = int(mix64(mix64(_u64(seed)) + GAMMA * _u64(epoch + 1))[0])
    return z - (1 << 64) if z >= (1 << 63) else z


def h32(seed, hop, v, p):
    """``p``: an array of positions; the upper half of the p-th output of the splitmix64 stream of (seed, hop, v)"""
    with np.errstate(over="ignore"):
        base = mix64(mix64(_u64(seed) + GAMMA * _u64(hop + 1)) ^ (_u64(v) * U64(0xD6E8FEB86659FD93)))
        return mix64(base + GAMMA * (np.asarray(p, dtype=U64) + U64(1))) >> U64(32)


def budget(d, size):
    """an int keeps min(d, size); a float (taken as float32, as the C ABI passes it) min(d, ceil(size * d)) in double"""
    if isinstance(size, float):
        return min(d, int(math.ceil(float(np.float32(size)) * d)))
    return min(d, int(size))


def sample_row(seed, hop, v, d, k):
    """ascending positions of the k smallest keys of a row of d entries"""
    if k >= d:
        return np.arange(d, dtype=np.int64)
    p = np.arange(d, dtype=U64)
    keys = (h32(seed, hop, v, p) << U64(32)) | p
    return np.sort(np.argsort(keys, kind="stable")[:k]).astype(np.int64)


def by_target_csr(edge_index, num_nodes):
    """(rowptr, col, eid) of the edge list as it is: entries of a row in list order"""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    order = np.argsort(dst, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=num_nodes))]).astype(np.int64)
    return rowptr, src[order], order.astype(np.int64)


def sample_hop(csr, targets, size, hop, seed, add_self_loops):
    """one block: (n_id, res_n_id or None, e_id, edge_index [2, E_s] with local ids)"""
    rowptr, col, eid = csr
    targets = np.asarray(targets, dtype=np.int64)
    src_g, e_id, tgt = [], [], []
    for t, v in enumerate(targets):
        s, d = int(rowptr[v]), int(rowptr[v + 1] - rowptr[v])
        pos = s + sample_row(seed, hop, int(v), d, budget(d, size))
        src_g.append(col[pos])
        e_id.append(eid[pos])
        tgt.append(np.full(len(pos), t, dtype=np.int64))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)      # noqa: E731
    src_g, e_id, tgt = cat(src_g), cat(e_id), cat(tgt)
    n_id = np.unique(np.concatenate([src_g, targets]) if add_self_loops else src_g)
    edge_index = np.stack([np.searchsorted(n_id, src_g), tgt])
    res_n_id = np.searchsorted(n_id, targets) if add_self_loops else None
    return n_id, res_n_id, e_id, edge_index


def data_flow(csr, targets, sizes, seed, add_self_loops):
    """the blocks of one batch in the order they are produced (hop 0 = next to the batch first)"""
    blocks, n_id = [], np.asarray(targets, dtype=np.int64)
    for hop, size in enumerate(sizes):
        blk = sample_hop(csr, n_id, size, hop, seed, add_self_loops)
        blocks.append(blk)
        n_id = blk[0]
    return blocks


def inclusion_counts(seed, hop, n_targets, d, k):
    """how often each position of a d-entry row is sampled over the targets 0 .. n_targets - 1, and the sample sizes"""
    counts = np.zeros(d, dtype=np.int64)
    sizes = []
    for v in range(n_targets):
        pos = sample_row(seed, hop, v, d, k)
        counts[pos] += 1
        sizes.append(len(np.unique(pos)))
    return counts, np.array(sizes)
