"""numpy restatement of Rule W of ``include/npi_gnn.h`` (second-order random walks by rejection) and of the pair layout of
``npi_walk_pairs``.  Pure numpy: it shares no code with the package.  Every walk is followed step by step and attempt by attempt as
the rule states it; the walks advance side by side only because each array operation handles one attempt of all of them."""
import numpy as np

from _negative_ref import C, GAMMA, U64, _u64, epoch_seed, mix64, mulhi  # noqa: F401

ONE = 1 << 32


def thresholds(p, q):
    """``(thr_ret, thr_nbr, thr_far)``: ``min(2^32, floor(2^32 a / mx))`` for a in (1/p, 1, 1/q), in double"""
    a = (1.0 / p, 1.0, 1.0 / q)
    return tuple(min(ONE, int(np.floor(ONE * (v / max(a))))) for v in a)


def by_source_csr(edge_index, N):
    """(rowptr, col) of the edge list as it is, columns ascending within a row, parallel edges kept"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    order = np.lexsort((ei[1], ei[0]))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=N))]).astype(np.int64)
    return rowptr, ei[1][order]


def walks(key, edge_index, N, start, L, thr=(ONE, ONE, ONE), tries=64):
    """Rule W: ``(walks [W, L + 1] int64, the number of steps whose tries ran out)``; a start outside ``[0, N)`` gives a row of -1"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    rowptr, col = by_source_csr(ei, N)
    codes = np.unique(ei[0] * int(N) + ei[1])
    start = np.asarray(start, dtype=np.int64)
    W = len(start)
    good = (start >= 0) & (start < N)
    out = np.full((W, L + 1), -1, dtype=np.int64)
    out[good, 0] = start[good]
    n = np.zeros(W, dtype=U64)                                    # attempts made so far, per walk
    exhausted = 0
    with np.errstate(over="ignore"):
        root = mix64(mix64(_u64(key)) + U64(3) * GAMMA)
        base = mix64(root ^ (np.arange(W, dtype=U64) * C))
        for t in range(1, L + 1):
            v = np.where(good, out[:, t - 1], 0)
            lo, d = rowptr[v], rowptr[v + 1] - rowptr[v]
            nxt = v.copy()                                        # d == 0: the walk stays, no word is consumed
            open_ = good & (d > 0)
            for _ in range(int(tries)):
                i = np.nonzero(open_)[0]
                if len(i) == 0:
                    break
                pick = mix64(base[i] + GAMMA * (U64(2) * n[i] + U64(1)))
                accept = mix64(base[i] + GAMMA * (U64(2) * n[i] + U64(2)))
                n[i] += U64(1)
                x = col[lo[i] + mulhi(pick, d[i]).astype(np.int64)]
                if t == 1:
                    thr_x = np.full(len(i), ONE, dtype=U64)          # no previous node: every candidate is accepted
                else:
                    prev = out[i, t - 2]
                    thr_x = np.where(x == prev, thr[0], np.where(np.isin(prev * int(N) + x, codes), thr[1], thr[2])).astype(U64)
                nxt[i] = x                                        # (the last candidate stays if none is accepted)
                open_[i[(accept >> U64(32)) < thr_x]] = False
            exhausted += int(open_.sum())
            out[good, t] = nxt[good]
    return out, exhausted


def pairs(key, walks_, c, S, N):
    """``npi_walk_pairs``: ``([2, M] int64, n_pos)`` -- PyG's ``torch.cat([rw[:, j:j + c] for j in range(J)], 0)`` windows, their
    ``(start, rest)`` pairs row by row, then ``S`` uniform nodes per window start"""
    walks_ = np.asarray(walks_, dtype=np.int64)
    W, L1 = walks_.shape
    rows = np.concatenate([walks_[:, j:j + c] for j in range(L1 + 1 - c)], axis=0)          # J = L + 2 - c windows, [R, c]
    R = len(rows)
    pos = np.stack([np.repeat(rows[:, 0], c - 1), rows[:, 1:].reshape(-1)])
    with np.errstate(over="ignore"):
        nbase = mix64(mix64(_u64(key)) + U64(4) * GAMMA)
        draws = mulhi(mix64(nbase + GAMMA * np.arange(1, R * S + 1, dtype=U64)), N).astype(np.int64)
    neg = np.stack([np.repeat(rows[:, 0], S), draws])
    return np.concatenate([pos, neg], axis=1), R * (c - 1)
