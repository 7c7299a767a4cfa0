"""numpy restatement of the two negative-sampling rules of ``include/npi_gnn.h`` (Rule P: distinct non-edge pairs; Rule T: the
corrupted target of given sources).  Pure numpy: it shares no code with the package.  ``edge_index``: the edge list as it is;
an "edge" is one of its columns, parallel edges count once."""
import numpy as np

from _sampler_ref import GAMMA, U64, _u64, epoch_seed, mix64  # noqa: F401

C = U64(0xD6E8FEB86659FD93)


def mulhi(a, n):
    """``(a * n) >> 64`` of the 128-bit product, for ``n < 2^32``"""
    a, n = np.asarray(a, dtype=U64), U64(n)
    return ((a >> U64(32)) * n + (((a & U64(0xFFFFFFFF)) * n) >> U64(32))) >> U64(32)


def edge_codes(edge_index, n_dst):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    return np.unique(ei[0] * int(n_dst) + ei[1])


def candidates(key, first, count, n_src, n_dst):
    """candidates ``first .. first + count - 1`` of Rule P: (src, dst) as int64"""
    with np.errstate(over="ignore"):
        base = mix64(mix64(_u64(key)) + GAMMA)
        i = np.arange(first, first + count, dtype=U64)
        src = mulhi(mix64(base + GAMMA * (U64(2) * i + U64(1))), n_src)
        dst = mulhi(mix64(base + GAMMA * (U64(2) * i + U64(2))), n_dst)
    return src.astype(np.int64), dst.astype(np.int64)


def pairs(key, edge_index, n_src, n_dst, M, no_loops=False, chunk=4096):
    """Rule P: ``([2, M] int64, candidates consumed)``.  The caller keeps ``M`` within the number of non-edges."""
    codes = edge_codes(edge_index, n_dst)
    seen, out, first, consumed = set(), [], 0, 0
    while len(out) < M:
        s, d = candidates(key, first, chunk, n_src, n_dst)
        c = s * int(n_dst) + d
        ok = ~np.isin(c, codes)
        if no_loops:
            ok &= s != d
        for j in np.nonzero(ok)[0]:
            cj = int(c[j])
            if cj not in seen:
                seen.add(cj)
                out.append((int(s[j]), int(d[j])))
                if len(out) == M:
                    consumed = first + int(j) + 1
                    break
        first += chunk
    return np.array(out, dtype=np.int64).reshape(-1, 2).T, consumed


def corrupt(key, edge_index, n_src, n_dst, src, tries=64):
    """Rule T: int64 ``[K]``; -1 where no try gives a non-edge or the source id lies outside ``[0, n_src)``"""
    codes = edge_codes(edge_index, n_dst)
    src = np.asarray(src, dtype=np.int64)
    k = np.arange(len(src), dtype=U64)
    good = (src >= 0) & (src < n_src)
    out = np.full(len(src), -1, dtype=np.int64)
    with np.errstate(over="ignore"):
        base = mix64(mix64(mix64(_u64(key)) + U64(2) * GAMMA) ^ (k * C))
        open_ = good.copy()
        for t in range(int(tries)):
            if not open_.any():
                break
            d = mulhi(mix64(base + GAMMA * U64(t + 1)), n_dst).astype(np.int64)
            hit = open_ & ~np.isin(np.where(good, src, 0) * int(n_dst) + d, codes)
            out[hit] = d[hit]
            open_ &= ~hit
    return out
