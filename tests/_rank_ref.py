"""Rule R of ``include/npi_gnn.h`` (``npi_rank_metrics``) restated in numpy, and the inputs the rank tests share.

``evaluate(scores, y)`` -> dict: ``thr`` (float32), ``tps`` / ``fps`` (int64), ``P``, ``N``, ``G``, ``U2`` (Python ints), ``auc``
(``U2 / (2.0 * P * N)`` in double) and ``ap`` (every term in double as the rule writes it, summed with ``math.fsum``).  The four
sklearn layouts are built from the curve exactly as ``npi_gnn_amd.rank`` builds them."""
import math

import numpy as np

TILE = 1024                      # positions per workgroup of the rank kernels (csrc/rank.hip: RANK_TILE)
SCAN_TILE, SORT_TILE = 2048, 4096
# every size at which one piece takes another path: wavefront, workgroup, rank tile, scan tile, sort tile, and the sorter's two
# launch regimes (at most / more than 64 sort tiles)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 64 * 4096, 64 * 4096 + 1)


def keys_of(scores):
    """step 1: s = score + 0.0f, the ascending-orderable transform of its bits, complemented"""
    s = (np.asarray(scores, dtype=np.float32) + np.float32(0.0)).astype(np.float32)
    b = s.view(np.uint32)
    u = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return (~u).astype(np.uint32)


def scores_of(keys):
    u = (~np.asarray(keys, dtype=np.uint32)).astype(np.uint32)
    b = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32)
    return b.view(np.float32)


def evaluate(scores, y=None, n_pos=None):
    scores = np.asarray(scores, dtype=np.float32)
    M = scores.size
    if y is None:
        y = (np.arange(M) < n_pos).astype(np.int64)
    y = np.asarray(y, dtype=np.int64)
    key = keys_of(scores)
    order = np.argsort(key, kind="stable")                                   # step 2
    key, lab = key[order], y[order]
    end = np.ones(M, dtype=bool)                                              # step 3
    if M > 1:
        end[:-1] = key[:-1] != key[1:]
    tp_all = np.cumsum(lab, dtype=np.int64)
    fp_all = np.arange(1, M + 1, dtype=np.int64) - tp_all
    thr, tps, fps = scores_of(key[end]), tp_all[end], fp_all[end]
    G = int(tps.size)
    P, N = (int(tps[-1]), int(fps[-1])) if G else (0, 0)
    tp0 = np.concatenate([[0], tps[:-1]]).astype(np.int64)                    # step 4
    fp0 = np.concatenate([[0], fps[:-1]]).astype(np.int64)
    U2 = sum(int(a) * int(b) for a, b in zip(fps - fp0, tps + tp0)) if G <= 4096 else int(np.sum((fps - fp0) * (tps + tp0)))
    auc = U2 / (2.0 * P * N) if P * N else float("nan")
    if P:
        terms = ((tps - tp0).astype(np.float64) / np.float64(P)) * (tps.astype(np.float64) / (tps + fps).astype(np.float64))
        ap = math.fsum(terms.tolist())
    else:
        ap = float("nan")
    return {"thr": thr, "tps": tps, "fps": fps, "P": P, "N": N, "G": G, "U2": U2, "auc": auc, "ap": ap}


def roc_curve(r):
    """sklearn's (fpr, tpr, thresholds) with drop_intermediate=False from a curve"""
    tps, fps = np.concatenate([[0], r["tps"]]).astype(np.float64), np.concatenate([[0], r["fps"]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return fps / np.float64(r["N"]), tps / np.float64(r["P"]), np.concatenate([[np.float32(np.inf)], r["thr"]]).astype(np.float32)


def precision_recall_curve(r):
    tps, fps = r["tps"].astype(np.float64), r["fps"].astype(np.float64)
    precision = tps / (tps + fps)
    recall = tps / np.float64(r["P"]) if r["P"] else np.ones_like(tps)
    return np.concatenate([precision[::-1], [1.0]]), np.concatenate([recall[::-1], [0.0]]), r["thr"][::-1].copy()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([17, *seed])


def labels(M, kind="30", seed=0):
    """``30``: about 30 % positives; ``P1`` / ``N1``: one positive / one negative; ``P0`` / ``N0``: none"""
    rng = _rng(1, M, seed)
    if kind == "30":
        return (rng.random(M) < 0.3).astype(np.int64)
    y = np.zeros(M, dtype=np.int64) if kind in ("P1", "P0") else np.ones(M, dtype=np.int64)
    if kind in ("P1", "N1"):
        y[rng.integers(0, M)] = 1 - y[0]
    return y


def tile_boundaries(M):
    """first positions of the rank, scan and sort tiles inside (0, M)"""
    return sorted({b for t in (TILE, SCAN_TILE, SORT_TILE) for b in range(t, M, t)})


def family(name, M, seed=0):
    """float32 scores [M] of one family.  The families that place tie groups against tile boundaries are built in SORTED
    (descending) order and then shuffled: the tile a group lands in is a matter of its rank, not of where it was given."""
    rng = _rng(2, M, seed, sum(map(ord, name)))
    if name == "distinct":                                                 # G = M
        s = (rng.permutation(M).astype(np.float32) - np.float32(M // 2)) * np.float32(0.25)
    elif name == "equal":                                                  # G = 1, auc exactly 0.5
        s = np.full(M, 0.375, dtype=np.float32)
    elif name == "seven":
        s = (rng.integers(0, 7, M).astype(np.float32) - np.float32(3)) / np.float32(4)
    elif name == "tile_fill":                                              # one group fills a whole tile and ends on the first
        rank = np.arange(M)                                                # element of the next: positions [TILE, 2 TILE]
        gid = np.where(rank < TILE, rank, np.where(rank <= 2 * TILE, TILE, rank - TILE))
        s = rng.permutation(-gid.astype(np.float32))
    elif name == "straddle":                                               # a two-element group across every tile boundary
        gid = np.arange(M)
        for b in tile_boundaries(M):
            gid[b] = gid[b - 1]
        s = rng.permutation(-gid.astype(np.float32))
    elif name == "sigmoid":                                                # saturated 0.0 / 1.0 ties
        x = (np.float32(8) * rng.standard_normal(M).astype(np.float32)).astype(np.float32)
        s = (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))).astype(np.float32)
        s[: min(M, 3)] = np.array([0.0, 1.0, 1.0], dtype=np.float32)[: min(M, 3)]
    elif name == "logprob":
        s = np.log(rng.random(M).astype(np.float32) * np.float32(0.999) + np.float32(1e-6)).astype(np.float32)
    elif name == "special":
        fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
        pool = np.array([0.0, -0.0, tiny, -tiny, np.float32(1e-40), np.float32(-1e-40), np.inf, -np.inf, fmax, -fmax, 1.0, -1.0,
                         np.finfo(np.float32).tiny], dtype=np.float32)
        s = pool[rng.integers(0, pool.size, M)]
        s[: min(M, pool.size)] = pool[: min(M, pool.size)]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(s, dtype=np.float32)


FAMILIES = ("distinct", "equal", "seven", "tile_fill", "straddle", "sigmoid", "logprob", "special")
