"""Rule K of ``include/npi_gnn.h`` (``npi_topk_links``) restated in numpy: fp64 scores, the candidate mask, the ``rank_key`` order
of ``csrc/rank_key.h`` and the id tie-break -- and the inputs the CPU and GPU tests share."""
import numpy as np
import torch

BAD_SOURCE, BAD_SCORE = 128, 1024            # NPI_STATUS_BAD_SOURCE_ID, NPI_STATUS_BAD_SCORE


def rank_key(s: np.ndarray) -> np.ndarray:
    """f32 scores -> uint32 keys, ascending key == descending score, -0.0 == +0.0 (Rule R 1)"""
    bits = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    u = np.where(bits & 0x80000000, ~bits, bits | np.uint32(0x80000000))
    return ~u


def scores64(z_src: torch.Tensor, z_dst: torch.Tensor) -> np.ndarray:
    with np.errstate(all="ignore"):
        return z_src.double().numpy() @ z_dst.double().numpy().T


def allowed(n_src, n_dst, exclude=None, allow_loops: bool = True) -> np.ndarray:
    """bool [n_src, n_dst]: the pairs neither excluded nor, with ``allow_loops`` off, a loop"""
    ok = np.ones((n_src, n_dst), dtype=bool)
    if exclude is not None and exclude.numel():
        e = exclude.numpy()
        inside = (e[0] >= 0) & (e[0] < n_src) & (e[1] >= 0) & (e[1] < n_dst)
        ok[e[0][inside], e[1][inside]] = False
    if not allow_loops:
        assert n_src == n_dst
        ok[np.arange(n_src), np.arange(n_src)] = False
    return ok


def candidates(D: np.ndarray, exclude=None, allow_loops: bool = True) -> np.ndarray:
    """bool [n_src, n_dst]: Rule K 2"""
    return allowed(D.shape[0], D.shape[1], exclude, allow_loops) & ~np.isnan(D)


def topk(z_src, z_dst, k, exclude=None, rows=None, allow_loops=True):
    """``(scores f32 [R, k], ids int64 [R, k], status)`` of Rule K; ``D`` rounded to f32 is the score (exact on the integer tables)"""
    D = scores64(z_src, z_dst)
    n_src, n_dst = D.shape
    ok = allowed(n_src, n_dst, exclude, allow_loops)
    with np.errstate(all="ignore"):
        s32 = D.astype(np.float32)
    key = rank_key(s32)
    q = np.arange(n_src) if rows is None else rows.numpy()
    scores = np.full((len(q), k), -np.inf, dtype=np.float32)
    ids = np.full((len(q), k), -1, dtype=np.int64)
    status = 0
    for r, i in enumerate(q):
        if not 0 <= i < n_src:
            status |= BAD_SOURCE
            continue
        nan = np.isnan(D[i])
        if (ok[i] & nan).any():                                    # a NaN counts where the pair is a candidate otherwise
            status |= BAD_SCORE
        js = np.nonzero(ok[i] & ~nan)[0]
        js = js[np.lexsort((js, key[i, js]))][:k]                  # by key, ties by id
        ids[r, :len(js)] = js
        scores[r, :len(js)] = s32[i, js] + np.float32(0.0)         # -0.0 -> +0.0
    return torch.from_numpy(scores), torch.from_numpy(ids), status


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------------
def int_tables(n_src, n_dst, F, seed=0):
    """integers in [-4, 4] as f32: every dot product is exact in any order (|sum| <= 16 * 260 < 2^24), ties everywhere"""
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randint(-4, 5, (n_src, F), generator=g).float(), torch.randint(-4, 5, (n_dst, F), generator=g).float())


def real_tables(n_src, n_dst, F, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(n_src, F, generator=g), torch.randn(n_dst, F, generator=g)


def edges(n_src, n_dst, E, seed=0):
    """a random [2, E] edge list; every tenth edge repeats the one before it (parallel edges)"""
    g = torch.Generator().manual_seed(3000 + seed)
    e = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    if E > 1:
        idx = torch.arange(1, E, 10)
        e[:, idx] = e[:, idx - 1]
    return e


def gamma(F):
    u = 2.0 ** -24
    return F * u / (1 - F * u)
