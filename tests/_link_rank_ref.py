"""Rule F of ``include/npi_gnn.h`` (``npi_link_ranks``) restated in numpy on top of ``_topk_ref``: fp64 scores rounded to f32, the
``rank_key`` order, the ``allowed`` mask -- and the metrics made of the counts."""
import numpy as np
import torch

import _topk_ref as tref

BAD_PAIR, BAD_SCORE = 256, 1024             # NPI_STATUS_BAD_PAIR_ID, NPI_STATUS_BAD_SCORE


def link_ranks(z_src, z_dst, edge_index, exclude=None, allow_loops=True):
    """``(counts int64 [Q, 4], scores f32 [Q], status)`` of Rule F; ``D`` rounded to f32 is the score (exact on the integer tables)"""
    D = tref.scores64(z_src, z_dst)
    n_src, n_dst = D.shape
    ok = tref.allowed(n_src, n_dst, exclude, allow_loops)
    with np.errstate(all="ignore"):
        s32 = D.astype(np.float32)
    key = tref.rank_key(s32).astype(np.int64)
    e = edge_index.numpy()
    Q = e.shape[1]
    counts = np.full((Q, 4), -1, dtype=np.int64)
    scores = np.full(Q, -np.inf, dtype=np.float32)
    status = 0
    cols = np.arange(n_dst)
    for q in range(Q):
        s, t = int(e[0, q]), int(e[1, q])
        if not (0 <= s < n_src and 0 <= t < n_dst):
            status |= BAD_PAIR
            continue
        nan = np.isnan(D[s])
        comp = ok[s] & (cols != t)                                 # a NaN counts where the pair is a competitor otherwise
        if nan[t] or (comp & nan).any():
            status |= BAD_SCORE
        if nan[t]:
            continue
        comp &= ~nan
        eq = comp & (key[s] == key[s, t])
        counts[q] = (int((comp & (key[s] < key[s, t])).sum()), int(eq.sum()), int((eq & (cols < t)).sum()), int(comp.sum()))
        scores[q] = s32[s, t] + np.float32(0.0)                    # -0.0 -> +0.0
    return torch.from_numpy(counts), torch.from_numpy(scores), status


def ranks(counts: np.ndarray, ties: str) -> np.ndarray:
    g, e, b = (counts[:, c].astype(np.float64) for c in range(3))
    return {"min": 1 + g, "max": 1 + g + e, "average": 1 + g + e / 2, "id": 1 + g + b}[ties]


def metrics(counts, ks=(1, 3, 10), ties="average") -> dict:
    """the masked means over the ranked rows (counts not -1), float64; NaN when there is none"""
    counts = np.asarray(counts)
    ok = counts[:, 0] >= 0
    r = ranks(counts[ok], ties)
    n = float(ok.sum())
    with np.errstate(all="ignore"):
        out = {"mrr": np.float64((1.0 / r).sum()) / n if n else np.nan, "mean_rank": np.float64(r.sum()) / n if n else np.nan}
        for k in ks:
            out[f"hits@{k}"] = np.float64((r <= k).sum()) / n if n else np.nan
    return out


def queries(n_src, n_dst, Q, exclude=None, seed=0):
    """``[2, Q]`` random query pairs; every fourth one is taken from the exclusion list itself (a known edge ranked against the
    non-edges)"""
    g = torch.Generator().manual_seed(4000 + seed)
    e = torch.stack([torch.randint(0, n_src, (Q,), generator=g), torch.randint(0, n_dst, (Q,), generator=g)])
    if exclude is not None and exclude.size(1):
        idx = torch.arange(0, Q, 4)
        e[:, idx] = exclude[:, torch.randint(0, exclude.size(1), (len(idx),), generator=g)]
    return e
