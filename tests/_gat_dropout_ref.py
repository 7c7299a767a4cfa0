"""Rule D -- the seeded attention-dropout mask of GATConv (``include/npi_gnn.h``) -- restated twice, in Python ints and in numpy
uint64 arrays, and an fp64-capable torch restatement of the bipartite GAT forward that takes the mask as ``keep_scale`` (the square
form has ``oracle/ref_conv.gat_conv(keep_scale=)``).  No GPU, no library."""
from fractions import Fraction

import numpy as np
import torch

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
C = 0xD6E8FEB86659FD93
DRAW_RULE_D = 6


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def epoch_seed(seed: int, draw: int) -> int:
    """the key of draw ``draw`` as an unsigned 64-bit integer (``npi_gnn_amd/_draw.py`` returns the same bits, signed)"""
    return mix64(mix64(seed) + G * (draw + 1))


def root(seed: int, draw: int) -> int:
    return mix64(mix64(epoch_seed(seed, draw)) + DRAW_RULE_D * G)


def word(rt: int, k: int, h: int) -> int:
    """``draw_word(draw_stream(root, k), h + 1)``"""
    return mix64(mix64(rt ^ ((k * C) & M64)) + G * (h + 1))


def threshold(p: float) -> int:
    return int(Fraction(float(p)) * 2 ** 64)


def scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - float(p)))


def _mix64_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def words_np(seed: int, draw: int, k, H: int):
    """``[len(k), H]`` uint64: the word of every slot ``k`` and head (wrapping uint64 arithmetic)"""
    with np.errstate(over="ignore"):
        k = np.asarray(k, dtype=np.uint64)
        stream = _mix64_np(np.uint64(root(seed, draw)) ^ (k * np.uint64(C)))
        return np.stack([_mix64_np(stream + np.uint64((G * (h + 1)) & M64)) for h in range(H)], axis=1)


def slots(eid, col):
    """the slot of every entry: its eid, or ``2^32 + i`` for the self loop appended at node i (eid < 0; col == i)"""
    eid = np.asarray(eid, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    return np.where(eid >= 0, eid, (1 << 32) + col).astype(np.uint64)


def keep_np(seed: int, draw: int, p: float, k, H: int):
    """``[len(k), H]`` float32: kappa = 0 where dropped, ``float32(1 / (1 - p))`` where kept"""
    dropped = words_np(seed, draw, k, H) < np.uint64(threshold(p))
    return np.where(dropped, np.float32(0), scale(p)).astype(np.float32)


def gat_bipartite(x_src, x_dst, edge_index, weight, att, bias=None, n_dst=None, heads=1, concat=True, negative_slope=0.2, relu=False,
                  keep_scale=None):
    """PyG 1.4.2 ``GATConv.forward((x_src, x_dst), edge_index, size)`` with ``alpha = alpha * keep_scale`` behind the softmax
    (``keep_scale [E, H]`` in the order of ``edge_index``'s columns, every column valid); ``tests/_bipartite_ref.gat_bipartite``
    with the dropout factor made explicit."""
    n_src = x_src.size(0)
    n_dst = (x_dst.size(0) if x_dst is not None else n_src) if n_dst is None else int(n_dst)
    H = int(heads)
    Cc = weight.size(1) // H
    s, d = edge_index[0], edge_index[1]
    h_src = (x_src @ weight).view(n_src, H, Cc)
    a = att.view(1, H, 2 * Cc)
    e = (h_src.index_select(0, s) * a[:, :, Cc:]).sum(-1)
    if x_dst is not None:
        h_dst = (x_dst @ weight).view(n_dst, H, Cc)
        e = e + (h_dst.index_select(0, d) * a[:, :, :Cc]).sum(-1)
    e = torch.nn.functional.leaky_relu(e, negative_slope)
    mx = torch.full((n_dst, H), -1e38, dtype=e.dtype).scatter_reduce(0, d.view(-1, 1).expand_as(e), e, reduce="amax", include_self=True)
    ex = (e - mx.index_select(0, d)).exp()
    den = torch.zeros((n_dst, H), dtype=e.dtype).index_add_(0, d, ex)
    alpha = ex / (den.index_select(0, d) + 1e-16)
    if keep_scale is not None:
        alpha = alpha * keep_scale.to(alpha.dtype)
    out = torch.zeros((n_dst, H, Cc), dtype=e.dtype).index_add_(0, d, alpha.unsqueeze(-1) * h_src.index_select(0, s))
    out = out.reshape(n_dst, H * Cc) if concat else out.mean(dim=1)
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out
