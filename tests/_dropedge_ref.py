"""Rule E (DropEdge, ``include/npi_gnn.h``) restated in numpy -- uint64 arrays, wrapping -- and, independently, in Python ints.
The reference of ``test_dropedge_cpu.py`` and ``test_gpu_dropedge.py``; it imports nothing from the package but ``epoch_seed`` /
``_mix64`` (the ints restatement), so that the numpy half stands on its own."""
from fractions import Fraction

import numpy as np

G = 0x9E3779B97F4A7C15
C = 0xD6E8FEB86659FD93
RULE_E = 8
_M64 = (1 << 64) - 1

# the answers pinned in include/npi_gnn.h (seed 0, draw 0)
KNOWN = {
    "key": 0xe220a8397b1dcdaf,
    "root": 0x3500c0e53fa8015b,
    "root_t0": 0x6ca685ee2acaed88,
    "root_t1": 0x7eeb741d67e7ca58,
    "directed": (0x7f2790ca6cae07ac, 0x4836408e21e38141),        # tick 0, slots 0 and 1, word 1
    "undirected": (0xa7db0d37986c2656, 0x37f4d516f27ca8a6),      # tick 0, slots 0 and 1 (pairs (0, 0) and (0, 1)), word 2
    "T": {0.5: 9223372036854775808, 0.3: 5534023222112865280, 1 - 2.0 ** -53: 18446744073709549568},
}


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def key_of(seed: int, draw: int) -> int:
    """epoch_seed(seed, draw) as the unsigned 64-bit number"""
    with np.errstate(over="ignore"):
        return int(mix64(mix64(np.uint64(seed & _M64)) + np.uint64(G) * np.uint64(draw + 1)))


def root_of(seed: int, draw: int) -> int:
    with np.errstate(over="ignore"):
        return int(mix64(mix64(np.uint64(key_of(seed, draw))) + np.uint64(RULE_E) * np.uint64(G)))


def root_t_of(seed: int, draw: int, tick: int = 0) -> int:
    with np.errstate(over="ignore"):
        return int(mix64(np.uint64(root_of(seed, draw)) + np.uint64(G) * np.uint64((tick + 1) & _M64)))


def threshold(p: float) -> int:
    """floor(p 2^64), p taken as the double it is"""
    return int(Fraction(float(p)) * 2 ** 64)


def slots(src, dst, undirected: bool):
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    if not undirected:
        return np.arange(src.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return (np.minimum(src, dst).astype(np.uint64) << np.uint64(32)) + np.maximum(src, dst).astype(np.uint64)


def words(src, dst, seed: int = 0, draw: int = 0, tick: int = 0, undirected: bool = False):
    rt = np.uint64(root_t_of(seed, draw, tick))
    with np.errstate(over="ignore"):
        stream = mix64(rt ^ (slots(src, dst, undirected) * np.uint64(C)))
        return mix64(stream + np.uint64(G) * np.uint64(2 if undirected else 1))


def keep_mask(src, dst, p: float, seed: int = 0, draw: int = 0, tick: int = 0, undirected: bool = False):
    """bool [E]: column e is KEPT"""
    return words(src, dst, seed, draw, tick, undirected) >= np.uint64(threshold(p))


def filtered(edge_index, p: float, seed: int = 0, draw: int = 0, tick: int = 0, undirected: bool = False):
    """(the kept columns in input order as an int64 array [2, E_kept], the mask)"""
    ei = np.asarray(edge_index, dtype=np.int64)
    m = keep_mask(ei[0], ei[1], p, seed, draw, tick, undirected)
    return ei[:, m], m


# ---- the second restatement: Python ints ------------------------------------------------------------------------------------------
def word_int(k: int, seed: int = 0, draw: int = 0, tick: int = 0, undirected: bool = False) -> int:
    from npi_gnn_amd._draw import _mix64, epoch_seed
    key = epoch_seed(seed, draw) & _M64
    root = _mix64(_mix64(key) + RULE_E * G)
    root_t = _mix64(root + G * (tick + 1))
    return _mix64(_mix64(root_t ^ ((k * C) & _M64)) + G * (2 if undirected else 1))


def roots_int(seed: int = 0, draw: int = 0):
    from npi_gnn_amd._draw import _mix64, epoch_seed
    key = epoch_seed(seed, draw) & _M64
    root = _mix64(_mix64(key) + RULE_E * G)
    return key, root, _mix64(root + G * 1), _mix64(root + G * 2)
