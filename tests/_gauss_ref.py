"""Rule N -- the seeded standard normal behind ``VGAE`` (``include/npi_gnn.h``) -- restated twice, in Python ints and in numpy uint64
arrays, with ``eps`` in float64: the integer stages are exact, ``ln`` / ``cos`` / ``sin`` are evaluated in float64 at the float32 inputs
``u1`` and ``theta``.  Plus the float64 torch composition of PyG's ``reparametrize`` / ``kl_loss`` with ``eps`` injected.  No GPU, no
library."""
import math

import numpy as np
import torch

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
C = 0xD6E8FEB86659FD93
DRAW_RULE_N = 7
TWO_PI_F32 = np.array([0x40C90FDB], dtype=np.uint32).view(np.float32)[0]
EPS_MAX = math.sqrt(48 * math.log(2))                  # u1 >= 2^-24


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def epoch_seed(seed: int, draw: int) -> int:
    """the key of draw ``draw`` as an unsigned 64-bit integer (``npi_gnn_amd/_draw.py`` returns the same bits, signed)"""
    return mix64(mix64(seed) + G * (draw + 1))


def root(seed: int, draw: int) -> int:
    return mix64(mix64(epoch_seed(seed, draw)) + DRAW_RULE_N * G)


def root_t(seed: int, draw: int, tick: int = 0) -> int:
    return mix64(root(seed, draw) + G * (tick + 1))


def word(rt: int, table: int, row: int, p: int) -> int:
    """``draw_word(draw_stream(root_t, table 2^32 + row), p + 1)``: the word of column pair ``p``"""
    slot = (table << 32) + row
    return mix64(mix64(rt ^ ((slot * C) & M64)) + G * (p + 1))


def eps_of_word(w: int):
    """the two values a word gives: columns ``2 p`` and ``2 p + 1``"""
    u1 = np.float32((w >> 40) + 1) * np.float32(2.0 ** -24)
    u2 = np.float32((w >> 16) & 0xFFFFFF) * np.float32(2.0 ** -24)
    theta = TWO_PI_F32 * u2
    assert u1.dtype == np.float32 and theta.dtype == np.float32
    r = math.sqrt(-2.0 * math.log(float(u1)))
    return r * math.cos(float(theta)), r * math.sin(float(theta))


def eps_int(seed: int, draw: int, tick: int, table: int, row: int, col: int) -> float:
    return eps_of_word(word(root_t(seed, draw, tick), table, row, col >> 1))[col & 1]


def _mix64_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def words_np(seed: int, draw: int, tick: int, table: int, rows, P: int):
    """``[len(rows), P]`` uint64: the words of column pairs ``0 .. P - 1`` of every row (wrapping uint64 arithmetic)"""
    with np.errstate(over="ignore"):
        slot = np.asarray(rows, dtype=np.uint64) + np.uint64(table << 32)
        stream = _mix64_np(np.uint64(root_t(seed, draw, tick)) ^ (slot * np.uint64(C)))
        steps = (np.arange(1, P + 1, dtype=np.uint64) * np.uint64(G))
        return _mix64_np(stream[:, None] + steps[None, :])


def eps_np(seed: int, draw: int, tick: int, table: int, rows, F: int):
    """``eps [len(rows), F]`` float64 for the given row numbers (``rows``: an int N means ``range(N)``)"""
    rows = np.arange(rows) if isinstance(rows, int) else np.asarray(rows)
    P = (F + 1) // 2
    w = words_np(seed, draw, tick, table, rows, P)
    u1 = ((w >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = ((w >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
    theta = TWO_PI_F32 * u2
    assert u1.dtype == np.float32 and theta.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    out = np.empty((len(rows), 2 * P), dtype=np.float64)
    out[:, 0::2] = r * np.cos(theta.astype(np.float64))
    out[:, 1::2] = r * np.sin(theta.astype(np.float64))
    return out[:, :F]


def ks_statistic(x) -> float:
    """the Kolmogorov-Smirnov distance of the sample ``x`` from N(0, 1)"""
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    n = x.size
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n)))


def distribution_figures(x):
    """``(|mean| sqrt(n), |var - 1| sqrt(n / 2), KS sqrt(n), max |x|)``: each of the first two is about a standard normal's
    magnitude for a true N(0, 1) sample, the third has its 1 % point at 1.63"""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.size
    return (abs(float(x.mean())) * math.sqrt(n), abs(float(x.var()) - 1.0) * math.sqrt(n / 2.0), ks_statistic(x) * math.sqrt(n),
            float(np.abs(x).max()))


def corr_figure(a, b) -> float:
    """``|corr(a, b)| sqrt(n)``"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return abs(float(np.corrcoef(a, b)[0, 1])) * math.sqrt(a.size)


def reparam_kl(mu, logvar, eps, n_total=None, max_logvar=10.0):
    """PyG 1.4.2 ``VGAE``: ``z = mu + eps * exp(0.5 * lv)`` and ``kl = -0.5 / n_total * sum(1 + lv - mu**2 - exp(lv))`` with
    ``lv = logvar.clamp(max=max_logvar)``, in the dtype of the arguments (torch; float64 for a reference)"""
    lv = logvar.clamp(max=max_logvar)
    n_total = max(mu.size(0), 1) if n_total is None else n_total           # (no row: the empty sum, 0)
    z = mu + eps * torch.exp(0.5 * lv)
    kl = -0.5 / n_total * torch.sum(1 + lv - mu ** 2 - lv.exp())
    return z, kl
