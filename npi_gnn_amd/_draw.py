"""What the seeded index features (``NeighborSampler``, ``NegativeSampler``, ``RandomWalker``, ``EdgeSplitter``) share on the host:
the key of a draw, the draw counter and the argument checks.  The device side of the generator is ``csrc/draw.h``."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

_M64 = (1 << 64) - 1
_LIMIT = 2 ** 31 - 1            # counts and id bounds stay below it (include/npi_gnn.h)


def _mix64(z: int) -> int:
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def epoch_seed(seed: int, epoch: int) -> int:
    """The ``seed`` argument of ``npi_sample_select`` for one epoch -- and the ``key`` of draw ``epoch`` of the other rules -- as a
    signed 64-bit integer: a splitmix64 step over ``seed`` and ``epoch`` (every hop of every batch of the epoch uses it; the hop
    index is a separate argument of the key)."""
    z = _mix64(_mix64(int(seed)) + 0x9E3779B97F4A7C15 * (int(epoch) + 1))
    return z - (1 << 64) if z >= (1 << 63) else z


def next_draw(obj, draw: Optional[int]) -> int:
    """the draw number of a call: the one given, or ``obj.draw``, the object's counter, which it then counts up"""
    if draw is None:
        draw = obj.draw
        obj.draw = draw + 1
    return int(draw)


def check_edge_index(edge_index) -> None:
    if not isinstance(edge_index, torch.Tensor) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("edge_index must be a LongTensor of shape [2, E]")


def pair_size(size, who: str) -> Tuple[int, int]:
    """``size``: ``(n_src, n_dst)``, or an int ``N`` for one id space"""
    entries = (size, size) if isinstance(size, int) and not isinstance(size, bool) else size
    if not isinstance(entries, (tuple, list)) or len(entries) != 2 or \
            any(isinstance(n, bool) or not isinstance(n, int) for n in entries):
        raise ValueError(f"{who}: size is an int N or a pair (n_src, n_dst) of ints, got {size!r}")
    n_src, n_dst = entries
    if n_src < 1 or n_dst < 1 or n_src >= _LIMIT or n_dst >= _LIMIT:
        raise ValueError(f"{who}: size entries lie in [1, 2^31 - 1), got {size!r}")
    return n_src, n_dst


def num_nodes(N, who: str, limit: int = _LIMIT, name: str = "num_nodes") -> int:
    """one id space: an int in ``[1, limit)``, ``limit`` a little below ``2^31``; ``name``: how ``who`` calls the argument"""
    if isinstance(N, bool) or not isinstance(N, int) or N < 1 or N >= limit:
        raise ValueError(f"{who}: {name} is an int in [1, 2^31 - {2 ** 31 - limit}), got {N!r}")
    return N
