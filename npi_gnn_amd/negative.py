"""Negative sampling on the MI355X: the pairs a link-prediction loss is taken against, drawn where the positives already are::

    neg = npi.NegativeSampler(edge_index, size=(n_src, n_dst), seed=0, allow_loops=True)   # sorts once: by-target side, sort_columns=True
    pairs = neg.pairs(num_neg_samples=None, draw=None, window=None)    # LongTensor [2, M]: row 0 into x_src, row 1 into x_dst
    k     = neg.corrupt(src, draw=None, tries=64)                      # LongTensor [K]; src: LongTensor of source ids (e.g. edge_index[0][batch])
    npi.negative_sampling(edge_index, size, num_neg_samples=None, seed=0)            # PyG's names: thin wrappers, one sampler per call
    i, j, k = npi.structured_negative_sampling(edge_index, size, seed=0)

The reference draws its negatives offline with a sequential Python loop (``src/generate_edgelist.py:108-139``: a uniform ncRNA, a
uniform protein, redraw a positive or a repeat, as many negatives as positives); PyG 1.4.2 ``negative_sampling`` /
``structured_negative_sampling`` run through ``random.sample`` and ``isin`` on the CPU.  Here ``pairs`` is Rule P and ``corrupt``
Rule T of ``include/npi_gnn.h``: counter-based splitmix64 candidates, a binary search of the sorted by-target row for membership,
and -- for ``pairs`` -- two stable radix sorts that keep the earliest occurrence of every valid candidate.  Both are pure functions
of ``(seed, draw, graph, ...)``; the random bits are not PyG's, the distributions are: ``pairs`` a uniform draw without replacement
from the non-edges, ``corrupt`` per slot a uniform non-neighbour of its source.

``pairs`` costs ONE host read in the usual case (``info``: did the window hold ``M`` distinct non-edges); ``corrupt`` none -- it may
run inside a stream capture.  CPU tensors raise ``NpiError``: there is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch

from . import graph as _graph
from ._draw import _LIMIT, check_edge_index, epoch_seed, next_draw, pair_size
from ._lib import NpiError, check, load, ptr, require_gpu, stream_ptr
from .graph import build_side


class NegativeSampler:
    """Negatives of the graph ``edge_index`` ``[2, E]`` (a GPU LongTensor; row 0 = source in ``[0, n_src)``, row 1 = target in
    ``[0, n_dst)``; PyG layout) with ``size = (n_src, n_dst)``, or an int ``N`` for one id space -- pass ``allow_loops=False`` there
    so that ``(v, v)`` is never a negative.  An "edge" is a column of ``edge_index`` as it is: no self loop is added or removed,
    parallel edges count once.

    ``seed`` and a draw number fix every result.  ``draw`` (readable and settable, like ``NeighborSampler.epoch``) is the number
    the next call takes when it is not given one; such a call counts it up.  ``num_non_edges``: how many pairs ``pairs`` can
    return at most (counted once, when the sampler is built).  The sort workspace belongs to the sampler and is reused."""

    def __init__(self, edge_index: torch.Tensor, size: Union[int, Tuple[int, int]], seed: int = 0, allow_loops: bool = True):
        check_edge_index(edge_index)
        self.n_src, self.n_dst = pair_size(size, "NegativeSampler")
        self.device = require_gpu(edge_index)
        self.edge_index, self.seed, self.allow_loops, self.draw = edge_index, int(seed), bool(allow_loops), 0
        n_src, n_dst = self.n_src, self.n_dst
        E = self.num_edges = int(edge_index.size(1))
        # by-target CSR of the edge list as it is, columns ascending within a row: what the membership search walks
        self.side = build_side(edge_index[1].contiguous(), edge_index[0].contiguous(), n_dst, n_src, self_loops=False,
                               drop_equal=False, sort_columns=True)
        # the number of non-edges, once: n_src * n_dst minus the distinct edges (and minus the loop cells that are no edges)
        row, col = self.side.rowidx[:E], self.side.col[:E]
        first = torch.ones(E, dtype=torch.bool, device=self.device)
        if E > 1:
            first[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
        counts = torch.stack([first.sum(), (first & (row == col)).sum()]).to(torch.int32)
        vals = torch.cat([counts] + _graph.pending_status(self.device)).tolist()
        _graph.raise_on_status(vals[2:])                       # an id out of range was dropped by the build: refused here
        distinct, loop_edges = vals[0], vals[1]
        self.num_non_edges = n_src * n_dst - distinct - (0 if self.allow_loops else min(n_src, n_dst) - loop_edges)
        self._cand = self._ws = None
        self.last_window = self.last_consumed = 0              # of the latest pairs(): the window that sufficed, info[1]

    # ---- Rule P ---------------------------------------------------------------------------------------------------------------------
    def default_window(self, M: int, canonical: bool = False) -> int:
        """How many candidates the first round of ``pairs`` looks at for ``M`` pairs (a policy, not part of the rule): the expected
        number of valid draws until ``M`` distinct ones have been seen -- ``Z ln(Z / (Z - M))`` of ``Z`` non-edges, the coupon
        collector's count -- over the non-edge density, plus 1 % and six standard deviations.  ``canonical``: the distinct ones are
        the ``Z / 2`` unordered non-edges; a candidate is valid as often as before."""
        density = self.num_non_edges / (self.n_src * self.n_dst)
        Z = self.num_non_edges // 2 if canonical else self.num_non_edges
        valid = Z * math.log(Z / (Z - M + 0.5)) if M < Z else Z * (math.log(Z) + 1.0)
        need = max(valid, float(M)) / density
        return int(1.01 * need + 6.0 * math.sqrt(need)) + 64

    def pairs(self, num_neg_samples: Optional[int] = None, draw: Optional[int] = None, window: Optional[int] = None,
              canonical: bool = False) -> torch.Tensor:
        """Rule P: ``[2, M]`` distinct non-edge pairs, ``M = min(num_neg_samples, num_non_edges)`` (``None``: the number of columns
        of ``edge_index``).  ``window``: the candidates of the first round (default: ``default_window(M)``); the result does not
        depend on it.  A round that holds fewer than ``M`` distinct non-edges is run again, from candidate 0, twice as long.

        ``canonical=True`` (Rule S 4; what ``EdgeSplitter`` asks of its sampler over the undirected form of a graph): every
        candidate ``(s, d)`` counts as ``(min, max)``, so the result holds ``a < b`` pairs, each unordered non-edge at most once, and
        ``M`` is clamped to ``num_non_edges // 2``.  It needs a SYMMETRIC edge list in one id space and ``allow_loops=False``."""
        M = self.num_edges if num_neg_samples is None else int(num_neg_samples)
        if canonical and (self.allow_loops or self.n_src != self.n_dst):
            raise ValueError("NegativeSampler.pairs: canonical=True needs one id space and allow_loops=False")
        if M < 0:
            raise ValueError(f"NegativeSampler.pairs: num_neg_samples must not be negative, got {num_neg_samples}")
        if window is not None and int(window) < 1:
            raise ValueError(f"NegativeSampler.pairs: window must be at least 1, got {window}")
        if window is not None:
            self._check_window(int(window))
        if torch.cuda.is_current_stream_capturing():
            raise NpiError("NegativeSampler.pairs reads a size back from the device and cannot run inside a stream capture")
        key = epoch_seed(self.seed, next_draw(self, draw))
        M = min(M, self.num_non_edges // 2 if canonical else self.num_non_edges)
        dev, lib, side = self.device, load(), self.side
        out = torch.empty((2, M), dtype=torch.int64, device=dev)
        if M == 0:
            return out
        W = max(self.default_window(M, canonical) if window is None else int(window), 1)
        info = torch.zeros(2, dtype=torch.int32, device=dev)
        st = stream_ptr(dev)
        flags = 0 if self.allow_loops else 1
        while True:
            self._check_window(W)
            cand, ws = self._buffers(W)
            check(lib.npi_negative_candidates(ptr(side.rowptr), ptr(side.col), self.n_dst, self.n_src, key, 0, W, flags, ptr(cand[0]),
                                              ptr(cand[1]), st), "npi_negative_candidates")
            if canonical:
                check(lib.npi_split_canonical(ptr(cand[0]), ptr(cand[1]), W, st), "npi_split_canonical")
            check(lib.npi_negative_distinct(ptr(cand[0]), ptr(cand[1]), W, self.n_src, self.n_dst, M, ptr(out[0]), ptr(out[1]),
                                            ptr(info), ptr(ws), int(ws.numel()), st), "npi_negative_distinct")
            found, consumed = info.tolist()                    # the ONE host read of a draw in the usual case
            if found >= M:
                self.last_window, self.last_consumed = W, consumed
                return out
            W *= 2                                             # from scratch: no state is carried between rounds

    @staticmethod
    def _check_window(W: int) -> None:
        if W >= _LIMIT:
            raise NpiError(f"NegativeSampler.pairs: a window of {W} candidates passes 2^31 - 1; ask for fewer pairs per call")

    def _buffers(self, W: int):
        """candidate pairs ``[2, >= W]`` int32 and the sort workspace for ``W`` entries, kept and grown as needed"""
        if self._cand is None or self._cand.size(1) < W:
            self._cand = self._ws = None                        # (let go of the short ones first)
            self._cand = torch.empty((2, W), dtype=torch.int32, device=self.device)
        nbytes = int(load().npi_negative_distinct_workspace_bytes(W))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._cand, self._ws

    # ---- Rule T ---------------------------------------------------------------------------------------------------------------------
    def corrupt(self, src: torch.Tensor, draw: Optional[int] = None, tries: int = 64) -> torch.Tensor:
        """Rule T: for every slot ``k`` a target ``out[k]`` with ``(src[k], out[k])`` not an edge -- the first of ``tries`` uniform
        draws that is none.  -1 where every try hit an edge (the source is joined to every target, or ``tries`` ran out) or where
        ``src[k]`` lies outside ``[0, n_src)``; either is reported through the status word (``graph.check_pending()`` raises).
        No host read: inside a stream capture pass a ``src`` that is already a contiguous LongTensor."""
        tries = int(tries)
        if tries < 1 or tries >= _LIMIT:
            raise ValueError(f"NegativeSampler.corrupt: tries must be at least 1, got {tries}")
        if not isinstance(src, torch.Tensor) or src.dtype != torch.int64 or src.dim() != 1:
            raise ValueError("NegativeSampler.corrupt: src must be a LongTensor of source ids, shape [K]")
        dev = require_gpu(src)
        if dev != self.device:
            raise NpiError(f"tensors on different devices: {self.device} vs {dev}")
        src = src.contiguous()
        K = int(src.numel())
        if K >= _LIMIT:
            raise NpiError("NegativeSampler.corrupt: more than 2^31 - 2 slots in one call")
        key = epoch_seed(self.seed, next_draw(self, draw))
        out = torch.empty(K, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        side = self.side
        check(load().npi_negative_targets(ptr(side.rowptr), ptr(side.col), self.n_dst, self.n_src, ptr(src), K, key, tries, ptr(out),
                                          ptr(status), stream_ptr(dev)), "npi_negative_targets")
        _graph.note_status(status)
        return out

    def __repr__(self):
        return f"NegativeSampler(size=({self.n_src}, {self.n_dst}), edges={self.num_edges}, non_edges={self.num_non_edges})"


def negative_sampling(edge_index: torch.Tensor, size, num_neg_samples: Optional[int] = None, seed: int = 0) -> torch.Tensor:
    """PyG's ``negative_sampling(edge_index, num_nodes, num_neg_samples)``: ``NegativeSampler(edge_index, size, seed).pairs(
    num_neg_samples)``.  One sampler -- one sort of the edge list -- per call: keep a ``NegativeSampler`` for a graph that stays."""
    return NegativeSampler(edge_index, size, seed=seed).pairs(num_neg_samples)


def structured_negative_sampling(edge_index: torch.Tensor, size, seed: int = 0):
    """PyG's ``structured_negative_sampling(edge_index, num_nodes)``: ``(i, j, k)`` with ``(i, j) = edge_index`` and ``k`` a
    target that ``i`` has no edge to (``NegativeSampler(edge_index, size, seed).corrupt(edge_index[0])``)."""
    neg = NegativeSampler(edge_index, size, seed=seed)
    return edge_index[0], edge_index[1], neg.corrupt(edge_index[0])
