"""Edge splits on the MI355X: one edge list -> a training graph plus held-out positive and negative edges, where the list already is::

    sp = npi.EdgeSplitter(edge_index, size, seed=0)          # size: int N -> one id space, src < dst kept; (n_src, n_dst) -> every column kept
    edges, e_id = sp.permutation(draw=None)                  # Rule S 1-2: [2, K], [K]
    s = sp.split(val_ratio=0.05, test_ratio=0.1, draw=None, negatives=True)
    #   s.train_pos_edge_index (the undirected form in one id space; as kept otherwise), s.val_pos_edge_index, s.test_pos_edge_index,
    #   s.val_neg_edge_index, s.test_neg_edge_index   (PyG's attribute names), s.train_e_id / val_e_id / test_e_id
    for fold in sp.kfold(k=5, draw=None, negatives=True):    # the reference's protocol: K negatives drawn once, both lists cut into k
        fold.train_pos_edge_index, fold.test_pos_edge_index, fold.train_neg_edge_index, fold.test_neg_edge_index
    npi.train_test_split_edges(edge_index, num_nodes, val_ratio=0.05, test_ratio=0.1, seed=0)   # PyG's name: one splitter per call
    npi.to_undirected(edge_index, num_nodes)                 # PyG's name

PyG 1.4.2 ``train_test_split_edges`` runs ``torch.randperm`` on the host, finds the held-out negatives through a dense ``[N, N]``
mask and finishes with ``to_undirected`` through ``torch_sparse.coalesce``; the reference cuts its positives and as many sampled
negatives into five folds offline (``src/generate_edgelist.py:460-494``; in-script: ``src/train.py:108-184``).  Here the order is
Rule S of ``include/npi_gnn.h``: every kept column gets the 64-bit word ``r_e`` of a counter-based stream, two stable radix sorts
put the columns in ascending ``r_e``, and the parts are slices of that order.  The held-out negatives of one id space are Rule P's
candidates over the undirected form of the whole list, each rewritten as ``(min, max)``: a uniform draw without replacement from the
upper-triangle non-edges that never materialises them.  Everything is a pure function of ``(seed, draw, edge list)``; the random bits
are not PyG's or the reference's, the distributions are.

A split reads ``K`` (and the negatives' ``info``) back once, so it cannot run inside a stream capture.  CPU tensors raise
``NpiError``: there is no CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Iterator, Optional, Tuple, Union

import torch

from . import graph as _graph
from ._draw import _LIMIT, check_edge_index, epoch_seed, next_draw, num_nodes, pair_size
from ._lib import NPI_SPLIT_UPPER, NpiError, check, load, ptr, require_gpu, stream_ptr
from .negative import NegativeSampler


@dataclass
class EdgeSplit:
    """The parts of ``EdgeSplitter.split`` (PyG's attribute names).  ``*_e_id``: the columns of the splitter's ``edge_index`` the
    positives are -- for the train part the columns of the train SLICE (``train_pos_edge_index`` is its undirected form in one id
    space, the slice itself otherwise).  The negatives are ``None`` with ``negatives=False``."""
    train_pos_edge_index: torch.Tensor
    val_pos_edge_index: torch.Tensor
    test_pos_edge_index: torch.Tensor
    val_neg_edge_index: Optional[torch.Tensor]
    test_neg_edge_index: Optional[torch.Tensor]
    train_e_id: torch.Tensor
    val_e_id: torch.Tensor
    test_e_id: torch.Tensor


@dataclass
class EdgeFold:
    """One fold of ``EdgeSplitter.kfold``: the test range of the order and its complement, of the positives and of the negatives"""
    train_pos_edge_index: torch.Tensor
    test_pos_edge_index: torch.Tensor
    train_neg_edge_index: Optional[torch.Tensor]
    test_neg_edge_index: Optional[torch.Tensor]
    train_e_id: torch.Tensor
    test_e_id: torch.Tensor


def _check_ratios(val_ratio, test_ratio) -> Tuple[float, float]:
    v, t = float(val_ratio), float(test_ratio)
    if not (0.0 <= v <= 1.0 and 0.0 <= t <= 1.0) or v + t > 1.0:
        raise ValueError(f"val_ratio and test_ratio lie in [0, 1] and sum to at most 1, got {val_ratio!r} and {test_ratio!r}")
    return v, t


def _check_folds(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or k < 2:
        raise ValueError(f"kfold: k is an int of at least 2, got {k!r}")
    return k


def _num_nodes(N, who: str) -> int:
    """one id space: an int in [1, 2^31 - 2) (the undirected form needs one id above every node's)"""
    return num_nodes(N, who, _LIMIT - 1, "the number of nodes")


def _no_capture(who: str) -> None:
    if torch.cuda.is_current_stream_capturing():
        raise NpiError(f"{who} reads a size back from the device and cannot run inside a stream capture")


def fold_bounds(K: int, k: int) -> list:
    """Rule S 3: fold ``f`` of ``k`` tests on ``[bounds[f], bounds[f + 1])`` of the ``K`` ordered columns"""
    return [f * K // k for f in range(k + 1)]


def _undirected(src: torch.Tensor, dst: torch.Tensor, N: int) -> torch.Tensor:
    """Rule S 5 of two contiguous id rows: ``[2, E_u]``.  ONE host read (the number of pairs, with the pending status words)."""
    dev, lib = src.device, load()
    E = int(src.numel())
    if 2 * E >= _LIMIT:
        raise NpiError("to_undirected: more than 2^30 - 1 columns in one call")
    _no_capture("to_undirected")
    out = torch.empty((3, 2 * E), dtype=torch.int64, device=dev)           # rows, columns and the (unused) smallest input column
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.npi_split_undirected_workspace_bytes(E)), dtype=torch.uint8, device=dev)
    check(lib.npi_split_undirected(ptr(src), ptr(dst), E, N, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(info), ptr(status), ptr(ws),
                                   int(ws.numel()), stream_ptr(dev)), "npi_split_undirected")
    _graph.note_status(status)
    return out[:2, :int(info.item())].contiguous()


def to_undirected(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """PyG's ``to_undirected(edge_index, num_nodes)``: both orientations of every column, sorted by ``(row, col)``, equal pairs
    once.  A column with an id outside ``[0, num_nodes)`` is dropped and reported (``graph.check_pending()`` raises)."""
    check_edge_index(edge_index)
    N = _num_nodes(num_nodes, "to_undirected")
    require_gpu(edge_index)
    return _undirected(edge_index[0].contiguous(), edge_index[1].contiguous(), N)


class EdgeSplitter:
    """Splits of the edge list ``edge_index`` ``[2, E]`` (a GPU LongTensor, PyG layout).  ``size``: an int ``N`` -- one id space:
    only ``src < dst`` columns are kept (PyG's ``row < col``: give both orientations, or the upper one), the training graph comes
    back in its undirected form and the held-out negatives are ``a < b`` pairs -- or ``(n_src, n_dst)``: every column is kept and
    the negatives are ``NegativeSampler.pairs`` over the whole list.  A column with an id out of range is dropped and reported
    (``graph.check_pending()`` raises).

    ``seed`` and a draw number fix every result; ``draw`` counts as ``NegativeSampler.draw`` does: a call without one takes the
    counter and counts it up, a replay with an explicit ``draw`` takes no number.  The sort workspace and -- once negatives have
    been asked for -- the ``NegativeSampler`` over the whole list belong to the splitter and are reused."""

    def __init__(self, edge_index: torch.Tensor, size: Union[int, Tuple[int, int]], seed: int = 0):
        check_edge_index(edge_index)
        self.upper = isinstance(size, int)
        self.n_src, self.n_dst = (_num_nodes(size, "EdgeSplitter"),) * 2 if self.upper else pair_size(size, "NegativeSampler")
        self.device = require_gpu(edge_index)
        self.num_edges = int(edge_index.size(1))
        if self.num_edges >= _LIMIT:
            raise NpiError("EdgeSplitter: more than 2^31 - 2 columns")
        self.edge_index, self.seed, self.draw = edge_index, int(seed), 0
        self._src, self._dst = edge_index[0].contiguous(), edge_index[1].contiguous()
        self._ws = self._neg = None

    # ---- Rule S 1-2 -----------------------------------------------------------------------------------------------------------------
    def permutation(self, draw: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The kept columns in the order of draw ``draw``: ``(edges [2, K], e_id [K])``, ``e_id`` the columns of ``edge_index``"""
        _no_capture("EdgeSplitter.permutation")
        return self._permutation(next_draw(self, draw))

    def _permutation(self, draw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        dev, lib, E = self.device, load(), self.num_edges
        if self._ws is None:
            self._ws = torch.empty(int(lib.npi_split_workspace_bytes(E)), dtype=torch.uint8, device=dev)
        out = torch.empty((3, E), dtype=torch.int64, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        check(lib.npi_split_permute(ptr(self._src), ptr(self._dst), E, self.n_src, self.n_dst, epoch_seed(self.seed, draw),
                                    NPI_SPLIT_UPPER if self.upper else 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(info),
                                    ptr(status), ptr(self._ws), int(self._ws.numel()), stream_ptr(dev)), "npi_split_permute")
        _graph.note_status(status)
        K = int(info.item())                                   # the ONE host read of a permutation
        return out[:2, :K].contiguous(), out[2, :K].contiguous()

    # ---- Rule S 3-5 -----------------------------------------------------------------------------------------------------------------
    def split(self, val_ratio: float = 0.05, test_ratio: float = 0.1, draw: Optional[int] = None, negatives: bool = True,
              window: Optional[int] = None) -> EdgeSplit:
        """PyG's ``train_test_split_edges``: of the ``K`` ordered columns the first ``floor(val_ratio K)`` are the val positives,
        the next ``floor(test_ratio K)`` the test positives, the rest the train slice.  ``negatives``: as many held-out negatives
        as held-out positives, ONE draw whose head goes to val and whose tail to test.  ``window``: ``NegativeSampler.pairs``'s;
        the result does not depend on it."""
        v, t = _check_ratios(val_ratio, test_ratio)
        _no_capture("EdgeSplitter.split")
        draw = next_draw(self, draw)
        edges, e_id = self._permutation(draw)
        K = int(e_id.numel())
        n_v, n_t = int(math.floor(v * K)), int(math.floor(t * K))
        train = edges[:, n_v + n_t:]
        if self.upper:
            train = _undirected(train[0], train[1], self.n_src)
        val_neg = test_neg = None
        if negatives:
            neg = self._negatives(draw, n_v + n_t, window)
            n_vn = min(n_v, int(neg.size(1)))                  # (a graph with fewer non-edges than held-out positives: val first)
            val_neg, test_neg = neg[:, :n_vn], neg[:, n_vn:]
        return EdgeSplit(train, edges[:, :n_v], edges[:, n_v:n_v + n_t], val_neg, test_neg, e_id[n_v + n_t:], e_id[:n_v],
                         e_id[n_v:n_v + n_t])

    def kfold(self, k: int = 5, draw: Optional[int] = None, negatives: bool = True, window: Optional[int] = None) -> Iterator[EdgeFold]:
        """The reference's cross-validation: ONE order of the ``K`` kept columns and ONE draw of ``K`` negatives, both cut into ``k``
        contiguous folds (Rule S 3); fold ``f`` tests on its range and trains on the complement, as kept (no undirected form)."""
        k = _check_folds(k)
        _no_capture("EdgeSplitter.kfold")
        counted, draw = draw is None, next_draw(self, draw)
        edges, e_id = self._permutation(draw)
        K = int(e_id.numel())
        if k > K:
            if counted:
                self.draw = draw                               # a refused call takes no draw number
            raise ValueError(f"kfold: k = {k} folds of {K} kept columns")
        neg = self._negatives(draw, K, window) if negatives else None
        return self._folds(k, edges, e_id, neg)

    @staticmethod
    def _folds(k, edges, e_id, neg) -> Iterator[EdgeFold]:
        K = int(e_id.numel())
        pb = fold_bounds(K, k)
        nb = fold_bounds(int(neg.size(1)), k) if neg is not None else None
        for f in range(k):
            lo, hi = pb[f], pb[f + 1]
            train_neg = test_neg = None
            if neg is not None:
                test_neg = neg[:, nb[f]:nb[f + 1]]
                train_neg = torch.cat([neg[:, :nb[f]], neg[:, nb[f + 1]:]], dim=1)
            yield EdgeFold(torch.cat([edges[:, :lo], edges[:, hi:]], dim=1), edges[:, lo:hi], train_neg, test_neg,
                           torch.cat([e_id[:lo], e_id[hi:]]), e_id[lo:hi])

    def _negatives(self, draw: int, M: int, window: Optional[int]) -> torch.Tensor:
        """``M`` held-out negatives of draw ``draw`` (fewer where the graph has fewer non-edges).  One id space: Rule S 4 over the
        undirected form of the whole list; two: Rule P as it is.  The sampler has the splitter's seed: the same key."""
        if M == 0:
            return torch.empty((2, 0), dtype=torch.int64, device=self.device)
        if self._neg is None:
            if self.upper:
                whole = _undirected(self._src, self._dst, self.n_src)
                self._neg = NegativeSampler(whole, self.n_src, seed=self.seed, allow_loops=False)
            else:
                self._neg = NegativeSampler(self.edge_index, (self.n_src, self.n_dst), seed=self.seed)
        return self._neg.pairs(M, draw=draw, window=window, canonical=self.upper)

    def __repr__(self):
        return f"EdgeSplitter(size=({self.n_src}, {self.n_dst}), edges={self.num_edges}, upper={self.upper})"


def train_test_split_edges(edge_index: torch.Tensor, num_nodes: int, val_ratio: float = 0.05, test_ratio: float = 0.1,
                           seed: int = 0) -> EdgeSplit:
    """PyG's ``train_test_split_edges(data, val_ratio, test_ratio)`` on an edge list: ``EdgeSplitter(edge_index, num_nodes,
    seed).split(val_ratio, test_ratio)``.  One splitter -- one sort of the whole list for the negatives -- per call."""
    check_edge_index(edge_index)
    if isinstance(num_nodes, bool) or not isinstance(num_nodes, int):
        raise ValueError(f"train_test_split_edges: num_nodes is an int (one id space), got {num_nodes!r}")
    _check_ratios(val_ratio, test_ratio)
    return EdgeSplitter(edge_index, num_nodes, seed=seed).split(val_ratio, test_ratio)
