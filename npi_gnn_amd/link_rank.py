"""Filtered link ranks on the MI355X: at which position does each held-out true link come out among all targets its source has no
known edge to -- the ranking evaluation that goes with ``topk_links``::

    known = npi.KnownLinks(train_edge_index, size)                     # built once, as for topk_links
    r = npi.link_ranks(z, test_edge_index, exclude=known)              # int64 [Q] counts, f32 [Q] scores
    r.rank(ties="average")                                             # 1-based ranks, [Q]
    m = npi.ranking_metrics(z, test_edge_index, exclude=known, ks=(1, 3, 10))     # {"mrr", "mean_rank", "hits@1", ...}
    m = model.test_ranking(z, test_edge_index, train_edge_index)       # GAE: one id space never counts (v, v)
    r = npi.InnerProductDecoder().ranks(z, test_edge_index, exclude=known)

``GAE.test`` ranks the positives against one sampled negative each; this ranks every positive against ALL the non-edges of its
source -- the filtered protocol, MRR / Hits@K / mean rank as link-prediction papers and the later PyG / OGB evaluators report
them -- and says whether ``predict(z, k)`` shows the true partner within its ``k`` slots.  It is Rule F of ``include/npi_gnn.h``
(``npi_link_ranks``): the scan of ``npi_topk_links`` (64 queries x 128 targets per tile on the f32 matrix cores, the known edges
masked on the chip) with a consumer that counts instead of selecting; the target's own score comes from the matrix cores too.
The counts are integers: exact, and bitwise the same for any ``splits``, any order or repetition of the queries and any
repetition of the call.  ``greater + equal_before`` is the 0-based position of the target in ``topk_links``' list of its source
(when the pair itself is not excluded).

Out of scope: the by-target direction (swap the tables and flip the lists), grouping queries by source to share rows, bf16
tables, gradients (the results are detached), and sampled-negative ranking (that is ``GAE.test``).  CPU tensors raise
``NpiError``: there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from . import graph as _graph
from ._lib import NPI_LINK_RANK_NO_LOOPS, NpiError, check, load, ptr, require_gpu, stream_ptr
from .functional import _pair_tables, _pitched
from .topk import _LIMIT, KnownLinks, _edge_list

TIES = ("min", "max", "average", "id")


class LinkRanks:
    """The counts of Rule F for ``Q`` query pairs: ``greater``, ``equal``, ``equal_before``, ``candidates`` (int64 ``[Q]`` each) and
    ``score`` (f32 ``[Q]``, the target's logit), all detached.  A query with an id out of range or a NaN target score holds ``-1``
    in every count and ``-inf`` as its score (and is reported through the status word)."""

    def __init__(self, counts: torch.Tensor, score: torch.Tensor):
        self.counts = counts                                   # int64 [Q, 4]
        self.greater, self.equal, self.equal_before, self.candidates = counts.unbind(1)
        self.score = score

    @property
    def valid(self) -> torch.Tensor:
        """bool ``[Q]``: the queries that were ranked"""
        return self.greater >= 0

    def rank(self, ties: str = "average") -> torch.Tensor:
        """The 1-based rank of every target: ``"min"``: ``1 + greater`` | ``"max"``: ``1 + greater + equal`` | ``"average"``:
        ``1 + greater + equal / 2`` (float64) | ``"id"``: ``1 + greater + equal_before`` (``topk_links``' order).  int64 but for
        ``"average"``; meaningless (<= 0) where ``valid`` is False."""
        if ties == "min":
            return self.greater + 1
        if ties == "max":
            return self.greater + self.equal + 1
        if ties == "average":
            return self.greater.double() + self.equal.double() / 2 + 1
        if ties == "id":
            return self.greater + self.equal_before + 1
        raise ValueError(f"LinkRanks.rank: ties is one of {TIES}, got {ties!r}")

    def metrics(self, ks: Sequence[int] = (1, 3, 10), ties: str = "average") -> Dict[str, torch.Tensor]:
        """``{"mrr", "mean_rank", "hits@k" ...}``: means over the ranked queries of ``1 / rank``, ``rank`` and ``rank <= k`` -- 0-d
        float64 device tensors, NaN when no query was ranked; nothing is read back."""
        ks = _check_ks(ks, "LinkRanks.metrics")
        rank = self.rank(ties).double()
        ok = self.valid
        n = ok.sum().double()                                  # 0 / 0 = NaN when there is none
        zero = torch.zeros((), dtype=torch.float64, device=rank.device)
        out = {"mrr": torch.where(ok, 1.0 / rank, zero).sum() / n, "mean_rank": torch.where(ok, rank, zero).sum() / n}
        for k in ks:
            out[f"hits@{k}"] = (ok & (rank <= k)).sum().double() / n
        return out


def _check_ks(ks, who: str):
    if isinstance(ks, (str, bytes)) or not isinstance(ks, (tuple, list)):
        raise TypeError(f"{who}: ks is a tuple of positive ints, got {type(ks).__name__}")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, int):
            raise TypeError(f"{who}: ks is a tuple of positive ints, got an element of type {type(k).__name__}")
        if k < 1:
            raise ValueError(f"{who}: every k of ks must be positive, got {k}")
    return tuple(ks)


def link_ranks(z, edge_index: torch.Tensor, exclude=None, allow_loops: bool = True, splits: int = 0) -> LinkRanks:
    """The filtered counts of Rule F for the query pairs ``edge_index [2, Q]`` (``edge_index[0]`` the source): a ``LinkRanks``.

    ``z``, ``exclude``, ``allow_loops``, ``splits``: exactly as ``topk_links`` takes them -- a float32 tensor ``[N, F]`` or a pair
    ``(z_src, z_dst)``, pitched views stay views; None, a ``KnownLinks`` (built once) or the ``[2, E]`` LongTensor of known edges
    (sorted on every call); ``allow_loops=False`` (one id space only): ``(v, v)`` is no competitor; ``splits``: column ranges
    counted separately (0: chosen from the sizes), the result does not depend on it.

    The target of a query is always ranked and is never its own competitor, also when the pair is in ``exclude`` or is a loop.  A
    pair with an id out of range, or with a NaN score, gets ``-1`` counts and is reported through the status word
    (``graph.check_pending()`` raises), as is a NaN competitor score, which is not counted.  Nothing is read back, so with a
    ``KnownLinks`` (or no exclusion) the call may run inside a stream capture."""
    who = "link_ranks"
    z_src, z_dst, n_src, n_dst = _pair_tables(z, None, who)
    if not isinstance(edge_index, torch.Tensor):
        raise TypeError(f"{who}: edge_index is a LongTensor of shape [2, Q], got {type(edge_index).__name__}")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"{who}: edge_index is a LongTensor of shape [2, Q] (got {edge_index.dtype} {tuple(edge_index.shape)})")
    if edge_index.size(1) >= _LIMIT:
        raise ValueError(f"{who}: more than 2^31 - 2 query pairs in one call")
    if isinstance(splits, bool) or not isinstance(splits, int):
        raise TypeError(f"{who}: splits must be an int, got {type(splits).__name__}")
    if splits < 0:
        raise ValueError(f"{who}: splits must be 0 (choose) or positive, got {splits}")
    if not allow_loops and z_dst is not None:
        raise ValueError(f"{who}: allow_loops=False belongs to one id space (z a single tensor)")
    if exclude is not None and not isinstance(exclude, KnownLinks):
        exclude = _edge_list(exclude, who)
    dev = require_gpu(z_src, z_dst, edge_index, exclude if isinstance(exclude, torch.Tensor) else None)
    if isinstance(exclude, torch.Tensor):
        exclude = KnownLinks(exclude, (n_src, n_dst)) if exclude.size(1) > 0 else None
    if exclude is not None:
        if exclude.size != (n_src, n_dst):
            raise ValueError(f"{who}: the KnownLinks were built for size {exclude.size}, the tables have {(n_src, n_dst)} rows")
        if exclude.device != dev:
            raise NpiError(f"tensors on different devices: {dev} vs {exclude.device}")
    z_src = _pitched(z_src.detach())
    z_dst = z_src if z_dst is None else _pitched(z_dst.detach())
    src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
    Q = int(src.numel())
    counts = torch.empty((Q, 4), dtype=torch.int64, device=dev)
    score = torch.empty(Q, dtype=torch.float32, device=dev)
    if Q == 0:
        return LinkRanks(counts, score)
    lib = load()
    nbytes = int(lib.npi_link_ranks_workspace_bytes(Q, n_dst, splits))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    side = None if exclude is None else exclude.side
    check(lib.npi_link_ranks(ptr(src), ptr(dst), Q, ptr(z_src), z_src.stride(0), n_src, ptr(z_dst), z_dst.stride(0), n_dst,
                             z_src.size(1), 0 if side is None else ptr(side.rowptr), 0 if side is None else ptr(side.col),
                             0 if allow_loops else NPI_LINK_RANK_NO_LOOPS, splits, ptr(counts), ptr(score), ptr(ws), nbytes,
                             ptr(status), stream_ptr(dev)), "npi_link_ranks")
    _graph.note_status(status)
    return LinkRanks(counts, score)


def ranking_metrics(z, pos_edge_index: torch.Tensor, exclude=None, ks: Sequence[int] = (1, 3, 10), ties: str = "average",
                    allow_loops: bool = True, splits: int = 0) -> Dict[str, torch.Tensor]:
    """``{"mrr", "mean_rank", "hits@k" for k in ks}`` of the positives ``pos_edge_index [2, Q]`` in the filtered setting
    (``link_ranks`` then ``LinkRanks.metrics``): 0-d float64 device tensors, no host read."""
    ks = _check_ks(ks, "ranking_metrics")
    if ties not in TIES:
        raise ValueError(f"ranking_metrics: ties is one of {TIES}, got {ties!r}")
    return link_ranks(z, pos_edge_index, exclude=exclude, allow_loops=allow_loops, splits=splits).metrics(ks, ties)
