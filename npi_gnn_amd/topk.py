"""Top-k link prediction on the MI355X: for every query row the ``k`` targets it most likely links to and has no known edge to::

    known = npi.KnownLinks(edge_index, size)                   # the known edges by source, columns sorted; built once
    scores, ids = npi.topk_links(z, k, exclude=known)          # f32 [R, k] logits, int64 [R, k] target ids; every source row
    scores, ids = npi.topk_links((z_rna, z_protein), 10, exclude=known, rows=some_rna)
    prob, ids = npi.InnerProductDecoder().topk(z, k, exclude=known)       # scores through sigmoid, as ``forward`` does
    prob, ids = model.predict(z, k, train_edge_index)                     # GAE: one id space never returns (v, v)

PyG 1.4.2 offers ``InnerProductDecoder.forward_all`` for this -- the dense ``[N, N]`` product, which this package declines --
and the reference scores its case studies pair by pair on the host (``src/case_study*.py``).  Here it is Rule K of
``include/npi_gnn.h`` (``npi_topk_links``): the scores of a tile of 64 queries x 128 targets on the f32 matrix cores, the known
edges masked and each row's best ``k`` kept on the chip; no score matrix is written.  The answer is unique -- descending score,
``-0.0`` equal to ``+0.0``, ties by ascending target id -- and bitwise the same for any ``splits``, any order of ``rows`` and
any repetition of the call.  Slots a row has no candidate for hold id ``-1`` and score ``-inf``.

Out of scope: gradients through the selection (the results are detached), bf16 tables, ``k > 128``, approximate search, per-pair
weights, a by-target query direction (swap the tables and flip the edge list).  CPU tensors raise ``NpiError``: there is no
CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import graph as _graph
from ._lib import NPI_TOPK_MAX, NPI_TOPK_NO_LOOPS, NpiError, check, load, ptr, require_gpu, stream_ptr
from .functional import _pair_tables, _pitched

_LIMIT = 2 ** 31 - 1


def _edge_list(edge_index, who: str) -> torch.Tensor:
    if not isinstance(edge_index, torch.Tensor):
        raise TypeError(f"{who}: the known edges are a LongTensor of shape [2, E], got {type(edge_index).__name__}")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"{who}: the known edges are a LongTensor of shape [2, E] (got {edge_index.dtype} {tuple(edge_index.shape)})")
    if edge_index.size(1) >= _LIMIT:
        raise ValueError(f"{who}: more than 2^31 - 2 edges")
    return edge_index


class KnownLinks:
    """The pairs ``topk_links`` must not return: ``edge_index [2, E]`` (``edge_index[0]`` the source, as everywhere in the bipartite
    form) as a by-source CSR with every row's columns ascending (``graph.build_side(sort_columns=True)``; parallel edges are
    kept, an id out of range is dropped and reported like a dropped edge).  ``size``: an int ``N`` (one id space) or
    ``(n_src, n_dst)``.  Built once -- one device sort -- and reused by every call."""

    def __init__(self, edge_index: torch.Tensor, size):
        who = "KnownLinks"
        edge_index = _edge_list(edge_index, who)
        if isinstance(size, bool):
            raise TypeError(f"{who}: size is an int N or a pair (n_src, n_dst)")
        if isinstance(size, int):
            size = (size, size)
        elif not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in size)):
            raise TypeError(f"{who}: size is an int N or a pair (n_src, n_dst)")
        n_src, n_dst = int(size[0]), int(size[1])
        if min(n_src, n_dst) < 1 or max(n_src, n_dst) >= _LIMIT:
            raise ValueError(f"{who}: size must lie in [1, 2^31 - 1), got {(n_src, n_dst)}")
        require_gpu(edge_index)
        self.size = (n_src, n_dst)
        self.num_edges = int(edge_index.size(1))
        self.side = _graph.build_side(edge_index[0].contiguous(), edge_index[1].contiguous(), n_src, n_dst, self_loops=False,
                                      drop_equal=False, sort_columns=True)

    @property
    def device(self) -> torch.device:
        return self.side.rowptr.device


def topk_links(z, k: int, exclude=None, rows: Optional[torch.Tensor] = None, allow_loops: bool = True,
               splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(scores, ids)``: for each query the ``k`` best targets of Rule K, ``scores`` f32 ``[R, k]`` (the logits ``<z_src[i],
    z_dst[j]>``) and ``ids`` int64 ``[R, k]``, best first.

    ``z``: a float32 tensor ``[N, F]`` (one id space) or a pair ``(z_src, z_dst)``; pitched views stay views.
    ``exclude``: None, a ``KnownLinks`` (built once), or the ``[2, E]`` LongTensor of known edges (sorted on every call).
    ``rows``: None -- every source row, in order -- or a LongTensor ``[R]`` of source ids (any order, repeats allowed).  An id
    outside ``[0, n_src)`` gets a row of ``-1`` / ``-inf`` and is reported through the status word (``graph.check_pending()`` raises).
    ``allow_loops=False`` (one id space only): ``(v, v)`` is no candidate.
    ``splits``: column ranges reduced separately (0: chosen from the sizes); the result does not depend on it.

    A NaN score is never returned and is reported through the status word.  Nothing is read back, so with a ``KnownLinks`` (or no
    exclusion) the call may run inside a stream capture.  The results carry no autograd graph."""
    who = "topk_links"
    z_src, z_dst, n_src, n_dst = _pair_tables(z, None, who)
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{who}: k must be an int, got {type(k).__name__}")
    if k < 1 or k > NPI_TOPK_MAX:
        raise ValueError(f"{who}: k must lie in [1, {NPI_TOPK_MAX}], got {k}")
    if isinstance(splits, bool) or not isinstance(splits, int):
        raise TypeError(f"{who}: splits must be an int, got {type(splits).__name__}")
    if splits < 0:
        raise ValueError(f"{who}: splits must be 0 (choose) or positive, got {splits}")
    if not allow_loops and z_dst is not None:
        raise ValueError(f"{who}: allow_loops=False belongs to one id space (z a single tensor)")
    if rows is not None:
        if not isinstance(rows, torch.Tensor):
            raise TypeError(f"{who}: rows must be a LongTensor of shape [R] or None, got {type(rows).__name__}")
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise ValueError(f"{who}: rows must be a LongTensor of shape [R] (got {rows.dtype} {tuple(rows.shape)})")
        if rows.numel() >= _LIMIT:
            raise ValueError(f"{who}: more than 2^31 - 2 query rows in one call")
    if exclude is not None and not isinstance(exclude, KnownLinks):
        exclude = _edge_list(exclude, who)
    dev = require_gpu(z_src, z_dst, rows, exclude if isinstance(exclude, torch.Tensor) else None)
    if isinstance(exclude, torch.Tensor):
        exclude = KnownLinks(exclude, (n_src, n_dst)) if exclude.size(1) > 0 else None
    if exclude is not None:
        if exclude.size != (n_src, n_dst):
            raise ValueError(f"{who}: the KnownLinks were built for size {exclude.size}, the tables have {(n_src, n_dst)} rows")
        if exclude.device != dev:
            raise NpiError(f"tensors on different devices: {dev} vs {exclude.device}")
    z_src = _pitched(z_src.detach())
    z_dst = z_src if z_dst is None else _pitched(z_dst.detach())
    rows = None if rows is None else rows.contiguous()
    R = n_src if rows is None else int(rows.numel())
    scores = torch.empty((R, k), dtype=torch.float32, device=dev)
    ids = torch.empty((R, k), dtype=torch.int64, device=dev)
    if R == 0:
        return scores, ids
    lib = load()
    nbytes = int(lib.npi_topk_links_workspace_bytes(R, n_dst, k, splits))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    side = None if exclude is None else exclude.side
    check(lib.npi_topk_links(ptr(rows), R, ptr(z_src), z_src.stride(0), n_src, ptr(z_dst), z_dst.stride(0), n_dst, z_src.size(1), k,
                             0 if side is None else ptr(side.rowptr), 0 if side is None else ptr(side.col),
                             0 if allow_loops else NPI_TOPK_NO_LOOPS, splits, ptr(scores), ptr(ids), ptr(ws), nbytes, ptr(status),
                             stream_ptr(dev)), "npi_topk_links")
    _graph.note_status(status)
    return scores, ids
