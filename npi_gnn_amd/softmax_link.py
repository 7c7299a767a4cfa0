"""The listwise link loss on the MI355X: for every positive ``(s, t)`` the log-probability of ``t`` under the softmax over EVERY
candidate target of ``s`` -- the objective whose optimum ``link_ranks`` / ``test_ranking`` measure::

    known = npi.KnownLinks(train_edge_index, size)                     # built once, as for topk_links / link_ranks
    lp = npi.link_log_softmax(z, pos_edge_index, exclude=known, scale=0.125)      # f32 [Q], differentiable
    loss = npi.listwise_loss(z, pos_edge_index, exclude=known, scale=0.125)       # 0-d f32: -lp.sum() / Q over the good pairs
    loss = model.listwise_loss(z, pos_edge_index)                      # GAE: the positives are the known edges

``ranking_loss(loss="softmax")`` trains against ``K <= 63`` sampled corruptions; this is the "1-N" / full-softmax loss of the
knowledge-graph-embedding and recommender literature, which with a small target side (NPInter2: 449 proteins) needs no sampling.
The torch route is ``F.cross_entropy(scale * z_src[src] @ z_dst.t() + mask, t)``: the dense ``[Q, n_dst]`` product, a dense mask,
the probability matrix kept for the backward, ``index_add_`` on float atomics.  Here it is Rule L of ``include/npi_gnn.h``
(``npi_softmax_link_*``): the scan of ``npi_topk_links`` with a consumer that carries an online ``(max, sum exp)`` per row, and a
recomputing backward of two more scans (query-major for ``dZ_src``, target-major for ``dZ_dst``) that never writes the
probabilities.  The target is always a candidate of its own query, also when the pair is in ``exclude`` (in training the
positives ARE the known edges); the OTHER known partners of the source are not in the denominator.

``lp`` is bitwise the same run to run and for any order or repetition of the queries; across different ``splits`` it agrees up to
rounding.  The gradients are bitwise the same run to run: no float atomics anywhere.

Out of scope: bf16 tables, grouping the queries by source to share score rows (the obvious next optimisation), per-target weights
or label smoothing, the by-target softmax (swap the tables and flip the lists), other decoders, a top-k truncated softmax,
gradients through ``scale``.  CPU tensors raise ``NpiError``: there is no CPU path.
"""
from __future__ import annotations

import torch

from . import graph as _graph
from ._lib import NPI_SOFTMAX_LINK_NO_LOOPS, NpiError, check, load, ptr, require_gpu, stream_ptr
from .functional import _PairList, _pair_grads, _pair_tables, _pitched, segsum
from .topk import KnownLinks, _edge_list


def _launch_args(z_src, z_dst, pairs: _PairList, side, flags: int, scale: float, splits: int):
    """the leading arguments the three entry points share, the tables as the kernels take them, and a workspace"""
    z_src = _pitched(z_src.detach())
    z_dst = z_src if z_dst is None else _pitched(z_dst.detach())
    dev, F = z_src.device, z_src.size(1)
    nbytes = int(load().npi_softmax_link_workspace_bytes(pairs.M, pairs.n_src, pairs.n_dst, F, splits))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    head = (ptr(pairs.src), ptr(pairs.dst), pairs.M, ptr(z_src), z_src.stride(0), pairs.n_src, ptr(z_dst), z_dst.stride(0), pairs.n_dst,
            F, 0 if side is None else ptr(side.rowptr), 0 if side is None else ptr(side.col), flags, scale, splits)
    return head, (z_src, z_dst), ws, nbytes, dev


class _LinkLogSoftmaxFn(torch.autograd.Function):
    """``(lp [Q], loss)`` of Rule L (``z_dst`` None: one table) under arbitrary upstream gradients of both.  Saved: the tables, ``lp``
    and ``lse`` (``[Q]`` each) and the pair list -- nothing of size ``Q * n_dst``."""

    @staticmethod
    def forward(ctx, z_src, z_dst, pairs: _PairList, side, flags: int, scale: float, splits: int):
        head, keep, ws, nbytes, dev = _launch_args(z_src, z_dst, pairs, side, flags, scale, splits)
        Q = pairs.M
        lp = torch.empty(Q, dtype=torch.float32, device=dev)
        lse = torch.empty(Q, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        check(load().npi_softmax_link_fwd(*head, ptr(lp), ptr(lse), ptr(loss), ptr(ws), nbytes, ptr(status), stream_ptr(dev)),
              "npi_softmax_link_fwd")
        _graph.note_status(status)
        ctx.pairs, ctx.side, ctx.flags, ctx.scale, ctx.splits = pairs, side, flags, scale, splits
        ctx.save_for_backward(z_src, z_dst, lp, lse)
        ctx.set_materialize_grads(False)
        return lp, loss

    @staticmethod
    def backward(ctx, g_lp, g_loss):
        z_src, z_dst, lp, lse = ctx.saved_tensors
        pairs, scale = ctx.pairs, ctx.scale
        one, Q = z_dst is None, pairs.M
        want_src, want_dst = ctx.needs_input_grad[0], (not one) and ctx.needs_input_grad[1]
        if not (want_src or want_dst):
            return (None,) * 7
        if Q == 0 or (g_lp is None and g_loss is None):
            return (torch.zeros_like(z_src) if want_src else None, torch.zeros_like(z_dst) if want_dst else None) + (None,) * 5
        u = None if g_lp is None else g_lp.to(torch.float32)
        if g_loss is not None:                                 # loss = -sum(lp) / Q
            share = (g_loss.to(torch.float32) * (-1.0 / Q)).expand(Q)
            u = share if u is None else u + share
        u = u.contiguous()
        # the sparse part: the target's own term u scale (1 - p_t), p_t = exp(lp) (0 for a bad pair: lp = 0), over the pair list
        d_src, d_dst = _pair_grads(pairs, z_src, z_dst, u * (-torch.expm1(lp)) * scale, want_src, want_dst)
        # the dense part: -u scale p_qj over the other candidates, by the two recomputing scans
        head, _keep, ws, nbytes, dev = _launch_args(z_src, z_dst, pairs, ctx.side, ctx.flags, scale, ctx.splits)
        F, lib = z_src.size(1), load()
        if want_src:
            dq = torch.empty((Q, F), dtype=torch.float32, device=dev)
            check(lib.npi_softmax_link_bwd_src(*head, ptr(lse), ptr(u), ptr(dq), ptr(ws), nbytes, stream_ptr(dev)),
                  "npi_softmax_link_bwd_src")
            if "query" not in pairs._sides:                    # rows: the sources, columns: the query indices
                pairs._sides["query"] = _graph.build_side(pairs.src, torch.arange(Q, dtype=torch.int64, device=dev), pairs.n_src, Q,
                                                          self_loops=False, drop_equal=False)
            d_src = d_src + segsum(None, pairs._sides["query"], dq)
        if want_dst or (one and want_src):
            dz = torch.empty((pairs.n_dst, F), dtype=torch.float32, device=dev)
            check(lib.npi_softmax_link_bwd_dst(*head, ptr(lse), ptr(u), ptr(dz), ptr(ws), nbytes, stream_ptr(dev)),
                  "npi_softmax_link_bwd_dst")
            if one:
                d_src = d_src + dz
            else:
                d_dst = d_dst + dz
        return (d_src, d_dst) + (None,) * 5


def _apply(z, edge_index, exclude, scale, allow_loops, splits, who: str):
    """the argument checks of ``topk_links`` / ``link_ranks`` -- all before any device work -- then the function"""
    z_src, z_dst, n_src, n_dst = _pair_tables(z, None, who)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"{who}: scale must be a number, got {type(scale).__name__}")
    scale = float(scale)
    if scale != scale or abs(scale) == float("inf") or scale <= 0:
        raise ValueError(f"{who}: scale must be finite and > 0 (got scale={scale})")
    if isinstance(splits, bool) or not isinstance(splits, int):
        raise TypeError(f"{who}: splits must be an int, got {type(splits).__name__}")
    if splits < 0:
        raise ValueError(f"{who}: splits must be 0 (choose) or positive, got {splits}")
    if not allow_loops and z_dst is not None:
        raise ValueError(f"{who}: allow_loops=False belongs to one id space (z a single tensor)")
    if not isinstance(edge_index, torch.Tensor):
        raise TypeError(f"{who}: edge_index is a LongTensor of shape [2, Q], got {type(edge_index).__name__}")
    pairs = _PairList(edge_index, n_src, n_dst, who)
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
    return _LinkLogSoftmaxFn.apply(z_src, z_dst, pairs, None if exclude is None else exclude.side,
                                   0 if allow_loops else NPI_SOFTMAX_LINK_NO_LOOPS, scale, splits)


def link_log_softmax(z, edge_index: torch.Tensor, exclude=None, scale: float = 1.0, allow_loops: bool = True,
                     splits: int = 0) -> torch.Tensor:
    """``lp [Q]`` (float32) of Rule L for the query pairs ``edge_index [2, Q]`` (``edge_index[0]`` the source): ``lp_q = x_t -
    logsumexp(x_j over the candidates j of s_q)`` with ``x_j = scale * <z_src[s_q], z_dst[j]>``; ``exp(lp_q)`` is the probability of
    the true target among all targets ``s_q`` has no known edge to.  Differentiable under ANY upstream gradient, to both tables.

    ``z``, ``exclude``, ``allow_loops``, ``splits``: exactly as ``topk_links`` / ``link_ranks`` take them -- a float32 tensor
    ``[N, F]`` or a pair ``(z_src, z_dst)``, pitched views stay views; None, a ``KnownLinks`` (built once) or the ``[2, E]``
    LongTensor of known edges (sorted on every call); ``allow_loops=False`` (one id space only): ``(v, v)`` is no candidate unless
    it is the target; ``splits``: ranges scanned separately (0: chosen from the sizes) -- ``lp`` agrees across ``splits`` up to
    rounding.  ``scale``: finite, > 0 (an inverse temperature; no gradient flows to it).

    The target is always a candidate, also when ``(s_q, t_q)`` is in ``exclude`` or is a loop; when it is the only one, ``lp_q`` and
    its gradients are exactly 0.  A pair with an id out of range gets ``lp_q = 0``, contributes to no gradient and is reported
    through the status word (``graph.check_pending()`` raises), as is a NaN score among the candidates, which makes ``lp_q`` NaN.

    The forward reads nothing back, so with a ``KnownLinks`` (or no exclusion) it may run inside a stream capture.  The backward
    builds the sides of the pair list its segmented sums need (``_PairList.side``: a device sort each, with allocations sized on the
    host, once per call): it may NOT be captured.  It saves the tables, ``lp``, ``lse`` and the pair list -- nothing of size ``Q *
    n_dst`` --, builds only what a table that requires grad needs, and under ``torch.no_grad()`` only the forward scan runs."""
    return _apply(z, edge_index, exclude, scale, allow_loops, splits, "link_log_softmax")[0]


def listwise_loss(z, pos_edge_index: torch.Tensor, exclude=None, scale: float = 1.0, allow_loops: bool = True,
                  splits: int = 0) -> torch.Tensor:
    """``-(sum of lp_q over the good pairs) / Q`` as a 0-d float32 (Rule L 6), ``lp`` as in ``link_log_softmax`` and the arguments as
    there.  The divisor counts pairs, not good pairs (nothing is read back); ``Q = 0`` gives 0.  The sum is the deterministic fp64
    scheme of ``link_loss`` out of the same launches that write ``lp``.  The forward may run inside a stream capture (with a
    ``KnownLinks`` or no exclusion); the backward may not (``link_log_softmax``)."""
    return _apply(z, pos_edge_index, exclude, scale, allow_loops, splits, "listwise_loss")[1]
