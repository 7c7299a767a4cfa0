"""Functional form of the conv hot path on MI355X: thin wrappers over the C ABI plus the
``torch.autograd.Function``s that give ``loss.backward()`` (reference
``src/train_with_twoDataset.PY:54``) the same gradients PyG 1.4.2's autograd graph produces.

Formulas (PyG 1.4.2):
  SAGEConv : out = mean_{j in N(i) U {i}} x_j @ W + b          (aggregate at F_in, then project)
  GCNConv  : out = sum_e norm_e (x @ W)[src e] + b,  norm_e = d^-1/2[src] w_e d^-1/2[dst],
             d = weighted out-degree incl. the self loop      (project first, aggregate at F_out)
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import torch

from ._draw import epoch_seed
from ._lib import (NPI_BF16, NPI_F32, NPI_GEMM_A_ZERO_PADDED, NPI_GEMM_EXACT_F32, NPI_GEMM_RESERVE_CUS, NPI_GEMM_SPLIT_F16X2,
                   NPI_GEMM_WORKSPACE_PREPARED, NPI_GAUSS_KL, NPI_GAUSS_SAMPLE, NPI_GROUP_LOGITS, NPI_GROUP_LOSS_BPR, NPI_GROUP_LOSS_MARGIN,
                   NPI_GROUP_LOSS_SOFTMAX, NPI_PAIR_LOGITS, NPI_PAIR_LOSS_BCE, NPI_PAIR_LOSS_GAE, NPI_PREPARE_F16X2, check, load, ptr,
                   require_gpu, stream_ptr)
from .graph import BipartiteGraph, CSRGraph, CSRSide, GraphBatch, HubPlan, as_graph, build_side, note_status, pair_list_side
from .schedule import DEFAULT, Schedule


_PROFILE = None     # bench.py sets this to a list to collect (start, end) events per segsum launch
_PROFILE_TAGS = None  # bench.py: dict tag -> list of (start, end) events around the GAT aggregation launches


class _tag_events:
    """HIP events on the launch stream around one aggregation launch, filed under ``tag`` (a no-op unless bench.py asked)"""

    def __init__(self, tag, dev):
        self.rec = _PROFILE_TAGS
        if self.rec is not None:
            self.tag, self.dev = tag, dev
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.rec is not None:
            self.e0.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            self.e1.record(torch.cuda.current_stream(self.dev))
            self.rec.setdefault(self.tag, []).append((self.e0, self.e1))
        return False

_PROFILE_GEMM = None  # likewise (name, flops, start, end) per projection GEMM, on the stream it is launched on


class _gemm_events:
    """HIP events around one GEMM entry point when bench.py asked for them (a no-op otherwise)."""

    def __init__(self, name, flops, dev):
        self.rec = _PROFILE_GEMM
        if self.rec is not None:
            self.name, self.flops, self.dev = name, flops, dev
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.rec is not None:
            self.e0.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            self.e1.record(torch.cuda.current_stream(self.dev))
            self.rec.append((self.name, self.flops, self.e0, self.e1))
        return False

# dW = agg^T dOut (MFMA-bound, launched as ONE workgroup per CU so that it leaves wave slots, LDS and
# registers free) runs on a side stream under the dX chain, whose aggregation is HBM-bound: the two then
# share every CU instead of queueing.  Measured at C4: 8.0 -> 7.1 ms per step.  (With the dW grid
# filling the chip twice over, as before, the same overlap gained 1 %.)  Only for graphs large enough
# for the kernels to outlast the stream bookkeeping (Schedule.overlap_streams / overlap_min_rows).
_SIDE_STREAMS = {}


def _overlaps(sch: Schedule, rows: int) -> bool:
    return sch.overlap_streams and rows >= sch.overlap_min_rows


def _side_stream(dev, k: int = 0) -> "torch.cuda.Stream":
    s = _SIDE_STREAMS.get((dev, k))
    if s is None:
        s = torch.cuda.Stream(device=dev)          # (a high-priority stream made no difference)
        _SIDE_STREAMS[(dev, k)] = s
    return s


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


def _fc(t: torch.Tensor, name: str, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 or bfloat16 storage (bf16: f32 accumulation inside the kernels); all operands alike."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name} must be float32 or bfloat16 (got {t.dtype})")
    if like is not None and t.dtype != like.dtype:
        raise TypeError(f"{name} is {t.dtype} but the other operand is {like.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _fcp(t: torch.Tensor, name: str) -> torch.Tensor:
    """as ``_fc``, but a 2-D operand may keep a row pitch (a column block of a wider buffer): the kernels take a leading
    dimension"""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.size(1):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{name} must be float32 or bfloat16 (got {t.dtype})")
        return t
    return _fc(t, name)


def _code(t: torch.Tensor) -> int:
    return NPI_BF16 if t.dtype == torch.bfloat16 else NPI_F32


def _check_out(out: torch.Tensor, rows: int, cols: int, like: torch.Tensor, what: str) -> None:
    """``out=`` buffers go straight to a kernel that writes ``rows`` rows of ``cols`` elements: anything else would be an
    out-of-bounds device write, so it is an error here (a slice of a larger buffer with a row pitch is fine)"""
    if (out.dim() != 2 or out.size(0) != rows or out.size(1) != cols or out.dtype != like.dtype or out.stride(1) != 1
            or out.device != like.device):
        raise ValueError(f"{what}: out must be [{rows}, {cols}] {like.dtype} with unit column stride on {like.device} "
                         f"(got {tuple(out.shape)} {out.dtype}, strides {tuple(out.stride())}, {out.device})")


def _out_or_new(out: Optional[torch.Tensor], rows: int, cols: int, like: torch.Tensor, what: str) -> torch.Tensor:
    """the ``out=`` of a wrapper: a new ``[rows, cols]`` tensor like ``like``, or the caller's once ``_check_out`` passes it"""
    if out is None:
        return torch.empty((rows, cols), dtype=like.dtype, device=like.device)
    _check_out(out, rows, cols, like, what)
    return out


def _second_part(part2: Optional[torch.Tensor], part1: torch.Tensor, name: str) -> Optional[torch.Tensor]:
    """the second part of a two-part gathered table (the GAT wrappers): float32, contiguous, the row pitch of the first"""
    if part2 is None:
        return None
    part2 = _f32c(part2, name)
    if part2.stride(0) != part1.stride(0):
        raise ValueError("the two parts of the table must share the row pitch")
    return part2


# ---------------------------------------------------------------------------------------------
# raw ops
# ---------------------------------------------------------------------------------------------
def segsum_scales_ok(side: CSRSide, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> bool:
    """can ``segsum(..., scales_out=)`` write the finished rows' power-of-two scales (f32 rows of 256 columns, 16-byte aligned)?"""
    return (x.dtype == torch.float32 and x.size(1) == 256 and side.nnz_max > 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
            and (out is None or (out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0)))


def segsum(graph: CSRGraph, side: CSRSide, x: torch.Tensor, w: Optional[torch.Tensor] = None,
           mean: bool = False, bias: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None,
           scales_out: Optional[torch.Tensor] = None, hub: Optional[HubPlan] = None,
           col_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = scale_i * sum_{p in row i} w[p] * x[col[p]] (+ bias): fused gather + segmented
    reduction (``npi_segsum``).  ``x2``: second part of a two-part table -- entries with
    ``col >= x.size(0)`` read ``x2[col - x.size(0)]`` (``npi_segsum_ex``; the sharded layers).
    ``scales_out`` ``[n_rows]`` f32: also the power-of-two scale of every finished row (what ``row_scales(out)`` would compute in
    a pass of its own; ``segsum_scales_ok``) for the fp16 x 2 projection behind the aggregation.
    ``hub``: ``side``'s plan (``hub_plan_for``) -- the plain launch walks ``hub.light`` (``w``: ITS per-entry weights) and the hub
    rows are summed by streaming the table (``npi_segsum_hub``, same stream): ``out[hub j] = sum_r col_scale[r] x[r]`` over the
    source rows ``r`` of hub j (``col_scale`` ``[n_cols]`` f32 or None: ones), divided by the ORIGINAL row's count under ``mean``."""
    dev = require_gpu(x, w, bias, x2, col_scale)
    x = _fcp(x, "x")
    if bias is not None:
        bias = _fc(bias, "bias", x)
    N, F = side.n_rows, x.size(1)                  # `graph` may be None for a stand-alone (sharded) side
    split = x.size(0)
    if x2 is not None:
        x2 = _fcp(x2, "x2")                         # (may be a column block of the buffer x is a block of: same pitch)
        if x2.dtype != x.dtype:
            raise TypeError(f"x2 is {x2.dtype} but the other operand is {x.dtype}")
        if x2.size(1) != F:
            raise ValueError("x2 must have the width of x")
        if x2.stride(0) != x.stride(0):
            x2 = x2.contiguous()
            if x2.stride(0) != x.stride(0):
                x = x.contiguous()
    if side.n_cols > split + (x2.size(0) if x2 is not None else 0):
        raise ValueError(f"the table has {split + (x2.size(0) if x2 is not None else 0)} rows, the adjacency indexes {side.n_cols}")
    if out is None:
        out = torch.empty((N, F), dtype=x.dtype, device=dev)
    else:
        _check_out(out, N, F, x, "segsum")
    full = side
    if hub is not None:
        if not (x.dtype == torch.float32 and F == 256 and x2 is None and bias is None and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
                and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0 and hub.light.n_rows == N):
            raise ValueError("segsum(hub=): the streaming path takes one f32 table of 256 columns, 16-byte aligned rows, no bias")
        if col_scale is not None:
            col_scale = _f32c(col_scale, "col_scale")
            if col_scale.numel() != side.n_cols:
                raise ValueError(f"segsum: col_scale has {col_scale.numel()} elements, the table {side.n_cols} rows")
        side = hub.light
    elif col_scale is not None:
        raise ValueError("segsum: col_scale belongs to the streaming path (hub=); the plain launch takes per-entry weights")
    carry = side.carry(F)
    prof = _PROFILE
    if prof is not None:        # bench.py: HIP events on the launch stream around this launch
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(dev))
    if scales_out is not None and (scales_out.dtype != torch.float32 or scales_out.numel() != N or not scales_out.is_contiguous()):
        raise ValueError("segsum: scales_out must be a contiguous float32 vector with one element per output row")
    check(load().npi_segsum_ex(ptr(side.rowptr), ptr(side.col), ptr(side.item_row), side.item, ptr(w), N, side.nnz_max,
                                ptr(x), x.stride(0), ptr(x2), split if x2 is not None else 0, ptr(out), out.stride(0), F,
                                _code(x), 1 if mean else 0, ptr(bias), ptr(carry), ptr(scales_out), stream_ptr(dev)), "npi_segsum")
    if hub is not None:
        check(load().npi_segsum_hub(ptr(hub.hub_rows), hub.H, ptr(hub.mask), ptr(full.rowptr), N, full.n_cols, ptr(col_scale), ptr(x),
                                    x.stride(0), ptr(out), out.stride(0), F, 1 if mean else 0, ptr(hub.partial()), ptr(scales_out),
                                    stream_ptr(dev)), "npi_segsum_hub")
    if prof is not None:
        ev1.record(torch.cuda.current_stream(dev))
        prof.append((ev0, ev1))
    return out


def hub_plan_for(graph: CSRGraph, side: CSRSide, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[HubPlan]:
    """``side``'s hub plan when the aggregation of ``x`` over it may take the streaming path (``CSRGraph.hub_stream``; f32, 256
    columns, 16-byte aligned rows) and the side has one; else None: the plain launch."""
    if not graph.hub_stream or not segsum_scales_ok(side, x, out) or x.size(0) != side.n_cols:
        return None
    return side.hub_plan()


# Arithmetic of the f32 projection GEMMs: an argument of every call (``flags``: 0 = the split on the 16-bit matrix cores,
# NPI_GEMM_EXACT_F32 = the exact-f32 MFMA kernels), and of every layer (``Schedule.f16x2_min_rows``: from how many rows on the
# layers' GEMMs take two fp16 pieces per operand).  Neither the library (ABI 3 on) nor this module keeps a switch.


def _gflags(sch: Schedule) -> int:
    """the ``flags`` a layer under schedule ``sch`` hands to its projection GEMMs (``Schedule.gemm_exact_f32``)"""
    return NPI_GEMM_EXACT_F32 if sch.gemm_exact_f32 else 0


def _f16x2(sch: Schedule, rows: int, K: int, N: int, dtype) -> bool:
    """does a layer under schedule ``sch`` run its f32 projection GEMMs (contraction K, output width N, ``rows`` rows) on two fp16
    pieces per operand (NPI_GEMM_SPLIT_F16X2: three matrix products per tile pair instead of six, the same f32-rounding-level error)?"""
    return (sch.f16x2_min_rows is not None and not sch.gemm_exact_f32 and rows >= sch.f16x2_min_rows and dtype == torch.float32
            and f16x2_shape(rows, K, N))


def _gemm_workspace(K: int, N: int, dev) -> torch.Tensor:
    """caller-owned scratch for the re-laid weight matrix: the library allocates nothing"""
    return torch.empty(int(load().npi_linear_workspace_bytes(K, N)), dtype=torch.uint8, device=dev)


def _pad128(k: int) -> int:
    return (int(k) + 127) // 128 * 128


def padded_aggregate_buffer(x: torch.Tensor, K: int, rows: int, bf16_ok: bool = False):
    """A zeroed ``[rows, Kp]`` f32 buffer (Kp = K rounded up to 128) whose first K columns the aggregation fills, or None.
    The reference's feature width is 178: with the aggregate kept 256 wide and its pad columns zero, the layer's forward GEMM and
    its weight-gradient GEMM take the matrix-core kernels (``NPI_GEMM_A_ZERO_PADDED``) instead of the guarded ones -- what
    ``InteractionGraph.batch`` does for extracted batches, here for features the caller hands over 178 wide.  Only when the
    padding costs less than half as much again (178 -> 256 yes, 65 -> 128 no).  (bf16 storage has no padded-operand flag: the
    layer pads its weight matrix with zero rows instead, ``_AggProjectFn``.)"""
    if (x.dtype not in ((torch.float32, torch.bfloat16) if bf16_ok else (torch.float32,)) or x.size(1) != K or K % 128 == 0
            or 2 * _pad128(K) > 3 * K or rows < 128):
        return None
    return torch.zeros((rows, _pad128(K)), dtype=x.dtype, device=x.device)


def f16x2_shape(M: int, K: int, N: int) -> bool:
    """shapes whose f32 projection GEMMs (contraction K, output width N, M rows) take the matrix-core kernel completely, i.e. where
    ``NPI_GEMM_SPLIT_F16X2`` applies to every output tile"""
    return M >= 128 and K % 32 == 0 and N % 128 == 0


def _check_scales(scales: Optional[torch.Tensor], rows: int, what: str) -> None:
    """the kernels read one scale per row of the left operand: anything else would be an out-of-bounds device read"""
    if scales is not None and (scales.dtype != torch.float32 or scales.dim() != 1 or scales.numel() != rows or not scales.is_contiguous()):
        raise ValueError(f"{what}: the row scales must be a contiguous float32 vector with one element per row ({rows}), "
                         f"got {tuple(scales.shape)} {scales.dtype}")


def row_scales(a: torch.Tensor) -> torch.Tensor:
    """``[M]`` power-of-two scales of the rows of ``a`` (``npi_row_scales``): the ``a_scales`` of ``linear_fwd`` /
    ``linear_bwd_data`` under ``NPI_GEMM_SPLIT_F16X2`` (two fp16 pieces per operand, three matrix products instead of six)"""
    dev = require_gpu(a)
    if a.dtype != torch.float32 or a.dim() != 2 or a.stride(1) != 1:
        raise TypeError("row_scales: a float32 matrix with unit column stride")
    out = torch.empty(a.size(0), dtype=torch.float32, device=dev)
    check(load().npi_row_scales(ptr(a), a.stride(0), a.size(0), a.size(1), ptr(out), stream_ptr(dev)), "npi_row_scales")
    return out


class Planes:
    """A re-laid copy of a weight matrix for the matrix-core GEMMs (``npi_linear_prepare``) and the arithmetic it was laid out for:
    three bf16 planes (``f16`` False; bf16 storage: one k-block-major copy) or the two fp16 planes + column scales of
    ``NPI_GEMM_SPLIT_F16X2`` calls.  The library cannot tell the two layouts apart, so the tag travels with the buffer and
    ``linear_fwd`` / ``linear_bwd_data`` refuse a copy of the other kind."""
    __slots__ = ("buf", "f16")

    def __init__(self, buf: torch.Tensor, f16: bool = False):
        self.buf, self.f16 = buf, bool(f16)


def _planes_for(ws: Optional["Planes"], f16: bool, what: str) -> torch.Tensor:
    if not isinstance(ws, Planes):
        raise TypeError(f"{what}: ws must come from prepare_weight (a functional.Planes)")
    if ws.f16 != f16:
        raise ValueError(f"{what}: the prepared weight copy holds {'fp16 x 2' if ws.f16 else 'bf16 x 3'} planes, this call runs on "
                         f"{'fp16 x 2 (row scales given)' if f16 else 'bf16 x 3 (no row scales)'}: prepare_weight(..., f16={f16})")
    return ws.buf


def prepare_weight(weight: torch.Tensor, backward: bool = True, f16: bool = False):
    """The re-laid copies of ``weight [K, N]`` the matrix-core GEMMs read (three bf16 planes for f32, a k-block-major copy for
    bf16; ``f16``: the two fp16 planes + column scales of ``NPI_GEMM_SPLIT_F16X2`` calls) for ``linear_fwd(..., ws=)`` and --
    ``backward`` -- ``linear_bwd_data(..., ws=)``, written by ONE launch
    (``npi_linear_prepare``) instead of one in front of every GEMM: ``(ws_fwd, ws_bwd or None)``, or ``(None, None)`` when the
    shape does not take those kernels anyway.  Valid while ``weight`` is unchanged (a layer's forward and its backward)."""
    K, N = weight.shape
    if (weight.dtype not in (torch.float32, torch.bfloat16) or K % 32 or N % 32 or weight.stride(1) != 1
            or not weight.is_cuda or (f16 and weight.dtype != torch.float32)):
        return None, None
    lib = load()
    dev = weight.device
    one = int(lib.npi_linear_workspace_bytes(K, N))
    ws = torch.empty(one * (2 if backward else 1), dtype=torch.uint8, device=dev)
    check(lib.npi_linear_prepare(ptr(weight), weight.stride(0), K, N, (3 if backward else 1) | (NPI_PREPARE_F16X2 if f16 else 0),
                                 _code(weight), ptr(ws), ws.numel(), stream_ptr(dev)), "npi_linear_prepare")
    return Planes(ws[:one], f16), (Planes(ws[one:], f16) if backward else None)


def _linear_call(flags: Optional[int], reserve_cus: int, scales: Optional[torch.Tensor], ws, *, f16_ok: bool, K: int, N: int, dev,
                 what: str):
    """what ``linear_fwd`` / ``linear_bwd_data`` make of their arithmetic arguments: ``(flags, scales or None, workspace tensor)``.
    ``f16_ok``: storage and shape serve the fp16 x 2 kernel (row scales given for anything else are dropped); ``ws``: the prepared
    copy to read (a ``Planes`` of the matching kind), or None for a scratch workspace of ``[K, N]``."""
    fl = int(flags or 0) | NPI_GEMM_RESERVE_CUS(reserve_cus)
    if scales is not None and (not f16_ok or fl & NPI_GEMM_EXACT_F32):
        scales = None                                           # (storage / flags the fp16 x 2 kernel does not serve)
    if scales is not None:
        fl |= NPI_GEMM_SPLIT_F16X2
    if ws is not None:
        return fl | NPI_GEMM_WORKSPACE_PREPARED, scales, _planes_for(ws, scales is not None, what)
    return fl, scales, _gemm_workspace(K, N, dev)


def linear_fwd(a: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
               rowscale: Optional[torch.Tensor] = None, relu: bool = False, flags: Optional[int] = None,
               out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, reserve_cus: int = 0,
               a_scales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``a @ weight + bias``.  ``a`` may be wider than ``weight`` has rows: ``[M, Kp]`` with Kp = K rounded up to 128 and
    the columns K.. ZERO (``NPI_GEMM_A_ZERO_PADDED``: the matrix-core kernel on Kp instead of the guarded one on an odd K).
    ``out``: write into this ``[M, N]`` tensor (rows may have a pitch; same dtype) instead of a new one.  ``ws``: the forward
    copy of ``prepare_weight(weight)`` -- no preparation launch in front of the GEMM.  ``reserve_cus``: leave that many CUs (a
    multiple of 8) to a kernel that runs beside the GEMM (``NPI_GEMM_RESERVE_CUS``; the sharded layers, ``Schedule.gemm_reserve_cus``).
    ``a_scales``: ``row_scales(a)`` -- the GEMM then runs on two fp16 pieces per operand (``NPI_GEMM_SPLIT_F16X2``: half the matrix
    work, the same f32-level accuracy); a ``ws`` handed over with it must come from ``prepare_weight(..., f16=True)``."""
    dev = require_gpu(a, weight, bias, rowscale, a_scales)
    a = _fc(a, "a")
    weight = _fc(weight, "weight", a)
    if bias is not None:
        bias = _fc(bias, "bias", a)
    M, Ka = a.shape
    K, N = weight.shape
    if Ka != K and (Ka != _pad128(K) or a.dtype != torch.float32):
        raise ValueError(f"a has {Ka} columns, weight {K} rows (a zero-padded a must be f32 and {_pad128(K)} wide)")
    out = _out_or_new(out, M, N, a, "linear_fwd")
    _check_scales(a_scales, M, "linear_fwd")
    padded = Ka != K                                            # neither a prepared copy nor fp16 x 2 serves a zero-padded a
    fl, a_scales, ws = _linear_call(int(flags or 0) | (NPI_GEMM_A_ZERO_PADDED if padded else 0), reserve_cus, a_scales,
                                    None if padded else ws, f16_ok=a.dtype == torch.float32 and not padded, K=Ka, N=N, dev=dev,
                                    what="linear_fwd")
    with _gemm_events("fwd", 2.0 * M * K * N, dev):
        check(load().npi_linear_fwd_ex(ptr(a), a.stride(0), ptr(weight), weight.stride(0), ptr(bias), ptr(rowscale),
                                        ptr(out), out.stride(0), M, K, N, 1 if relu else 0, _code(a),
                                        fl, ptr(ws), ws.numel(), ptr(a_scales), stream_ptr(dev)),
              "npi_linear_fwd")
    return out


def linear_bwd_data(dc: torch.Tensor, weight: torch.Tensor,
                    rowscale: Optional[torch.Tensor] = None, flags: Optional[int] = None,
                    out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, reserve_cus: int = 0,
                    dc_scales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rowscale * (dc @ weight.T)``; ``out``: write into this ``[M, K]`` tensor (a row block of a larger buffer); ``ws``: the
    backward copy of ``prepare_weight(weight)``; ``dc_scales``: ``row_scales(dc)`` -- the fp16 x 2 arithmetic, as in ``linear_fwd``."""
    dev = require_gpu(dc, weight, rowscale, dc_scales)
    dc = _fc(dc, "dC")
    weight = _fc(weight, "weight", dc)
    M, N = dc.shape
    K = weight.size(0)
    da = _out_or_new(out, M, K, dc, "linear_bwd_data")
    _check_scales(dc_scales, M, "linear_bwd_data")
    fl, dc_scales, ws = _linear_call(flags, reserve_cus, dc_scales, ws, f16_ok=dc.dtype == torch.float32, K=K, N=N, dev=dev,
                                     what="linear_bwd_data")
    with _gemm_events("bwd_data", 2.0 * M * K * N, dev):
        check(load().npi_linear_bwd_data_ex(ptr(dc), dc.stride(0), ptr(weight), weight.stride(0), ptr(rowscale),
                                             ptr(da), da.stride(0), M, K, N, _code(dc),
                                             fl, ptr(ws), ws.numel(), ptr(dc_scales), stream_ptr(dev)),
              "npi_linear_bwd_data")
    return da


def linear_fwd_scores_ok(a: torch.Tensor, weight: torch.Tensor) -> bool:
    """can ``linear_fwd_scores`` take these operands (f32, aligned, one column tile of the split kernel covers the output)?"""
    return (a.dtype == torch.float32 and weight.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1
            and weight.stride(1) == 1 and a.stride(0) % 4 == 0 and weight.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0
            and weight.data_ptr() % 16 == 0
            and bool(load().npi_linear_fwd_scores_supported(a.size(0), weight.size(0), weight.size(1))))


def linear_fwd_scores(a: torch.Tensor, weight: torch.Tensor, att2: torch.Tensor, a_scales: Optional[torch.Tensor] = None):
    """``(h, a_dst, a_src)``: ``h = a @ weight`` and the row dots ``h @ att[:N]``, ``h @ att[N:]`` taken from the accumulators in
    the GEMM's store epilogue (``npi_linear_fwd_scores``; one head, ``att2`` holds ``2 N`` values)."""
    dev = require_gpu(a, weight, att2)
    M, K = a.shape
    N = weight.size(1)
    att2 = _f32c(att2.reshape(-1), "att")
    if att2.numel() != 2 * N:
        raise ValueError("linear_fwd_scores: att must hold 2 N values")
    _check_scales(a_scales, M, "linear_fwd_scores")
    h = torch.empty((M, N), dtype=torch.float32, device=dev)
    a_dst = torch.empty((M, 1), dtype=torch.float32, device=dev)
    a_src = torch.empty((M, 1), dtype=torch.float32, device=dev)
    ws = _gemm_workspace(K, N, dev)
    with _gemm_events("fwd", 2.0 * M * K * N, dev):
        check(load().npi_linear_fwd_scores(ptr(a), a.stride(0), ptr(weight), weight.stride(0), ptr(att2), ptr(h), h.stride(0),
                                               ptr(a_dst), ptr(a_src), M, K, N, ptr(ws), ws.numel(), ptr(a_scales), stream_ptr(dev)),
              "npi_linear_fwd_scores")
    return h, a_dst, a_src


def linear_bwd_data_rank2_ok(dc: torch.Tensor, weight: torch.Tensor) -> bool:
    """can ``linear_bwd_data_rank2`` take these operands (f32, aligned, a shape the split kernel covers completely)?"""
    M, N = dc.shape
    return (dc.dtype == torch.float32 and weight.dtype == torch.float32 and dc.stride(1) == 1 and weight.stride(1) == 1
            and dc.stride(0) % 4 == 0 and weight.stride(0) % 4 == 0 and dc.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0
            and bool(load().npi_linear_bwd_data_rank2_supported(M, weight.size(0), N)))


def linear_bwd_data_rank2(dc: torch.Tensor, weight: torch.Tensor, row0: torch.Tensor, row1: torch.Tensor,
                          col0: torch.Tensor, col1: torch.Tensor, dc_scales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dc @ weight.T + row0 (x) col0 + row1 (x) col1`` with the rank-2 term added in the GEMM's store epilogue
    (``npi_linear_bwd_data_rank2``; ``row*`` are ``[M]``, ``col*`` ``[K]``)."""
    dev = require_gpu(dc, weight, row0, row1, col0, col1)
    M, N = dc.shape
    K = weight.size(0)
    if row0.numel() != M or row1.numel() != M or col0.numel() != K or col1.numel() != K:
        raise ValueError("linear_bwd_data_rank2: row vectors must have M entries, column vectors K")
    row0, row1, col0, col1 = (_f32c(t.reshape(-1), "rank-2 vector") for t in (row0, row1, col0, col1))
    _check_scales(dc_scales, M, "linear_bwd_data_rank2")
    da = torch.empty((M, K), dtype=torch.float32, device=dev)
    ws = _gemm_workspace(K, N, dev)
    with _gemm_events("bwd_data", 2.0 * M * K * N, dev):
        check(load().npi_linear_bwd_data_rank2(ptr(dc), dc.stride(0), ptr(weight), weight.stride(0), ptr(row0), ptr(row1),
                                               ptr(col0), ptr(col1), ptr(da), da.stride(0), M, K, N, ptr(ws), ws.numel(), ptr(dc_scales),
                                               stream_ptr(dev)), "npi_linear_bwd_data_rank2")
    return da


def gat_rank2_cols(weight: torch.Tensor, att2: torch.Tensor) -> torch.Tensor:
    """``U [2, K] = [att_dst ; att_src] @ weight.T`` (one head; ``att2`` is ``[1, 2C]`` or ``[2, C]``): the column vectors of
    ``linear_bwd_data_rank2`` (``npi_gat_rank2_cols``)"""
    dev = require_gpu(weight, att2)
    weight, att2 = _f32c(weight, "weight"), _f32c(att2.reshape(2, -1), "att")
    K, C = weight.shape
    U = torch.empty((2, K), dtype=torch.float32, device=dev)
    check(load().npi_gat_rank2_cols(ptr(weight), weight.stride(0), ptr(att2), K, C, ptr(U), stream_ptr(dev)), "npi_gat_rank2_cols")
    return U


def gat_rank2_tail(P: torch.Tensor, weight: torch.Tensor, att2: torch.Tensor, dw: Optional[torch.Tensor], want_datt: bool):
    """``dw += P.T @ att`` in place (``dw`` None: skipped) and, when asked, ``datt [2, C] = P @ weight`` -- one launch
    (``npi_gat_rank2_tail``); P is ``[2, K]`` = x^T [g_dst g_src]"""
    dev = require_gpu(P, weight, att2, dw)
    P, weight, att2 = _f32c(P, "P"), _f32c(weight, "weight"), _f32c(att2.reshape(2, -1), "att")
    K, C = weight.shape
    if dw is not None and (dw.shape != (K, C) or dw.dtype != torch.float32 or dw.stride(1) != 1):
        raise ValueError("gat_rank2_tail: dw must be a [K, C] float32 tensor with unit column stride")
    datt = torch.empty((2, C), dtype=torch.float32, device=dev) if want_datt else None
    if dw is None and datt is None:
        return None
    check(load().npi_gat_rank2_tail(ptr(P), ptr(weight), weight.stride(0), ptr(att2), K, C, ptr(dw),
                                    dw.stride(0) if dw is not None else 0, ptr(datt), stream_ptr(dev)), "npi_gat_rank2_tail")
    return datt


def col_scales(a: Optional[torch.Tensor] = None, row_scales: Optional[torch.Tensor] = None, cols: Optional[int] = None) -> torch.Tensor:
    """``[K]`` power-of-two COLUMN scales for ``linear_bwd_weight(a_cs=, dc_cs=)`` (``npi_col_scales``): from the column maxima
    of ``a`` (one pass over it -- for a matrix that does not change between steps, once), or -- ``a`` None -- the smallest of the
    ``row_scales`` its producer wrote, for each of ``cols`` columns alike (no pass over the matrix; two small launches on every
    call -- a library launch or a graph replay rewrites a scales tensor without torch seeing it, so nothing is kept between calls)."""
    lib = load()
    if a is not None:
        dev = require_gpu(a)
        if a.dtype != torch.float32 or a.dim() != 2 or a.stride(1) != 1:
            raise TypeError("col_scales: a float32 matrix with unit column stride")
        M, K = a.shape
    else:
        if row_scales is None or cols is None:
            raise ValueError("col_scales: a matrix, or its row scales and its column count")
        dev = require_gpu(row_scales)
        _check_scales(row_scales, row_scales.numel(), "col_scales")
        M, K = int(row_scales.numel()), int(cols)
    n_ws = int(lib.npi_col_scales_workspace_elems(M, K))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    out = torch.empty(K, dtype=torch.float32, device=dev)
    check(lib.npi_col_scales(ptr(a), a.stride(0) if a is not None else 0, M, K, ptr(row_scales) if a is None else 0, ptr(out), ptr(ws),
                             n_ws, stream_ptr(dev)), "npi_col_scales")
    return out


def dw_f16x2_shape(M: int, K: int, N: int) -> bool:
    """shapes whose f32 weight-gradient GEMM takes the fp16 x 2 matrix-core kernel (``linear_bwd_weight(a_cs=, dc_cs=)``)"""
    return M >= 4096 and K % 128 == 0 and N % 128 == 0


def linear_bwd_weight(a: torch.Tensor, dc: torch.Tensor, want_bias: bool = True, shared: bool = False,
                      flags: Optional[int] = None, k_valid: Optional[int] = None, a_cs: Optional[torch.Tensor] = None,
                      dc_cs: Optional[torch.Tensor] = None):
    """``shared``: the GEMM will run beside an HBM-bound kernel on another stream (smaller grid; a per-call argument of
    ``npi_linear_bwd_weight_ex``, no process-wide switch is touched).  ``k_valid``: ``a`` is ``[M, Kp]`` with only the
    first ``k_valid`` columns data and the rest ZERO (see ``linear_fwd``); dW then has ``k_valid`` rows.
    ``a_cs`` / ``dc_cs`` (both or none; ``col_scales``): the column scales of the two operands -- the GEMM then runs on two fp16
    pieces per operand (``NPI_GEMM_SPLIT_F16X2``: three matrix products per tile instead of six; ``dw_f16x2_shape``)."""
    dev = require_gpu(a, dc)
    a = _fc(a, "a")
    dc = _fc(dc, "dC", a)
    M, Ka = a.shape
    N = dc.size(1)
    K = Ka if k_valid is None else int(k_valid)
    fl = int(flags or 0)
    if K != Ka:
        if Ka != _pad128(K) or a.dtype != torch.float32:
            raise ValueError(f"a zero-padded a must be f32 and {_pad128(K)} wide (got {Ka})")
        fl |= NPI_GEMM_A_ZERO_PADDED
    if (a_cs is None) != (dc_cs is None):
        raise ValueError("linear_bwd_weight: a_cs and dc_cs come together")
    if a_cs is not None and (a.dtype != torch.float32 or K != Ka or fl & NPI_GEMM_EXACT_F32 or not dw_f16x2_shape(M, K, N)):
        a_cs = dc_cs = None                                     # (storage / shape / flags the fp16 x 2 kernel does not serve)
    if a_cs is not None:
        for v, n, what in ((a_cs, K, "a_cs"), (dc_cs, N, "dc_cs")):
            if v.dtype != torch.float32 or v.numel() != n or not v.is_contiguous() or v.device != a.device:
                raise ValueError(f"linear_bwd_weight: {what} must be a contiguous float32 vector with {n} entries on the operands' device")
        fl |= NPI_GEMM_SPLIT_F16X2
    lib = load()
    n_ws = int(lib.npi_linear_bwd_weight_workspace_elems(M, Ka, N))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    dw = torch.empty((K, N), dtype=a.dtype, device=dev)
    db = torch.empty(N, dtype=a.dtype, device=dev) if want_bias else None
    with _gemm_events("bwd_weight", 2.0 * M * K * N, dev):
        check(lib.npi_linear_bwd_weight_ex(ptr(a), a.stride(0), ptr(dc), dc.stride(0), ptr(dw), dw.stride(0), ptr(db),
                                           M, K, N, ptr(ws), n_ws, _code(a), fl,
                                           1 if shared else 0, ptr(a_cs), ptr(dc_cs), stream_ptr(dev)),
              "npi_linear_bwd_weight")
    return dw, db


def _layer_calls_ok() -> bool:
    """the one-call-per-layer entry points (npi_conv_fwd / npi_conv_bwd) issue the same launches as the per-op calls; the per-op
    calls are kept while bench.py's per-launch event hooks are on (the hooks sit around the single launches)"""
    return _PROFILE is None and _PROFILE_GEMM is None and _PROFILE_TAGS is None


def conv_fwd(side: CSRSide, x: torch.Tensor, w_entry: Optional[torch.Tensor], mean: bool, weight: torch.Tensor,
             bias: Optional[torch.Tensor], relu: bool, want_bwd_copy: bool):
    """aggregate-then-project as ONE call (``npi_conv_fwd``): ``(agg, out, ws_bwd or None)``.  ``agg`` is ``[N, Ka]`` with Ka = the
    weight's row count, or that rounded up to 128 with zero pad columns (``padded_aggregate_buffer``).  The same launches as
    ``segsum`` + ``prepare_weight`` + ``linear_fwd``."""
    dev = require_gpu(x, weight, bias, w_entry)
    x = _fcp(x, "x")
    weight = _fc(weight, "weight", x)
    if bias is not None:
        bias = _fc(bias, "bias", x)
    N, F = side.n_rows, x.size(1)
    K, Nout = weight.shape
    if side.n_cols > x.size(0):
        raise ValueError(f"the table has {x.size(0)} rows, the adjacency indexes {side.n_cols}")
    agg = padded_aggregate_buffer(x, K, N)
    if agg is None:
        agg = torch.empty((N, F), dtype=x.dtype, device=dev)
    Ka = agg.size(1)
    if Ka != K and (x.dtype != torch.float32 or Ka != _pad128(K) or F not in (K, Ka)):
        # (F == Ka: x is itself the zero-padded base of the caller's features, sage_conv(pad_base=))
        raise ValueError(f"x has {F} columns, weight {K} rows (a zero-padded x / aggregate must be f32 and {_pad128(K)} wide)")
    lib = load()
    flags = NPI_GEMM_A_ZERO_PADDED if Ka != K else 0
    can_prepare = (Ka == K and K % 32 == 0 and Nout % 32 == 0 and weight.stride(1) == 1)
    which = (3 if want_bwd_copy else 1) if can_prepare else 0
    one = int(lib.npi_linear_workspace_bytes(Ka, Nout))
    ws = torch.empty(one * (2 if which == 3 else 1), dtype=torch.uint8, device=dev)
    out = torch.empty((N, Nout), dtype=x.dtype, device=dev)
    check(lib.npi_conv_fwd(ptr(side.rowptr), ptr(side.col), ptr(side.item_row), side.item, ptr(w_entry), N, side.nnz_max, ptr(x),
                           x.stride(0), F, 1 if mean else 0, ptr(agg), agg.stride(0), ptr(side.carry(F)), ptr(weight), weight.stride(0),
                           ptr(bias), ptr(out), out.stride(0), K, Nout, 1 if relu else 0, _code(x), flags, which, ptr(ws), ws.numel(),
                           stream_ptr(dev)), "npi_conv_fwd")
    return agg, out, (Planes(ws[one:], False) if which == 3 else None)


def conv_bwd(tside: CSRSide, grad_out: torch.Tensor, out_relu: Optional[torch.Tensor], agg: torch.Tensor, weight: torch.Tensor,
             rowscale: Optional[torch.Tensor], t_w: Optional[torch.Tensor], ws_bwd: Optional[torch.Tensor], want_x: bool,
             want_w: bool, want_bias: bool):
    """the backward of ``conv_fwd`` as ONE call (``npi_conv_bwd``): ``(dx, dw, db)``.  The same launches as ``relu_backward`` +
    ``linear_bwd_weight`` + ``linear_bwd_data`` + ``segsum`` over the transposed side, on one stream."""
    dev = require_gpu(grad_out, agg, weight, rowscale, t_w)
    lib = load()
    N, Nout = grad_out.shape
    K = weight.size(0)
    Ka = agg.size(1)
    flags = NPI_GEMM_A_ZERO_PADDED if Ka != K else 0
    dz = torch.empty((N, Nout), dtype=torch.float32, device=dev) if out_relu is not None else None
    dw = db = dws = dagg = dx = None
    n_ws = 0
    if want_w:
        n_ws = int(lib.npi_linear_bwd_weight_workspace_elems(N, Ka, Nout))
        dws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        dw = torch.empty((K, Nout), dtype=agg.dtype, device=dev)
        db = torch.empty(Nout, dtype=agg.dtype, device=dev) if want_bias else None
    prepared = ws_bwd is not None
    ws_bwd = _planes_for(ws_bwd, False, "conv_bwd") if prepared else None
    if want_x:
        dagg = torch.empty((N, K), dtype=grad_out.dtype, device=dev)
        dx = torch.empty((N, K), dtype=grad_out.dtype, device=dev)
        if ws_bwd is None:
            ws_bwd = _gemm_workspace(K, Nout, dev)
    check(lib.npi_conv_bwd(ptr(grad_out), grad_out.stride(0), ptr(out_relu), out_relu.stride(0) if out_relu is not None else 0, ptr(dz),
                           Nout, N, K, Nout, _code(grad_out), flags, ptr(agg), agg.stride(0), ptr(dw), Nout, ptr(db), ptr(dws), n_ws,
                           ptr(weight), weight.stride(0), ptr(rowscale), ptr(dagg), K, ptr(ws_bwd),
                           ws_bwd.numel() if ws_bwd is not None else 0, 1 if prepared else 0, ptr(tside.rowptr), ptr(tside.col),
                           ptr(tside.item_row), tside.item, ptr(t_w), tside.nnz_max, ptr(dx), K,
                           ptr(tside.carry(K)) if want_x else 0, stream_ptr(dev)), "npi_conv_bwd")
    return dx, dw, db



class _L2NormalizeFn(torch.autograd.Function):
    """``F.normalize(x, p=2, dim=-1)`` for f32 rows (``npi_l2_normalize_rows`` / ``_bwd``)"""

    @staticmethod
    def forward(ctx, x, eps: float):
        dev = require_gpu(x)
        x = _f32c(x, "x")
        M, F = x.shape
        y = torch.empty((M, F), dtype=torch.float32, device=dev)
        nrm = torch.empty(M, dtype=torch.float32, device=dev)
        check(load().npi_l2_normalize_rows(ptr(x), x.stride(0), M, F, float(eps), ptr(y), y.stride(0), ptr(nrm), stream_ptr(dev)),
              "npi_l2_normalize_rows")
        ctx.eps = float(eps)
        ctx.save_for_backward(y, nrm)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, nrm = ctx.saved_tensors
        dev = y.device
        dy = _f32c(dy, "grad_out")
        M, F = y.shape
        dx = torch.empty((M, F), dtype=torch.float32, device=dev)
        check(load().npi_l2_normalize_rows_bwd(ptr(dy), dy.stride(0), ptr(y), y.stride(0), ptr(nrm), M, F, ctx.eps, ptr(dx),
                                               dx.stride(0), stream_ptr(dev)), "npi_l2_normalize_rows_bwd")
        return dx, None


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """``torch.nn.functional.normalize(x, p=2.0, dim=-1)`` (what ``SAGEConv(normalize=True)`` ends with); f32 2-D through the
    package's own kernels, other storage types through the torch op"""
    if x.dtype != torch.float32 or x.dim() != 2:
        return torch.nn.functional.normalize(x, p=2.0, dim=-1, eps=eps)
    return _L2NormalizeFn.apply(x, eps)


def relu_backward(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dz = dy where y > 0 else 0 (``y``: the output of a fused ReLU); f32 through ``npi_relu_backward``, other storage types
    through the equivalent torch op"""
    if dy.dtype != torch.float32 or y.dtype != torch.float32 or dy.dim() != 2:
        return torch.ops.aten.threshold_backward(dy, y, 0)
    dev = require_gpu(dy, y)
    if dy.stride(1) != 1:
        dy = dy.contiguous()
    if y.stride(1) != 1:
        y = y.contiguous()
    M, F = dy.shape
    dz = torch.empty((M, F), dtype=torch.float32, device=dev)
    check(load().npi_relu_backward(ptr(dy), dy.stride(0), ptr(y), y.stride(0), M, F, ptr(dz), dz.stride(0), stream_ptr(dev)),
          "npi_relu_backward")
    return dz


def colsum(x: torch.Tensor) -> torch.Tensor:
    dev = require_gpu(x)
    x = _f32c(x, "x")
    M, N = x.shape
    n_ws = int(load().npi_colsum_workspace_elems(M, N))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    check(load().npi_colsum(ptr(x), x.stride(0), M, N, ptr(out), ptr(ws), n_ws, stream_ptr(dev)), "npi_colsum")
    return out


def entry_weights(graph: CSRGraph, edge_weight: Optional[torch.Tensor], fill: float = 1.0):
    """``edge_weight [E]`` in the entry order of both orientations, self loops included
    (``add_remaining_self_loops(edge_index, edge_weight, fill, N)``: an existing self loop's weight becomes that
    node's loop weight, every other node's loop weighs ``fill``).  Returns ``[by_dst, by_src]``."""
    lib = load()
    dev = graph.device
    N = graph.num_nodes
    s = stream_ptr(dev)
    loop_w = None
    if edge_weight is not None:
        require_gpu(edge_weight)
        edge_weight = _f32c(edge_weight.detach(), "edge_weight").view(-1)       # ([E, 1], as PyG's `edge_weight.view(-1, 1)` takes it)
        if edge_weight.numel() != graph.num_edges:
            raise ValueError(f"edge_weight has {edge_weight.numel()} entries, edge_index {graph.num_edges} columns")
    src, dst = graph._src, graph._dst
    m = (src == dst) & (src >= 0)                        # (-1, -1) columns are padding (npi_filter_adj), not self loops
    if bool(m.any()):
        loop_w = torch.full((N,), fill, dtype=torch.float32, device=dev)
        loop_w[src[m]] = edge_weight[m] if edge_weight is not None else 1.0
    out = []
    for side in (graph.by_dst, graph.by_src):
        we = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev)
        check(lib.npi_entry_weights(ptr(side.eid), ptr(side.rowidx), ptr(side.rowptr), ptr(edge_weight),
                                    ptr(loop_w), fill, N, side.nnz_max, ptr(we), s), "npi_entry_weights")
        out.append(we)
    return out


def mean_bwd_weights(graph: CSRGraph, tside: CSRSide, w_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-entry weights of the TRANSPOSED aggregation of a mean layer when it runs on dOut itself: ``scatter_mean``'s divisor
    belongs to the target, i.e. to the GATHERED row of the by-source side -- ``w[p] = inv_count[col[p]]`` (times the entry's edge
    weight, ``w_src``).  ``npi_entry_col_scale``; without edge weights computed once per graph and side (kept on the graph)."""
    cache = graph.__dict__.setdefault("_mean_t_w", {})
    key = id(tside)
    if w_src is None and key in cache:
        return cache[key]
    dev = graph.device
    inv = graph.inv_count(graph.by_dst)
    out = torch.empty(max(tside.nnz_max, 1), dtype=torch.float32, device=dev)
    check(load().npi_entry_col_scale(ptr(tside.col), ptr(tside.rowptr), ptr(inv), ptr(w_src), tside.n_rows, inv.numel(), tside.nnz_max,
                                     ptr(out), stream_ptr(dev)), "npi_entry_col_scale")
    if w_src is None:
        cache[key] = out
    return out


def _aggregate_first_ok(sch: Schedule, f16: bool, weight: torch.Tensor, grad_out: torch.Tensor, tside: CSRSide, ws_bwd) -> bool:
    """can the backward of an aggregate-then-project layer run as ``dX = (A^T dOut) W^T`` with the GEMM on fp16 x 2 -- the
    transposed aggregation on dOut itself, writing the row scales of its output (``_backward_aggregate_first``)?"""
    # (both row counts: dW's contraction runs over the TARGET rows, the data GEMM over the source rows -- one number on a square graph)
    return (sch.aggregate_first_backward and f16 and isinstance(ws_bwd, Planes) and ws_bwd.f16 and grad_out.dtype == torch.float32 and grad_out.size(1) == 256
            and segsum_scales_ok(tside, grad_out) and f16x2_shape(min(grad_out.size(0), tside.n_rows), grad_out.size(1), weight.size(0)))


def _dw_beside(agg, grad_out, has_bias: bool, k_valid, flags: int, aggregate, read_beside):
    """The two-stream fork of an aggregate-then-project backward: ``dW = agg^T dOut`` (+ db) on the launch stream, ``aggregate()``
    -- the transposed aggregation -- on the side stream.  Returns ``(aggregate(), dw, db)``.

    dW is independent of the dX chain.  It is launched on THIS stream right behind whatever produced the aggregation's input, one
    workgroup per CU (``shared=True``), so that it is resident everywhere before the aggregation -- sent to a second HIP stream --
    fills the remaining wave slots; the two then share every CU.  (The other way round the aggregation wins the race, takes every
    register of every SIMD, and dW only starts when it is over.)  ``read_beside``: the tensors allocated on the launch stream that
    the aggregation reads or writes."""
    dev = grad_out.device
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    side.wait_stream(main)                                       # the aggregation's input is complete for the side stream
    dw, db = linear_bwd_weight(agg, grad_out, want_bias=has_bias, shared=True, k_valid=k_valid, flags=flags)
    with torch.cuda.stream(side):
        out = aggregate()
    for buf in read_beside:
        buf.record_stream(side)                                  # allocated on main, used on side
    out.record_stream(main)                                      # consumed on main (a no-op where main allocated it)
    main.wait_stream(side)
    return out, dw, db


def _backward_aggregate_first(graph, tside: CSRSide, w_t: Optional[torch.Tensor], agg, weight, grad_out, ws_bwd: "Planes", want_w: bool,
                              has_bias: bool, overlap: bool, k_valid=None, hub: Optional[HubPlan] = None):
    """``dX = (A_w^T dOut) W^T`` instead of ``A_w^T (dOut W^T)`` -- the same number up to fp32 rounding (the aggregation is linear;
    GCNConv's forward uses the same freedom).  What it buys on large graphs: the transposed aggregation now WRITES
    the left operand of the backward's data GEMM, so it writes that operand's row scales too (``segsum(scales_out=)``) and the
    GEMM runs on two fp16 pieces per operand -- three matrix products instead of six -- with no pass over dOut for its scales
    (which arrive from outside the layer).  dW = agg^T dOut needs neither and goes first on the launch stream, so that it is
    resident on every CU before the aggregation -- on the side stream -- fills the remaining wave slots (as before).
    ``w_t``: per-entry weights of the transposed side (``mean_bwd_weights`` / the GCN norm).  ``hub``: ``tside``'s plan -- then
    ``w_t`` belongs to ``hub.light`` and the hub rows take the mean's divisors as a column scale.  Returns ``(dx, dw, db)``."""
    dev = grad_out.device
    cs = graph.inv_count(graph.by_dst) if hub is not None else None
    N, Nout = tside.n_rows, grad_out.size(1)                     # (rows of dX: the SOURCE id space -- grad_out's own on a square graph)
    t = torch.empty((N, Nout), dtype=torch.float32, device=dev)
    t_scales = torch.empty(N, dtype=torch.float32, device=dev)
    dw = db = None

    def aggregate():
        return segsum(graph, tside, grad_out, w=w_t, mean=False, out=t, scales_out=t_scales, hub=hub, col_scale=cs)

    if overlap and want_w:
        _, dw, db = _dw_beside(agg, grad_out, has_bias, k_valid, 0, aggregate, (grad_out, t, t_scales))
    else:
        if want_w:
            dw, db = linear_bwd_weight(agg, grad_out, want_bias=has_bias, k_valid=k_valid)
        aggregate()
    dx = linear_bwd_data(t, weight, ws=ws_bwd, dc_scales=t_scales)
    return dx, dw, db


# ---------------------------------------------------------------------------------------------
# d edge_weight of SAGEConv / GCNConv
# ---------------------------------------------------------------------------------------------
def edge_dot(side: CSRSide, a: torch.Tensor, b: torch.Tensor, n_edges: int, row_scale: Optional[torch.Tensor] = None,
             mul: Optional[torch.Tensor] = None, want_entry: bool = False, d_edge: Optional[torch.Tensor] = None,
             d_loop: Optional[torch.Tensor] = None):
    """``g[p] = row_scale[i] * <a[i, :], b[col[p], :]>`` for every entry ``p`` of ``side`` (``i`` its row; ``npi_edge_dot``): the
    gradient w.r.t. the per-entry weight of ``segsum(side, b, w=...)`` when ``a`` is the gradient of its output.  ``a`` / ``b``
    f32, rows may have a pitch.  ``d_edge [n_edges]`` / ``d_loop [n_rows]``: written through ``side.eid`` (an edge's element by its
    one entry, a node's by its implicit self loop; other elements are left as they are).  ``want_entry``: also ``g`` in entry
    order, and with ``mul [nnz_max]`` the products ``g * mul`` -- returns ``(g_entry, gm_entry)``, None where not asked for."""
    dev = require_gpu(a, b, row_scale, mul, d_edge, d_loop)
    for t, name in ((a, "a"), (b, "b")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.size(1):
            raise ValueError(f"edge_dot: {name} must be float32 [rows, F] with unit column stride")
    F = a.size(1)
    if b.size(1) != F or a.size(0) < side.n_rows or b.size(0) < side.n_cols:
        raise ValueError(f"edge_dot: a {tuple(a.shape)} / b {tuple(b.shape)} do not fit a side of {side.n_rows} rows over {side.n_cols}")
    for t, n, name in ((row_scale, side.n_rows, "row_scale"), (mul, side.nnz_max, "mul"), (d_edge, n_edges, "d_edge"),
                       (d_loop, side.n_rows, "d_loop")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n):
            raise ValueError(f"edge_dot: {name} must be a contiguous float32 vector of at least {n} elements")
    g = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev) if want_entry else None
    gm = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev) if (want_entry and mul is not None) else None
    if g is None and (d_edge is None or d_edge.numel() == 0) and d_loop is None:
        return None, None                                           # (no edges and nothing else asked for)
    check(load().npi_edge_dot(ptr(side.rowptr), ptr(side.col), ptr(side.rowidx), ptr(side.eid), side.n_rows, side.n_cols, side.nnz_max,
                              n_edges, ptr(a), a.stride(0), ptr(b), b.stride(0), F, ptr(row_scale), ptr(mul) if gm is not None else 0,
                              ptr(g), ptr(gm), ptr(d_edge), ptr(d_loop), stream_ptr(dev)), "npi_edge_dot")
    return g, gm


def _loop_edges(graph: CSRGraph) -> torch.Tensor:
    """positions of the existing self-loop columns ``(k, k)`` of the edge list (padding ``(-1, -1)`` is none), kept on the graph"""
    idx = graph.__dict__.get("_loop_edge_idx")
    if idx is None:
        idx = ((graph._src == graph._dst) & (graph._src >= 0)).nonzero().view(-1)
        graph._loop_edge_idx = idx
    return idx


class _EdgeWeightGradFn(torch.autograd.Function):
    """Makes ``edge_weight`` a differentiable input of a SAGEConv / GCNConv call: the identity on the layer's output, whose
    backward hands ``dOut`` on unchanged -- so dX, dW and db come from the layer's own backward, launch for launch as without a
    weight gradient -- and computes ``d edge_weight`` beside it (``sage_conv`` / ``gcn_conv`` have the closed forms):

      * aggregate-first layers (SAGEConv, GCNConv with F_in <= F_out): ``dAgg = dOut W^T`` (one GEMM of its own: the layer's
        backward forms ``dAgg`` only in one of its two orders, and never when fp16 x 2 applies), dotted per by-target entry
        against the gathered rows of ``x`` -- the one tensor saved in addition (the layer itself keeps ``agg``, not ``x``);
      * project-first GCNConv (F_in > F_out): ``xW`` is recomputed (one GEMM) and dotted against ``dOut`` at the narrower width
        F_out, instead of keeping ``xW`` alive through the step or gathering at F_in;
      * GCNConv(normalize=True): the chain through ``deg^-1/2`` (two ``npi_seg_rowsum_ex`` over ``g norm``, ``npi_gcn_norm_bwd``).

    Existing self-loop edges take the gradient of their node's loop entry (a few lines of indexing, per such edge)."""

    @staticmethod
    def forward(ctx, out, edge_weight, x, weight, graph: CSRGraph, kind: str, relu: bool, norm):
        ctx.graph, ctx.kind, ctx.relu, ctx.norm = graph, kind, relu, norm
        ctx.w_shape = edge_weight.shape
        ctx.save_for_backward(x, weight, *([out] if relu else []))
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[1]:
            return grad_out, None, None, None, None, None, None, None
        x, weight = ctx.saved_tensors[:2]
        graph: CSRGraph = ctx.graph
        side = graph.by_dst
        dev = grad_out.device
        N, E = side.n_rows, graph.num_edges
        go = _f32c(grad_out, "grad_out")
        if ctx.relu:
            go = relu_backward(go, ctx.saved_tensors[2])
        x = x.detach()                                              # (may be a column block of a wider buffer: the dot takes a pitch)
        if x.stride(1) != 1:
            x = x.contiguous()
        weight = weight.detach()
        if ctx.kind == "gcn" and weight.size(0) > weight.size(1):
            a, b = go, linear_fwd(x, weight)                         # <dOut_i, (xW)_j> at width F_out
        else:
            a, b = linear_bwd_data(go, weight), x                    # <dAgg_i, x_j> at width F_in
            if ctx.kind == "concat":
                a = a[:, x.size(1):]                                 # the aggregate's half of [x | mean] (a row pitch of 2 F)
        d_edge = torch.zeros(E, dtype=torch.float32, device=dev)     # padding columns and dropped edges: 0
        d_loop = torch.zeros(N, dtype=torch.float32, device=dev) if graph.self_loops else None
        gcn_norm = ctx.kind == "gcn" and isinstance(ctx.norm, GCNNorm)
        if not gcn_norm:
            # SAGEConv: the mean's divisor belongs to the row; GCNConv(normalize=False): norm IS the weight
            edge_dot(side, a, b, E, row_scale=graph.inv_count(side) if ctx.kind != "gcn" else None, d_edge=d_edge, d_loop=d_loop)
        else:
            nrm: GCNNorm = ctx.norm
            g, gm = edge_dot(side, a, b, E, mul=nrm.by_dst, want_entry=True)
            s_dst = seg_rowsum(side, gm, 1)                                                  # entries whose TARGET is k
            s_src = seg_rowsum(graph.by_src, gm, 1, map_=_transpose_map(graph))              # entries whose SOURCE is k
            check(load().npi_gcn_norm_bwd(ptr(side.rowptr), ptr(side.col), ptr(side.rowidx), ptr(side.eid), N, side.nnz_max, E, ptr(g),
                                          ptr(nrm.deg), ptr(s_dst), ptr(s_src), ptr(d_edge), ptr(d_loop), stream_ptr(dev)),
                  "npi_gcn_norm_bwd")
        if graph.self_loops and E > 0:
            le = _loop_edges(graph)
            if le.numel():
                d_edge[le] = d_loop[graph._src[le]]
        return grad_out, d_edge.view(ctx.w_shape), None, None, None, None, None, None


def _with_edge_weight_grad(out, edge_weight, x, weight, graph: CSRGraph, kind: str, relu: bool = False, norm=None):
    if edge_weight is None or not edge_weight.requires_grad or not torch.is_grad_enabled():
        return out
    return _EdgeWeightGradFn.apply(out, edge_weight, x, weight, graph, kind, relu, norm)


def _check_edge_weight_grad(edge_weight, x, weight) -> bool:
    """does this call want ``d edge_weight``?  f32 only: other storage types keep refusing (never silently detached)"""
    if edge_weight is None or not edge_weight.requires_grad or not torch.is_grad_enabled():
        return False
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or edge_weight.dtype != torch.float32:
        raise NotImplementedError("gradients w.r.t. edge_weight are implemented for float32 features and weights only")
    return True


# ---------------------------------------------------------------------------------------------
# SAGEConv
# ---------------------------------------------------------------------------------------------
class _AggProjectFn(torch.autograd.Function):
    """Aggregate, then project: ``out = act(agg @ W + b)`` with ``agg[i] = scale_i sum_{p in row i} w_dst[p] x[col[p]]`` over
    ``graph.by_dst`` -- a ``CSRGraph`` or, on two id spaces, a ``BipartiteGraph``.  The one schedule of SAGEConv (``mean``; per-entry
    weights from ``edge_weight`` or none), of GCNConv evaluated as ``(A_hat x) W + b`` (``gcn_conv``: no mean, the weights are the
    norm) and of the pair form of SAGEConv.  The aggregate is saved, so in the backward dW = agg^T dOut does not wait for the
    transposed aggregation: on graphs large enough it runs beside it (``_dw_beside``).

    ``w_dst`` / ``w_src``: the per-entry weights of the two orientations, or None.  ``layer_dtypes``: the storage types for which
    the layer has the whole-layer entry points (``conv_fwd`` / ``conv_bwd``, one id space only) and the zero-padded aggregate
    (``padded_aggregate_buffer``): f32 and bf16 for SAGEConv, f32 for GCNConv, none for the pair form.  The unweighted mean
    alone takes the hub plans (``hub_plan_for``) and, on a symmetric edge list, the by-target side for the transposed aggregation."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph, w_dst, w_src, mean: bool, relu: bool, sch: Schedule, layer_dtypes: tuple):
        d = graph.by_dst
        ctx.graph, ctx.w_src, ctx.mean, ctx.relu, ctx.sch, ctx.layer_dtypes = graph, w_src, mean, relu, sch, layer_dtypes
        ctx.has_bias = bias is not None
        ctx.k_rows = None
        hubs = mean and w_dst is None
        fl = _gflags(sch)                                       # (exact-f32 MFMA kernels on request: the per-op calls carry the flag)
        ctx.f16 = (x.dtype == weight.dtype and x.size(1) == weight.size(0)
                   and _f16x2(sch, d.n_rows, weight.size(0), weight.size(1), x.dtype) and segsum_scales_ok(d, x))
        if ctx.f16:
            # large graphs, 256 features: the projection on two fp16 pieces per operand -- the aggregation writes the row scales of
            # agg itself (a wave maximum per finished row); where it cannot, a pass over agg would cost what the GEMM saves
            agg = torch.empty((d.n_rows, x.size(1)), dtype=x.dtype, device=x.device)
            scales = torch.empty(agg.size(0), dtype=torch.float32, device=x.device)
            # (unweighted mean: the heaviest rows by streaming x once, the rest by the plain launch -- CSRGraph.hub_stream)
            hub = hub_plan_for(graph, d, x, agg) if hubs else None
            segsum(graph, d, x, w=w_dst, mean=mean, out=agg, scales_out=scales, hub=hub)
            # both fp16 x 2 copies of W in one call: the backward runs aggregate-first (_backward_aggregate_first), so its data GEMM
            # takes the row scales the transposed aggregation writes -- no pass over dOut, which arrives from outside the layer
            wsf, ctx.ws_bwd = prepare_weight(weight, backward=ctx.needs_input_grad[0], f16=True)
            out = linear_fwd(agg, weight, bias, relu=relu, ws=wsf, a_scales=scales)
        elif not fl and _layer_calls_ok() and x.dtype == weight.dtype and x.dtype in layer_dtypes and not (
                x.dtype == torch.bfloat16 and weight.size(0) % 128 != 0 and 2 * _pad128(weight.size(0)) <= 3 * weight.size(0)):
            # the whole layer call as one entry point (the same launches; one trip through the C ABI instead of three)
            agg, out, ctx.ws_bwd = conv_fwd(d, x, w_dst, mean, weight, bias, relu, ctx.needs_input_grad[0])
        else:
            # a2-a4: gather + scatter_mean (w_dst: PyG's `edge_weight.view(-1, 1) * x_j`; the mean still divides by the count)
            # x may be the zero-padded base of the caller's features (sage_conv): agg then keeps the padded width -- zero
            # columns stay zero under a weighted mean -- and both GEMMs run on it (linear_fwd / linear_bwd_weight)
            agg = padded_aggregate_buffer(x, weight.size(0), d.n_rows, bf16_ok=torch.bfloat16 in layer_dtypes) if (
                not fl and x.dtype in layer_dtypes) else None
            if agg is None:
                agg = segsum(graph, d, x, w=w_dst, mean=mean, hub=hub_plan_for(graph, d, x) if hubs else None)
            else:
                segsum(graph, d, x, w=w_dst, mean=mean, out=agg[:, : x.size(1)])
            if agg.size(1) != weight.size(0) and agg.dtype == torch.bfloat16:
                # bf16 storage, zero-padded aggregate: W gets zero ROWS to match (one small launch) and all three GEMMs of the layer
                # run the aligned bf16 matrix-core kernels; dAgg and dW are computed padded and cut back to the true width
                ctx.k_rows = weight.size(0)
                weight = torch.nn.functional.pad(weight.detach(), (0, 0, 0, agg.size(1) - weight.size(0)))
            # both re-laid copies of W (for this GEMM and for dAgg = dOut W^T of the backward) in one launch
            wsf, ctx.ws_bwd = prepare_weight(weight, backward=ctx.needs_input_grad[0]) if (
                agg.size(1) == weight.size(0) and agg.dtype == weight.dtype and not fl) else (None, None)
            out = linear_fwd(agg, weight, bias, relu=relu, ws=wsf, flags=fl)  # a5: agg @ W + b (ReLU in the epilogue on request)
        ctx.k_valid = weight.size(0) if agg.size(1) != weight.size(0) else None       # (an f32 aggregate wider than W: pad columns)
        ctx.save_for_backward(agg, weight, *([out] if relu else []))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        agg, weight = ctx.saved_tensors[:2]
        graph, w_src, mean, sch = ctx.graph, ctx.w_src, ctx.mean, ctx.sch
        none = (None,) * 7                                      # (graph, w_dst, w_src, mean, relu, sch, layer_dtypes)
        grad_out = _fc(grad_out, "grad_out", agg)
        want_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        want_x = ctx.needs_input_grad[0]
        hubs = mean and w_src is None
        ts = None
        if want_x:
            # symmetric edge list, unweighted mean: A^T has the rows of A (graph.CSRGraph.symmetric) -- skip the second sort
            ts = graph.by_dst if (hubs and graph.symmetric) else graph.by_src
        overlap = want_w and want_x and _overlaps(sch, grad_out.size(0))
        fl = _gflags(sch)
        if (not fl and not overlap and ctx.k_rows is None and _layer_calls_ok() and (want_w or want_x) and not ctx.f16
                and grad_out.dtype in ctx.layer_dtypes):
            # one stream: the whole backward as one entry point (ReLU mask, dW + db, dAgg GEMM, transposed aggregation)
            out_relu = None
            if ctx.relu:
                if grad_out.dtype == torch.float32:
                    out_relu = ctx.saved_tensors[2]
                else:
                    grad_out = relu_backward(grad_out, ctx.saved_tensors[2])
            return conv_bwd(ts if want_x else graph.by_dst, grad_out, out_relu, agg, weight,
                            graph.inv_count(graph.by_dst) if mean else None, w_src, ctx.ws_bwd, want_x, want_w, ctx.has_bias) + none
        if ctx.relu:                                            # threshold_backward, as F.relu's autograd does it
            grad_out = relu_backward(grad_out, ctx.saved_tensors[2])
        if want_x and _aggregate_first_ok(sch, ctx.f16, weight, grad_out, ts, ctx.ws_bwd):
            # unweighted mean: the weights are inv_count[col], a factor of the GATHERED row -- the streaming path's column scale;
            # the plain launch over the light side takes the same factors per entry (cached per graph and side)
            hub = hub_plan_for(graph, ts, grad_out) if hubs else None
            w_t = mean_bwd_weights(graph, ts if hub is None else hub.light, w_src) if mean else w_src
            return _backward_aggregate_first(graph, ts, w_t, agg, weight, grad_out, ctx.ws_bwd, want_w, ctx.has_bias, overlap,
                                             ctx.k_valid, hub=hub) + none
        ws_bwd = ctx.ws_bwd if not (isinstance(ctx.ws_bwd, Planes) and ctx.ws_bwd.f16) else None     # (fp16 x 2 planes: not for this order)
        dx = dw = db = None
        if want_w and not overlap:
            dw, db = linear_bwd_weight(agg, grad_out, want_bias=ctx.has_bias, k_valid=ctx.k_valid, flags=fl)   # aggT dOut, colsum
        if want_x:
            # dAgg = dOut W^T, under a mean pre-divided by the in-count of its row (fused epilogue), then
            # dX[j] = sum over the entries whose SOURCE is j  ==  segsum over the by-source CSR
            dagg = linear_bwd_data(grad_out, weight, rowscale=graph.inv_count(graph.by_dst) if mean else None, ws=ws_bwd, flags=fl)
            if ctx.k_rows is not None:
                dagg = dagg[:, : ctx.k_rows]                                 # (the pad columns of dAgg: dOut times zero rows)

            def aggregate():
                return segsum(graph, ts, dagg, w=w_src, mean=False, hub=hub_plan_for(graph, ts, dagg) if hubs else None)

            if overlap:
                dx, dw, db = _dw_beside(agg, grad_out, ctx.has_bias, ctx.k_valid, fl, aggregate, (dagg,))
            else:
                dx = aggregate()
        if dw is not None and ctx.k_rows is not None:
            dw = dw[: ctx.k_rows]                                             # the gradient of the zero rows is not W's
        return (dx, dw, db) + none


class _SageConcatFn(torch.autograd.Function):
    """``SAGEConv(concat=True)`` (PyG 1.4.2): ``out = [x | mean_{j -> i} x_j] @ W[2F, Fo] + b`` over the edge list AS IT IS (no
    self loop appended).  The mean is written straight into the right half of the ``[N, 2F]`` operand of ONE projection GEMM
    (K = 2F); the backward splits ``dOut W^T`` into its two halves: the left one is x's own share, the right one -- divided by
    the in-count -- goes through the transposed aggregation."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph: CSRGraph, w_entry=None):
        N, F = x.shape
        cat = torch.empty((N, 2 * F), dtype=x.dtype, device=x.device)
        cat[:, :F].copy_(x)
        segsum(graph, graph.by_dst, x, w=w_entry[0] if w_entry else None, mean=True, out=cat[:, F:])
        out = linear_fwd(cat, weight, bias)
        ctx.graph, ctx.F = graph, F
        ctx.w_src = w_entry[1] if w_entry else None
        ctx.has_bias = bias is not None
        ctx.save_for_backward(cat, weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cat, weight = ctx.saved_tensors
        graph: CSRGraph = ctx.graph
        F = ctx.F
        grad_out = _fc(grad_out, "grad_out", cat)
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = linear_bwd_weight(cat, grad_out, want_bias=ctx.has_bias)
        if ctx.needs_input_grad[0]:
            dcat = linear_bwd_data(grad_out, weight)                              # [N, 2F]
            dagg = dcat[:, F:] * graph.inv_count(graph.by_dst).view(-1, 1).to(dcat.dtype)     # scatter_mean's divisor, per TARGET
            dx = segsum(graph, graph.by_src, dagg.contiguous(), w=ctx.w_src, mean=False)
            dx += dcat[:, :F]
        return dx, dw, db, None, None


def sage_conv(x: torch.Tensor, edge_index, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
              normalize: bool = False, edge_weight: Optional[torch.Tensor] = None, relu: bool = False,
              pad_base: Optional[torch.Tensor] = None, schedule: Schedule = DEFAULT, concat: bool = False,
              aggr: str = "mean") -> torch.Tensor:
    """PyG 1.4.2 ``SAGEConv(normalize=False, concat=False).forward`` on MI355X
    (call sites: reference ``src/classes.py:62,66,70``).  ``edge_weight [E]`` scales the messages.  ``pad_base``: the wider
    buffer ``x`` is the leading columns of, its other columns zero (``GraphBatch.pad_base``).

    ``edge_weight`` is differentiable (f32 layers; bf16 storage raises ``NotImplementedError``).  With entry ``p`` of the
    by-target CSR = (target ``i``, source ``j``, edge ``eid[p]``) and ``dAgg = dOut W^T`` (``relu`` / ``normalize`` only change
    ``dOut`` first; ``concat=True``: the right half of ``dOut W^T``, the edge list as it is)::

        g_p = inv_count[i] * <dAgg[i, :], x[j, :]>          d edge_weight[eid[p]] = g_p

    (``_EdgeWeightGradFn``, ``npi_edge_dot``).  As under ``add_remaining_self_loops``, an existing self-loop edge ``(k, k)``
    receives the gradient of node k's loop entry -- if several such edges name the same node, EACH of them receives it (what
    the backward of autograd's ``index_put`` does) -- the loop entries of the other nodes carry the constant 1, and padding
    columns ``(-1, -1)`` and dropped edges get 0.  The gradient has ``edge_weight``'s shape and dtype.

    ``aggr="max"``: the maximum over the same entries instead of their mean (``segmax``, Rule X; float32, no ``edge_weight``;
    ``schedule`` only names the GEMM flags) -- ``_SageMaxFn``."""
    if aggr != "mean":
        _check_aggr(aggr, "sage_conv")
        return _sage_conv_max(x, edge_index, weight, bias, normalize, edge_weight, relu, schedule, concat)
    require_gpu(x, weight, bias)
    w_grad = _check_edge_weight_grad(edge_weight, x, weight)
    x_in = x
    if concat:
        # PyG 1.4.2: ``concat=True`` skips add_remaining_self_loops -- the edge list as it is, weight [2 F_in, F_out]
        if isinstance(edge_index, CSRGraph):
            graph = edge_index
            if graph.self_loops or not graph.keep_equal:
                raise ValueError("sage_conv(concat=True) aggregates over the edge list as it is: build the graph with "
                                 "CSRGraph(edge_index, N, self_loops=False, keep_equal=True)")
            if graph.num_nodes != x.size(0):
                raise ValueError(f"CSRGraph was built for {graph.num_nodes} nodes, x has {x.size(0)}")
        else:
            ei = edge_index.edge_index if hasattr(edge_index, "edge_index") else edge_index      # a GraphBatch or the [2, E] tensor
            graph = CSRGraph(ei, x.size(0), self_loops=False, keep_equal=True)
        if weight.size(0) != 2 * x.size(1):
            raise ValueError(f"sage_conv(concat=True): weight must have {2 * x.size(1)} rows (got {weight.size(0)})")
        w_entry = entry_weights(graph, edge_weight, 1.0) if edge_weight is not None else None
        out = _SageConcatFn.apply(x, weight, bias, graph, w_entry)
        if w_grad:
            out = _with_edge_weight_grad(out, edge_weight, x_in, weight, graph, "concat")
        if relu:
            out = torch.relu(out)
        return l2_normalize(out) if normalize else out
    graph = as_graph(edge_index, x.size(0))
    w_entry = entry_weights(graph, edge_weight, 1.0) if edge_weight is not None else None
    # features that are a view of a wider buffer whose extra columns are zero (InteractionGraph.batch: 178 -> 256): the
    # layer runs on the padded buffer, so that its GEMMs take the matrix-core kernels instead of the guarded ones
    base = pad_base
    if (base is not None and not x.requires_grad and x.dtype == torch.float32 and base.size(0) == x.size(0)
            and base.size(1) == _pad128(x.size(1)) and weight.size(0) == x.size(1) and base.data_ptr() == x.data_ptr()):
        x = base
    if relu and normalize:
        raise ValueError("sage_conv: relu=True applies to the projection's output; normalize=True comes after it in PyG")
    w_dst, w_src = w_entry or (None, None)
    out = _AggProjectFn.apply(x, weight, bias, graph, w_dst, w_src, True, relu, schedule, (torch.float32, torch.bfloat16))
    if w_grad:
        out = _with_edge_weight_grad(out, edge_weight, x_in, weight, graph, "sage", relu)
    if normalize:
        out = l2_normalize(out)
    return out


# ---------------------------------------------------------------------------------------------
# Max aggregation (include/npi_gnn.h: RULE X) and SAGEConv(aggr="max")
# ---------------------------------------------------------------------------------------------
def _check_aggr(aggr, who: str) -> None:
    if aggr not in ("mean", "max"):
        raise ValueError(f"{who}: aggr must be 'mean' or 'max' (got {aggr!r})")


def _f32_rows(t: torch.Tensor, name: str, who: str) -> torch.Tensor:
    """an f32 ``[rows, F]`` operand of the max kernels: unit column stride, any row pitch >= F (anything else is copied)"""
    if t.dtype != torch.float32:
        raise NotImplementedError(f"{who}: {name} is {t.dtype}; max aggregation runs on float32 tables (bf16 storage is not implemented)")
    if t.dim() != 2 or t.size(1) < 1:
        raise ValueError(f"{who}: {name} must be a [rows, F] tensor with F >= 1")
    return t if t.stride(1) == 1 and t.stride(0) >= t.size(1) else t.contiguous()


def _pitch(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))     # (the stride of a single row means nothing)


def _segmax_workspace(side: CSRSide, F: int, dev) -> torch.Tensor:
    """the per-call scratch of ``npi_segmax`` / ``npi_segmax_bwd`` (head / tail partial rows of every item); needs no clearing"""
    return torch.empty(int(load().npi_segmax_workspace_bytes(side.nnz_max, side.item, F)), dtype=torch.uint8, device=dev)


def segmax_side(side: CSRSide, x: torch.Tensor, out: Optional[torch.Tensor] = None):
    """``(out, arg)`` of Rule X over ONE side (``npi_segmax``): ``out[i] = max_{p in row i} x[col[p]]``, ``arg`` the winners' ``eid``
    (int32; -1 the appended loop, -2 a row without entries, whose ``out`` is 0).  ``out``: write the maxima into this ``[n_rows, F]``
    tensor (a column block of a wider buffer is fine).  Not differentiable: ``segmax`` is."""
    dev = require_gpu(x, out)
    x = _f32_rows(x, "x", "segmax")
    N, F = side.n_rows, x.size(1)
    if x.size(0) < side.n_cols:
        raise ValueError(f"segmax: the table has {x.size(0)} rows, the adjacency indexes {side.n_cols}")
    if out is None:
        out = torch.empty((N, F), dtype=torch.float32, device=dev)
    else:
        _check_out(out, N, F, x, "segmax")
    arg = torch.empty((N, F), dtype=torch.int32, device=dev)
    ws = _segmax_workspace(side, F, dev)
    check(load().npi_segmax(ptr(side.rowptr), ptr(side.col), ptr(side.eid), ptr(side.rowidx), side.item, N, side.n_cols, side.nnz_max,
                            ptr(x), _pitch(x), F, ptr(out), _pitch(out), ptr(arg), F, ptr(ws), ws.numel(), stream_ptr(dev)), "npi_segmax")
    return out, arg


def segmax_bwd_side(tside: CSRSide, dout: torch.Tensor, arg: torch.Tensor) -> torch.Tensor:
    """``dX`` of Rule X over the by-SOURCE side (``npi_segmax_bwd``): row j sums ``dout[i, c]`` over its entries ``(j -> i)`` whose
    ``eid`` is ``arg[i, c]`` -- a gather in a fixed order, no float atomics, bitwise reproducible."""
    dev = require_gpu(dout, arg)
    dout = _f32_rows(dout, "grad_out", "segmax")
    F = dout.size(1)
    if arg.dtype != torch.int32 or arg.shape != dout.shape or arg.stride(1) != 1 or arg.stride(0) < F:
        raise ValueError("segmax: arg must be the int32 [rows, F] winners of the forward, the shape of grad_out")
    if dout.size(0) < tside.n_cols:
        raise ValueError(f"segmax: grad_out has {dout.size(0)} rows, the by-source side indexes {tside.n_cols}")
    dx = torch.empty((tside.n_rows, F), dtype=torch.float32, device=dev)
    ws = _segmax_workspace(tside, F, dev)
    check(load().npi_segmax_bwd(ptr(tside.rowptr), ptr(tside.col), ptr(tside.eid), ptr(tside.rowidx), tside.item, tside.n_rows,
                                tside.n_cols, tside.nnz_max, ptr(dout), _pitch(dout), ptr(arg), _pitch(arg), F, ptr(dx), F, ptr(ws),
                                ws.numel(), stream_ptr(dev)), "npi_segmax_bwd")
    return dx


class _SegmaxFn(torch.autograd.Function):
    """``segmax`` over a graph: ``by_dst`` forward, ``by_src`` (built on first use) backward; ``arg`` is kept and not differentiable"""

    @staticmethod
    def forward(ctx, x, graph):
        out, arg = segmax_side(graph.by_dst, x)
        ctx.graph = graph
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        (arg,) = ctx.saved_tensors
        return segmax_bwd_side(ctx.graph.by_src, dout, arg), None


def segmax(graph_or_side, x: torch.Tensor):
    """``(out, arg)``: the max aggregation of PyG's ``MessagePassing(aggr='max')`` under Rule X (``include/npi_gnn.h``) --
    ``out[i, c] = max_{j -> i} x[j, c]`` (a target without an entry: 0), ``arg[i, c]`` the column of ``edge_index`` that won (int32;
    -1: the appended self loop, -2: no entry; ties: the smallest column, the loop last; NaN beats every number).  Both are a pure
    function of ``(x, edge list, self_loops)``: bitwise the same for either item size and for ``sort_columns`` on or off.
    ``graph_or_side``: a ``CSRGraph``, a ``BipartiteGraph`` (``x`` = the source table), a ``GraphBatch``, the ``[2, E]`` tensor
    (sorted here, self loops appended, as the layers do) or one ``CSRSide`` (then nothing is differentiable: a side alone has no
    transposed side).  Differentiable in ``x``: the gradient of ``out[i, c]`` goes to the winner's row, summed over the by-source side
    in a fixed order (no float atomics; bitwise reproducible).  float32 only; ``x`` may keep a row pitch."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("segmax: x must be a [rows, F] tensor")
    if x.dtype != torch.float32:
        raise NotImplementedError(f"segmax: x is {x.dtype}; max aggregation runs on float32 tables (bf16 storage is not implemented)")
    require_gpu(x)
    g = graph_or_side
    if isinstance(g, CSRSide):
        if x.requires_grad and torch.is_grad_enabled():
            raise ValueError("segmax: a CSRSide alone has no by-source side for the backward; pass the CSRGraph / BipartiteGraph")
        return segmax_side(g, x)
    if isinstance(g, GraphBatch):
        g = g.graph()
    elif isinstance(g, torch.Tensor):
        g = CSRGraph(g, x.size(0))
    if not isinstance(g, (CSRGraph, BipartiteGraph)):
        raise TypeError("segmax: the first argument is a CSRGraph, a BipartiteGraph, a GraphBatch, a CSRSide or the [2, E] edge_index")
    if x.size(0) != g.by_dst.n_cols:
        raise ValueError(f"segmax: the graph gathers from {g.by_dst.n_cols} rows, x has {x.size(0)}")
    return _SegmaxFn.apply(x, g)


def _root_only_side(graph: BipartiteGraph, res_n_id: torch.Tensor) -> CSRSide:
    """the side that scatters ``N_dst`` root rows back through ``res_n_id`` as ONE deterministic segmented sum (row ``res_n_id[i]`` holds
    entry i; duplicates accumulate in list order) -- the root term of ``SAGEConv(concat=True, aggr='max')``'s backward in the pair form;
    kept for as long as ``res_n_id`` is the same tensor in the same state (``BipartiteGraph.root_side`` is the precedent)"""
    key = (res_n_id.data_ptr(), res_n_id._version, tuple(res_n_id.shape))
    kept = graph.__dict__.get("_root_only")
    if kept is None or kept[0] != key:
        nd = graph.num_dst
        side = build_side(res_n_id.reshape(-1), torch.arange(nd, dtype=torch.int64, device=graph.device), graph.num_src, nd,
                          self_loops=False, drop_equal=False, item=graph.by_dst.item)
        kept = graph._root_only = (key, side, res_n_id)
    return kept[1]


class _SageMaxFn(torch.autograd.Function):
    """``SAGEConv(aggr='max')``: ``out = act([root |] max_{j -> i} x_j) @ W + b``.  Forward: ``npi_segmax`` (written straight into the
    right half of the GEMM's operand under ``concat``), then ``linear_fwd`` with the bias and the ``relu=`` epilogue.  Backward:
    ``linear_bwd_weight``, ``linear_bwd_data``, ``npi_segmax_bwd`` over the by-source side.  ``res_n_id``: the pair form's root rows."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph, res_n_id, concat: bool, relu: bool, flags: int):
        d = graph.by_dst
        x = _f32_rows(x, "x", "sage_conv")
        N, F = d.n_rows, x.size(1)
        if concat:
            a = torch.empty((N, 2 * F), dtype=torch.float32, device=x.device)
            if res_n_id is None:
                a[:, :F].copy_(x)
            else:
                rows_gather(x, res_n_id, a[:, :F], status=d.status)
            _, arg = segmax_side(d, x, out=a[:, F:])
        else:
            a, arg = segmax_side(d, x)
        out = linear_fwd(a, weight, bias, relu=relu, flags=flags)
        ctx.graph, ctx.F, ctx.res_n_id, ctx.concat, ctx.relu, ctx.flags = graph, F, res_n_id, concat, relu, flags
        ctx.has_bias = bias is not None
        ctx.save_for_backward(a, weight, arg, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        a, weight, arg, out = ctx.saved_tensors
        graph, F = ctx.graph, ctx.F
        g = _f32c(grad_out, "grad_out")
        if ctx.relu:
            g = relu_backward(g, out)
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = linear_bwd_weight(a, g, want_bias=ctx.has_bias, flags=ctx.flags)
        if ctx.needs_input_grad[0]:
            da = linear_bwd_data(g, weight, flags=ctx.flags)                      # [N, F], or [N, 2F]: [d root | d max]
            dx = segmax_bwd_side(graph.by_src, da[:, F:] if ctx.concat else da, arg)
            if ctx.concat and ctx.res_n_id is None:
                dx += da[:, :F]
            elif ctx.concat:
                dx += segsum(graph, _root_only_side(graph, ctx.res_n_id), da[:, :F], mean=False)
        return dx, dw, db, None, None, None, None, None


def _refuse_for_max(who: str, x, weight, bias, edge_weight) -> None:
    """what ``aggr='max'`` does not take, said before any device work; then the usual device check"""
    if edge_weight is not None:
        raise NotImplementedError(f"{who}(aggr='max'): edge_weight is not implemented (weighted messages under max are out of scope)")
    for t, name in ((x, "x"), (weight, "weight"), (bias, "bias")):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{who}(aggr='max'): {name} is {t.dtype}; max aggregation runs on float32 features and weights "
                                      "(bf16 storage is not implemented)")
    require_gpu(x, weight, bias)


def _sage_conv_max(x, edge_index, weight, bias, normalize: bool, edge_weight, relu: bool, schedule: Schedule, concat: bool):
    who = "sage_conv"
    _refuse_for_max(who, x, weight, bias, edge_weight)
    if relu and normalize:
        raise ValueError(f"{who}: relu=True applies to the projection's output; normalize=True comes after it in PyG")
    N, F = x.shape
    if weight.size(0) != (2 if concat else 1) * F:
        raise ValueError(f"{who}(aggr='max'): weight must have {(2 if concat else 1) * F} rows (got {weight.size(0)})")
    if not concat:
        graph = as_graph(edge_index, N)
    elif isinstance(edge_index, CSRGraph):                      # the edge list as it is, as for the mean
        graph = edge_index
        if graph.self_loops or not graph.keep_equal:
            raise ValueError("sage_conv(concat=True) aggregates over the edge list as it is: build the graph with "
                             "CSRGraph(edge_index, N, self_loops=False, keep_equal=True)")
        if graph.num_nodes != N:
            raise ValueError(f"CSRGraph was built for {graph.num_nodes} nodes, x has {N}")
    else:
        ei = edge_index.edge_index if hasattr(edge_index, "edge_index") else edge_index
        graph = CSRGraph(ei, N, self_loops=False, keep_equal=True)
    out = _SageMaxFn.apply(x, weight, bias, graph, None, concat, relu, _gflags(schedule))
    return l2_normalize(out) if normalize else out


def _sage_conv_bipartite_max(x, edge_index, weight, bias, size, res_n_id, normalize: bool, concat: bool, edge_weight, relu: bool,
                             schedule: Schedule):
    who = "sage_conv_bipartite"
    x_src, _, n_src, n_dst = _pair_sizes(x, size, who, edge_index)
    _refuse_for_max(who, x_src, weight, bias, edge_weight)
    if relu and normalize:
        raise ValueError(f"{who}: relu=True applies to the projection's output; normalize=True comes after it in PyG")
    if weight.size(0) != (2 if concat else 1) * x_src.size(1):
        raise ValueError(f"{who}(aggr='max'): weight must have {(2 if concat else 1) * x_src.size(1)} rows (got {weight.size(0)})")
    if concat:
        if res_n_id is None:
            raise ValueError(f"{who}(concat=True): res_n_id [N_dst] is required -- the rows of x_src that are the targets' own features")
        if res_n_id.dtype != torch.int64 or res_n_id.dim() != 1 or res_n_id.numel() != n_dst:
            raise ValueError(f"{who}: res_n_id must be a LongTensor [{n_dst}] (one row of x_src per target)")
        require_gpu(x_src, res_n_id)
    graph = _as_bipartite(edge_index, n_src, n_dst, who)
    out = _SageMaxFn.apply(x_src, weight, bias, graph, res_n_id.contiguous() if concat else None, concat, relu, _gflags(schedule))
    return l2_normalize(out) if normalize else out


# ---------------------------------------------------------------------------------------------
# GCNConv
# ---------------------------------------------------------------------------------------------
class GCNNorm:
    """Per-entry symmetric normalisation for both orientations (``GCNConv.norm``), cacheable."""

    def __init__(self, graph: CSRGraph, edge_weight: Optional[torch.Tensor] = None, improved: bool = False, keep_deg: bool = False):
        """``keep_deg``: keep the weighted degrees (``.deg``) -- the backward w.r.t. ``edge_weight`` needs them (``gcn_conv``)"""
        lib = load()
        dev = graph.device
        N = graph.num_nodes
        fill = 2.0 if improved else 1.0
        s = stream_ptr(dev)
        sides = (graph.by_dst, graph.by_src)
        w_entry = entry_weights(graph, edge_weight, fill) if (edge_weight is not None or improved) else [None, None]
        deg = None
        if w_entry[1] is not None:      # weighted degree over SOURCE rows
            deg = torch.empty(N, dtype=torch.float32, device=dev)
            check(lib.npi_row_weight_sum(ptr(graph.by_src.rowptr), ptr(w_entry[1]), N, ptr(deg), s),
                  "npi_row_weight_sum")
        self.norm = []
        for k, side in enumerate(sides):
            nrm = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev)
            check(lib.npi_gcn_norm(ptr(side.rowidx), ptr(side.col), ptr(side.rowptr), ptr(w_entry[k]), ptr(deg),
                                   ptr(graph.by_src.rowptr), N, side.nnz_max, ptr(nrm), s), "npi_gcn_norm")
            self.norm.append(nrm)
        self.graph = graph
        self.deg = deg if keep_deg else None

    @property
    def by_dst(self) -> torch.Tensor:
        return self.norm[0]

    @property
    def by_src(self) -> torch.Tensor:
        return self.norm[1]


class PlainWeights:
    """``GCNConv(normalize=False)`` (PyG 1.4.2: ``norm = edge_weight``): the per-entry weights of both orientations over the edge
    list AS IT IS -- no self loop appended, existing ones ordinary entries -- in the shape the GCN functions take (``.graph``,
    ``.by_dst``, ``.by_src``; None = unweighted)."""

    def __init__(self, edge_index, num_nodes: int, edge_weight: Optional[torch.Tensor] = None):
        if isinstance(edge_index, CSRGraph):
            if edge_index.self_loops or not edge_index.keep_equal:
                raise ValueError("GCNConv(normalize=False) aggregates over the edge list as it is: build the graph with "
                                 "CSRGraph(edge_index, N, self_loops=False, keep_equal=True)")
            self.graph = edge_index
        else:
            ei = edge_index.edge_index if hasattr(edge_index, "edge_index") else edge_index
            self.graph = CSRGraph(ei, num_nodes, self_loops=False, keep_equal=True)
        w = entry_weights(self.graph, edge_weight, 1.0) if edge_weight is not None else [None, None]
        self.by_dst, self.by_src = w


class _GcnConvFn(torch.autograd.Function):
    """PyG's literal order: project, then aggregate at width F_out (used when F_in > F_out, e.g. C1's 178 -> 64)."""

    @staticmethod
    def forward(ctx, x, weight, bias, norm: GCNNorm):
        graph = norm.graph
        xw = linear_fwd(x, weight)                                            # project first
        out = segsum(graph, graph.by_dst, xw, w=norm.by_dst, bias=bias)       # sum_e norm_e xw[src] + b
        ctx.norm = norm
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        norm: GCNNorm = ctx.norm
        graph = norm.graph
        grad_out = _fc(grad_out, "grad_out", x)
        dx = dw = db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            # the column-sum kernel is f32: bf16 storage (BASELINE.json configs[1] style training) widens dOut for it
            db = colsum(grad_out) if grad_out.dtype == torch.float32 else colsum(grad_out.float()).to(grad_out.dtype)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dxw = segsum(graph, graph.by_src, grad_out, w=norm.by_src)        # A_hat^T dOut
            if ctx.needs_input_grad[1]:
                dw, _ = linear_bwd_weight(x, dxw, want_bias=False)
            if ctx.needs_input_grad[0]:
                dx = linear_bwd_data(dxw, weight)
        return dx, dw, db, None


def gcn_conv(x: torch.Tensor, edge_index, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
             edge_weight: Optional[torch.Tensor] = None, improved: bool = False,
             norm: Optional[GCNNorm] = None, schedule: Schedule = DEFAULT, normalize: bool = True) -> torch.Tensor:
    """PyG 1.4.2 ``GCNConv.forward`` (normalize=True) on MI355X.  Evaluated as ``(A_hat x) W + b`` when the input is not wider
    than the output (``_AggProjectFn``: the aggregation at the narrower width, dW under the backward aggregation), in PyG's
    literal order ``A_hat (x W) + b`` otherwise -- the same number up to fp32 rounding.

    ``edge_weight`` is differentiable (f32 layers; bf16 storage raises ``NotImplementedError``; a precomputed ``norm=`` is a
    constant, so passing it together with an ``edge_weight`` that requires grad raises ``ValueError``).  With entry ``p`` of the
    by-target CSR = (target ``i``, source ``j``, edge ``eid[p]``), ``g_p = <dAgg[i, :], x[j, :]>``, ``dAgg = dOut W^T`` (in the
    project-first order ``<dOut[i, :], (xW)[j, :]>``, the same number):

      * ``normalize=False``: ``d edge_weight[eid[p]] = g_p`` (the edge list as it is);
      * ``normalize=True``: ``norm_p = dis[j] w_p dis[i]``, ``dis = deg^-1/2``, ``deg[k]`` = the sum of ``w_p`` over the entries
        whose source is k (loops included, weight 1 or -- ``improved`` -- 2).  ``g_p`` is the gradient w.r.t. ``norm_p``, and with
        ``s[k]`` = the sum of ``g_p norm_p`` over the entries whose source is k plus that over the entries whose target is k::

            d w_p = g_p dis[j] dis[i] - s[j] / (2 deg[j])          (both terms 0 where deg <= 0: PyG masks the inf)

        and ``d edge_weight[eid[p]] = d w_p``.  As under ``add_remaining_self_loops``, an existing self-loop edge ``(k, k)``
        receives the gradient of node k's loop entry -- if several such edges name the same node, EACH of them receives it (what
        the backward of autograd's ``index_put`` does) -- the other nodes' loop entries carry the constant fill, and padding
        columns ``(-1, -1)`` and dropped edges get 0.

    The gradient has ``edge_weight``'s shape and dtype (``_EdgeWeightGradFn``: ``npi_edge_dot``, ``npi_gcn_norm_bwd``)."""
    require_gpu(x, weight, bias)
    w_grad = _check_edge_weight_grad(edge_weight, x, weight)
    if w_grad and norm is not None:
        raise ValueError("gcn_conv: norm= is a precomputed constant; an edge_weight that requires grad cannot be passed with it "
                         "(leave norm=None, or detach the weight)")
    if norm is None:
        norm = GCNNorm(as_graph(edge_index, x.size(0)), edge_weight, improved, keep_deg=w_grad) if normalize else \
            PlainWeights(edge_index, x.size(0), edge_weight)            # normalize=False: norm = edge_weight, no self loops
    if weight.size(0) <= weight.size(1):
        # (A_hat x) W + b: the aggregation at the narrower width, the aggregate saved -- dW = agg^T dOut (db fused) no longer waits
        # for the backward aggregation and runs on the matrix cores UNDER it (C3's first layer aggregates at 178 instead of 256)
        out = _AggProjectFn.apply(x, weight, bias, norm.graph, norm.by_dst, norm.by_src, False, False, schedule, (torch.float32,))
    else:
        out = _GcnConvFn.apply(x, weight, bias, norm)
    if w_grad:
        out = _with_edge_weight_grad(out, edge_weight, x, weight, norm.graph, "gcn", False, norm)
    return out


# ---------------------------------------------------------------------------------------------
# GATConv
# ---------------------------------------------------------------------------------------------
def _transpose_map(graph: CSRGraph) -> torch.Tensor:
    """by-target position of every by-source entry (same directed edge; loop -> loop), cached."""
    tm = getattr(graph, "_tmap", None)
    if tm is None:
        lib = load()
        dev, N, E = graph.device, graph.num_nodes, graph.num_edges
        d, s_ = graph.by_dst, graph.by_src
        st = stream_ptr(dev)
        pos = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        check(lib.npi_edge_positions(ptr(d.eid), ptr(d.rowptr), N, d.nnz_max, E, ptr(pos), st), "npi_edge_positions")
        tm = torch.empty(max(s_.nnz_max, 1), dtype=torch.int32, device=dev)
        check(lib.npi_entry_transpose_map(ptr(s_.eid), ptr(s_.rowidx), ptr(s_.rowptr), ptr(d.rowptr), ptr(pos), N,
                                          s_.nnz_max, ptr(tm), st), "npi_entry_transpose_map")
        graph._tmap = tm
    return tm


def _inverse_transpose_map(graph: CSRGraph) -> torch.Tensor:
    """by-source position of every by-target entry (inverse of ``_transpose_map``), cached; index work in torch, once per graph"""
    inv = getattr(graph, "_tmap_inv", None)
    if inv is None:
        tm = _transpose_map(graph)
        n = tm.numel()
        idx = torch.arange(n, device=tm.device)
        valid = idx < graph.by_src.rowptr[-1]                       # entries past nnz (dropped edges / padding) hold garbage
        inv = torch.zeros(n + 1, dtype=torch.int32, device=tm.device)
        inv.scatter_(0, torch.where(valid, tm.long(), torch.full_like(idx, n)), idx.to(torch.int32))
        inv = inv[:n].contiguous()
        graph._tmap_inv = inv
    return inv


def _as_i64(u: int) -> int:
    """the int64 with the bits of an unsigned 64-bit number (how the C ABI takes Rule D's threshold, as it takes the key)"""
    return u - (1 << 64) if u >= (1 << 63) else u


@dataclass(frozen=True)
class AttentionDropout:
    """GATConv's attention dropout as a SEEDED rule (Rule D, ``include/npi_gnn.h``): head ``h`` of an edge is dropped iff a word that
    is a pure function of ``(seed, draw, edge, h)`` lies below ``floor(p 2^64)``; a kept attention weight is scaled by
    ``1 / (1 - p)``.  The fused kernels recompute the decision per entry from the entry's ``eid`` in both orientations, so no mask
    array exists and a step is reproducible from ``(seed, draw)``.  ``gat_conv(..., dropout=AttentionDropout(p, seed, draw))``."""
    p: float
    seed: int
    draw: int = 0

    def __post_init__(self):
        if isinstance(self.p, bool) or not isinstance(self.p, (int, float)) or not 0.0 <= float(self.p) < 1.0:
            raise ValueError(f"AttentionDropout: p must be a number in [0, 1), got {self.p!r}")
        for name in ("seed", "draw"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"AttentionDropout: {name} must be an int, got {v!r}")
        if self.draw < 0:
            raise ValueError(f"AttentionDropout: draw must be >= 0, got {self.draw!r}")

    @property
    def key(self) -> int:
        """the ``key`` of the C ABI: ``epoch_seed(seed, draw)``, as every other seeded rule"""
        return epoch_seed(self.seed, self.draw)

    @property
    def threshold(self) -> int:
        """``floor(p 2^64)`` in exact integer arithmetic, ``p`` taken as the double it is"""
        return int(Fraction(float(self.p)) * 2 ** 64)

    @property
    def scale(self) -> float:
        """``float32(1 / (1 - p))``: what a kept attention weight is multiplied by"""
        return float(torch.tensor(1.0 / (1.0 - float(self.p)), dtype=torch.float64).to(torch.float32))

    def args(self, side: CSRSide):
        """the trailing arguments of the ``*_dropout`` entry points for a launch over ``side``"""
        return ptr(side.eid), self.key, _as_i64(self.threshold), self.scale


_GAT_FUSED_SHAPES = "one head of at most 256 channels (a multiple of 4), or 2 / 4 / 8 heads of 32 / 64 / 128 channels with heads * out <= 256"


def gat_fused_shape(H: int, C: int) -> bool:
    """Shapes the fused backward serves (``npi_gat_backward_fused_heads``): ONE gather pass over the by-source entries yields
    the aggregation half of d hfeat AND every entry's score gradient -- one head of <= 256 channels, or 2 / 4 / 8 heads of
    32 / 64 / 128 channels with H C <= 256.  Everything else takes ``npi_gat_edge_grad`` (a gather pass over the by-target
    entries) followed by the by-source aggregation."""
    return C % 4 == 0 and H * C <= 256 and (H == 1 or (H in (2, 4, 8) and C in (32, 64, 128)))


def _gat_aggregate(graph, side, x, H, C, a_dst, a_src, m, s, slope, by_source, bias=None, g_dst=None,
                   g_src=None, att=None, alpha=None, alpha_map=None, x2=None, out=None):
    """``x2``: second part of a two-part table (see ``segsum``); ``out``: write into this ``[n_rows, H C]`` buffer."""
    dev = x.device
    x = _f32c(x, "x")
    x2 = _second_part(x2, x, "x2")
    out = _out_or_new(out, side.n_rows, H * C, x, "gat_aggregate")
    check(load().npi_gat_aggregate_ex(ptr(side.rowptr), ptr(side.col), ptr(side.item_row), side.item, side.n_rows, side.nnz_max,
                                      ptr(x), x.stride(0), ptr(x2), x.size(0) if x2 is not None else 0,
                                      ptr(out), out.stride(0), H, C, ptr(a_dst), ptr(a_src),
                                      ptr(m), ptr(s), float(slope), 1 if by_source else 0, ptr(bias), ptr(g_dst),
                                      ptr(g_src), ptr(att), ptr(alpha), ptr(alpha_map), ptr(side.carry(H * C)),
                                      stream_ptr(dev)), "npi_gat_aggregate")
    return out


def gat_scores(hfeat, att2, H, C):
    """a_dst[i,h] = <hfeat[i,h,:], att[h,:C]>, a_src[i,h] = <hfeat[i,h,:], att[h,C:]>"""
    dev = hfeat.device
    N = hfeat.size(0)
    a_dst = torch.empty((N, H), dtype=torch.float32, device=dev)
    a_src = torch.empty((N, H), dtype=torch.float32, device=dev)
    check(load().npi_gat_scores(ptr(hfeat), hfeat.stride(0), ptr(att2), N, H, C, ptr(a_dst), ptr(a_src), stream_ptr(dev)),
          "npi_gat_scores")
    return a_dst, a_src


def gat_softmax_stats(side: CSRSide, a_row, a_col, H, slope, want_scores: bool = False):
    """(m, s) [n_rows, H]: row max and sum of exp(. - max) of leaky_relu(a_row[row] + a_col[col]) over the entries of
    every row of ``side`` (an empty row gets m = 0, s = 0); item-parallel segmented scan (``npi_gat_softmax_stats_ex``).
    ``want_scores``: also the score of every entry ``[nnz_max, H]`` (entry order), for ``npi_gat_aggregate_scores`` --
    returns (m, s, scores)."""
    lib = load()
    dev = a_row.device
    m = torch.empty((side.n_rows, H), dtype=torch.float32, device=dev)
    s = torch.empty((side.n_rows, H), dtype=torch.float32, device=dev)
    n_ws = int(lib.npi_seg_scan_workspace_elems(side.nnz_max, H))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    e = torch.empty((max(side.nnz_max, 1), H), dtype=torch.float32, device=dev) if want_scores else None
    check(lib.npi_gat_softmax_stats_ex(ptr(side.rowptr), ptr(side.col), ptr(side.rowidx), ptr(a_row), ptr(a_col),
                                       side.n_rows, side.nnz_max, H, float(slope), ptr(m), ptr(s), ptr(e), ptr(ws), n_ws,
                                       stream_ptr(dev)), "npi_gat_softmax_stats_ex")
    return (m, s, e) if want_scores else (m, s)


def gat_rowdot(a, b, bias, H, C):
    """D[i,h] = <a[i,h,:], b[i,h,:] - bias[h,:]>"""
    dev = a.device
    N = a.size(0)
    D = torch.empty((N, H), dtype=torch.float32, device=dev)
    check(load().npi_gat_rowdot(ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(bias), N, H, C, ptr(D), stream_ptr(dev)),
          "npi_gat_rowdot")
    return D


def gat_rowdot_colsum(a, b, bias, H, C, want_colsum: bool = True, relu_mask: bool = False):
    """(D, colsum(a) or None): ``gat_rowdot`` and the bias gradient in one pass over ``a`` (= dOut) and ``b`` (= out);
    falls back on the two separate kernels for unaligned rows or H C > 1024.  ``relu_mask``: ``b`` is the output of a fused
    ReLU -- the gradient is masked first (``a' = a`` where ``b > 0``), D and the column sums use ``a'``, and ``a'`` is returned
    as a third value (the gradient of the pre-activation, which the rest of the backward consumes)."""
    lib = load()
    dev = a.device
    N = a.size(0)
    ok = (C % 4 == 0 and H * C <= 1024 and a.stride(0) % 4 == 0 and b.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0
          and b.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 16 == 0))
    if not ok:
        if relu_mask:
            a = relu_backward(a, b)
        res = (gat_rowdot(a, b, bias, H, C), (colsum(a) if want_colsum else None))
        return res + (a,) if relu_mask else res
    D = torch.empty((N, H), dtype=torch.float32, device=dev)
    cs = torch.empty(H * C, dtype=torch.float32, device=dev) if want_colsum else None
    am = torch.empty((N, H * C), dtype=torch.float32, device=dev) if relu_mask else None
    n_ws = int(lib.npi_gat_rowdot_colsum_workspace_elems(N, H, C)) if want_colsum else 0
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    check(lib.npi_gat_rowdot_colsum_relu(ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(bias), N, H, C, ptr(D), ptr(cs), ptr(am),
                                         am.stride(0) if am is not None else 0, ptr(ws), n_ws, stream_ptr(dev)),
          "npi_gat_rowdot_colsum")
    return (D, cs, am) if relu_mask else (D, cs)


def gat_aggregate_scores(side: CSRSide, table, table2, C, scores, m, s, bias=None, out=None, relu: bool = False):
    """One head: out[r] = sum_p exp(scores[p] - m[r]) / (s[r] + 1e-16) table[col p] (+ bias) over the entries of row r, the
    per-entry scores coming from ``gat_softmax_stats(..., want_scores=True)``; ``table2``: second part of a two-part table."""
    dev = table.device
    table = _f32c(table, "table")
    table2 = _second_part(table2, table, "table2")
    out = _out_or_new(out, side.n_rows, C, table, "gat_aggregate_scores")
    if side.nnz_max == 0:
        out = out.zero_() if bias is None else out.copy_(bias.view(1, -1).expand_as(out))
        return out.clamp_(min=0) if relu else out
    with _tag_events("gat_fwd_aggregate", dev):
        check(load().npi_gat_aggregate_scores(ptr(side.rowptr), ptr(side.col), ptr(side.item_row), side.item, side.n_rows,
                                              side.nnz_max, ptr(table), table.stride(0), ptr(table2),
                                              table.size(0) if table2 is not None else 0, ptr(out), out.stride(0), C, ptr(scores),
                                              ptr(m), ptr(s), ptr(bias), 1 if relu else 0, ptr(side.carry(C)), stream_ptr(dev)),
              "npi_gat_aggregate_scores")
    return out


def gat_aggregate_fused(side: CSRSide, table, table2, C, a_dst, att2, slope, bias=None, out=None, relu: bool = False,
                        scales_out: Optional[torch.Tensor] = None, H: int = 1, dropout: Optional[AttentionDropout] = None):
    """One head of at most 256 channels, or ``H`` = 2 / 4 / 8 heads on the shapes of ``gat_fused_shape``: ``(out, m, s)`` -- the
    forward aggregation together with the softmax statistics ``[n_rows, H]`` of every row, in ONE launch
    (``npi_gat_aggregate_fused_heads``): an online softmax whose scores' source half is recomputed from the gathered
    rows (``att2``: the layer's ``[H, 2C]`` attention vectors) -- no statistics pass, no per-entry score array, no gather of
    ``a_src``.  ``a_dst`` ``[n_rows, H]``; ``table2``: second part of a two-part table.  ``scales_out`` ``[n_rows]`` (one head of 256
    channels): also the power-of-two scale of every stored row (bias and ReLU applied) -- the ``x_scales`` of the next layer's
    projection.  ``dropout``: attention dropout under Rule D inside the launch (``npi_gat_aggregate_fused_heads_dropout``): an entry
    adds ``alpha kappa h_j``; ``m``, ``s`` stay the statistics of the undropped scores."""
    dev = table.device
    table = _f32c(table, "table")
    table2 = _second_part(table2, table, "table2")
    out = _out_or_new(out, side.n_rows, H * C, table, "gat_aggregate_fused")
    m = torch.empty((side.n_rows, H), dtype=torch.float32, device=dev)
    s = torch.empty((side.n_rows, H), dtype=torch.float32, device=dev)
    lib = load()
    fn, extra = (lib.npi_gat_aggregate_fused_heads, ()) if dropout is None else (lib.npi_gat_aggregate_fused_heads_dropout, dropout.args(side))
    with _tag_events("gat_fwd_aggregate", dev):
        check(fn(ptr(side.rowptr), ptr(side.col), ptr(side.rowidx), ptr(side.item_row), side.item,
                 side.n_rows, side.nnz_max, ptr(table), table.stride(0), ptr(table2),
                 table.size(0) if table2 is not None else 0, ptr(out), out.stride(0), H, C,
                 ptr(a_dst.contiguous()), ptr(_f32c(att2.reshape(-1), "att")), float(slope), ptr(bias),
                 1 if relu else 0, ptr(m), ptr(s), ptr(side.carry(H * C)), ptr(scales_out),
                 stream_ptr(dev), *extra),
              "npi_gat_aggregate_fused_heads")
    return out, m, s


def gat_pack_targets(a_dst, m, s, D, out=None):
    """[n, 4] = (a_dst, m, 1 / (s + 1e-16), D) of every target node (one head): what ``gat_backward_fused_packed`` gathers.
    ``out``: a contiguous ``[n, 4]`` f32 tensor to fill (a slice of a larger table)."""
    dev = a_dst.device
    n = a_dst.numel()
    if out is not None and (out.shape != (n, 4) or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError(f"gat_pack_targets: out must be a contiguous [{n}, 4] float32 tensor")
    t = out if out is not None else torch.empty((n, 4), dtype=torch.float32, device=dev)
    check(load().npi_gat_pack_targets(ptr(a_dst.contiguous()), ptr(m.contiguous()), ptr(s.contiguous()), ptr(D.contiguous()), n,
                                      ptr(t), stream_ptr(dev)), "npi_gat_pack_targets")
    return t


def gat_backward_fused_packed(side: CSRSide, dout, dout2, hrow, C, tpack, a_src_rows, slope, out=None, H: int = 1,
                              scales_out: Optional[torch.Tensor] = None, rowsum_out: Optional[torch.Tensor] = None,
                              dropout: Optional[AttentionDropout] = None):
    """By-SOURCE side: (out [n_rows, H C] = sum_q alpha_q dout[col q], dz [nnz_max, H] per entry and head) in one gather pass;
    ``dout2``: second part of the gathered table; ``tpack`` [n_cols H, 4] indexed by (column id, head); ``hrow`` /
    ``a_src_rows``: features and source scores of the ROW nodes.  H in {1, 2, 4, 8} (npi_gat_backward_fused_heads).
    ``scales_out`` ``[n_rows]`` (H C == 256): also the power-of-two scale of every row of ``out``, for the fp16 x 2 GEMM behind it.
    ``rowsum_out`` ``[n_rows]`` (one head): also the row sums of dz -- ``seg_rowsum(side, dz, 1)`` -- from the lanes that compute dz.
    ``dropout``: attention dropout under Rule D (``npi_gat_backward_fused_heads_dropout``): ``out = sum_q alpha_q kappa_q dout[col q]``,
    ``dz = alpha (kappa <dOut_i, h_j> - D_i) leaky_relu'``."""
    dev = dout.device
    dout = _f32c(dout, "dout")
    dout2 = _second_part(dout2, dout, "dout2")
    hrow = _f32c(hrow, "hrow")
    out = _out_or_new(out, side.n_rows, H * C, dout, "gat_backward_fused_packed")
    dz = torch.empty(max(side.nnz_max, 1) * H, dtype=torch.float32, device=dev)
    if rowsum_out is not None and (H != 1 or rowsum_out.numel() != side.n_rows or rowsum_out.dtype != torch.float32
                                   or not rowsum_out.is_contiguous()):
        raise ValueError("gat_backward_fused_packed: rowsum_out must be a contiguous float32 [n_rows] tensor (one head)")
    if side.nnz_max == 0:
        if scales_out is not None:
            scales_out.fill_(2.0 ** 126)                     # (all rows zero: what npi_row_scales gives a row with no magnitude)
        if rowsum_out is not None:
            rowsum_out.zero_()
        return out.zero_(), dz
    n_ws = int(load().npi_seg_scan_workspace_elems(side.nnz_max, 1)) if rowsum_out is not None else 0
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev) if n_ws else None
    lib = load()
    fn, extra = (lib.npi_gat_backward_fused_heads, ()) if dropout is None else (lib.npi_gat_backward_fused_heads_dropout, dropout.args(side))
    with _tag_events("gat_bwd_fused", dev):
        check(fn(ptr(side.rowptr), ptr(side.col), ptr(side.rowidx), ptr(side.item_row), side.item,
                 side.n_rows, side.nnz_max, ptr(dout), dout.stride(0), ptr(dout2),
                 dout.size(0) if dout2 is not None else 0, ptr(hrow), hrow.stride(0), ptr(out),
                 out.stride(0), H, C, ptr(tpack), ptr(a_src_rows.contiguous()), float(slope), ptr(dz),
                 ptr(side.carry(H * C)), ptr(scales_out), ptr(rowsum_out), ptr(ws), n_ws,
                 stream_ptr(dev), *extra),
              "npi_gat_backward_fused_heads")
    return out, dz


def gat_rank1_add(dh, g_dst, g_src, att2, H, C):
    """dh[j, h, :] += g_dst[j, h] att[h, :C] + g_src[j, h] att[h, C:] in place"""
    check(load().npi_gat_rank1_add(ptr(dh), dh.stride(0), ptr(g_dst), ptr(g_src), ptr(att2), dh.size(0), H, C,
                                   stream_ptr(dh.device)), "npi_gat_rank1_add")
    return dh


def gat_edge_grad(side: CSRSide, col_feat, col_feat2, row_feat, H, C, a_dst, a_src, m, s, D, slope, swap,
                  alpha_out=None, dropout: Optional[AttentionDropout] = None):
    """dz per entry of ``side`` (``npi_gat_edge_grad_ex``).  swap = 0: rows are targets (row_feat = dOut rows; a_dst,
    m, s, D by row; a_src by column; col_feat = gathered hfeat).  swap = 1: rows are sources (row_feat = their hfeat;
    a_src by row; a_dst, m, s, D by column; col_feat = gathered dOut).  ``dropout``: Rule D's factor on the dot inside dz
    (``npi_gat_edge_grad_dropout``), the same in both orientations."""
    dev = row_feat.device
    dz = torch.empty((max(side.nnz_max, 1), H), dtype=torch.float32, device=dev)
    col_feat = _f32c(col_feat, "col_feat")
    col_feat2 = _second_part(col_feat2, col_feat, "col_feat2")
    lib = load()
    fn, extra = (lib.npi_gat_edge_grad_ex, ()) if dropout is None else (lib.npi_gat_edge_grad_dropout, dropout.args(side))
    check(fn(ptr(side.rowptr), ptr(side.col), ptr(side.rowidx), side.n_rows, side.nnz_max,
             ptr(col_feat), col_feat.stride(0), ptr(col_feat2),
             col_feat.size(0) if col_feat2 is not None else 0,
             ptr(row_feat), row_feat.stride(0), H, C, ptr(a_dst), ptr(a_src), ptr(m), ptr(s),
             ptr(D), float(slope), int(swap), ptr(dz), ptr(alpha_out), stream_ptr(dev), *extra),
          "npi_gat_edge_grad")
    return dz


def seg_rowsum(side: CSRSide, vals, H, map_=None):
    """out[r, h] = sum over the entries p of row r of vals[map ? map[p] : p, h]"""
    lib = load()
    dev = vals.device
    out = torch.empty((side.n_rows, H), dtype=torch.float32, device=dev)
    n_ws = int(lib.npi_seg_scan_workspace_elems(side.nnz_max, H))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    check(lib.npi_seg_rowsum_ex(ptr(side.rowptr), ptr(side.rowidx), ptr(vals), ptr(map_), side.n_rows, side.nnz_max, H,
                                ptr(out), ptr(ws), n_ws, stream_ptr(dev)), "npi_seg_rowsum_ex")
    return out


def gat_att_grad(hfeat, g_dst, g_src, H, C):
    lib = load()
    dev = hfeat.device
    N = hfeat.size(0)
    n_ws = int(lib.npi_gat_att_grad_workspace_elems(N, H, C))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    datt = torch.empty((H, 2 * C), dtype=torch.float32, device=dev)
    check(lib.npi_gat_att_grad(ptr(hfeat), hfeat.stride(0), ptr(g_dst), ptr(g_src), N, H, C, ptr(datt), ptr(ws), n_ws,
                               stream_ptr(dev)), "npi_gat_att_grad")
    return datt


class _GatConvFn(torch.autograd.Function):
    """Returns the concatenated heads [N, H*C] (bias fused when given)."""

    @staticmethod
    def forward(ctx, x, weight, att, bias, graph: CSRGraph, heads: int, slope: float, relu: bool = False,
                sch: Schedule = DEFAULT, x_scales: Optional[torch.Tensor] = None, want_scales: bool = False,
                dropout: Optional[AttentionDropout] = None):
        H = int(heads)
        C = weight.size(1) // H
        att2 = _f32c(att.reshape(H, 2 * C), "att")
        d = graph.by_dst
        # dropout (Rule D): inside the two fused launches only -- gat_conv sends every other shape / schedule to the composed variant
        if dropout is not None and not (gat_fused_shape(H, C) and d.nnz_max > 0 and sch.gat_fused_stats):
            raise ValueError("_GatConvFn: attention dropout runs inside the fused kernels only")
        # x_scales (row_scales(x): computed once for a feature matrix that does not change between steps, or handed on by the
        # layer in front): the projection on two fp16 pieces per operand
        _check_scales(x_scales, x.size(0), "gat_conv(x_scales=)")
        xs = x_scales if (x_scales is not None and _f16x2(sch, x.size(0), weight.size(0), weight.size(1), x.dtype)) else None
        fl = _gflags(sch)                                       # (exact-f32 kernels on request: no store-epilogue fusions)
        if H == 1 and sch.gat_scores_epilogue and not fl and linear_fwd_scores_ok(x, weight):
            hfeat, a_dst, a_src = linear_fwd_scores(x, weight, att2, a_scales=xs)   # x @ W, both scores in its store epilogue
        else:
            hfeat = linear_fwd(x, weight, a_scales=xs, flags=fl)             # x @ W
            a_dst, a_src = gat_scores(hfeat, att2, H, C)
        out_scales = None
        if H == 1 and C % 4 == 0 and C <= 256 and d.nnz_max > 0 and sch.gat_fused_stats:
            # the statistics inside the aggregation launch: every item computes its entries' scores, rows cut by an item boundary
            # merge their parts' (max, sum exp) where cut rows are resolved (round 5: one pass over col / rowidx and a launch less)
            if want_scales and C == 256:
                out_scales = torch.empty(d.n_rows, dtype=torch.float32, device=x.device)
            out, m, s = gat_aggregate_fused(d, hfeat, None, C, a_dst, att2, slope, bias=bias, relu=relu, scales_out=out_scales,
                                            dropout=dropout)
        elif H > 1 and gat_fused_shape(H, C) and d.nnz_max > 0 and sch.gat_fused_stats:
            # 2 / 4 / 8 heads: the same launch, a head per group of C / 4 lanes (statistics per head, ReLU in its epilogue)
            out, m, s = gat_aggregate_fused(d, hfeat, None, C, a_dst, att2, slope, bias=bias, relu=relu, H=H, dropout=dropout)
        elif H == 1 and C % 4 == 0 and d.nnz_max > 0:
            # the statistics pass leaves the score of every entry; the aggregation reads it back (one coalesced load per
            # 64 entries) instead of gathering a_src[j] per entry and redoing the leaky_relu
            m, s, scores = gat_softmax_stats(d, a_dst, a_src, H, slope, want_scores=True)
            out = gat_aggregate_scores(d, hfeat, None, C, scores, m, s, bias=bias, relu=relu)
            del scores
        else:
            m, s = gat_softmax_stats(d, a_dst, a_src, H, slope)
            out = _gat_aggregate(graph, d, hfeat, H, C, a_dst, a_src, m, s, slope, False, bias=bias)
            if relu:                                     # several heads / odd widths: the ReLU as its own pass
                out = torch.relu_(out)
        ctx.relu = bool(relu)
        ctx.graph, ctx.H, ctx.C, ctx.slope = graph, H, C, float(slope)
        ctx.has_bias = bias is not None
        ctx.sch = sch
        ctx.dropout = dropout
        ctx.x_scales = xs                                    # (the backward's dW GEMM takes its column scales from them)
        ctx.save_for_backward(x, weight, att2, hfeat, a_dst, a_src, m, s, out,
                              bias if bias is not None else torch.empty(0, device=x.device))
        if want_scales:
            if out_scales is None:                                           # (a shape whose aggregation cannot write them)
                out_scales = torch.empty(0, dtype=torch.float32, device=x.device)
            ctx.mark_non_differentiable(out_scales)
            return out, out_scales
        return out

    @staticmethod
    def backward(ctx, grad_out, _grad_scales=None):
        x, weight, att2, hfeat, a_dst, a_src, m, s, out, bias = ctx.saved_tensors
        graph: CSRGraph = ctx.graph
        H, C, slope, sch = ctx.H, ctx.C, ctx.slope, ctx.sch
        dev = x.device
        grad_out = _f32c(grad_out, "grad_out")
        d, sr = graph.by_dst, graph.by_src
        N = graph.num_nodes
        # D_i = <dOut_i, out_i - b> = sum_p alpha_p dalpha_p  (softmax backward) and db = column sums of dOut: one pass
        # (a fused ReLU: the same pass masks the gradient first and hands the masked gradient on)
        if ctx.relu:
            D, db, grad_out = gat_rowdot_colsum(grad_out, out, bias if ctx.has_bias else None, H, C,
                                                want_colsum=ctx.has_bias and ctx.needs_input_grad[3], relu_mask=True)
        else:
            D, db = gat_rowdot_colsum(grad_out, out, bias if ctx.has_bias else None, H, C,
                                      want_colsum=ctx.has_bias and ctx.needs_input_grad[3])
        if gat_fused_shape(H, C):
            # (a_dst, m, 1/s, D) of every (target, head) in one float4; alpha is recomputed per entry by the lane that owns it
            tpack = gat_pack_targets(a_dst, m, s, D)                           # [N H, 4]
            dh = torch.empty((N, H * C), dtype=torch.float32, device=dev)
            rank2 = (sch.gat_rank2_epilogue and not sch.gemm_exact_f32 and H == 1 and N >= sch.gat_rank2_min_rows and ctx.needs_input_grad[0]
                     and x.dtype == torch.float32 and weight.size(0) % 4 == 0 and linear_bwd_data_rank2_ok(dh, weight))
            # dX's GEMM on two fp16 pieces per operand: the row scales of d hfeat from the pass that writes it (256 channels)
            dh_scales = (torch.empty(N, dtype=torch.float32, device=dev)
                         if rank2 and H * C == 256 and _f16x2(sch, N, H * C, weight.size(0), x.dtype) else None)
            # one head: the by-source row sums of dz (g_src) come out of the same launch
            g_src = torch.empty((N, 1), dtype=torch.float32, device=dev) if (H == 1 and sch.gat_src_rowsum_fused) else None
            dh, dz = gat_backward_fused_packed(sr, grad_out, None, hfeat, C, tpack, a_src, slope, out=dh, H=H, scales_out=dh_scales,
                                               rowsum_out=g_src, dropout=ctx.dropout)
            dz = dz.view(-1, H)
            if rank2:
                return _GatConvFn._backward_rank2(ctx, x, weight, att2, dh, dz, db, C, dh_scales, g_src)
            if g_src is None:
                g_src = seg_rowsum(sr, dz, H)                                     # dz is in by-source entry order here
            g_dst = seg_rowsum(d, dz, H, map_=_inverse_transpose_map(graph))
            # d hfeat_j = sum_i alpha_ij dOut_i + g_dst[j] att[:C] + g_src[j] att[C:]
            gat_rank1_add(dh, g_dst, g_src, att2, H, C)
        else:
            # dz per by-target entry, then its row sums in both orientations;
            # one head: keep the alpha this kernel computes; the by-source pass reads it back through the transpose map
            alpha = torch.empty((max(d.nnz_max, 1), H), dtype=torch.float32, device=dev) if H == 1 else None
            dz = gat_edge_grad(d, hfeat, None, grad_out, H, C, a_dst, a_src, m, s, D, slope, 0, alpha_out=alpha)
            g_dst = seg_rowsum(d, dz, H)
            g_src = seg_rowsum(sr, dz, H, map_=_transpose_map(graph))
            dh = _gat_aggregate(graph, sr, grad_out, H, C, a_dst, a_src, m, s, slope, True,
                                g_dst=g_dst, g_src=g_src, att=att2, alpha=alpha,
                                alpha_map=_transpose_map(graph) if alpha is not None else None)
        # datt streams hfeat once (HBM-bound) and depends only on g_dst / g_src; the two GEMMs that follow are MFMA-bound:
        # on large graphs the attention gradient runs on the side stream UNDER them
        overlap = (ctx.needs_input_grad[2] and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and _overlaps(sch, N))
        datt = None
        if overlap:
            main = torch.cuda.current_stream(dev)
            side = _side_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                datt = gat_att_grad(hfeat, g_dst, g_src, H, C).view(1, H, 2 * C)
            for t in (hfeat, g_dst, g_src):
                t.record_stream(side)
            datt.record_stream(main)
        elif ctx.needs_input_grad[2]:
            datt = gat_att_grad(hfeat, g_dst, g_src, H, C).view(1, H, 2 * C)
        dw = linear_bwd_weight(x, dh, want_bias=False, flags=_gflags(sch))[0] if ctx.needs_input_grad[1] else None
        dx = linear_bwd_data(dh, weight, flags=_gflags(sch)) if ctx.needs_input_grad[0] else None
        if overlap:
            main.wait_stream(side)
        return dx, dw, datt, db, None, None, None, None, None, None, None, None

    @staticmethod
    def _backward_rank2(ctx, x, weight, att2, dh, dz, db, C, dh_scales=None, g_src=None):
        """The tail of the one-head backward without ever forming d hfeat' = dh + g_dst (x) a1 + g_src (x) a2 (a1 = att[:C],
        a2 = att[C:]; g_dst / g_src = row sums of dz by target / by source).  With P = [x^T g_dst; x^T g_src] ([2, K], ONE
        pass over x):
            dX   = dh W^T + g_dst (x) (W a1) + g_src (x) (W a2)      the rank-2 term in the GEMM's store epilogue
            dW   = x^T dh + P^T [a1; a2]                              a [K, C] outer-product correction
            datt = [P W]                                              since hfeat = x W
        Only dX needs g_dst / g_src; dW = x^T dh needs neither.  So the MFMA-bound dW GEMM goes on the launch stream and the
        HBM-bound passes -- the by-target row sum of dz (a gather through the transpose map) and the pass over x -- run on
        the side stream beside it (both fit next to a dW workgroup on a CU: <= 70 VGPRs, <= 8 KB LDS); dX waits for the row
        sums only.  The [2, .] products
        are two small launches (``npi_gat_rank2_cols`` in front, ``npi_gat_rank2_tail`` behind)."""
        dev = x.device
        graph: CSRGraph = ctx.graph
        K = weight.size(0)
        A = att2.view(2, C)                                                   # rows a1, a2
        U = gat_rank2_cols(weight, A)                                         # [2, K]: W a1, W a2
        main = torch.cuda.current_stream(dev)
        overlap = _overlaps(ctx.sch, x.size(0))
        side = _side_stream(dev) if overlap else main
        # dW = x^T dh is EXPOSED here (the pass that produced dh is the layer's big HBM-bound kernel): two fp16 pieces per operand
        # when both operands come with row scales -- x's handed in (gat_conv(x_scales=)), dh's written by the fused pass -- from
        # which their column scales follow without a pass over either matrix (col_scales(row_scales=))
        dw_kw = {}
        if (dh_scales is not None and ctx.x_scales is not None and ctx.needs_input_grad[1]
                and dw_f16x2_shape(x.size(0), x.size(1), dh.size(1)) and x.dtype == torch.float32):
            dw_kw = dict(a_cs=col_scales(row_scales=ctx.x_scales, cols=x.size(1)), dc_cs=col_scales(row_scales=dh_scales, cols=dh.size(1)))
        tmap = _inverse_transpose_map(graph)                                  # cached; built on the launch stream
        # g_src handed in: the fused pass has already summed dz by source row (Schedule.gat_src_rowsum_fused).  Otherwise: dz is in
        # by-source entry order, its by-source row sum a coalesced, latency-bound pass (0.09 ms alone, 0.31 ms with one wave per
        # SIMD beside a dW workgroup), so it stays in front of dW unless the schedule asks for it beside dW
        src_beside = overlap and ctx.sch.gat_src_rowsum_beside_dw and g_src is None
        if not src_beside and g_src is None:
            g_src = seg_rowsum(graph.by_src, dz, 1)
        if overlap:
            side.wait_stream(main)
            # resident before the side stream's passes ask for wave slots
            dw = linear_bwd_weight(x, dh, want_bias=False, **dw_kw)[0] if ctx.needs_input_grad[1] else None
        with torch.cuda.stream(side):
            if src_beside:
                g_src = seg_rowsum(graph.by_src, dz, 1)
            g_dst = seg_rowsum(graph.by_dst, dz, 1, map_=tmap)                # 128-byte lines of a 4-byte permutation
            have_g = torch.cuda.Event()
            have_g.record(side)
            P = gat_att_grad(x, g_dst, g_src, 1, K).view(2, K)                # x^T g_dst, x^T g_src
        if not overlap:
            dw = linear_bwd_weight(x, dh, want_bias=False, **dw_kw)[0] if ctx.needs_input_grad[1] else None
        main.wait_event(have_g)
        dx = linear_bwd_data_rank2(dh, weight, g_dst, g_src, U[0], U[1], dc_scales=dh_scales)
        if overlap:
            for t in (x, dz, tmap, g_src):
                t.record_stream(side)
            for t in (P, g_dst) + ((g_src,) if src_beside else ()):
                t.record_stream(main)
            main.wait_stream(side)
        # dW += P^T [a1; a2] and d att = P W in one small launch behind the GEMMs
        datt = gat_rank2_tail(P, weight, A, dw, ctx.needs_input_grad[2])
        if datt is not None:
            datt = datt.view(1, 1, 2 * C)
        return dx, dw, datt, db, None, None, None, None, None, None, None, None


def _valid_entries(side: CSRSide) -> torch.Tensor:
    """``[nnz_max, 1]`` bool: entry slots that hold an entry (capacity past ``rowptr[N]`` -- dropped self loops, out-of-range ids -- is
    never written by the CSR build and never read by a kernel; element-wise torch ops over whole entry arrays must mask it)"""
    return (torch.arange(max(side.nnz_max, 1), device=side.rowptr.device) < side.rowptr[-1]).view(-1, 1)


class _GatDropoutFn(torch.autograd.Function):
    """GATConv with ATTENTION DROPOUT in training mode (PyG 1.4.2 ``GATConv.message``: ``alpha = softmax(alpha, edge_index_i)``,
    ``alpha = F.dropout(alpha, p, training)``, ``x_j * alpha``).  ``keep`` ``[nnz_max, H]``, in by-target entry order, holds
    ``0`` for a dropped attention weight and ``1 / (1 - p)`` for a kept one.  The layer's fast kernels never hold alpha (both
    directions recompute it per entry), so this variant -- a regulariser for small graphs, used by nothing in the reference --
    materialises alpha per entry and head and is COMPOSED from the per-op kernels: the score / statistics pass, one weighted
    aggregation per head in each direction (``npi_segsum_ex`` with per-entry weights over a column block), the per-entry dots
    ``<dOut_i, h_j>`` from ``npi_gat_edge_grad`` (called with alpha = 1, D = 0, slope = 1: its dz IS the dot), segmented row sums
    and the element-wise softmax backward on ``[nnz, H]`` arrays in torch.  With dropout the softmax term is unchanged:
    ``sum_j alpha_ij dalpha_ij = sum_j alpha'_ij <dOut_i, h_j> = <dOut_i, out_i - b>`` (alpha' = alpha keep)."""

    @staticmethod
    def forward(ctx, x, weight, att, bias, graph: CSRGraph, heads: int, slope: float, keep: torch.Tensor):
        H = int(heads)
        C = weight.size(1) // H
        att2 = _f32c(att.reshape(H, 2 * C), "att")
        d = graph.by_dst
        N = d.n_rows
        keep = _f32c(keep, "keep")
        if keep.shape != (max(d.nnz_max, 1), H):
            raise ValueError(f"gat_conv: keep must be [{max(d.nnz_max, 1)}, {H}] (by-target entry order), got {tuple(keep.shape)}")
        hfeat = linear_fwd(x, weight)
        a_dst, a_src = gat_scores(hfeat, att2, H, C)
        m, s, e = gat_softmax_stats(d, a_dst, a_src, H, slope, want_scores=True)
        ri = d.rowidx.long().clamp_(0, max(N - 1, 0))                       # (slots past nnz hold garbage row ids)
        valid = _valid_entries(d)
        alpha = torch.where(valid, torch.exp(e - m[ri]) / (s[ri] + 1e-16), torch.zeros((), device=x.device))
        alpha_k = torch.where(valid, alpha * keep, torch.zeros((), device=x.device))
        out = torch.empty((N, H * C), dtype=torch.float32, device=x.device)
        for h in range(H):
            blk = slice(h * C, (h + 1) * C)
            segsum(graph, d, hfeat[:, blk], w=alpha_k[:, h].contiguous(), out=out[:, blk],
                   bias=bias[blk].contiguous() if bias is not None else None)
        ctx.graph, ctx.H, ctx.C, ctx.slope, ctx.has_bias = graph, H, C, float(slope), bias is not None
        ctx.save_for_backward(x, weight, att2, hfeat, e, alpha, alpha_k, keep, out,
                              bias if bias is not None else torch.empty(0, device=x.device))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, att2, hfeat, e, alpha, alpha_k, keep, out, bias = ctx.saved_tensors
        graph: CSRGraph = ctx.graph
        H, C, slope = ctx.H, ctx.C, ctx.slope
        dev = x.device
        grad_out = _f32c(grad_out, "grad_out")
        d, sr = graph.by_dst, graph.by_src
        N = d.n_rows
        D, db = gat_rowdot_colsum(grad_out, out, bias if ctx.has_bias else None, H, C,
                                  want_colsum=ctx.has_bias and ctx.needs_input_grad[3])
        zeros, ones = torch.zeros((N, H), device=dev), torch.ones((N, H), device=dev)
        if C % 4 == 0:
            dots = gat_edge_grad(d, hfeat, None, grad_out, H, C, zeros, zeros, zeros, ones, zeros, 1.0, 0)    # <dOut_i, h_j>
        else:                                 # rows that are no multiple of 16 bytes: the per-entry dots of one head at a time
            dots = torch.stack([edge_dot(d, grad_out[:, h * C:(h + 1) * C], hfeat[:, h * C:(h + 1) * C], graph.num_edges,
                                         want_entry=True)[0] for h in range(H)], dim=1)
        ri = d.rowidx.long().clamp_(0, max(N - 1, 0))
        zero = torch.zeros((), device=dev)
        gprime = torch.where(e > 0, torch.ones((), device=dev), torch.full((), slope, device=dev))        # e = leaky_relu(z)
        dz = torch.where(_valid_entries(d), alpha * (keep * dots - D[ri]) * gprime, zero)
        tm = _transpose_map(graph)
        g_dst = seg_rowsum(d, dz, H)
        g_src = seg_rowsum(sr, dz, H, map_=tm)
        # d hfeat_j = sum_i alpha'_ij dOut_i + g_dst[j] att[:C] + g_src[j] att[C:]
        alpha_src = torch.where(_valid_entries(sr), alpha_k[tm.long().clamp_(0, alpha_k.size(0) - 1)], zero)
        dh = torch.empty((N, H * C), dtype=torch.float32, device=dev)
        for h in range(H):
            blk = slice(h * C, (h + 1) * C)
            segsum(graph, sr, grad_out[:, blk], w=alpha_src[:, h].contiguous(), out=dh[:, blk])
        if C % 4 == 0:
            gat_rank1_add(dh, g_dst, g_src, att2, H, C)
        else:                                 # (npi_gat_rank1_add works on 16-byte lanes: element-wise here, as the softmax backward)
            dh.view(N, H, C).add_(g_dst.unsqueeze(-1) * att2[:, :C]).add_(g_src.unsqueeze(-1) * att2[:, C:])
        datt = gat_att_grad(hfeat, g_dst, g_src, H, C).view(1, H, 2 * C) if ctx.needs_input_grad[2] else None
        dw = linear_bwd_weight(x, dh, want_bias=False)[0] if ctx.needs_input_grad[1] else None
        dx = linear_bwd_data(dh, weight) if ctx.needs_input_grad[0] else None
        return dx, dw, datt, db, None, None, None, None


def gat_dropout_keep(graph, heads: int, p: float, seed: Optional[int] = None, draw: int = 0, side: str = "by_dst") -> torch.Tensor:
    """A ``keep`` array for ``gat_conv(..., keep=)``.  ``seed`` None: a fresh one, Bernoulli(1 - p) / (1 - p) per by-target entry
    and head (torch's generator: the distribution of ``F.dropout``, not its random bits for a given seed).  ``seed`` an int: the
    mask of ``AttentionDropout(p, seed, draw)`` -- Rule D, what the fused kernels recompute per entry -- written out as
    ``[nnz_max, heads]`` in the entry order of ``side`` (``"by_dst"`` or ``"by_src"``) of a ``CSRGraph`` or ``BipartiteGraph``
    (``npi_gat_dropout_keep``); slots behind the last entry hold 0."""
    if not 0.0 <= p < 1.0:
        raise ValueError("gat_dropout_keep: p must be in [0, 1)")
    if seed is None:
        d = graph.by_dst
        return torch.empty((max(d.nnz_max, 1), int(heads)), dtype=torch.float32, device=d.rowptr.device).bernoulli_(1.0 - p).div_(1.0 - p)
    if side not in ("by_dst", "by_src"):
        raise ValueError(f"gat_dropout_keep: side is 'by_dst' or 'by_src', got {side!r}")
    rule = AttentionDropout(p, seed, draw)
    sd: CSRSide = getattr(graph, side)
    dev = sd.rowptr.device
    keep = torch.zeros((max(sd.nnz_max, 1), int(heads)), dtype=torch.float32, device=dev)
    check(load().npi_gat_dropout_keep(ptr(sd.rowptr), ptr(sd.col), ptr(sd.eid), sd.n_rows, sd.nnz_max, int(heads), rule.key,
                                      _as_i64(rule.threshold), rule.scale, ptr(keep), stream_ptr(dev)), "npi_gat_dropout_keep")
    return keep


def gat_conv(x: torch.Tensor, edge_index, weight: torch.Tensor, att: torch.Tensor,
             bias: Optional[torch.Tensor] = None, heads: int = 1, concat: bool = True,
             negative_slope: float = 0.2, relu: bool = False, schedule: Schedule = DEFAULT,
             keep: Optional[torch.Tensor] = None, x_scales: Optional[torch.Tensor] = None, return_scales: bool = False,
             dropout: Optional[AttentionDropout] = None):
    """PyG 1.4.2 ``GATConv.forward`` on MI355X; ``att`` is ``[1, H, 2C]``.  ``relu=True`` (an extension, as in
    ``sage_conv``): ``F.relu(conv(x, edge_index))`` with the ReLU in the aggregation's row epilogue and its backward mask in the
    pass that computes the softmax term -- one head; other shapes apply it as a separate pass.  ``keep``: attention dropout in
    training mode (``_GatDropoutFn``; ``gat_dropout_keep`` draws one) -- the composed, slower variant of the layer.
    ``x_scales``: ``row_scales(x)`` -- the projection ``x @ W`` then runs on two fp16 pieces per operand (large graphs; EXPERIMENTS
    A34).  Computed ONCE for a feature matrix that does not change between steps, or taken from the layer in front:
    ``return_scales=True`` returns ``(out, out_scales)`` with the scales of the output's rows written by the aggregation launch
    itself (one head of 256 channels; otherwise ``out_scales`` is None) -- what the next layer takes as its ``x_scales``.
    ``dropout``: an ``AttentionDropout(p, seed, draw)`` -- attention dropout in training mode as a seeded rule, recomputed per entry
    INSIDE the fused kernels on the shapes of ``gat_fused_shape`` with the default schedule (every option above keeps working);
    other shapes and ``gat_fused_stats=False`` take the composed variant under the SAME mask (``gat_dropout_keep(seed=)``)."""
    require_gpu(x, weight, att, bias, x_scales)
    graph = as_graph(edge_index, x.size(0))
    if dropout is not None:
        if keep is not None:
            raise ValueError("gat_conv: keep= and dropout= are two ways to say the mask; pass one")
        if not isinstance(dropout, AttentionDropout):
            raise TypeError(f"gat_conv: dropout is an AttentionDropout(p, seed, draw), got {type(dropout).__name__}")
        H = int(heads)
        if not (gat_fused_shape(H, weight.size(1) // H) and graph.by_dst.nnz_max > 0 and schedule.gat_fused_stats):
            keep, dropout = gat_dropout_keep(graph, H, dropout.p, seed=dropout.seed, draw=dropout.draw), None
    if keep is not None:
        out = _GatDropoutFn.apply(x, weight, att, bias if concat else None, graph, heads, negative_slope, keep)
        if not concat:
            out = out.view(x.size(0), heads, -1).mean(dim=1)
            out = out + bias if bias is not None else out
        out = torch.relu(out) if relu else out
        return (out, None) if return_scales else out
    if concat:
        if return_scales:
            out, sc = _GatConvFn.apply(x, weight, att, bias, graph, heads, negative_slope, relu, schedule, x_scales, True, dropout)
            return out, (sc if sc.numel() else None)
        return _GatConvFn.apply(x, weight, att, bias, graph, heads, negative_slope, relu, schedule, x_scales, False, dropout)
    out = _GatConvFn.apply(x, weight, att, None, graph, heads, negative_slope, False, schedule, x_scales, False, dropout)
    out = out.view(x.size(0), heads, -1).mean(dim=1)          # head average (concat=False)
    out = out + bias if bias is not None else out
    out = torch.relu(out) if relu else out
    return (out, None) if return_scales else out


# ---------------------------------------------------------------------------------------------
# Bipartite ``(x_src, x_dst)`` / ``size=`` form of SAGEConv and GATConv (PyG 1.4.2 MessagePassing.propagate with a size pair)
# ---------------------------------------------------------------------------------------------
# Everything under these layers already has two id spaces -- the CSR build, the aggregation (plain and hub-streamed), the per-entry
# dots, the GAT statistics / aggregation / backward kernels and the GEMMs, built for the sharded layers -- so the layers below are
# compositions of those entry points over the sides of a ``graph.BipartiteGraph``.  The one new kernel is ``npi_rows_gather``.
def rows_gather(x: torch.Tensor, idx: Optional[torch.Tensor], out: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i, :] = x[idx[i], :]`` (``idx`` None: the identity) in one pass, ``out`` possibly a column block of a wider buffer
    (``npi_rows_gather``).  f32 or bf16, unit column stride.  An id outside ``[0, x.size(0))`` gives a ZERO row and raises
    ``NPI_STATUS_BAD_ROW_ID`` in ``status`` (an int32 device word, e.g. a side's; filed with ``note_status`` here: the host sees it
    at its next device read); no synchronisation."""
    dev = require_gpu(x, idx, out, status)
    for t, name in ((x, "x"), (out, "out")):
        if t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.size(1):
            raise ValueError(f"rows_gather: {name} must be float32 / bfloat16 [rows, F] with unit column stride")
    n, F = out.shape
    if x.dtype != out.dtype or x.size(1) != F or x.device != out.device:
        raise ValueError("rows_gather: x and out must share dtype, width and device")
    if idx is not None:
        if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() != n or not idx.is_contiguous():
            raise ValueError(f"rows_gather: idx must be a contiguous LongTensor [{n}]")
    elif x.size(0) < n:
        raise ValueError("rows_gather: the identity gather needs at least as many source rows as output rows")
    if status is not None and (status.dtype != torch.int32 or status.numel() < 1):
        raise ValueError("rows_gather: status must be an int32 device word")
    check(load().npi_rows_gather(ptr(x), x.stride(0), x.size(0), ptr(idx), n, F, ptr(out), out.stride(0), _code(x), ptr(status),
                                 stream_ptr(dev)), "npi_rows_gather")
    if status is not None and idx is not None:
        note_status(status)
    return out


def _pair_sizes(x, size, who: str, edge_index=None):
    """PyG 1.4.2 size resolution of the pair form: ``(x_src, x_dst or None, N_src, N_dst)``; every mismatch is a ValueError.
    A ``BipartiteGraph`` in place of ``edge_index`` names ``N_dst`` where neither ``x_dst`` nor ``size[1]`` does."""
    if len(x) != 2:
        raise ValueError(f"{who}: the bipartite form takes x = (x_src, x_dst) (x_dst may be None)")
    x_src, x_dst = x
    if x_src is None:
        raise ValueError(f"{who}: x_src (x[0]) is required: the messages are gathered from it")
    for t, name in ((x_src, "x_src"), (x_dst, "x_dst")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 2):
            raise ValueError(f"{who}: {name} must be a [rows, F] tensor")
    if size is not None and (not isinstance(size, (tuple, list)) or len(size) != 2):
        raise ValueError(f"{who}: size must be a pair (N_src, N_dst)")
    s0, s1 = (None, None) if size is None else size
    n_src = int(x_src.size(0))
    if s0 is not None and int(s0) != n_src:
        raise ValueError(f"{who}: x_src has {n_src} rows, size[0] is {int(s0)}")
    if x_dst is not None:
        n_dst = int(x_dst.size(0))
        if s1 is not None and int(s1) != n_dst:
            raise ValueError(f"{who}: x_dst has {n_dst} rows, size[1] is {int(s1)}")
    else:
        n_dst = int(s1) if s1 is not None else (edge_index.num_dst if isinstance(edge_index, BipartiteGraph) else n_src)
    return x_src, x_dst, n_src, n_dst


def _as_bipartite(edge_index, n_src: int, n_dst: int, who: str) -> BipartiteGraph:
    if isinstance(edge_index, (CSRGraph, GraphBatch)):
        raise TypeError(f"{who}: a {type(edge_index).__name__} holds ONE id space (self loops included); the pair form (x_src, x_dst) "
                        "takes the [2, E] edge_index or a BipartiteGraph")
    if isinstance(edge_index, BipartiteGraph):
        if edge_index.size != (n_src, n_dst):
            raise ValueError(f"{who}: the BipartiteGraph was built for size {edge_index.size}, the features give {(n_src, n_dst)}")
        return edge_index
    if not isinstance(edge_index, torch.Tensor):
        raise TypeError(f"{who}: edge_index must be the [2, E] LongTensor or a BipartiteGraph")
    return BipartiteGraph(edge_index, (n_src, n_dst))


def _bipartite_entry_weights(graph: BipartiteGraph, edge_weight: torch.Tensor):
    """``edge_weight [E]`` in the entry order of both sides (there are no loop entries): ``[by_dst, by_src]``, and the flat weight"""
    dev = require_gpu(edge_weight)
    ew = _f32c(edge_weight.detach(), "edge_weight").view(-1)
    if ew.numel() != graph.num_edges:
        raise ValueError(f"edge_weight has {ew.numel()} entries, edge_index {graph.num_edges} columns")
    out = []
    for side in (graph.by_dst, graph.by_src):
        we = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev)
        check(load().npi_entry_weights(ptr(side.eid), ptr(side.rowidx), ptr(side.rowptr), ptr(ew), 0, 1.0, side.n_rows, side.nnz_max,
                                       ptr(we), stream_ptr(dev)), "npi_entry_weights")
        out.append(we)
    return out, ew


def _root_weights(graph: BipartiteGraph, side: CSRSide, ew: Optional[torch.Tensor]) -> torch.Tensor:
    """per-entry weights of ``BipartiteGraph.root_side``: ``inv_count[i]`` (times the edge's weight) for an edge entry whose target
    is i, 1 for a root entry -- ``npi_entry_col_scale`` over the table ``[inv_count ; ones]``; without edge weights kept on the side"""
    if ew is None and "_root_w" in side.__dict__:
        return side._root_w
    dev, nd = graph.device, graph.num_dst
    table = torch.cat([graph.inv_count(), torch.ones(nd, dtype=torch.float32, device=dev)])
    w_in = None
    if ew is not None:
        ext = torch.cat([ew, torch.ones(nd, dtype=torch.float32, device=dev)])             # eid of a root entry: E + i
        w_in = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev)
        check(load().npi_entry_weights(ptr(side.eid), ptr(side.rowidx), ptr(side.rowptr), ptr(ext), 0, 1.0, side.n_rows, side.nnz_max,
                                       ptr(w_in), stream_ptr(dev)), "npi_entry_weights")
    out = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=dev)
    check(load().npi_entry_col_scale(ptr(side.col), ptr(side.rowptr), ptr(table), ptr(w_in), side.n_rows, 2 * nd, side.nnz_max,
                                     ptr(out), stream_ptr(dev)), "npi_entry_col_scale")
    if ew is None:
        side._root_w = out
    return out


class _SageBipartiteConcatFn(torch.autograd.Function):
    """``out = [x_src[res_n_id] | mean_{e: j -> i}(w_e x_src[j])] @ W[2F, Fo] + b``: the gathered roots (``npi_rows_gather``) and the
    mean (``segsum(out=)``) are written straight into the two halves of the ``[N_dst, 2F]`` operand of ONE projection GEMM.  The
    backward's ``dX_src`` -- the transposed aggregation of ``dcat[:, F:] / count`` plus the scatter of ``dcat[:, :F]`` through
    ``res_n_id`` -- is ONE segmented sum over ``BipartiteGraph.root_side`` with the two halves of ``dcat`` as the two parts of its
    table: a fixed order, no float atomics, bitwise reproducible; duplicates in ``res_n_id`` accumulate."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph: BipartiteGraph, res_n_id, w_entry=None, ew=None):
        d = graph.by_dst
        F = x.size(1)
        cat = torch.empty((d.n_rows, 2 * F), dtype=x.dtype, device=x.device)
        rows_gather(x, res_n_id, cat[:, :F], status=d.status)
        segsum(graph, d, x, w=w_entry[0] if w_entry else None, mean=True, out=cat[:, F:])
        out = linear_fwd(cat, weight, bias)
        ctx.graph, ctx.F, ctx.res_n_id, ctx.ew = graph, F, res_n_id, ew
        ctx.has_bias = bias is not None
        ctx.save_for_backward(cat, weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cat, weight = ctx.saved_tensors
        graph: BipartiteGraph = ctx.graph
        F = ctx.F
        grad_out = _f32c(grad_out, "grad_out")
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = linear_bwd_weight(cat, grad_out, want_bias=ctx.has_bias)
        if ctx.needs_input_grad[0]:
            dcat = linear_bwd_data(grad_out, weight)                              # [N_dst, 2F]: [d root | d mean]
            side = graph.root_side(ctx.res_n_id)
            dx = segsum(graph, side, dcat[:, F:], w=_root_weights(graph, side, ctx.ew), x2=dcat[:, :F], mean=False)
        return dx, dw, db, None, None, None, None


def sage_conv_bipartite(x, edge_index, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, size=None,
                        res_n_id: Optional[torch.Tensor] = None, normalize: bool = False, concat: bool = False,
                        edge_weight: Optional[torch.Tensor] = None, relu: bool = False, schedule: Schedule = DEFAULT,
                        aggr: str = "mean") -> torch.Tensor:
    """PyG 1.4.2 ``SAGEConv.forward((x_src, x_dst), edge_index, edge_weight, size, res_n_id)``: ``edge_index[0]`` indexes
    ``x_src``, ``edge_index[1]`` the ``N_dst`` output rows (``N_dst``: ``x_dst``'s rows, else ``size[1]``, else ``N_src``).  No self
    loop is added or removed; a target without an in-edge gets ``bias`` (or 0).

    ``concat=False``: ``mean_{e: j -> i}(w_e x_src[j]) @ weight + bias`` (the mean divides by the in-edge count); ``x_dst`` is not
    read.  ``concat=True``: ``[x_src[res_n_id] | mean] @ weight[2F, out] + bias`` with ``res_n_id`` a LongTensor ``[N_dst]`` of rows
    of ``x_src`` (an id out of range gives a zero root row and is reported like a dropped edge, ``graph.note_status``).
    ``edge_index``: the ``[2, E]`` tensor (sorted here, every call) or a ``BipartiteGraph``.  float32 only.  Gradients: ``x_src``,
    ``weight``, ``bias`` and ``edge_weight`` (``d edge_weight[e] = inv_count[i] <dAgg[i], x_src[j]>``, ``npi_edge_dot`` over the
    by-target side).  ``aggr="max"``: the maximum over a target's in-edges instead of their mean (``segmax``, Rule X; no ``edge_weight``)."""
    who = "sage_conv_bipartite"
    if aggr != "mean":
        _check_aggr(aggr, who)
        return _sage_conv_bipartite_max(x, edge_index, weight, bias, size, res_n_id, normalize, concat, edge_weight, relu, schedule)
    x_src, x_dst, n_src, n_dst = _pair_sizes(x, size, who, edge_index)
    if concat and res_n_id is None:
        raise ValueError(f"{who}(concat=True): res_n_id [N_dst] is required -- the rows of x_src that are the targets' own features")
    if relu and normalize and not concat:
        raise ValueError(f"{who}: relu=True applies to the projection's output; normalize=True comes after it in PyG")
    if isinstance(edge_index, (CSRGraph, GraphBatch)):
        _as_bipartite(edge_index, n_src, n_dst, who)
    if weight.size(0) != (2 if concat else 1) * x_src.size(1):
        raise ValueError(f"{who}: weight must have {(2 if concat else 1) * x_src.size(1)} rows (got {weight.size(0)})")
    if concat and (res_n_id.dtype != torch.int64 or res_n_id.dim() != 1 or res_n_id.numel() != n_dst):
        raise ValueError(f"{who}: res_n_id must be a LongTensor [{n_dst}] (one row of x_src per target)")
    require_gpu(x_src, weight, bias, edge_weight, res_n_id)
    if x_src.dtype != torch.float32 or weight.dtype != torch.float32:
        raise NotImplementedError(f"{who}: the bipartite layers run on float32 features and weights (bf16 storage is not implemented "
                                  "for the pair form)")
    w_grad = _check_edge_weight_grad(edge_weight, x_src, weight)
    graph = _as_bipartite(edge_index, n_src, n_dst, who)
    x_in = x_src
    x_src = _f32c(x_src, "x_src")
    w_entry = ew = None
    if edge_weight is not None:
        w_entry, ew = _bipartite_entry_weights(graph, edge_weight)
    if concat:
        out = _SageBipartiteConcatFn.apply(x_src, weight, bias, graph, res_n_id.contiguous(), w_entry, ew)
        if w_grad:
            out = _with_edge_weight_grad(out, edge_weight, x_in, weight, graph, "concat")
        if relu:
            out = torch.relu(out)
        return l2_normalize(out) if normalize else out
    w_dst, w_src = w_entry or (None, None)
    out = _AggProjectFn.apply(x_src, weight, bias, graph, w_dst, w_src, True, relu, schedule, ())
    if w_grad:
        out = _with_edge_weight_grad(out, edge_weight, x_in, weight, graph, "sage", relu)
    return l2_normalize(out) if normalize else out


class _GatBipartiteFn(torch.autograd.Function):
    """GATConv over a ``BipartiteGraph``: ``h_src = x_src W``, ``h_dst = x_dst W`` (the same W; ``shared``: ``x_dst`` IS ``x_src``,
    projected once), ``e = leaky_relu(<h_dst[i], att[:C]> + <h_src[j], att[C:]>)`` (no target term when ``x_dst`` is None), softmax
    over the in-edges of i with the ``+1e-16`` denominator, ``out[i] = sum alpha h_src[j]`` (+ bias).  Composed from the per-op entry
    points, which take row and column tables separately: one head takes the fused aggregation (statistics inside the launch) and,
    on the shapes ``gat_fused_shape`` names, the packed fused backward over ``by_src`` (d h_src, dz and its by-source row sums in
    one gather pass); ``g_dst`` -- needed only when there is a target term -- is one ``npi_gat_edge_grad`` pass over ``by_dst``."""

    @staticmethod
    def forward(ctx, x_src, x_dst, weight, att, bias, graph: BipartiteGraph, heads: int, slope: float, relu: bool, sch: Schedule,
                shared: bool, dropout: Optional[AttentionDropout] = None):
        H = int(heads)
        C = weight.size(1) // H
        dev = x_src.device
        att2 = _f32c(att.reshape(H, 2 * C), "att")
        d = graph.by_dst
        fl = _gflags(sch)
        h_src = linear_fwd(x_src, weight, flags=fl)
        a_own, a_src = gat_scores(h_src, att2, H, C)
        h_dst = None
        if shared:
            a_dst = a_own
        elif x_dst is not None:
            h_dst = linear_fwd(x_dst, weight, flags=fl)
            a_dst, _ = gat_scores(h_dst, att2, H, C)
        else:
            a_dst = torch.zeros((d.n_rows, H), dtype=torch.float32, device=dev)
        del a_own
        if d.nnz_max == 0:                                       # no edges: every row is empty -- zeros (+ bias)
            m = torch.zeros((d.n_rows, H), dtype=torch.float32, device=dev)
            s = torch.zeros((d.n_rows, H), dtype=torch.float32, device=dev)
            out = torch.zeros((d.n_rows, H * C), dtype=torch.float32, device=dev)
            if bias is not None:
                out += bias.view(1, -1)
            if relu:
                out = torch.relu_(out)
        elif H == 1 and C % 4 == 0 and C <= 256 and sch.gat_fused_stats:
            out, m, s = gat_aggregate_fused(d, h_src, None, C, a_dst, att2, slope, bias=bias, relu=relu, dropout=dropout)
        elif H > 1 and gat_fused_shape(H, C) and sch.gat_fused_stats:
            out, m, s = gat_aggregate_fused(d, h_src, None, C, a_dst, att2, slope, bias=bias, relu=relu, H=H, dropout=dropout)
        elif dropout is not None:                                # (gat_conv_bipartite refuses these before it gets here)
            raise NotImplementedError("_GatBipartiteFn: attention dropout runs inside the fused kernels only")
        else:
            m, s = gat_softmax_stats(d, a_dst, a_src, H, slope)
            out = _gat_aggregate(graph, d, h_src, H, C, a_dst, a_src, m, s, slope, False, bias=bias)
            if relu:
                out = torch.relu_(out)
        ctx.graph, ctx.H, ctx.C, ctx.slope, ctx.sch = graph, H, C, float(slope), sch
        ctx.dropout = dropout
        ctx.relu, ctx.shared, ctx.has_dst, ctx.has_bias = bool(relu), bool(shared), x_dst is not None, bias is not None
        empty = torch.empty(0, device=dev)
        ctx.save_for_backward(x_src, x_dst if x_dst is not None else empty, weight, att2, h_src, h_dst if h_dst is not None else empty,
                              a_dst, a_src, m, s, out, bias if bias is not None else empty)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x_src, x_dst, weight, att2, h_src, h_dst, a_dst, a_src, m, s, out, bias = ctx.saved_tensors
        graph: BipartiteGraph = ctx.graph
        H, C, slope, sch = ctx.H, ctx.C, ctx.slope, ctx.sch
        dev = x_src.device
        grad_out = _f32c(grad_out, "grad_out")
        d, sr = graph.by_dst, graph.by_src
        n_src, n_dst = sr.n_rows, d.n_rows
        want_db = ctx.has_bias and ctx.needs_input_grad[4]
        if ctx.relu:
            D, db, grad_out = gat_rowdot_colsum(grad_out, out, bias if ctx.has_bias else None, H, C, want_colsum=want_db, relu_mask=True)
        else:
            D, db = gat_rowdot_colsum(grad_out, out, bias if ctx.has_bias else None, H, C, want_colsum=want_db)
        target_term = ctx.shared or ctx.has_dst
        zeros = lambda n: torch.zeros((n, H), dtype=torch.float32, device=dev)            # noqa: E731
        g_dst = None
        if d.nnz_max == 0:
            dh = torch.zeros((n_src, H * C), dtype=torch.float32, device=dev)
            g_src = zeros(n_src)
            g_dst = zeros(n_dst)
        else:
            if gat_fused_shape(H, C):
                tpack = gat_pack_targets(a_dst, m, s, D)                                 # [N_dst H, 4], gathered by column id
                g_src = torch.empty((n_src, 1), dtype=torch.float32, device=dev) if (H == 1 and sch.gat_src_rowsum_fused) else None
                dh, dz = gat_backward_fused_packed(sr, grad_out, None, h_src, C, tpack, a_src, slope, H=H, rowsum_out=g_src,
                                                   dropout=ctx.dropout)
                if g_src is None:
                    g_src = seg_rowsum(sr, dz.view(-1, H), H)
            else:
                # rows are sources: dz recomputed in the orientation it is summed in, then the by-source aggregation of dOut
                dz = gat_edge_grad(sr, grad_out, None, h_src, H, C, a_dst, a_src, m, s, D, slope, 1)
                g_src = seg_rowsum(sr, dz, H)
                dh = _gat_aggregate(graph, sr, grad_out, H, C, a_dst, a_src, m, s, slope, True)
            del dz
            if target_term:
                dz = gat_edge_grad(d, h_src, None, grad_out, H, C, a_dst, a_src, m, s, D, slope, 0, dropout=ctx.dropout)
                g_dst = seg_rowsum(d, dz, H)
                del dz
        fl = _gflags(sch)
        want_w, want_att = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dx_src = dx_dst = dw = datt = None
        if ctx.shared:
            # one id space: d h_j = sum_i alpha_ij dOut_i + g_dst[j] att[:C] + g_src[j] att[C:]
            gat_rank1_add(dh, g_dst, g_src, att2, H, C)
            if want_att:
                datt = gat_att_grad(h_src, g_dst, g_src, H, C)
            if want_w:
                dw = linear_bwd_weight(x_src, dh, want_bias=False, flags=fl)[0]
            if ctx.needs_input_grad[0]:
                dx_src = linear_bwd_data(dh, weight, flags=fl)
        else:
            gat_rank1_add(dh, zeros(n_src), g_src, att2, H, C)                           # d h_src_j += g_src[j] att[C:]
            if want_att:
                datt = gat_att_grad(h_src, zeros(n_src), g_src, H, C)                    # (its [:C] half is zero)
            if want_w:
                dw = linear_bwd_weight(x_src, dh, want_bias=False, flags=fl)[0]
            if ctx.needs_input_grad[0]:
                dx_src = linear_bwd_data(dh, weight, flags=fl)
            if ctx.has_dst and (want_w or want_att or ctx.needs_input_grad[1]):
                dh_dst = torch.zeros((n_dst, H * C), dtype=torch.float32, device=dev)
                gat_rank1_add(dh_dst, g_dst, zeros(n_dst), att2, H, C)                   # d h_dst_i = g_dst[i] att[:C]
                if want_att:
                    datt = datt + gat_att_grad(h_dst, g_dst, zeros(n_dst), H, C)
                if want_w:
                    dw = dw + linear_bwd_weight(x_dst, dh_dst, want_bias=False, flags=fl)[0]      # dW = x_src^T dh_src + x_dst^T dh_dst
                if ctx.needs_input_grad[1]:
                    dx_dst = linear_bwd_data(dh_dst, weight, flags=fl)
        if datt is not None:
            datt = datt.view(1, H, 2 * C)
        return dx_src, dx_dst, dw, datt, db, None, None, None, None, None, None, None


def gat_conv_bipartite(x, edge_index, weight: torch.Tensor, att: torch.Tensor, bias: Optional[torch.Tensor] = None, size=None,
                       heads: int = 1, concat: bool = True, negative_slope: float = 0.2, relu: bool = False,
                       schedule: Schedule = DEFAULT, shared: bool = False, dropout: Optional[AttentionDropout] = None):
    """PyG 1.4.2 ``GATConv.forward((x_src, x_dst), edge_index, size)``: attention over the edge list AS IT IS (with ``size`` given
    PyG neither removes nor adds self loops), ``edge_index[0]`` indexing ``x_src`` and ``edge_index[1]`` the ``N_dst`` output rows.
    ``x_dst`` None: the score has no target term and ``att[..., :C]`` gets a zero gradient.  ``shared``: ``x_dst`` is ``x_src``
    itself (a tensor ``x`` with ``size=(N, N)``): projected once.  A target without an in-edge gets ``bias`` (or 0).
    ``dropout``: an ``AttentionDropout(p, seed, draw)`` -- attention dropout in training mode under Rule D, inside the fused kernels
    (the shapes of ``gat_fused_shape`` with ``schedule.gat_fused_stats``; anything else is a ``NotImplementedError``: the pair form
    has no composed variant).  Gradients: ``x_src``, ``x_dst``, ``weight``, ``att``, ``bias``."""
    who = "gat_conv_bipartite"
    x_src, x_dst, n_src, n_dst = _pair_sizes(x, size, who, edge_index)
    if shared and (x_dst is not None and x_dst is not x_src or n_dst != n_src):
        raise ValueError(f"{who}: shared=True means x_dst is x_src (one table, size (N, N))")
    if isinstance(edge_index, (CSRGraph, GraphBatch)):
        _as_bipartite(edge_index, n_src, n_dst, who)
    if x_dst is not None and x_dst.size(1) != x_src.size(1):
        raise ValueError(f"{who}: x_src and x_dst share the weight matrix, so they must have the same width")
    if weight.size(0) != x_src.size(1) or weight.size(1) % int(heads) or att.numel() != 2 * weight.size(1):
        raise ValueError(f"{who}: weight must be [F_in, heads * out] and att [1, heads, 2 * out]")
    require_gpu(x_src, x_dst, weight, att, bias)
    if x_src.dtype != torch.float32 or weight.dtype != torch.float32 or (x_dst is not None and x_dst.dtype != torch.float32):
        raise NotImplementedError(f"{who}: the bipartite layers run on float32 features and weights (bf16 storage is not implemented "
                                  "for the pair form)")
    graph = _as_bipartite(edge_index, n_src, n_dst, who)
    if x_dst is x_src and x_dst is not None:
        shared = True
    x_src = _f32c(x_src, "x_src")
    x_dst = None if (shared or x_dst is None) else _f32c(x_dst, "x_dst")
    if dropout is not None:
        if not isinstance(dropout, AttentionDropout):
            raise TypeError(f"{who}: dropout is an AttentionDropout(p, seed, draw), got {type(dropout).__name__}")
        if not (gat_fused_shape(int(heads), weight.size(1) // int(heads)) and schedule.gat_fused_stats):
            raise NotImplementedError(f"{who}: attention dropout runs inside the fused kernels, which serve {_GAT_FUSED_SHAPES} "
                                      f"(with schedule.gat_fused_stats); got heads={int(heads)}, out={weight.size(1) // int(heads)}")
    fused_bias = bias if concat else None
    out = _GatBipartiteFn.apply(x_src, x_dst, weight, att, fused_bias, graph, heads, negative_slope, relu and concat, schedule, shared,
                                dropout)
    if concat:
        return out
    out = out.view(n_dst, int(heads), -1).mean(dim=1)
    out = out + bias if bias is not None else out
    return torch.relu(out) if relu else out


# ---------------------------------------------------------------------------------------------
# Link prediction: pair scores and the loss over them (PyG 1.4.2 ``InnerProductDecoder`` / ``GAE.recon_loss``).  The forward is ONE
# launch over the pair list as it is (``npi_pair_score``: no CSR, no sort); the backward is the aggregation the layers already
# use -- ``segsum`` over the sides of the pair list with ``d loss / d logit`` as per-entry weights -- so it has no float atomics
# and is bitwise reproducible, where autograd's ``index_add_`` of the torch composition is not.
PAIR_LOSSES = {"gae": NPI_PAIR_LOSS_GAE, "bce": NPI_PAIR_LOSS_BCE}
_PAIR_LIMIT = 2 ** 31 - 1


def _pair_tables(z, size, who: str):
    """``z``: a tensor ``[N, F]`` (one id space) or a pair ``(z_src, z_dst)``; ``(z_src, z_dst or None, n_src, n_dst)`` with
    ``z_dst`` None when both ends read ONE table (a pair of the same tensor included)"""
    if isinstance(z, torch.Tensor):
        z_src = z_dst = z
    elif isinstance(z, (tuple, list)) and len(z) == 2 and all(isinstance(t, torch.Tensor) for t in z):
        z_src, z_dst = z
    else:
        raise TypeError(f"{who}: z is a tensor [N, F] (one id space) or a pair (z_src, z_dst) of tensors")
    for t, name in ((z_src, "z_src"), (z_dst, "z_dst")):
        if t.dim() != 2 or t.size(1) < 1:
            raise ValueError(f"{who}: {name} must be a [rows, F] tensor with F >= 1 (got shape {tuple(t.shape)})")
    if z_src.size(1) != z_dst.size(1):
        raise ValueError(f"{who}: z_src has {z_src.size(1)} columns, z_dst {z_dst.size(1)}: an inner product needs equal widths")
    n_src, n_dst = int(z_src.size(0)), int(z_dst.size(0))
    if size is not None:
        if not isinstance(size, (tuple, list)) or len(size) != 2:
            raise ValueError(f"{who}: size must be a pair (n_src, n_dst)")
        if (int(size[0]), int(size[1])) != (n_src, n_dst):
            raise ValueError(f"{who}: size is {tuple(size)!r}, the tables have {(n_src, n_dst)} rows")
    if max(n_src, n_dst, z_src.size(1)) >= _PAIR_LIMIT:
        raise ValueError(f"{who}: table rows and width stay below 2^31 - 1")
    for t, name in ((z_src, "z_src"), (z_dst, "z_dst")):
        if t.dtype == torch.bfloat16:
            raise NotImplementedError(f"{who}: the pair scores run on float32 tables (bf16 storage is not implemented)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
    return z_src, (None if z_dst is z_src else z_dst), n_src, n_dst


class _PairList:
    """The ``M`` pairs of one call -- ``src``, ``dst`` contiguous LongTensors -- and, built only when a backward asks, the CSR sides
    its gradients are summed over: the caller's ``BipartiteGraph`` of the pairs when one was passed, else a side per request."""

    def __init__(self, edge_index, n_src: int, n_dst: int, who: str):
        self.graph = None
        if isinstance(edge_index, BipartiteGraph):
            if edge_index.size != (n_src, n_dst):
                raise ValueError(f"{who}: the BipartiteGraph of the pairs was built for size {edge_index.size}, the tables give "
                                 f"{(n_src, n_dst)}")
            self.graph, self.src, self.dst = edge_index, edge_index._src, edge_index._dst
        elif isinstance(edge_index, torch.Tensor):
            if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
                raise ValueError(f"{who}: the pairs are a LongTensor of shape [2, M] (got {edge_index.dtype} {tuple(edge_index.shape)})")
            self.src, self.dst = edge_index[0].contiguous(), edge_index[1].contiguous()
        else:
            raise TypeError(f"{who}: the pairs are the [2, M] LongTensor or a BipartiteGraph of it")
        self.n_src, self.n_dst, self.M = n_src, n_dst, int(self.src.numel())
        if self.M >= _PAIR_LIMIT:
            raise ValueError(f"{who}: more than 2^31 - 2 pairs in one call")
        self._sides = {}

    def side(self, which: str) -> CSRSide:
        """``"dst"``: pairs grouped by target over the source table; ``"src"``: by source over the target table; ``"both"``: one id
        space, both ends as keys (``graph.pair_list_side``)"""
        if which not in self._sides:
            g = self.graph
            if which == "dst":
                side = g.by_dst if g is not None else build_side(self.dst, self.src, self.n_dst, self.n_src, self_loops=False, drop_equal=False)
            elif which == "src":
                side = g.by_src if g is not None else build_side(self.src, self.dst, self.n_src, self.n_dst, self_loops=False, drop_equal=False)
            else:
                side = g.pair_side() if g is not None else pair_list_side(self.src, self.dst, self.n_src)
            self._sides[which] = side
        return self._sides[which]


def _pitched(t: torch.Tensor) -> torch.Tensor:
    """a table as the kernels take it: unit column stride, any row pitch >= F (a view of a wider buffer stays a view)"""
    return t if (t.stride(1) == 1 and t.stride(0) >= t.size(1)) else t.contiguous()


def _pair_score_launch(z_src, z_dst, pairs: _PairList, n_pos: int, mode: int, want_logits: bool, want_coef: bool, want_loss: bool):
    """one ``npi_pair_score`` launch (plus the one-workgroup sum of the partials when the loss is asked for): ``(logits, coef, loss)``"""
    dev = require_gpu(z_src, z_dst, pairs.src, pairs.dst)
    z_src = _pitched(z_src)
    z_dst = z_src if z_dst is None else _pitched(z_dst)
    M, lib = pairs.M, load()
    f32 = dict(dtype=torch.float32, device=dev)
    logits = torch.empty(M, **f32) if want_logits else None
    coef = torch.empty(M, **f32) if want_coef else None
    loss = torch.empty((), **f32) if want_loss else None
    ws = torch.empty(int(lib.npi_pair_score_workspace_bytes(M)), dtype=torch.uint8, device=dev) if want_loss else None
    if M == 0 and not want_loss:
        return logits, coef, loss                              # empty outputs (null pointers to the library): nothing to launch
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.npi_pair_score(ptr(pairs.src), ptr(pairs.dst), M, int(n_pos), ptr(z_src), z_src.stride(0), pairs.n_src, ptr(z_dst),
                             z_dst.stride(0), pairs.n_dst, z_src.size(1), mode, ptr(logits), ptr(coef), ptr(loss), ptr(ws),
                             0 if ws is None else int(ws.numel()), ptr(status), stream_ptr(dev)), "npi_pair_score")
    note_status(status)
    return logits, coef, loss


def _side_weights(side: CSRSide, g: torch.Tensor) -> torch.Tensor:
    """per-pair values ``g`` (indexed by ``eid``) in the entry order of ``side``"""
    we = torch.empty(max(side.nnz_max, 1), dtype=torch.float32, device=g.device)
    check(load().npi_entry_weights(ptr(side.eid), ptr(side.rowidx), ptr(side.rowptr), ptr(g), 0, 1.0, side.n_rows, side.nnz_max, ptr(we),
                                   stream_ptr(g.device)), "npi_entry_weights")
    return we


def _pair_grads(pairs: _PairList, z_src, z_dst, g: torch.Tensor, want_src: bool, want_dst: bool):
    """``(dZ_src, dZ_dst)`` for ``d loss / d logit = g [M]``: ``dZ_dst[j] = sum_{m: dst_m = j} g_m z_src[src_m]`` over the by-target
    side, ``dZ_src[i] = sum_{m: src_m = i} g_m z_dst[dst_m]`` over the by-source side -- only the sides asked for are built -- or, with
    ONE table (``z_dst`` None), both terms in one segmented sum over ``pair_list_side`` (returned as ``dZ_src``)."""
    if pairs.M == 0:
        return (torch.zeros_like(z_src) if want_src else None,
                torch.zeros_like(z_dst) if (want_dst and z_dst is not None) else None)
    if z_dst is None:
        side = pairs.side("both")
        return segsum(None, side, _pitched(z_src), w=_side_weights(side, torch.cat([g, g]))), None
    d_src = d_dst = None
    if want_dst:
        side = pairs.side("dst")
        d_dst = segsum(None, side, _pitched(z_src), w=_side_weights(side, g))
    if want_src:
        side = pairs.side("src")
        d_src = segsum(None, side, _pitched(z_dst), w=_side_weights(side, g))
    return d_src, d_dst


class _PairScoreFn(torch.autograd.Function):
    """``logits[m] = <z_src[src_m], z_dst[dst_m]>`` (``z_dst`` None: one table) under an arbitrary upstream ``d logits``"""

    @staticmethod
    def forward(ctx, z_src, z_dst, pairs: _PairList):
        logits = _pair_score_launch(z_src, z_dst, pairs, pairs.M, NPI_PAIR_LOGITS, True, False, False)[0]
        ctx.pairs = pairs
        ctx.save_for_backward(z_src, z_dst)
        return logits

    @staticmethod
    def backward(ctx, grad):
        z_src, z_dst = ctx.saved_tensors
        d_src, d_dst = _pair_grads(ctx.pairs, z_src, z_dst, _f32c(grad, "grad"), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d_src, d_dst, None


class _LinkLossFn(torch.autograd.Function):
    """the scalar loss of ``npi_pair_score`` over ``cat([pos, neg], 1)``; ``coef = d loss / d logit`` comes out of the same launch and
    is all the backward keeps of it (no logits are written)"""

    @staticmethod
    def forward(ctx, z_src, z_dst, pairs: _PairList, n_pos: int, mode: int):
        want_coef = any(ctx.needs_input_grad[:2])
        _, coef, loss = _pair_score_launch(z_src, z_dst, pairs, n_pos, mode, False, want_coef, True)
        ctx.pairs, ctx.coef = pairs, coef
        ctx.save_for_backward(z_src, z_dst)
        return loss

    @staticmethod
    def backward(ctx, grad):
        z_src, z_dst = ctx.saved_tensors
        g = ctx.coef * grad.to(torch.float32)
        d_src, d_dst = _pair_grads(ctx.pairs, z_src, z_dst, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d_src, d_dst, None, None, None


def pair_scores(z, edge_index, size=None) -> torch.Tensor:
    """PyG 1.4.2 ``InnerProductDecoder.forward(z, edge_index, sigmoid=False)``: ``logits[m] = <z_src[edge_index[0, m]],
    z_dst[edge_index[1, m]]>``, ``[M]`` float32.  ``z``: a tensor ``[N, F]`` (one id space) or a pair ``(z_src, z_dst)``
    (``edge_index[0]`` indexes ``z_src``, as everywhere in the bipartite form; ``size``, if given, must be their row counts).
    ``edge_index``: the ``[2, M]`` LongTensor, read in list order by ONE launch with no sort -- or a ``BipartiteGraph`` of it, whose
    sides the backward then uses instead of sorting the list itself.  Under ``torch.no_grad()`` nothing is built at all.

    Gradients: both tables, under any upstream gradient, each a deterministic segmented sum (bitwise reproducible; only the side
    of a table that requires grad is built).  An id outside its table gives logit 0 and is reported like a dropped edge
    (``graph.check_pending()`` raises ``IndexError``).  float32 only; CPU tensors raise ``NpiError``."""
    who = "pair_scores"
    z_src, z_dst, n_src, n_dst = _pair_tables(z, size, who)
    pairs = _PairList(edge_index, n_src, n_dst, who)
    require_gpu(z_src, z_dst, pairs.src)
    return _PairScoreFn.apply(z_src, z_dst, pairs)


def link_loss(z, pos_edge_index, neg_edge_index=None, loss: str = "gae", num_pos: Optional[int] = None) -> torch.Tensor:
    """The link-prediction loss of the positives ``pos_edge_index [2, P]`` and the negatives ``neg_edge_index [2, Q]`` as a scalar,
    in ONE forward launch that writes no logits:

    ``loss="gae"``: PyG 1.4.2 ``GAE.recon_loss`` -- ``-log(sigmoid(x) + 1e-15).mean()`` over the positives plus
    ``-log(1 - sigmoid(x) + 1e-15).mean()`` over the negatives, in float32 as PyG evaluates it.  A part without a pair adds 0
    (PyG's ``mean()`` of an empty tensor is NaN).
    ``loss="bce"``: ``binary_cross_entropy_with_logits(x, labels)`` with the mean over all ``P + Q`` pairs, in the stable form --
    finite and accurate at any logit.

    ``z`` as in ``pair_scores``.  A ``BipartiteGraph`` of ``torch.cat([pos, neg], 1)`` may stand in place of ``pos_edge_index``
    (then ``neg_edge_index`` is None and ``num_pos`` says how many leading pairs are positives): the backward uses its sides.
    Gradients: both tables, ``d loss / d logit`` from the forward launch times the upstream gradient as the per-entry weights of
    the aggregation -- no float atomics, bitwise reproducible."""
    who = "link_loss"
    if loss not in PAIR_LOSSES:
        raise ValueError(f"{who}: loss is 'gae' or 'bce', got {loss!r}")
    z_src, z_dst, n_src, n_dst = _pair_tables(z, None, who)
    if isinstance(pos_edge_index, BipartiteGraph):
        if neg_edge_index is not None or num_pos is None:
            raise ValueError(f"{who}: a BipartiteGraph holds cat([pos, neg], 1); pass neg_edge_index=None and num_pos")
        pairs = _PairList(pos_edge_index, n_src, n_dst, who)
        n_pos = int(num_pos)
        if n_pos < 0 or n_pos > pairs.M:
            raise ValueError(f"{who}: num_pos must lie in [0, {pairs.M}], got {num_pos}")
    else:
        if num_pos is not None:
            raise ValueError(f"{who}: num_pos belongs to the BipartiteGraph form; with tensors the positives are pos_edge_index")
        for t, name in ((pos_edge_index, "pos_edge_index"), (neg_edge_index, "neg_edge_index")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who}: {name} must be a LongTensor of shape [2, M]")
            if t.dtype != torch.int64 or t.dim() != 2 or t.size(0) != 2:
                raise ValueError(f"{who}: {name} must be a LongTensor of shape [2, M] (got {t.dtype} {tuple(t.shape)})")
        require_gpu(z_src, z_dst, pos_edge_index, neg_edge_index)
        n_pos = int(pos_edge_index.size(1))
        pairs = _PairList(torch.cat([pos_edge_index, neg_edge_index], 1), n_src, n_dst, who)
    require_gpu(z_src, z_dst, pairs.src)
    return _LinkLossFn.apply(z_src, z_dst, pairs, n_pos, PAIR_LOSSES[loss])


# ---- ranking losses over corrupted targets (``csrc/group_score.hip``) ------------------------------------------------
# Rule G (``include/npi_gnn.h``): every positive ``(i, j)`` with its own ``K`` corrupted targets -- ``NegativeSampler.corrupt``,
# ``structured_negative_sampling`` or the ids of ``topk_links`` -- is one GROUP of ``1 + K`` slots that share the source row.  ONE
# forward launch scores the groups from ``pos_edge_index`` and ``neg_dst`` as they are and reduces them to BPR, a margin hinge or the
# sampled softmax; the expanded pair list exists only in the backward, which is ``_pair_grads`` over it.
GROUP_LOSSES = {"bpr": NPI_GROUP_LOSS_BPR, "margin": NPI_GROUP_LOSS_MARGIN, "softmax": NPI_GROUP_LOSS_SOFTMAX}
GROUP_MAX_K = 63


class _GroupList:
    """The ``P`` groups of one call: ``src``, ``dst`` contiguous ``[P]`` LongTensors, ``neg`` ``[P, K]`` with unit column stride and
    row pitch ``ld_neg`` (a view of a wider buffer stays a view), and -- built only when a backward asks -- the expanded
    ``_PairList`` of the ``P (1 + K)`` slots in slot order, empty and bad slots clamped into the tables (they carry weight 0)."""

    def __init__(self, pos_edge_index, neg_dst, n_src: int, n_dst: int, who: str):
        if not isinstance(pos_edge_index, torch.Tensor) or not isinstance(neg_dst, torch.Tensor):
            raise TypeError(f"{who}: pos_edge_index is a LongTensor of shape [2, P], neg_dst one of shape [P, K] (or [P])")
        if pos_edge_index.dtype != torch.int64 or pos_edge_index.dim() != 2 or pos_edge_index.size(0) != 2:
            raise ValueError(f"{who}: pos_edge_index must be a LongTensor of shape [2, P] (got {pos_edge_index.dtype} "
                             f"{tuple(pos_edge_index.shape)})")
        P = int(pos_edge_index.size(1))
        if neg_dst.dtype != torch.int64 or neg_dst.dim() not in (1, 2) or neg_dst.size(0) != P:
            raise ValueError(f"{who}: neg_dst must be a LongTensor of shape [P, K] or [P] with P = {P} (got {neg_dst.dtype} "
                             f"{tuple(neg_dst.shape)})")
        if neg_dst.dim() == 1:
            neg_dst = neg_dst[:, None]
        K = int(neg_dst.size(1))
        if K > GROUP_MAX_K:
            raise ValueError(f"{who}: at most {GROUP_MAX_K} corrupted targets per positive (got K = {K})")
        if P * (1 + K) >= _PAIR_LIMIT:
            raise ValueError(f"{who}: more than 2^31 - 2 slots in one call")
        if K == 0:
            ld = 0
        elif (K == 1 or neg_dst.stride(1) == 1) and (P <= 1 or neg_dst.stride(0) >= K):
            ld = int(neg_dst.stride(0)) if P > 1 else K
        else:
            neg_dst, ld = neg_dst.contiguous(), K
        self.src, self.dst, self.neg, self.ld_neg = pos_edge_index[0].contiguous(), pos_edge_index[1].contiguous(), neg_dst, ld
        self.n_src, self.n_dst, self.P, self.K = n_src, n_dst, P, K
        self._pairs = None

    def targets(self) -> torch.Tensor:
        """``[P, 1 + K]``: the positive's target, then the corrupted ones"""
        return torch.cat([self.dst[:, None], self.neg], 1)

    def valid(self) -> torch.Tensor:
        """``[P, 1 + K]`` bool: the slots that read rows (Rule G: neither empty nor bad, in a group that is not dropped)"""
        tgt = self.targets()
        keep = (self.src >= 0) & (self.src < self.n_src) & (self.dst >= 0) & (self.dst < self.n_dst)
        return keep[:, None] & (tgt >= 0) & (tgt < self.n_dst)

    def pairs(self) -> _PairList:
        if self._pairs is None:
            C = 1 + self.K
            src = self.src.repeat_interleave(C).clamp(min=0, max=max(self.n_src - 1, 0))
            tgt = self.targets().clamp(min=0, max=max(self.n_dst - 1, 0)).flatten()
            self._pairs = _PairList(torch.stack([src, tgt]), self.n_src, self.n_dst, "ranking_loss")
        return self._pairs


def _group_score_launch(z_src, z_dst, groups: _GroupList, mode: int, margin: float, scale: float, want_logits: bool, want_coef: bool,
                        want_loss: bool):
    """one ``npi_group_score`` launch (plus the one-workgroup sum of the partials when the loss is asked for): ``(logits, coef,
    loss)``, the first two ``[P, 1 + K]``"""
    dev = require_gpu(z_src, z_dst, groups.src, groups.dst, groups.neg)
    z_src = _pitched(z_src)
    z_dst = z_src if z_dst is None else _pitched(z_dst)
    P, K, lib = groups.P, groups.K, load()
    f32 = dict(dtype=torch.float32, device=dev)
    logits = torch.empty((P, 1 + K), **f32) if want_logits else None
    coef = torch.empty((P, 1 + K), **f32) if want_coef else None
    loss = torch.empty((), **f32) if want_loss else None
    ws = torch.empty(int(lib.npi_group_score_workspace_bytes(P, K)), dtype=torch.uint8, device=dev) if want_loss else None
    if P == 0 and not want_loss:
        return logits, coef, loss                              # empty outputs (null pointers to the library): nothing to launch
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.npi_group_score(ptr(groups.src), ptr(groups.dst), P, ptr(groups.neg) if K else 0, groups.ld_neg, K, ptr(z_src),
                              z_src.stride(0), groups.n_src, ptr(z_dst), z_dst.stride(0), groups.n_dst, z_src.size(1), mode,
                              float(margin), float(scale), ptr(logits), ptr(coef), ptr(loss), ptr(ws),
                              0 if ws is None else int(ws.numel()), ptr(status), stream_ptr(dev)), "npi_group_score")
    note_status(status)
    return logits, coef, loss


class _GroupScoreFn(torch.autograd.Function):
    """``logits[p, c]`` of Rule G under an arbitrary upstream ``d logits`` (ignored at empty, bad and dropped slots)"""

    @staticmethod
    def forward(ctx, z_src, z_dst, groups: _GroupList):
        logits = _group_score_launch(z_src, z_dst, groups, NPI_GROUP_LOGITS, 0.0, 1.0, True, False, False)[0]
        ctx.groups = groups
        ctx.save_for_backward(z_src, z_dst)
        return logits

    @staticmethod
    def backward(ctx, grad):
        z_src, z_dst = ctx.saved_tensors
        groups = ctx.groups
        g = torch.where(groups.valid(), grad.to(torch.float32), torch.zeros((), dtype=torch.float32, device=grad.device)).flatten()
        d_src, d_dst = _pair_grads(groups.pairs(), z_src, z_dst, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d_src, d_dst, None


class _RankingLossFn(torch.autograd.Function):
    """the scalar loss of ``npi_group_score``; ``coef = d loss / d logit`` ``[P, 1 + K]`` comes out of the same launch and is all the
    backward keeps of it (no logits are written).  Empty, bad and dropped slots hold coefficient exactly 0."""

    @staticmethod
    def forward(ctx, z_src, z_dst, groups: _GroupList, mode: int, margin: float, scale: float):
        want_coef = any(ctx.needs_input_grad[:2])
        _, coef, loss = _group_score_launch(z_src, z_dst, groups, mode, margin, scale, False, want_coef, True)
        ctx.groups, ctx.coef = groups, coef
        ctx.save_for_backward(z_src, z_dst)
        return loss

    @staticmethod
    def backward(ctx, grad):
        z_src, z_dst = ctx.saved_tensors
        g = (ctx.coef * grad.to(torch.float32)).flatten()
        d_src, d_dst = _pair_grads(ctx.groups.pairs(), z_src, z_dst, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d_src, d_dst, None, None, None, None


def group_scores(z, pos_edge_index, neg_dst) -> torch.Tensor:
    """The logits of every positive and of its own corrupted targets, ``[P, 1 + K]`` float32 (Rule G, ``npi_group_score``): column 0
    is ``<z_src[i], z_dst[j]>`` of the positive ``(i, j) = pos_edge_index[:, p]``, column ``c`` that of ``(i, neg_dst[p, c - 1])``.
    ``z`` as in ``pair_scores``; ``neg_dst``: ``[P, K]`` int64, ``0 <= K <= 63`` (``[P]`` means ``K = 1``) -- what
    ``NegativeSampler.corrupt``, ``structured_negative_sampling`` or ``topk_links`` return; a row-pitched view stays a view.  A slot
    holding ``-1`` is empty: ``-inf``, nothing read, nothing reported.  Any other id outside the target table gives ``-inf`` too and
    is reported (``graph.check_pending()`` raises ``IndexError``); a positive with an id out of range drops its group: all zeros,
    reported.  ONE launch that reads each source row once per batch of eight slots, not once per slot.

    Gradients: both tables, under any upstream gradient; the upstream value at an empty, bad or dropped slot is ignored.  The
    backward is ``pair_scores``' (segmented sums over the expanded list, built there only): no float atomics, bitwise reproducible."""
    who = "group_scores"
    z_src, z_dst, n_src, n_dst = _pair_tables(z, None, who)
    groups = _GroupList(pos_edge_index, neg_dst, n_src, n_dst, who)
    require_gpu(z_src, z_dst, groups.src, groups.neg)
    return _GroupScoreFn.apply(z_src, z_dst, groups)


def ranking_loss(z, pos_edge_index, neg_dst, loss: str = "bpr", margin: float = 1.0, scale: float = 1.0) -> torch.Tensor:
    """A ranking loss of the positives ``pos_edge_index [2, P]`` against their own corrupted targets ``neg_dst [P, K]`` as a 0-d
    float32, in ONE forward launch that writes no logits.  With ``d_c = scale * (x_c - x_0)`` over the valid corrupted slots of a
    group (``x`` as in ``group_scores``):

    ``loss="bpr"``: ``softplus(d_c)`` -- ``-logsigmoid(scale * (x_pos - x_neg))`` --, summed and divided by ``P K``.
    ``loss="margin"``: ``max(0, margin + d_c)``, divided by ``P K``; the derivative at the kink is 0.
    ``loss="softmax"``: the sampled softmax / InfoNCE ``-log softmax(scale * x)[0]`` over the group's valid slots, divided by ``P``.

    The divisors count slots, not valid slots (no device count is read back, so the forward may sit in a stream capture): an empty
    (``-1``) slot adds 0 where masking followed by ``mean()`` would shrink the divisor.  ``K = 0``, a group without a valid
    corrupted target, and ``P = 0`` give 0.  ``margin`` is read by ``"margin"`` only.  Gradients: both tables, ``d loss / d
    logit`` from the forward launch times the upstream gradient as the per-entry weights of the layers' own aggregation over the
    expanded list -- no float atomics, bitwise reproducible; only the side of a table that requires grad is built, and under
    ``torch.no_grad()`` nothing is."""
    who = "ranking_loss"
    if loss not in GROUP_LOSSES:
        raise ValueError(f"{who}: loss is 'bpr', 'margin' or 'softmax', got {loss!r}")
    margin, scale = float(margin), float(scale)
    if margin != margin or scale != scale or abs(margin) == float("inf") or abs(scale) == float("inf") or scale <= 0:
        raise ValueError(f"{who}: margin and scale must be finite and scale > 0 (got margin={margin}, scale={scale})")
    z_src, z_dst, n_src, n_dst = _pair_tables(z, None, who)
    groups = _GroupList(pos_edge_index, neg_dst, n_src, n_dst, who)
    require_gpu(z_src, z_dst, groups.src, groups.neg)
    return _RankingLossFn.apply(z_src, z_dst, groups, GROUP_LOSSES[loss], margin, scale)


# ---- VGAE: the seeded reparametrisation and the KL term (``csrc/gauss.hip``) ---------------------------------------
# PyG's ``mu + randn_like(logvar) * exp(0.5 * logvar)`` and ``-0.5 * mean(sum(1 + logvar - mu**2 - logvar.exp(), 1))`` in ONE launch
# forward and ONE backward.  The noise is Rule N, a pure function of ``(seed, draw, tick, table, row, column)`` that the backward
# recomputes -- as Rule D's mask is recomputed -- so no ``eps`` and no ``sigma`` tensor is saved; the KL term is a deterministic fp64
# sum (``npi_pair_score``'s scheme), so a VGAE step is bitwise reproducible.
@dataclass(frozen=True, eq=False)
class GaussianNoise:
    """The host side of Rule N (``include/npi_gnn.h``), the seeded standard normal: ``eps[row, column]`` of a table is a pure function
    of ``(seed, draw, tick, table, row, column)``.  ``tick``: None, or a one-element int64 DEVICE tensor that the kernels read -- the
    key travels by value, so a captured step replays the same draw; a caller that wants fresh noise on every replay of a HIP graph
    counts the word up inside the graph (``tick.add_(1)``)."""
    seed: int
    draw: int = 0
    tick: Optional[torch.Tensor] = None

    def __post_init__(self):
        for name in ("seed", "draw"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"GaussianNoise: {name} must be an int, got {v!r}")
        if self.draw < 0:
            raise ValueError(f"GaussianNoise: draw must be >= 0, got {self.draw!r}")
        t = self.tick
        if t is not None:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != 1:
                raise ValueError("GaussianNoise: tick is None or a one-element int64 device tensor")
            require_gpu(t)

    @property
    def key(self) -> int:
        """the ``key`` of the C ABI: ``epoch_seed(seed, draw)``, as every other seeded rule"""
        return epoch_seed(self.seed, self.draw)


def _gauss_table(table) -> int:
    if isinstance(table, bool) or table not in (0, 1):
        raise ValueError(f"table is 0 (one id space, or z_src) or 1 (z_dst), got {table!r}")
    return int(table)


def _gauss_rule(rule, who: str) -> GaussianNoise:
    if not isinstance(rule, GaussianNoise):
        raise TypeError(f"{who}: rule must be a GaussianNoise(seed, draw, tick), got {type(rule).__name__}")
    return rule


def gaussian_noise(N: int, F: int, rule: GaussianNoise, table: int = 0, device=None) -> torch.Tensor:
    """``eps [N, F]`` float32 of Rule N itself (``npi_gauss_noise``): what ``reparametrize_kl`` draws under the same ``rule`` and
    ``table``, for tests and for variants composed from torch operations.  ``device``: where to write (default: the tick's, else
    ``cuda``)."""
    who = "gaussian_noise"
    rule, table = _gauss_rule(rule, who), _gauss_table(table)
    for v, name in ((N, "N"), (F, "F")):
        if isinstance(v, bool) or not isinstance(v, int) or v < (1 if name == "F" else 0) or v >= _PAIR_LIMIT:
            raise ValueError(f"{who}: {name} is an int in [{1 if name == 'F' else 0}, 2^31 - 1), got {v!r}")
    dev = torch.device(device) if device is not None else (torch.device("cuda") if rule.tick is None else rule.tick.device)
    eps = torch.empty((N, F), dtype=torch.float32, device=dev)
    require_gpu(eps, rule.tick)
    check(load().npi_gauss_noise(N, F, rule.key, ptr(rule.tick), table, ptr(eps), F, stream_ptr(eps.device)), "npi_gauss_noise")
    return eps


def _gauss_tables(mu, logvar, who: str):
    for t, name in ((mu, "mu"), (logvar, "logvar")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a tensor [N, F]")
        if t.dim() != 2 or t.size(1) < 1:
            raise ValueError(f"{who}: {name} must be a [N, F] tensor with F >= 1 (got shape {tuple(t.shape)})")
        if t.dtype == torch.bfloat16:
            raise NotImplementedError(f"{who}: float32 tables only (bf16 storage is not implemented)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
    if mu.shape != logvar.shape:
        raise ValueError(f"{who}: mu is {tuple(mu.shape)}, logvar {tuple(logvar.shape)}")
    if max(mu.size(0), mu.size(1)) >= _PAIR_LIMIT:
        raise ValueError(f"{who}: rows and width stay below 2^31 - 1")


class _ReparamKlFn(torch.autograd.Function):
    """``(z, kl)`` of one ``npi_gauss_sample_kl`` launch (``kl`` alone when ``sample`` is False).  The backward is one
    ``npi_gauss_sample_kl_bwd`` launch that regenerates the noise; it keeps ``mu``, ``logvar`` and a copy of the tick word, and an
    output nobody differentiates costs nothing in it."""

    @staticmethod
    def forward(ctx, mu, logvar, rule: Optional[GaussianNoise], table: int, n_total: int, max_logvar: float, sample: bool):
        tick = rule.tick if sample else None
        dev = require_gpu(mu, logvar, tick)
        mu_, lv_ = _pitched(mu), _pitched(logvar)
        N, F = int(mu.size(0)), int(mu.size(1))
        lib = load()
        z = torch.empty((N, F), dtype=torch.float32, device=dev) if sample else None
        kl = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib.npi_gauss_workspace_bytes(N, F)), dtype=torch.uint8, device=dev)
        key = rule.key if sample else 0
        flags = NPI_GAUSS_KL | (NPI_GAUSS_SAMPLE if sample else 0)
        check(lib.npi_gauss_sample_kl(ptr(mu_), mu_.stride(0), ptr(lv_), lv_.stride(0), N, F, n_total, max_logvar, key, ptr(tick), table,
                                      flags, ptr(z), F, ptr(kl), ptr(ws), int(ws.numel()), stream_ptr(dev)), "npi_gauss_sample_kl")
        # the backward redraws under the tick the forward saw, whatever the caller has counted since
        keep_tick = tick is not None and any(ctx.needs_input_grad[:2])
        ctx.call = (key, tick.clone() if keep_tick else None, table, n_total, max_logvar, sample)
        ctx.save_for_backward(mu_, lv_)
        ctx.set_materialize_grads(False)
        return (z, kl) if sample else kl

    @staticmethod
    def backward(ctx, *grads):
        key, tick, table, n_total, max_logvar, sample = ctx.call
        g_z, g_kl = grads if sample else (None, grads[0])
        want_mu, want_lv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_z is None and g_kl is None) or not (want_mu or want_lv):
            return (None,) * 7
        mu, logvar = ctx.saved_tensors
        N, F = int(mu.size(0)), int(mu.size(1))
        g_z = None if g_z is None else _pitched(g_z)
        g_kl = None if g_kl is None else g_kl.to(torch.float32).reshape(1)
        dev = mu.device
        # without a KL gradient d mu IS g_z: nothing to write
        d_mu = torch.empty((N, F), dtype=torch.float32, device=dev) if (want_mu and g_kl is not None) else None
        d_lv = torch.empty((N, F), dtype=torch.float32, device=dev) if want_lv else None
        if N > 0 and (d_mu is not None or d_lv is not None):
            flags = (NPI_GAUSS_SAMPLE if g_z is not None else 0) | (NPI_GAUSS_KL if g_kl is not None else 0)
            check(load().npi_gauss_sample_kl_bwd(ptr(mu), mu.stride(0), ptr(logvar), logvar.stride(0), N, F, n_total, max_logvar, key,
                                                 ptr(tick), table, flags, ptr(g_z), 0 if g_z is None else g_z.stride(0), ptr(g_kl),
                                                 ptr(d_mu), F, ptr(d_lv), F, stream_ptr(dev)), "npi_gauss_sample_kl_bwd")
        if want_mu and g_kl is None:
            d_mu = g_z
        return d_mu, d_lv, None, None, None, None, None


def reparametrize_kl(mu: torch.Tensor, logvar: torch.Tensor, rule: Optional[GaussianNoise] = None, table: int = 0,
                     n_total: Optional[int] = None, max_logvar: float = 10.0, sample: bool = True):
    """PyG 1.4.2 ``VGAE.reparametrize`` and ``VGAE.kl_loss`` in one launch: ``(z, kl)`` with ``lv = min(logvar, max_logvar)``,

    ``z = mu + eps * exp(0.5 * lv)`` -- ``eps`` Rule N under ``rule`` (a ``GaussianNoise``) and ``table`` (0: one id space or the source
    table, 1: the target table of a pair) -- and ``kl = -0.5 / n_total * sum(1 + lv - mu**2 - exp(lv))``, a 0-d float32 tensor;
    ``n_total``: the node count of the mean (default ``N``; ``n_src + n_dst`` when the call is one table of a pair).
    ``sample=False`` (evaluation): ``z`` is ``mu`` itself, nothing is drawn (``rule`` may be None) and the launch computes ``kl`` only.

    ``mu`` / ``logvar`` may be column blocks of one wider tensor (``h[:, :F]``, ``h[:, F:]`` of an encoder with ONE aggregation for
    both heads): they are read in place.  Gradients: both inputs under any upstream ``(d z, d kl)``, one launch that regenerates
    ``eps``; an output that is not differentiated costs nothing, and without a ``kl`` gradient ``d mu`` is ``d z`` itself.  A clamped
    entry (``logvar > max_logvar``) gets ``d logvar = 0``, as ``clamp(max=)`` gives.  float32 only; CPU tensors raise ``NpiError``."""
    who = "reparametrize_kl"
    _gauss_tables(mu, logvar, who)
    table = _gauss_table(table)
    if sample:
        rule = _gauss_rule(rule, who)
    N = int(mu.size(0))
    n_total = N if n_total is None else n_total
    if isinstance(n_total, bool) or not isinstance(n_total, int) or n_total < N or n_total >= _PAIR_LIMIT:
        raise ValueError(f"{who}: n_total is an int in [N, 2^31 - 1), got {n_total!r}")
    if isinstance(max_logvar, bool) or not isinstance(max_logvar, (int, float)) or max_logvar != max_logvar:
        raise ValueError(f"{who}: max_logvar must be a number, got {max_logvar!r}")
    require_gpu(mu, logvar, rule.tick if sample else None)
    out = _ReparamKlFn.apply(mu, logvar, rule, table, max(n_total, 1), float(max_logvar), bool(sample))
    return out if sample else (mu, out)
