"""Ranking metrics on the MI355X: ROC-AUC, average precision and the score curves of an evaluation, computed where the scores are::

    auc, ap = npi.rank_metrics(scores, y)                      # 0-d float64 device tensors, no host read
    auc, ap = npi.rank_metrics(scores, n_pos=P)                # the first P scores are the positives: cat([pos, neg])
    npi.roc_auc_score(y_true, y_score)                         # sklearn's names and argument order: Python floats, ONE host read
    npi.average_precision_score(y_true, y_score)
    fpr, tpr, thresholds = npi.roc_curve(y_true, y_score)                  # device tensors; ONE host read (the curve's length)
    precision, recall, thresholds = npi.precision_recall_curve(y_true, y_score)

PyG 1.4.2 ``GAE.test`` and the reference's ROC / PR figures (``src/compare_withKmer_noKmer.py:20-54``) copy the scores to the host
and call sklearn.  Here all of it is Rule R of ``include/npi_gnn.h`` (``npi_rank_metrics``): one device sort of the scores, two
passes over the sorted stream for sklearn's ``_binary_clf_curve`` -- thresholds, ``tps``, ``fps`` at the ends of the tie groups --
and one over that curve for the two areas.  ``auc`` is exact (an int64 count over a double product), ``ap`` a double sum in a fixed
order; both and the curve are bitwise the same for any permutation of the input.

Out of scope: sample weights, multiclass / ``average=``, ``drop_intermediate=True`` (the curves keep every threshold),
``max_fpr``, bf16 / fp64 scores.  Scores are float32 GPU tensors; anything else raises ``NpiError``: there is no CPU path.
"""
from __future__ import annotations

import struct
from typing import Optional, Tuple

import torch

from . import graph as _graph
from ._lib import NpiError, check, load, ptr, require_gpu, stream_ptr

_LIMIT = 2 ** 31 - 1            # M stays below it (include/npi_gnn.h)


def _scores(scores, what: str) -> torch.Tensor:
    if not isinstance(scores, torch.Tensor):
        raise TypeError(f"{what}: scores must be a tensor, got {type(scores).__name__}")
    if not scores.is_cuda or scores.dtype != torch.float32:
        raise NpiError(f"{what}: scores must be a float32 tensor on an MI355X (HIP); got {scores.dtype} on {scores.device}.  "
                       "There is no CPU path and no bf16 / fp64 form")
    if scores.dim() != 1:
        raise ValueError(f"{what}: scores must have shape [M], got {tuple(scores.shape)}")
    if scores.numel() >= _LIMIT:
        raise NpiError(f"{what}: more than 2^31 - 2 scores in one call")
    return scores.detach().contiguous()


def _labels(y, scores: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"{what}: labels must be a tensor, got {type(y).__name__}")
    if y.dtype.is_floating_point or y.dtype.is_complex:
        raise ValueError(f"{what}: labels must be integers (0 / 1) or booleans, got {y.dtype}")
    if y.shape != scores.shape:
        raise ValueError(f"{what}: {tuple(y.shape)} labels for {tuple(scores.shape)} scores")
    if require_gpu(y) != scores.device:
        raise NpiError(f"tensors on different devices: {scores.device} vs {y.device}")
    return y.to(torch.int64).contiguous()


def _run(scores, y, n_pos, curve: bool, what: str):
    """``npi_rank_metrics``: ``(result [2] f64, counts [4] i64, status [1] i32, (thr, tps, fps) or None)``, nothing read back"""
    if (y is None) == (n_pos is None):
        raise ValueError(f"{what}: give the labels y or the count n_pos (the first n_pos scores are the positives), not "
                         f"{'both' if y is not None else 'neither'}")
    scores = _scores(scores, what)
    M = int(scores.numel())
    if y is not None:
        y, n_pos = _labels(y, scores, what), 0
    else:
        if isinstance(n_pos, bool) or not isinstance(n_pos, int):
            raise TypeError(f"{what}: n_pos must be an int, got {type(n_pos).__name__}")
        if n_pos < 0 or n_pos > M:
            raise ValueError(f"{what}: n_pos must lie in [0, {M}], got {n_pos}")
    dev, lib = scores.device, load()
    result = torch.empty(2, dtype=torch.float64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(lib.npi_rank_workspace_bytes(M))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pts = None
    if curve:
        pts = (torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.int32, device=dev),
               torch.empty(M, dtype=torch.int32, device=dev))
    thr, tps, fps = pts if curve else (None, None, None)
    check(lib.npi_rank_metrics(ptr(scores), ptr(y), M, n_pos, ptr(result), ptr(counts), ptr(thr), ptr(tps), ptr(fps), ptr(status),
                               ptr(ws), nbytes, stream_ptr(dev)), "npi_rank_metrics")
    return result, counts, status, pts


def rank_metrics(scores: torch.Tensor, y: Optional[torch.Tensor] = None, n_pos: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(auc, ap)`` of float32 GPU ``scores`` ``[M]`` as 0-d float64 device tensors: ``roc_auc_score`` and
    ``average_precision_score`` of Rule R.  Labels: ``y`` ``[M]`` (0 / 1, any integer dtype or bool), or ``n_pos``: the first
    ``n_pos`` scores are the positives (``torch.cat([pos, neg])``).  No host read, so it may run inside a stream capture; a NaN
    score or a label other than 0 / 1 is reported through the status word (``graph.check_pending()`` raises).  ``auc`` is NaN
    without a positive or without a negative, ``ap`` without a positive."""
    result, _, status, _ = _run(scores, y, n_pos, False, "rank_metrics")
    _graph.note_status(status)
    return result[0], result[1]


def _read(dev, result, counts, status):
    """the ONE host read of the sklearn-named functions: ``(auc, ap, P, N, G)``; every pending status word rides along"""
    if torch.cuda.is_current_stream_capturing():
        raise NpiError("this function reads from the device and cannot run inside a stream capture; rank_metrics can")
    words = [result.view(torch.int64), counts, status.to(torch.int64)] + [t.to(torch.int64) for t in _graph.pending_status(dev)]
    vals = torch.cat(words).tolist()
    _graph.raise_on_status(vals[6:])
    auc, ap = struct.unpack("<2d", struct.pack("<2q", vals[0], vals[1]))
    return auc, ap, vals[2], vals[3], vals[4]


def roc_auc_score(y_true: torch.Tensor, y_score: torch.Tensor) -> float:
    """sklearn's ``roc_auc_score(y_true, y_score)`` for binary labels: a Python float from one host read.  ``ValueError`` as there
    for a NaN score and when only one class is present."""
    result, counts, status, _ = _run(y_score, y_true, None, False, "roc_auc_score")
    auc, _, P, N, _ = _read(y_score.device, result, counts, status)
    if P == 0 or N == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return auc


def average_precision_score(y_true: torch.Tensor, y_score: torch.Tensor) -> float:
    """sklearn's ``average_precision_score(y_true, y_score)`` for binary labels: a Python float from one host read (NaN without
    a positive, where sklearn warns and returns 0).  ``ValueError`` for a NaN score."""
    result, counts, status, _ = _run(y_score, y_true, None, False, "average_precision_score")
    return _read(y_score.device, result, counts, status)[1]


def roc_curve(y_true: torch.Tensor, y_score: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """sklearn's ``roc_curve(y_true, y_score, drop_intermediate=False)``: ``(fpr, tpr, thresholds)`` as device tensors of
    ``G + 1`` points (``G`` distinct scores; one host read for it), float64 rates and float32 thresholds, with the leading
    ``(0, 0)`` point at threshold ``inf``.  ``drop_intermediate`` is fixed at ``False``: every threshold is kept.  A rate without
    its class is NaN, as in sklearn."""
    result, counts, status, (thr, tps, fps) = _run(y_score, y_true, None, True, "roc_curve")
    _, _, _, _, G = _read(y_score.device, result, counts, status)
    zero = torch.zeros(1, dtype=torch.float64, device=thr.device)
    tp, fp = torch.cat([zero, tps[:G].double()]), torch.cat([zero, fps[:G].double()])
    thresholds = torch.cat([torch.full((1,), float("inf"), dtype=torch.float32, device=thr.device), thr[:G]])
    return fp / counts[1].double(), tp / counts[0].double(), thresholds          # 0 / 0 = NaN: the class is missing


def precision_recall_curve(y_true: torch.Tensor, y_score: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """sklearn's ``precision_recall_curve(y_true, y_score)`` (``drop_intermediate=False``): ``(precision, recall, thresholds)`` as
    device tensors, thresholds ascending (``G`` of them; one host read for it), precision and recall with the final ``(1, 0)``
    point behind them.  Without a positive recall is 1 at every threshold, as in sklearn."""
    result, counts, status, (thr, tps, fps) = _run(y_score, y_true, None, True, "precision_recall_curve")
    _, _, P, _, G = _read(y_score.device, result, counts, status)
    tp, fp = tps[:G].double(), fps[:G].double()
    precision = tp / (tp + fp)                                                      # tp + fp >= 1 at every group end
    recall = tp / counts[0].double() if P > 0 else torch.ones_like(tp)              # (a tensor divisor: a true division, not a reciprocal)
    one, zero = torch.ones(1, dtype=torch.float64, device=thr.device), torch.zeros(1, dtype=torch.float64, device=thr.device)
    return torch.cat([precision.flip(0), one]), torch.cat([recall.flip(0), zero]), thr[:G].flip(0)
