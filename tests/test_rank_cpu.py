"""Ranking metrics without a GPU: the restatement ``tests/_rank_ref.py`` of Rule R against the brute-force pairwise definition of
``U2``, the literal precision / recall sum and sklearn; the new C-ABI symbols; the argument errors of ``npi_rank_metrics`` and of
the Python layer."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
import _rank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_rank_metrics", "npi_rank_workspace_bytes")
CASES = [(name, M) for name in ref.FAMILIES for M in (1, 2, 7, 65, 300)]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _cmp(a, b):
    """a > b, a == b as numbers (sklearn's comparison: -0.0 == 0.0)"""
    return np.greater.outer(a, b), np.equal.outer(a, b)


@pytest.mark.parametrize("name,M", CASES)
def test_restatement_equals_the_pairwise_definition_and_the_literal_ap_sum(name, M):
    for kind in ("30", "P1", "N1", "P0", "N0"):
        s, y = ref.family(name, M), ref.labels(M, kind)
        r = ref.evaluate(s, y)
        pos, neg = s[y == 1].astype(np.float64), s[y == 0].astype(np.float64)
        gt, eq = _cmp(pos, neg)
        assert r["U2"] == 2 * int(gt.sum()) + int(eq.sum()), (name, M, kind)
        assert (r["P"], r["N"]) == (pos.size, neg.size) and r["G"] == np.unique(s.astype(np.float64)).size
        assert np.all(np.diff(r["thr"].astype(np.float64)) < 0)                   # strictly descending, one per distinct score
        if pos.size and neg.size:
            assert r["auc"] == r["U2"] / (2.0 * pos.size * neg.size) and 0.0 <= r["auc"] <= 1.0
        else:
            assert math.isnan(r["auc"])
        # AP literally: at every distinct score t (descending), precision and recall of "score >= t"; sum of recall steps x precision
        if pos.size:
            ap, prev = 0.0, 0.0
            for t in np.unique(s.astype(np.float64))[::-1]:
                tp, fp = int((pos >= t).sum()), int((neg >= t).sum())
                ap += (tp / pos.size - prev) * (tp / (tp + fp))
                prev = tp / pos.size
            assert abs(r["ap"] - ap) <= 1e-12, (name, M, kind)
        else:
            assert math.isnan(r["ap"])
    if name == "equal":
        assert ref.evaluate(ref.family(name, M), ref.labels(M, "30"))["G"] == 1
    # the n_pos form is the y form of arange < n_pos, and a permutation changes nothing
    s = ref.family(name, M)
    a, b = ref.evaluate(s, n_pos=M // 3), ref.evaluate(s, (np.arange(M) < M // 3).astype(np.int64))
    perm = np.random.default_rng(M).permutation(M)
    c = ref.evaluate(s[perm], (np.arange(M) < M // 3).astype(np.int64)[perm])
    for k in ("P", "N", "G", "U2"):
        assert a[k] == b[k] == c[k]
    for k in ("thr", "tps", "fps"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()


def test_key_transform_orders_like_the_numbers_and_inverts_bitwise():
    s = ref.family("special", 200)
    k = ref.keys_of(s)
    back = ref.scores_of(k)
    want = (s + np.float32(0.0)).astype(np.float32)
    assert back.tobytes() == want.tobytes() and not np.signbit(back[s == 0]).any()
    gt, eq = _cmp(s.astype(np.float64), s.astype(np.float64))
    assert np.array_equal(np.less.outer(k, k), gt) and np.array_equal(np.equal.outer(k, k), eq)


@pytest.mark.parametrize("name,M", [c for c in CASES if c[1] >= 7])
def test_restatement_equals_sklearn(name, M):
    skm = pytest.importorskip("sklearn.metrics")
    s, y = ref.family(name, M), ref.labels(M, "30", seed=3)
    s, y = s[np.isfinite(s)], y[np.isfinite(s)]                                   # sklearn refuses +-inf scores; Rule R ranks them
    if y.min() == y.max():
        y[0] = 1 - y[0]
    r = ref.evaluate(s, y)
    assert abs(r["auc"] - skm.roc_auc_score(y, s)) <= 1e-12
    assert abs(r["ap"] - skm.average_precision_score(y, s)) <= 1e-12
    fpr, tpr, thr = skm.roc_curve(y, s, drop_intermediate=False)
    mine = ref.roc_curve(r)
    assert np.array_equal(mine[0], fpr) and np.array_equal(mine[1], tpr)
    assert np.array_equal(mine[2].astype(np.float64), thr.astype(np.float64))     # (numeric: sklearn keeps -0.0 where it met it)
    precision, recall, thr = skm.precision_recall_curve(y, s)
    mine = ref.precision_recall_curve(r)
    assert np.array_equal(mine[0], precision) and np.array_equal(mine[1], recall)
    assert np.array_equal(mine[2].astype(np.float64), thr.astype(np.float64))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("#define NPI_STATUS_BAD_SCORE 1024", "#define NPI_STATUS_BAD_LABEL 2048", "RULE R", "_binary_clf_curve",
                 "roc_auc_score", "average_precision_score", "GAE.test"):
        assert word in header, word
    assert (_lib.NPI_STATUS_BAD_SCORE, _lib.NPI_STATUS_BAD_LABEL) == (1024, 2048)
    assert _lib.NPI_STATUS_BAD_SCORE == 2 * _lib.NPI_STATUS_WALK_TRIES                   # the next free bits
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "rank.hip" in SOURCES and "rank.hip" not in HOST_ONLY
    for name in ("rank_metrics", "roc_auc_score", "average_precision_score", "roc_curve", "precision_recall_curve"):
        assert name in npi.__all__ and hasattr(npi, name), name
    assert callable(npi.GAE.test)


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG, P = None, 2 ** 31 - 1, 16                # P: a non-null, 16-byte aligned stand-in for a device pointer (never read)
    ws = lib.npi_rank_workspace_bytes(100)

    def call(scores=P, y=P, M=100, n_pos=0, result=P, counts=P, thr=P, tps=P, fps=P, status=N, work=P, nbytes=ws):
        return lib.npi_rank_metrics(scores, y, M, n_pos, result, counts, thr, tps, fps, status, work, nbytes, N)

    calls = {
        "null scores": dict(scores=N), "null result": dict(result=N), "null counts": dict(counts=N), "null workspace": dict(work=N),
        "negative M": dict(M=-1), "M 2^31 - 1": dict(M=BIG, nbytes=2 ** 44),
        "negative n_pos": dict(y=N, n_pos=-1), "n_pos above M": dict(y=N, n_pos=101),
        "curve without thr": dict(thr=N), "curve without tps": dict(tps=N), "curve without fps": dict(fps=N),
        "only thr": dict(tps=N, fps=N), "only tps": dict(thr=N, fps=N), "only fps": dict(thr=N, tps=N),
        "short workspace": dict(nbytes=ws - 1), "misaligned workspace": dict(work=24), "negative workspace size": dict(nbytes=-1),
        "null result, no example": dict(M=0, result=N), "partial curve, no example": dict(M=0, thr=N),
    }
    for name, kw in calls.items():
        assert call(**kw) == -1, name
        assert b"npi_rank_metrics" in lib.npi_last_error(), (name, lib.npi_last_error())
    assert lib.npi_rank_workspace_bytes(-1) == -1 and lib.npi_rank_workspace_bytes(BIG) == -1
    assert lib.npi_rank_workspace_bytes(0) > 0 and lib.npi_rank_workspace_bytes(0) % 16 == 0
    assert ws % 16 == 0 and lib.npi_rank_workspace_bytes(BIG - 1) > 16 * (BIG - 1)
    # four words per score for the sorter, and three 8-byte words per 1,024 scores behind them
    assert lib.npi_rank_workspace_bytes(2 ** 20) >= 16 * 2 ** 20 + 3 * 8 * 2 ** 10
    assert lib.npi_rank_workspace_bytes(2 ** 20 + 1) >= lib.npi_rank_workspace_bytes(2 ** 20)


# ---- the Python layer: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_function_argument_errors_and_no_cpu_fallback():
    s, y = torch.rand(10), (torch.arange(10) % 2)
    # CPU tensors and the wrong dtype: no CPU path, no bf16 / fp64 form
    for call in (lambda: npi.rank_metrics(s, y), lambda: npi.rank_metrics(s, n_pos=3), lambda: npi.roc_auc_score(y, s),
                 lambda: npi.average_precision_score(y, s), lambda: npi.roc_curve(y, s), lambda: npi.precision_recall_curve(y, s),
                 lambda: npi.rank_metrics(s.double(), y), lambda: npi.rank_metrics(s.bfloat16(), n_pos=3),
                 lambda: npi.rank_metrics(y, y)):
        with pytest.raises(npi.NpiError):
            call()
    with pytest.raises(TypeError):
        npi.rank_metrics([0.1, 0.2], n_pos=1)
    with pytest.raises(ValueError, match="neither"):
        npi.rank_metrics(s)
    with pytest.raises(ValueError, match="both"):
        npi.rank_metrics(s, y, 3)
    model = npi.GAE(torch.nn.Identity())
    with pytest.raises(npi.NpiError):
        model.test(torch.randn(6, 4), torch.tensor([[0, 1], [1, 2]]), torch.tensor([[0, 3], [4, 5]]))


def test_label_and_count_argument_errors(monkeypatch):
    """the checks behind the device check, reached with it stubbed out: nothing here gets as far as a launch"""
    from npi_gnn_amd import rank
    s = torch.rand(10)
    monkeypatch.setattr(rank, "_scores", lambda scores, what: scores)
    for bad in (-1, 11):
        with pytest.raises(ValueError, match="n_pos"):
            rank.rank_metrics(s, n_pos=bad)
    for bad in (3.0, True, "3"):
        with pytest.raises(TypeError, match="n_pos"):
            rank.rank_metrics(s, n_pos=bad)
    with pytest.raises(ValueError, match="integers"):
        rank.rank_metrics(s, torch.rand(10))
    with pytest.raises(ValueError, match="labels for"):
        rank.rank_metrics(s, torch.zeros(9, dtype=torch.long))
    with pytest.raises(TypeError, match="labels"):
        rank.rank_metrics(s, [0] * 10)
