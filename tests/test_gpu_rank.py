"""``npi_rank_metrics`` on the MI355X against Rule R restated on the host (``tests/_rank_ref.py``): counts, ``tps`` / ``fps`` and
``U2`` integer-exact, thresholds bitwise, ``auc`` bitwise equal to ``U2 / (2.0 P N)``, ``ap`` within 1e-12 of the ``math.fsum`` of
the same fp64 terms (a fixed-tree fp64 sum of G <= 2^19 non-negative terms totalling at most 1 errs by about (log2 G + a few) *
2^-53, some 3e-15: the bar is that with margin)."""
import math

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import graph as NG
import _rank_ref as ref

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
SENTINEL = -7


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _call(dev, s, y=None, n_pos=None, curve=True):
    """the C entry point on host arrays; the curve buffers (capacity M) are pre-filled with a sentinel"""
    lib = _lib.load()
    M = int(s.size)
    sd = _t(s, dev)
    yd = None if y is None else _t(np.asarray(y, dtype=np.int64), dev)
    result = torch.full((2,), 123.0, dtype=torch.float64, device=dev)
    counts = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(lib.npi_rank_workspace_bytes(M))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    thr = torch.full((M,), float(SENTINEL), dtype=torch.float32, device=dev) if curve else None
    tps = torch.full((M,), SENTINEL, dtype=torch.int32, device=dev) if curve else None
    fps = torch.full((M,), SENTINEL, dtype=torch.int32, device=dev) if curve else None
    _lib.check(lib.npi_rank_metrics(_lib.ptr(sd), _lib.ptr(yd), M, 0 if n_pos is None else int(n_pos), _lib.ptr(result),
                                    _lib.ptr(counts), _lib.ptr(thr), _lib.ptr(tps), _lib.ptr(fps), _lib.ptr(status), _lib.ptr(ws),
                                    nbytes, _lib.stream_ptr(dev)), "npi_rank_metrics")
    out = {"result": result.cpu().numpy(), "counts": counts.cpu().numpy(), "status": int(status.item())}
    if curve:
        out.update(thr=thr.cpu().numpy(), tps=tps.cpu().numpy(), fps=fps.cpu().numpy())
    return out


def _same(a, b):
    """bitwise: NaN equals NaN"""
    return a.tobytes() == b.tobytes()


def _check(out, r, what):
    P, N, G, U2 = (int(v) for v in out["counts"])
    assert (P, N, G, U2) == (r["P"], r["N"], r["G"], r["U2"]), what
    assert out["status"] == 0, what
    auc, ap = (float(v) for v in out["result"])
    if P and N:
        assert auc == U2 / (2.0 * P * N) == r["auc"], (what, auc, r["auc"])
    else:
        assert math.isnan(auc), what
    if P:
        print(what, "ap", ap, "ref", r["ap"], "diff", abs(ap - r["ap"]))
        assert abs(ap - r["ap"]) <= AP_TOL, (what, ap, r["ap"])
    else:
        assert math.isnan(ap), what
    if "thr" in out:
        assert np.array_equal(out["tps"][:G], r["tps"]) and np.array_equal(out["fps"][:G], r["fps"]), what
        assert _same(out["thr"][:G], r["thr"]), what
        assert (out["tps"][G:] == SENTINEL).all() and (out["fps"][G:] == SENTINEL).all() and (out["thr"][G:] == SENTINEL).all(), what


@pytest.mark.parametrize("M", ref.SIZES)
def test_curve_counts_and_areas_equal_rule_r(dev, M):
    n_pos = min(M, max(0, round(0.3 * M)))
    for name in ref.FAMILIES:
        s, y = ref.family(name, M), ref.labels(M, "30")
        r = ref.evaluate(s, y)
        out = _call(dev, s, y=y)
        _check(out, r, (name, M, "y"))
        bare = _call(dev, s, y=y, curve=False)                                  # no curve written: the same numbers
        assert _same(bare["result"], out["result"]) and _same(bare["counts"], out["counts"]) and bare["status"] == 0
        _check(_call(dev, s, n_pos=n_pos), ref.evaluate(s, n_pos=n_pos), (name, M, "n_pos"))
        if name == "equal" and r["P"] and r["N"]:
            assert r["G"] == 1 and float(out["result"][0]) == 0.5
        if name == "distinct":
            assert r["G"] == M


@pytest.mark.parametrize("M", (1, 2, 65, 1025, 4097))
def test_one_or_no_example_of_a_class(dev, M):
    for name in ("distinct", "seven", "equal"):
        for kind in ("P1", "N1", "P0", "N0"):
            s, y = ref.family(name, M), ref.labels(M, kind)
            out = _call(dev, s, y=y)
            _check(out, ref.evaluate(s, y), (name, M, kind))
            P, N = int(out["counts"][0]), int(out["counts"][1])
            assert math.isnan(out["result"][0]) == (P == 0 or N == 0) and math.isnan(out["result"][1]) == (P == 0)
        for n_pos in (0, M):
            _check(_call(dev, s, n_pos=n_pos), ref.evaluate(s, n_pos=n_pos), (name, M, "n_pos", n_pos))


def test_no_example_at_all(dev):
    out = _call(dev, np.zeros(0, dtype=np.float32), n_pos=0)
    assert np.isnan(out["result"]).all() and (out["counts"] == 0).all() and out["status"] == 0
    out = _call(dev, np.zeros(0, dtype=np.float32), y=np.zeros(0, dtype=np.int64), curve=False)
    assert np.isnan(out["result"]).all() and (out["counts"] == 0).all()


@pytest.mark.parametrize("M", (4097, 64 * 4096 + 1))
def test_twice_and_permuted_are_bitwise_equal(dev, M):
    for name in ("seven", "sigmoid", "distinct", "straddle"):
        s, y = ref.family(name, M, seed=1), ref.labels(M, "30", seed=1)
        a, b = _call(dev, s, y=y), _call(dev, s, y=y)
        perm = np.random.default_rng(M).permutation(M)
        c = _call(dev, s[perm], y=y[perm])
        for k in ("result", "counts", "thr", "tps", "fps"):
            assert _same(a[k], b[k]) and _same(a[k], c[k]), (name, M, k)
        assert int(a["counts"][2]) == ref.evaluate(s, y)["G"]


def test_status_bits_and_nothing_written_past_the_curve(dev):
    for M in (5, 1025, 4097):
        s, y = ref.family("seven", M), ref.labels(M, "30")
        bad_s = s.copy()
        bad_s[M // 2] = np.nan
        out = _call(dev, bad_s, y=y)
        assert out["status"] == _lib.NPI_STATUS_BAD_SCORE
        G = int(out["counts"][2])
        assert 1 <= G <= M and int(out["counts"][0]) + int(out["counts"][1]) == M
        assert (out["tps"][G:] == SENTINEL).all() and (out["fps"][G:] == SENTINEL).all() and (out["thr"][G:] == SENTINEL).all()
        bad_y = y.copy()
        bad_y[M // 2], bad_y[0] = 2, -1
        out = _call(dev, s, y=bad_y)
        assert out["status"] == _lib.NPI_STATUS_BAD_LABEL
        good = np.where((bad_y == 0) | (bad_y == 1), bad_y, 0)                  # such a label counts as 0
        out["status"] = 0                                                       # (checked above; everything else as for `good`)
        _check(out, ref.evaluate(s, good), ("bad label", M))
        both = _call(dev, bad_s, y=bad_y, curve=False)
        assert both["status"] == _lib.NPI_STATUS_BAD_SCORE | _lib.NPI_STATUS_BAD_LABEL
        assert _call(dev, bad_s, n_pos=M // 3)["status"] == _lib.NPI_STATUS_BAD_SCORE


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_sklearn_named_functions_equal_rule_r(dev):
    NG.check_pending()
    for name, M in (("seven", 300), ("sigmoid", 1500), ("special", 257)):
        s, y = ref.family(name, M), ref.labels(M, "30")
        r = ref.evaluate(s, y)
        sd, yd = _t(s, dev), _t(y, dev)
        auc, ap = npi.rank_metrics(sd, yd)
        assert auc.dtype == torch.float64 and auc.dim() == 0 and auc.is_cuda and ap.dtype == torch.float64 and ap.dim() == 0
        assert float(auc) == r["auc"] and abs(float(ap) - r["ap"]) <= AP_TOL
        assert npi.roc_auc_score(yd, sd) == r["auc"] and abs(npi.average_precision_score(yd, sd) - r["ap"]) <= AP_TOL
        assert npi.roc_auc_score(yd.to(torch.int32), sd) == r["auc"] and npi.roc_auc_score(yd.bool(), sd) == r["auc"]
        for mine, want in ((npi.roc_curve(yd, sd), ref.roc_curve(r)), (npi.precision_recall_curve(yd, sd), ref.precision_recall_curve(r))):
            for a, b in zip(mine, want):
                assert a.is_cuda and a.dtype == torch.from_numpy(b).dtype and _same(a.cpu().numpy(), b), name
        # the n_pos form; a strided view is made contiguous
        n_pos = M // 4
        rn = ref.evaluate(s, n_pos=n_pos)
        wide = torch.stack([sd, -sd], dim=1)
        auc, ap = npi.rank_metrics(wide[:, 0], n_pos=n_pos)
        assert not wide[:, 0].is_contiguous() and float(auc) == rn["auc"] and abs(float(ap) - rn["ap"]) <= AP_TOL
    NG.check_pending()


def test_sklearn_named_functions_raise_where_sklearn_does(dev):
    NG.check_pending()
    s, y = ref.family("seven", 100), ref.labels(100, "30")
    bad = s.copy()
    bad[7] = np.nan
    for fn in (npi.roc_auc_score, npi.average_precision_score, npi.roc_curve, npi.precision_recall_curve):
        with pytest.raises(ValueError, match="NaN"):
            fn(_t(y, dev), _t(bad, dev))
    for kind in ("P0", "N0"):
        with pytest.raises(ValueError, match="one class"):
            npi.roc_auc_score(_t(ref.labels(100, kind), dev), _t(s, dev))
    assert math.isnan(npi.average_precision_score(_t(ref.labels(100, "P0"), dev), _t(s, dev)))
    two = y.copy()
    two[3] = 2
    with pytest.raises(ValueError, match="0 / 1"):
        npi.roc_auc_score(_t(two, dev), _t(s, dev))
    # rank_metrics reads nothing: the word is filed and raised at the next read
    npi.rank_metrics(_t(bad, dev), _t(y, dev))
    with pytest.raises(ValueError, match="NaN"):
        NG.check_pending()
    NG.check_pending()


def test_gae_test_equals_rule_r_and_sklearn(dev):
    NG.check_pending()
    rng = np.random.default_rng(5)
    z = _t((1.5 * rng.standard_normal((60, 16))).astype(np.float32), dev)
    pos, neg = _t(rng.integers(0, 60, (2, 700)), dev), _t(rng.integers(0, 60, (2, 900)), dev)
    model = npi.GAE(torch.nn.Identity())
    auc, ap = model.test(z, pos, neg)
    assert auc.is_cuda and auc.dtype == torch.float64
    pred = torch.cat([model.decode(z, pos, sigmoid=True), model.decode(z, neg, sigmoid=True)]).cpu().numpy()
    r = ref.evaluate(pred, n_pos=700)
    assert r["G"] < 1600                                                        # the saturated sigmoid ties some pairs
    assert float(auc) == r["auc"] and abs(float(ap) - r["ap"]) <= AP_TOL
    skm = pytest.importorskip("sklearn.metrics")
    y = np.concatenate([np.ones(700), np.zeros(900)])
    assert abs(float(auc) - skm.roc_auc_score(y, pred)) <= 1e-12 and abs(float(ap) - skm.average_precision_score(y, pred)) <= 1e-12
    NG.check_pending()


def test_rank_metrics_under_capture(dev):
    """``rank_metrics`` inside ``torch.cuda.graph`` with preallocated scores, replayed twice with new scores: the eager result"""
    M = 5000
    a, b = _t(ref.family("sigmoid", M, seed=2), dev), _t(ref.family("seven", M, seed=3), dev)
    y = _t(ref.labels(M, "30"), dev)
    eager = [tuple(float(v) for v in npi.rank_metrics(s, y)) for s in (a, b)]
    NG.check_pending()
    scores = a.clone()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        auc, ap = npi.rank_metrics(scores, y)
    for s, want in ((a, eager[0]), (b, eager[1])):
        scores.copy_(s)
        cg.replay()
        torch.cuda.synchronize()
        assert (float(auc), float(ap)) == want
