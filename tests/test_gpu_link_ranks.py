"""``npi_link_ranks`` on the MI355X against Rule F restated on the host (``tests/_link_rank_ref.py``) and against ``topk_links`` on the
device.

On integer tables (entries in [-4, 4]: every dot product is exact in any order, ties everywhere) ``counts`` and ``scores`` must equal
the restatement BITWISE.  On ``randn`` tables the counts are bracketed by the bound that holds for any f32 summation order of F
products, ``tol(i, j) = (gamma_F + g64_F) <|z_src[i]|, |z_dst[j]|>`` (``test_gpu_topk_links.py``): a competitor that beats the target
by more than both tolerances in fp64 must be counted ``greater``, and whatever is counted ``greater`` or ``equal`` must reach the
target within both tolerances -- derived, not measured."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
import _link_rank_ref as ref
import _topk_ref as tref

pytestmark = pytest.mark.gpu

SHAPES = [(63, 127, 64), (65, 129, 65), (130, 1000, 260), (130, 300, 100), (1, 1, 1), (1, 1000, 3), (130, 1, 1)]
QS = (1, 63, 65, 200)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.cpu().contiguous().numpy().tobytes() == b.cpu().contiguous().numpy().tobytes()


def _run(dev, zs, zd, q, exclude=None, **kw):
    """``link_ranks`` on host inputs (``zd`` None: one id space); ``(counts, scores)`` on the host"""
    z = zs.to(dev) if zd is None else (zs.to(dev), zd.to(dev))
    ex = exclude.to(dev) if isinstance(exclude, torch.Tensor) else exclude
    r = npi.link_ranks(z, q.to(dev), exclude=ex, **kw)
    assert r.counts.dtype == torch.int64 and r.score.dtype == torch.float32 and not r.score.requires_grad
    assert r.counts.shape == (q.size(1), 4) and r.score.shape == (q.size(1),)
    for c, part in enumerate((r.greater, r.equal, r.equal_before, r.candidates)):
        assert _same(part, r.counts[:, c])
    return r.counts.cpu(), r.score.cpu()


def _check(got, want, what):
    assert _same(got[0], want[0]), (what, "counts", got[0][:8].tolist(), want[0][:8].tolist())
    assert _same(got[1], want[1]), (what, "scores")


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_integer_tables_equal_the_restatement_bitwise(dev, shape):
    n_src, n_dst, F = shape
    NG.check_pending()
    zs, zd = tref.int_tables(n_src, n_dst, F, seed=n_dst + F)
    ex = tref.edges(n_src, n_dst, 3 * n_src, seed=F)
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))
    for Q in QS:
        q = ref.queries(n_src, n_dst, Q, ex, seed=Q)
        want = ref.link_ranks(zs, zd, q, ex)
        assert want[2] == 0
        _check(_run(dev, zs, zd, q, known), want, (shape, Q))
    q = ref.queries(n_src, n_dst, 65, ex, seed=7)
    _check(_run(dev, zs, zd, q), ref.link_ranks(zs, zd, q), (shape, "no exclusion"))
    _check(_run(dev, zs, zd, q, ex), ref.link_ranks(zs, zd, q, ex), (shape, "an edge list"))
    NG.check_pending()                                                    # nothing to report


def test_one_id_space_without_loops(dev):
    NG.check_pending()
    z = tref.int_tables(130, 130, 64, seed=9)[0]
    z[5] = 4.0                                                            # rows whose best partner is themselves
    z[77] = -4.0
    ex = tref.edges(130, 130, 400, seed=9)
    q = ref.queries(130, 130, 200, ex, seed=9)
    q[:, 1::8] = q[0, 1::8]                                               # queries (v, v): ranked, and never their own competitor
    q[:, 1] = 5
    for loops in (False, True):
        want = ref.link_ranks(z, z, q, ex, allow_loops=loops)
        _check(_run(dev, z, None, q, ex, allow_loops=loops), want, ("loops", loops))
    a, b = ref.link_ranks(z, z, q, ex, allow_loops=False)[0], ref.link_ranks(z, z, q, ex, allow_loops=True)[0]
    assert int(a[1, 0]) == 0 and not torch.equal(a, b)                    # (5, 5) is the best pair of row 5; the flag matters
    NG.check_pending()


def test_pitched_and_misaligned_views(dev):
    NG.check_pending()
    n_src, n_dst, F = 65, 300, 64
    zs, zd = tref.int_tables(n_src, n_dst, F, seed=5)
    ex = tref.edges(n_src, n_dst, 200, seed=5)
    q = ref.queries(n_src, n_dst, 130, ex, seed=5).to(dev)
    want = ref.link_ranks(zs, zd, q.cpu(), ex)
    for pad in (4, 5):                                                    # a 16-byte pitch (the fast form) and one that is not
        bs = torch.full((n_src, F + pad), 99.0, device=dev)
        bd = torch.full((n_dst, F + pad), 99.0, device=dev)
        bs[:, :F], bd[:, :F] = zs.to(dev), zd.to(dev)
        vs, vd = bs[:, :F], bd[:, :F]
        assert vs.stride(0) == F + pad and not vs.is_contiguous()
        r = npi.link_ranks((vs, vd), q, exclude=ex.to(dev))
        _check((r.counts, r.score), want, ("pitch", pad))
    flat_s = torch.zeros(n_src * F + 1, device=dev)                       # a base 4 bytes past a 16-byte boundary: the guarded form
    flat_d = torch.zeros(n_dst * F + 1, device=dev)
    vs, vd = flat_s[1:].view(n_src, F), flat_d[1:].view(n_dst, F)
    vs.copy_(zs)
    vd.copy_(zd)
    assert vs.data_ptr() % 16 == 4 and vd.data_ptr() % 16 == 4
    for tables, what in (((vs, vd), "misaligned base"), ((vs, zd.to(dev)), "one misaligned table")):
        r = npi.link_ranks(tables, q, exclude=ex.to(dev))
        _check((r.counts, r.score), want, what)
    NG.check_pending()


def test_bad_ids_repeated_and_permuted_queries(dev):
    NG.check_pending()
    zs, zd = tref.int_tables(130, 300, 65, seed=2)
    ex = tref.edges(130, 300, 500, seed=2)
    q = ref.queries(130, 300, 200, ex, seed=2)
    base = _run(dev, zs, zd, q, ex)
    _check(base, ref.link_ranks(zs, zd, q, ex), "queries")
    g = torch.Generator().manual_seed(2)
    perm = torch.randperm(200, generator=g)
    got = _run(dev, zs, zd, q[:, perm], ex, splits=2)
    _check(got, (base[0][perm], base[1][perm]), "permuted")
    rep = torch.tensor([3, 3, 199, 0, 3, 64, 63, 0])
    got = _run(dev, zs, zd, q[:, rep], ex, splits=3)
    _check(got, (base[0][rep], base[1][rep]), "repeated")
    NG.check_pending()
    bad = torch.tensor([[7, 130, 2, -1, 129, 2 ** 40, 5, 5, 5], [3, 3, 300, 4, 299, 0, -1, 2 ** 40, 6]])
    want = ref.link_ranks(zs, zd, bad, ex)
    assert want[2] == ref.BAD_PAIR
    got = _run(dev, zs, zd, bad, ex)
    _check(got, want, "queries with bad ids")
    for r in (1, 2, 3, 5, 6, 7):
        assert got[0][r].tolist() == [-1] * 4 and float(got[1][r]) == float("-inf")
    with pytest.raises(IndexError, match="link_ranks"):
        NG.check_pending()
    NG.check_pending()                                                    # reported once


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_results_do_not_depend_on_splits_or_the_call(dev, kind):
    NG.check_pending()
    n_src, n_dst, F = 130, 1000, 100
    zs, zd = (tref.int_tables if kind == "exact" else tref.real_tables)(n_src, n_dst, F, seed=11)
    ex = tref.edges(n_src, n_dst, 2000, seed=11)
    q = ref.queries(n_src, n_dst, 200, ex, seed=11)
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))
    base = _run(dev, zs, zd, q, known)
    if kind == "exact":
        _check(base, ref.link_ranks(zs, zd, q, ex), "default splits")
    for splits in (1, 2, 3, 7, 64):
        _check(_run(dev, zs, zd, q, known, splits=splits), base, ("splits", splits))
    _check(_run(dev, zs, zd, q, known), base, "a second call")
    NG.check_pending()


# ---- NaN / inf -----------------------------------------------------------------------------------------------------------------------------
def test_nan_and_infinities(dev):
    NG.check_pending()
    zs, zd = tref.int_tables(65, 127, 3, seed=8)
    zs[:, 0] = torch.arange(65).float() % 4 + 1                          # a positive first column: inf * it is inf, never NaN
    zd[5, 0], zd[7, 0] = float("inf"), float("-inf")
    q = torch.stack([torch.arange(65), torch.arange(65) % 10])            # targets 0 .. 9: the infinities and (later) the NaN among them
    clean = _run(dev, zs, zd, q)
    NG.check_pending()                                                    # infinities alone report nothing
    _check(clean, ref.link_ranks(zs, zd, q), "infinities")
    assert clean[0][5].tolist()[:2] == [0, 0] and float(clean[1][5]) == float("inf")
    assert clean[0][7].tolist() == [126, 0, 0, 126] and float(clean[1][7]) == float("-inf")
    zd[9, 2] = float("nan")
    ex = torch.tensor([[3, 3], [9, 10]])
    want = ref.link_ranks(zs, zd, q, ex)
    assert want[2] == ref.BAD_SCORE
    got = _run(dev, zs, zd, q, ex)
    _check(got, want, "a NaN target row")
    assert got[0][9].tolist() == [-1] * 4 and got[0][19].tolist() == [-1] * 4            # the NaN is the target
    assert int(got[0][0][3]) == 125 and int(got[0][3][3]) == 124                         # a NaN competitor is not counted
    with pytest.raises(ValueError, match="NaN"):
        NG.check_pending()
    # the NaN pair excluded for the only query, and not its target: nothing to report
    one = torch.tensor([[3], [4]])
    _check(_run(dev, zs, zd, one, ex), ref.link_ranks(zs, zd, one, ex), "the NaN pair excluded")
    NG.check_pending()
    # ... but as the target it is ranked although excluded: NaN, a row of -1
    one = torch.tensor([[3], [9]])
    got = _run(dev, zs, zd, one, ex)
    assert got[0].tolist() == [[-1] * 4]
    with pytest.raises(ValueError, match="NaN"):
        NG.check_pending()


# ---- real-valued tables ---------------------------------------------------------------------------------------------------------------------
def _real_case(F):
    n_src, n_dst = 65, 1000
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=F)
    ex = tref.edges(n_src, n_dst, 1500, seed=F)
    q = ref.queries(n_src, n_dst, 200, ex, seed=F)
    return n_src, n_dst, zs, zd, ex, q


@pytest.mark.parametrize("F", [64, 100, 260])
def test_real_tables_agree_with_topk_links_on_the_device(dev, F):
    """Rule F 4 on the device: the threshold is the scan's own key"""
    NG.check_pending()
    n_src, n_dst, zs, zd, ex, q = _real_case(F)
    k = 128
    z = (zs.to(dev), zd.to(dev))
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))
    r = npi.link_ranks(z, q.to(dev), exclude=known)
    ts, ti = npi.topk_links(z, k, exclude=known)
    ts, ti = ts.cpu().numpy(), ti.cpu().numpy()
    pos = (r.greater + r.equal_before).cpu().numpy()
    score = r.score.cpu().numpy()
    ok = tref.allowed(n_src, n_dst, ex)
    inside = checked = 0
    for i, (s, t) in enumerate(q.t().tolist()):
        if not ok[s, t]:
            continue
        checked += 1
        found = np.nonzero(ti[s] == t)[0]
        assert (len(found) == 1) == (pos[i] < k), (i, s, t)
        if pos[i] < k:
            inside += 1
            assert found[0] == pos[i], (i, s, t)
            assert ts[s, pos[i]].tobytes() == score[i].tobytes(), (i, s, t)
    assert checked >= 140 and 5 <= inside < checked                      # both sides of k = 128 among 1000 targets
    NG.check_pending()


@pytest.mark.parametrize("F", [64, 100, 260])
def test_real_tables_within_the_bracket_of_any_summation_order(dev, F):
    NG.check_pending()
    n_src, n_dst, zs, zd, ex, q = _real_case(F)
    D = tref.scores64(zs, zd)
    cand = tref.candidates(D, ex)
    u64 = 2.0 ** -53
    tol = (tref.gamma(F) + F * u64 / (1 - F * u64)) * (zs.double().abs().numpy() @ zd.double().abs().numpy().T)
    counts, score = _run(dev, zs, zd, q, ex)
    counts, score = counts.numpy(), score.double().numpy()
    for i, (s, t) in enumerate(q.t().tolist()):
        comp = cand[s].copy()
        comp[t] = False
        greater, equal, before, n = counts[i]
        assert n == comp.sum(), i
        assert abs(score[i] - D[s, t]) <= tol[s, t], i
        surely = int((comp & (D[s] - tol[s] > D[s, t] + tol[s, t])).sum())
        maybe = int((comp & (D[s] + tol[s] >= D[s, t] - tol[s, t])).sum())
        assert surely <= greater and greater + equal <= maybe, (i, surely, greater, equal, maybe)
        assert 0 <= before <= equal
    NG.check_pending()


# ---- the metrics and the wrappers ---------------------------------------------------------------------------------------------------------
def test_ranking_metrics_wrappers_and_tie_rules(dev):
    NG.check_pending()
    n = 130
    z = tref.int_tables(n, n, 64, seed=21)[0]
    ex = tref.edges(n, n, 400, seed=21)
    q = ref.queries(n, n, 200, ex, seed=21)
    q[:, 2::16] = q[0, 2::16]
    zd = tref.int_tables(n, 300, 64, seed=22)[1]
    q2 = ref.queries(n, 300, 200, None, seed=22)
    q2[0, 7] = n                                                          # one bad pair: left out of the means
    ex2 = tref.edges(n, 300, 400, seed=22)
    want1 = ref.link_ranks(z, z, q, ex, allow_loops=False)[0].numpy()
    want2 = ref.link_ranks(z, zd, q2, ex2)[0].numpy()
    zg, zdg = z.to(dev), zd.to(dev)
    model, dec = npi.GAE(torch.nn.Identity()), npi.InnerProductDecoder()

    def close(got, want, ks):
        assert set(got) == {"mrr", "mean_rank"} | {f"hits@{k}" for k in ks}
        for name, v in got.items():
            assert v.dtype == torch.float64 and v.dim() == 0 and v.device.type == "cuda", name
            if name.startswith("hits"):
                assert float(v) == float(want[name]), (name, float(v), want[name])
            else:
                assert abs(float(v) - want[name]) <= 1e-12 * abs(want[name]), (name, float(v), want[name])

    for ties in ("min", "max", "average", "id"):
        ks = (1, 3, 10) if ties != "id" else (1, 50)
        close(model.test_ranking(zg, q.to(dev), ex.to(dev), ks=ks, ties=ties), ref.metrics(want1, ks, ties), ks)
        close(npi.ranking_metrics((zg, zdg), q2.to(dev), exclude=ex2.to(dev), ks=ks, ties=ties), ref.metrics(want2, ks, ties), ks)
        r = dec.ranks((zg, zdg), q2.to(dev), exclude=ex2.to(dev))
        ok = want2[:, 0] >= 0
        assert r.valid.cpu().numpy().tolist() == ok.tolist()
        got = r.rank(ties).cpu().numpy()
        assert got.dtype == (np.float64 if ties == "average" else np.int64)
        assert (got[ok] == ref.ranks(want2[ok], ties)).all(), ties
    with pytest.raises(IndexError):
        NG.check_pending()                                                # the bad pair of q2
    # a pair (z, z) is one id space to the model, as in predict; the default ks and ties
    close(model.test_ranking((zg, zg), q.to(dev), npi.KnownLinks(ex.to(dev), n)), ref.metrics(want1), (1, 3, 10))
    # no ranked query: NaN
    none = npi.ranking_metrics(zg, torch.tensor([[n], [0]], device=dev))
    assert all(bool(torch.isnan(v)) for v in none.values())
    with pytest.raises(IndexError):
        NG.check_pending()
    empty = npi.link_ranks(zg, torch.zeros((2, 0), dtype=torch.int64, device=dev))
    assert empty.counts.shape == (0, 4) and empty.score.shape == (0,)
    with pytest.raises(ValueError, match="size"):
        npi.link_ranks((zg[:60], zdg), q2.to(dev), exclude=npi.KnownLinks(ex2.to(dev), (n, 300)))
    NG.check_pending()


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
def test_link_ranks_under_capture(dev):
    """one ``link_ranks`` call (a ``KnownLinks``) inside ``torch.cuda.graph`` on one stream, replayed twice"""
    NG.check_pending()
    zs, zd = tref.real_tables(130, 1000, 64, seed=13)
    ex = tref.edges(130, 1000, 1000, seed=13)
    q = ref.queries(130, 1000, 200, ex, seed=13).to(dev)
    z = (zs.to(dev), zd.to(dev))
    known = npi.KnownLinks(ex.to(dev), (130, 1000))
    eager = npi.link_ranks(z, q, exclude=known)
    NG.check_pending()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        r = npi.link_ranks(z, q, exclude=known)
    for _ in range(2):
        r.counts.fill_(7)
        r.score.fill_(7.0)
        cg.replay()
        torch.cuda.synchronize()
        _check((r.counts, r.score), (eager.counts, eager.score), "replay")
