"""``npi_topk_links`` on the MI355X against Rule K restated on the host (``tests/_topk_ref.py``).

On integer tables (entries in [-4, 4]: every dot product is exact in any order, ties everywhere) ``scores`` and ``ids`` must equal
the restatement BITWISE.  On ``randn`` tables the bar is the bound that holds for any f32 summation order of F products,
``tol(i, j) = (gamma_F + g64_F) <|z_src[i]|, |z_dst[j]|>`` with ``gamma_F = F u / (1 - F u)``, ``u = 2^-24`` (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1: one rounding per fmaf) and ``g64_F`` the same with ``u = 2^-53`` for the fp64 reference's
own error -- derived, not measured."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
import _topk_ref as ref

pytestmark = pytest.mark.gpu

_NS, _ND, _FS, _KS = (1, 63, 65, 130), (1, 127, 129, 300, 1000), (1, 3, 64, 65, 100, 260), (1, 5, 64, 128)
# the tile-edge values together (64 query rows, 128 targets, k-steps of 32) and the extremes, then a walk through the product
CASES = [(63, 127, 64, 64), (65, 129, 65, 128), (65, 127, 65, 5), (63, 129, 64, 1), (130, 1000, 260, 128), (130, 300, 100, 64),
         (1, 1, 1, 1), (1, 1000, 3, 128), (130, 1, 1, 5), (65, 129, 64, 128)]
CASES += [(_NS[i % 4], _ND[i % 5], _FS[i % 6], _KS[(i // 3) % 4]) for i in range(30)]


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _run(dev, zs, zd, k, exclude=None, rows=None, **kw):
    """``topk_links`` on host inputs (``zd`` None: one id space); the results on the host"""
    z = zs.to(dev) if zd is None else (zs.to(dev), zd.to(dev))
    ex = exclude.to(dev) if isinstance(exclude, torch.Tensor) else exclude
    s, i = npi.topk_links(z, k, exclude=ex, rows=None if rows is None else rows.to(dev), **kw)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and not s.requires_grad
    return s.cpu(), i.cpu()


def _check(got, want, what):
    assert _same(got[1], want[1]), (what, "ids")
    assert _same(got[0], want[0]), (what, "scores")


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_every_size():
    assert len(CASES) == 40
    for col, vals in enumerate((_NS, _ND, _FS, _KS)):
        assert {c[col] for c in CASES} == set(vals)
    assert any(k > n_dst for _, n_dst, _, k in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_integer_tables_equal_the_restatement_bitwise(dev, case):
    n_src, n_dst, F, k = case
    NG.check_pending()
    zs, zd = ref.int_tables(n_src, n_dst, F, seed=n_dst + F)
    ex = ref.edges(n_src, n_dst, 3 * n_src, seed=k)
    want = ref.topk(zs, zd, k, ex)
    assert want[2] == 0
    _check(_run(dev, zs, zd, k, ex), want, case)
    NG.check_pending()                                                    # nothing to report


def test_pitched_and_misaligned_views(dev):
    NG.check_pending()
    n_src, n_dst, F, k = 65, 300, 64, 64
    zs, zd = ref.int_tables(n_src, n_dst, F, seed=5)
    ex = ref.edges(n_src, n_dst, 200, seed=5)
    want = ref.topk(zs, zd, k, ex)
    for pad in (4, 5):                                                    # a 16-byte pitch (the fast form) and one that is not
        bs = torch.full((n_src, F + pad), 99.0, device=dev)
        bd = torch.full((n_dst, F + pad), 99.0, device=dev)
        bs[:, :F], bd[:, :F] = zs.to(dev), zd.to(dev)
        vs, vd = bs[:, :F], bd[:, :F]
        assert vs.stride(0) == F + pad and not vs.is_contiguous()
        s, i = npi.topk_links((vs, vd), k, exclude=ex.to(dev))
        _check((s, i), want, ("pitch", pad))
    flat_s = torch.zeros(n_src * F + 1, device=dev)                       # a base 4 bytes past a 16-byte boundary: the guarded form
    flat_d = torch.zeros(n_dst * F + 1, device=dev)
    vs, vd = flat_s[1:].view(n_src, F), flat_d[1:].view(n_dst, F)
    vs.copy_(zs)
    vd.copy_(zd)
    assert vs.data_ptr() % 16 == 4 and vd.data_ptr() % 16 == 4
    _check(npi.topk_links((vs, vd), k, exclude=ex.to(dev)), want, "misaligned base")
    _check(npi.topk_links((vs, zd.to(dev)), k, exclude=ex.to(dev)), want, "one misaligned table")
    NG.check_pending()


def test_one_id_space_without_loops(dev):
    NG.check_pending()
    z = ref.int_tables(130, 130, 64, seed=9)[0]
    z[5] = 4.0                                                            # rows whose best partner is themselves
    z[77] = -4.0
    ex = ref.edges(130, 130, 400, seed=9)
    for k in (5, 128):
        want = ref.topk(z, z, k, ex, allow_loops=False)
        got = _run(dev, z, None, k, ex, allow_loops=False)
        _check(got, want, ("no loops", k))
        assert not bool((got[1] == torch.arange(130)[:, None]).any())
        loops = _run(dev, z, None, k, ex)
        _check(loops, ref.topk(z, z, k, ex), ("loops", k))
        assert int(loops[1][5, 0]) == 5 or (5 in ex[1][ex[0] == 5].tolist())
    NG.check_pending()


def test_rows_permuted_repeated_and_out_of_range(dev):
    NG.check_pending()
    zs, zd = ref.int_tables(130, 300, 65, seed=2)
    ex = ref.edges(130, 300, 500, seed=2)
    full = ref.topk(zs, zd, 5, ex)
    rows = torch.tensor([129, 3, 64, 3, 0, 63, 65, 100, 3])
    got = _run(dev, zs, zd, 5, ex, rows)
    _check(got, ref.topk(zs, zd, 5, ex, rows), "rows")
    assert _same(got[1], full[1][rows]) and _same(got[0], full[0][rows])
    NG.check_pending()
    bad = torch.tensor([7, 130, 2, -1, 129, 2 ** 40])
    want = ref.topk(zs, zd, 5, ex, bad)
    assert want[2] == ref.BAD_SOURCE
    got = _run(dev, zs, zd, 5, ex, bad)
    _check(got, want, "rows with bad ids")
    for r in (1, 3, 5):
        assert bool((got[1][r] == -1).all()) and bool((got[0][r] == float("-inf")).all())
    with pytest.raises(ValueError, match="source id"):
        NG.check_pending()
    NG.check_pending()                                                    # reported once


# ---- exclusion -------------------------------------------------------------------------------------------------------------------------------
def test_exclusion_sets(dev):
    NG.check_pending()
    n_src, n_dst, F, k = 65, 1000, 3, 64
    zs, zd = ref.int_tables(n_src, n_dst, F, seed=4)
    g = torch.Generator().manual_seed(4)
    every = torch.arange(n_dst)
    parts = [ref.edges(n_src, n_dst, 400, seed=4),
             torch.stack([torch.zeros(n_dst, dtype=torch.int64), every]),                              # row 0: every target
             torch.stack([torch.ones(n_dst - (k - 1), dtype=torch.int64), torch.randperm(n_dst, generator=g)[:n_dst - (k - 1)]]),
             torch.stack([torch.full((900,), 64, dtype=torch.int64), torch.randperm(n_dst, generator=g)[:900]])]    # a hub row
    ex = torch.cat(parts, 1)
    ex = ex[:, torch.randperm(ex.size(1), generator=g)]
    want = ref.topk(zs, zd, k, ex)
    assert bool((want[1][0] == -1).all()) and int((want[1][1] >= 0).sum()) == k - 1 and int((want[1][64] >= 0).sum()) == k
    plain = _run(dev, zs, zd, k, ex)
    _check(plain, want, "edge list")
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))
    assert known.size == (n_src, n_dst) and known.num_edges == ex.size(1)
    _check(_run(dev, zs, zd, k, known), want, "KnownLinks")
    _check(_run(dev, zs, zd, 128, known, splits=7), ref.topk(zs, zd, 128, ex), "KnownLinks, k = 128, 7 splits")
    _check(_run(dev, zs, zd, k), ref.topk(zs, zd, k), "no exclusion")
    _check(_run(dev, zs, zd, k, torch.zeros((2, 0), dtype=torch.int64)), ref.topk(zs, zd, k), "an empty edge list")
    with pytest.raises(ValueError, match="size"):
        npi.topk_links((zs[:60].to(dev), zd.to(dev)), k, exclude=known)
    NG.check_pending()


# ---- ties and zeros ------------------------------------------------------------------------------------------------------------------------
def test_ties_and_zeros(dev):
    NG.check_pending()
    zs, zd = ref.int_tables(65, 300, 64, seed=6)
    zd = zd[(torch.arange(300) // 3) * 3].contiguous()                   # every row three times
    ex = ref.edges(65, 300, 300, seed=6)
    got = _run(dev, zs, zd, 64, ex)
    _check(got, ref.topk(zs, zd, 64, ex), "duplicated rows")
    s, i = got
    tie = s[:, 1:] == s[:, :-1]
    assert bool(tie.any()) and bool((i[:, 1:][tie] > i[:, :-1][tie]).all())
    # all-zero tables: the first k ids that are not excluded
    zero_s, zero_d = torch.zeros(65, 5), torch.zeros(300, 5)
    got = _run(dev, zero_s, zero_d, 64, ex)
    _check(got, ref.topk(zero_s, zero_d, 64, ex), "zeros")
    ok = ref.allowed(65, 300, ex)
    for r in (0, 33, 64):
        assert got[1][r].tolist() == np.nonzero(ok[r])[0][:64].tolist()
    # zeros of both signs: products -0.0 and +0.0, and sums that underflow to -0.0, all rank and come out as +0.0
    zs = torch.tensor([[0.0], [-0.0], [-1e-30], [1e-30]])
    zd = torch.tensor([[1e-30], [0.0], [-0.0], [5.0], [-1e-30], [-3.0]] * 25)
    got = _run(dev, zs, zd, 128)
    _check(got, ref.topk(zs, zd, 128), "signed zeros")
    assert not bool(torch.signbit(got[0][:2]).any()) and bool((got[0][:2] == 0).all()) and got[1][0].tolist() == list(range(128))
    zero = got[0] == 0
    assert bool(zero[2:].any()) and not bool(torch.signbit(got[0][zero]).any())
    NG.check_pending()


# ---- NaN / inf -----------------------------------------------------------------------------------------------------------------------------
def test_nan_targets_are_never_returned_and_infinities_are_ordinary_scores(dev):
    NG.check_pending()
    zs, zd = ref.int_tables(65, 127, 3, seed=8)
    zs[:, 0] = torch.arange(65).float() % 4 + 1                          # a positive first column: inf * it is inf, never NaN
    zd[5, 0], zd[7, 0] = float("inf"), float("-inf")
    clean = _run(dev, zs, zd, 128)
    NG.check_pending()                                                    # infinities alone report nothing
    _check(clean, ref.topk(zs, zd, 128), "infinities")
    assert bool((clean[1][:, 0] == 5).all()) and bool((clean[1][:, 126] == 7).all()) and bool((clean[1][:, 127] == -1).all())
    assert bool((clean[0][:, 0] == float("inf")).all()) and bool((clean[0][:, 126] == float("-inf")).all())
    zd[9, 2] = float("nan")
    ex = torch.tensor([[3, 3], [9, 10]])
    want = ref.topk(zs, zd, 128, ex)
    assert want[2] == ref.BAD_SCORE
    got = _run(dev, zs, zd, 128, ex)
    _check(got, want, "a NaN target")
    assert not bool((got[1] == 9).any()) and not bool(torch.isnan(got[0]).any())
    with pytest.raises(ValueError, match="NaN"):
        NG.check_pending()
    # the NaN pair excluded for the only query: nothing to report
    one = _run(dev, zs, zd, 5, ex, rows=torch.tensor([3]))
    _check(one, ref.topk(zs, zd, 5, ex, rows=torch.tensor([3])), "the NaN pair excluded")
    NG.check_pending()


# ---- independence of the split, of the order of rows and of the call --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "real"])
def test_results_do_not_depend_on_splits_row_order_or_the_call(dev, kind):
    NG.check_pending()
    n_src, n_dst, F, k = 130, 1000, 100, 64
    zs, zd = (ref.int_tables if kind == "exact" else ref.real_tables)(n_src, n_dst, F, seed=11)
    ex = ref.edges(n_src, n_dst, 2000, seed=11)
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))
    base = _run(dev, zs, zd, k, known)
    if kind == "exact":
        _check(base, ref.topk(zs, zd, k, ex), "default splits")
    for splits in (1, 2, 3, 7, 8, 64, 1000):
        _check(_run(dev, zs, zd, k, known, splits=splits), base, ("splits", splits))
    _check(_run(dev, zs, zd, k, known), base, "a second call")
    g = torch.Generator().manual_seed(11)
    a, b = torch.randperm(n_src, generator=g), torch.randperm(n_src, generator=g)
    ra, rb = _run(dev, zs, zd, k, known, a, splits=2), _run(dev, zs, zd, k, known, b, splits=3)
    inv_a, inv_b = torch.argsort(a), torch.argsort(b)
    _check((ra[0][inv_a], ra[1][inv_a]), base, "rows order a")
    _check((rb[0][inv_b], rb[1][inv_b]), base, "rows order b")
    NG.check_pending()


# ---- real-valued tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [64, 100, 260])
def test_real_tables_within_the_bound_of_any_summation_order(dev, F):
    NG.check_pending()
    n_src, n_dst, k = 65, 1000, 64
    zs, zd = ref.real_tables(n_src, n_dst, F, seed=F)
    ex = ref.edges(n_src, n_dst, 1500, seed=F)
    ex = torch.cat([ex, torch.stack([torch.full((960,), 7, dtype=torch.int64), torch.arange(960)])], 1)     # row 7: 40 candidates
    D = ref.scores64(zs, zd)
    cand = ref.candidates(D, ex)
    u64 = 2.0 ** -53
    tol = (ref.gamma(F) + F * u64 / (1 - F * u64)) * (zs.double().abs().numpy() @ zd.double().abs().numpy().T)
    s, i = _run(dev, zs, zd, k, ex)
    s, i = s.double().numpy(), i.numpy()
    worst = 0.0
    for r in range(n_src):
        n = min(k, int(cand[r].sum()))
        js = i[r, :n]
        assert (i[r, n:] == -1).all() and np.isneginf(s[r, n:]).all() and (js >= 0).all(), r            # the number of real entries
        assert cand[r, js].all() and len(set(js.tolist())) == n, r                                       # candidates, distinct
        err = np.abs(s[r, :n] - D[r, js])
        worst = max(worst, float((err / tol[r, js]).max()) if n else 0.0)
        assert (err <= tol[r, js]).all(), r
        assert (np.diff(s[r, :n]) <= 0).all(), r                                                          # non-increasing ...
        eq = np.diff(s[r, :n]) == 0
        assert (np.diff(js)[eq] > 0).all(), r                                                             # ... ties by ascending id
        if n:
            rest = cand[r].copy()
            rest[js] = False
            last = js[-1]
            assert (D[r, rest] <= D[r, last] + tol[r, rest] + tol[r, last]).all(), r                      # nothing better was left out
    print(F, "worst error / bound", worst)
    assert 0 < int(cand[7].sum()) <= 40                                                                    # fewer than k candidates
    NG.check_pending()


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
def test_topk_links_under_capture(dev):
    """one ``topk_links`` call (every source row, a ``KnownLinks``) inside ``torch.cuda.graph`` on one stream, replayed twice"""
    NG.check_pending()
    zs, zd = ref.real_tables(130, 1000, 64, seed=13)
    ex = ref.edges(130, 1000, 1000, seed=13)
    z = (zs.to(dev), zd.to(dev))
    known = npi.KnownLinks(ex.to(dev), (130, 1000))
    eager = npi.topk_links(z, 32, exclude=known)
    NG.check_pending()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        s, i = npi.topk_links(z, 32, exclude=known)
    for _ in range(2):
        s.fill_(7.0)
        i.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        _check((s, i), eager, "replay")


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------------
def test_decoder_topk_and_gae_predict(dev):
    NG.check_pending()
    zs, zd = ref.real_tables(65, 300, 64, seed=17)
    ex = ref.edges(65, 300, 300, seed=17).to(dev)
    z = (zs.to(dev), zd.to(dev))
    logits, ids = npi.topk_links(z, 10, exclude=ex)
    dec = npi.InnerProductDecoder()
    p, pi = dec.topk(z, 10, exclude=ex)
    assert _same(p, torch.sigmoid(logits)) and _same(pi, ids)
    raw, ri = dec.topk(z, 10, exclude=ex, rows=torch.tensor([4, 2], device=dev), sigmoid=False)
    assert _same(raw, logits[[4, 2]]) and _same(ri, ids[[4, 2]])
    assert not hasattr(dec, "forward_all")
    # one id space: never (v, v), never a known edge
    z1 = ref.real_tables(130, 1, 64, seed=19)[0].to(dev).requires_grad_(True)
    e1 = ref.edges(130, 130, 2000, seed=19).to(dev)
    model = npi.GAE(torch.nn.Identity())
    p, ids = model.predict(z1, 128, e1)
    assert p.shape == (130, 128) and not p.requires_grad and float(p.min()) >= 0.0 and float(p.max()) <= 1.0
    ids = ids.cpu()
    assert not bool((ids == torch.arange(130)[:, None]).any())
    known = set(map(tuple, e1.t().tolist()))
    pairs = {(r, int(j)) for r in range(130) for j in ids[r] if j >= 0}
    assert not (pairs & known)
    assert all(int((ids[r] >= 0).sum()) == min(128, 130 - 1 - len({b for a, b in known if a == r and b != r})) for r in range(130))
    lp, lids = model.predict(z1, 128, npi.KnownLinks(e1, 130), sigmoid=False)
    assert _same(lids, ids) and _same(torch.sigmoid(lp), p)
    # two id spaces: loops are ordinary pairs
    p2, i2 = model.predict(z, 10, ex, rows=torch.tensor([0, 1], device=dev))
    assert _same(i2, npi.topk_links(z, 10, exclude=ex)[1][:2])
    NG.check_pending()
