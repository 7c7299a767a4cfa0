"""``npi_softmax_link_*`` on the MI355X against Rule L restated in fp64 on the host (``tests/_softmax_link_ref.py``) and against
``link_ranks`` on the device.

The bar is the project's ``GRAD_REL`` (1e-5, ``_util.rel_max``: max |diff| / max |reference|) for ``lp``, the loss, ``dZ_src`` and
``dZ_dst``; ``tests/test_softmax_link_cpu.py`` shows that the restatement's own float32 form sits a factor of four inside it on
every parity input used here.  The exact cases, the views, the reproducibility and the order against ``link_ranks`` are bitwise."""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
from _util import GRAD_REL, rel_max
import _softmax_link_ref as ref
import _topk_ref as tref

pytestmark = pytest.mark.gpu

SCALE = ref.SCALE


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.detach().cpu().contiguous().numpy().tobytes() == b.detach().cpu().contiguous().numpy().tobytes()


def _zero(t: torch.Tensor) -> bool:
    return bool((t == 0).all())


def _run(dev, zs, zd, q, u=None, exclude=None, want=(True, True), **kw):
    """``link_log_softmax`` on host inputs (``zd`` None: one id space) and, with ``u``, its backward under that upstream gradient:
    ``(lp, dZ_src, dZ_dst)`` on the device"""
    a = zs.to(dev).requires_grad_(u is not None and want[0])
    b = None if zd is None else zd.to(dev).requires_grad_(u is not None and want[1])
    lp = npi.link_log_softmax(a if b is None else (a, b), q.to(dev), exclude=exclude, **kw)
    assert lp.dtype == torch.float32 and lp.shape == (q.size(1),)
    if u is None:
        assert not lp.requires_grad
        return lp, None, None
    (lp * u.to(dev)).sum().backward()
    return lp.detach(), a.grad, None if b is None else b.grad


def _within(got, want, what):
    for g, w, name in zip(got, want, ("lp", "dZ_src", "dZ_dst")):
        if w is None:
            assert g is None, (what, name)
            continue
        err = rel_max(g, w)
        print(what, name, "rel_max", err)
        assert err <= GRAD_REL, (what, name, err)


# ---- parity with the fp64 restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", ref.QS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_parity_with_the_restatement(dev, shape, Q):
    n_src, n_dst, F = shape
    NG.check_pending()
    zs, zd, ex, q, u = ref.inputs(shape, Q)
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))
    got = {}
    for name, exclude in (("known", known), ("edges", ex.to(dev)), ("none", None)):
        want = ref.expected(shape, Q, exclude is not None)
        got[name] = _run(dev, zs, zd, q, u, exclude, scale=SCALE)
        _within(got[name], want, (shape, Q, name))
        with torch.no_grad():
            loss = npi.listwise_loss((zs.to(dev), zd.to(dev)), q.to(dev), exclude=exclude, scale=SCALE)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and not loss.requires_grad
        want_loss = ref.loss(want[0], Q)
        assert abs(float(loss) - float(want_loss)) <= GRAD_REL * abs(float(want_loss)), (shape, Q, name, float(loss), float(want_loss))
        # rows of sources that occur in no query, and of targets no query can reach, are exactly 0 where the reference's are
        for g, w in zip(got[name][1:], want[1:]):
            never = (w == 0).all(1)
            assert _zero(g[never.to(dev)]), (shape, Q, name)
    assert all(_same(a, b) for a, b in zip(got["known"], got["edges"]))                  # the per-call sort builds the same CSR
    # gradients to one table only, and to neither: what is built is what is asked for, the values are the same bits
    lp_s, ds, dd = _run(dev, zs, zd, q, u, known, want=(True, False), scale=SCALE)
    assert dd is None and _same(ds, got["known"][1]) and _same(lp_s, got["known"][0])
    lp_d, ds, dd = _run(dev, zs, zd, q, u, known, want=(False, True), scale=SCALE)
    assert ds is None and _same(dd, got["known"][2]) and _same(lp_d, got["known"][0])
    with torch.no_grad():
        lp_n = _run(dev, zs, zd, q, None, known, scale=SCALE)[0]
    assert _same(lp_n, got["known"][0])
    NG.check_pending()


@pytest.mark.parametrize("splits", [1, 2, 3, 64])
@pytest.mark.parametrize("shape", [(130, 1000, 260), (40, 449, 256)], ids=lambda c: "x".join(map(str, c)))
def test_every_split_count_is_within_the_bar(dev, shape, splits):
    NG.check_pending()
    zs, zd, ex, q, u = ref.inputs(shape, 200)
    known = npi.KnownLinks(ex.to(dev), shape[:2])
    _within(_run(dev, zs, zd, q, u, known, scale=SCALE, splits=splits), ref.expected(shape, 200, True), (shape, "splits", splits))
    NG.check_pending()


@pytest.mark.parametrize("shape", [(65, 129, 65), (40, 449, 256)], ids=lambda c: "x".join(map(str, c)))
def test_listwise_loss_gradients(dev, shape):
    """the scalar form under its own backward: u = -1 / Q for every pair, times the upstream gradient of the loss"""
    NG.check_pending()
    Q = 65
    zs, zd, ex, q, _ = ref.inputs(shape, Q)
    want = ref.link_log_softmax(zs.double(), zd.double(), q, ex, True, SCALE, torch.full((Q,), -3.0 / Q))
    a, b = zs.to(dev).requires_grad_(), zd.to(dev).requires_grad_()
    loss = npi.listwise_loss((a, b), q.to(dev), exclude=ex.to(dev), scale=SCALE)
    (3.0 * loss).backward()
    _within((loss.detach(), a.grad, b.grad), (ref.loss(want[0], Q), want[1], want[2]), (shape, "listwise_loss"))
    NG.check_pending()


# ---- exact cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 1, 1), (1, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_a_single_target_gives_exact_zeros(dev, shape):
    n_src, n_dst, F = shape
    NG.check_pending()
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=3)
    for Q in (1, 65):
        q = ref.queries(n_src, n_dst, Q, seed=3)
        lp, ds, dd = _run(dev, zs * 50, zd, q, ref.upstream(Q, seed=1) + 1.0, scale=SCALE)
        assert _zero(lp) and _zero(ds) and _zero(dd), (shape, Q)
        a = (zs * 50).to(dev).requires_grad_()
        loss = npi.listwise_loss((a, zd.to(dev)), q.to(dev), scale=2.0)
        loss.backward()
        assert float(loss.detach()) == 0.0 and _zero(a.grad)
    NG.check_pending()


def test_a_source_with_every_other_target_excluded_gives_exact_zeros(dev):
    NG.check_pending()
    n_src, n_dst, F, s, t = 5, 200, 16, 2, 77
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=4)
    others = torch.tensor([j for j in range(n_dst) if j != t])
    for with_target in (False, True):                                     # ... and the target itself excluded too: it stays in
        cols = torch.arange(n_dst) if with_target else others
        ex = torch.stack([torch.full_like(cols, s), cols])
        q = torch.tensor([[0, s, 4, s], [5, t, 199, t]])
        u = torch.tensor([0.0, 1.5, 0.0, -2.0])                           # only the queries of that source carry a gradient
        lp, ds, dd = _run(dev, zs, zd, q, u, ex.to(dev), scale=0.5)
        assert float(lp[1]) == 0.0 and float(lp[3]) == 0.0 and float(lp[0]) < 0.0
        assert _zero(ds) and _zero(dd), with_target
        with torch.no_grad():
            loss = npi.listwise_loss((zs.to(dev), zd.to(dev)), q[:, [1, 3]].to(dev), exclude=ex.to(dev), scale=0.5)
        assert float(loss) == 0.0
    NG.check_pending()


def test_bad_pairs_give_zero_and_change_no_gradient(dev):
    NG.check_pending()
    n_src, n_dst, F = 65, 129, 65
    zs, zd, ex, q, _ = ref.inputs((n_src, n_dst, F), 63)
    bad = torch.tensor([[n_src, 3, -1, 5, 2 ** 40, 7], [4, n_dst, 6, -1, 8, 2 ** 40]])
    both = torch.cat([q, bad], 1)
    known = npi.KnownLinks(ex.to(dev), (n_src, n_dst))

    def grads(pairs):
        a, b = zs.to(dev).requires_grad_(), zd.to(dev).requires_grad_()
        lp = npi.link_log_softmax((a, b), pairs.to(dev), exclude=known, scale=SCALE)
        (-lp.sum()).backward()
        return lp.detach(), a.grad, b.grad

    clean = grads(q)
    NG.check_pending()
    lp, ds, dd = grads(both)
    assert _zero(lp[-6:]) and _same(lp[:-6], clean[0])
    assert _same(ds, clean[1]) and _same(dd, clean[2])
    with pytest.raises(IndexError):                                       # (the forward's word, and the sides of the backward drop them too)
        NG.check_pending()
    NG.check_pending()                                                    # reported once
    with torch.no_grad():                                                 # the divisor counts pairs, not good pairs
        loss = npi.listwise_loss((zs.to(dev), zd.to(dev)), both.to(dev), exclude=known, scale=SCALE)
    want = ref.loss(ref.expected((n_src, n_dst, F), 63, True)[0], 69)
    assert abs(float(loss) - float(want)) <= GRAD_REL * abs(float(want))
    with pytest.raises(IndexError):
        NG.check_pending()
    empty = npi.link_log_softmax((zs.to(dev), zd.to(dev)), torch.zeros((2, 0), dtype=torch.int64, device=dev))
    assert empty.shape == (0,)
    assert float(npi.listwise_loss((zs.to(dev), zd.to(dev)), torch.zeros((2, 0), dtype=torch.int64, device=dev))) == 0.0
    NG.check_pending()


# ---- the masking is real ---------------------------------------------------------------------------------------------------------------
def test_an_excluded_target_that_outscores_everything_is_ignored(dev):
    NG.check_pending()
    n_src, n_dst, F, scale = 20, 300, 32, 0.5
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=6)
    s, t, hot = 3, 10, 50
    top = float((zs[s] @ zd.t()).abs().max())
    zd[hot] = zs[s] * ((top + 20.0 / scale) / float(zs[s] @ zs[s]))        # beats every other target of s by >= 20 / scale
    q = torch.cat([torch.tensor([[s], [t]]), ref.queries(n_src, n_dst, 64, seed=6)], 1)
    u = ref.upstream(65, seed=6)
    ex = torch.tensor([[s, 7], [hot, 8]])
    want = ref.link_log_softmax(zs.double(), zd.double(), q, ex, True, scale, u)
    unmasked = ref.link_log_softmax(zs.double(), zd.double(), q, None, True, scale)[0]
    assert float(want[0][0] - unmasked[0]) > 15.0                         # a kernel that fails to mask is off by about 20
    got = _run(dev, zs, zd, q, u, ex.to(dev), scale=scale)
    _within(got, want[:3], "an excluded hot target")
    # the target itself listed in `exclude` is still in its own denominator
    ex2 = torch.tensor([[s, 7, s], [hot, 8, t]])
    got2 = _run(dev, zs, zd, q, u, ex2.to(dev), scale=scale)
    _within(got2, ref.link_log_softmax(zs.double(), zd.double(), q, ex2, True, scale, u)[:3], "the target excluded")
    assert _same(got2[0][:1], got[0][:1])
    NG.check_pending()


def test_one_id_space_with_and_without_loops(dev):
    NG.check_pending()
    n, F, scale = 65, 16, 0.25
    z = tref.real_tables(n, n, F, seed=7)[0]                               # <z_v, z_v> = |z_v|^2: every row is its own best partner
    ex = tref.edges(n, n, 3 * n, seed=7)
    q = ref.queries(n, n, 130, seed=7)
    q[:, 1::8] = q[0, 1::8]                                                # queries (v, v)
    u = ref.upstream(130, seed=7)
    got = {}
    for loops in (True, False):
        want = ref.link_log_softmax(z.double(), None, q, ex, loops, scale, u)
        got[loops] = _run(dev, z, None, q, u, ex.to(dev), scale=scale, allow_loops=loops)
        _within(got[loops], want[:3], ("one id space, loops", loops))
    assert float((got[True][0] - got[False][0]).abs().max()) > 1e-2
    assert _same(got[True][0][1::8], got[False][0][1::8])                  # (v, v) as the target is in either way
    NG.check_pending()


# ---- extreme scores, NaN -------------------------------------------------------------------------------------------------------------------
def test_extreme_scores_stay_finite(dev):
    NG.check_pending()
    n_src, n_dst, F = 30, 200, 16
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=8)
    zs = zs * (80.0 / float((zs @ zd.t()).abs().max()))                    # |x| reaches 80: exp(x) alone overflows nowhere, exp(2 x) would
    q = ref.queries(n_src, n_dst, 130, seed=8)
    u = ref.upstream(130, seed=8)
    want = ref.link_log_softmax(zs.double(), zd.double(), q, None, True, 1.0, u)
    assert float(want[0].min()) < -60.0
    lp, ds, dd = _run(dev, zs, zd, q, u, scale=1.0)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(ds).all()) and bool(torch.isfinite(dd).all())
    _within((lp,), (want[0],), "extreme scores")
    NG.check_pending()


def test_a_nan_candidate_makes_lp_nan_and_is_reported(dev):
    NG.check_pending()
    zs, zd = tref.real_tables(65, 127, 3, seed=9)
    q = torch.stack([torch.arange(65), torch.arange(65) % 10])
    ex = torch.tensor([[3, 3, 40], [9, 10, 9]])
    clean = _run(dev, zs, zd, q, None, ex.to(dev), scale=SCALE)[0]
    NG.check_pending()
    zd[9, 2] = float("nan")
    lp = _run(dev, zs, zd, q, None, ex.to(dev), scale=SCALE)[0]
    spared = torch.zeros(65, dtype=torch.bool)
    spared[[3, 40]] = True                                                 # the queries that exclude target 9
    assert bool(torch.isnan(lp.cpu()[~spared]).all())
    assert _same(lp.cpu()[spared], clean.cpu()[spared])
    with pytest.raises(ValueError, match="NaN"):
        NG.check_pending()
    one = torch.tensor([[3], [9]])                                         # ... but as the target it is in although excluded
    assert bool(torch.isnan(_run(dev, zs, zd, one, None, ex.to(dev), scale=SCALE)[0]).all())
    with pytest.raises(ValueError, match="link_log_softmax"):
        NG.check_pending()


# ---- views -----------------------------------------------------------------------------------------------------------------------------------
def test_pitched_and_misaligned_views(dev):
    NG.check_pending()
    n_src, n_dst, F = 65, 300, 64
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=5)
    ex = tref.edges(n_src, n_dst, 200, seed=5)
    q = ref.queries(n_src, n_dst, 130, seed=5)
    u = ref.upstream(130, seed=5)
    base = _run(dev, zs, zd, q, u, ex.to(dev), scale=SCALE)
    want = ref.link_log_softmax(zs.double(), zd.double(), q, ex, True, SCALE, u)[:3]
    _within(base, want, "contiguous")
    for pad in (4, 5):                                                    # a 16-byte pitch (the fast form) and one that is not
        bs = torch.full((n_src, F + pad), 99.0, device=dev)
        bd = torch.full((n_dst, F + pad), 99.0, device=dev)
        bs[:, :F], bd[:, :F] = zs.to(dev), zd.to(dev)
        vs, vd = bs[:, :F].requires_grad_(), bd[:, :F].requires_grad_()
        assert vs.stride(0) == F + pad and not vs.is_contiguous()
        lp = npi.link_log_softmax((vs, vd), q.to(dev), exclude=ex.to(dev), scale=SCALE)
        assert _same(lp, base[0]), ("pitch", pad)
        (lp * u.to(dev)).sum().backward()
        _within((lp, vs.grad, vd.grad), want, ("pitch", pad))
    flat_s = torch.zeros(n_src * F + 1, device=dev)                       # a base 4 bytes past a 16-byte boundary: the guarded form
    flat_d = torch.zeros(n_dst * F + 1, device=dev)
    vs, vd = flat_s[1:].view(n_src, F), flat_d[1:].view(n_dst, F)
    vs.copy_(zs)
    vd.copy_(zd)
    assert vs.data_ptr() % 16 == 4 and vd.data_ptr() % 16 == 4
    for tables, what in (((vs, vd), "misaligned base"), ((vs, zd.to(dev)), "one misaligned table")):
        assert _same(npi.link_log_softmax(tables, q.to(dev), exclude=ex.to(dev), scale=SCALE), base[0]), what
    NG.check_pending()


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------------------
def test_calls_repeat_bitwise_and_queries_may_be_permuted_and_repeated(dev):
    NG.check_pending()
    shape = (130, 1000, 260)
    zs, zd, ex, q, u = ref.inputs(shape, 200)
    known = npi.KnownLinks(ex.to(dev), shape[:2])
    for splits in (0, 3):
        first = _run(dev, zs, zd, q, u, known, scale=SCALE, splits=splits)
        again = _run(dev, zs, zd, q, u, known, scale=SCALE, splits=splits)
        assert all(_same(a, b) for a, b in zip(first, again)), splits
        with torch.no_grad():
            z = (zs.to(dev), zd.to(dev))
            assert _same(npi.listwise_loss(z, q.to(dev), exclude=known, scale=SCALE, splits=splits),
                         npi.listwise_loss(z, q.to(dev), exclude=known, scale=SCALE, splits=splits))
        g = torch.Generator().manual_seed(2)
        perm = torch.randperm(200, generator=g)
        assert _same(_run(dev, zs, zd, q[:, perm], None, known, scale=SCALE, splits=splits)[0], first[0][perm.to(dev)])
        rep = torch.tensor([3, 3, 199, 0, 3, 64, 63, 0])
        assert _same(_run(dev, zs, zd, q[:, rep], None, known, scale=SCALE, splits=splits)[0], first[0][rep.to(dev)])
    NG.check_pending()


# ---- consistency with the neighbours ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "real"])
def test_a_full_enumeration_sums_to_one_and_orders_as_link_ranks_counts(dev, kind):
    """one source, no exclusion, every target queried: the probabilities sum to 1 and -lp orders the targets as the ``greater``
    counts of ``link_ranks`` do -- on the integer tables (ties everywhere) equal counts mean bit-equal lp"""
    NG.check_pending()
    n_src, n_dst, F = 3, 449, 8
    zs, zd = (tref.int_tables if kind == "exact" else tref.real_tables)(n_src, n_dst, F, seed=12)
    q = torch.stack([torch.full((n_dst,), 1, dtype=torch.int64), torch.arange(n_dst)])
    z = (zs.to(dev), zd.to(dev))
    lp = npi.link_log_softmax(z, q.to(dev), scale=SCALE).double().cpu()
    assert abs(float(torch.exp(lp).sum()) - 1.0) <= n_dst * 2.0 ** -22
    greater = npi.link_ranks(z, q.to(dev)).greater.cpu()
    order = torch.argsort(greater, stable=True)
    g, l = greater[order].tolist(), lp[order].tolist()
    ties = 0
    for i in range(1, n_dst):
        if g[i] == g[i - 1]:
            ties += 1
            assert l[i] == l[i - 1], (i, g[i], l[i], l[i - 1])
        else:
            assert l[i] < l[i - 1], (i, g[i - 1], g[i], l[i - 1], l[i])
    assert (ties > 100) if kind == "exact" else (ties == 0)
    NG.check_pending()


def test_gae_listwise_loss_is_the_functional_form(dev):
    NG.check_pending()
    model = npi.GAE(torch.nn.Identity())
    zs, zd, ex, q, _ = ref.inputs((65, 129, 65), 65)
    z, pos, known = (zs.to(dev), zd.to(dev)), q.to(dev), ex.to(dev)
    with torch.no_grad():
        assert _same(model.listwise_loss(z, pos), npi.listwise_loss(z, pos, exclude=pos))
        assert _same(model.listwise_loss(z, pos, known, scale=SCALE), npi.listwise_loss(z, pos, exclude=known, scale=SCALE))
        kl = npi.KnownLinks(known, (65, 129))
        assert _same(model.listwise_loss(z, pos, kl, scale=SCALE), npi.listwise_loss(z, pos, exclude=known, scale=SCALE))
        one = zs.to(dev)
        pos1 = ref.queries(65, 65, 65, seed=1).to(dev)
        assert _same(model.listwise_loss(one, pos1, scale=SCALE), npi.listwise_loss(one, pos1, exclude=pos1, scale=SCALE, allow_loops=False))
        assert not _same(model.listwise_loss(one, pos1, scale=SCALE), npi.listwise_loss(one, pos1, exclude=pos1, scale=SCALE))
    a = zs.to(dev).requires_grad_()
    model.listwise_loss(a, pos1, scale=SCALE).backward()
    want = ref.link_log_softmax(zs.double(), None, pos1.cpu(), pos1.cpu(), False, SCALE, torch.full((65,), -1.0 / 65))
    _within((a.grad,), (want[1],), "GAE.listwise_loss, one id space")
    NG.check_pending()


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
def test_listwise_loss_forward_under_capture(dev):
    """the forward (``torch.no_grad()``, a ``KnownLinks``) inside ``torch.cuda.graph`` on one stream, replayed twice"""
    NG.check_pending()
    shape = (130, 1000, 260)
    zs, zd, ex, q, _ = ref.inputs(shape, 200)
    z, qd = (zs.to(dev), zd.to(dev)), q.to(dev)
    known = npi.KnownLinks(ex.to(dev), shape[:2])
    with torch.no_grad():
        eager = npi.listwise_loss(z, qd, exclude=known, scale=SCALE)
        eager_lp = npi.link_log_softmax(z, qd, exclude=known, scale=SCALE)
        NG.check_pending()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=stream):
            loss = npi.listwise_loss(z, qd, exclude=known, scale=SCALE)
            lp = npi.link_log_softmax(z, qd, exclude=known, scale=SCALE)
        for _ in range(2):
            loss.fill_(7.0)
            lp.fill_(7.0)
            cg.replay()
            torch.cuda.synchronize()
            assert _same(loss, eager) and _same(lp, eager_lp)
    NG.check_pending()
