"""``npi.group_scores`` / ``npi.ranking_loss`` / ``GAE.ranking_loss`` on the GPU against the fp64 restatement ``tests/_group_ref.py``
(checked against the literal torch compositions by ``tests/test_group_loss_cpu.py``).

The bar is the project's: ``_util.rel_max <= _util.GRAD_REL`` (1e-5 of the largest reference entry).  ``test_group_loss_cpu.py``
measures the same formulas in float32 torch on these very inputs -- at most 9e-7, and 2.3e-6 on the softmax coefficients at logits
of +-60 -- so the bar leaves a factor of four and more to the kernel's different summation order.  The ``margin`` inputs keep every hinge 1e-3 off its kink (asserted there), a hundred times what
an f32 logit on these tables can be off by, so no kink flips between the device and the reference.  Tables of 37 x 23 rows."""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import functional as F_
from npi_gnn_amd import graph as NG
import _group_ref as ref
from _util import GRAD_REL, rel_max

pytestmark = pytest.mark.gpu

_REF = {}
KINDS = tuple(dict.fromkeys(k for k, _, _ in ref.cases()))


def _want(key, *args, **kw):
    """the fp64 reference of a case, computed once"""
    if key not in _REF:
        _REF[key] = ref.evaluate(*args, **kw)
    return _REF[key]


def _close(got, want, what):
    err = rel_max(got, want)
    assert err <= GRAD_REL, (what, err)


def _leaf(t, dev, grad=True):
    return t.to(dev).requires_grad_(grad)


def _raw(zs, zd, src, dst, neg, kind, margin, scale, dev):
    """(logits, coef, loss) of one launch"""
    groups = F_._GroupList(torch.stack([src, dst]).to(dev), neg.to(dev), zs.size(0), zd.size(0), "test")
    return F_._group_score_launch(zs.to(dev), zd.to(dev), groups, F_.GROUP_LOSSES[kind], margin, scale, True, True, True)


# ---- group_scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ref.F_CASES)
def test_group_scores_logits_and_both_gradients(dev, F):
    """every lane width and chunk count x every shape of the slot -> lane mapping, n_src != n_dst, a random upstream gradient whose
    values at the empty slots are NaN (they are ignored)"""
    for P, K in ref.SHAPES:
        zs, zd, src, dst, neg = ref.inputs(P, K, F, "bpr")
        x64, valid = ref.logits(zs.double(), zd.double(), src, dst, neg)
        up = torch.randn(P, 1 + K, generator=torch.Generator().manual_seed(P + K))
        d_src, d_dst = ref.table_grads(zs.double(), zd.double(), src, dst, neg, torch.where(valid, up, torch.zeros(())).double())
        up[~valid] = float("nan")
        a, b = _leaf(zs, dev), _leaf(zd, dev)
        x = npi.group_scores((a, b), torch.stack([src, dst]).to(dev), neg.to(dev))
        assert x.shape == (P, 1 + K) and x.dtype == torch.float32
        x.backward(up.to(dev))
        assert ref.rel_finite(x, x64) <= GRAD_REL, ("logits", F, P, K)
        _close(a.grad, d_src, ("dZ_src", F, P, K))
        _close(b.grad, d_dst, ("dZ_dst", F, P, K))
    NG.check_pending()                                                    # an empty slot is no bad id: nothing to report


def test_decoder_passthrough_and_k_equal_one_as_a_vector(dev):
    zs, zd, src, dst, neg = ref.inputs(33, 1, 64, "bpr")
    pos = torch.stack([src, dst]).to(dev)
    x = npi.group_scores((zs.to(dev), zd.to(dev)), pos, neg.to(dev))
    assert torch.equal(npi.group_scores((zs.to(dev), zd.to(dev)), pos, neg[:, 0].to(dev)), x)
    dec = npi.InnerProductDecoder()
    assert torch.equal(dec.group_scores((zs.to(dev), zd.to(dev)), pos, neg.to(dev)), x)
    prob = dec.group_scores((zs.to(dev), zd.to(dev)), pos, neg.to(dev), sigmoid=True)
    assert torch.equal(prob, torch.sigmoid(x)) and bool((prob[neg.to(dev)[:, 0] == -1, 1] == 0).all())


# ---- ranking_loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", ref.F_CASES)
def test_ranking_loss_value_and_both_gradients(dev, F, kind):
    for F_i, P, K, k, margin, scale in ref.parity_inputs():
        if (F_i, k) != (F, kind):
            continue
        zs, zd, src, dst, neg = ref.inputs(P, K, F, kind, margin, scale)
        up = ref.upstream_of(P, K, F)
        want = _want((F, P, K, kind, margin, scale), zs, zd, src, dst, neg, kind, margin, scale, upstream=up)
        a, b = _leaf(zs, dev), _leaf(zd, dev)
        loss = npi.ranking_loss((a, b), torch.stack([src, dst]).to(dev), neg.to(dev), loss=kind, margin=margin, scale=scale)
        assert loss.shape == () and loss.dtype == torch.float32
        (loss * up).backward()
        what = (F, P, K, kind, scale)
        _close(loss, want["loss"], ("loss",) + what)
        _close(a.grad, want["d_src"], ("dZ_src",) + what)
        _close(b.grad, want["d_dst"], ("dZ_dst",) + what)
        if K == 0:
            assert float(loss.detach()) == 0 and float(a.grad.abs().max()) == 0 and float(b.grad.abs().max()) == 0
    NG.check_pending()


@pytest.mark.parametrize("kind", KINDS)
def test_raw_launch_logits_coef_and_loss_together(dev, kind):
    """one launch asked for all three outputs: the coefficients against the reference's, exact zeros at the empty slots, and
    coef_0 = -(sum of the others)"""
    for P, K in ((33, 1), (9, 8), (6, 63)):
        zs, zd, src, dst, neg = ref.inputs(P, K, 64, kind, 1.0, 1.0)
        want = _want((64, P, K, kind, 1.0, 1.0, "raw"), zs, zd, src, dst, neg, kind, 1.0, 1.0)
        x, coef, loss = _raw(zs, zd, src, dst, neg, kind, 1.0, 1.0, dev)
        assert ref.rel_finite(x, want["logits"]) <= GRAD_REL
        _close(coef, want["coef"], "coef")
        _close(loss, want["loss"], "loss")
        assert bool((coef.cpu()[~want["valid"]] == 0).all())
        assert bool((coef[:, 0] <= 0).all()) and float((coef[:, 0] + coef[:, 1:].double().sum(1)).abs().max()) <= 1e-6 * float(coef.abs().max())


@pytest.mark.parametrize("kind", KINDS)
def test_pitched_tables_at_a_four_byte_offset_and_a_pitched_neg_view(dev, kind):
    """views of wider buffers whose rows start 4 bytes off a 16-byte boundary, with an odd pitch: F = 64 would take 16-byte lanes, these
    rows cannot -- the one-float-per-lane path over a pitch; ``neg_dst`` a column block of a wider id buffer (ld_neg > K)"""
    P, K = 9, 8
    zs, zd, src, dst, neg = ref.inputs(P, K, 64, kind)
    want = _want((64, P, K, kind, 1.0, 1.0, "raw"), zs, zd, src, dst, neg, kind, 1.0, 1.0)
    wide_s, wide_d = torch.zeros(ref.N_SRC, 71, device=dev), torch.zeros(ref.N_DST, 69, device=dev)
    wide_s[:, 1:65], wide_d[:, 1:65] = zs.to(dev), zd.to(dev)
    wide_s.requires_grad_(True), wide_d.requires_grad_(True)
    a, b = wide_s[:, 1:65], wide_d[:, 1:65]
    assert a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 4 and a.stride(0) == 71 and not a.is_contiguous()
    wide_n = torch.full((P, K + 5), 10 ** 9, dtype=torch.int64, device=dev)              # ids no table holds around the block
    wide_n[:, 2:2 + K] = neg.to(dev)
    nv = wide_n[:, 2:2 + K]
    assert nv.stride(0) == K + 5 and not nv.is_contiguous()
    pos = torch.stack([src, dst]).to(dev)
    x = npi.group_scores((a.detach(), b.detach()), pos, nv)
    assert ref.rel_finite(x, want["logits"]) <= GRAD_REL
    loss = npi.ranking_loss((a, b), pos, nv, loss=kind)
    loss.backward()
    _close(loss, want["loss"], "loss")
    _close(wide_s.grad[:, 1:65], want["d_src"], "dZ_src")
    _close(wide_d.grad[:, 1:65], want["d_dst"], "dZ_dst")
    assert float(wide_s.grad[:, :1].abs().max()) == 0 and float(wide_s.grad[:, 65:].abs().max()) == 0
    NG.check_pending()                                                    # nothing outside the block was read as an id


@pytest.mark.parametrize("kind", KINDS)
def test_one_id_space(dev, kind):
    """one table for both ends (a tensor, and the pair of the same tensor): both terms of dZ in one segmented sum"""
    z, src, dst, neg = ref.one_space_inputs(kind)
    want = _want(("one", kind), z, z, src, dst, neg, kind, upstream=0.5)
    pos, nd = torch.stack([src, dst]).to(dev), neg.to(dev)
    grads = []
    for form in ("tensor", "pair"):
        a = _leaf(z, dev)
        loss = npi.ranking_loss(a if form == "tensor" else (a, a), pos, nd, loss=kind)
        (loss * 0.5).backward()
        _close(loss, want["loss"], "loss")
        _close(a.grad, want["d_src"] + want["d_dst"], "dZ")
        grads.append(a.grad)
    assert torch.equal(grads[0], grads[1])


# ---- reproducibility and the independence of a group from its place in the list -------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_permuting_the_groups_permutes_the_outputs_bitwise_and_runs_repeat_bitwise(dev, kind):
    for P, K, F in ((33, 1, 64), (22, 2, 3), (9, 8, 260), (9, 31, 64)):
        zs, zd, src, dst, neg = ref.inputs(P, K, F, kind)
        perm = torch.randperm(P, generator=torch.Generator().manual_seed(P))
        x, coef, _ = _raw(zs, zd, src, dst, neg, kind, 1.0, 2.5 if kind != "margin" else 1.0, dev)
        xp, coefp, _ = _raw(zs, zd, src[perm], dst[perm], neg[perm], kind, 1.0, 2.5 if kind != "margin" else 1.0, dev)
        assert torch.equal(x[perm.to(dev)], xp) and torch.equal(coef[perm.to(dev)], coefp), (P, K, F)
        runs = []
        for order in (None, None, perm):
            s, d, n = (src, dst, neg) if order is None else (src[order], dst[order], neg[order])
            a, b = _leaf(zs, dev), _leaf(zd, dev)
            loss = npi.ranking_loss((a, b), torch.stack([s, d]).to(dev), n.to(dev), loss=kind)
            loss.backward()
            runs.append((loss.detach(), a.grad, b.grad))
        for u, v in zip(runs[0], runs[1]):
            assert torch.equal(u, v)                                      # the same call twice: bitwise
        for u, v in zip(runs[0], runs[2]):
            _close(v, u.double(), "permuted")                              # another order of the same sums


def test_only_the_table_that_requires_grad_gets_a_side_and_no_grad_builds_nothing(dev, monkeypatch):
    P, K = 9, 8
    zs, zd, src, dst, neg = ref.inputs(P, K, 64, "softmax")
    want = _want((64, P, K, "softmax", 1.0, 1.0, "raw"), zs, zd, src, dst, neg, "softmax", 1.0, 1.0)
    pos, nd = torch.stack([src, dst]).to(dev), neg.to(dev)
    built = []
    real = F_.build_side
    monkeypatch.setattr(F_, "build_side", lambda key, val, n_rows, n_cols, **kw: built.append((n_rows, n_cols)) or real(key, val, n_rows, n_cols, **kw))
    with torch.no_grad():
        loss = npi.ranking_loss((zs.to(dev), zd.to(dev)), pos, nd, loss="softmax")
        x = npi.group_scores((zs.to(dev), zd.to(dev)), pos, nd)
    _close(loss, want["loss"], "loss")
    assert ref.rel_finite(x, want["logits"]) <= GRAD_REL
    assert built == []
    a, b = _leaf(zs, dev, grad=False), _leaf(zd, dev)
    npi.ranking_loss((a, b), pos, nd, loss="softmax").backward()
    assert a.grad is None and built == [(ref.N_DST, ref.N_SRC)]            # the by-target side alone
    _close(b.grad, want["d_dst"], "dZ_dst")
    a, b = _leaf(zs, dev), _leaf(zd, dev, grad=False)
    npi.ranking_loss((a, b), pos, nd, loss="softmax").backward()
    assert b.grad is None and built[1:] == [(ref.N_SRC, ref.N_DST)]
    _close(a.grad, want["d_src"], "dZ_src")


# ---- extreme logits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_logits_of_sixty_times_a_scale_of_two_and_a_half(dev, kind):
    zs, zd, src, dst, neg = ref.extreme_groups()
    want = _want(("extreme", kind), zs, zd, src, dst, neg, kind, 1.0, 2.5)
    assert float(want["logits"].max()) > 59.99 and float(want["logits"].min()) < -59.99
    x, coef, loss = _raw(zs, zd, src, dst, neg, kind, 1.0, 2.5, dev)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(coef).all())
    _close(x, want["logits"], "logits")
    if kind != "margin":                                                  # (a hinge at |d| of 300 may sit on either side of its kink)
        _close(loss, want["loss"], "loss")
        _close(coef, want["coef"], "coef")


def test_no_groups(dev):
    zs, zd = ref.tables(64)
    a, b = _leaf(zs, dev), _leaf(zd, dev)
    pos = torch.empty((2, 0), dtype=torch.int64, device=dev)
    for K in (0, 4):
        neg = torch.empty((0, K), dtype=torch.int64, device=dev)
        for kind in KINDS:
            loss = npi.ranking_loss((a, b), pos, neg, loss=kind)
            assert float(loss.detach()) == 0.0
            loss.backward()
            assert float(a.grad.abs().max()) == 0 and float(b.grad.abs().max()) == 0
        assert npi.group_scores((a, b), pos, neg).shape == (0, 1 + K)


# ---- ids out of range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bad_ids_give_the_documented_zeros_and_are_reported_and_an_empty_slot_is_not(dev, kind):
    NG.check_pending()
    P, K = 21, 7
    zs, zd, src, dst, neg = ref.inputs(P, K, 64, kind)
    assert bool((neg == -1).any())
    x0, c0, l0 = _raw(zs, zd, src, dst, neg, kind, 1.0, 1.0, dev)
    NG.check_pending()                                                    # -1 slots: nothing to report
    # a corrupted id of n_dst: as an empty slot, but reported
    bad = neg.clone()
    col = int((bad[3] >= 0).nonzero()[0])
    bad[3, col] = ref.N_DST
    want = ref.evaluate(zs, zd, src, dst, bad, kind)
    x, coef, loss = _raw(zs, zd, src, dst, bad, kind, 1.0, 1.0, dev)
    assert float(x[3, col + 1]) == float("-inf") and float(coef[3, col + 1]) == 0
    assert ref.rel_finite(x, want["logits"]) <= GRAD_REL
    _close(coef, want["coef"], "coef")
    _close(loss, want["loss"], "loss")
    other = torch.ones(P, dtype=torch.bool)
    other[3] = False
    assert torch.equal(x[other.to(dev)], x0[other.to(dev)]) and torch.equal(coef[other.to(dev)], c0[other.to(dev)])
    with pytest.raises(IndexError, match="pair"):
        NG.check_pending()
    NG.check_pending()                                                    # reported once
    # a positive out of range drops its whole group
    for row, value in ((0, ref.N_SRC), (0, -1), (1, ref.N_DST), (1, -1), (1, 2 ** 40)):
        pos = torch.stack([src, dst])
        pos[row, 5] = value
        want = ref.evaluate(zs, zd, pos[0], pos[1], neg, kind)
        x, coef, loss = _raw(zs, zd, pos[0], pos[1], neg, kind, 1.0, 1.0, dev)
        assert bool((x[5] == 0).all()) and bool((coef[5] == 0).all())
        _close(loss, want["loss"], "loss")
        other = torch.ones(P, dtype=torch.bool)
        other[5] = False
        assert torch.equal(x[other.to(dev)], x0[other.to(dev)]) and torch.equal(coef[other.to(dev)], c0[other.to(dev)])
        with pytest.raises(IndexError, match="pair"):
            NG.check_pending()
    # through autograd: the bad slots add nothing to either table
    pos = torch.stack([src, dst])
    pos[0, 5] = ref.N_SRC
    want = ref.evaluate(zs, zd, pos[0], pos[1], bad, kind)
    a, b = _leaf(zs, dev), _leaf(zd, dev)
    npi.ranking_loss((a, b), pos.to(dev), bad.to(dev), loss=kind).backward()
    _close(a.grad, want["d_src"], "dZ_src")
    _close(b.grad, want["d_dst"], "dZ_dst")
    with pytest.raises(IndexError):
        NG.check_pending()


# ---- hard negatives from topk_links ---------------------------------------------------------------------------------------------------
def test_the_ids_of_topk_links_as_hard_negatives(dev):
    """k larger than some rows' candidate count: their last slots hold -1, which is the empty slot of Rule G"""
    zs, zd = ref.tables(64)
    g = torch.Generator().manual_seed(12)
    src = torch.randint(0, ref.N_SRC, (60,), generator=g)
    dst = torch.randint(0, ref.N_DST, (60,), generator=g)
    full = torch.stack([torch.full((ref.N_DST - 4,), 7), torch.arange(ref.N_DST - 4)])      # source 7 knows all targets but four
    known = torch.cat([torch.stack([src, dst]), full], 1)
    pos = torch.stack([torch.cat([src, torch.tensor([7, 7])]), torch.cat([dst, torch.tensor([0, 1])])])
    k = 8
    _, ids = npi.topk_links((zs.to(dev), zd.to(dev)), k, exclude=known.to(dev), rows=pos[0].to(dev))
    assert ids.shape == (62, k) and bool((ids[-1, 4:] == -1).all()) and bool((ids[:60] >= 0).any())
    for kind in KINDS:
        want = ref.evaluate(zs, zd, pos[0], pos[1], ids.cpu(), kind)
        loss = npi.ranking_loss((zs.to(dev), zd.to(dev)), pos.to(dev), ids, loss=kind)
        _close(loss, want["loss"], ("loss", kind))
    NG.check_pending()


# ---- GAE.ranking_loss -----------------------------------------------------------------------------------------------------------------
def test_gae_ranking_loss_draws_the_targets_of_corrupt(dev):
    zs, zd = ref.tables(64, 300, 40)
    z1 = ref.tables(64, 300, 300, seed=1)[0]
    pos = torch.stack(ref.link.pair_list(600, 300, 40)).to(dev)
    a, b, c = zs.to(dev), zd.to(dev), z1.to(dev)
    for kind in KINDS:
        model, twin = npi.GAE(torch.nn.Identity()), npi.GAE(torch.nn.Identity())
        got = model.ranking_loss((a, b), pos, num_neg=4, loss=kind, seed=7)
        neg = npi.NegativeSampler(pos, (300, 40), seed=7).corrupt(pos[0].repeat_interleave(4), draw=0).view(600, 4)
        assert torch.equal(got, npi.ranking_loss((a, b), pos, neg, loss=kind)) and model.draw == 1
        assert torch.equal(twin.ranking_loss((a, b), pos, num_neg=4, loss=kind, seed=7), got)
        second = model.ranking_loss((a, b), pos, num_neg=4, loss=kind, seed=7)          # draw 1: other targets
        assert not torch.equal(second, got) and model.draw == 2
        assert torch.equal(twin.ranking_loss((a, b), pos, num_neg=4, loss=kind, seed=7), second)
        given = model.ranking_loss((a, b), pos, loss=kind, neg_dst=neg, scale=2.0, margin=0.5)
        assert torch.equal(given, npi.ranking_loss((a, b), pos, neg, loss=kind, scale=2.0, margin=0.5)) and model.draw == 2
        # known_edge_index: the corrupted targets avoid ITS edges
        known = torch.cat([pos, torch.stack([pos[0], (pos[1] + 1) % 40])], 1)
        k_neg = npi.NegativeSampler(known, (300, 40), seed=7).corrupt(pos[0].repeat_interleave(4), draw=2).view(600, 4)
        assert torch.equal(model.ranking_loss((a, b), pos, num_neg=4, loss=kind, known_edge_index=known, seed=7),
                           npi.ranking_loss((a, b), pos, k_neg, loss=kind)) and model.draw == 3
        # one id space
        one = npi.GAE(torch.nn.Identity())
        n1 = npi.NegativeSampler(pos, 300, seed=7, allow_loops=False).corrupt(pos[0].repeat_interleave(2), draw=0).view(600, 2)
        assert torch.equal(one.ranking_loss(c, pos, num_neg=2, loss=kind, seed=7), npi.ranking_loss(c, pos, n1, loss=kind))
    NG.check_pending()


def test_twenty_sgd_steps_of_ranking_loss_lower_the_loss(dev):
    g = torch.Generator().manual_seed(21)
    ei = torch.stack([torch.randint(0, 500, (4000,), generator=g), torch.randint(0, 300, (4000,), generator=g)]).to(dev)
    x_src = (torch.randn(500, 64, generator=g) * 0.5).to(dev)
    torch.manual_seed(5)
    model = npi.GAE(npi.SAGEConv(64, 64).to(dev))
    opt = torch.optim.SGD(model.parameters(), lr=1.0)
    graph = npi.BipartiteGraph(ei, (500, 300))
    losses = []
    for _ in range(20):
        opt.zero_grad()
        z_dst = model.encode((x_src, None), graph, size=(500, 300))
        loss = model.ranking_loss((x_src, z_dst), ei, num_neg=4, loss="softmax")
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert model.draw == 20 and losses[-1] < losses[0], losses
