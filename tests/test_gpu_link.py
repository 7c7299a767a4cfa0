"""``npi.pair_scores`` / ``npi.link_loss`` / ``npi.InnerProductDecoder`` / ``npi.GAE`` on the GPU against the fp64 restatement
``tests/_link_ref.py`` (checked against the literal PyG composition by ``tests/test_link_cpu.py``).

The bar is the project's: ``_util.rel_max <= _util.GRAD_REL`` (1e-5 of the largest reference entry).  An f32 dot over F <= 260
terms of random sign carries about eps sqrt(F) ~ 1e-6 of the largest logit, so the bar leaves a factor of about ten; the ``gae``
parity cases keep the logits within +-4 (asserted), beyond which ``1 - s`` loses digits in float32 -- PyG's formula, not the
kernel.  ``test_link_cpu.py`` measures the same formulas in float32 torch on these very inputs: at most 6e-7."""
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import functional as F_
from npi_gnn_amd import graph as NG
import _link_ref as ref
from _util import GRAD_REL, rel_max

pytestmark = pytest.mark.gpu

_REF = {}


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


# ---- pair_scores / InnerProductDecoder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ref.F_CASES)
def test_pair_scores_logits_and_both_gradients(dev, F):
    """every lane width and chunk count x every tail of the group of eight and the block of 64, n_src != n_dst, a random upstream
    gradient"""
    zs, zd = ref.tables(F)
    for M in ref.M_CASES:
        src, dst = ref.pair_list(M)
        up = torch.randn(M, generator=torch.Generator().manual_seed(M))
        x64 = ref.logits(zs.double(), zd.double(), src, dst)
        d_src, d_dst = ref.table_grads(zs.double(), zd.double(), src, dst, up.double())
        a, b = _leaf(zs, dev), _leaf(zd, dev)
        ei = torch.stack([src, dst]).to(dev)
        x = npi.pair_scores((a, b), ei, size=(ref.N_SRC, ref.N_DST))
        assert x.shape == (M,) and x.dtype == torch.float32
        x.backward(up.to(dev))
        _close(x, x64, ("logits", F, M))
        _close(a.grad, d_src, ("dZ_src", F, M))
        _close(b.grad, d_dst, ("dZ_dst", F, M))


@pytest.mark.parametrize("sigmoid", [True, False])
def test_inner_product_decoder(dev, sigmoid):
    zs, zd = ref.tables(64)
    src, dst = ref.pair_list(1000)
    up = torch.randn(1000, generator=torch.Generator().manual_seed(3)).double()
    x64 = ref.logits(zs.double(), zd.double(), src, dst)
    s64 = torch.sigmoid(x64)
    want = s64 if sigmoid else x64
    g64 = up * s64 * (1 - s64) if sigmoid else up
    d_src, d_dst = ref.table_grads(zs.double(), zd.double(), src, dst, g64)
    a, b = _leaf(zs, dev), _leaf(zd, dev)
    out = npi.InnerProductDecoder()((a, b), torch.stack([src, dst]).to(dev), sigmoid=sigmoid)
    out.backward(up.float().to(dev))
    _close(out, want, "decoder output")
    _close(a.grad, d_src, "dZ_src")
    _close(b.grad, d_dst, "dZ_dst")


# ---- link_loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gae", "bce"])
@pytest.mark.parametrize("F", ref.F_CASES)
def test_link_loss_value_and_both_gradients(dev, F, kind):
    zs, zd = ref.tables(F)
    for M in ref.M_CASES:
        src, dst = ref.pair_list(M)
        ei = torch.stack([src, dst]).to(dev)
        for n_pos in ref.n_pos_cases(M):
            upstream = 1.0 if n_pos else -2.5                              # (the n_pos = 0 cases: a non-unit upstream gradient)
            want = _want((F, M, n_pos, kind), zs, zd, src, dst, n_pos, kind, upstream=upstream)
            assert float(want["logits"].abs().max()) <= 4.0
            a, b = _leaf(zs, dev), _leaf(zd, dev)
            loss = npi.link_loss((a, b), ei[:, :n_pos], ei[:, n_pos:], loss=kind)
            assert loss.shape == () and loss.dtype == torch.float32
            (loss * upstream).backward()
            _close(loss, want["loss"], ("loss", F, M, n_pos))
            _close(a.grad, want["d_src"], ("dZ_src", F, M, n_pos))
            _close(b.grad, want["d_dst"], ("dZ_dst", F, M, n_pos))


@pytest.mark.parametrize("kind", ["gae", "bce"])
def test_pitched_tables_at_a_four_byte_offset(dev, kind):
    """views of wider buffers whose rows start 4 bytes off a 16-byte boundary, with an odd pitch: F = 64 would take 16-byte lanes, these
    rows cannot -- the one-float-per-lane path over a pitch -- and the results agree with the reference all the same"""
    zs, zd = ref.tables(64)
    src, dst = ref.pair_list(1000)
    want = _want((64, 1000, 333, kind), zs, zd, src, dst, 333, kind)
    wide_s, wide_d = torch.zeros(ref.N_SRC, 71, device=dev), torch.zeros(ref.N_DST, 69, device=dev)
    wide_s[:, 1:65], wide_d[:, 1:65] = zs.to(dev), zd.to(dev)
    wide_s.requires_grad_(True), wide_d.requires_grad_(True)
    a, b = wide_s[:, 1:65], wide_d[:, 1:65]
    assert a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 4 and a.stride(0) == 71 and not a.is_contiguous()
    ei = torch.stack([src, dst]).to(dev)
    x = npi.pair_scores((a.detach(), b.detach()), ei)
    _close(x, want["logits"], "logits")
    loss = npi.link_loss((a, b), ei[:, :333], ei[:, 333:], loss=kind)
    loss.backward()
    _close(loss, want["loss"], "loss")
    _close(wide_s.grad[:, 1:65], want["d_src"], "dZ_src")
    _close(wide_d.grad[:, 1:65], want["d_dst"], "dZ_dst")
    assert float(wide_s.grad[:, :1].abs().max()) == 0 and float(wide_s.grad[:, 65:].abs().max()) == 0


@pytest.mark.parametrize("kind", ["gae", "bce"])
def test_three_hundred_pairs_of_one_source_and_repeated_pairs_accumulate(dev, kind):
    zs, zd = ref.tables(256)
    src, dst = ref.hub_pairs()
    want = _want(("hub", kind), zs, zd, src, dst, 150, kind)
    a, b = _leaf(zs, dev), _leaf(zd, dev)
    ei = torch.stack([src, dst]).to(dev)
    loss = npi.link_loss((a, b), ei[:, :150], ei[:, 150:], loss=kind)
    loss.backward()
    _close(loss, want["loss"], "loss")
    _close(a.grad, want["d_src"], "dZ_src")
    _close(b.grad, want["d_dst"], "dZ_dst")


@pytest.mark.parametrize("kind", ["gae", "bce"])
def test_one_id_space(dev, kind):
    """one table for both ends (a tensor, and the pair of the same tensor): both terms of dZ in one segmented sum; loops (v, v) and
    repeated pairs included"""
    z = ref.tables(64, 30, 30)[0]
    src, dst = ref.pair_list(200, 30, 30)
    src[:5] = dst[:5]
    want = _want(("one", kind), z, z, src, dst, 70, kind, upstream=0.5)
    ei = torch.stack([src, dst]).to(dev)
    grads = []
    for form in ("tensor", "pair"):
        a = _leaf(z, dev)
        loss = npi.link_loss(a if form == "tensor" else (a, a), ei[:, :70], ei[:, 70:], loss=kind)
        (loss * 0.5).backward()
        _close(loss, want["loss"], "loss")
        _close(a.grad, want["d_src"] + want["d_dst"], "dZ")
        grads.append(a.grad)
    assert torch.equal(grads[0], grads[1])
    a = _leaf(z, dev)
    up = torch.randn(200, generator=torch.Generator().manual_seed(8))
    x = npi.pair_scores(a, ei)
    x.backward(up.to(dev))
    d_src, d_dst = ref.table_grads(z.double(), z.double(), src, dst, up.double())
    _close(x, want["logits"], "logits")
    _close(a.grad, d_src + d_dst, "dZ of pair_scores")


def test_only_the_table_that_requires_grad_gets_a_side_and_no_grad_builds_nothing(dev, monkeypatch):
    zs, zd = ref.tables(64)
    src, dst = ref.pair_list(1000)
    want = _want((64, 1000, 333, "gae"), zs, zd, src, dst, 333, "gae")
    ei = torch.stack([src, dst]).to(dev)
    built = []
    real = F_.build_side
    monkeypatch.setattr(F_, "build_side", lambda key, val, n_rows, n_cols, **kw: built.append((n_rows, n_cols)) or real(key, val, n_rows, n_cols, **kw))
    with torch.no_grad():
        loss = npi.link_loss((zs.to(dev), zd.to(dev)), ei[:, :333], ei[:, 333:])
        x = npi.pair_scores((zs.to(dev), zd.to(dev)), ei)
    _close(loss, want["loss"], "loss")
    _close(x, want["logits"], "logits")
    assert built == []
    a, b = _leaf(zs, dev, grad=False), _leaf(zd, dev)
    npi.link_loss((a, b), ei[:, :333], ei[:, 333:]).backward()
    assert a.grad is None and built == [(ref.N_DST, ref.N_SRC)]            # the by-target side alone
    _close(b.grad, want["d_dst"], "dZ_dst")
    a, b = _leaf(zs, dev), _leaf(zd, dev, grad=False)
    npi.link_loss((a, b), ei[:, :333], ei[:, 333:]).backward()
    assert b.grad is None and built[1:] == [(ref.N_SRC, ref.N_DST)]
    _close(a.grad, want["d_src"], "dZ_src")


# ---- extreme logits ---------------------------------------------------------------------------------------------------------------------
def _raw(zs, zd, src, dst, n_pos, kind, dev):
    """(logits, coef, loss) of one launch"""
    pairs = F_._PairList(torch.stack([src, dst]).to(dev), zs.size(0), zd.size(0), "test")
    return F_._pair_score_launch(zs.to(dev), zd.to(dev), pairs, n_pos, F_.PAIR_LOSSES[kind], True, True, True)


def test_bce_at_logits_of_sixty_is_finite_and_accurate(dev):
    zs, zd, src, dst = ref.extreme_tables()
    n_pos = src.numel() // 3
    want = _want(("extreme", "bce"), zs, zd, src, dst, n_pos, "bce")
    assert float(want["logits"].max()) > 59.99 and float(want["logits"].min()) < -59.99
    x, coef, loss = _raw(zs, zd, src, dst, n_pos, "bce", dev)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(coef).all())
    _close(x, want["logits"], "logits")
    _close(loss, want["loss"], "loss")
    _close(coef, want["coef"], "coef")


def test_gae_at_logits_of_sixty_is_finite_with_the_right_signs(dev):
    zs, zd, src, dst = ref.extreme_tables()
    n_pos = src.numel() // 3
    x, coef, loss = _raw(zs, zd, src, dst, n_pos, "gae", dev)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(coef).all()) and float(loss) > 0
    assert bool((coef[:n_pos] <= 0).all()) and bool((coef[n_pos:] >= 0).all())
    a, b = _leaf(zs, dev), _leaf(zd, dev)
    ei = torch.stack([src, dst]).to(dev)
    npi.link_loss((a, b), ei[:, :n_pos], ei[:, n_pos:]).backward()
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())


def test_no_pairs_and_empty_parts(dev):
    zs, zd = ref.tables(64)
    a, b = _leaf(zs, dev), _leaf(zd, dev)
    none = torch.empty((2, 0), dtype=torch.int64, device=dev)
    for kind in ("gae", "bce"):
        loss = npi.link_loss((a, b), none, none, loss=kind)
        assert float(loss.detach()) == 0.0
        loss.backward()
        assert float(a.grad.abs().max()) == 0 and float(b.grad.abs().max()) == 0
    assert npi.pair_scores((a, b), none).shape == (0,)


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gae", "bce"])
def test_bitwise_reproducible_and_equal_with_a_prebuilt_graph(dev, kind):
    zs, zd = ref.tables(256, 300, 200, seed=2)
    src, dst = ref.pair_list(5000, 300, 200)
    ei = torch.stack([src, dst]).to(dev)
    z1 = ref.tables(256, 300, 300, seed=3)[0]
    ei1 = torch.stack(ref.pair_list(5000, 300, 300, seed=1)).to(dev)

    def run(tables, pairs, prebuilt):
        leaves = [_leaf(t, dev) for t in tables]
        z = leaves[0] if len(leaves) == 1 else tuple(leaves)
        n = leaves[0].size(0), leaves[-1].size(0)
        if prebuilt:
            loss = npi.link_loss(z, npi.BipartiteGraph(pairs, n), loss=kind, num_pos=2000)
        else:
            loss = npi.link_loss(z, pairs[:, :2000], pairs[:, 2000:], loss=kind)
        loss.backward()
        coef = F_._pair_score_launch(tables[0].to(dev), tables[-1].to(dev), F_._PairList(pairs, *n, "test"), 2000, F_.PAIR_LOSSES[kind],
                                     False, True, False)[1]
        return [loss.detach(), coef] + [t.grad for t in leaves]

    for tables, pairs in (((zs, zd), ei), ((z1,), ei1)):
        first = run(tables, pairs, False)
        for other in (run(tables, pairs, False), run(tables, pairs, True)):
            for u, v in zip(first, other):
                assert torch.equal(u, v)
    # pair_scores under an upstream gradient, raw list and prebuilt graph
    up = torch.randn(5000, generator=torch.Generator().manual_seed(4)).to(dev)
    outs = []
    for pairs in (ei, ei, npi.BipartiteGraph(ei, (300, 200))):
        a, b = _leaf(zs, dev), _leaf(zd, dev)
        x = npi.pair_scores((a, b), pairs)
        x.backward(up)
        outs.append((x.detach(), a.grad, b.grad))
    for other in outs[1:]:
        for u, v in zip(outs[0], other):
            assert torch.equal(u, v)


# ---- ids out of range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [0, 1])
def test_an_id_outside_its_table_scores_zero_and_is_reported(dev, row):
    NG.check_pending()
    zs, zd = ref.tables(64)
    src, dst = ref.pair_list(1000)
    ei = torch.stack([src, dst]).to(dev)
    bad = ei.clone()
    at = torch.tensor([0, 63, 64, 500, 999], device=dev)
    bad[row, at] = torch.tensor([-1, (ref.N_SRC, ref.N_DST)[row], 2 ** 40, -2 ** 40, 2 ** 31], device=dev)
    keep = torch.ones(1000, dtype=torch.bool, device=dev)
    keep[at] = False
    with torch.no_grad():
        clean = npi.pair_scores((zs.to(dev), zd.to(dev)), ei)
        NG.check_pending()                                                # nothing to report
        x = npi.pair_scores((zs.to(dev), zd.to(dev)), bad)
    assert bool((x[at] == 0).all()) and torch.equal(x[keep], clean[keep])
    with pytest.raises(IndexError, match="pair"):
        NG.check_pending()
    NG.check_pending()                                                    # reported once
    logits, coef, loss = _raw(zs, zd, bad[0].cpu(), bad[1].cpu(), 333, "bce", dev)
    assert bool((coef[at] == 0).all()) and bool(torch.isfinite(loss))
    ok = _raw(zs, zd, src[keep.cpu()], dst[keep.cpu()], 330, "bce", dev)[2]          # positions 0, 63 and 64 were positives
    _close(loss * 1000, ok * 995, "the loss without the bad pairs' terms")
    with pytest.raises(IndexError, match="pair"):
        NG.check_pending()


# ---- through a layer ----------------------------------------------------------------------------------------------------------------
def _layer_case(dev):
    g = torch.Generator().manual_seed(21)
    ei = torch.stack([torch.randint(0, 500, (4000,), generator=g), torch.randint(0, 300, (4000,), generator=g)]).to(dev)
    x_src = (torch.randn(500, 64, generator=g) * 0.5).to(dev)
    torch.manual_seed(5)
    conv = npi.SAGEConv(64, 64).to(dev)
    return ei, x_src, conv


def _torch_loss(x, n_pos, kind):
    if kind == "gae":
        return -torch.log(torch.sigmoid(x[:n_pos]) + ref.EPS).mean() - torch.log(1 - torch.sigmoid(x[n_pos:]) + ref.EPS).mean()
    y = (torch.arange(x.numel(), device=x.device) < n_pos).float()
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y)


@pytest.mark.parametrize("kind", ["gae", "bce"])
def test_layer_gradients_equal_the_torch_composition(dev, kind):
    """bipartite SAGEConv(64, 64) over 500 x 300 nodes and 4,000 edges; the loss over its output: dW and db against the torch
    composition (z[i] * z[j]).sum(1) with the same loss on the same device output"""
    ei, x_src, conv = _layer_case(dev)
    neg = npi.negative_sampling(ei, (500, 300), seed=1)
    both = torch.cat([ei, neg], 1)
    z_dst = conv((x_src, None), ei, size=(500, 300))
    loss = npi.link_loss((x_src, z_dst), ei, neg, loss=kind)
    loss.backward()
    dw, db = conv.weight.grad.clone(), conv.bias.grad.clone()
    conv.zero_grad()
    z2 = conv((x_src, None), ei, size=(500, 300))
    assert torch.equal(z2, z_dst)
    want = _torch_loss((x_src[both[0]] * z2[both[1]]).sum(1), 4000, kind)
    want.backward()
    _close(loss, want, "loss")
    _close(dw, conv.weight.grad, "dW")
    _close(db, conv.bias.grad, "db")


def test_twenty_sgd_steps_of_recon_loss_lower_the_loss(dev):
    ei, x_src, conv = _layer_case(dev)
    model = npi.GAE(conv)
    opt = torch.optim.SGD(model.parameters(), lr=3.0)
    graph = npi.BipartiteGraph(ei, (500, 300))
    losses = []
    for _ in range(20):
        opt.zero_grad()
        z_dst = model.encode((x_src, None), graph, size=(500, 300))
        loss = model.recon_loss((x_src, z_dst), ei)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert model.draw == 20 and losses[-1] < losses[0], losses


# ---- GAE.recon_loss draws its own negatives -----------------------------------------------------------------------------------------------
def test_recon_loss_draws_the_negatives_of_negative_sampling(dev):
    zs, zd = ref.tables(64, 300, 40)
    z1 = ref.tables(64, 300, 300, seed=1)[0]
    pos = torch.stack(ref.pair_list(600, 300, 40)).to(dev)
    a, b, c = zs.to(dev), zd.to(dev), z1.to(dev)
    for kind in ("gae", "bce"):
        model, twin = npi.GAE(torch.nn.Identity()), npi.GAE(torch.nn.Identity())
        got = model.recon_loss((a, b), pos, loss=kind, seed=7)
        by_hand = npi.link_loss((a, b), pos, npi.negative_sampling(pos, (300, 40), seed=7), loss=kind)
        assert torch.equal(got, by_hand) and model.draw == 1
        assert torch.equal(twin.recon_loss((a, b), pos, loss=kind, seed=7), got)
        second = model.recon_loss((a, b), pos, loss=kind, seed=7)                      # draw 1: other negatives
        assert not torch.equal(second, got) and model.draw == 2
        assert torch.equal(twin.recon_loss((a, b), pos, loss=kind, seed=7), second)
        assert torch.equal(model.recon_loss((a, b), pos, pos, loss=kind), npi.link_loss((a, b), pos, pos, loss=kind)) and model.draw == 2
        # one id space: (v, v) is never a negative
        one = npi.GAE(torch.nn.Identity())
        neg = npi.NegativeSampler(pos, 300, seed=7, allow_loops=False).pairs(draw=0)
        assert neg.shape == (2, 600) and bool((neg[0] != neg[1]).all())
        assert torch.equal(one.recon_loss(c, pos, loss=kind, seed=7), npi.link_loss(c, pos, neg, loss=kind))
