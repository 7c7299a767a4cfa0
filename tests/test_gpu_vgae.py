"""VGAE on the device: Rule N's noise against its float64 restatement, the fused sample + KL launch and its backward against the
float64 torch composition with the reference noise injected, the identities that hold bit for bit (replays, KL alone, pitched views,
row prefixes, the backward's noise being the forward's), the distribution of the device noise, the ``VGAE`` module (one id space and
the pair form, evaluation mode, the draw counter, a captured step with a tick word) and ``ARGA`` / ``ARGVA``.

Tolerances (``U = 2^-24``, the unit roundoff of float32):
  noise    |eps - eps_ref| <= 16 U max(1, |eps_ref|): u1 and theta are bit-identical, logf / sincosf / sqrtf within 2 ulp each, r <= 5.77
  z        |z - z_ref| <= 2 U |z_ref| + 24 U sigma_ref max(1, |eps_ref|): the noise bound, expf within 2 ulp, one fma rounding
  kl       |kl - kl_ref| <= 8 U 0.5 / n_total sum (1 + |lv| + mu^2 + exp(lv)): three f32 roundings and one expf per term, the sum in fp64
  gradients: the project's bar, ``rel_max <= GRAD_REL``"""
import math

import numpy as np
import pytest
import torch

import _gauss_ref as R
import npi_gnn_amd as npi
from _util import GRAD_REL, rel_max
from npi_gnn_amd import functional as NF

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED, DRAW = 11, 2
SHAPES = [(1, 1), (3, 2), (257, 33), (300, 64), (300, 6), (5000, 8), (0, 16)]
CASES = [(N, F, False) for N, F in SHAPES] + [(300, 64, True), (300, 6, True)]      # True: the halves of one [N, 2 F] tensor
IDS = [f"{N}x{F}{'-pitched' if p else ''}" for N, F, p in CASES]
PLANTED = {1: 12.0, 2: 10.0, 4: 0.0}                    # flat positions of logvar: clamped, exactly MAX_LOGVAR, zero


def _tables(N, F, planted=PLANTED):
    """``mu ~ N(0, 1)``, ``logvar ~ U(-6, 3)`` with the planted values where they fit, float32 on the host"""
    g = torch.Generator().manual_seed(1000 * N + F)
    mu = torch.randn(N, F, generator=g)
    logvar = torch.rand(N, F, generator=g) * 9 - 6
    for pos, v in planted.items():
        if pos < N * F:
            logvar.view(-1)[pos] = v
    return mu, logvar


def _on_device(mu, logvar, dev, pitched, grad=False):
    """the tables as the call sees them: two tensors, or the two column blocks of one ``[N, 2 F]`` tensor (which is returned too)"""
    if not pitched:
        m, l = mu.to(dev).requires_grad_(grad), logvar.to(dev).requires_grad_(grad)
        return m, l, None
    h = torch.cat([mu, logvar], 1).to(dev).requires_grad_(grad)
    F = mu.size(1)
    return h[:, :F], h[:, F:], h


def _eps_ref(N, F, seed=SEED, draw=DRAW, tick=0, table=0):
    return torch.from_numpy(R.eps_np(seed, draw, tick, table, N, F)).reshape(N, F)


def _z_bound(z_ref, lv64, eps_ref):
    return 2 * U * z_ref.abs() + 24 * U * torch.exp(0.5 * lv64) * eps_ref.abs().clamp(min=1.0)


def _kl_bound(mu64, lv64, n_total):
    return 8 * U * 0.5 / n_total * float((1 + lv64.abs() + mu64 ** 2 + lv64.exp()).sum())


# ---- the noise on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", SHAPES)
@pytest.mark.parametrize("table,tick", [(0, None), (1, 5)])
def test_noise_on_the_device_is_rule_n(dev, N, F, table, tick):
    word = None if tick is None else torch.tensor([tick], dtype=torch.int64, device=dev)
    got = NF.gaussian_noise(N, F, NF.GaussianNoise(SEED, DRAW, word), table=table, device=dev)
    assert got.shape == (N, F) and got.dtype == torch.float32 and got.device.type == "cuda"
    ref = _eps_ref(N, F, tick=0 if tick is None else tick, table=table)
    if N == 0:
        return
    ratio = ((got.cpu().double() - ref).abs() / (U * ref.abs().clamp(min=1.0))).max()
    print(f"noise {N}x{F} table {table} tick {tick}: max |eps - eps_ref| / (U max(1, |eps_ref|)) = {float(ratio):.3f}")
    assert float(ratio) <= 16


def test_noise_of_a_row_prefix_is_the_prefix_and_a_pitched_output_is_the_same(dev):
    rule = NF.GaussianNoise(SEED, DRAW)
    for F in (64, 33):
        whole = NF.gaussian_noise(700, F, rule, device=dev)
        assert torch.equal(NF.gaussian_noise(123, F, rule, device=dev), whole[:123])
        assert torch.equal(NF.gaussian_noise(700, F, rule, device=dev), whole)
    # columns: a narrower table is the column prefix, through the 16-byte and the scalar lanes alike
    assert torch.equal(NF.gaussian_noise(700, 33, rule, device=dev), NF.gaussian_noise(700, 64, rule, device=dev)[:, :33])


def test_more_tiles_than_the_grid_holds(dev):
    """2063 tiles for 2048 workgroups: the last rows are written in a workgroup's second pass"""
    N, F = 132000, 64
    assert N * F // 4096 + 1 > 2048
    rule = NF.GaussianNoise(SEED, DRAW)
    eps = NF.gaussian_noise(N, F, rule, device=dev)
    rows = np.concatenate([np.arange(3), np.arange(N - 300, N)])
    ref = torch.from_numpy(R.eps_np(SEED, DRAW, 0, 0, rows, F))
    got = eps[torch.from_numpy(rows).to(dev)].cpu().double()
    assert float(((got - ref).abs() / (U * ref.abs().clamp(min=1.0))).max()) <= 16
    # sigma = exp(0) = 1 exactly: z is the one rounding of mu + eps; the KL term against float64 on the device
    mu = torch.randn(N, F, device=dev)
    logvar = torch.zeros(N, F, device=dev)
    z, kl = NF.reparametrize_kl(mu, logvar, rule)
    assert torch.equal(z, (mu.double() + eps.double()).float())
    kl_ref = 0.5 / N * float((mu.double() ** 2).sum())
    assert abs(float(kl) - kl_ref) <= _kl_bound(mu.double(), logvar.double(), N)
    assert torch.equal(NF.reparametrize_kl(mu, logvar, sample=False)[1], kl)


def test_distribution_of_the_device_noise(dev):
    eps = NF.gaussian_noise(4096, 64, NF.GaussianNoise(0, 0), device=dev).cpu().numpy()
    mean, var, ks, top = R.distribution_figures(eps)
    print(f"device noise: |mean| sqrt(n) {mean:.3f}  |var - 1| sqrt(n / 2) {var:.3f}  KS sqrt(n) {ks:.3f}  max |eps| {top:.3f}")
    assert mean <= 4 and var <= 4 and ks <= 1.63 and top <= R.EPS_MAX


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F,pitched", CASES, ids=IDS)
def test_forward_matches_float64_with_the_reference_noise(dev, N, F, pitched):
    mu, logvar = _tables(N, F)
    m, l, _ = _on_device(mu, logvar, dev, pitched)
    z, kl = NF.reparametrize_kl(m, l, NF.GaussianNoise(SEED, DRAW))
    assert z.shape == (N, F) and z.dtype == torch.float32 and kl.shape == () and kl.dtype == torch.float32
    if N == 0:
        assert float(kl) == 0.0
        return
    eps = _eps_ref(N, F)
    z_ref, kl_ref = R.reparam_kl(mu.double(), logvar.double(), eps)
    lv64 = logvar.double().clamp(max=10.0)
    excess = ((z.cpu().double() - z_ref).abs() / _z_bound(z_ref, lv64, eps)).max()
    kl_err, kl_tol = abs(float(kl) - float(kl_ref.detach())), _kl_bound(mu.double(), lv64, N)
    print(f"forward {N}x{F}{' pitched' if pitched else ''}: max |dz| / bound {float(excess):.3f}  |dkl| / bound {kl_err / kl_tol:.3f}")
    assert float(excess) <= 1 and kl_err <= kl_tol
    # the KL-only launch gives the same word, and z is mu there
    z0, kl0 = NF.reparametrize_kl(m, l, sample=False)
    assert z0 is m and torch.equal(kl0, kl)
    # n_total: the mean over more rows than the table has
    kl2 = NF.reparametrize_kl(m, l, NF.GaussianNoise(SEED, DRAW), n_total=2 * N + 3)[1]
    assert abs(float(kl2) - float(kl_ref) * N / (2 * N + 3)) <= _kl_bound(mu.double(), lv64, 2 * N + 3)


@pytest.mark.parametrize("N,F", [(3, 2), (300, 64), (300, 6)])
def test_logvar_minus_infinity(dev, N, F):
    """``sigma = 0``: ``z == mu`` bitwise there, and ``kl = +inf`` as in PyG; the gradient of z is finite"""
    mu, logvar = _tables(N, F, planted={3: -math.inf, **PLANTED})
    m, l, _ = _on_device(mu, logvar, dev, False, grad=True)
    z, kl = NF.reparametrize_kl(m, l, NF.GaussianNoise(SEED, DRAW))
    assert float(kl.detach()) == math.inf
    assert torch.equal(z.detach().view(-1)[3].cpu(), mu.view(-1)[3])
    eps = _eps_ref(N, F)
    z_ref, _ = R.reparam_kl(mu.double(), logvar.double(), eps)
    assert float(((z.detach().cpu().double() - z_ref).abs() / _z_bound(z_ref, logvar.double().clamp(max=10.0), eps).clamp(min=1e-300)).max()) <= 1
    z.sum().backward()
    assert float(l.grad.view(-1)[3]) == 0.0 and bool(torch.isfinite(l.grad).all()) and bool((m.grad == 1).all())


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _upstream(N, F):
    g = torch.Generator().manual_seed(N + 7 * F)
    sign = torch.randint(0, 2, (N, F), generator=g) * 2.0 - 1.0
    return sign * (0.5 + torch.rand(N, F, generator=g)), 1.7          # |g_z| in [0.5, 1.5): the noise can be read back from d logvar


@pytest.mark.parametrize("part", ["kl", "z", "both"])
@pytest.mark.parametrize("N,F,pitched", CASES, ids=IDS)
def test_backward_matches_float64(dev, N, F, pitched, part):
    mu, logvar = _tables(N, F)
    gz, gk = _upstream(N, F)
    mr, lr = mu.double().requires_grad_(True), logvar.double().requires_grad_(True)
    z_ref, kl_ref = R.reparam_kl(mr, lr, _eps_ref(N, F))
    m, l, h = _on_device(mu, logvar, dev, pitched, grad=True)
    z, kl = NF.reparametrize_kl(m, l, NF.GaussianNoise(SEED, DRAW))
    # an output that takes no part is ABSENT from the graph (its gradient is None, not zero)
    loss_ref = sum(([(z_ref * gz.double()).sum()] if part != "kl" else []) + ([gk * kl_ref] if part != "z" else []))
    loss = sum(([(z * gz.to(dev)).sum()] if part != "kl" else []) + ([gk * kl] if part != "z" else []))
    if N == 0:
        loss.backward()
        return
    loss_ref.backward()
    loss.backward()
    d_mu, d_lv = (h.grad[:, :F], h.grad[:, F:]) if pitched else (m.grad, l.grad)
    print(f"backward {N}x{F} {part}: d_mu {rel_max(d_mu, mr.grad):.3g}  d_logvar {rel_max(d_lv, lr.grad):.3g}")
    assert rel_max(d_mu, mr.grad) <= GRAD_REL and rel_max(d_lv, lr.grad) <= GRAD_REL
    if N * F > 1:
        assert float(logvar.view(-1)[1]) == 12.0 and float(d_lv.reshape(-1)[1]) == 0.0            # clamped: exactly zero
    if N * F > 2 and part != "kl":
        assert float(d_lv.reshape(-1)[2]) != 0.0                                                  # exactly MAX_LOGVAR: not clamped
    if part == "z":
        assert torch.equal(d_mu.cpu(), gz)                                                        # d mu IS g_z


# ---- identities that hold bit for bit ----------------------------------------------------------------------------------------------
def _step(dev, mu, logvar, rule, pitched=False, table=0, gz=None, gk=1.7):
    m, l, h = _on_device(mu, logvar, dev, pitched, grad=True)
    z, kl = NF.reparametrize_kl(m, l, rule, table=table)
    gz = _upstream(*mu.shape)[0] if gz is None else gz
    ((z * gz.to(dev)).sum() + gk * kl).backward()
    F = mu.size(1)
    d_mu, d_lv = (h.grad[:, :F], h.grad[:, F:]) if pitched else (m.grad, l.grad)
    return z.detach(), kl.detach(), d_mu, d_lv


@pytest.mark.parametrize("N,F", [(300, 64), (300, 6), (257, 33)])
def test_replays_and_pitched_views_are_bitwise_equal(dev, N, F):
    mu, logvar = _tables(N, F)
    rule = NF.GaussianNoise(SEED, DRAW)
    first = _step(dev, mu, logvar, rule)
    for other in (_step(dev, mu, logvar, NF.GaussianNoise(SEED, DRAW)), _step(dev, mu, logvar, rule, pitched=True)):
        for a, b in zip(first, other):
            assert torch.equal(a, b)
    # a pitched pair whose rows are NOT 16-byte aligned (the scalar lanes) computes the same as the 16-byte lanes
    wide = torch.zeros(N, 2 * F + 1, device=dev)
    wide[:, :F], wide[:, F + 1:] = mu.to(dev), logvar.to(dev)
    z, kl = NF.reparametrize_kl(wide[:, :F], wide[:, F + 1:], rule)
    assert torch.equal(z, first[0]) and torch.equal(kl, first[1])
    # a different draw, tick or table changes z (and nothing else changes kl)
    tick = torch.tensor([1], dtype=torch.int64, device=dev)
    tick0 = torch.zeros(1, dtype=torch.int64, device=dev)
    assert torch.equal(_step(dev, mu, logvar, NF.GaussianNoise(SEED, DRAW, tick0))[0], first[0])           # a tick word of 0: no word
    for changed in (_step(dev, mu, logvar, NF.GaussianNoise(SEED, DRAW + 1)), _step(dev, mu, logvar, NF.GaussianNoise(SEED + 1, DRAW)),
                    _step(dev, mu, logvar, NF.GaussianNoise(SEED, DRAW, tick)), _step(dev, mu, logvar, rule, table=1)):
        assert not torch.equal(changed[0], first[0]) and torch.equal(changed[1], first[1])


@pytest.mark.parametrize("N,F", [(300, 64), (257, 33)])
def test_the_forward_and_the_backward_draw_the_noise_of_npi_gauss_noise(dev, N, F):
    mu, logvar = _tables(N, F, planted={})
    rule = NF.GaussianNoise(SEED, DRAW)
    eps = NF.gaussian_noise(N, F, rule, device=dev).cpu().double()
    # sigma = 1: z is the ONE rounding of mu + eps
    z1, _ = NF.reparametrize_kl(mu.to(dev), torch.zeros(N, F, device=dev), rule)
    assert torch.equal(z1.cpu(), (mu.double() + eps).float())
    # any sigma: one fma rounding and expf's 2 ulp
    sigma = torch.exp(0.5 * logvar.double())
    z, _ = NF.reparametrize_kl(mu.to(dev), logvar.to(dev), rule)
    want = mu.double() + eps * sigma
    assert bool(((z.cpu().double() - want).abs() <= U * want.abs() + 4 * U * (eps * sigma).abs()).all())
    # the backward: with d z alone, d logvar = 0.5 g_z eps sigma -- the eps it implies is the forward's.  The tick has moved on
    # between the forward and the backward: the backward redraws under the value the forward saw
    tick = torch.tensor([3], dtype=torch.int64, device=dev)
    ticked = NF.GaussianNoise(SEED, DRAW, tick)
    eps3 = NF.gaussian_noise(N, F, ticked, device=dev).cpu().double()
    gz = _upstream(N, F)[0]
    l = logvar.to(dev).requires_grad_(True)
    z3, _ = NF.reparametrize_kl(mu.to(dev), l, ticked)
    tick.add_(1)
    (z3 * gz.to(dev)).sum().backward()
    implied = l.grad.cpu().double() / (0.5 * gz.double() * sigma)
    assert rel_max(implied, eps3) <= GRAD_REL
    assert not torch.equal(eps3, eps)


# ---- the modules ------------------------------------------------------------------------------------------------------------------
class _Encoder(torch.nn.Module):
    """one projection for both heads: the halves of its output are mu and logvar (pitched views, read in place)"""

    def __init__(self, fin=16, fout=8):
        super().__init__()
        self.lin = torch.nn.Linear(fin, 2 * fout)
        self.fout = fout

    def reset_parameters(self):
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            self.lin.weight.copy_((torch.rand(self.lin.weight.shape, generator=g) - 0.5) * 0.5)
            self.lin.bias.zero_()
            self.lin.bias[self.fout:] = -3.0                   # sigma about 0.22: the logits of the decoder stay small

    def forward(self, x, edge_index=None):
        h = self.lin(x)
        return h[:, :self.fout], h[:, self.fout:]


class _PairEncoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.src, self.dst = _Encoder(16, 8), _Encoder(12, 8)

    def forward(self, x, edge_index=None):
        return self.src(x[0]), self.dst(x[1])


def _graph(n_src, n_dst, E, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    neg = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    return pos, neg


def _recon_ref(z_src, z_dst, pos, neg):
    """PyG 1.4.2 ``GAE.recon_loss`` in the dtype of the tables"""
    def prob(ei):
        return torch.sigmoid((z_src[ei[0]] * z_dst[ei[1]]).sum(dim=1))
    return -torch.log(prob(pos) + 1e-15).mean() - torch.log(1 - prob(neg) + 1e-15).mean()


def test_vgae_step_matches_the_float64_composition(dev):
    N, E = 200, 600
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(1)) * 0.3
    pos, neg = _graph(N, N, E, 2)
    model = npi.VGAE(_Encoder(), seed=SEED).to(dev)
    model.draw_noise = DRAW
    W, b = model.encoder.lin.weight, model.encoder.lin.bias
    z = model.encode(x.to(dev), pos.to(dev))
    assert model.draw_noise == DRAW + 1 and z.shape == (N, 8)
    loss = model.recon_loss(z, pos.to(dev), neg.to(dev)) + model.kl_loss() / N
    loss.backward()
    Wr, br = W.detach().cpu().double().requires_grad_(True), b.detach().cpu().double().requires_grad_(True)
    h = x.double() @ Wr.t() + br
    z_ref, kl_ref = R.reparam_kl(h[:, :8], h[:, 8:], _eps_ref(N, 8))
    loss_ref = _recon_ref(z_ref, z_ref, pos, neg) + kl_ref / N
    loss_ref.backward()
    print(f"VGAE step: loss {float(loss.detach()):.6f} ref {float(loss_ref.detach()):.6f}  dW {rel_max(W.grad, Wr.grad):.3g}  db {rel_max(b.grad, br.grad):.3g}")
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-5 * abs(float(loss_ref.detach()))
    assert rel_max(W.grad, Wr.grad) <= GRAD_REL and rel_max(b.grad, br.grad) <= GRAD_REL
    assert torch.equal(model.__mu__, model.encoder(x.to(dev))[0]) and model.kl_loss() is model.kl_loss()
    # setting the counters back replays the step bit for bit, negatives drawn on the device included
    def step():
        model.zero_grad()
        zz = model.encode(x.to(dev), pos.to(dev))
        total = model.recon_loss(zz, pos.to(dev)) + model.kl_loss() / N
        total.backward()
        return zz.detach().clone(), total.detach().clone(), W.grad.clone(), b.grad.clone()
    model.draw_noise, model.draw = 0, 0
    one, two = step(), step()
    assert (model.draw_noise, model.draw) == (2, 2) and not torch.equal(one[0], two[0])
    model.draw_noise, model.draw = 0, 0
    for a, c in zip(one, step()):
        assert torch.equal(a, c)
    # evaluation: z is mu, nothing is drawn; kl_loss() then comes from a KL-only launch and is the training launch's word
    kl_train = model.kl_loss().detach().clone()
    model.eval()
    z_eval = model.encode(x.to(dev), pos.to(dev))
    assert model.draw_noise == 1 and torch.equal(z_eval, model.encoder(x.to(dev))[0]) and torch.equal(model.kl_loss(), kl_train)
    # explicit arguments: a KL-only launch over them
    mu, logvar = _tables(300, 6)
    kl = model.kl_loss(mu.to(dev), logvar.to(dev))
    kl_ref = R.reparam_kl(mu.double(), logvar.double(), torch.zeros(300, 6).double())[1]
    assert abs(float(kl) - float(kl_ref.detach())) <= _kl_bound(mu.double(), logvar.double().clamp(max=10.0), 300)
    # everything of GAE runs on the result
    auc, ap = model.test(z_eval, pos.to(dev), neg.to(dev))
    assert 0.0 <= float(auc) <= 1.0 and 0.0 <= float(ap) <= 1.0
    prob, ids = model.predict(z_eval, 3, pos.to(dev))
    assert prob.shape == (N, 3) and ids.shape == (N, 3)


def test_vgae_pair_form(dev):
    n_src, n_dst, E = 50, 30, 200
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n_src, 16, generator=g) * 0.3, torch.randn(n_dst, 12, generator=g) * 0.3)
    pos, neg = _graph(n_src, n_dst, E, 4)
    model = npi.VGAE(_PairEncoder(), seed=SEED).to(dev)
    model.draw_noise = DRAW
    z = model.encode((x[0].to(dev), x[1].to(dev)))
    assert isinstance(z, tuple) and z[0].shape == (n_src, 8) and z[1].shape == (n_dst, 8) and model.draw_noise == DRAW + 1
    n = n_src + n_dst
    loss = model.recon_loss(z, pos.to(dev), neg.to(dev)) + model.kl_loss() / n
    loss.backward()
    params = [model.encoder.src.lin.weight, model.encoder.src.lin.bias, model.encoder.dst.lin.weight, model.encoder.dst.lin.bias]
    refs = [p.detach().cpu().double().requires_grad_(True) for p in params]
    hs, hd = x[0].double() @ refs[0].t() + refs[1], x[1].double() @ refs[2].t() + refs[3]
    zs, kls = R.reparam_kl(hs[:, :8], hs[:, 8:], _eps_ref(n_src, 8, table=0), n_total=n)
    zd, kld = R.reparam_kl(hd[:, :8], hd[:, 8:], _eps_ref(n_dst, 8, table=1), n_total=n)
    kl_ref = kls + kld
    (_recon_ref(zs, zd, pos, neg) + kl_ref / n).backward()
    # z and kl against float64 over the encoder's own float32 outputs: table 0 for the sources, table 1 for the targets
    mus, lvs = ([t.detach().cpu().double() for t in pair] for pair in (model.__mu__, model.__logvar__))
    kl_dev_ref = 0.0
    for t in (0, 1):
        eps = _eps_ref(mus[t].size(0), 8, table=t)
        z_ref, kl_t = R.reparam_kl(mus[t], lvs[t], eps, n_total=n)
        assert float(((z[t].detach().cpu().double() - z_ref).abs() / _z_bound(z_ref, lvs[t], eps)).max()) <= 1, t
        kl_dev_ref += float(kl_t)
    # (each table's bound, then the two float32 words and their float32 sum: three more roundings of at most the whole)
    assert abs(float(model.kl_loss().detach()) - kl_dev_ref) <= _kl_bound(torch.cat(mus), torch.cat(lvs), n) + 3 * U * kl_dev_ref
    assert abs(float(model.kl_loss().detach()) - float(kl_ref.detach())) <= 1e-5 * float(kl_ref.detach())
    for p, r in zip(params, refs):
        assert rel_max(p.grad, r.grad) <= GRAD_REL
    kl_pair = model.kl_loss(model.__mu__, model.__logvar__)
    assert torch.equal(kl_pair, model.kl_loss().detach())
    model.eval()
    z_eval = model.encode((x[0].to(dev), x[1].to(dev)))
    assert torch.equal(z_eval[0], model.__mu__[0]) and torch.equal(z_eval[1], model.__mu__[1]) and model.draw_noise == DRAW + 1
    assert torch.equal(model.kl_loss(), kl_pair)


def test_captured_encode_draws_fresh_noise_per_replay(dev):
    N = 200
    x = (torch.randn(N, 16, generator=torch.Generator().manual_seed(1)) * 0.3).to(dev)
    tick = torch.zeros(1, dtype=torch.int64, device=dev)
    model = npi.VGAE(_Encoder(), seed=SEED, tick=tick).to(dev)

    def eager(t):
        tick.fill_(t)
        model.draw_noise = DRAW
        with torch.no_grad():
            return model.encode(x).clone(), model.kl_loss().clone()

    want = [eager(t) for t in range(3)]
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[1][0], want[2][0])
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):
            eager(0)
        tick.zero_()
        model.draw_noise = DRAW
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, stream=s):
            z = model.encode(x)
            kl = model.kl_loss()
            tick.add_(1)
    torch.cuda.current_stream(dev).wait_stream(s)
    tick.zero_()
    for t in range(3):
        graph.replay()
        torch.cuda.synchronize(dev)
        assert int(tick) == t + 1
        assert torch.equal(z, want[t][0]) and torch.equal(kl, want[t][1]), t


def test_arga_and_argva(dev):
    N = 200
    x = (torch.randn(N, 16, generator=torch.Generator().manual_seed(1)) * 0.3).to(dev)
    disc = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1))
    model = npi.ARGVA(_Encoder(), disc, seed=SEED).to(dev)
    z = model.encode(x)
    d = model.discriminator
    assert torch.equal(model.reg_loss(z), -torch.log(torch.sigmoid(d(z)) + 1e-15).mean())
    torch.manual_seed(3)
    got = model.discriminator_loss(z)
    torch.manual_seed(3)
    real, fake = torch.sigmoid(d(torch.randn_like(z))), torch.sigmoid(d(z.detach()))
    assert torch.equal(got, -torch.log(real + 1e-15).mean() - torch.log(1 - fake + 1e-15).mean())
    got.backward()
    assert model.encoder.lin.weight.grad is None and d[0].weight.grad is not None       # z is detached in the discriminator's loss
    # ARGVA's variational half is VGAE's
    plain = npi.VGAE(_Encoder(), seed=SEED).to(dev)
    assert torch.equal(plain.encode(x), z) and torch.equal(plain.kl_loss(), model.kl_loss())
    arga = npi.ARGA(lambda t: t[:, :8], torch.nn.Linear(8, 1).to(dev))
    assert torch.equal(arga.reg_loss(arga.encode(x)), -torch.log(torch.sigmoid(arga.discriminator(x[:, :8])) + 1e-15).mean())
