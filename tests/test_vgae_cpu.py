"""The seeded standard normal (Rule N) and the ``VGAE`` surface without a GPU: the rule's known answers, its int and numpy forms agreeing,
the distribution and independence of the reference noise, the four new symbols with the unchanged ABI version, every entry point
refusing arguments outside its contract with ``NPI_ERR_ARG`` before anything is launched (the arguments are checked on the host; no
pointer is followed), and the Python-side argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _gauss_ref as R
import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import functional as NF

NPI_ERR_ARG = -1
A = 0x10000                      # a 16-byte aligned stand-in for every pointer: never dereferenced by a refused call
KEY = 12345
SAMPLE, KL = _lib.NPI_GAUSS_SAMPLE, _lib.NPI_GAUSS_KL
NEW = ("npi_gauss_workspace_bytes", "npi_gauss_sample_kl", "npi_gauss_sample_kl_bwd", "npi_gauss_noise")


def test_known_answers():
    assert R.epoch_seed(0, 0) == 0xE220A8397B1DCDAF
    assert R.root(0, 0) == 0x17B5B595BF33339A
    assert R.root_t(0, 0, 0) == 0xA7EF72C3DB16C2D7 and R.root_t(0, 0, 1) == 0xA8877CAA7F09CAB9
    rt = R.root_t(0, 0, 0)
    assert (R.word(rt, 0, 0, 0), R.word(rt, 0, 0, 1)) == (0x889234032688D558, 0x069A7CAF18CE8061)
    assert (R.word(rt, 0, 1, 0), R.word(rt, 0, 1, 1)) == (0x205B65805DFF0D2E, 0x01CA425F2169D826)
    assert R.word(rt, 1, 0, 0) == 0xE4E0ADF25A413B08
    want = [1.1176605005754783, 0.08659600134496356, -1.0901547752580947, -2.475222608957373]
    assert [R.eps_int(0, 0, 0, 0, 0, c) for c in range(4)] == pytest.approx(want, rel=1e-15, abs=0)
    assert R.eps_np(0, 0, 0, 0, 1, 4)[0].tolist() == pytest.approx(want, rel=1e-15, abs=0)
    assert float(R.TWO_PI_F32) == float(np.float32(2 * math.pi))


def test_the_numpy_form_and_the_int_form_agree():
    for seed, draw, tick, table in ((0, 0, 0, 0), (12345, 7, 3, 1), (1, 0, 2 ** 40, 0)):
        rows = [0, 1, 77, 2 ** 31 - 3]
        w = R.words_np(seed, draw, tick, table, rows, 4)
        rt = R.root_t(seed, draw, tick)
        assert w.tolist() == [[R.word(rt, table, r, p) for p in range(4)] for r in rows]
        eps = R.eps_np(seed, draw, tick, table, rows, 7)                    # odd F: the last word's second value is cut off
        assert eps.shape == (4, 7)
        for i, r in enumerate(rows):
            for c in range(7):
                assert eps[i, c] == pytest.approx(R.eps_int(seed, draw, tick, table, r, c), rel=1e-14, abs=1e-300)
    # an int N means rows 0 .. N - 1; a prefix of the rows and of the columns is a slice
    assert np.array_equal(R.eps_np(3, 1, 0, 0, 5, 8)[:3, :5], R.eps_np(3, 1, 0, 0, 3, 5))


def test_the_package_holds_the_same_key():
    rule = NF.GaussianNoise(0, 0)
    assert rule.key & R.M64 == R.epoch_seed(0, 0) and rule.tick is None
    assert NF.GaussianNoise(12345, 7).key & R.M64 == R.epoch_seed(12345, 7)


@pytest.fixture(scope="module")
def eps0():
    return R.eps_np(0, 0, 0, 0, 4096, 64)


def test_distribution_of_the_reference_noise(eps0):
    n = eps0.size
    assert n == 262144
    mean, var, ks, top = R.distribution_figures(eps0)
    print(f"|mean| sqrt(n) {mean:.3f}  |var - 1| sqrt(n / 2) {var:.3f}  KS sqrt(n) {ks:.3f}  max |eps| {top:.3f}")
    assert mean <= 4 and var <= 4
    assert ks <= 1.63                                                       # the 1 % point
    assert top <= R.EPS_MAX == math.sqrt(48 * math.log(2))                  # the rule's bound: u1 >= 2^-24


def test_independence_of_tables_draws_ticks_and_rows(eps0):
    others = {"table 1": R.eps_np(0, 0, 0, 1, 4096, 64), "draw 1": R.eps_np(0, 1, 0, 0, 4096, 64), "tick 1": R.eps_np(0, 0, 1, 0, 4096, 64)}
    for name, other in others.items():
        assert not np.array_equal(other, eps0)
        fig = R.corr_figure(eps0, other)
        print(name, f"{fig:.3f}")
        assert fig <= 4, name
    assert R.corr_figure(eps0[:-1], eps0[1:]) <= 4                          # a row against the next one
    assert R.corr_figure(eps0[:, 0::2], eps0[:, 1::2]) <= 4                 # the two values of one word


def test_symbols_and_abi_version():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    assert lib.npi_abi_version() == 4                                       # an additive change
    assert (SAMPLE, KL) == (1, 2)


def test_workspace_query():
    lib = _lib.load()
    ws = lib.npi_gauss_workspace_bytes
    assert ws(0, 16) == 16 and ws(1, 1) == 16 and ws(1024, 4) == 16          # one tile of 1024 groups of four columns
    assert ws(1025, 4) == 16 and ws(1025, 5) == 8 * 3 + 8                    # 2 and 3 tiles, rounded up to 16 bytes
    assert ws(1 << 20, 256) == 8 * ((1 << 20) * 64 // 1024)
    for N, F in ((-1, 4), (2 ** 31 - 1, 4), (4, 0), (4, -1), (4, 2 ** 31 - 1), (2 ** 31 - 2, 2 ** 31 - 2)):
        assert ws(N, F) == -1, (N, F)


def _fwd(lib, N=100, F=8, ld_mu=None, ld_lv=None, n_total=None, tick=None, table=0, flags=SAMPLE | KL, z=A, ld_z=None, kl=A,
         partials=A, partials_bytes=1 << 20, mu=A, logvar=A):
    return lib.npi_gauss_sample_kl(mu, F if ld_mu is None else ld_mu, logvar, F if ld_lv is None else ld_lv, N, F,
                                   N if n_total is None else n_total, 10.0, KEY, tick, table, flags, z, F if ld_z is None else ld_z, kl,
                                   partials, partials_bytes, None)


def _bwd(lib, N=100, F=8, ld_mu=None, ld_lv=None, n_total=None, table=0, flags=SAMPLE | KL, g_z=A, ld_gz=None, g_kl=A, d_mu=A,
         ld_dmu=None, d_logvar=A, ld_dlv=None, mu=A, logvar=A):
    return lib.npi_gauss_sample_kl_bwd(mu, F if ld_mu is None else ld_mu, logvar, F if ld_lv is None else ld_lv, N, F,
                                       N if n_total is None else n_total, 10.0, KEY, None, table, flags, g_z,
                                       F if ld_gz is None else ld_gz, g_kl, d_mu, F if ld_dmu is None else ld_dmu, d_logvar,
                                       F if ld_dlv is None else ld_dlv, None)


def _noise(lib, N=100, F=8, table=0, eps=A, ld=None, n_total=None):           # (n_total: of the shared size cases; no such argument)
    return lib.npi_gauss_noise(N, F, KEY, None, table, eps, F if ld is None else ld, None)


BIG = 2 ** 31 - 1
SIZES = {"N < 0": dict(N=-1), "N = 2^31 - 1": dict(N=BIG, n_total=BIG), "F = 0": dict(F=0), "F < 0": dict(F=-3), "F = 2^31 - 1": dict(F=BIG),
         "table 2": dict(table=2), "table -1": dict(table=-1)}
FLAGS = {"no flags": dict(flags=0), "unknown flag": dict(flags=4), "unknown flag beside known ones": dict(flags=SAMPLE | KL | 8)}
TOTALS = {"n_total < N": dict(n_total=99), "n_total < 0": dict(N=0, n_total=-1), "n_total = 2^31 - 1": dict(n_total=BIG)}


def test_arguments_outside_the_contract_are_refused_before_a_launch():
    lib = _lib.load()
    cases = {
        "npi_gauss_sample_kl": (_fwd, {
            **SIZES, **FLAGS, **TOTALS, "ld_mu < F": dict(ld_mu=7), "ld_lv < F": dict(ld_lv=7), "ld_z < F": dict(ld_z=7),
            "KL without kl": dict(kl=None), "KL without partials": dict(partials=None), "KL alone without kl": dict(flags=KL, kl=None, z=None),
            "partials too short": dict(N=2000, partials_bytes=16), "partials misaligned": dict(partials=A + 8),
            "SAMPLE without z": dict(z=None), "SAMPLE alone without z": dict(flags=SAMPLE, z=None, kl=None, partials=None),
            "null mu": dict(mu=None), "null logvar": dict(logvar=None)}),
        "npi_gauss_sample_kl_bwd": (_bwd, {
            **SIZES, **FLAGS, **TOTALS, "ld_mu < F": dict(ld_mu=7), "ld_lv < F": dict(ld_lv=7), "ld_gz < F": dict(ld_gz=7),
            "ld_dmu < F": dict(ld_dmu=7), "ld_dlv < F": dict(ld_dlv=7), "null mu": dict(mu=None), "null logvar": dict(logvar=None),
            "no output": dict(d_mu=None, d_logvar=None)}),
        "npi_gauss_noise": (_noise, {**SIZES, "ld < F": dict(ld=7), "null eps": dict(eps=None)}),
    }
    for who, (call, shapes) in cases.items():
        for name, kw in shapes.items():
            assert call(lib, **kw) == NPI_ERR_ARG, (who, name)
            msg = lib.npi_last_error().decode()
            assert msg.startswith(who + ":"), (who, name, msg)
    # n_total < 1 with N > 0 cannot be reached past n_total >= N; n_total == 0 is fine with N == 0, where nothing is launched ...
    assert _bwd(lib, N=0, n_total=0) == 0 and _noise(lib, N=0) == 0 and _noise(lib, N=0, eps=None) == 0
    assert _fwd(lib, N=0, n_total=0, flags=SAMPLE, kl=None, partials=None) == 0
    # ... but the checks come first
    assert _bwd(lib, N=0, flags=0) == NPI_ERR_ARG and _noise(lib, N=0, table=3) == NPI_ERR_ARG
    assert _fwd(lib, N=0, flags=KL, kl=None) == NPI_ERR_ARG


def test_python_argument_checks():
    for bad in (dict(seed="x"), dict(seed=True), dict(seed=0.5), dict(seed=0, draw=-1), dict(seed=0, draw=1.0), dict(seed=0, tick=3),
                dict(seed=0, tick=torch.zeros(1, dtype=torch.int32)), dict(seed=0, tick=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            NF.GaussianNoise(**bad)
    with pytest.raises(npi.NpiError):
        NF.GaussianNoise(0, tick=torch.zeros(1, dtype=torch.int64))          # the tick is a DEVICE word
    with pytest.raises(Exception):                                          # frozen
        NF.GaussianNoise(0).seed = 1
    rule = NF.GaussianNoise(3, 2)
    mu, lv = torch.zeros(5, 4), torch.zeros(5, 4)
    with pytest.raises(npi.NpiError):                                       # no CPU path
        NF.reparametrize_kl(mu, lv, rule)
    with pytest.raises(npi.NpiError):
        NF.reparametrize_kl(mu, lv, sample=False)
    with pytest.raises(npi.NpiError):
        NF.gaussian_noise(5, 4, rule, device="cpu")
    with pytest.raises(TypeError):
        NF.reparametrize_kl(mu, lv, None)                                   # sampling needs a rule
    with pytest.raises(TypeError):
        NF.reparametrize_kl(mu, lv, (0, 0))
    with pytest.raises(TypeError):
        NF.reparametrize_kl(mu.double(), lv.double(), rule)
    with pytest.raises(NotImplementedError):
        NF.reparametrize_kl(mu.bfloat16(), lv.bfloat16(), rule)
    with pytest.raises(ValueError):
        NF.reparametrize_kl(mu, lv[:4], rule)
    with pytest.raises(ValueError):
        NF.reparametrize_kl(mu[0], lv[0], rule)
    for kw in (dict(table=2), dict(table=True), dict(n_total=4), dict(n_total=5.0), dict(max_logvar="10"), dict(max_logvar=float("nan"))):
        with pytest.raises(ValueError):
            NF.reparametrize_kl(mu, lv, rule, **kw)
    for kw in (dict(N=-1, F=4), dict(N=4, F=0), dict(N=4.0, F=4), dict(N=4, F=4, table=5)):
        with pytest.raises(ValueError):
            NF.gaussian_noise(rule=rule, **kw)
    with pytest.raises(TypeError):
        NF.gaussian_noise(4, 4, None)


def test_module_surface():
    enc = torch.nn.Linear(4, 6)
    model = npi.VGAE(enc, seed=5)
    assert isinstance(model, npi.GAE) and isinstance(model.decoder, npi.InnerProductDecoder)
    assert (model.seed, model.draw_noise, model.draw, model.tick) == (5, 0, 0, None)
    model.draw_noise = 7
    assert model.draw_noise == 7 and model.draw == 0                        # separate from the negatives' counter
    assert sorted(model.state_dict()) == ["encoder.bias", "encoder.weight"]
    with pytest.raises(ValueError):
        npi.VGAE(enc, seed="x")
    with pytest.raises(ValueError):
        model.kl_loss()                                                     # nothing encoded yet
    with pytest.raises(TypeError):
        model.encode(torch.zeros(3, 4))                                     # the encoder returns one tensor, not (mu, logvar)
    from npi_gnn_amd import autoencoder as AE
    assert AE.MAX_LOGVAR == 10 and AE.EPS == 1e-15
    # evaluation: z is mu itself, nothing is drawn -- no GPU needed for that
    model.eval()
    mu, lv = torch.zeros(3, 2), torch.zeros(3, 2)
    assert model.reparametrize(mu, lv) is mu and model.draw_noise == 7
    # ARGA / ARGVA: torch compositions over the discriminator
    disc = torch.nn.Linear(2, 1)
    arga = npi.ARGA(torch.nn.Linear(4, 2), disc)
    z = torch.randn(9, 2)
    want = -torch.log(torch.sigmoid(disc(z)) + 1e-15).mean()
    assert torch.equal(arga.reg_loss(z), want)
    torch.manual_seed(3)
    got = arga.discriminator_loss(z)
    torch.manual_seed(3)
    real, fake = torch.sigmoid(disc(torch.randn_like(z))), torch.sigmoid(disc(z))
    assert torch.equal(got, -torch.log(real + 1e-15).mean() - torch.log(1 - fake + 1e-15).mean())
    assert sorted(arga.state_dict()) == ["discriminator.bias", "discriminator.weight", "encoder.bias", "encoder.weight"]
    w = disc.weight.detach().clone()
    arga.reset_parameters()
    assert not torch.equal(disc.weight, w)                                  # the discriminator is reset with the rest
    argva = npi.ARGVA(torch.nn.Linear(4, 2), disc, seed=9)
    assert isinstance(argva, npi.ARGA) and isinstance(argva, npi.VGAE)
    assert npi.ARGVA.kl_loss is npi.VGAE.kl_loss and npi.ARGVA.encode is npi.VGAE.encode and npi.ARGVA.reg_loss is npi.ARGA.reg_loss
    assert (argva.seed, argva.draw_noise) == (9, 0) and argva.discriminator is disc
