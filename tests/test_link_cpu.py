"""Pair scores and the link loss without a GPU: the restatement ``tests/_link_ref.py`` against the literal PyG composition under
torch autograd, the new C-ABI symbols, the argument errors of ``npi_pair_score`` and of the Python layer, and what float32 alone
costs on the GPU tests' inputs against the bar they assert."""
import ctypes
import os
import re

import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import functional as F_
import _link_ref as ref
from _util import GRAD_REL, rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_pair_score", "npi_pair_score_workspace_bytes")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _pyg(z_src, z_dst, pos, neg, kind):
    """PyG 1.4.2 written out literally: InnerProductDecoder.forward + GAE.recon_loss, or binary_cross_entropy_with_logits"""
    def decoder(ei, sigmoid=True):
        value = (z_src[ei[0]] * z_dst[ei[1]]).sum(dim=1)
        return torch.sigmoid(value) if sigmoid else value
    if kind == "gae":
        pos_loss = -torch.log(decoder(pos) + ref.EPS).mean()
        neg_loss = -torch.log(1 - decoder(neg) + ref.EPS).mean()
        return pos_loss + neg_loss
    x = decoder(torch.cat([pos, neg], 1), sigmoid=False)
    y = torch.cat([torch.ones(pos.size(1)), torch.zeros(neg.size(1))]).to(x.dtype)
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y)


@pytest.mark.parametrize("kind", ["gae", "bce"])
def test_restatement_equals_the_pyg_composition_under_autograd(kind):
    for F, M in ((3, 9), (64, 65), (257, 1000)):
        zs, zd = ref.tables(F)
        src, dst = ref.pair_list(M)
        n_pos = M // 3
        r = ref.evaluate(zs, zd, src, dst, n_pos, kind, upstream=2.5)
        a, b = zs.double().requires_grad_(True), zd.double().requires_grad_(True)
        ei = torch.stack([src, dst])
        loss = _pyg(a, b, ei[:, :n_pos], ei[:, n_pos:], kind)
        (2.5 * loss).backward()
        assert rel_max(r["loss"], loss) <= 1e-13
        assert rel_max(r["d_src"], a.grad) <= 1e-12 and rel_max(r["d_dst"], b.grad) <= 1e-12
        # d loss / d logit, and the gradient of plain logits under a random upstream gradient
        x = ref.logits(zs.double(), zd.double(), src, dst).requires_grad_(True)
        lx = _pyg_from_logits(x, n_pos, kind)
        lx.backward()
        assert rel_max(r["coef"], x.grad) <= 1e-12
    # one id space: both terms land in one table
    z = ref.tables(64, 30, 30)[0]
    src, dst = ref.pair_list(200, 30, 30)
    r = ref.evaluate(z, z, src, dst, 70, kind)
    a = z.double().requires_grad_(True)
    ei = torch.stack([src, dst])
    _pyg(a, a, ei[:, :70], ei[:, 70:], kind).backward()
    assert rel_max(r["d_src"] + r["d_dst"], a.grad) <= 1e-12


def _pyg_from_logits(x, n_pos, kind):
    if kind == "gae":
        return -torch.log(torch.sigmoid(x[:n_pos]) + ref.EPS).mean() - torch.log(1 - torch.sigmoid(x[n_pos:]) + ref.EPS).mean()
    y = (torch.arange(x.numel()) < n_pos).to(x.dtype)
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y)


def test_an_empty_part_adds_zero_and_extreme_logits_stay_finite():
    zs, zd = ref.tables(64)
    src, dst = ref.pair_list(65)
    for kind in ("gae", "bce"):
        for n_pos in (0, 65):
            r = ref.evaluate(zs, zd, src, dst, n_pos, kind)
            assert torch.isfinite(r["loss"]) and torch.isfinite(r["coef"]).all()
    zs, zd, src, dst = ref.extreme_tables()
    x = ref.logits(zs.double(), zd.double(), src, dst)
    assert abs(float(x.max()) - 60.0) < 1e-3 and abs(float(x.min()) + 60.0) < 1e-3
    for dtype in (torch.float64, torch.float32):
        for kind in ("gae", "bce"):
            r = ref.evaluate(zs, zd, src, dst, src.numel() // 3, kind, dtype=dtype)
            assert torch.isfinite(r["loss"]) and torch.isfinite(r["coef"]).all(), (dtype, kind)


# ---- what float32 alone costs on the GPU tests' inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ref.F_CASES)
def test_float32_restatement_meets_the_gpu_bar_on_the_gpu_inputs(F):
    """The bar of tests/test_gpu_link.py (GRAD_REL = 1e-5 of the largest reference entry) against float32 arithmetic itself: the
    same formulas in float32 torch on the CPU, every shape of the GPU parity cases.  Printed: the worst ratio per quantity."""
    zs, zd = ref.tables(F)
    worst = {}
    for M in ref.M_CASES:
        src, dst = ref.pair_list(M)
        for n_pos in ref.n_pos_cases(M):
            for kind in ("gae", "bce"):
                r64 = ref.evaluate(zs, zd, src, dst, n_pos, kind)
                r32 = ref.evaluate(zs, zd, src, dst, n_pos, kind, dtype=torch.float32)
                assert float(r64["logits"].abs().max()) <= 4.0
                for k in r64:
                    worst[k] = max(worst.get(k, 0.0), rel_max(r32[k], r64[k]))
    print(F, worst)
    for k, v in worst.items():
        assert v <= GRAD_REL, (k, v)


def test_float32_restatement_meets_the_gpu_bar_at_logits_of_sixty():
    zs, zd, src, dst = ref.extreme_tables()
    r64 = ref.evaluate(zs, zd, src, dst, src.numel() // 3, "bce")
    r32 = ref.evaluate(zs, zd, src, dst, src.numel() // 3, "bce", dtype=torch.float32)
    for k in ("loss", "coef"):
        assert rel_max(r32[k], r64[k]) <= GRAD_REL, k


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("#define NPI_PAIR_LOGITS 0", "#define NPI_PAIR_LOSS_GAE 1", "#define NPI_PAIR_LOSS_BCE 2",
                 "#define NPI_STATUS_BAD_PAIR_ID 256", "InnerProductDecoder.forward", "GAE.recon_loss",
                 "(z[edge_index[0]] * z[edge_index[1]]).sum(dim=1)", "binary_cross_entropy_with_logits"):
        assert word in header, word
    assert (_lib.NPI_PAIR_LOGITS, _lib.NPI_PAIR_LOSS_GAE, _lib.NPI_PAIR_LOSS_BCE, _lib.NPI_STATUS_BAD_PAIR_ID) == (0, 1, 2, 256)
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "pair_score.hip" in SOURCES and "pair_score.hip" not in HOST_ONLY
    for name in ("InnerProductDecoder", "GAE", "pair_scores", "link_loss"):
        assert name in npi.__all__ and hasattr(npi, name), name
    assert F_.pair_scores is npi.pair_scores and F_.link_loss is npi.link_loss


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG, P = None, 2 ** 31 - 1, 16                # P: a non-null, 16-byte aligned stand-in for a device pointer (never read)
    ws = lib.npi_pair_score_workspace_bytes(100)
    LOG, GAE, BCE = _lib.NPI_PAIR_LOGITS, _lib.NPI_PAIR_LOSS_GAE, _lib.NPI_PAIR_LOSS_BCE

    def call(src=P, dst=P, M=100, n_pos=30, zs=P, lds=8, n_src=4, zd=P, ldd=8, n_dst=4, F=8, mode=GAE, logits=P, coef=P, loss=P,
             part=P, nbytes=ws, status=N):
        return lib.npi_pair_score(src, dst, M, n_pos, zs, lds, n_src, zd, ldd, n_dst, F, mode, logits, coef, loss, part, nbytes,
                                  status, N)

    calls = {
        "null src": dict(src=N), "null dst": dict(dst=N), "null z_src": dict(zs=N), "null z_dst": dict(zd=N),
        "no output": dict(logits=N, coef=N, loss=N),
        "negative M": dict(M=-1), "M 2^31 - 1": dict(M=BIG, nbytes=2 ** 40), "negative F": dict(F=-8), "F 0": dict(F=0),
        "F 2^31 - 1": dict(F=BIG, lds=BIG, ldd=BIG), "negative n_src": dict(n_src=-1), "n_src 2^31 - 1": dict(n_src=BIG),
        "negative n_dst": dict(n_dst=-1), "n_dst 2^31 - 1": dict(n_dst=BIG), "negative n_pos": dict(n_pos=-1),
        "n_pos above M": dict(n_pos=101), "pitch below F (source)": dict(lds=7), "pitch below F (target)": dict(ldd=7),
        "unknown mode": dict(mode=3), "negative mode": dict(mode=-1),
        "coef in LOGITS mode": dict(mode=LOG, loss=N), "loss in LOGITS mode": dict(mode=LOG, coef=N),
        "loss without workspace": dict(part=N), "short workspace": dict(nbytes=ws - 1), "misaligned workspace": dict(part=24),
        "negative workspace size": dict(nbytes=-1),
    }
    for name, kw in calls.items():
        assert call(**kw) == -1, name
        assert b"npi_pair_score" in lib.npi_last_error(), (name, lib.npi_last_error())
    assert call(mode=BCE, part=N) == -1 and call(mode=BCE, F=0) == -1
    assert lib.npi_pair_score_workspace_bytes(-1) == -1 and lib.npi_pair_score_workspace_bytes(BIG) == -1
    assert lib.npi_pair_score_workspace_bytes(0) >= 8 and lib.npi_pair_score_workspace_bytes(0) % 16 == 0
    assert ws >= 8 and ws % 16 == 0 and lib.npi_pair_score_workspace_bytes(2 ** 21) >= 8 * 2 ** 21 // 256
    # nothing to do: no launch, no error (the loss of no pair is written by the runtime, so it is not asked for without a device)
    assert call(src=N, dst=N, M=0, n_pos=0, zs=N, zd=N, coef=N, loss=N, part=N, nbytes=0) == 0
    assert call(src=N, dst=N, M=0, n_pos=0, mode=LOG, coef=N, loss=N, part=N, nbytes=0) == 0


# ---- the Python layer: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_function_and_class_argument_errors_and_no_cpu_fallback():
    z, zd = torch.randn(6, 4), torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    for bad_z in (None, "z", (z,), (z, zd, z), (z, None), [z, 3]):
        with pytest.raises(TypeError):
            npi.pair_scores(bad_z, ei)
        with pytest.raises(TypeError):
            npi.link_loss(bad_z, ei, ei)
    for bad_z in (z[0], (z, zd[:, :3]), torch.randn(6, 0), (z, zd[0])):
        with pytest.raises(ValueError):
            npi.pair_scores(bad_z, ei)
    for bad_z in (z.double(), (z, zd.half()), z.long()):
        with pytest.raises(TypeError):
            npi.pair_scores(bad_z, ei)
    with pytest.raises(NotImplementedError):
        npi.pair_scores(z.bfloat16(), ei)
    with pytest.raises(NotImplementedError):
        npi.link_loss((z, zd.bfloat16()), ei, ei)
    for bad_size in ((6,), 6, (6, 6), (5, 6)):
        with pytest.raises(ValueError):
            npi.pair_scores((z, zd), ei, size=bad_size)
    for bad_ei in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
        with pytest.raises(ValueError):
            npi.pair_scores(z, bad_ei)
        with pytest.raises(ValueError):
            npi.link_loss(z, bad_ei, ei)
        with pytest.raises(ValueError):
            npi.link_loss(z, ei, bad_ei)
    with pytest.raises(TypeError):
        npi.pair_scores(z, [[0, 1], [1, 0]])
    with pytest.raises(TypeError):
        npi.link_loss(z, ei, None)
    with pytest.raises(ValueError, match="loss"):
        npi.link_loss(z, ei, ei, loss="hinge")
    with pytest.raises(ValueError, match="num_pos"):
        npi.link_loss(z, ei, ei, num_pos=2)
    # arguments in order, tensors on the CPU
    for call in (lambda: npi.pair_scores(z, ei), lambda: npi.pair_scores((z, zd), ei, size=(6, 5)), lambda: npi.link_loss(z, ei, ei),
                 lambda: npi.link_loss((z, zd), ei, ei, loss="bce"), lambda: npi.InnerProductDecoder()(z, ei),
                 lambda: npi.InnerProductDecoder()((z, zd), ei, sigmoid=False)):
        with pytest.raises(npi.NpiError):
            call()
    model = npi.GAE(torch.nn.Linear(4, 4))
    assert isinstance(model.decoder, npi.InnerProductDecoder) and model.draw == 0
    assert model.encode(z).shape == (6, 4) and npi.GAE(torch.nn.Identity(), decoder=torch.nn.Identity()).decode(z) is z
    before = model.encoder.weight.detach().clone()
    model.reset_parameters()
    assert not torch.equal(before, model.encoder.weight)
    with pytest.raises(ValueError, match="loss"):
        model.recon_loss(z, ei, loss="hinge")
    with pytest.raises(npi.NpiError):
        model.recon_loss(z, ei, ei)
    with pytest.raises(npi.NpiError):
        model.recon_loss(z, ei)
    with pytest.raises(npi.NpiError):
        model.recon_loss((z, zd), ei, loss="bce", seed=3)
    assert model.draw == 0                                                         # a refused call takes no draw number
    assert not hasattr(npi.InnerProductDecoder, "forward_all")
