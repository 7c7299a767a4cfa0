"""Ranking losses over corrupted targets without a GPU: the restatement ``tests/_group_ref.py`` against the literal torch
compositions under autograd, what float32 alone costs on the GPU tests' inputs against the bar they assert, the hinge condition of
the ``margin`` inputs, the new C-ABI symbols, and the argument errors of ``npi_group_score`` and of the Python layer."""
import ctypes
import os
import re

import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import functional as F_
import _group_ref as ref
from _util import GRAD_REL, rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_group_score", "npi_group_score_workspace_bytes")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _torch_loss(x, valid, kind, margin, scale):
    """the literal compositions: -logsigmoid, clamp(min=0), cross_entropy with -inf-masked columns; divisors P K / P K / P"""
    P, C = x.shape
    K = C - 1
    if P == 0 or (K == 0 and kind != "softmax"):
        return x.sum() * 0
    if kind == "softmax":
        ok = valid[:, 0]                                                  # a dropped group has no row in the cross-entropy
        cols = torch.where(valid[ok], scale * x[ok], torch.full_like(x[ok], float("-inf")))
        ce = torch.nn.functional.cross_entropy(cols, torch.zeros(int(ok.sum()), dtype=torch.int64), reduction="sum")
        return ce / P
    V = valid[:, 1:]
    diff = (x[:, :1] - x[:, 1:])[V]                                         # x_pos - x_neg of the valid corrupted slots
    if kind == "bpr":
        return -torch.nn.functional.logsigmoid(scale * diff).sum() / (P * K)
    return (margin - scale * diff).clamp(min=0).sum() / (P * K)


def _autograd(zs, zd, src, dst, neg, kind, margin, scale, upstream, one=False):
    """(loss, dZ_src, dZ_dst) -- or (loss, dZ) for one table -- of the literal composition in fp64"""
    a = zs.double().requires_grad_(True)
    b = a if one else zd.double().requires_grad_(True)
    n_src, n_dst = a.size(0), b.size(0)
    tgt, keep, valid = ref.slots(src, dst, neg, n_src, n_dst)
    x = (a[src.clamp(0, n_src - 1)][:, None, :] * b[tgt.clamp(0, n_dst - 1)]).sum(-1)
    loss = _torch_loss(x, valid, kind, margin, scale)
    (upstream * loss).backward()
    return (loss.detach(), a.grad) if one else (loss.detach(), a.grad, b.grad if b.grad is not None else torch.zeros_like(b))


@pytest.mark.parametrize("kind,margin,scale", ref.cases() + (("margin", 0.3, 2.5),))
def test_restatement_equals_the_torch_compositions_under_autograd(kind, margin, scale):
    for F, (P, K) in ((3, (9, 3)), (64, (33, 1)), (64, (5, 0)), (257, (21, 7)), (64, (6, 63))):
        zs, zd, src, dst, neg = ref.inputs(P, K, F, kind, margin, scale)
        if K:
            assert bool((neg == -1).any()) and bool((neg[P // 2] == -1).all())
            neg[0, 0] = ref.N_DST + 3                                        # a bad id: as an empty slot
        if P > 4:
            src[1] = -5                                                     # a dropped group
        r = ref.evaluate(zs, zd, src, dst, neg, kind, margin, scale, upstream=2.5)
        loss, ga, gb = _autograd(zs, zd, src, dst, neg, kind, margin, scale, 2.5)
        assert rel_max(r["loss"], loss) <= 1e-12, (F, P, K)
        if K:
            assert rel_max(r["d_src"], ga) <= 1e-11 and rel_max(r["d_dst"], gb) <= 1e-11, (F, P, K)
        else:
            assert float(r["loss"]) == 0 and float(r["d_src"].abs().max()) == 0 and float(r["d_dst"].abs().max()) == 0
        # d loss / d logit itself
        x = ref.logits(zs.double(), zd.double(), src, dst, neg)[0]
        xs = torch.where(r["valid"], x, torch.zeros_like(x)).requires_grad_(True)
        _torch_loss(xs, r["valid"], kind, margin, scale).backward()
        if K:
            assert rel_max(r["coef"], xs.grad) <= 1e-11
        assert bool((r["coef"][~r["valid"]] == 0).all())
        assert float((r["coef"].sum(1)).abs().max()) <= 1e-14                # coef_0 = -sum of the others
    # one id space: both terms land in one table
    z, src, dst, neg = ref.one_space_inputs(kind, margin, scale)
    r = ref.evaluate(z, z, src, dst, neg, kind, margin, scale, upstream=-1.5)
    loss, g = _autograd(z, z, src, dst, neg, kind, margin, scale, -1.5, one=True)
    assert rel_max(r["loss"], loss) <= 1e-12 and rel_max(r["d_src"] + r["d_dst"], g) <= 1e-11


def test_empty_groups_and_extreme_logits():
    zs, zd = ref.tables(64)
    none = torch.empty(0, dtype=torch.int64)
    for kind, margin, scale in ref.cases():
        r = ref.evaluate(zs, zd, none, none, torch.empty((0, 4), dtype=torch.int64), kind, margin, scale)
        assert float(r["loss"]) == 0 and r["logits"].shape == (0, 5)
        src, dst, neg = ref.groups(9, 3)
        neg[:] = -1                                                         # no valid corrupted target anywhere
        r = ref.evaluate(zs, zd, src, dst, neg, kind, margin, scale)
        assert float(r["loss"]) == 0 and float(r["coef"].abs().max()) == 0 and bool(torch.isinf(r["logits"][:, 1:]).all())
    zs, zd, src, dst, neg = ref.extreme_groups()
    x = ref.logits(zs.double(), zd.double(), src, dst, neg)[0]
    assert abs(float(x.max()) - 60.0) < 1e-3 and abs(float(x.min()) + 60.0) < 1e-3
    for dtype in (torch.float64, torch.float32):
        for kind in ("bpr", "margin", "softmax"):
            r = ref.evaluate(zs, zd, src, dst, neg, kind, 1.0, 2.5, dtype=dtype)
            assert torch.isfinite(r["loss"]) and torch.isfinite(r["coef"]).all(), (dtype, kind)


# ---- what float32 alone costs on the GPU tests' inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ref.F_CASES)
def test_float32_restatement_meets_the_gpu_bar_on_the_gpu_inputs(F):
    """The bar of tests/test_gpu_group_loss.py (GRAD_REL = 1e-5 of the largest reference entry) against float32 arithmetic itself: the
    same formulas in float32 torch on the CPU, every input of the GPU parity cases.  Printed: the worst ratio per quantity."""
    worst = {}
    for F_, P, K, kind, margin, scale in ref.parity_inputs():
        if F_ != F:
            continue
        zs, zd, src, dst, neg = ref.inputs(P, K, F, kind, margin, scale)
        up = ref.upstream_of(P, K, F)
        r64 = ref.evaluate(zs, zd, src, dst, neg, kind, margin, scale, upstream=up)
        r32 = ref.evaluate(zs, zd, src, dst, neg, kind, margin, scale, upstream=up, dtype=torch.float32)
        assert float(r64["logits"][r64["valid"]].abs().max()) <= 4.0
        for k in ("logits", "loss", "coef", "d_src", "d_dst"):
            err = ref.rel_finite(r32[k], r64[k]) if k == "logits" else rel_max(r32[k], r64[k])
            worst[k] = max(worst.get(k, 0.0), err)
    z, src, dst, neg = ref.one_space_inputs("softmax")
    r64, r32 = (ref.evaluate(z, z, src, dst, neg, "softmax", dtype=t) for t in (torch.float64, torch.float32))
    worst["d_one"] = rel_max(r32["d_src"] + r32["d_dst"], r64["d_src"] + r64["d_dst"])
    print(F, worst)
    for k, v in worst.items():
        assert v <= GRAD_REL, (k, v)


def test_float32_restatement_meets_the_gpu_bar_at_extreme_logits():
    zs, zd, src, dst, neg = ref.extreme_groups()
    for kind in ("bpr", "softmax"):
        r64 = ref.evaluate(zs, zd, src, dst, neg, kind, 1.0, 2.5)
        r32 = ref.evaluate(zs, zd, src, dst, neg, kind, 1.0, 2.5, dtype=torch.float32)
        for k in ("loss", "coef"):
            print(kind, k, rel_max(r32[k], r64[k]))
            assert rel_max(r32[k], r64[k]) <= GRAD_REL, (kind, k)


def test_every_margin_parity_input_keeps_its_hinges_off_the_kink():
    """for every ``margin`` parity case a seed in 0 .. 31 exists whose fp64 reference has every valid |margin + d_c| >= 1e-3, and both
    branches of the hinge occur over the cases"""
    active = total = 0
    margins = [(F, P, K, m, s) for F, P, K, kind, m, s in ref.parity_inputs() if kind == "margin"]
    assert len(margins) == len(ref.F_CASES) * len(ref.SHAPES)
    for F, P, K, margin, scale in margins:
        assert ref._seed(P, K, F, "margin", margin, scale, ref.N_SRC, ref.N_DST) is not None, (F, P, K)
        zs, zd, src, dst, neg = ref.inputs(P, K, F, "margin", margin, scale)
        assert ref.hinge_gap(zs, zd, src, dst, neg, margin, scale) >= ref.HINGE_GAP, (F, P, K)
        r = ref.evaluate(zs, zd, src, dst, neg, "margin", margin, scale)
        V = r["valid"].clone()
        V[:, 0] = False
        active += int((r["coef"][V] > 0).sum())
        total += int(V.sum())
    print("active hinges:", active, "of", total)
    assert 0 < active < total
    ref.one_space_inputs("margin")                                          # (asserts the same of the one-id-space input)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("#define NPI_GROUP_LOGITS 0", "#define NPI_GROUP_LOSS_BPR 1", "#define NPI_GROUP_LOSS_MARGIN 2",
                 "#define NPI_GROUP_LOSS_SOFTMAX 3", "Rule G", "In numpy"):
        assert word in header, word
    assert (_lib.NPI_GROUP_LOGITS, _lib.NPI_GROUP_LOSS_BPR, _lib.NPI_GROUP_LOSS_MARGIN, _lib.NPI_GROUP_LOSS_SOFTMAX) == (0, 1, 2, 3)
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "group_score.hip" in SOURCES and "group_score.hip" not in HOST_ONLY
    for name in ("group_scores", "ranking_loss"):
        assert name in npi.__all__ and hasattr(npi, name), name
    assert F_.group_scores is npi.group_scores and F_.ranking_loss is npi.ranking_loss
    assert hasattr(npi.GAE, "ranking_loss") and hasattr(npi.InnerProductDecoder, "group_scores")
    assert F_.GROUP_LOSSES == {"bpr": 1, "margin": 2, "softmax": 3}


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG, A = None, 2 ** 31 - 1, 16                # A: a non-null, 16-byte aligned stand-in for a device pointer (never read)
    ws = lib.npi_group_score_workspace_bytes(100, 8)
    LOG, BPR, MAR, SOF = 0, 1, 2, 3
    inf, nan = float("inf"), float("nan")

    def call(src=A, dst=A, P=100, neg=A, ld_neg=8, K=8, zs=A, lds=8, n_src=4, zd=A, ldd=8, n_dst=4, F=8, mode=BPR, margin=1.0,
             scale=1.0, logits=A, coef=A, loss=A, part=A, nbytes=ws, status=N):
        return lib.npi_group_score(src, dst, P, neg, ld_neg, K, zs, lds, n_src, zd, ldd, n_dst, F, mode, margin, scale, logits, coef,
                                   loss, part, nbytes, status, N)

    calls = {
        "null src": dict(src=N), "null dst": dict(dst=N), "null neg": dict(neg=N), "null z_src": dict(zs=N), "null z_dst": dict(zd=N),
        "no output": dict(logits=N, coef=N, loss=N),
        "negative P": dict(P=-1), "P 2^31 - 1": dict(P=BIG, K=0, ld_neg=0, nbytes=2 ** 40),
        "P (1 + K) 2^31 - 1": dict(P=2 ** 28, K=7, nbytes=2 ** 40), "negative K": dict(K=-1), "K 64": dict(K=64, ld_neg=64),
        "pitch below K": dict(ld_neg=7), "negative F": dict(F=-8), "F 0": dict(F=0), "F 2^31 - 1": dict(F=BIG, lds=BIG, ldd=BIG),
        "negative n_src": dict(n_src=-1), "n_src 2^31 - 1": dict(n_src=BIG), "negative n_dst": dict(n_dst=-1),
        "n_dst 2^31 - 1": dict(n_dst=BIG), "pitch below F (source)": dict(lds=7), "pitch below F (target)": dict(ldd=7),
        "unknown mode": dict(mode=4), "negative mode": dict(mode=-1),
        "coef in LOGITS mode": dict(mode=LOG, loss=N), "loss in LOGITS mode": dict(mode=LOG, coef=N),
        "loss without workspace": dict(part=N), "short workspace": dict(nbytes=ws - 1), "misaligned workspace": dict(part=24),
        "negative workspace size": dict(nbytes=-1),
        "margin inf": dict(mode=MAR, margin=inf), "margin nan": dict(margin=nan), "scale inf": dict(scale=inf),
        "scale nan": dict(scale=nan), "scale 0": dict(scale=0.0), "scale negative": dict(mode=SOF, scale=-1.0),
    }
    for name, kw in calls.items():
        assert call(**kw) == -1, name
        assert b"npi_group_score" in lib.npi_last_error(), (name, lib.npi_last_error())
    for mode in (MAR, SOF):
        assert call(mode=mode, part=N) == -1 and call(mode=mode, F=0) == -1
    q = lib.npi_group_score_workspace_bytes
    assert q(-1, 1) == -1 and q(BIG, 0) == -1 and q(10, -1) == -1 and q(10, 64) == -1 and q(2 ** 28, 7) == -1
    assert q(0, 0) >= 8 and q(0, 0) % 16 == 0 and q(0, 63) >= 8
    assert ws >= 8 and ws % 16 == 0
    # one partial per workgroup of four wavefronts of 64 // (1 + K) whole groups
    for K in (0, 1, 2, 7, 8, 31, 32, 63):
        per_wg = 4 * (64 // (1 + K))
        assert q(10 ** 6, K) >= 8 * -(-10 ** 6 // per_wg) and q(10 ** 6, K) % 16 == 0, K
    # nothing to do: no launch, no error (the loss of no group is written by the runtime, so it is not asked for without a device)
    assert call(src=N, dst=N, P=0, neg=N, zs=N, zd=N, coef=N, loss=N, part=N, nbytes=0) == 0
    assert call(src=N, dst=N, P=0, neg=N, K=0, ld_neg=0, mode=LOG, zs=N, zd=N, coef=N, loss=N, part=N, nbytes=0) == 0


# ---- the Python layer: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_function_and_class_argument_errors_and_no_cpu_fallback():
    z, zd = torch.randn(6, 4), torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    neg = torch.tensor([[0, 1], [2, 3], [4, -1]])
    for fn in (npi.group_scores, npi.ranking_loss):
        for bad_z in (None, "z", (z,), (z, zd, z), (z, None), [z, 3]):
            with pytest.raises(TypeError):
                fn(bad_z, ei, neg)
        for bad_z in (z[0], (z, zd[:, :3]), torch.randn(6, 0), (z, zd[0])):
            with pytest.raises(ValueError):
                fn(bad_z, ei, neg)
        for bad_z in (z.double(), (z, zd.half()), z.long()):
            with pytest.raises(TypeError):
                fn(bad_z, ei, neg)
        with pytest.raises(NotImplementedError):
            fn(z.bfloat16(), ei, neg)
        with pytest.raises(NotImplementedError):
            fn((z, zd.bfloat16()), ei, neg)
        for bad_ei in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(z, bad_ei, neg)
        for bad_neg in (neg.float(), neg.to(torch.int32), neg[:2], neg[:, :, None], torch.zeros((3, 64), dtype=torch.int64),
                        torch.tensor(1)):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(z, ei, bad_neg)
        for bad in ([[0, 1], [1, 0]], None):
            with pytest.raises(TypeError, match=fn.__name__):
                fn(z, bad, neg)
            with pytest.raises(TypeError, match=fn.__name__):
                fn(z, ei, bad)
    with pytest.raises(ValueError, match="loss"):
        npi.ranking_loss(z, ei, neg, loss="gae")
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(margin=float("nan")),
               dict(margin=float("-inf"))):
        with pytest.raises(ValueError, match="ranking_loss"):
            npi.ranking_loss(z, ei, neg, loss="margin", **kw)
    # arguments in order, tensors on the CPU
    model = npi.GAE(torch.nn.Identity())
    for call in (lambda: npi.group_scores(z, ei, neg), lambda: npi.group_scores((z, zd), ei, neg[:, 0]),
                 lambda: npi.ranking_loss(z, ei, neg), lambda: npi.ranking_loss((z, zd), ei, neg, loss="softmax", scale=2.0),
                 lambda: npi.ranking_loss(z, ei, neg[:, :0], loss="margin", margin=0.5),
                 lambda: npi.InnerProductDecoder().group_scores(z, ei, neg), lambda: model.ranking_loss(z, ei, neg_dst=neg),
                 lambda: model.ranking_loss(z, ei, num_neg=4), lambda: model.ranking_loss((z, zd), ei, loss="softmax", seed=3)):
        with pytest.raises(npi.NpiError):
            call()
    with pytest.raises(ValueError, match="loss"):
        model.ranking_loss(z, ei, loss="bce")
    for bad in (-1, 64):
        with pytest.raises(ValueError, match="num_neg"):
            model.ranking_loss(z, ei, num_neg=bad)
    assert model.draw == 0                                                         # a refused call takes no draw number
