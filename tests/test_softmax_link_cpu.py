"""The listwise link loss without a GPU: the restatement ``tests/_softmax_link_ref.py`` against a literal loop over a dense fp64
product, the bar of the GPU parity tests against the restatement's own float32 form, the new C-ABI symbols, the argument refusals
of ``npi_softmax_link_*`` (all before the GPU is touched) and of the Python layer, and the workspace bound."""
import ctypes
import math
import os
import re

import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from _util import GRAD_REL, rel_max
import _softmax_link_ref as ref
import _topk_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_softmax_link_workspace_bytes", "npi_softmax_link_fwd", "npi_softmax_link_bwd_src", "npi_softmax_link_bwd_dst")
SHAPES = [(20, 30, 3, True), (33, 33, 8, False), (7, 1, 1, True), (12, 150, 5, True)]        # test_link_rank_cpu.py's


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _literal(z_src, z_dst, edge_index, exclude, allow_loops, scale, u):
    """dense fp64 product, then per query a plain Python loop over the targets: ``(lp, dZ_src, dZ_dst)``"""
    zs, zd = z_src.double(), z_dst.double()
    D = torch.matmul(zs, zd.t())
    n_src, n_dst = D.shape
    banned = set() if exclude is None else {(int(a), int(b)) for a, b in exclude.t().tolist()}
    lp = torch.zeros(edge_index.size(1), dtype=torch.float64)
    ds, dd = torch.zeros_like(zs), torch.zeros_like(zd)
    for q, (s, t) in enumerate(edge_index.t().tolist()):
        if not (0 <= s < n_src and 0 <= t < n_dst):
            continue
        cand = [j for j in range(n_dst) if j == t or ((s, j) not in banned and (allow_loops or j != s))]
        x = [scale * float(D[s, j]) for j in cand]
        m = max(x)
        lse = m + math.log(sum(math.exp(v - m) for v in x))
        lp[q] = scale * float(D[s, t]) - lse
        for j, v in zip(cand, x):
            c = float(u[q]) * ((1.0 if j == t else 0.0) - math.exp(v - lse)) * scale
            ds[s] += c * zd[j]
            dd[j] += c * zs[s]
    return lp, ds, dd


def test_restatement_equals_the_literal_loop_over_a_dense_product():
    seen_bad = 0
    for n_src, n_dst, F, loops in SHAPES:
        zs, zd = tref.real_tables(n_src, n_dst, F, seed=F)
        zs, zd = zs.double(), zd.double()
        one = not loops
        ex = tref.edges(n_src, n_dst, 3 * n_src, seed=F)
        q = ref.queries(n_src, n_dst, 4 * n_src, seed=F)
        if one:
            q[:, 1::8] = q[0, 1::8]                                        # queries (v, v)
        bad = torch.cat([q, torch.tensor([[n_src, -1, 0, 2 ** 40], [0, 0, n_dst, 0]])], 1)
        for e, pairs in ((None, q), (ex, q), (ex, bad)):
            u = ref.upstream(pairs.size(1), seed=F)
            lp, ds, dd, st = ref.link_log_softmax(zs, None if one else zd, pairs, e, loops, 0.5, u)
            llp, lds, ldd = _literal(zs, zs if one else zd, pairs, e, loops, 0.5, u)
            assert st == (ref.BAD_PAIR if pairs is bad else 0)
            assert float((lp - llp).abs().max()) < 1e-12, (n_src, n_dst, F)
            if one:
                assert dd is None and rel_max(ds, lds + ldd) < 1e-12
            else:
                assert rel_max(ds, lds) < 1e-12 and rel_max(dd, ldd) < 1e-12
            if pairs is bad:
                seen_bad += 1
                assert bool((lp[-4:] == 0).all())
                good = ref.link_log_softmax(zs, None if one else zd, q, e, loops, 0.5, u[:-4])
                assert torch.equal(good[0], lp[:-4]) and torch.equal(good[1], ds)      # a bad pair adds to no sum
        if n_dst == 1:                                                     # the target is the only candidate: exactly 0
            assert bool((lp == 0).all()) and bool((ds == 0).all()) and bool((dd == 0).all())
    assert seen_bad == len(SHAPES)
    # the target stays in its own denominator when the pair itself is excluded; a NaN candidate makes lp NaN
    zs = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    zd = torch.tensor([[1.0, 0.0], [2.0, 0.0], [3.0, 0.0]], dtype=torch.float64)
    q = torch.tensor([[0, 0], [0, 1]])
    lp = ref.link_log_softmax(zs, zd, q, torch.tensor([[0, 0], [0, 2]]))[0]
    assert abs(float(lp[0]) - (1 - math.log(math.e + math.e ** 2))) < 1e-15 and float(lp[1]) == 0.0
    zd[2, 0] = float("nan")
    lp, _, _, st = ref.link_log_softmax(zs, zd, q)
    assert bool(torch.isnan(lp).all()) and st == ref.BAD_SCORE
    assert float(ref.loss(torch.tensor([-1.0, -3.0, 0.0]), 3)) == 4 / 3 and float(ref.loss(torch.zeros(0), 0)) == 0.0


def test_the_bar_of_the_gpu_tests_is_usable():
    """on every parity input the restatement in float32 stays within GRAD_REL / 4 of the restatement in float64: a correct float32
    kernel has room (the check test_group_loss_cpu.py makes for Rule G)"""
    worst = 0.0
    for shape in ref.SHAPES:
        for Q in ref.QS:
            for excluded in (True, False):
                got = ref.expected(shape, Q, excluded, torch.float32)
                want = ref.expected(shape, Q, excluded)
                for g, w, what in zip(got, want, ("lp", "dZ_src", "dZ_dst")):
                    err = rel_max(g, w)
                    worst = max(worst, err)
                    assert err <= GRAD_REL / 4, (shape, Q, excluded, what, err)
    assert worst > 0.0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("#define NPI_SOFTMAX_LINK_NO_LOOPS 1", "RULE L", "F.cross_entropy", "InnerProductDecoder.forward_all",
                 "grouping the queries by source"):
        assert word in header, word
    assert header.index("RULE F") < header.index("RULE L")
    assert _lib.NPI_SOFTMAX_LINK_NO_LOOPS == 1
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "softmax_link.hip" in SOURCES and "softmax_link.hip" not in HOST_ONLY
    for name in ("link_log_softmax", "listwise_loss"):
        assert name in npi.__all__ and hasattr(npi, name), name
    assert hasattr(npi.GAE, "listwise_loss")
    # one tile producer: the new unit walks score_tile.h's scan and brings no matrix instruction of its own
    body = open(os.path.join(ROOT, "npi_gnn_amd", "csrc", "softmax_link.hip")).read()
    assert '#include "score_tile.h"' in body and "mfma_f32_32x32x2f32" not in body and "atomicAdd" not in body


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG, P = None, 2 ** 31 - 1, 16                # P: a non-null, 16-byte aligned stand-in for a device pointer (never read)
    ws = lib.npi_softmax_link_workspace_bytes(100, 50, 300, 8, 0)

    def fwd(src=P, dst=P, Q=100, zs=P, lds=8, n_src=50, zd=P, ldd=8, n_dst=300, F=8, rowptr=P, col=P, flags=0, scale=1.0, splits=0,
            a=P, b=P, c=P, work=P, nbytes=ws, status=N):
        return lib.npi_softmax_link_fwd(src, dst, Q, zs, lds, n_src, zd, ldd, n_dst, F, rowptr, col, flags, scale, splits, a, b, c,
                                        work, nbytes, status, N)

    def bwd(fn):
        def call(src=P, dst=P, Q=100, zs=P, lds=8, n_src=50, zd=P, ldd=8, n_dst=300, F=8, rowptr=P, col=P, flags=0, scale=1.0,
                 splits=0, a=P, b=P, c=P, work=P, nbytes=ws, status=N):
            return fn(src, dst, Q, zs, lds, n_src, zd, ldd, n_dst, F, rowptr, col, flags, scale, splits, a, b, c, work, nbytes, N)
        return call

    calls = {
        "null src": dict(src=N), "null dst": dict(dst=N), "null z_src": dict(zs=N), "null z_dst": dict(zd=N),
        "null first output or input": dict(a=N), "null second": dict(b=N), "null workspace": dict(work=N),
        "rowptr without col": dict(col=N), "col without rowptr": dict(rowptr=N),
        "negative Q": dict(Q=-1), "Q 2^31 - 1": dict(Q=BIG, nbytes=2 ** 60), "negative n_src": dict(n_src=-1),
        "n_src 2^31 - 1": dict(n_src=BIG), "negative n_dst": dict(n_dst=-1), "n_dst 2^31 - 1": dict(n_dst=BIG, nbytes=2 ** 60),
        "F 0": dict(F=0), "negative F": dict(F=-8), "F 2^31 - 1": dict(F=BIG, lds=BIG, ldd=BIG),
        "pitch below F (source)": dict(lds=7), "pitch below F (target)": dict(ldd=7),
        "NO_LOOPS with two id spaces": dict(flags=_lib.NPI_SOFTMAX_LINK_NO_LOOPS), "unknown flag": dict(flags=2),
        "short workspace": dict(nbytes=ws - 1), "misaligned workspace": dict(work=24), "negative workspace size": dict(nbytes=-1),
        "negative splits": dict(splits=-1),
        "workspace of fewer splits": dict(splits=3, nbytes=lib.npi_softmax_link_workspace_bytes(100, 50, 300, 8, 3) - 16),
        "scale 0": dict(scale=0.0), "negative scale": dict(scale=-1.0), "scale inf": dict(scale=float("inf")),
        "scale NaN": dict(scale=float("nan")),
    }
    for who, call in (("npi_softmax_link_fwd", fwd), ("npi_softmax_link_bwd_src", bwd(lib.npi_softmax_link_bwd_src)),
                      ("npi_softmax_link_bwd_dst", bwd(lib.npi_softmax_link_bwd_dst))):
        for name, kw in calls.items():
            assert call(**kw) == -1, (who, name)
            assert who.encode() in lib.npi_last_error(), (who, name, lib.npi_last_error())
        assert call(Q=0, F=0) == -1                                                   # nothing to do, but the sizes are still checked
        if call is not fwd:                                                           # (the forward's third output, the loss, may be NULL)
            assert call(c=N) == -1, (who, "null result")
    # nothing to do: no launch, no error, whatever the pointers
    assert fwd(Q=0, c=N) == 0
    assert fwd(src=N, dst=N, Q=0, zs=N, zd=N, rowptr=N, col=N, a=N, b=N, c=N, work=N, nbytes=0) == 0
    assert bwd(lib.npi_softmax_link_bwd_src)(src=N, dst=N, Q=0, zs=N, zd=N, rowptr=N, col=N, a=N, b=N, c=N, work=N, nbytes=0) == 0
    assert bwd(lib.npi_softmax_link_bwd_dst)(Q=0, n_dst=0, n_src=0, c=N, work=N, nbytes=0) == 0


def test_workspace_query_is_bounded_and_nowhere_near_a_score_matrix():
    q = _lib.load().npi_softmax_link_workspace_bytes
    BIG = 2 ** 31 - 1
    assert 0 < q(2 ** 20, 2 ** 20, 2 ** 20, 64, 0) < 4 * 2 ** 40 / 1000
    for Q, n_dst, F in ((0, 0, 1), (1, 1, 1), (100, 300, 8), (16658, 449, 256), (4096, 100000, 128)):
        sizes = [q(Q, 50, n_dst, F, s) for s in (0, 1, 2, 3, 7, 64, 1000)]
        assert all(v > 0 and v % 16 == 0 for v in sizes), (Q, n_dst, F, sizes)
        assert sizes[1] <= sizes[2] <= sizes[3] <= sizes[4] <= sizes[5] == sizes[6] and sizes[0] <= sizes[5]
        assert sizes[1] >= 4 * F * max(Q, n_dst)                                      # an F-wide row per query and per target ...
        assert sizes[5] <= 64 * 4 * F * (max(Q, 1) + max(n_dst, 1)) + 64 * 8 * max(Q, 1) + 16 * max(Q, 1) + 64      # ... per split
    assert q(BIG - 1, BIG - 1, BIG - 1, BIG - 1, 64) == -1                                # more bytes than an int64 holds
    for bad in ((-1, 10, 10, 8, 0), (BIG, 10, 10, 8, 0), (10, -1, 10, 8, 0), (10, 10, BIG, 8, 0), (10, 10, 10, 0, 0), (10, 10, 10, 8, -1)):
        assert q(*bad) == -1, bad


# ---- the Python layer: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_function_argument_errors_and_no_cpu_fallback():
    z, zd = torch.randn(6, 4), torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    for fn in (npi.link_log_softmax, npi.listwise_loss):
        for bad_z in (None, "z", (z,), (z, zd, z), (z, None), [z, 3]):
            with pytest.raises(TypeError):
                fn(bad_z, ei)
        for bad_z in (z[0], (z, zd[:, :3]), torch.randn(6, 0), (z, zd[0])):
            with pytest.raises(ValueError):
                fn(bad_z, ei)
        for bad_z in (z.double(), (z, zd.half()), z.long()):
            with pytest.raises(TypeError):
                fn(bad_z, ei)
        with pytest.raises(NotImplementedError):
            fn(z.bfloat16(), ei)
        for bad_q in ("edges", [[0], [1]], 3, None):
            with pytest.raises(TypeError):
                fn(z, bad_q)
        for bad_q in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
            with pytest.raises(ValueError):
                fn(z, bad_q)
        for bad_ex in ("edges", [[0], [1]], 3):
            with pytest.raises(TypeError):
                fn(z, ei, exclude=bad_ex)
        for bad_ex in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
            with pytest.raises(ValueError):
                fn(z, ei, exclude=bad_ex)
        with pytest.raises(ValueError, match="allow_loops"):
            fn((z, zd), ei, allow_loops=False)
        with pytest.raises(ValueError, match="splits"):
            fn(z, ei, splits=-1)
        for bad_splits in (1.5, True, "2"):
            with pytest.raises(TypeError):
                fn(z, ei, splits=bad_splits)
        for bad_scale in (0, 0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="scale"):
                fn(z, ei, scale=bad_scale)
        for bad_scale in ("1", None, True, torch.tensor(1.0)):
            with pytest.raises(TypeError):
                fn(z, ei, scale=bad_scale)
    # arguments in order, tensors on the CPU
    model = npi.GAE(torch.nn.Identity())
    for call in (lambda: npi.link_log_softmax(z, ei), lambda: npi.link_log_softmax((z, zd), ei, exclude=ei, splits=3, scale=0.5),
                 lambda: npi.listwise_loss(z, ei, allow_loops=False), lambda: npi.listwise_loss((z, zd), ei, exclude=ei),
                 lambda: model.listwise_loss(z, ei), lambda: model.listwise_loss((z, zd), ei, ei, scale=2.0)):
        with pytest.raises(npi.NpiError):
            call()
