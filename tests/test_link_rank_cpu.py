"""Filtered link ranks without a GPU: the restatement ``tests/_link_rank_ref.py`` against a literal loop over a dense product and
against ``_topk_ref.topk`` through Rule F 4, the new C-ABI symbols, the argument refusals of ``npi_link_ranks`` (all before the GPU
is touched) and of the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
import _link_rank_ref as ref
import _topk_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_link_ranks", "npi_link_ranks_workspace_bytes")
SHAPES = [(20, 30, 3, True), (33, 33, 8, False), (7, 1, 1, True), (12, 150, 5, True)]


def _inputs(n_src, n_dst, F, loops, maker):
    zs, zd = maker(n_src, n_dst, F, seed=F)
    if not loops:
        zd = zs
    ex = tref.edges(n_src, n_dst, 3 * n_src, seed=F)
    q = ref.queries(n_src, n_dst, 4 * n_src, ex, seed=F)
    if not loops:
        q[:, 1::8] = q[0, 1::8]                                           # queries (v, v)
    return zs, zd, ex, q


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _literal(z_src, z_dst, edge_index, exclude, allow_loops):
    """dense matmul, then per query a plain Python loop over the targets"""
    D = torch.matmul(z_src.double(), z_dst.double().t()).float()
    n_src, n_dst = D.shape
    banned = set() if exclude is None else {(int(a), int(b)) for a, b in exclude.t().tolist()}
    out, sc = [], []
    for s, t in edge_index.t().tolist():
        if not (0 <= s < n_src and 0 <= t < n_dst) or torch.isnan(D[s, t]):
            out.append([-1] * 4)
            sc.append(float("-inf"))
            continue
        mine = float(D[s, t])
        g = e = b = c = 0
        for j in range(n_dst):
            if j == t or (s, j) in banned or (not allow_loops and j == s) or torch.isnan(D[s, j]):
                continue
            v = float(D[s, j])
            c += 1
            g += v > mine
            e += v == mine                                                 # -0.0 == +0.0 in Python too
            b += v == mine and j < t
        out.append([g, e, b, c])
        sc.append(mine + 0.0)
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 4), torch.tensor(sc, dtype=torch.float32)


def test_restatement_equals_the_literal_loop_over_a_dense_product():
    for n_src, n_dst, F, loops in SHAPES:
        for maker in (tref.int_tables, tref.real_tables):
            zs, zd, ex, q = _inputs(n_src, n_dst, F, loops, maker)
            bad = torch.cat([q, torch.tensor([[n_src, -1, 0, 2 ** 40], [0, 0, n_dst, 0]])], 1)
            for e, pairs in ((None, q), (ex, q), (ex, bad)):
                c, s, st = ref.link_ranks(zs, zd, pairs, e, loops)
                lc, ls = _literal(zs, zd, pairs, e, loops)
                assert torch.equal(c, lc) and torch.equal(s, ls), (n_src, n_dst, F)
                assert st == (ref.BAD_PAIR if pairs is bad else 0)
                if pairs is bad:
                    assert bool((c[-4:] == -1).all()) and bool(torch.isneginf(s[-4:]).all())
    # zeros of both signs tie and the score comes out as +0.0; a NaN competitor is not counted; a NaN target is a row of -1
    zs = torch.tensor([[1.0, 0.0], [-1.0, 0.0]])
    zd = torch.tensor([[0.0, 5.0], [-0.0, 1.0], [float("inf"), 0.0], [float("nan"), 0.0], [2.0, 0.0]])
    q = torch.tensor([[0, 1, 0, 1, 0], [1, 1, 4, 2, 3]])
    c, s, st = ref.link_ranks(zs, zd, q)
    assert c.tolist() == [[2, 1, 1, 3], [0, 1, 1, 3], [1, 0, 0, 3], [3, 0, 0, 3], [-1, -1, -1, -1]] and st == ref.BAD_SCORE
    assert not np.signbit(s.numpy()[:2]).any() and s.tolist()[2:] == [2.0, float("-inf"), float("-inf")]
    lc, ls = _literal(zs, zd, q, None, True)
    assert torch.equal(c, lc) and torch.equal(s, ls)


def test_restatement_agrees_with_topk_through_rule_f_4():
    """greater + equal_before is the 0-based position of the target in ``_topk_ref.topk``'s list of its source when the pair is not
    excluded; an excluded (or loop) target is in no list"""
    seen = ties = excluded = 0
    for n_src, n_dst, F, loops in SHAPES:
        for maker in (tref.int_tables, tref.real_tables):
            zs, zd, ex, q = _inputs(n_src, n_dst, F, loops, maker)
            c, s, st = ref.link_ranks(zs, zd, q, ex, loops)
            assert st == 0
            k = 128
            ts, ti, _ = tref.topk(zs, zd, k, ex, None, loops)
            ok = tref.allowed(n_src, n_dst, ex, loops)
            for (src, dst), (g, e, b, n), sc in zip(q.t().tolist(), c.tolist(), s.tolist()):
                row = ti[src].tolist()
                assert n == int(ok[src].sum()) - int(ok[src, dst])
                if ok[src, dst]:
                    pos = g + b
                    assert (dst in row) == (pos < k)
                    if pos < k:
                        assert row[pos] == dst and float(ts[src, pos]) == sc
                else:
                    excluded += 1
                    assert dst not in row
                seen += 1
                ties += e > 0
    assert seen > 250 and ties > 50 and excluded > 50


def test_metrics_of_the_restatement():
    counts = np.array([[0, 0, 0, 9], [2, 2, 1, 9], [-1, -1, -1, -1], [9, 0, 0, 9]])
    assert ref.ranks(counts[[0, 1, 3]], "min").tolist() == [1, 3, 10] and ref.ranks(counts[[0, 1, 3]], "max").tolist() == [1, 5, 10]
    assert ref.ranks(counts[[0, 1, 3]], "average").tolist() == [1, 4, 10] and ref.ranks(counts[[0, 1, 3]], "id").tolist() == [1, 4, 10]
    m = ref.metrics(counts, ks=(1, 3, 10), ties="min")
    assert m["hits@1"] == 1 / 3 and m["hits@3"] == 2 / 3 and m["hits@10"] == 1.0 and m["mean_rank"] == 14 / 3
    assert abs(m["mrr"] - (1 + 1 / 3 + 0.1) / 3) < 1e-15
    assert all(np.isnan(v) for v in ref.metrics(counts[2:3]).values())


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("#define NPI_LINK_RANK_NO_LOOPS 1", "RULE F", "equal_before", "Out of scope: the by-target direction"):
        assert word in header, word
    assert header.index("RULE K") < header.index("RULE F")
    assert _lib.NPI_LINK_RANK_NO_LOOPS == 1
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "link_rank.hip" in SOURCES and "link_rank.hip" not in HOST_ONLY
    for name in ("link_ranks", "ranking_metrics", "LinkRanks"):
        assert name in npi.__all__ and hasattr(npi, name), name
    assert hasattr(npi.InnerProductDecoder, "ranks") and hasattr(npi.GAE, "test_ranking")
    # one tile producer, shared by its two users
    csrc = os.path.join(ROOT, "npi_gnn_amd", "csrc")
    assert "mfma_f32_32x32x2f32" in open(os.path.join(csrc, "score_tile.h")).read()
    for user in ("topk.hip", "link_rank.hip"):
        body = open(os.path.join(csrc, user)).read()
        assert '#include "score_tile.h"' in body and "mfma_f32_32x32x2f32" not in body, user


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG, P = None, 2 ** 31 - 1, 16                # P: a non-null, 16-byte aligned stand-in for a device pointer (never read)
    ws = lib.npi_link_ranks_workspace_bytes(100, 300, 0)

    def call(src=P, dst=P, Q=100, zs=P, lds=8, n_src=50, zd=P, ldd=8, n_dst=300, F=8, rowptr=P, col=P, flags=0, splits=0, counts=P,
             scores=P, work=P, nbytes=ws, status=N):
        return lib.npi_link_ranks(src, dst, Q, zs, lds, n_src, zd, ldd, n_dst, F, rowptr, col, flags, splits, counts, scores, work,
                                  nbytes, status, N)

    calls = {
        "null src": dict(src=N), "null dst": dict(dst=N), "null z_src": dict(zs=N), "null z_dst": dict(zd=N),
        "null counts": dict(counts=N), "null scores": dict(scores=N), "null workspace": dict(work=N),
        "rowptr without col": dict(col=N), "col without rowptr": dict(rowptr=N),
        "negative Q": dict(Q=-1), "Q 2^31 - 1": dict(Q=BIG, nbytes=2 ** 50), "negative n_src": dict(n_src=-1),
        "n_src 2^31 - 1": dict(n_src=BIG), "negative n_dst": dict(n_dst=-1), "n_dst 2^31 - 1": dict(n_dst=BIG, nbytes=2 ** 50),
        "F 0": dict(F=0), "negative F": dict(F=-8), "F 2^31 - 1": dict(F=BIG, lds=BIG, ldd=BIG),
        "pitch below F (source)": dict(lds=7), "pitch below F (target)": dict(ldd=7),
        "NO_LOOPS with two id spaces": dict(flags=_lib.NPI_LINK_RANK_NO_LOOPS), "unknown flag": dict(flags=2),
        "short workspace": dict(nbytes=ws - 1), "misaligned workspace": dict(work=24), "negative workspace size": dict(nbytes=-1),
        "negative splits": dict(splits=-1),
        "workspace of fewer splits": dict(splits=3, nbytes=lib.npi_link_ranks_workspace_bytes(100, 300, 3) - 16),
    }
    for name, kw in calls.items():
        assert call(**kw) == -1, name
        assert b"npi_link_ranks" in lib.npi_last_error(), (name, lib.npi_last_error())
    # nothing to do: no launch, no error, whatever the pointers
    assert call(Q=0) == 0
    assert call(src=N, dst=N, Q=0, zs=N, zd=N, rowptr=N, col=N, counts=N, scores=N, work=N, nbytes=0) == 0
    assert call(Q=0, n_src=300, flags=_lib.NPI_LINK_RANK_NO_LOOPS) == 0
    assert call(Q=0, F=0) == -1                                                       # ... but the sizes are still checked


def test_workspace_query():
    q = _lib.load().npi_link_ranks_workspace_bytes
    BIG = 2 ** 31 - 1
    for Q, n_dst in ((0, 0), (1, 1), (100, 300), (4636, 1700), (65536, 2 ** 20), (3, 10 ** 6)):
        sizes = [q(Q, n_dst, s) for s in (0, 1, 2, 3, 7, 64, 1000)]
        assert all(v > 0 and v % 16 == 0 for v in sizes), (Q, n_dst, sizes)
        assert sizes[1] >= max(Q, 1) * 20 and sizes[1] <= sizes[2] <= sizes[3] <= sizes[4] <= sizes[5] == sizes[6]
        assert sizes[0] <= sizes[5]
    for bad in ((-1, 10, 0), (BIG, 10, 0), (10, -1, 0), (10, BIG, 0), (10, 10, -1)):
        assert q(*bad) == -1, bad
    # the default split count is npi_topk_links': few queries are split so that they fill the chip, many are not
    assert q(64, 2 ** 20, 0) == q(64, 2 ** 20, 64) and q(65536, 2 ** 20, 0) == q(65536, 2 ** 20, 1)


# ---- the Python layer: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_function_argument_errors_and_no_cpu_fallback():
    z, zd = torch.randn(6, 4), torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    for bad_z in (None, "z", (z,), (z, zd, z), (z, None), [z, 3]):
        with pytest.raises(TypeError):
            npi.link_ranks(bad_z, ei)
    for bad_z in (z[0], (z, zd[:, :3]), torch.randn(6, 0), (z, zd[0])):
        with pytest.raises(ValueError):
            npi.link_ranks(bad_z, ei)
    for bad_z in (z.double(), (z, zd.half()), z.long()):
        with pytest.raises(TypeError):
            npi.link_ranks(bad_z, ei)
    with pytest.raises(NotImplementedError):
        npi.link_ranks(z.bfloat16(), ei)
    for bad_q in ("edges", [[0], [1]], 3, None):
        with pytest.raises(TypeError):
            npi.link_ranks(z, bad_q)
    for bad_q in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
        with pytest.raises(ValueError):
            npi.link_ranks(z, bad_q)
    for bad_ex in ("edges", [[0], [1]], 3):
        with pytest.raises(TypeError):
            npi.link_ranks(z, ei, exclude=bad_ex)
    for bad_ex in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
        with pytest.raises(ValueError):
            npi.link_ranks(z, ei, exclude=bad_ex)
    with pytest.raises(ValueError, match="allow_loops"):
        npi.link_ranks((z, zd), ei, allow_loops=False)
    with pytest.raises(ValueError, match="splits"):
        npi.link_ranks(z, ei, splits=-1)
    for bad_splits in (1.5, True, "2"):
        with pytest.raises(TypeError):
            npi.link_ranks(z, ei, splits=bad_splits)
    for bad_ks in (3, "13", None, (1, 2.0), (True,)):
        with pytest.raises(TypeError):
            npi.ranking_metrics(z, ei, ks=bad_ks)
    with pytest.raises(ValueError):
        npi.ranking_metrics(z, ei, ks=(1, 0))
    with pytest.raises(ValueError, match="ties"):
        npi.ranking_metrics(z, ei, ties="first")
    r = npi.LinkRanks(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2))
    with pytest.raises(ValueError, match="ties"):
        r.rank("first")
    assert r.rank("min").tolist() == [1, 1] and r.rank("average").dtype == torch.float64
    # arguments in order, tensors on the CPU
    model = npi.GAE(torch.nn.Identity())
    for call in (lambda: npi.link_ranks(z, ei), lambda: npi.link_ranks((z, zd), ei, exclude=ei, splits=3),
                 lambda: npi.link_ranks(z, ei, allow_loops=False), lambda: npi.ranking_metrics(z, ei, exclude=ei, ks=(1, 5), ties="id"),
                 lambda: npi.InnerProductDecoder().ranks(z, ei), lambda: npi.InnerProductDecoder().ranks((z, zd), ei, exclude=ei),
                 lambda: model.test_ranking(z, ei, ei), lambda: model.test_ranking((z, zd), ei, ei, ks=(1,))):
        with pytest.raises(npi.NpiError):
            call()
