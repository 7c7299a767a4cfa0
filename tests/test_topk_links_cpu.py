"""Top-k link prediction without a GPU: the restatement ``tests/_topk_ref.py`` against a literal dense composition, the new C-ABI
symbols and constants, the argument refusals of ``npi_topk_links`` (all before the GPU is touched) and of the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
import _topk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npi_topk_links", "npi_topk_links_workspace_bytes")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _literal(z_src, z_dst, k, exclude, rows, allow_loops):
    """dense matmul -> mask -> stable sort by (-score, id), row by row in plain Python"""
    D = torch.matmul(z_src.double(), z_dst.double().t())
    n_src, n_dst = D.shape
    banned = set()
    if exclude is not None:
        banned = {(int(a), int(b)) for a, b in exclude.t().tolist()}
    out_s, out_i = [], []
    for i in (range(n_src) if rows is None else rows.tolist()):
        if not 0 <= i < n_src:
            out_s.append([float("-inf")] * k)
            out_i.append([-1] * k)
            continue
        js = [j for j in range(n_dst) if (i, j) not in banned and (allow_loops or i != j) and not torch.isnan(D[i, j])]
        js = sorted(js, key=lambda j: (-float(D[i, j].float()), j))[:k]
        out_s.append([float(D[i, j].float()) + 0.0 for j in js] + [float("-inf")] * (k - len(js)))
        out_i.append(js + [-1] * (k - len(js)))
    return torch.tensor(out_s, dtype=torch.float32).reshape(-1, k), torch.tensor(out_i, dtype=torch.int64).reshape(-1, k)


def test_restatement_equals_the_literal_dense_composition():
    cases = [(20, 30, 3, 5, True), (33, 33, 8, 40, False), (7, 1, 1, 3, True), (12, 50, 5, 128, True)]
    for n_src, n_dst, F, k, loops in cases:
        for maker in (ref.int_tables, ref.real_tables):
            zs, zd = maker(n_src, n_dst, F, seed=F)
            if not loops:
                zd = zs
            ex = ref.edges(n_src, n_dst, 3 * n_src, seed=k)
            rows = torch.tensor([n_src - 1, 0, 0, n_src, -1, 2 % n_src])
            for e, r in ((None, None), (ex, None), (ex, rows)):
                s, i, st = ref.topk(zs, zd, k, e, r, loops)
                ls, li = _literal(zs, zd, k, e, r, loops)
                assert torch.equal(i, li) and torch.equal(s, ls), (n_src, n_dst, F, k)
                assert st == (ref.BAD_SOURCE if r is not None else 0)
    # zeros of both signs tie and come out as +0.0; a NaN target is no candidate; +-inf are ordinary scores
    zs = torch.tensor([[1.0, 0.0], [-1.0, 0.0]])
    zd = torch.tensor([[0.0, 5.0], [-0.0, 1.0], [float("inf"), 0.0], [float("nan"), 0.0], [2.0, 0.0]])
    s, i, st = ref.topk(zs, zd, 5)
    assert i.tolist() == [[2, 4, 0, 1, -1], [0, 1, 4, 2, -1]] and st == ref.BAD_SCORE
    assert np.signbit(s.numpy()[:, :4]).tolist() == [[False] * 4, [False, False, True, True]]
    ls, li = _literal(zs, zd, 5, None, None, True)
    assert torch.equal(i, li) and torch.equal(s, ls)
    # the key: ascending key is descending score, one key for the two zeros
    v = np.array([np.inf, 3.0, 1e-40, 0.0, -0.0, -1e-40, -2.0, -np.inf], dtype=np.float32)
    key = ref.rank_key(v).astype(np.int64)
    assert key[3] == key[4] and (np.diff(np.delete(key, 4)) > 0).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("#define NPI_TOPK_MAX 128", "#define NPI_TOPK_NO_LOOPS 1", "RULE K", "InnerProductDecoder.forward_all", "case_study",
                 "torch.topk"):
        assert word in header, word
    assert (_lib.NPI_TOPK_MAX, _lib.NPI_TOPK_NO_LOOPS) == (128, 1)
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "topk.hip" in SOURCES and "topk.hip" not in HOST_ONLY
    for name in ("KnownLinks", "topk_links"):
        assert name in npi.__all__ and hasattr(npi, name), name
    assert hasattr(npi.InnerProductDecoder, "topk") and hasattr(npi.GAE, "predict")
    assert not hasattr(npi.InnerProductDecoder, "forward_all")
    # the key function lives in one header, shared by its two users
    csrc = os.path.join(ROOT, "npi_gnn_amd", "csrc")
    assert "rank_key(" in open(os.path.join(csrc, "rank_key.h")).read()
    for user in ("rank.hip", "topk.hip"):
        body = open(os.path.join(csrc, user)).read()
        assert '#include "rank_key.h"' in body and "uint32_t rank_key(" not in body, user


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG, P = None, 2 ** 31 - 1, 16                # P: a non-null, 16-byte aligned stand-in for a device pointer (never read)
    ws = lib.npi_topk_links_workspace_bytes(100, 300, 10, 0)

    def call(rows=P, R=100, zs=P, lds=8, n_src=50, zd=P, ldd=8, n_dst=300, F=8, k=10, rowptr=P, col=P, flags=0, splits=0, scores=P,
             ids=P, work=P, nbytes=ws, status=N):
        return lib.npi_topk_links(rows, R, zs, lds, n_src, zd, ldd, n_dst, F, k, rowptr, col, flags, splits, scores, ids, work, nbytes,
                                  status, N)

    calls = {
        "null z_src": dict(zs=N), "null z_dst": dict(zd=N), "null scores": dict(scores=N), "null ids": dict(ids=N),
        "null workspace": dict(work=N), "rowptr without col": dict(col=N), "col without rowptr": dict(rowptr=N),
        "k 0": dict(k=0), "k 129": dict(k=129), "negative k": dict(k=-1),
        "negative R": dict(R=-1), "R 2^31 - 1": dict(R=BIG, nbytes=2 ** 50), "negative n_src": dict(n_src=-1),
        "n_src 2^31 - 1": dict(n_src=BIG), "negative n_dst": dict(n_dst=-1), "n_dst 2^31 - 1": dict(n_dst=BIG, nbytes=2 ** 50),
        "F 0": dict(F=0), "negative F": dict(F=-8), "F 2^31 - 1": dict(F=BIG, lds=BIG, ldd=BIG),
        "pitch below F (source)": dict(lds=7), "pitch below F (target)": dict(ldd=7),
        "NO_LOOPS with two id spaces": dict(flags=_lib.NPI_TOPK_NO_LOOPS), "unknown flag": dict(flags=2),
        "short workspace": dict(nbytes=ws - 1), "misaligned workspace": dict(work=24), "negative workspace size": dict(nbytes=-1),
        "negative splits": dict(splits=-1),
        "workspace of fewer splits": dict(splits=3, nbytes=lib.npi_topk_links_workspace_bytes(100, 300, 10, 3) - 16),
    }
    for name, kw in calls.items():
        assert call(**kw) == -1, name
        assert b"npi_topk_links" in lib.npi_last_error(), (name, lib.npi_last_error())
    # nothing to do: no launch, no error, whatever the pointers
    assert call(R=0) == 0
    assert call(rows=N, R=0, zs=N, zd=N, rowptr=N, col=N, scores=N, ids=N, work=N, nbytes=0) == 0
    assert call(R=0, n_src=300, flags=_lib.NPI_TOPK_NO_LOOPS) == 0
    assert call(R=0, k=0) == -1                                                       # ... but the sizes are still checked


def test_workspace_query():
    q = _lib.load().npi_topk_links_workspace_bytes
    BIG = 2 ** 31 - 1
    for R, n_dst, k in ((0, 0, 1), (1, 1, 1), (100, 300, 10), (4636, 1700, 32), (65536, 2 ** 20, 32), (3, 10 ** 6, 128)):
        sizes = [q(R, n_dst, k, s) for s in (0, 1, 2, 3, 7, 64, 1000)]
        assert all(v > 0 and v % 16 == 0 for v in sizes), (R, n_dst, k, sizes)
        assert sizes[1] >= max(R, 1) * k * 8 and sizes[1] <= sizes[2] <= sizes[3] <= sizes[4] <= sizes[5] == sizes[6]
        assert sizes[0] <= sizes[5]
    for bad in ((-1, 10, 5, 0), (BIG, 10, 5, 0), (10, -1, 5, 0), (10, BIG, 5, 0), (10, 10, 0, 0), (10, 10, 129, 0), (10, 10, 5, -1)):
        assert q(*bad) == -1, bad
    # few queries are split so that they still fill the chip, many are not
    assert q(64, 2 ** 20, 8, 0) == q(64, 2 ** 20, 8, 64) and q(65536, 2 ** 20, 8, 0) == q(65536, 2 ** 20, 8, 1)


# ---- the Python layer: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_function_and_class_argument_errors_and_no_cpu_fallback():
    z, zd = torch.randn(6, 4), torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    for bad_z in (None, "z", (z,), (z, zd, z), (z, None), [z, 3]):
        with pytest.raises(TypeError):
            npi.topk_links(bad_z, 3)
    for bad_z in (z[0], (z, zd[:, :3]), torch.randn(6, 0), (z, zd[0])):
        with pytest.raises(ValueError):
            npi.topk_links(bad_z, 3)
    for bad_z in (z.double(), (z, zd.half()), z.long()):
        with pytest.raises(TypeError):
            npi.topk_links(bad_z, 3)
    with pytest.raises(NotImplementedError):
        npi.topk_links(z.bfloat16(), 3)
    with pytest.raises(NotImplementedError):
        npi.topk_links((z, zd.bfloat16()), 3)
    for bad_k in (2.0, "3", None, True):
        with pytest.raises(TypeError):
            npi.topk_links(z, bad_k)
    for bad_k in (0, -1, 129):
        with pytest.raises(ValueError, match="k must lie"):
            npi.topk_links(z, bad_k)
    for bad_ex in ("edges", [[0], [1]], 3):
        with pytest.raises(TypeError):
            npi.topk_links(z, 3, exclude=bad_ex)
    for bad_ex in (ei.float(), ei.to(torch.int32), ei[0], ei.t().contiguous()):
        with pytest.raises(ValueError):
            npi.topk_links(z, 3, exclude=bad_ex)
        with pytest.raises(ValueError):
            npi.KnownLinks(bad_ex, 6)
    for bad_rows in ([0, 1], 3):
        with pytest.raises(TypeError):
            npi.topk_links(z, 3, rows=bad_rows)
    for bad_rows in (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor([0, 1], dtype=torch.int32)):
        with pytest.raises(ValueError):
            npi.topk_links(z, 3, rows=bad_rows)
    with pytest.raises(ValueError, match="allow_loops"):
        npi.topk_links((z, zd), 3, allow_loops=False)
    with pytest.raises(ValueError, match="splits"):
        npi.topk_links(z, 3, splits=-1)
    with pytest.raises(TypeError):
        npi.topk_links(z, 3, splits=1.5)
    for bad_size in (None, 6.0, (6,), (6, 5, 4), (6, 5.0), True):
        with pytest.raises(TypeError):
            npi.KnownLinks(ei, bad_size)
    for bad_size in (0, (6, 0), (-1, 5), 2 ** 31 - 1):
        with pytest.raises(ValueError):
            npi.KnownLinks(ei, bad_size)
    # arguments in order, tensors on the CPU
    model = npi.GAE(torch.nn.Identity())
    for call in (lambda: npi.topk_links(z, 3), lambda: npi.topk_links((z, zd), 128, exclude=ei, rows=torch.tensor([0, 5])),
                 lambda: npi.topk_links(z, 1, allow_loops=False, splits=3), lambda: npi.KnownLinks(ei, 6),
                 lambda: npi.KnownLinks(ei, (6, 5)), lambda: npi.InnerProductDecoder().topk(z, 3),
                 lambda: npi.InnerProductDecoder().topk((z, zd), 3, exclude=ei, sigmoid=False), lambda: model.predict(z, 3, ei),
                 lambda: model.predict((z, zd), 3, ei, rows=torch.tensor([1]), sigmoid=False)):
        with pytest.raises(npi.NpiError):
            call()
