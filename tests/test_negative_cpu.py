"""Negative sampling without a GPU: the two rules themselves (on the numpy restatement ``tests/_negative_ref.py``), the new C-ABI
symbols, the argument errors of the entry points and of ``NegativeSampler``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
import _negative_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("npi_negative_candidates", "npi_negative_targets", "npi_negative_distinct_workspace_bytes", "npi_negative_distinct")


# ---- the graphs of the statistical cases, shared with tests/test_gpu_negative.py -------------------------------------------------------
def mod4_graph():
    """n_src = n_dst = 32, edge iff (s + d) % 4 == 0: 256 edges, 768 non-edges; (edge_index, edge mask [32, 32])"""
    s, d = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    mask = (s + d) % 4 == 0
    return np.stack([s[mask], d[mask]]), mask


def even_targets_graph():
    """n_dst = 64, source 0 joined to the 32 even targets"""
    return np.stack([np.zeros(32, dtype=np.int64), np.arange(0, 64, 2)])


# ---- the rules -------------------------------------------------------------------------------------------------------------------------
def test_rule_p_is_uniform_over_the_non_edges():
    """4,096 draws of M = 192 of the 768 non-edges: every cell's inclusion count is Binomial(4096, 1/4), mean 1024, sigma 27.7; all
    768 within 6 sigma = 166 (false-alarm rate ~ 768 * 2e-9).  Seen: max deviation 95; 294 candidates consumed on average, 339 at
    most."""
    ei, mask = mod4_graph()
    counts = np.zeros((32, 32), dtype=np.int64)
    consumed = []
    for draw in range(4096):
        p, c = ref.pairs(ref.epoch_seed(0, draw), ei, 32, 32, 192, chunk=512)
        assert p.shape == (2, 192) and len(set(map(tuple, p.T))) == 192        # 192 distinct pairs
        counts[p[0], p[1]] += 1
        consumed.append(c)
    dev = np.abs(counts[~mask] - 1024)
    print("max deviation:", dev.max(), "candidates consumed: mean", np.mean(consumed), "max", max(consumed))
    assert counts[mask].sum() == 0                                             # no edge cell is ever drawn
    assert (dev <= 166).all(), counts


def test_rule_t_is_uniform_over_the_non_neighbours():
    """4,096 slots of source 0, joined to the 32 even of 64 targets: every odd target's count is Binomial(4096, 1/32), mean 128,
    sigma 11.1; all within 6 sigma = 67.  Seen: max deviation 19."""
    out = ref.corrupt(ref.epoch_seed(0, 0), even_targets_graph(), 1, 64, np.zeros(4096, dtype=np.int64))
    cnt = np.bincount(out, minlength=64)
    print("max deviation:", np.abs(cnt[1::2] - 128).max())
    assert (out >= 0).all() and cnt[0::2].sum() == 0                           # no even target is ever returned
    assert (np.abs(cnt[1::2] - 128) <= 67).all(), cnt


def test_rules_are_pure_functions_of_the_key_and_nested_in_m():
    ei, _ = mod4_graph()
    k0, k1 = ref.epoch_seed(0, 0), ref.epoch_seed(0, 1)
    a, ca = ref.pairs(k0, ei, 32, 32, 192)
    b, cb = ref.pairs(k0, ei, 32, 32, 192, chunk=7)                            # the round structure plays no part
    assert np.array_equal(a, b) and ca == cb
    assert not np.array_equal(a, ref.pairs(k1, ei, 32, 32, 192)[0])
    short, cs = ref.pairs(k0, ei, 32, 32, 50)
    assert np.array_equal(short, a[:, :50]) and cs <= ca                       # the first M' are a prefix of the first M > M'
    loops = ref.pairs(k0, ei, 32, 32, 192, no_loops=True)[0]
    assert (loops[0] != loops[1]).all() and (a[0] == a[1]).any()
    src = np.arange(32).repeat(8)
    t0 = ref.corrupt(k0, ei, 32, 32, src)
    assert np.array_equal(t0, ref.corrupt(k0, ei, 32, 32, src)) and not np.array_equal(t0, ref.corrupt(k1, ei, 32, 32, src))
    assert ((src + t0) % 4 != 0).all()
    # a full row, a bad id, tries running out
    full = np.stack([np.zeros(4, dtype=np.int64), np.arange(4)])
    assert ref.corrupt(k0, full, 2, 4, [0, 1, -1, 2]).tolist()[0::2] == [-1, -1] and ref.corrupt(k0, full, 2, 4, [0, 1, -1, 2])[3] == -1
    assert ref.mulhi(np.array([2 ** 64 - 1, 2 ** 63, 0], dtype=np.uint64), 10).tolist() == [9, 5, 0]
    assert ref.mulhi(np.array([2 ** 64 - 1], dtype=np.uint64), 2 ** 31 - 2).tolist() == [2 ** 31 - 3]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("0x9E3779B97F4A7C15", "0xD6E8FEB86659FD93", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",        # the hash written out
                 "src/generate_edgelist.py:108-139", "negative_sampling", "structured_negative_sampling",        # the calls replaced
                 "NPI_STATUS_NO_NEGATIVE 64", "NPI_STATUS_BAD_SOURCE_ID 128"):
        assert word in header, word
    assert _lib.NPI_STATUS_NO_NEGATIVE == 64 and _lib.NPI_STATUS_BAD_SOURCE_ID == 128
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import SOURCES
    assert "negative.hip" in SOURCES
    for name in ("NegativeSampler", "negative_sampling", "structured_negative_sampling"):
        assert name in npi.__all__ and hasattr(npi, name), name


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG = None, 2 ** 31 - 1
    ws = lib.npi_negative_distinct_workspace_bytes(100)
    calls = {
        "npi_negative_candidates (null)": lambda: lib.npi_negative_candidates(N, N, 4, 4, 0, 0, 8, 0, 16, 16, N),
        "npi_negative_candidates (null outputs)": lambda: lib.npi_negative_candidates(16, 16, 4, 4, 0, 0, 8, 0, N, N, N),
        "npi_negative_candidates (negative window)": lambda: lib.npi_negative_candidates(16, 16, 4, 4, 0, 0, -1, 0, 16, 16, N),
        "npi_negative_candidates (window 2^31 - 1)": lambda: lib.npi_negative_candidates(16, 16, 4, 4, 0, 0, BIG, 0, 16, 16, N),
        "npi_negative_candidates (n_src 2^31 - 1)": lambda: lib.npi_negative_candidates(16, 16, 4, BIG, 0, 0, 8, 0, 16, 16, N),
        "npi_negative_candidates (n_dst 2^31 - 1)": lambda: lib.npi_negative_candidates(16, 16, BIG, 4, 0, 0, 8, 0, 16, 16, N),
        "npi_negative_candidates (negative n_dst)": lambda: lib.npi_negative_candidates(16, 16, -4, 4, 0, 0, 8, 0, 16, 16, N),
        "npi_negative_candidates (negative first)": lambda: lib.npi_negative_candidates(16, 16, 4, 4, 0, -1, 8, 0, 16, 16, N),
        "npi_negative_candidates (flag)": lambda: lib.npi_negative_candidates(16, 16, 4, 4, 0, 0, 8, 2, 16, 16, N),
        "npi_negative_targets (null)": lambda: lib.npi_negative_targets(N, N, 4, 4, 16, 8, 0, 64, 16, N, N),
        "npi_negative_targets (null slots)": lambda: lib.npi_negative_targets(16, 16, 4, 4, N, 8, 0, 64, N, N, N),
        "npi_negative_targets (negative count)": lambda: lib.npi_negative_targets(16, 16, 4, 4, 16, -1, 0, 64, 16, N, N),
        "npi_negative_targets (count 2^31 - 1)": lambda: lib.npi_negative_targets(16, 16, 4, 4, 16, BIG, 0, 64, 16, N, N),
        "npi_negative_targets (n_src 2^31 - 1)": lambda: lib.npi_negative_targets(16, 16, 4, BIG, 16, 8, 0, 64, 16, N, N),
        "npi_negative_targets (n_dst 0)": lambda: lib.npi_negative_targets(16, 16, 0, 4, 16, 8, 0, 64, 16, N, N),
        "npi_negative_targets (tries 0)": lambda: lib.npi_negative_targets(16, 16, 4, 4, 16, 8, 0, 0, 16, N, N),
        "npi_negative_targets (tries -3)": lambda: lib.npi_negative_targets(16, 16, 4, 4, 16, 8, 0, -3, 16, N, N),
        "npi_negative_distinct (null)": lambda: lib.npi_negative_distinct(N, N, 100, 4, 4, 8, 16, 16, 16, 16, ws, N),
        "npi_negative_distinct (null info)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, 4, 8, 16, 16, N, 16, ws, N),
        "npi_negative_distinct (null outputs)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, 4, 8, N, N, 16, 16, ws, N),
        "npi_negative_distinct (null workspace)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, 4, 8, 16, 16, 16, N, ws, N),
        "npi_negative_distinct (negative window)": lambda: lib.npi_negative_distinct(16, 16, -1, 4, 4, 8, 16, 16, 16, 16, ws, N),
        "npi_negative_distinct (window 2^31 - 1)": lambda: lib.npi_negative_distinct(16, 16, BIG, 4, 4, 8, 16, 16, 16, 16, ws, N),
        "npi_negative_distinct (negative M)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, 4, -1, 16, 16, 16, 16, ws, N),
        "npi_negative_distinct (n_src 2^31 - 1)": lambda: lib.npi_negative_distinct(16, 16, 100, BIG, 4, 8, 16, 16, 16, 16, ws, N),
        "npi_negative_distinct (n_dst 2^31 - 1)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, BIG, 8, 16, 16, 16, 16, ws, N),
        "npi_negative_distinct (misaligned workspace)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, 4, 8, 16, 16, 16, 24, ws, N),
        "npi_negative_distinct (short workspace)": lambda: lib.npi_negative_distinct(16, 16, 100, 4, 4, 8, 16, 16, 16, 16, ws - 1, N),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.split()[0].encode() in lib.npi_last_error(), (name, lib.npi_last_error())
    assert lib.npi_negative_distinct_workspace_bytes(-1) == -1 and lib.npi_negative_distinct_workspace_bytes(BIG) == -1
    assert lib.npi_negative_distinct_workspace_bytes(0) > 0 and ws >= 16 * 100
    assert lib.npi_negative_distinct_workspace_bytes(300_000) >= 16 * 300_000
    # nothing to do: no launch, no error
    assert lib.npi_negative_candidates(16, 16, 4, 4, 0, 0, 0, 0, N, N, N) == 0
    assert lib.npi_negative_targets(16, 16, 4, 4, N, 0, 0, 64, N, N, N) == 0
    assert lib.npi_negative_distinct(N, N, 0, 4, 4, 8, N, N, 16, N, 0, N) == 0


# ---- NegativeSampler: argument errors, no CPU path --------------------------------------------------------------------------------------
def test_class_argument_errors_and_no_cpu_fallback():
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    for bad_ei in (ei.float(), ei.to(torch.int32), ei[0], [[0, 1], [1, 0]]):     # a LongTensor [2, E], nothing else
        with pytest.raises(ValueError):
            npi.NegativeSampler(bad_ei, size=(4, 4))
    for bad_size in ((0, 4), (4, -1), 0, -3, (4,), (4, 4, 4), (4.0, 4), "4", (2 ** 31 - 1, 4), True):
        with pytest.raises(ValueError):
            npi.NegativeSampler(ei, size=bad_size)
        with pytest.raises(ValueError):
            npi.negative_sampling(ei, bad_size)
    with pytest.raises(npi.NpiError):                                              # arguments in order, tensors on the CPU
        npi.NegativeSampler(ei, size=(4, 4))
    with pytest.raises(npi.NpiError):
        npi.NegativeSampler(ei, size=4, allow_loops=False)
    with pytest.raises(npi.NpiError):
        npi.negative_sampling(ei, 4, num_neg_samples=3)
    with pytest.raises(npi.NpiError):
        npi.structured_negative_sampling(ei, (4, 4))
    # the methods, with the constructor's device work out of reach
    neg = object.__new__(npi.NegativeSampler)
    neg.n_src, neg.n_dst, neg.num_edges, neg.num_non_edges, neg.seed, neg.draw = 4, 4, 4, 12, 0, 0
    neg.device, neg.allow_loops = torch.device("cpu"), True
    with pytest.raises(ValueError, match="num_neg_samples"):
        neg.pairs(num_neg_samples=-1)
    with pytest.raises(ValueError, match="window"):
        neg.pairs(window=0)
    neg.side = None
    with pytest.raises(npi.NpiError, match="2\\^31 - 1"):                          # refused before anything is launched
        neg.pairs(2, draw=0, window=2 ** 31 - 1)
    for tries in (0, -5):
        with pytest.raises(ValueError, match="tries"):
            neg.corrupt(torch.tensor([0, 1]), tries=tries)
    with pytest.raises(ValueError):
        neg.corrupt(torch.tensor([0.5, 1.0]))
    with pytest.raises(npi.NpiError):
        neg.corrupt(torch.tensor([0, 1]))
    assert neg.draw == 0                                                           # a refused call takes no draw number
