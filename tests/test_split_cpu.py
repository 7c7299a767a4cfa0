"""Edge splits without a GPU: Rule S itself (on the numpy restatement ``tests/_split_ref.py``), the new C-ABI symbols, the argument
errors of the entry points and of ``EdgeSplitter`` / ``train_test_split_edges`` / ``to_undirected``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
import _split_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("npi_split_workspace_bytes", "npi_split_permute", "npi_split_canonical", "npi_split_undirected_workspace_bytes",
       "npi_split_undirected")


# ---- the inputs of the statistical cases, shared with tests/test_gpu_split.py ------------------------------------------------------------
def columns24():
    """24 columns over two id spaces of 24: every one is kept"""
    return np.stack([np.arange(24), (7 * np.arange(24)) % 24]), (24, 24)


def mod4_undirected():
    """N = 32, edge iff (a + b) % 4 == 0, both orientations (and the loops (a, a) with a even); (edge_index, edge mask [32, 32])"""
    a, b = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    mask = (a + b) % 4 == 0
    return np.stack([a[mask], b[mask]]), mask


def uniformity(perms):
    """perms [draws, 24] (column at each position) -> (largest |count(c at p) - mean|, largest |count(c in [0, 6)) - mean|)"""
    draws = perms.shape[0]
    cell = np.zeros((24, 24), dtype=np.int64)
    np.add.at(cell, (perms, np.broadcast_to(np.arange(24), perms.shape)), 1)
    head = np.bincount(perms[:, :6].ravel(), minlength=24)
    return np.abs(cell - draws / 24).max(), np.abs(head - draws / 4).max()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_rule_s_is_a_uniform_permutation():
    """K = 24 kept columns, 4,096 draws.  Column c at position p: Binomial(4096, 1/24), mean 170.7, sigma 12.8 -- all 576 cells
    within 6 sigma = 77.  Column c in the test part [0, 6): Binomial(4096, 1/4), sigma 27.7 -- all 24 within 6 sigma = 166.
    Seen: 46.3 and 54."""
    ei, (n_src, n_dst) = columns24()
    perms = np.stack([ref.permutation(ref.epoch_seed(0, d), ei, n_src, n_dst, False)[1] for d in range(4096)])
    assert (np.sort(perms, axis=1) == np.arange(24)).all()                      # every draw is a permutation
    cell, head = uniformity(perms)
    print("largest deviation of a (column, position) cell:", cell, "of a column's count in the test part:", head)
    assert cell <= 77 and head <= 166


def test_rule_s_is_a_pure_function_of_the_key_and_the_input_column():
    rng = np.random.default_rng(0)
    ei = rng.integers(0, 20, size=(2, 200))
    k0, k1 = ref.epoch_seed(0, 0), ref.epoch_seed(0, 1)
    a, ea = ref.permutation(k0, ei, 20, 20, True)
    b, eb = ref.permutation(k0, ei, 20, 20, True)
    assert np.array_equal(a, b) and np.array_equal(ea, eb)
    assert not np.array_equal(ea, ref.permutation(k1, ei, 20, 20, True)[1])
    # upper drops the loops and the src > dst columns, and nothing else
    assert (a[0] < a[1]).all() and np.array_equal(np.sort(ea), np.nonzero(ei[0] < ei[1])[0])
    assert np.array_equal(ei[:, ea], a)
    full, ef = ref.permutation(k0, ei, 20, 20, False)
    assert np.array_equal(np.sort(ef), np.arange(200)) and (full[0] >= full[1]).any()
    # an out-of-range column in the middle: dropped, reported, and no other column's r_e moves (r_e depends on e alone)
    bad = np.concatenate([ei[:, :100], np.array([[3], [20]]), ei[:, 100:]], axis=1)
    kept, any_bad = ref.keep_mask(bad, 20, 20, False)
    assert any_bad and not kept[100] and kept.sum() == 200 and not ref.keep_mask(ei, 20, 20, False)[1]
    assert np.array_equal(ref.words(k0, 201)[:200], ref.words(k0, 200))
    eb2 = ref.permutation(k0, bad, 20, 20, False)[1]
    assert 100 not in eb2 and np.array_equal(np.sort(eb2), np.delete(np.arange(201), 100))
    head = ref.permutation(k0, ei[:, :100], 20, 20, False)[1]                  # the first 100 columns keep their mutual order
    assert np.array_equal(eb2[eb2 < 100], head) and np.array_equal(ef[ef < 100], head)
    assert len(np.unique(ref.words(k0, 100_000))) == 100_000                   # no ties
    # the parts
    assert ref.fold_bounds(23, 5) == [0, 4, 9, 13, 18, 23] and npi.split.fold_bounds(23, 5) == [0, 4, 9, 13, 18, 23]
    assert ref.part_sizes(1999, 0.05, 0.1) == (99, 199) and ref.part_sizes(10, 0.0, 1.0) == (0, 10)


def test_upper_negatives_are_distinct_upper_non_edges_and_nested_in_m():
    ei, mask = mod4_undirected()
    N, key = 32, ref.epoch_seed(0, 0)
    und = ref.to_undirected(ei, N)
    assert np.array_equal(und, np.stack(np.nonzero(mask)))                     # already undirected: sorted, itself
    upper_non = {(a, b) for a in range(N) for b in range(a + 1, N) if not mask[a, b]}
    assert ref.num_upper_non_edges(ei, N) == len(upper_non) == 376
    neg = ref.upper_negatives(key, ei, N, 100)
    assert neg.shape == (2, 100) and (neg[0] < neg[1]).all() and len(set(map(tuple, neg.T))) == 100
    assert not mask[neg[0], neg[1]].any() and not mask[neg[1], neg[0]].any()
    assert np.array_equal(ref.upper_negatives(key, ei, N, 100, chunk=7), neg)   # the round structure plays no part
    assert np.array_equal(ref.upper_negatives(key, ei, N, 30), neg[:, :30])     # the first M' are a prefix of the first M > M'
    assert not np.array_equal(ref.upper_negatives(ref.epoch_seed(0, 1), ei, N, 100), neg)
    every = ref.upper_negatives(key, ei, N, 10_000)                              # clamped: exactly the upper non-edges
    assert every.shape == (2, 376) and set(map(tuple, every.T)) == upper_non
    # one orientation only gives the same undirected form
    assert np.array_equal(ref.to_undirected(ei[:, ei[0] <= ei[1]], N), und)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    rule = header[header.index("Edge splits:"):]                             # the section and Rule S in it
    for word in ("mix64(mix64(mix64(key) + 5 * G))", "mix64(base + G * (e + 1))", "src/generate_edgelist.py:460-494",
                 "src/train.py:108-184", "NPI_SPLIT_UPPER 1", "NPI_STATUS_BAD_PAIR_ID"):
        assert word in rule, word
    assert "train_test_split_edges" in header and _lib.NPI_SPLIT_UPPER == 1
    assert _lib.load().npi_abi_version() == 4                                  # additive
    from npi_gnn_amd.build import HOST_ONLY, SOURCES
    assert "split.hip" in SOURCES and "split.hip" not in HOST_ONLY
    for name in ("EdgeSplitter", "train_test_split_edges", "to_undirected"):
        assert name in npi.__all__ and hasattr(npi, name), name


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG = None, 2 ** 31 - 1
    ws = lib.npi_split_workspace_bytes(100)
    wu = lib.npi_split_undirected_workspace_bytes(100)
    permute = lambda src=16, dst=16, E=100, n_src=4, n_dst=4, flags=0, o1=16, o2=16, o3=16, info=16, w=16, wb=ws: \
        lib.npi_split_permute(src, dst, E, n_src, n_dst, 0, flags, o1, o2, o3, info, N, w, wb, N)        # noqa: E731
    undirected = lambda src=16, dst=16, E=100, n=4, o1=16, o2=16, o3=16, info=16, w=16, wb=wu: \
        lib.npi_split_undirected(src, dst, E, n, o1, o2, o3, info, N, w, wb, N)                             # noqa: E731
    calls = {
        "npi_split_permute (null input)": lambda: permute(src=N),
        "npi_split_permute (null dst)": lambda: permute(dst=N),
        "npi_split_permute (null output)": lambda: permute(o2=N),
        "npi_split_permute (null e_id)": lambda: permute(o3=N),
        "npi_split_permute (null info)": lambda: permute(info=N),
        "npi_split_permute (null info, empty)": lambda: permute(E=0, info=N),
        "npi_split_permute (null workspace)": lambda: permute(w=N),
        "npi_split_permute (negative E)": lambda: permute(E=-1),
        "npi_split_permute (E 2^31 - 1)": lambda: permute(E=BIG),
        "npi_split_permute (n_src 2^31 - 1)": lambda: permute(n_src=BIG),
        "npi_split_permute (n_dst 2^31 - 1)": lambda: permute(n_dst=BIG),
        "npi_split_permute (n_src 0)": lambda: permute(n_src=0),
        "npi_split_permute (negative n_dst)": lambda: permute(n_dst=-4),
        "npi_split_permute (flag 2)": lambda: permute(flags=2),
        "npi_split_permute (flag -1)": lambda: permute(flags=-1),
        "npi_split_permute (misaligned workspace)": lambda: permute(w=24),
        "npi_split_permute (short workspace)": lambda: permute(wb=ws - 1),
        "npi_split_canonical (null)": lambda: lib.npi_split_canonical(N, 16, 8, N),
        "npi_split_canonical (null dst)": lambda: lib.npi_split_canonical(16, N, 8, N),
        "npi_split_canonical (negative window)": lambda: lib.npi_split_canonical(16, 16, -1, N),
        "npi_split_canonical (window 2^31 - 1)": lambda: lib.npi_split_canonical(16, 16, BIG, N),
        "npi_split_undirected (null input)": lambda: undirected(src=N),
        "npi_split_undirected (null output)": lambda: undirected(o1=N),
        "npi_split_undirected (null e_id)": lambda: undirected(o3=N),
        "npi_split_undirected (null info)": lambda: undirected(info=N),
        "npi_split_undirected (null workspace)": lambda: undirected(w=N),
        "npi_split_undirected (negative E)": lambda: undirected(E=-1),
        "npi_split_undirected (2 E at 2^31)": lambda: undirected(E=2 ** 30),
        "npi_split_undirected (N 2^31 - 2)": lambda: undirected(n=BIG - 1),
        "npi_split_undirected (N 0)": lambda: undirected(n=0),
        "npi_split_undirected (misaligned workspace)": lambda: undirected(w=24),
        "npi_split_undirected (short workspace)": lambda: undirected(wb=wu - 1),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.split()[0].encode() in lib.npi_last_error(), (name, lib.npi_last_error())
    for query in (lib.npi_split_workspace_bytes, lib.npi_split_undirected_workspace_bytes):
        assert query(-1) == -1 and query(BIG) == -1 and query(0) > 0
    assert lib.npi_split_undirected_workspace_bytes(2 ** 30) == -1
    assert ws >= 20 * 100 and lib.npi_split_workspace_bytes(300_000) >= 20 * 300_000     # the sorter's four arrays and the positions
    # an existing entry point keeps refusing what it refused: the canonical form is a call of its own, not a flag of the candidates
    assert lib.npi_negative_candidates(16, 16, 4, 4, 0, 0, 8, 2, 16, 16, N) == -1
    # nothing to do: no kernel, no error (the empty input's info[0] = 0 is a memset on the stream: tests/test_gpu_split.py)
    assert lib.npi_split_canonical(N, N, 0, N) == 0


# ---- EdgeSplitter: argument errors, no CPU path ------------------------------------------------------------------------------------------
def test_class_argument_errors_and_no_cpu_fallback():
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    for bad_ei in (ei.float(), ei.to(torch.int32), ei[0], [[0, 1], [1, 0]], torch.zeros(3, 4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            npi.EdgeSplitter(bad_ei, 4)
        with pytest.raises(ValueError):
            npi.train_test_split_edges(bad_ei, 4)
        with pytest.raises(ValueError):
            npi.to_undirected(bad_ei, 4)
    for bad_size in ((0, 4), (4, -1), 0, -3, (4,), (4, 4, 4), (4.0, 4), "4", (2 ** 31 - 1, 4), 2 ** 31 - 2, True, 4.0):
        with pytest.raises(ValueError):
            npi.EdgeSplitter(ei, bad_size)
    for bad_n in (0, -3, (4, 4), "4", 2 ** 31 - 2, True, 4.0):
        with pytest.raises(ValueError):
            npi.train_test_split_edges(ei, bad_n)
        with pytest.raises(ValueError):
            npi.to_undirected(ei, bad_n)
    for v, t in ((-0.1, 0.1), (0.1, -0.1), (1.5, 0.0), (0.0, 1.01), (0.6, 0.5)):
        with pytest.raises(ValueError, match="ratio"):
            npi.train_test_split_edges(ei, 4, val_ratio=v, test_ratio=t)
    with pytest.raises(npi.NpiError):                                              # arguments in order, tensors on the CPU
        npi.EdgeSplitter(ei, 4)
    with pytest.raises(npi.NpiError):
        npi.EdgeSplitter(ei, (4, 4))
    with pytest.raises(npi.NpiError):
        npi.train_test_split_edges(ei, 4)
    with pytest.raises(npi.NpiError):
        npi.to_undirected(ei, 4)
    # the methods, with the constructor's device work out of reach
    sp = object.__new__(npi.EdgeSplitter)
    sp.n_src, sp.n_dst, sp.num_edges, sp.seed, sp.draw, sp.upper = 4, 4, 4, 0, 0, True
    for v, t in ((-0.1, 0.1), (0.1, 1.5), (0.6, 0.5)):
        with pytest.raises(ValueError, match="ratio"):
            sp.split(val_ratio=v, test_ratio=t)
    for k in (1, 0, -2, 2.0, True):
        with pytest.raises(ValueError, match="k"):
            sp.kfold(k=k)
    assert sp.draw == 0                                                            # a refused call takes no draw number
    neg = object.__new__(npi.NegativeSampler)                                      # the canonical form: one id space, no loops
    neg.n_src, neg.n_dst, neg.num_edges, neg.num_non_edges, neg.seed, neg.draw, neg.allow_loops = 4, 4, 4, 12, 0, 0, True
    with pytest.raises(ValueError, match="canonical"):
        neg.pairs(2, canonical=True)
    assert neg.draw == 0
