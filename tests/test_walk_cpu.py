"""Random walks and Node2Vec without a GPU: Rule W and the pair layout themselves (on the numpy restatement ``tests/_walk_ref.py``),
the new C-ABI symbols, the argument errors of the entry points and of ``RandomWalker`` / ``Node2Vec``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import walk as npi_walk
import _walk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("npi_random_walk", "npi_walk_pairs")
ONE = 2 ** 32


# ---- the graphs and verdicts of the statistical cases, shared with tests/test_gpu_walk.py ----------------------------------------------
def star_graph():
    """node 0 -> nodes 1 .. 100 (directed: every leaf is a dead end); N = 101"""
    return np.stack([np.zeros(100, dtype=np.int64), np.arange(1, 101)]), 101


def house_graph():
    """undirected edges {0-1, 0-2, 0-3, 1-2, 3-4} in both directions, node 5 isolated; N = 6"""
    e = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [3, 4]]).T
    return np.concatenate([e, e[::-1]], axis=1), 6


def branchy_graph():
    """A directed graph that holds every branch of the walk kernel, N = 300: node 0 with 100 out-edges, nodes 1 .. 269 with random
    out-edges, 270 .. 279 with exactly one, 280 .. 289 reachable but without out-edges (dead ends), 290 .. 299 isolated; self loops at
    10 .. 19, 200 columns repeated (parallel edges), shuffled.  ``(edge_index, 300)``"""
    rng = np.random.default_rng(23)
    hub = np.stack([np.zeros(100, dtype=np.int64), rng.permutation(290)[:100]])
    rand = np.stack([rng.integers(1, 270, 1500), rng.integers(0, 290, 1500)])
    one = np.stack([np.arange(270, 280), rng.integers(0, 290, 10)])
    one[1, 0], one[1, 1] = 285, 271                                  # 270 -> a dead end; 271 -> itself (its only edge: a self loop)
    loops = np.stack([np.arange(10, 20), np.arange(10, 20)])
    ei = np.concatenate([hub, rand, one, loops], axis=1)
    ei = np.concatenate([ei, ei[:, rng.integers(100, 1600, 200)]], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    deg = np.bincount(ei[0], minlength=300)
    assert deg[0] == 100 and (deg[270:280] == 1).all() and deg[280:].sum() == 0 and np.bincount(ei[1], minlength=300)[290:].sum() == 0
    assert np.isin(np.arange(280, 290), ei[1]).any() and len(np.unique(ei[0] * 300 + ei[1])) < ei.shape[1]
    return ei, 300


def check_uniform_pick(w):
    """40,000 walks of 3 steps from the centre of the star: chi^2 of the first step over the 100 leaves below the 99.9 % quantile
    of chi^2(99), 148.2; every walk stays at its leaf (a dead end) for steps 2 and 3"""
    assert w.shape == (40_000, 4) and (w[:, 0] == 0).all()
    cnt = np.bincount(w[:, 1], minlength=101)
    chi2 = float(((cnt[1:] - 400.0) ** 2 / 400.0).sum())
    print("chi^2:", chi2)
    assert cnt[0] == 0 and cnt.sum() == 40_000 and chi2 < 148.2, chi2
    assert (w[:, 2] == w[:, 1]).all() and (w[:, 3] == w[:, 1]).all()
    return chi2


def check_pq_bias(w):
    """40,000 walks of 2 steps from node 1 with p = 0.5, q = 2: among those that went to node 0, the second step returns to 1,
    moves to the common neighbour 2 or away to 3 with weights (1/p, 1, 1/q) = (2, 1, 0.5); each frequency within 5 binomial
    standard deviations"""
    assert w.shape == (40_000, 3) and (w[:, 0] == 1).all() and np.isin(w[:, 1], [0, 2]).all()
    sel = w[w[:, 1] == 0, 2]
    n = len(sel)
    assert np.isin(sel, [1, 2, 3]).all()
    zs = []
    for node, weight in ((1, 2.0), (2, 1.0), (3, 0.5)):
        pr = weight / 3.5
        zs.append(abs((sel == node).sum() - n * pr) / np.sqrt(n * pr * (1 - pr)))
    print("walks through node 0:", n, "|z|:", zs)
    assert n > 15_000 and max(zs) <= 5.0, (n, zs)
    return n, max(zs)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def test_threshold_arithmetic():
    assert ref.thresholds(1, 1) == (ONE, ONE, ONE) == npi_walk.walk_thresholds(1, 1) == npi_walk.walk_thresholds(1.0, 1.0)
    assert ref.thresholds(0.5, 2) == (2 ** 32, 2 ** 31, 2 ** 30) == npi_walk.walk_thresholds(0.5, 2)
    assert npi_walk.walk_thresholds(4, 0.25) == (2 ** 28, 2 ** 30, 2 ** 32) == ref.thresholds(4, 0.25)
    assert npi_walk.walk_thresholds(3, 3) == (ONE // 3, ONE, ONE // 3)           # floor(2^32 / 3), in double exactly
    assert npi_walk.walk_thresholds(1e-300, 1e300) == (ONE, 0, 0)
    for p, q in ((0, 1), (1, 0), (-1, 1), (1, -2.0), (float("inf"), 1), (1, float("nan")), (1e-320, 1)):
        with pytest.raises(ValueError, match="positive and finite"):
            npi_walk.walk_thresholds(p, q)


def test_uniform_pick_statistics():
    """observed: chi^2 = 108.4"""
    ei, N = star_graph()
    w, exhausted = ref.walks(ref.epoch_seed(0, 0), ei, N, np.zeros(40_000, dtype=np.int64), 3)
    assert exhausted == 0
    check_uniform_pick(w)


def test_pq_bias_statistics():
    """observed: 20,024 walks through node 0, |z| <= 1.04, no step out of tries"""
    ei, N = house_graph()
    w, exhausted = ref.walks(ref.epoch_seed(0, 0), ei, N, np.ones(40_000, dtype=np.int64), 2, thr=ref.thresholds(0.5, 2), tries=64)
    assert exhausted == 0
    check_pq_bias(w)


def test_tries_run_out():
    """one try per step with p = 0.5, q = 2: a rejected candidate is taken all the same and counted (observed: 4,333 of 16,000
    steps)"""
    ei, N = house_graph()
    start = np.ones(2000, dtype=np.int64)
    w, exhausted = ref.walks(ref.epoch_seed(0, 0), ei, N, start, 8, thr=ref.thresholds(0.5, 2), tries=1)
    print("steps out of tries:", exhausted)
    assert exhausted > 0
    rowptr, col = ref.by_source_csr(ei, N)
    codes = set((ei[0] * N + ei[1]).tolist())
    assert all(int(a) * N + int(b) in codes for a, b in zip(w[:, :-1].ravel(), w[:, 1:].ravel()))     # every step is an edge
    # one try takes its candidate whether accepted or not: the walks of p = q = 1, where nothing runs out; more tries change them
    # from the second step on (the first has no previous node)
    u, none = ref.walks(ref.epoch_seed(0, 0), ei, N, start, 8, tries=1)
    assert none == 0 and np.array_equal(u, w)
    b, few = ref.walks(ref.epoch_seed(0, 0), ei, N, start, 8, thr=ref.thresholds(0.5, 2), tries=2)
    assert 0 < few < exhausted and np.array_equal(b[:, :2], w[:, :2]) and not np.array_equal(b, w)


def test_dead_ends_bad_starts_and_purity():
    # 0 -> 1 -> 2 (dead end), 3 isolated, parallel edge 0 -> 1 twice, self loop at 4
    ei = np.array([[0, 0, 1, 4], [1, 1, 2, 4]])
    start = np.array([0, 3, -1, 5, 2, 4, 0])
    k0, k1 = ref.epoch_seed(0, 0), ref.epoch_seed(0, 1)
    for thr in ((ONE, ONE, ONE), ref.thresholds(0.5, 2)):
        w, exhausted = ref.walks(k0, ei, 5, start, 4, thr=thr)
        assert exhausted == 0
        assert w.tolist() == [[0, 1, 2, 2, 2], [3, 3, 3, 3, 3], [-1] * 5, [-1] * 5, [2, 2, 2, 2, 2], [4, 4, 4, 4, 4], [0, 1, 2, 2, 2]]
    assert ref.walks(k0, ei, 5, start, 0)[0].tolist() == [[0], [3], [-1], [-1], [2], [4], [0]]
    # a pure function of the key; one stream per SLOT: the prefix of a longer call, and repeated starts differ
    ei, N = house_graph()
    start = np.zeros(64, dtype=np.int64)
    a = ref.walks(k0, ei, N, start, 6)[0]
    assert np.array_equal(a, ref.walks(k0, ei, N, start, 6)[0]) and not np.array_equal(a, ref.walks(k1, ei, N, start, 6)[0])
    assert np.array_equal(ref.walks(k0, ei, N, start[:5], 6)[0], a[:5]) and len(np.unique(a, axis=0)) > 32
    assert np.array_equal(ref.walks(k0, ei, N, start, 3)[0], a[:, :4])            # ... and nested in L
    # p = q = 1 through the general path (thresholds one below 2^32 would differ; exactly 2^32 accepts every word)
    b, _ = ref.walks(k0, ei, N, start, 6, thr=(ONE, ONE, ONE), tries=1)
    assert np.array_equal(a, b)


def test_pair_layout_is_pygs_slicing():
    """PyG 1.4.2 ``Node2Vec.__random_walk__`` / ``loss`` on a hand-made walks tensor: windows ``rw[:, j:j + c]`` concatenated along
    dim 0, ``start = walk[:, 0]``, ``rest = walk[:, 1:]``"""
    rw = torch.tensor([[0, 1, 2, 3, 4], [10, 11, 12, 13, 14], [-1, -1, -1, -1, -1]])
    for c, S in ((2, 1), (3, 2), (5, 3), (4, 0)):
        walk = torch.cat([rw[:, j:j + c] for j in range(1 + 4 + 1 - c)], dim=0)
        start, rest = walk[:, 0], walk[:, 1:].contiguous()
        got, n_pos = ref.pairs(ref.epoch_seed(0, 0), rw.numpy(), c, S, 20)
        R = walk.size(0)
        assert n_pos == R * (c - 1) and got.shape == (2, R * (c - 1 + S))
        assert torch.equal(torch.from_numpy(got[0, :n_pos]), start.view(-1, 1).expand(R, c - 1).reshape(-1))
        assert torch.equal(torch.from_numpy(got[1, :n_pos]), rest.view(-1))
        assert torch.equal(torch.from_numpy(got[0, n_pos:]), start.view(-1, 1).expand(R, S).reshape(-1))
        assert ((got[1, n_pos:] >= 0) & (got[1, n_pos:] < 20)).all()
    # the negatives: a counter-based stream over (row, sample), so fewer walks see a prefix-compatible stream only per row count
    a, _ = ref.pairs(ref.epoch_seed(0, 0), rw.numpy(), 3, 2, 20)
    b, _ = ref.pairs(ref.epoch_seed(0, 1), rw.numpy(), 3, 2, 20)
    assert np.array_equal(a[:, :18], b[:, :18]) and not np.array_equal(a[1, 18:], b[1, 18:])
    big, _ = ref.pairs(ref.epoch_seed(0, 0), np.zeros((500, 5), dtype=np.int64), 3, 4, 7)
    cnt = np.bincount(big[1, 3000:], minlength=7)                                  # 6,000 draws over 7 nodes: mean 857, sigma 27
    assert cnt.sum() == 6000 and (np.abs(cnt - 6000 / 7) < 6 * 27.1).all(), cnt


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    for word in ("RULE W", "root    = mix64(mix64(key) + 3 * G)", "nbase = mix64(mix64(key) + 4 * G)", "node2vec-master/src/main.py",
                 "torch_cluster.random_walk", "NPI_STATUS_WALK_TRIES 512"):
        assert word in header, word
    assert _lib.NPI_STATUS_WALK_TRIES == 512
    assert _lib.load().npi_abi_version() == 4
    from npi_gnn_amd.build import SOURCES
    assert "walk.hip" in SOURCES
    for name in ("RandomWalker", "random_walk", "Node2Vec"):
        assert name in npi.__all__ and hasattr(npi, name), name


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N, BIG = None, 2 ** 31 - 1

    def walk(rowptr=16, col=16, n=4, start=16, W=8, L=5, key=0, thr=(ONE, ONE, ONE), tries=64, walks=16, status=N):
        return lib.npi_random_walk(rowptr, col, n, start, W, L, key, thr[0], thr[1], thr[2], tries, walks, status, N)

    def pairs(walks=16, W=8, L=5, c=3, S=2, n=4, src=16, dst=16):
        return lib.npi_walk_pairs(walks, W, L, c, S, n, 0, src, dst, N)

    calls = {
        "npi_random_walk (null graph)": lambda: walk(rowptr=N, col=N),
        "npi_random_walk (null start)": lambda: walk(start=N),
        "npi_random_walk (null walks)": lambda: walk(walks=N),
        "npi_random_walk (negative count)": lambda: walk(W=-1),
        "npi_random_walk (count 2^31 - 1)": lambda: walk(W=BIG),
        "npi_random_walk (negative length)": lambda: walk(L=-1),
        "npi_random_walk (N 0)": lambda: walk(n=0),
        "npi_random_walk (N 2^31 - 1)": lambda: walk(n=BIG),
        "npi_random_walk (tries 0)": lambda: walk(tries=0),
        "npi_random_walk (tries -3)": lambda: walk(tries=-3),
        "npi_random_walk (thr_ret 2^32 + 1)": lambda: walk(thr=(ONE + 1, ONE, ONE)),
        "npi_random_walk (thr_nbr 2^32 + 1)": lambda: walk(thr=(ONE, ONE + 1, ONE)),
        "npi_random_walk (thr_far -1)": lambda: walk(thr=(ONE, ONE, -1)),
        "npi_walk_pairs (null walks)": lambda: pairs(walks=N),
        "npi_walk_pairs (null outputs)": lambda: pairs(src=N, dst=N),
        "npi_walk_pairs (negative count)": lambda: pairs(W=-1),
        "npi_walk_pairs (count 2^31 - 1)": lambda: pairs(W=BIG),
        "npi_walk_pairs (negative length)": lambda: pairs(L=-1),
        "npi_walk_pairs (negative samples)": lambda: pairs(S=-1),
        "npi_walk_pairs (N 0)": lambda: pairs(n=0),
        "npi_walk_pairs (N 2^31 - 1)": lambda: pairs(n=BIG),
        "npi_walk_pairs (c 1)": lambda: pairs(c=1),
        "npi_walk_pairs (c L + 2)": lambda: pairs(c=7),
        "npi_walk_pairs (M 2^31 - 1)": lambda: pairs(W=2 ** 28, L=5, c=3, S=0),          # R = 4 * 2^28, M = 2^31
        "npi_walk_pairs (M through S)": lambda: pairs(W=2 ** 20, L=5, c=3, S=2 ** 9),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.split()[0].encode() in lib.npi_last_error(), (name, lib.npi_last_error())
    # nothing to do: no launch, no error
    assert walk(start=N, W=0, walks=N) == 0
    assert pairs(walks=N, W=0, src=N, dst=N) == 0


# ---- RandomWalker / Node2Vec: argument errors, no CPU path ------------------------------------------------------------------------------
def test_class_argument_errors_and_no_cpu_fallback():
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    for bad_ei in (ei.float(), ei.to(torch.int32), ei[0], [[0, 1], [1, 0]]):
        with pytest.raises(ValueError):
            npi.RandomWalker(bad_ei, 4)
    for bad_n in (0, -3, 4.0, "4", 2 ** 31 - 1, True, (4, 4)):
        with pytest.raises(ValueError, match="num_nodes"):
            npi.RandomWalker(ei, bad_n)
    for kw in (dict(p=0), dict(q=-1.0), dict(p=float("inf")), dict(q=float("nan")), dict(tries=0), dict(tries=-2)):
        with pytest.raises(ValueError):
            npi.RandomWalker(ei, 4, **kw)
    with pytest.raises(npi.NpiError):                                              # arguments in order, tensors on the CPU
        npi.RandomWalker(ei, 4)
    with pytest.raises(npi.NpiError):
        npi.random_walk(ei[0], ei[1], torch.tensor([0, 1]), 3, num_nodes=4)
    with pytest.raises(ValueError):
        npi.random_walk(ei[0], ei[1][:2], torch.tensor([0, 1]), 3, num_nodes=4)
    # the method, with the constructor's device work out of reach
    rw = object.__new__(npi.RandomWalker)
    rw.num_nodes, rw.seed, rw.draw, rw.tries, rw.thresholds, rw.device, rw.side = 4, 0, 0, 64, (ONE, ONE, ONE), torch.device("cpu"), None
    for bad_len in (-1, 2.0, True, 2 ** 31 - 1):
        with pytest.raises(ValueError, match="walk_length"):
            rw.walks(torch.tensor([0, 1]), bad_len)
    for bad_start in (torch.tensor([0.5]), torch.tensor([[0, 1]]), [0, 1]):
        with pytest.raises(ValueError, match="start"):
            rw.walks(bad_start, 3)
    with pytest.raises(npi.NpiError):
        rw.walks(torch.tensor([0, 1]), 3)
    assert rw.draw == 0                                                            # a refused call takes no draw number


def test_node2vec_is_pygs_module_on_the_host():
    model = npi.Node2Vec(50, 16, walk_length=8, context_size=4, walks_per_node=2)
    sd = model.state_dict()
    assert list(sd) == ["embedding.weight"] and tuple(sd["embedding.weight"].shape) == (50, 16)
    assert model.num_negative_samples == 3 and model.draw == 0
    assert npi.Node2Vec(50, 16, 8, 4, num_negative_samples=7).num_negative_samples == 7
    model.load_state_dict({"embedding.weight": torch.ones(50, 16)})                # a PyG checkpoint's layout
    assert torch.equal(model(torch.tensor([3, 4])), torch.ones(2, 16))
    with pytest.raises(AssertionError):
        npi.Node2Vec(50, 16, walk_length=3, context_size=4)
    for kw in (dict(p=0), dict(q=float("inf")), dict(num_negative_samples=-1), dict(walks_per_node=0)):
        with pytest.raises(ValueError):
            npi.Node2Vec(50, 16, 8, 4, **kw)
    with pytest.raises(ValueError):
        npi.Node2Vec(50, 16, 8, 1)                                                 # a window of one node has no pair
    with pytest.raises(npi.NpiError):                                              # no CPU path
        model.loss(torch.tensor([[0, 1], [1, 0]]))
    assert model.draw == 0
