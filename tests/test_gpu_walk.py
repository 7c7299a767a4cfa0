"""``npi.RandomWalker`` / ``npi_walk_pairs`` on the GPU: every walk and every pair against the numpy restatement of Rule W
(``tests/_walk_ref.py``, checked by ``tests/test_walk_cpu.py``) element for element, the statistics of the rule through the class
with the bounds and seeds of the CPU cases, and the structural properties (a stream belongs to a slot, replay, capture)."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import graph as NG
from npi_gnn_amd import walk as npi_walk
import _walk_ref as ref
from test_walk_cpu import branchy_graph, check_pq_bias, check_uniform_pick, house_graph, star_graph

pytestmark = pytest.mark.gpu

_CACHE = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _starts():
    """1,000 starts on ``branchy_graph``: random ones (repeats), the hub, one-edge rows, dead ends, an isolated node and two ids
    out of range"""
    if "starts" not in _CACHE:
        s = np.random.default_rng(4).integers(0, 300, 1000)
        s[:8] = [0, 0, 270, 271, 285, 295, 0, 12]
        s[500], s[999] = -1, 300
        _CACHE["starts"] = s
    return _CACHE["starts"]


def _want(L, pq, tries, seed=0, draw=0):
    key = ("walks", L, pq, tries, seed, draw)
    if key not in _CACHE:
        ei, N = branchy_graph()
        _CACHE[key] = ref.walks(ref.epoch_seed(seed, draw), ei, N, _starts(), L, thr=ref.thresholds(*pq), tries=tries)
    return _CACHE[key]


def _status_bits(dev):
    """the OR of the status words filed since the last check (taken off the pending list)"""
    bits = 0
    for t in NG.pending_status(dev):
        bits |= int(t.item())
    return bits


@pytest.mark.parametrize("tries", [64, 1])
@pytest.mark.parametrize("pq", [(1, 1), (0.5, 2), (4, 0.25)])
@pytest.mark.parametrize("L", [1, 7, 80])
def test_walks_equal_the_restatement(dev, L, pq, tries):
    ei, N = branchy_graph()
    NG.check_pending()
    rw = npi.RandomWalker(_t(ei, dev), N, seed=0, p=pq[0], q=pq[1], tries=tries)
    got = rw.walks(_t(_starts(), dev), L)
    want, exhausted = _want(L, pq, tries)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1000, L + 1) and rw.draw == 1
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    bits = _status_bits(dev)
    assert bits & _lib.NPI_STATUS_BAD_SOURCE_ID and not bits & 1                   # the two bad starts; the build dropped nothing
    assert bool(bits & _lib.NPI_STATUS_WALK_TRIES) == (exhausted > 0), (bits, exhausted)
    if pq == (1, 1):
        assert exhausted == 0
    assert (want[[500, 999]] == -1).all() and (want[5] == 295).all() and (want[4] == 285).all() and (want[3] == 271).all()


def test_status_is_reported_through_check_pending(dev):
    ei, N = house_graph()
    NG.check_pending()
    rw = npi.RandomWalker(_t(ei, dev), N, p=0.5, q=2, tries=1)
    rw.walks(torch.ones(2000, dtype=torch.int64, device=dev), 8)
    with pytest.raises(ValueError, match="tries"):
        NG.check_pending()
    rw.walks(torch.tensor([1, 6], device=dev), 2)
    with pytest.raises(IndexError, match="source id"):
        NG.check_pending()
    NG.check_pending()                                                              # read once: nothing is left


def test_statistics_on_the_device(dev):
    """the three cases of tests/test_walk_cpu.py through the class: bitwise the same walks, so the same verdicts"""
    ei, N = star_graph()
    NG.check_pending()
    w = npi.RandomWalker(_t(ei, dev), N, seed=0).walks(torch.zeros(40_000, dtype=torch.int64, device=dev), 3)
    assert abs(check_uniform_pick(w.cpu().numpy()) - 108.435) < 1e-6
    ei, N = house_graph()
    w = npi.RandomWalker(_t(ei, dev), N, seed=0, p=0.5, q=2, tries=64).walks(torch.ones(40_000, dtype=torch.int64, device=dev), 2)
    assert check_pq_bias(w.cpu().numpy())[0] == 20_024
    assert _status_bits(dev) == 0                                                  # no step out of tries
    w = npi.RandomWalker(_t(ei, dev), N, seed=0, p=0.5, q=2, tries=1).walks(torch.ones(2000, dtype=torch.int64, device=dev), 8)
    want, exhausted = ref.walks(ref.epoch_seed(0, 0), ei, N, np.ones(2000, dtype=np.int64), 8, thr=ref.thresholds(0.5, 2), tries=1)
    assert exhausted > 0 and torch.equal(w.cpu(), torch.from_numpy(want))
    assert _status_bits(dev) == _lib.NPI_STATUS_WALK_TRIES


def test_draws_replay_and_differ(dev):
    ei, N = branchy_graph()
    rw = npi.RandomWalker(_t(ei, dev), N, seed=3, p=0.5, q=2)
    start = _t(_starts()[:400].clip(0, 299), dev)
    a = rw.walks(start, 20)                                                         # draw 0
    b = rw.walks(start, 20)                                                         # draw 1
    assert rw.draw == 2 and not torch.equal(a, b)
    assert torch.equal(rw.walks(start, 20, draw=0), a) and torch.equal(rw.walks(start, 20, draw=1), b) and rw.draw == 2
    rw.draw = 0
    assert torch.equal(rw.walks(start, 20), a)
    want = ref.walks(ref.epoch_seed(3, 1), ei, N, start.cpu().numpy(), 20, thr=ref.thresholds(0.5, 2))[0]
    assert torch.equal(b.cpu(), torch.from_numpy(want))
    # torch_cluster's name: one walker per call
    c = npi.random_walk(_t(ei[0], dev), _t(ei[1], dev), start, 20, p=0.5, q=2, num_nodes=N, seed=3)
    assert torch.equal(c, a)
    assert torch.equal(npi.random_walk(_t(ei[0], dev), _t(ei[1], dev), start, 20, p=0.5, q=2, seed=3), a)   # N from the largest id: the same rows
    NG.check_pending()


@pytest.mark.parametrize("pq", [(1, 1), (0.5, 2)])
def test_a_stream_belongs_to_a_slot_not_to_the_launch(dev, pq):
    """W = 1, W = 4,097 (17 workgroups) and W = 2048 * 256 + 300 (the grid strides) over the same starts: shared prefixes agree, and
    the long one equals the restatement"""
    ei, N = branchy_graph()
    rw = npi.RandomWalker(_t(ei, dev), N, seed=0, p=pq[0], q=pq[1])
    W = 2048 * 256 + 300
    start = np.random.default_rng(6).integers(0, 300, W)
    big = rw.walks(_t(start, dev), 3, draw=0)
    mid = rw.walks(_t(start[:4097], dev), 3, draw=0)
    one = rw.walks(_t(start[:1], dev), 3, draw=0)
    assert torch.equal(big[:4097], mid) and torch.equal(mid[:1], one)
    want = ref.walks(ref.epoch_seed(0, 0), ei, N, start, 3, thr=ref.thresholds(*pq))[0]
    assert torch.equal(big.cpu(), torch.from_numpy(want))
    NG.check_pending()


@pytest.mark.parametrize("W,L,c,S", [(257, 4, 5, 1), (257, 8, 3, 2), (257, 20, 10, 9), (257, 8, 4, 0), (20_000, 8, 3, 2)])
def test_walk_pairs_equal_the_restatement(dev, W, L, c, S):
    """the issue's three shapes at W = 257, no negatives at all, and M = 560,000 pairs (the grid strides)"""
    ei, N = branchy_graph()
    start = np.random.default_rng(8).integers(0, 300, W)
    start[3] = -1                                                                   # a bad walk: its -1 entries are copied
    walks = ref.walks(ref.epoch_seed(0, 0), ei, N, start, L)[0]
    key = ref.epoch_seed(0, 5)
    want, n_pos = ref.pairs(key, walks, c, S, N)
    got, got_pos = npi_walk.walk_pairs(_t(walks, dev), c, S, N, key)
    assert got_pos == n_pos and got.dtype == torch.int64 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert (want[:, :n_pos] == -1).any()
    with pytest.raises(ValueError, match="context_size"):
        npi_walk.walk_pairs(_t(walks, dev), L + 2, S, N, key)


def test_walks_under_capture(dev):
    """``walks`` inside ``torch.cuda.graph`` with a preallocated ``start``, replayed twice: the eager output, no host read"""
    ei, N = branchy_graph()
    rw = npi.RandomWalker(_t(ei, dev), N, seed=4, p=0.5, q=2)
    rng = np.random.default_rng(9)
    a, b = _t(rng.integers(0, 300, 3000), dev), _t(rng.integers(0, 300, 3000), dev)
    eager_a, eager_b = rw.walks(a, 12, draw=6), rw.walks(b, 12, draw=6)
    NG.check_pending()
    start = a.clone()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        out = rw.walks(start, 12, draw=6)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    start.copy_(b)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b)
    want = ref.walks(ref.epoch_seed(4, 6), ei, N, a.cpu().numpy(), 12, thr=ref.thresholds(0.5, 2))[0]
    assert torch.equal(eager_a.cpu(), torch.from_numpy(want))
