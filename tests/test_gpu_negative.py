"""``npi.NegativeSampler`` on the GPU: every result against the numpy restatement of the two rules (``tests/_negative_ref.py``, checked
by ``tests/test_negative_cpu.py``) element for element, the statistics of both rules through the class with the bounds and seeds of
the CPU cases, and structural properties at a size checked with torch ops alone."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
import _negative_ref as ref
from test_negative_cpu import even_targets_graph, mod4_graph

pytestmark = pytest.mark.gpu

_CACHE = {}


def _small():
    """n_src = 300, n_dst = 40; 3,000 columns: target 5 with 100 in-edges, 2,700 random ones over targets 0 .. 36 (37 - 39 stay
    without in-edges), 200 repeats of earlier columns, shuffled.  (The Rule T case adds a source joined to all 40 targets.)"""
    if "small" not in _CACHE:
        rng = np.random.default_rng(11)
        hub = np.stack([rng.permutation(300)[:100], np.full(100, 5)])
        rand = np.stack([rng.integers(0, 300, 2700), rng.integers(0, 37, 2700)])
        ei = np.concatenate([hub, rand], axis=1)
        ei = np.concatenate([ei, ei[:, rng.integers(0, 2800, 200)]], axis=1)[:, rng.permutation(3000)]
        assert ei.shape == (2, 3000) and np.bincount(ei[1], minlength=40)[37:].sum() == 0 and np.bincount(ei[1])[5] > 64
        _CACHE["small"] = ei
    return _CACHE["small"]


def _small_want(no_loops):
    key = ("small_want", no_loops)
    if key not in _CACHE:
        _CACHE[key] = ref.pairs(ref.epoch_seed(0, 0), _small(), 300, 40, 3000, no_loops=no_loops)
    return _CACHE[key]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("allow_loops", [True, False])
def test_small_graph_in_list_order_equals_the_restatement(dev, allow_loops):
    """membership on empty, short, long and repeated-column rows; the loop flag"""
    ei = _small()
    neg = npi.NegativeSampler(_t(ei, dev), size=(300, 40), seed=0, allow_loops=allow_loops)
    distinct = len(ref.edge_codes(ei, 40))
    loop_edges = len(np.intersect1d(ref.edge_codes(ei, 40), np.arange(40) * 41))
    assert neg.num_non_edges == 300 * 40 - distinct - (0 if allow_loops else 40 - loop_edges)
    got = neg.pairs()                                                   # M = E, draw 0
    want, consumed = _small_want(not allow_loops)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 3000)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert neg.last_consumed == consumed <= neg.last_window and neg.draw == 1
    if not allow_loops:
        assert bool((got[0] != got[1]).all())
    assert not torch.equal(neg.pairs(), got)                            # draw 1
    assert torch.equal(neg.pairs(draw=0), got) and neg.draw == 2        # a replay takes no draw number


def test_the_result_does_not_depend_on_the_window(dev):
    neg = npi.NegativeSampler(_t(_small(), dev), size=(300, 40))
    want, consumed = _small_want(False)
    for window in (64, None, 100_000):                                  # several doublings, the default, one long round
        got = neg.pairs(draw=0, window=window)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), window
        assert neg.last_consumed == consumed
    assert neg.last_window == 100_000
    with pytest.raises(npi.NpiError, match="window"):                   # a window that passes 2^31 - 1
        neg.pairs(draw=0, window=2 ** 31 - 1)
    short = neg.pairs(1000, draw=0)
    assert torch.equal(short.cpu(), torch.from_numpy(want[:, :1000]))  # nested in M


def test_exhausting_the_complement(dev):
    """n_src = 37, n_dst = 23, 600 distinct cells of 851 (the first 50 twice): all 251 non-edges, from a window of 256 -- several
    doublings, heavy repeats among the valid candidates"""
    cells = np.random.default_rng(5).permutation(851)[:600]
    cells = np.concatenate([cells, cells[:50]])
    ei = np.stack([cells // 23, cells % 23])
    neg = npi.NegativeSampler(_t(ei, dev), size=(37, 23))
    assert neg.num_non_edges == 251
    got = neg.pairs(10_000, draw=0, window=256)                         # clamped to every non-edge
    want, consumed = ref.pairs(ref.epoch_seed(0, 0), ei, 37, 23, 251)
    print("candidates consumed:", consumed, "window:", neg.last_window)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert neg.last_consumed == consumed and neg.last_window >= consumed > 256
    codes = np.sort((got[0] * 23 + got[1]).cpu().numpy())
    assert np.array_equal(codes, np.setdiff1d(np.arange(851), cells))  # as a set: exactly the complement


@pytest.mark.parametrize("M,window", [(280_000, 300_000), (100_000, 120_000)])
def test_two_sort_keys_and_both_sort_paths(dev, M, window):
    """n_src = n_dst = 70,000: ids of 17 bits each, pair codes past 2^32; a window above and one below the 262,144 entries at
    which the radix sort changes from the launch-bound path to the scanned one"""
    if "big" not in _CACHE:
        _CACHE["big"] = np.random.default_rng(5).integers(0, 70_000, (2, 200_000))
    ei = _CACHE["big"]
    neg = npi.NegativeSampler(_t(ei, dev), size=70_000)
    got = neg.pairs(M, draw=0, window=window)
    want, consumed = ref.pairs(ref.epoch_seed(0, 0), ei, 70_000, 70_000, M, chunk=1 << 17)
    print("candidates consumed:", consumed)
    assert neg.last_window == window and neg.last_consumed == consumed
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_no_edges_and_the_clamp(dev):
    neg = npi.NegativeSampler(torch.empty((2, 0), dtype=torch.int64, device=dev), size=(5, 3))
    assert neg.num_non_edges == 15
    assert tuple(neg.pairs().shape) == (2, 0)                           # M = E = 0
    got = neg.pairs(100, draw=0)
    want, _ = ref.pairs(ref.epoch_seed(0, 0), np.zeros((2, 0), dtype=np.int64), 5, 3, 15)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert sorted((got[0] * 3 + got[1]).tolist()) == list(range(15))   # every candidate valid; all 15 cells


def test_rule_t_equals_the_restatement_and_reports_both_bits(dev):
    ei = _small()
    full = np.stack([np.full(40, 7), np.arange(40)])                    # source 7 joined to all 40 targets
    ei = np.concatenate([ei, full], axis=1)
    neg = npi.NegativeSampler(_t(ei, dev), size=(300, 40), seed=2)
    key = ref.epoch_seed(2, 0)
    src = ei[0][ei[0] != 7]
    got = neg.corrupt(_t(src, dev))
    NG.check_pending()                                                  # nothing to report
    assert torch.equal(got.cpu(), torch.from_numpy(ref.corrupt(key, ei, 300, 40, src))) and int(got.min()) >= 0
    src = np.random.default_rng(3).integers(0, 300, 100_000)
    src[src == 7] = 8
    want = ref.corrupt(key, ei, 300, 40, src)
    assert torch.equal(neg.corrupt(_t(src, dev), draw=0).cpu(), torch.from_numpy(want))
    NG.check_pending()
    # the full source: -1 in exactly its slots, the others unaffected
    src_full = src.copy()
    src_full[[5, 70_000]] = 7
    got = neg.corrupt(_t(src_full, dev), draw=0).cpu().numpy()
    with pytest.raises(ValueError, match="non-edge"):
        NG.check_pending()
    assert got[5] == got[70_000] == -1 and np.array_equal(np.delete(got, [5, 70_000]), np.delete(want, [5, 70_000]))
    # ids out of range: never dereferenced, -1 in exactly their slots
    src_bad = src.copy()
    src_bad[[0, 99_999]] = [-1, 300]
    got = neg.corrupt(_t(src_bad, dev), draw=0).cpu().numpy()
    with pytest.raises(IndexError, match="source id"):
        NG.check_pending()
    assert got[0] == got[99_999] == -1 and np.array_equal(got[1:-1], want[1:-1])
    assert np.array_equal(got, ref.corrupt(key, ei, 300, 40, src_bad))
    # tries: one draw per slot leaves -1 where it hit an edge
    got = neg.corrupt(_t(src, dev), draw=0, tries=1).cpu().numpy()
    want1 = ref.corrupt(key, ei, 300, 40, src, tries=1)
    assert np.array_equal(got, want1) and (want1 == -1).any()
    with pytest.raises(ValueError, match="non-edge"):
        NG.check_pending()
    NG.check_pending()                                                  # read once: nothing is left


def test_rule_t_under_capture(dev):
    """``corrupt`` inside ``torch.cuda.graph`` with a preallocated ``src``, replayed twice: the eager output, no host read"""
    ei = _small()
    neg = npi.NegativeSampler(_t(ei, dev), size=(300, 40), seed=4)
    rng = np.random.default_rng(9)
    a, b = _t(rng.integers(0, 300, 5000), dev), _t(rng.integers(0, 300, 5000), dev)
    eager_a, eager_b = neg.corrupt(a, draw=6), neg.corrupt(b, draw=6)
    NG.check_pending()
    src = a.clone()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        out = neg.corrupt(src, draw=6)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    src.copy_(b)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b)
    assert torch.equal(eager_a.cpu(), torch.from_numpy(ref.corrupt(ref.epoch_seed(4, 6), ei, 300, 40, a.cpu().numpy())))
    with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=stream):
        with pytest.raises(npi.NpiError, match="capture"):
            neg.pairs(10, draw=0)
    torch.cuda.synchronize()


def test_rule_p_statistics_on_the_device(dev):
    """the uniformity case of tests/test_negative_cpu.py through the class: 4,096 ``pairs`` calls of 192 with ``window=512``; the
    same 6 sigma bound with the same seeds -- it holds for the restatement, so it holds for an exact implementation"""
    ei, mask = mod4_graph()
    neg = npi.NegativeSampler(_t(ei, dev), size=(32, 32), seed=0)
    assert neg.num_non_edges == 768
    counts = torch.zeros(32 * 32, dtype=torch.int64, device=dev)
    for draw in range(4096):
        p = neg.pairs(192, window=512)                                  # the sampler's own counter: draw = 0 .. 4095
        counts += torch.bincount(p[0] * 32 + p[1], minlength=1024)
    assert neg.draw == 4096
    counts = counts.view(32, 32).cpu().numpy()
    dev_ = np.abs(counts[~mask] - 1024)
    print("max deviation:", dev_.max())
    assert counts.max() <= 4096 and counts.sum() == 4096 * 192          # (192 distinct pairs per draw: no cell twice in a draw)
    assert counts[mask].sum() == 0 and (dev_ <= 166).all(), counts


def test_rule_t_statistics_on_the_device(dev):
    neg = npi.NegativeSampler(_t(even_targets_graph(), dev), size=(1, 64), seed=0)
    out = neg.corrupt(torch.zeros(4096, dtype=torch.int64, device=dev))
    NG.check_pending()
    cnt = torch.bincount(out, minlength=64).cpu().numpy()
    print("max deviation:", np.abs(cnt[1::2] - 128).max())
    assert cnt[0::2].sum() == 0 and (np.abs(cnt[1::2] - 128) <= 67).all(), cnt


def test_properties_at_a_larger_size(dev):
    """n_src = 200,000, n_dst = 2,000, 2M columns with Zipf-weighted targets, M = E: no output is an edge, all outputs distinct,
    ids in range, info[1] within the window, a replay bitwise equal, another draw different"""
    rng = np.random.default_rng(17)
    w = 1.0 / np.arange(1, 2001)
    ei = np.stack([rng.integers(0, 200_000, 2_000_000), rng.choice(2000, 2_000_000, p=w / w.sum())])
    t = _t(ei, dev)
    neg = npi.NegativeSampler(t, size=(200_000, 2000), seed=1)
    edge_codes = torch.unique(t[0] * 2000 + t[1])
    assert neg.num_non_edges == 200_000 * 2000 - int(edge_codes.numel())
    got = neg.pairs()
    assert tuple(got.shape) == (2, 2_000_000) and 0 < neg.last_consumed <= neg.last_window
    assert int(got[0].min()) >= 0 and int(got[0].max()) < 200_000 and int(got[1].min()) >= 0 and int(got[1].max()) < 2000
    codes = got[0] * 2000 + got[1]
    assert not bool(torch.isin(codes, edge_codes).any())
    assert int(torch.unique(codes).numel()) == 2_000_000
    assert torch.equal(neg.pairs(draw=0), got)
    assert not torch.equal(neg.pairs(draw=1), got)
    # the head of the result against the restatement (the candidates of a prefix do not depend on M)
    want, _ = ref.pairs(ref.epoch_seed(1, 0), ei, 200_000, 2000, 2000)
    assert torch.equal(got[:, :2000].cpu(), torch.from_numpy(want))


def test_the_wrappers_equal_the_class(dev):
    ei = _t(_small(), dev)
    neg = npi.NegativeSampler(ei, size=(300, 40), seed=5)
    assert torch.equal(npi.negative_sampling(ei, (300, 40), seed=5), neg.pairs(draw=0))
    assert torch.equal(npi.negative_sampling(ei, (300, 40), num_neg_samples=77, seed=5), neg.pairs(77, draw=0))
    i, j, k = npi.structured_negative_sampling(ei, (300, 40), seed=5)
    assert torch.equal(i, ei[0]) and torch.equal(j, ei[1]) and torch.equal(k, neg.corrupt(ei[0], draw=0))
    NG.check_pending()
    assert not bool(torch.isin(i * 40 + k, ei[0] * 40 + ei[1]).any())
    with pytest.raises(IndexError):                                     # an id out of range is refused when the sampler is built
        npi.NegativeSampler(torch.tensor([[0, 300], [1, 2]], device=dev), size=(300, 40))
