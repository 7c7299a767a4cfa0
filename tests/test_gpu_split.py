"""Edge splits on the device against the numpy restatement of Rule S (``tests/_split_ref.py``): the order, the undirected form,
the parts, the held-out negatives, the folds, the statistics of the order and one toy link-prediction run from a split."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
import _split_ref as ref
from test_split_cpu import columns24, uniformity

pytestmark = pytest.mark.gpu

_CACHE = {}


def _one_space(bad=True):
    """N = 200; 5,000 columns: 2,200 random ones (40 of them made loops) in both orientations, 300 repeats of earlier columns, 300
    more random ones, shuffled.  ``bad``: three of the last 300 hold an id out of range (-1, 200 and 250); otherwise they are in
    range -- the same list apart from those three columns."""
    if "one" not in _CACHE:
        rng = np.random.default_rng(5)
        base = rng.integers(0, 200, (2, 2200))
        base[1, :40] = base[0, :40]
        ei = np.concatenate([base, base[::-1]], axis=1)
        ei = np.concatenate([ei, ei[:, rng.integers(0, 4400, 300)], rng.integers(0, 200, (2, 300))], axis=1)
        perm = rng.permutation(5000)
        clean, dirty = ei.copy(), ei.copy()
        dirty[0, 4997], dirty[1, 4998], dirty[0, 4999] = -1, 200, 250
        _CACHE["one"] = (np.ascontiguousarray(clean[:, perm]), np.ascontiguousarray(dirty[:, perm]))
        assert dirty.shape == (2, 5000) and (ei[0] == ei[1]).sum() >= 80
    return _CACHE["one"][1 if bad else 0]


def _two_spaces():
    """n_src = 300, n_dst = 40; 3,000 columns, 200 of them repeats of earlier ones"""
    if "two" not in _CACHE:
        rng = np.random.default_rng(11)
        ei = np.stack([rng.integers(0, 300, 2800), rng.integers(0, 40, 2800)])
        _CACHE["two"] = np.concatenate([ei, ei[:, rng.integers(0, 2800, 200)]], axis=1)[:, rng.permutation(3000)]
    return _CACHE["two"]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _reported():
    """the pending status words hold an out-of-range id: raised, and gone afterwards"""
    with pytest.raises(IndexError, match="outside its range"):
        NG.check_pending()
    NG.check_pending()


def _same(got, want):
    return got.dtype == torch.int64 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)


# ---- 5. the order ------------------------------------------------------------------------------------------------------------------------
def test_permutation_one_id_space_equals_the_restatement_and_reports_bad_ids(dev):
    ei = _one_space()
    NG.check_pending()
    sp = npi.EdgeSplitter(_t(ei, dev), 200, seed=0)
    edges, e_id = sp.permutation()
    want, want_id = ref.permutation(ref.epoch_seed(0, 0), ei, 200, 200, True)
    assert 2000 < want.shape[1] < 2500 and _same(edges, want) and _same(e_id, want_id)
    assert bool((edges[0] < edges[1]).all())
    _reported()
    again, again_id = sp.permutation(draw=0)                              # a replay: bitwise equal, and takes no draw number
    assert torch.equal(again, edges) and torch.equal(again_id, e_id) and sp.draw == 1
    other, other_id = sp.permutation()                                     # draw 1
    assert sp.draw == 2 and not torch.equal(other_id, e_id) and torch.equal(other_id.sort().values, e_id.sort().values)
    assert _same(other_id, ref.permutation(ref.epoch_seed(0, 1), ei, 200, 200, True)[1])
    _reported()
    # the clean list without its three differing columns comes out in the same order: r_e depends on e alone
    clean = _one_space(bad=False)
    ce, cid = npi.EdgeSplitter(_t(clean, dev), 200, seed=0).permutation()
    want_c = ref.permutation(ref.epoch_seed(0, 0), clean, 200, 200, True)
    assert _same(ce, want_c[0]) and _same(cid, want_c[1])
    bad_cols = np.nonzero((ei != clean).any(axis=0))[0]
    assert len(bad_cols) == 3 and np.array_equal(cid.cpu().numpy()[~np.isin(want_c[1], bad_cols)], want_id)
    NG.check_pending()                                                     # nothing to report


def test_permutation_two_id_spaces_equals_the_restatement(dev):
    ei = _two_spaces()
    sp = npi.EdgeSplitter(_t(ei, dev), (300, 40), seed=3)
    edges, e_id = sp.permutation()
    want, want_id = ref.permutation(ref.epoch_seed(3, 0), ei, 300, 40, False)
    assert want.shape == (2, 3000) and _same(edges, want) and _same(e_id, want_id)       # every column is kept, repeats included
    assert torch.equal(_t(ei, dev)[:, e_id], edges)
    NG.check_pending()


@pytest.mark.parametrize("E", [0, 1, 4096, 4097, 70_000])
def test_permutation_at_the_sorter_s_sizes(dev, E):
    """the empty input, one entry, exactly one sort tile, one over, and past the 64 tiles (65,536 pairs) up to which the sorter
    derives its offsets inside the scatter; one id space, so about half of the columns are dropped and padded"""
    rng = np.random.default_rng(E)
    ei = rng.integers(0, 1000, (2, E))
    if E == 1:
        ei[:] = [[2], [7]]
    edges, e_id = npi.EdgeSplitter(_t(ei, dev), 1000, seed=1).permutation()
    want, want_id = ref.permutation(ref.epoch_seed(1, 0), ei, 1000, 1000, True)
    assert _same(edges, want) and _same(e_id, want_id)
    full, full_id = npi.EdgeSplitter(_t(ei, dev), (1000, 1000), seed=1).permutation()      # nothing dropped: no padding
    want, want_id = ref.permutation(ref.epoch_seed(1, 0), ei, 1000, 1000, False)
    assert full.shape[1] == E and _same(full, want) and _same(full_id, want_id)
    NG.check_pending()


# ---- 6. the undirected form --------------------------------------------------------------------------------------------------------------
def test_to_undirected_equals_unique_over_both_orientations(dev):
    ei = _one_space()
    und = npi.to_undirected(_t(ei, dev), 200)
    want = ref.to_undirected(ei, 200)
    assert _same(und, want)
    _reported()
    code = want[0] * 200 + want[1]
    assert (np.diff(code) > 0).all() and np.array_equal(np.unique(np.concatenate([code, want[1] * 200 + want[0]])), code)
    assert (want[0] == want[1]).any()                                      # loops stay, once
    assert torch.equal(npi.to_undirected(und, 200), und)                   # already undirected: itself
    upper = und[:, und[0] <= und[1]]
    assert torch.equal(npi.to_undirected(upper, 200), und)                 # one orientation is enough
    assert tuple(npi.to_undirected(und[:, :0], 200).shape) == (2, 0)
    NG.check_pending()


# ---- 7. train / val / test ---------------------------------------------------------------------------------------------------------------
def test_split_parts_partition_the_kept_columns_and_the_negatives_equal_the_restatement(dev):
    ei = _one_space(bad=False)
    eid = _t(ei, dev)
    sp = npi.EdgeSplitter(eid, 200, seed=0)
    s = sp.split(val_ratio=0.05, test_ratio=0.1)
    key = ref.epoch_seed(0, 0)
    want, want_id = ref.permutation(key, ei, 200, 200, True)
    K = want.shape[1]
    n_v, n_t = ref.part_sizes(K, 0.05, 0.1)
    assert n_v == int(0.05 * K) > 100 and n_t == int(0.1 * K)
    assert _same(s.val_e_id, want_id[:n_v]) and _same(s.test_e_id, want_id[n_v:n_v + n_t]) and _same(s.train_e_id, want_id[n_v + n_t:])
    ids = torch.cat([s.val_e_id, s.test_e_id, s.train_e_id]).cpu().numpy()
    assert len(np.unique(ids)) == K and np.array_equal(np.sort(ids), np.nonzero(ei[0] < ei[1])[0])     # disjoint; exactly the kept
    assert _same(s.val_pos_edge_index, want[:, :n_v]) and _same(s.test_pos_edge_index, want[:, n_v:n_v + n_t])
    assert torch.equal(s.train_pos_edge_index, npi.to_undirected(eid[:, s.train_e_id], 200))
    assert _same(s.train_pos_edge_index, ref.to_undirected(want[:, n_v + n_t:], 200))
    # the held-out negatives: one draw, val first
    neg = torch.cat([s.val_neg_edge_index, s.test_neg_edge_index], dim=1)
    assert s.val_neg_edge_index.shape[1] == n_v and s.test_neg_edge_index.shape[1] == n_t
    assert _same(neg, ref.upper_negatives(key, ei, 200, n_v + n_t))
    a, b = neg.cpu().numpy()
    edge = np.zeros((200, 200), dtype=bool)
    edge[ei[0], ei[1]] = True
    assert (a < b).all() and len(np.unique(a * 200 + b)) == n_v + n_t and not edge[a, b].any() and not edge[b, a].any()
    # the window plays no part; a replay takes no draw number
    for window in (64, 100_000):
        r = sp.split(val_ratio=0.05, test_ratio=0.1, draw=0, window=window)
        for name in ("train_pos_edge_index", "val_pos_edge_index", "test_pos_edge_index", "val_neg_edge_index", "test_neg_edge_index",
                     "train_e_id", "val_e_id", "test_e_id"):
            assert torch.equal(getattr(r, name), getattr(s, name)), (window, name)
    assert sp.draw == 1
    none = sp.split(0.0, 0.0, negatives=False)
    assert none.val_neg_edge_index is None and none.val_e_id.numel() == 0 and none.train_e_id.numel() == K
    NG.check_pending()


def test_split_of_a_list_with_bad_ids(dev):
    """without negatives the bad columns are dropped and reported; the sampler the negatives need refuses such a list"""
    ei = _one_space()
    NG.check_pending()
    sp = npi.EdgeSplitter(_t(ei, dev), 200, seed=0)
    s = sp.split(val_ratio=0.05, test_ratio=0.1, negatives=False)
    in_range = ((ei >= 0) & (ei < 200)).all(axis=0)
    ids = torch.cat([s.val_e_id, s.test_e_id, s.train_e_id]).cpu().numpy()
    assert np.array_equal(np.sort(ids), np.nonzero(in_range & (ei[0] < ei[1]))[0])
    _reported()
    with pytest.raises(IndexError):
        sp.split(val_ratio=0.05, test_ratio=0.1)
    NG.check_pending()
    with pytest.raises(ValueError, match="folds"):
        npi.EdgeSplitter(_t(ei[:, :4], dev), (300, 300)).kfold(k=5)


def test_upper_negatives_exhaust_the_complement(dev):
    """the graph of the CPU case: N = 32, edge iff (a + b) % 4 == 0.  M above the bound is clamped to exactly the upper non-edges"""
    from test_split_cpu import mod4_undirected
    ei, mask = mod4_undirected()
    sp = npi.EdgeSplitter(_t(ei, dev), 32, seed=0)
    K = int((ei[0] < ei[1]).sum())
    s = sp.split(val_ratio=0.5, test_ratio=0.5)                            # every kept column is held out
    assert s.train_pos_edge_index.shape[1] == K - 2 * (K // 2) and s.val_e_id.numel() == s.test_e_id.numel() == K // 2
    neg = torch.cat([s.val_neg_edge_index, s.test_neg_edge_index], dim=1)
    assert _same(neg, ref.upper_negatives(ref.epoch_seed(0, 0), ei, 32, 2 * (K // 2)))
    every = sp._negatives(0, 10_000, None)
    assert _same(every, ref.upper_negatives(ref.epoch_seed(0, 0), ei, 32, 10_000)) and every.shape[1] == 376
    assert torch.equal(every[:, :neg.shape[1]], neg)                       # nested in M


def test_splitting_inside_a_capture_raises(dev):
    ei = _t(_two_spaces(), dev)
    sp = npi.EdgeSplitter(ei, (300, 40), seed=0)
    sp.permutation()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream):
        for call in (sp.permutation, sp.split, sp.kfold, lambda: npi.to_undirected(ei[:, :10], 300)):
            with pytest.raises(npi.NpiError, match="capture"):
                call()
    torch.cuda.synchronize()
    assert sp.draw == 1                                                    # a refused call takes no draw number


# ---- 8. folds ----------------------------------------------------------------------------------------------------------------------------
def test_kfold_partitions_the_positives_and_one_draw_of_negatives(dev):
    ei = _two_spaces()
    eid = _t(ei, dev)
    sp = npi.EdgeSplitter(eid, (300, 40), seed=0)
    folds = list(sp.kfold(k=5))
    assert len(folds) == 5 and sp.draw == 1
    want, want_id = ref.permutation(ref.epoch_seed(0, 0), ei, 300, 40, False)
    bounds = ref.fold_bounds(3000, 5)
    pairs = npi.NegativeSampler(eid, (300, 40), seed=0).pairs(3000, draw=0)
    assert pairs.shape[1] == 3000
    tests, neg_tests = [], []
    for f, fold in enumerate(folds):
        lo, hi = bounds[f], bounds[f + 1]
        assert _same(fold.test_e_id, want_id[lo:hi]) and _same(fold.test_pos_edge_index, want[:, lo:hi])
        assert _same(fold.train_e_id, np.concatenate([want_id[:lo], want_id[hi:]]))
        assert torch.equal(fold.train_pos_edge_index, eid[:, fold.train_e_id])
        assert len(np.intersect1d(fold.train_e_id.cpu().numpy(), fold.test_e_id.cpu().numpy())) == 0
        assert fold.train_e_id.numel() + fold.test_e_id.numel() == 3000
        assert torch.equal(fold.test_neg_edge_index, pairs[:, lo:hi])
        assert torch.equal(fold.train_neg_edge_index, torch.cat([pairs[:, :lo], pairs[:, hi:]], dim=1))
        tr, te = (x.cpu().numpy() for x in (fold.train_neg_edge_index, fold.test_neg_edge_index))
        assert len(np.intersect1d(tr[0] * 40 + tr[1], te[0] * 40 + te[1])) == 0
        tests.append(fold.test_e_id)
        neg_tests.append(fold.test_neg_edge_index)
    sizes = [t.numel() for t in tests]
    assert max(sizes) - min(sizes) <= 1
    assert np.array_equal(np.sort(torch.cat(tests).cpu().numpy()), np.arange(3000))       # every kept column in exactly one test fold
    assert torch.equal(torch.cat(neg_tests, dim=1), pairs)
    # uneven folds, one id space (the negatives in their canonical form), no negatives
    up = npi.EdgeSplitter(_t(_one_space(bad=False), dev), 200, seed=0)
    seven = list(up.kfold(k=7, draw=0))
    K = sum(f.test_e_id.numel() for f in seven)
    assert [f.test_e_id.numel() for f in seven] == list(np.diff(ref.fold_bounds(K, 7)))
    neg = torch.cat([f.test_neg_edge_index for f in seven], dim=1)
    assert _same(neg, ref.upper_negatives(ref.epoch_seed(0, 0), _one_space(bad=False), 200, K))
    assert all(f.train_neg_edge_index is None for f in up.kfold(k=2, draw=0, negatives=False))
    NG.check_pending()


# ---- 9. the statistics of the order ------------------------------------------------------------------------------------------------------
def test_rule_s_statistics_on_the_device(dev):
    """tests/test_split_cpu.py::test_rule_s_is_a_uniform_permutation through the class: the same 24 columns, bounds and seeds, so
    the same figures (46.3 and 54)"""
    ei, size = columns24()
    sp = npi.EdgeSplitter(_t(ei, dev), size, seed=0)
    perms = torch.stack([sp.permutation()[1] for _ in range(4096)]).cpu().numpy()
    assert sp.draw == 4096 and (np.sort(perms, axis=1) == np.arange(24)).all()
    cell, head = uniformity(perms)
    print("largest deviation of a (column, position) cell:", cell, "of a column's count in the test part:", head)
    assert cell <= 77 and head <= 166
    NG.check_pending()


# ---- 10. end to end ----------------------------------------------------------------------------------------------------------------------
def test_split_then_loss_then_metrics_at_toy_size(dev):
    """N = 64, a ring plus 100 chords in both orientations; the encoder is the learnable N x 16 table"""
    rng = np.random.default_rng(2)
    ring = np.stack([np.arange(64), (np.arange(64) + 1) % 64])
    chords = rng.integers(0, 64, (2, 100))
    half = np.concatenate([ring, chords], axis=1)
    ei = _t(np.concatenate([half, half[::-1]], axis=1), dev)

    def run():
        torch.manual_seed(0)
        table = torch.nn.Embedding(64, 16).to(dev)
        s = npi.train_test_split_edges(ei, 64, val_ratio=0.05, test_ratio=0.1, seed=0)
        model = npi.GAE(encoder=None)
        z = table.weight
        loss = model.recon_loss(z, s.train_pos_edge_index)
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(table.weight.grad).all()) and bool(table.weight.grad.abs().sum() > 0)
        assert s.test_neg_edge_index.shape[1] == s.test_pos_edge_index.shape[1] > 0
        auc, ap = model.test(z.detach(), s.test_pos_edge_index, s.test_neg_edge_index)
        return float(auc), float(ap), float(loss.detach())

    first, second = run(), run()
    assert first == second                                                 # bitwise
    assert all(np.isfinite(v) for v in first) and 0.0 <= first[0] <= 1.0 and 0.0 <= first[1] <= 1.0
    NG.check_pending()
