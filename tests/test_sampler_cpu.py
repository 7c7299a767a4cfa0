"""The neighbour sampler without a GPU: the sampling rule itself (on the numpy restatement ``tests/_sampler_ref.py``), the new
C-ABI symbols, the argument errors of the entry points and of ``NeighborSampler``, and the host-side batching."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import _lib
from npi_gnn_amd import sampler as S
import _sampler_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: key seeds of the statistical cases, shared with tests/test_gpu_sampler.py
STAT_SEED = ref.epoch_seed(0, 0)
HUB_STAT_SEED = ref.epoch_seed(7, 0)

NEW = ("npi_sample_counts", "npi_sample_select", "npi_sample_workspace_elems", "npi_sample_relabel_count", "npi_sample_relabel")


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_inclusion_counts_of_the_rule_are_binomial():
    """4096 targets with a 64-entry row each, k = 16: every position's inclusion count is Binomial(4096, 1/4), mean 1024,
    sigma 27.7; all 64 within 6 sigma (false-alarm rate ~ 64 * 2e-9 = 1e-7)"""
    counts, sizes = ref.inclusion_counts(STAT_SEED, 0, 4096, 64, 16)
    print("min / max inclusion count:", counts.min(), counts.max())
    assert (sizes == 16).all()                                                     # 16 distinct positions per target
    assert counts.sum() == 4096 * 16
    assert (np.abs(counts - 1024) <= 166).all(), counts


def test_inclusion_counts_of_the_hub_case_are_binomial():
    """256 targets with a 4,096-entry row each, k = 1024: Binomial(256, 1/4), mean 64, sigma 6.9; all 4,096 positions within
    7 sigma = 49 (false-alarm rate ~ 4096 * 2.6e-12 = 1e-8) -- the bound the device test applies with this seed"""
    counts, sizes = ref.inclusion_counts(HUB_STAT_SEED, 0, 256, 4096, 1024)
    print("min / max inclusion count:", counts.min(), counts.max())
    assert (sizes == 1024).all()
    assert (np.abs(counts - 64) <= 49).all()


def test_rule_basics():
    assert np.array_equal(ref.sample_row(1, 0, 5, 7, 7), np.arange(7))              # d <= k: every entry
    assert np.array_equal(ref.sample_row(1, 0, 5, 7, 9), np.arange(7))
    assert len(ref.sample_row(1, 0, 5, 0, 3)) == 0
    a = ref.sample_row(1, 0, 5, 1025, 25)
    assert len(a) == 25 and (np.diff(a) > 0).all()                                  # ascending, distinct
    assert np.array_equal(a, ref.sample_row(1, 0, 5, 1025, 25))                     # a pure function
    assert not np.array_equal(a, ref.sample_row(2, 0, 5, 1025, 25))                 # of the seed,
    assert not np.array_equal(a, ref.sample_row(1, 1, 5, 1025, 25))                 # the hop
    assert not np.array_equal(a, ref.sample_row(1, 0, 6, 1025, 25))                 # and the node
    assert set(ref.sample_row(1, 0, 5, 1025, 10)) <= set(a)                         # the k smallest keys: nested in k
    assert ref.budget(10, 0.5) == 5 and ref.budget(11, 0.5) == 6 and ref.budget(1, 0.01) == 1 and ref.budget(0, 0.5) == 0
    assert ref.budget(10, 25) == 10 and ref.budget(100, 25) == 25 and ref.budget(7, 1.0) == 7


def test_epoch_seed_restatement_matches_the_package():
    for seed, epoch in ((0, 0), (0, 1), (7, 0), (-3, 5), (2 ** 62, 1000)):
        assert ref.epoch_seed(seed, epoch) == S.epoch_seed(seed, epoch)
        assert -2 ** 63 <= S.epoch_seed(seed, epoch) < 2 ** 63
    assert S.epoch_seed(0, 0) != S.epoch_seed(0, 1) != S.epoch_seed(1, 0)


def test_block_construction_by_hand():
    """edges (source -> target): 3->0, 4->0, 3->0 (a duplicate), 2->1, 1->1 (a loop column), nothing into 2"""
    ei = np.array([[3, 4, 3, 2, 1], [0, 0, 0, 1, 1]])
    csr = ref.by_target_csr(ei, 5)
    assert csr[0].tolist() == [0, 3, 5, 5, 5, 5] and csr[1].tolist() == [3, 4, 3, 2, 1] and csr[2].tolist() == [0, 1, 2, 3, 4]
    n_id, res, e_id, lei = ref.sample_hop(csr, [1, 2, 0], 10, 0, 3, add_self_loops=True)
    assert n_id.tolist() == [0, 1, 2, 3, 4] and res.tolist() == [1, 2, 0]
    assert e_id.tolist() == [3, 4, 0, 1, 2] and lei.tolist() == [[2, 1, 3, 4, 3], [0, 0, 2, 2, 2]]
    n_id, res, e_id, lei = ref.sample_hop(csr, [1, 2, 0], 10, 0, 3, add_self_loops=False)
    assert n_id.tolist() == [1, 2, 3, 4] and res is None and lei.tolist() == [[1, 0, 2, 3, 2], [0, 0, 2, 2, 2]]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "npi_gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert "torch_cluster.neighbor_sampler" in header and "0xBF58476D1CE4E5B9" in header     # the call replaced, the hash written out
    assert _lib.load().npi_abi_version() == 4
    import test_boundary_cpu as B
    B.test_every_declared_symbol_is_exported_and_bound()
    B.test_ctypes_prototypes_have_the_headers_argument_lists()
    B.test_the_library_allocates_nothing_and_keeps_no_state()
    B.test_product_package_never_imports_the_oracle()
    B.test_no_module_level_switch_on_the_layer_path()


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    lib = _lib.load()
    N = None
    calls = {
        "npi_sample_counts (negative count)": lambda: lib.npi_sample_counts(N, 4, N, -1, 5, 0.0, N, N, N),
        "npi_sample_counts (fraction 0, budget 0)": lambda: lib.npi_sample_counts(8, 4, 8, 4, 0, 0.0, 8, N, N),
        "npi_sample_counts (fraction 1.5)": lambda: lib.npi_sample_counts(8, 4, 8, 4, 0, 1.5, 8, N, N),
        "npi_sample_counts (negative budget)": lambda: lib.npi_sample_counts(8, 4, 8, 4, -2, 0.0, 8, N, N),
        "npi_sample_counts (budget and fraction)": lambda: lib.npi_sample_counts(8, 4, 8, 4, 3, 0.5, 8, N, N),
        "npi_sample_counts (null)": lambda: lib.npi_sample_counts(N, 4, N, 4, 5, 0.0, N, N, N),
        "npi_sample_select (negative count)": lambda: lib.npi_sample_select(8, 8, 8, 4, 8, -1, 8, 0, 0, 8, 8, 8, 4, N, N),
        "npi_sample_select (negative capacity)": lambda: lib.npi_sample_select(8, 8, 8, 4, 8, 4, 8, 0, 0, 8, 8, 8, -4, N, N),
        "npi_sample_select (null)": lambda: lib.npi_sample_select(N, N, N, 4, N, 4, N, 0, 0, N, N, N, 4, N, N),
        "npi_sample_relabel_count (negative count)": lambda: lib.npi_sample_relabel_count(8, 8, -1, 4, 8, 1, 16, 4, 8, 8, N),
        "npi_sample_relabel_count (null)": lambda: lib.npi_sample_relabel_count(N, N, 4, 4, N, 1, N, 4, N, N, N),
        "npi_sample_relabel_count (alignment)": lambda: lib.npi_sample_relabel_count(8, 8, 4, 4, 8, 1, 20, 4, 8, 8, N),
        "npi_sample_relabel (negative count)": lambda: lib.npi_sample_relabel(16, 4, 8, 8, 8, 8, -1, 8, 4, 2, 8, 8, 8, 8, 8, N, N),
        "npi_sample_relabel (more ids than nodes)": lambda: lib.npi_sample_relabel(16, 4, 8, 8, 8, 8, 4, 8, 4, 5, 8, 8, 8, 8, 8, N, N),
        "npi_sample_relabel (null)": lambda: lib.npi_sample_relabel(N, 4, N, N, N, N, 4, N, 4, 2, N, N, N, N, N, N, N),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.split()[0].encode() in lib.npi_last_error(), (name, lib.npi_last_error())
    assert lib.npi_sample_workspace_elems(-1) == -1 and lib.npi_sample_workspace_elems(0) == 1
    assert lib.npi_sample_workspace_elems(1_000_000) >= 1_000_000 // 1024 + 1
    # nothing to do: no launch, no error
    assert lib.npi_sample_select(N, N, N, 4, N, 0, N, 0, 0, N, N, N, 0, N, N) == 0


# ---- NeighborSampler: argument errors, no CPU path -------------------------------------------------------------------------------------
def test_sampler_argument_errors_and_no_cpu_fallback():
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    with pytest.raises(ValueError, match="bipartite"):
        npi.NeighborSampler(ei, 4, size=2, bipartite=False)
    with pytest.raises(ValueError, match="flow"):
        npi.NeighborSampler(ei, 4, size=2, flow="target_to_source")
    with pytest.raises(ValueError, match="num_hops"):
        npi.NeighborSampler(ei, 4, size=[5, 3, 2], num_hops=2)
    with pytest.raises(ValueError):
        npi.NeighborSampler(ei, 4, size=[5], num_hops=2)
    for bad in (0, -1, 0.0, 1.5, "3"):
        with pytest.raises(ValueError):
            npi.NeighborSampler(ei, 4, size=bad)
    with pytest.raises(ValueError):
        npi.NeighborSampler(ei.float(), 4, size=2)
    with pytest.raises(npi.NpiError):
        npi.NeighborSampler(ei, 4, size=[5, 3], num_hops=2, batch_size=2, add_self_loops=True)
    with pytest.raises(npi.NpiError):
        npi.NeighborSampler(ei, 4, size=0.5)
    assert npi.Block is S.Block and npi.DataFlow is S.DataFlow


def test_data_flow_orders_blocks_from_the_outermost_hop():
    batch = torch.tensor([5, 6])
    flow = npi.DataFlow(batch)
    hop0, hop1 = torch.tensor([1, 5, 6]), torch.tensor([0, 1, 2, 5, 6])
    flow.append(hop0, torch.tensor([1, 2]), torch.tensor([9]), torch.tensor([[0], [1]]))
    flow.append(hop1, torch.tensor([1, 3, 4]), torch.tensor([4, 7]), torch.tensor([[0, 2], [0, 1]]))
    assert len(flow) == 2 and flow.n_id is batch and flow.batch_size == 2
    assert flow[0].n_id is hop1 and flow[1].n_id is hop0 and [b.size for b in flow] == [(5, 3), (3, 2)]
    assert flow[0].size[1] == flow[1].size[0]                                        # a block's targets: the next block's n_id


# ---- batching: pure host code ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
def test_batches_partition_the_subset(shuffle):
    n, bs = 1000, 96
    full = S.epoch_batches(n, bs, shuffle, False, seed=3, epoch=0)
    assert [b.numel() for b in full] == [96] * 10 + [40]
    assert torch.equal(torch.cat(full).sort().values, torch.arange(n))               # every position exactly once
    dropped = S.epoch_batches(n, bs, shuffle, True, seed=3, epoch=0)
    assert len(dropped) == 10 and all(torch.equal(a, b) for a, b in zip(dropped, full))
    assert len(S.epoch_batches(960, bs, shuffle, True, seed=3, epoch=0)) == 10      # nothing short: nothing dropped
    assert S.epoch_batches(0, bs, shuffle, False, seed=3, epoch=0) == []
    if not shuffle:
        assert torch.equal(torch.cat(full), torch.arange(n))


def test_shuffle_is_a_function_of_seed_and_epoch():
    a = torch.cat(S.epoch_batches(500, 64, True, False, seed=11, epoch=4))
    assert torch.equal(a, torch.cat(S.epoch_batches(500, 64, True, False, seed=11, epoch=4)))
    assert not torch.equal(a, torch.cat(S.epoch_batches(500, 64, True, False, seed=11, epoch=5)))
    assert not torch.equal(a, torch.cat(S.epoch_batches(500, 64, True, False, seed=12, epoch=4)))
    with pytest.raises(ValueError):
        S.epoch_batches(10, 0, True, False, 0, 0)


def test_sampler_epochs_with_the_device_part_out_of_reach():
    """``__call__`` with the constructor's device work skipped and ``sample`` replaced: the batches of one epoch partition the
    subset, ``drop_last`` drops the short one, equal (seed, epoch) replay, consecutive epochs differ"""
    def make(seed, drop_last=False):
        s = object.__new__(npi.NeighborSampler)
        s.device, s.num_nodes, s.batch_size, s.shuffle, s.drop_last, s.seed, s.epoch = torch.device("cpu"), 300, 64, True, drop_last, seed, 0
        s.sample = lambda targets, seed=None: targets
        return s
    subset = torch.arange(300)[torch.arange(300) % 3 != 0]                             # 200 ids
    mask = torch.zeros(300, dtype=torch.bool)
    mask[subset] = True
    a = make(5)
    e0 = list(a(subset))
    assert a.epoch == 1 and [b.numel() for b in e0] == [64, 64, 64, 8]
    assert torch.equal(torch.cat(e0).sort().values, subset)
    e1 = list(a(mask))
    assert a.epoch == 2 and torch.equal(torch.cat(e1).sort().values, subset) and not torch.equal(torch.cat(e0), torch.cat(e1))
    b = make(5)
    assert all(torch.equal(x, y) for x, y in zip(e0, b(subset)))                      # same seed, same epoch
    b.epoch = 1
    assert all(torch.equal(x, y) for x, y in zip(e1, b(subset)))                      # epoch is settable: a replay
    assert [x.numel() for x in make(5, drop_last=True)(subset)] == [64, 64, 64]
    assert torch.equal(torch.cat(list(make(5)(None))).sort().values, torch.arange(300))
