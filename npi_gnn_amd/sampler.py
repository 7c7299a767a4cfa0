"""Neighbour sampling on the MI355X: PyG 1.4.2's ``torch_geometric.data.NeighborSampler`` in its bipartite form, producing
``DataFlow`` blocks for the pair form of ``SAGEConv`` / ``GATConv``::

    sampler = npi.NeighborSampler(edge_index, num_nodes, size=[25, 10], num_hops=2, batch_size=1024, shuffle=True, seed=0)
    for flow in sampler(subset):                      # subset: None (all nodes), a LongTensor of ids or a bool mask
        x = feat[flow[0].n_id]
        for block in flow:                            # outermost hop first
            x = conv((x, None), block.graph(), size=block.size, res_n_id=block.res_n_id)
        loss = crit(x, y[flow.n_id])

The reference walks the hops on the CPU (``torch_cluster.neighbor_sampler`` + ``torch.unique``); here every hop is three launches
over the by-target CSR of the edge list as it is (``npi_sample_counts``, ``npi_sample_select``, ``npi_sample_relabel_count`` /
``npi_sample_relabel``; ``include/npi_gnn.h`` states the sampling rule).  The sample of a node is a pure function of
``(seed, epoch, hop, node, its row)``: it does not depend on the other nodes of the batch, so a run can be replayed exactly
(``sampler.epoch``).  The random bits are not PyG's; the distribution -- uniform without replacement, at most ``size[l]``
in-neighbours per node of hop ``l`` -- and every field of ``Block`` / ``DataFlow`` are.

The same sampler serves PyG's OTHER data flow (``bipartite=False``, ``__produce_subgraph__``) for the layers that work in one id
space -- ``GCNConv``, the fused ``SAGEConv`` / ``GATConv``, ``GraphBatch``::

    for sub in sampler.subgraphs(subset):             # one relabelled subgraph per batch: the union of the hops' sampled edges
        g = sub.graph()                               # CSRGraph(sub.edge_index, sub.num_nodes)
        x = conv2(conv1(feat[sub.n_id], g).relu(), g)
        loss = crit(x[sub.sub_b_id], y[sub.b_id])

Its hops are the blocks above without self loops; ``npi_sample_union`` and ``npi_sample_coalesce`` then relabel both edge ends into
the ascending union of the batch and every hop's sources and merge equal pairs (``SubgraphBatch``), at the price of one more host read.

ONE host read per hop: the number of distinct source ids and of sampled edges fix the shapes of the block's tensors (as
``InteractionGraph.batch`` reads its totals).  A fractional ``size`` costs a second one (the edge total is not bounded by
``size * targets``).  Never inside a stream capture; CPU tensors raise ``NpiError`` -- there is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from . import graph as _graph
from ._draw import epoch_seed                                 # noqa: F401  (tools and tests import it from here)
from ._lib import NpiError, check, load, ptr, require_gpu, stream_ptr
from .graph import BipartiteGraph, CSRGraph, build_side


def epoch_batches(n: int, batch_size: int, shuffle: bool, drop_last: bool, seed: int, epoch: int) -> List[torch.Tensor]:
    """Positions ``[0, n)`` of one epoch cut into batches (host LongTensors): in order, or -- ``shuffle`` -- by
    ``torch.randperm`` under a ``torch.Generator`` seeded from ``(seed, epoch)``.  ``drop_last`` drops a short last batch."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(epoch_seed(seed, epoch) & ((1 << 63) - 1))
        order = torch.randperm(n, generator=g)
    else:
        order = torch.arange(n)
    out = list(torch.split(order, batch_size)) if n else []
    if drop_last and out and out[-1].numel() < batch_size:
        out.pop()
    return out


class Block:
    """One hop of a ``DataFlow`` (PyG 1.4.2 ``torch_geometric.data.sampler.Block``): ``n_id`` the global ids of the block's sources
    (ascending), ``res_n_id`` the position of every target in ``n_id`` (None without ``add_self_loops``), ``e_id`` the sampled
    columns of the original ``edge_index``, ``edge_index`` ``[2, E_s]`` with LOCAL ids (row 0 into ``n_id``, row 1 into the hop's
    target list), ``size = (N_src, N_dst)``."""

    __slots__ = ("n_id", "res_n_id", "e_id", "edge_index", "size", "_graph")

    def __init__(self, n_id, res_n_id, e_id, edge_index, size):
        self.n_id, self.res_n_id, self.e_id, self.edge_index, self.size = n_id, res_n_id, e_id, edge_index, tuple(size)
        self._graph = None

    def graph(self) -> BipartiteGraph:
        """``BipartiteGraph(edge_index, size)``, built on first use and kept (what the layers aggregate over)."""
        if self._graph is None:
            self._graph = BipartiteGraph(self.edge_index, self.size)
        return self._graph

    def __repr__(self):
        return f"Block(size={self.size}, edges={int(self.edge_index.size(1))})"


class DataFlow:
    """The blocks of one batch (PyG 1.4.2 ``DataFlow``): ``n_id`` the batch's targets, ``flow[0]`` the OUTERMOST hop (whose
    ``n_id`` gathers the input features), ``flow[len(flow) - 1]`` the hop next to the batch; iteration runs in that order, and
    every block's target list is the next block's ``n_id``."""

    def __init__(self, n_id: torch.Tensor, flow: str = "source_to_target"):
        self.n_id, self.flow = n_id, flow
        self.__last_n_id__ = n_id
        self.blocks: List[Block] = []

    @property
    def batch_size(self) -> int:
        return int(self.n_id.size(0))

    def append(self, n_id, res_n_id, e_id, edge_index) -> None:
        self.blocks.append(Block(n_id, res_n_id, e_id, edge_index, (int(n_id.size(0)), int(self.__last_n_id__.size(0)))))
        self.__last_n_id__ = n_id

    def __len__(self) -> int:
        return len(self.blocks)

    def __getitem__(self, idx: int) -> Block:
        return self.blocks[::-1][idx]

    def __iter__(self):
        return iter(self.blocks[::-1])

    def to(self, device):
        if torch.device(device) != self.n_id.device:
            raise NpiError("DataFlow.to: the blocks live on the GPU they were sampled on")
        return self

    def __repr__(self):
        sizes = [self.blocks[-1 - i].size[0] for i in range(len(self))] + [self.batch_size]
        return "DataFlow(" + " <- ".join(str(s) for s in reversed(sizes)) + ")"


class SubgraphBatch:
    """One batch of the one-id-space data flow (what PyG 1.4.2 ``NeighborSampler(bipartite=False)`` yields as a ``Data``):
    ``n_id`` the global ids of the subgraph's nodes, ascending -- the batch and every hop's sampled sources; ``edge_index``
    ``[2, E_u]`` the sampled edges of all hops with LOCAL ids on both ends (positions in ``n_id``), equal pairs merged, in ascending
    ``(source, target)`` order; ``e_id`` per column the smallest column of the original ``edge_index`` among the merged ones;
    ``b_id`` the batch's global ids as given; ``sub_b_id`` their positions in ``n_id`` (the rows the loss is taken on);
    ``num_nodes = len(n_id)``."""

    __slots__ = ("edge_index", "e_id", "n_id", "b_id", "sub_b_id", "num_nodes", "_graph")

    def __init__(self, edge_index, e_id, n_id, b_id, sub_b_id, num_nodes):
        self.edge_index, self.e_id, self.n_id, self.b_id, self.sub_b_id = edge_index, e_id, n_id, b_id, sub_b_id
        self.num_nodes = int(num_nodes)
        self._graph = None

    def graph(self) -> CSRGraph:
        """``CSRGraph(edge_index, num_nodes)``, built on first use and kept (what the square layers aggregate over)."""
        if self._graph is None:
            self._graph = CSRGraph(self.edge_index, self.num_nodes)
        return self._graph

    def to(self, device):
        if torch.device(device) != self.n_id.device:
            raise NpiError("SubgraphBatch.to: the subgraph lives on the GPU it was sampled on")
        return self

    def __repr__(self):
        return f"SubgraphBatch(num_nodes={self.num_nodes}, edges={int(self.edge_index.size(1))}, batch_size={int(self.b_id.size(0))})"


def _hop_budget(s) -> tuple:
    """(integer budget, fraction) of one ``size`` entry, as ``npi_sample_counts`` takes them"""
    if isinstance(s, bool) or not isinstance(s, (int, float)):
        raise ValueError(f"NeighborSampler: size entries are ints >= 1 or floats in (0, 1], got {s!r}")
    if isinstance(s, int):
        if s < 1:
            raise ValueError(f"NeighborSampler: an integer size must be at least 1, got {s}")
        return s, 0.0
    if not (0.0 < s <= 1.0):
        raise ValueError(f"NeighborSampler: a float size is a fraction in (0, 1], got {s}")
    return 0, float(s)


class NeighborSampler:
    """PyG 1.4.2 ``NeighborSampler(data, size, num_hops, batch_size, shuffle, drop_last, bipartite=True, add_self_loops,
    flow='source_to_target')`` over ``edge_index`` ``[2, E]`` (a GPU LongTensor; PyG layout) of a graph of ``num_nodes`` nodes.

    ``size``: a number or one per hop, hop 0 being the one next to the batch: an int keeps at most that many in-neighbours of a
    node, a float in (0, 1] the fraction ``ceil(size * degree)``.  ``add_self_loops``: every target is also a source of its
    block and ``Block.res_n_id`` says where (what ``SAGEConv(concat=True)`` and ``GATConv``'s ``x_dst`` need); no edge is added.
    ``seed``: with ``sampler.epoch`` (the count of the epoch the next call runs; readable and settable) it fixes the shuffle and
    every sample.  ``sampler(subset)`` is one epoch: a generator of ``DataFlow``\\ s; it counts ``epoch`` up when it is called.
    ``sampler.subgraphs(subset)`` is one epoch of PyG's other data flow (``bipartite=False``): a generator of
    ``SubgraphBatch``\\ es; the constructor's ``bipartite`` stays True (one sampler serves both).  Only ``flow='source_to_target'``
    exists."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, size: Union[int, float, Sequence], num_hops: int = 1,
                 batch_size: int = 1, shuffle: bool = False, drop_last: bool = False, bipartite: bool = True,
                 add_self_loops: bool = False, flow: str = "source_to_target", seed: int = 0):
        if not bipartite:
            raise ValueError("NeighborSampler: bipartite=False is not a constructor switch here: one sampler serves both data flows; "
                             "iterate sampler.subgraphs(subset) for the subgraph flow (sampler(subset) is the bipartite one)")
        if flow != "source_to_target":
            raise ValueError(f"NeighborSampler: flow={flow!r} is not available; only flow='source_to_target'")
        num_hops = int(num_hops)
        if num_hops < 1:
            raise ValueError("NeighborSampler: num_hops must be at least 1")
        sizes = list(size) if isinstance(size, (list, tuple)) else [size] * num_hops
        if len(sizes) != num_hops:
            raise ValueError(f"NeighborSampler: size has {len(sizes)} entries for num_hops={num_hops}")
        self._budgets = [_hop_budget(s) for s in sizes]
        if int(batch_size) < 1:
            raise ValueError("NeighborSampler: batch_size must be at least 1")
        if not isinstance(edge_index, torch.Tensor) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError("edge_index must be a LongTensor of shape [2, E]")
        self.device = require_gpu(edge_index)
        self.edge_index, self.num_nodes = edge_index, int(num_nodes)
        if not 0 <= self.num_nodes < 2 ** 31 - 1:
            raise ValueError("NeighborSampler: num_nodes out of range")
        self.size, self.num_hops, self.batch_size = sizes, num_hops, int(batch_size)
        self.shuffle, self.drop_last, self.add_self_loops = bool(shuffle), bool(drop_last), bool(add_self_loops)
        self.flow, self.seed, self.epoch = flow, int(seed), 0
        N = self.num_nodes
        # by-target CSR of the edge list as it is: no loop added or removed, eid = the edge's column
        self.side = build_side(edge_index[1].contiguous(), edge_index[0].contiguous(), N, N, self_loops=False, drop_equal=False)
        i32 = dict(dtype=torch.int32, device=self.device)
        self._scratch = torch.zeros(max(N, 1), **i32)         # zero between calls: npi_sample_relabel leaves it so
        self._ws = torch.empty(int(load().npi_sample_workspace_elems(N)), **i32)

    # ---- one hop ----------------------------------------------------------------------------------------------------------------------
    def sample_hop(self, targets: torch.Tensor, hop: int, seed: int):
        """One hop back from ``targets`` (int64 global ids on the device) with the budget of ``size[hop]`` and the key seed
        ``seed``: ``(n_id, res_n_id, e_id, edge_index)`` of the block.  One host read (two for a fractional size)."""
        return self._hop(targets, hop, seed, self.add_self_loops)[:4]

    def _hop(self, targets: torch.Tensor, hop: int, seed: int, add_self_loops: bool):
        """``sample_hop`` with the self-loop switch as an argument, and behind the block's four fields what ``npi_sample_select``
        wrote: int32 ``[3, E_s]`` -- global source id, edge-list column, index into ``targets`` -- of the sampled entries."""
        if torch.cuda.is_current_stream_capturing():
            raise NpiError("NeighborSampler: sampling reads sizes back from the device and cannot run inside a stream capture")
        lib, dev, side, N = load(), self.device, self.side, self.num_nodes
        require_gpu(targets)
        targets = targets.to(torch.int64).contiguous()
        n = int(targets.numel())
        budget, frac = self._budgets[hop]
        st = stream_ptr(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        cnt = torch.empty(max(n, 1), **i32)
        status = torch.empty(1, **i32)
        check(lib.npi_sample_counts(ptr(side.rowptr), N, ptr(targets), n, budget, frac, ptr(cnt), ptr(status), st), "npi_sample_counts")
        offsets = torch.zeros(n + 1, **i64)
        if n:
            torch.cumsum(cnt[:n], 0, out=offsets[1:])
        cap = n * budget if budget else int(offsets[-1].item())     # a fraction: the total is not bounded by the budget
        if cap > 2 ** 31 - 1:
            raise OverflowError("NeighborSampler: more than 2^31 - 1 sampled edges in one hop; use smaller batches")
        out = torch.empty((3, max(cap, 1)), **i32)                  # source id (global), edge id, local target index
        check(lib.npi_sample_select(ptr(side.rowptr), ptr(side.col), ptr(side.eid), N, ptr(targets), n, ptr(offsets), int(seed), int(hop),
                                    ptr(out[0]), ptr(out[1]), ptr(out[2]), cap, ptr(status), st), "npi_sample_select")
        info = torch.empty(2, **i32)
        loops = 1 if add_self_loops else 0
        check(lib.npi_sample_relabel_count(ptr(out[0]), ptr(offsets), n, cap, ptr(targets), loops, ptr(self._scratch), N, ptr(self._ws),
                                           ptr(info), st), "npi_sample_relabel_count")
        # the host read of the hop; the status words nobody has looked at yet ride along (graph.pending_status)
        pending = _graph.pending_status(dev)
        vals = torch.cat([info, status] + pending).tolist()
        U, E = vals[0], vals[1]
        n_id = torch.empty(U, **i64)
        ei = torch.empty((2, E), **i64)
        e_id = torch.empty(E, **i64)
        res = torch.empty(n, **i64) if add_self_loops else None
        check(lib.npi_sample_relabel(ptr(self._scratch), N, ptr(self._ws), ptr(out[0]), ptr(out[1]), ptr(out[2]), E, ptr(targets), n, U,
                                     ptr(n_id), ptr(ei[0]) if E else 0, ptr(ei[1]) if E else 0, ptr(e_id), ptr(res), ptr(status), st),
              "npi_sample_relabel")
        _graph.raise_on_status(vals[2:])                            # (after the scratch has been cleaned again)
        _graph.note_status(status)                                  # npi_sample_relabel's own bit: read with the next hop's sizes
        return n_id, res, e_id, ei, out[:, :E]

    def sample(self, targets: torch.Tensor, seed: Optional[int] = None) -> DataFlow:
        """The ``DataFlow`` of one batch of target ids; ``seed``: the key seed (default: that of the current epoch)."""
        seed = epoch_seed(self.seed, self.epoch) if seed is None else int(seed)
        targets = targets.to(device=self.device, dtype=torch.int64).contiguous()
        flow = DataFlow(targets, self.flow)
        n_id = targets
        for hop in range(self.num_hops):
            n_id, res, e_id, ei = self.sample_hop(n_id, hop, seed)
            flow.append(n_id, res, e_id, ei)
        return flow

    # ---- the one-id-space flow ----------------------------------------------------------------------------------------------------------
    def hop_entries(self, b_id: torch.Tensor, seed: int):
        """The sampled entries of every hop back from ``b_id``, concatenated, with GLOBAL ids on both ends: int32 ``(src_g, dst_g,
        eid)``.  The hops are those of ``sample`` without self loops, whatever ``add_self_loops`` this sampler was given."""
        src_g, dst_g, eid = [], [], []
        t_l = b_id
        for hop in range(self.num_hops):
            nxt, _, _, _, raw = self._hop(t_l, hop, seed, False)
            src_g.append(raw[0])
            dst_g.append(t_l[raw[2].long()].to(torch.int32))          # a hop's targets are indices into ITS target list
            eid.append(raw[1])
            t_l = nxt
        return torch.cat(src_g), torch.cat(dst_g), torch.cat(eid)

    def union_subgraph(self, b_id: torch.Tensor, src_g: torch.Tensor, dst_g: torch.Tensor, eid: torch.Tensor) -> "SubgraphBatch":
        """``hop_entries``' arrays and the batch -> the ``SubgraphBatch``: ``npi_sample_union`` (ascending union of all ids, both
        edge ends and the batch relabelled), ``npi_sample_coalesce`` (equal pairs merged, ascending), then ONE host read of both
        sizes -- ``n_id`` and the edge arrays are sized by their bounds ``min(N, n + E)`` and ``E`` and trimmed."""
        if torch.cuda.is_current_stream_capturing():
            raise NpiError("NeighborSampler: sampling reads sizes back from the device and cannot run inside a stream capture")
        lib, dev, N = load(), self.device, self.num_nodes
        n, E = int(b_id.numel()), int(src_g.numel())
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        if E > 2 ** 31 - 2:
            raise OverflowError("NeighborSampler: more than 2^31 - 2 sampled edges in one subgraph; use smaller batches")
        if n == 0 and E == 0:
            return SubgraphBatch(torch.empty((2, 0), **i64), torch.empty(0, **i64), torch.empty(0, **i64), b_id, b_id.clone(), 0)
        st = stream_ptr(dev)
        cap = min(N, n + E)                                             # a hop's target is a batch id or a source of the hop before
        n_id = torch.empty(cap, **i64)
        local = torch.empty((2, max(E, 1)), **i32)
        sub_b_id = torch.empty(n, **i64)
        info = torch.zeros(3, **i32)                                    # U, E (npi_sample_union); E_u (npi_sample_coalesce)
        status = torch.zeros(1, **i32)
        check(lib.npi_sample_union(ptr(src_g), ptr(dst_g), E, ptr(b_id), n, ptr(self._scratch), N, ptr(self._ws), cap, ptr(n_id),
                                   ptr(local[0]), ptr(local[1]), ptr(sub_b_id), ptr(info), ptr(status), st), "npi_sample_union")
        ei = torch.empty((2, E), **i64)
        e_id = torch.empty(E, **i64)
        if E:
            nbytes = int(lib.npi_sample_coalesce_workspace_bytes(E))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib.npi_sample_coalesce(ptr(local[0]), ptr(local[1]), ptr(eid), E, cap, ptr(ei[0]), ptr(ei[1]), ptr(e_id),
                                          ptr(info[2:]), ptr(ws), nbytes, st), "npi_sample_coalesce")
        # the host read of the union: both sizes at once, the status words nobody has looked at yet riding along
        pending = _graph.pending_status(dev)
        vals = torch.cat([info, status] + pending).tolist()
        _graph.raise_on_status(vals[3:])
        U, E_u = vals[0], vals[2]
        return SubgraphBatch(ei[:, :E_u].contiguous(), e_id[:E_u], n_id[:U], b_id, sub_b_id, U)

    def sample_subgraph(self, targets: torch.Tensor, seed: Optional[int] = None) -> "SubgraphBatch":
        """The ``SubgraphBatch`` of one batch of target ids (PyG 1.4.2 ``__produce_subgraph__``; ``include/npi_gnn.h`` states the
        semantics); ``seed``: the key seed (default: that of the current epoch).  One host read beyond the hops'."""
        seed = epoch_seed(self.seed, self.epoch) if seed is None else int(seed)
        b_id = targets.to(device=self.device, dtype=torch.int64).contiguous()
        return self.union_subgraph(b_id, *self.hop_entries(b_id, seed))

    # ---- one epoch --------------------------------------------------------------------------------------------------------------------
    def subset_ids(self, subset) -> torch.Tensor:
        dev = self.device
        if subset is None:
            return torch.arange(self.num_nodes, dtype=torch.int64, device=dev)
        subset = subset.to(dev)
        if subset.dtype in (torch.bool, torch.uint8):
            return subset.nonzero().view(-1)
        return subset.to(torch.int64).view(-1)

    def __call__(self, subset=None):
        """One epoch over ``subset``: a generator of ``DataFlow``\\ s.  The epoch's number is taken -- and ``epoch`` counted up --
        now, not at the first ``next()``."""
        return self._epoch(subset, self.sample)

    def subgraphs(self, subset=None):
        """One epoch over ``subset`` in the one-id-space flow: a generator of ``SubgraphBatch``\\ es.  Epoch counting, shuffle and key
        seed are those of ``__call__``: for a given ``(seed, epoch)`` both run over the same id lists."""
        return self._epoch(subset, self.sample_subgraph)

    def _epoch(self, subset, sample):
        epoch = self.epoch
        self.epoch = epoch + 1
        ids = self.subset_ids(subset)
        seed = epoch_seed(self.seed, epoch)
        batches = epoch_batches(int(ids.numel()), self.batch_size, self.shuffle, self.drop_last, self.seed, epoch)

        def run():
            for pos in batches:
                yield sample(ids[pos.to(self.device)], seed)
        return run()
