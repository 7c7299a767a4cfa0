"""Random walks and the Node2Vec model on the MI355X: the node2vec columns of the feature vector, trained where the graph is::

    rw = npi.RandomWalker(edge_index, num_nodes, seed=0, p=1.0, q=1.0, tries=64)   # sorts once: by-source side, sort_columns=True
    walks = rw.walks(start, walk_length, draw=None)                    # LongTensor [len(start), walk_length + 1]; no host read
    npi.random_walk(row, col, start, walk_length, p=1, q=1, num_nodes=None, seed=0)   # torch_cluster's name: one walker per call

    model = npi.Node2Vec(num_nodes, embedding_dim, walk_length, context_size, walks_per_node=1, p=1, q=1,
                         num_negative_samples=None, seed=0).cuda()
    z = model(subset)                                                  # embedding rows, as PyG
    loss = model.loss(edge_index, subset=None)                         # walks -> pairs -> link_loss(..., "gae")

The reference computes these columns offline (``node2vec-master/src/main.py``: alias-sampled walks with p = q = 1, 10 x 80 per node,
then gensim skip-gram) and reads them from ``result.emb`` files; PyG 1.4.2 has the same thing as ``torch_geometric.nn.models.Node2Vec``
over ``torch_cluster.random_walk``.  Here ``walks`` is Rule W of ``include/npi_gnn.h``: one counter-based splitmix64 stream per walk
slot, a uniform pick of a neighbour, and -- for ``p`` or ``q`` other than 1 -- node2vec's second-order bias by rejection, membership
by a binary search of the sorted by-source row (no alias tables).  ``Node2Vec.loss`` is PyG's: every window of ``context_size`` nodes of
every walk gives ``context_size - 1`` positive pairs, every window start ``num_negative_samples`` uniform nodes as negatives, and the
loss over them is ``GAE.recon_loss`` -- ``functional.link_loss(..., "gae")``, forward and backward on the package's own kernels,
bitwise reproducible.  The random bits are not torch_cluster's or PyG's, the distributions are.

Pass the undirected edge list (both directions), as the reference's node2vec does; one id space only.  CPU tensors raise
``NpiError``: there is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import nn

from . import functional as F_
from . import graph as _graph
from ._draw import _LIMIT, check_edge_index, epoch_seed, next_draw, num_nodes as _num_nodes
from ._lib import NPI_PAIR_LOSS_GAE, NpiError, check, load, ptr, require_gpu, stream_ptr
from .graph import build_side

_ONE = 2 ** 32                  # the threshold that accepts every candidate


def walk_thresholds(p: float, q: float) -> Tuple[int, int, int]:
    """``(thr_ret, thr_nbr, thr_far)`` of Rule W: ``min(2^32, floor(2^32 * a / mx))`` for ``a`` in ``(1/p, 1, 1/q)`` -- node2vec's
    unnormalised weights of returning, of moving to a common neighbour and of moving away -- and ``mx`` the largest of them, in
    double.  ``p == q == 1``: three times ``2^32``."""
    p, q = float(p), float(q)
    if not (math.isfinite(p) and math.isfinite(q) and p > 0.0 and q > 0.0):
        raise ValueError(f"RandomWalker: p and q must be positive and finite, got p={p!r}, q={q!r}")
    a = (1.0 / p, 1.0, 1.0 / q)
    mx = max(a)
    if not math.isfinite(mx):
        raise ValueError(f"RandomWalker: p and q must be positive and finite with finite inverses, got p={p!r}, q={q!r}")
    return tuple(min(_ONE, int(math.floor(_ONE * (v / mx)))) for v in a)      # (2^32 * x is exact: the product cannot round)


class RandomWalker:
    """Walks over the graph ``edge_index`` ``[2, E]`` (a GPU LongTensor, PyG layout, one id space of ``num_nodes`` nodes): a step
    goes from a node to the target of one of its out-edges.  An edge is a column of ``edge_index`` as it is: no self loop is added
    or removed; parallel edges weigh in the pick, as in torch_cluster, and count once for the p/q bias.  A node without out-edges
    keeps the walk where it is.

    ``seed`` and a draw number fix every result.  ``draw`` (readable and settable, like ``NegativeSampler.draw``) is the number
    the next call takes when it is not given one; such a call counts it up."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, seed: int = 0, p: float = 1.0, q: float = 1.0, tries: int = 64):
        check_edge_index(edge_index)
        self.num_nodes = _num_nodes(num_nodes, "RandomWalker")
        self.thresholds = walk_thresholds(p, q)
        self.tries = int(tries)
        if self.tries < 1 or self.tries >= _LIMIT:
            raise ValueError(f"RandomWalker: tries must be at least 1, got {tries}")
        self.device = require_gpu(edge_index)
        self.edge_index, self.seed, self.p, self.q, self.draw = edge_index, int(seed), float(p), float(q), 0
        self.num_edges = int(edge_index.size(1))
        # by-source CSR of the edge list as it is, columns ascending within a row: what the pick indexes and the p/q search walks.
        # An id out of range is dropped by the build and reported with the next status read (graph.check_pending()).
        N = self.num_nodes
        self.side = build_side(edge_index[0].contiguous(), edge_index[1].contiguous(), N, N, self_loops=False, drop_equal=False,
                               sort_columns=True)

    def walks(self, start: torch.Tensor, walk_length: int, draw: Optional[int] = None) -> torch.Tensor:
        """Rule W: ``[len(start), walk_length + 1]`` -- row ``w`` is the walk of slot ``w``, from ``start[w]`` (torch_cluster's
        layout).  Slots are independent streams: a start that is repeated gives different walks.  A start outside
        ``[0, num_nodes)`` gives a row of -1; a step whose ``tries`` candidates were all rejected takes the last one; either is
        reported through the status word (``graph.check_pending()`` raises).  No host read: inside a stream capture pass a
        ``start`` that is already a contiguous LongTensor."""
        if isinstance(walk_length, bool) or not isinstance(walk_length, int) or walk_length < 0 or walk_length >= _LIMIT:
            raise ValueError(f"RandomWalker.walks: walk_length must be a non-negative int, got {walk_length!r}")
        if not isinstance(start, torch.Tensor) or start.dtype != torch.int64 or start.dim() != 1:
            raise ValueError("RandomWalker.walks: start must be a LongTensor of node ids, shape [W]")
        dev = require_gpu(start)
        if dev != self.device:
            raise NpiError(f"tensors on different devices: {self.device} vs {dev}")
        start = start.contiguous()
        W = int(start.numel())
        if W >= _LIMIT:
            raise NpiError("RandomWalker.walks: more than 2^31 - 2 walks in one call")
        key = epoch_seed(self.seed, next_draw(self, draw))
        out = torch.empty((W, walk_length + 1), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        side, thr = self.side, self.thresholds
        check(load().npi_random_walk(ptr(side.rowptr), ptr(side.col), self.num_nodes, ptr(start), W, walk_length, key, thr[0], thr[1],
                                     thr[2], self.tries, ptr(out), ptr(status), stream_ptr(dev)), "npi_random_walk")
        _graph.note_status(status)
        return out

    def __repr__(self):
        return f"RandomWalker(num_nodes={self.num_nodes}, edges={self.num_edges}, p={self.p}, q={self.q}, tries={self.tries})"


def random_walk(row: torch.Tensor, col: torch.Tensor, start: torch.Tensor, walk_length: int, p: float = 1, q: float = 1,
                num_nodes: Optional[int] = None, seed: int = 0) -> torch.Tensor:
    """torch_cluster's ``random_walk(row, col, start, walk_length, p, q, num_nodes)``:
    ``RandomWalker(stack([row, col]), num_nodes, seed, p, q).walks(start, walk_length)``.  One walker -- one sort of the edge list
    -- per call: keep a ``RandomWalker`` for a graph that stays.  ``num_nodes=None`` reads the largest id back from the device."""
    for t, name in ((row, "row"), (col, "col"), (start, "start")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"random_walk: {name} must be a 1-D LongTensor")
    if row.numel() != col.numel():
        raise ValueError(f"random_walk: row has {row.numel()} entries, col {col.numel()}")
    require_gpu(row, col, start)
    if num_nodes is None:
        num_nodes = int(torch.cat([row, col, start]).max()) + 1 if row.numel() + start.numel() else 1
    return RandomWalker(torch.stack([row, col]), num_nodes, seed=seed, p=p, q=q).walks(start, walk_length)


def walk_pairs(walks: torch.Tensor, context_size: int, num_negative_samples: int, num_nodes: int, key: int) -> Tuple[torch.Tensor, int]:
    """The pair list of PyG's ``Node2Vec.loss`` over ``walks [W, L + 1]`` (``npi_walk_pairs``): ``([2, M], n_pos)`` in the
    ``cat([pos, neg], 1)`` layout ``link_loss`` scores -- the ``n_pos = R (c - 1)`` positives ``(window start, the node k places
    on)`` of the ``R = (L + 2 - c) W`` windows in PyG's order, then ``S`` uniform nodes per window start (``key``: an
    ``epoch_seed``).  No host read."""
    if not isinstance(walks, torch.Tensor) or walks.dtype != torch.int64 or walks.dim() != 2 or walks.size(1) < 1:
        raise ValueError("walk_pairs: walks must be a LongTensor [W, L + 1]")
    dev = require_gpu(walks)
    walks = walks.contiguous()
    W, L = int(walks.size(0)), int(walks.size(1)) - 1
    c, S, N = int(context_size), int(num_negative_samples), _num_nodes(num_nodes, "RandomWalker")
    if c < 2 or c > L + 1:
        raise ValueError(f"walk_pairs: context_size lies in [2, walk_length + 1] = [2, {L + 1}], got {context_size}")
    if S < 0:
        raise ValueError(f"walk_pairs: num_negative_samples must not be negative, got {num_negative_samples}")
    R = (L + 2 - c) * W
    M = R * (c - 1 + S)
    if W >= _LIMIT or M >= _LIMIT:
        raise NpiError(f"walk_pairs: {M} pairs pass 2^31 - 2; use fewer walks per call")
    pairs = torch.empty((2, M), dtype=torch.int64, device=dev)
    check(load().npi_walk_pairs(ptr(walks), W, L, c, S, N, int(key), ptr(pairs[0]) if M else 0, ptr(pairs[1]) if M else 0,
                                stream_ptr(dev)), "npi_walk_pairs")
    return pairs, R * (c - 1)


class Node2Vec(nn.Module):
    """PyG 1.4.2 ``Node2Vec(num_nodes, embedding_dim, walk_length, context_size, walks_per_node=1, p=1, q=1,
    num_negative_samples=None)``: the same constructor, ``forward``, ``loss`` and ``state_dict`` layout (``embedding.weight``), so a
    PyG checkpoint loads.  ``num_negative_samples=None`` means ``context_size - 1``.  ``seed`` and ``draw`` (the number of ``loss``
    calls made; readable and settable) fix the walks and the negatives of every call.  ``Node2Vec.test`` is not provided."""

    MAX_WALKERS = 8             # edge lists whose sorted side is kept

    def __init__(self, num_nodes: int, embedding_dim: int, walk_length: int, context_size: int, walks_per_node: int = 1, p: float = 1,
                 q: float = 1, num_negative_samples: Optional[int] = None, seed: int = 0, tries: int = 64):
        super().__init__()
        assert walk_length >= context_size
        self.num_nodes, self.embedding_dim = _num_nodes(num_nodes, "RandomWalker"), int(embedding_dim)
        self.walk_length, self.context_size, self.walks_per_node = int(walk_length), int(context_size), int(walks_per_node)
        if self.context_size < 2 or self.walks_per_node < 1:
            raise ValueError("Node2Vec: context_size must be at least 2 and walks_per_node at least 1")
        walk_thresholds(p, q)                                  # (refuses a bad p or q here, not at the first loss)
        self.p, self.q, self.seed, self.tries, self.draw = float(p), float(q), int(seed), int(tries), 0
        self.num_negative_samples = self.context_size - 1 if num_negative_samples is None else int(num_negative_samples)
        if self.num_negative_samples < 0:
            raise ValueError(f"Node2Vec: num_negative_samples must not be negative, got {num_negative_samples}")
        self.embedding = nn.Embedding(self.num_nodes, self.embedding_dim)
        self._walkers = {}                                     # id(edge_index) -> (edge_index, its version, RandomWalker)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self.embedding.reset_parameters()

    def forward(self, subset: torch.Tensor) -> torch.Tensor:
        """the embedding rows of the nodes ``subset``"""
        return self.embedding(subset)

    def walker(self, edge_index: torch.Tensor) -> RandomWalker:
        """the ``RandomWalker`` of ``edge_index``: one per tensor OBJECT seen (identity and version, like the graph caches of the
        layers), so the sort is paid once for an edge list that stays"""
        hit = self._walkers.get(id(edge_index))
        if hit is not None and hit[0] is edge_index and hit[1] == edge_index._version:
            return hit[2]
        rw = RandomWalker(edge_index, self.num_nodes, seed=self.seed, p=self.p, q=self.q, tries=self.tries)
        self._walkers.pop(id(edge_index), None)
        while len(self._walkers) >= self.MAX_WALKERS:
            self._walkers.pop(next(iter(self._walkers)))
        self._walkers[id(edge_index)] = (edge_index, edge_index._version, rw)
        return rw

    def sample(self, edge_index: torch.Tensor, subset: Optional[torch.Tensor] = None, draw: Optional[int] = None):
        """the walks and the pair list of one ``loss`` call: ``(walks [W, walk_length + 1], pairs [2, M], n_pos)`` with
        ``subset.repeat(walks_per_node)`` as the starts (``subset=None``: every node).  ``draw=None`` takes the model's counter and
        counts it up."""
        rw = self.walker(edge_index)
        if subset is None:
            subset = torch.arange(self.num_nodes, device=rw.device)
        draw = next_draw(self, draw)
        walks = rw.walks(subset.repeat(self.walks_per_node), self.walk_length, draw=draw)
        pairs, n_pos = walk_pairs(walks, self.context_size, self.num_negative_samples, self.num_nodes, epoch_seed(self.seed, draw))
        return walks, pairs, n_pos

    def loss(self, edge_index: torch.Tensor, subset: Optional[torch.Tensor] = None) -> torch.Tensor:
        """PyG's ``Node2Vec.loss(edge_index, subset)``: ``-log(sigmoid(<z_start, z_context>) + 1e-15).mean()`` over the positive
        pairs plus ``-log(1 - sigmoid(<z_start, z_random>) + 1e-15).mean()`` over the negative ones.  The pair list goes to the
        loss path of ``functional.link_loss`` as it is written; the backward reaches ``embedding.weight`` through deterministic
        segmented sums (no float atomics)."""
        z = F_._pair_tables(self.embedding.weight, None, "Node2Vec.loss")[0]
        require_gpu(z)
        _, pairs, n_pos = self.sample(edge_index, subset)
        plist = F_._PairList(pairs, self.num_nodes, self.num_nodes, "Node2Vec.loss")
        return F_._LinkLossFn.apply(z, None, plist, n_pos, NPI_PAIR_LOSS_GAE)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.num_nodes}, {self.embedding_dim}, p={self.p}, q={self.q})"
