"""DropEdge (PyG 1.4.2 ``torch_geometric.utils.dropout_adj``) under Rule E of ``include/npi_gnn.h``: a column of ``edge_index`` is
dropped iff a word that is a pure function of ``(seed, draw, tick, column)`` -- undirected: of the column's unordered pair of ends --
lies below ``floor(p 2^64)``.  ``CSRGraph.drop_edges`` / ``BipartiteGraph.drop_edges`` filter both CSR sides of a graph without a
sort (``npi_csr_drop_side``: the kept entries keep their order and the parent's column numbers); ``dropout_adj`` is PyG's call over
the edge list itself, ``drop_edge_mask`` the decision, ``DropEdge`` the module with a draw counter."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Optional

import torch
from torch import nn

from . import _lib
from ._draw import check_edge_index, epoch_seed, next_draw
from ._lib import check, load, ptr, require_gpu, stream_ptr
from .graph import BipartiteGraph, CSRGraph, CSRSide, GraphBatch


def _as_i64(u: int) -> int:
    return u - (1 << 64) if u >= (1 << 63) else u


def check_p(p, who: str) -> float:
    """``p`` in ``[0, 1)``; PyG also takes ``p = 1`` (no edge left), this package does not"""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or math.isnan(float(p)) or not 0.0 <= float(p) < 1.0:
        raise ValueError(f"{who}: p must be a number in [0, 1), got {p!r}")
    return float(p)


def threshold(p: float) -> int:
    """``floor(p 2^64)`` in exact integer arithmetic, ``p`` taken as the double it is (Rule E's ``T``)"""
    return int(Fraction(float(p)) * 2 ** 64)


def _rule(who: str, p, seed, draw, tick, undirected, dev):
    """the trailing rule arguments of the C ABI: key, tick pointer, threshold, flags"""
    p = check_p(p, who)
    for name, v in (("seed", seed), ("draw", draw)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{who}: {name} must be an int, got {v!r}")
    if draw < 0:
        raise ValueError(f"{who}: draw must be >= 0, got {draw!r}")
    if tick is not None:
        if not isinstance(tick, torch.Tensor) or tick.dtype != torch.int64 or tick.numel() != 1 or not tick.is_cuda:
            raise ValueError(f"{who}: tick is None or a one-element int64 device tensor")
        if dev is not None and tick.device != dev:
            raise _lib.NpiError(f"{who}: tick lives on {tick.device}, the graph on {dev}")
    return epoch_seed(seed, draw), ptr(tick), _as_i64(threshold(p)), (_lib.NPI_DROP_UNDIRECTED if undirected else 0)


def _empty_side(parent: CSRSide) -> CSRSide:
    """arrays of the parent's capacity and item size"""
    dev = parent.rowptr.device
    i32 = dict(dtype=torch.int32, device=dev)
    n = max(parent.nnz_max, 1)
    side = CSRSide(torch.empty(parent.n_rows + 1, **i32), torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32),
                   torch.empty(parent.n_items + 1, **i32), parent.status, parent.nnz_max, parent.n_items)
    side.n_rows, side.n_cols, side.item, side.rect_hub = parent.n_rows, parent.n_cols, parent.item, parent.rect_hub
    side._hub_asked = True                        # never a hub plan: it costs a host read per side, and this side lives for one step
    return side


def _fits(side: Optional[CSRSide], parent: CSRSide) -> bool:
    return (side is not None and side.nnz_max == parent.nnz_max and side.n_rows == parent.n_rows and side.item == parent.item
            and side.rowptr.device == parent.rowptr.device)


def drop_side(parent: CSRSide, n_edges: int, rule, out: Optional[CSRSide] = None) -> CSRSide:
    """``npi_csr_drop_side`` of one side; ``out``: a side an earlier call returned for the same parent (its arrays are reused, what
    was derived from them is dropped)"""
    lib = load()
    dev = parent.rowptr.device
    key, tick, T, flags = rule
    side = out if _fits(out, parent) else _empty_side(parent)
    side._inv_cnt = None
    side.__dict__.pop("_root_w", None)
    ws_n = int(lib.npi_drop_edges_workspace_elems(parent.nnz_max))
    ws = torch.empty(ws_n, dtype=torch.int32, device=dev)
    check(lib.npi_csr_drop_side(ptr(parent.rowptr), ptr(parent.col), ptr(parent.eid), ptr(parent.rowidx), parent.n_rows, parent.nnz_max,
                                int(n_edges), key, tick, T, flags, side.nnz_max, side.item, ptr(side.rowptr), ptr(side.col), ptr(side.eid),
                                ptr(side.rowidx), ptr(side.item_row), ptr(ws), ws_n, stream_ptr(dev)), "npi_csr_drop_side")
    return side


_GRAPH_CACHES = ("_mean_t_w", "_tmap", "_tmap_inv", "_loop_edge_idx", "_root_only")


def _shell(parent, out):
    """a graph object over the parent's edge list, without any side: ``out`` (a graph an earlier ``drop_edges`` of this parent returned)
    with what was derived from its old sides dropped, or a new one"""
    if out is not None:
        if type(out) is not type(parent) or getattr(out, "dropped_from", None) is not parent:
            raise ValueError("drop_edges: out= takes a graph that an earlier drop_edges of this very graph returned")
        for name in _GRAPH_CACHES:
            out.__dict__.pop(name, None)
        return out
    g = object.__new__(type(parent))
    g.__dict__.update({k: v for k, v in parent.__dict__.items() if k not in _GRAPH_CACHES})
    g.by_dst, g._by_src = None, None
    g.dropped_from = parent
    return g


def drop_edges_csr(graph: CSRGraph, p, seed=0, draw=0, tick=None, undirected=False, training=True, out=None) -> CSRGraph:
    p = check_p(p, "CSRGraph.drop_edges")
    rule = _rule("CSRGraph.drop_edges", p, seed, draw, tick, undirected, graph.device)
    if not training or p == 0.0:
        return graph
    g = _shell(graph, out)
    g.by_dst = drop_side(graph.by_dst, graph.num_edges, rule, g.by_dst)
    g._by_src = drop_side(graph.by_src, graph.num_edges, rule, g._by_src)
    g.symmetric = bool(graph.symmetric and undirected)
    return g


class _DroppedBipartite(BipartiteGraph):
    """what ``BipartiteGraph.drop_edges`` returns: the derived sides are the DROP of the parent's (``root_side``), never a fresh sort"""

    def root_side(self, res_n_id: torch.Tensor) -> CSRSide:
        key = (res_n_id.data_ptr(), res_n_id._version, tuple(res_n_id.shape))
        if self._root is None or self._root[0] != key:
            parent = self.dropped_from.root_side(res_n_id)
            self._root = (key, drop_side(parent, self.num_edges, self._drop_rule), res_n_id)
        return self._root[1]

    def pair_side(self) -> CSRSide:
        raise ValueError("BipartiteGraph.pair_side: not on a graph drop_edges returned (the pair list of a score or a loss is not "
                         "subject to DropEdge: take it from the parent)")


def drop_edges_bipartite(graph: BipartiteGraph, p, seed=0, draw=0, tick=None, undirected=False, training=True, out=None) -> BipartiteGraph:
    if undirected:
        raise ValueError("BipartiteGraph.drop_edges: undirected=True needs one id space (the two ends of a column live in two)")
    p = check_p(p, "BipartiteGraph.drop_edges")
    rule = _rule("BipartiteGraph.drop_edges", p, seed, draw, tick, False, graph.device)
    if not training or p == 0.0:
        return graph
    if out is not None and (not isinstance(out, _DroppedBipartite) or out.dropped_from is not graph):
        raise ValueError("drop_edges: out= takes a graph that an earlier drop_edges of this very graph returned")
    if out is None:
        g = object.__new__(_DroppedBipartite)
        g.__dict__.update({k: v for k, v in graph.__dict__.items() if k not in _GRAPH_CACHES})
        g.by_dst, g._by_src = None, None
        g.dropped_from = graph
    else:
        g = out
        for name in _GRAPH_CACHES:
            g.__dict__.pop(name, None)
    g._root, g._pair, g._drop_rule = None, None, rule
    g.by_dst = drop_side(graph.by_dst, graph.num_edges, rule, g.by_dst)
    g._by_src = drop_side(graph.by_src, graph.num_edges, rule, g._by_src)
    return g


def drop_edge_mask(edge_index: torch.Tensor, p, seed: int = 0, draw: int = 0, tick: Optional[torch.Tensor] = None,
                   undirected: bool = False) -> torch.Tensor:
    """bool ``[E]``: column e of ``edge_index`` is KEPT under Rule E (``npi_drop_edge_keep``) -- the decision ``drop_edges`` and
    ``dropout_adj`` make, for tests and for variants composed from torch operations."""
    check_edge_index(edge_index)
    key, tk, T, flags = _rule("drop_edge_mask", p, seed, draw, tick, undirected, None)
    dev = require_gpu(edge_index, tick)
    E = int(edge_index.size(1))
    src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
    keep = torch.empty(E, dtype=torch.uint8, device=dev)
    check(load().npi_drop_edge_keep(ptr(src), ptr(dst), E, key, tk, T, flags, ptr(keep), stream_ptr(dev)), "npi_drop_edge_keep")
    return keep.bool()


def dropout_adj(edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor] = None, p: float = 0.5, force_undirected: bool = False,
                num_nodes: Optional[int] = None, training: bool = True, seed: int = 0, draw: int = 0,
                tick: Optional[torch.Tensor] = None, pad: bool = False):
    """PyG 1.4.2 ``dropout_adj``: ``(edge_index, edge_attr)`` with every column dropped with probability ``p`` -- under Rule E, so the
    result is a function of ``(seed, draw, tick)`` and not of torch's generator (``npi_drop_edge_list``: the kept columns compacted
    in input order, ``edge_attr``'s rows following).  ``p`` in ``[0, 1)``: PyG's ``p = 1`` is refused.  ``training=False`` or
    ``p == 0``: the inputs themselves.  ``num_nodes`` is accepted for PyG's signature and not needed.

    ``pad=False`` reads ONE word back (the length).  ``pad=True`` reads nothing: the list keeps its length ``E``, the kept columns in
    front and ``(-1, -1)`` columns behind them (the padding every consumer of this package drops), ``edge_attr`` keeps ``E`` rows
    with zeros behind the kept ones -- capture-safe.

    ``force_undirected=True`` keys the rule on the column's unordered pair of ends: ``(u, v)``, ``(v, u)`` and parallel duplicates
    are kept or dropped together, and the output is the input's columns whose pair is kept, in INPUT order.  For a list that holds
    both directions this is PyG's edge set; PyG returns it in another order (``row < col`` first, then the mirrored half) and
    discards ``(i, i)`` columns there, which stay subject to the rule here like any other column."""
    check_edge_index(edge_index)
    key, tk, T, flags = _rule("dropout_adj", p, seed, draw, tick, force_undirected, None)
    E = int(edge_index.size(1))
    if edge_attr is not None and edge_attr.size(0) != E:
        raise ValueError(f"dropout_adj: edge_attr has {edge_attr.size(0)} rows, edge_index {E} columns")
    if not training or T == 0:
        return edge_index, edge_attr
    dev = require_gpu(edge_index, edge_attr, tick)
    lib = load()
    src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
    out = torch.empty((2, E), dtype=torch.int64, device=dev)
    newpos = torch.empty(max(E, 1), dtype=torch.int32, device=dev) if edge_attr is not None else None
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws_n = int(lib.npi_drop_edges_workspace_elems(E))
    ws = torch.empty(ws_n, dtype=torch.int32, device=dev)
    check(lib.npi_drop_edge_list(ptr(src), ptr(dst), E, key, tk, T, flags, ptr(out[0]), ptr(out[1]), ptr(newpos), ptr(count),
                                 1 if pad else 0, ptr(ws), ws_n, stream_ptr(dev)), "npi_drop_edge_list")
    if pad:
        if edge_attr is not None:
            # row newpos[e] <- row e; the dropped rows land in a spare last row that is cut off again (no length is read)
            pos = newpos[:E].long()
            pos = torch.where(pos < 0, torch.full_like(pos, E), pos)
            attr = torch.zeros((E + 1,) + tuple(edge_attr.shape[1:]), dtype=edge_attr.dtype, device=dev)
            attr.index_copy_(0, pos, edge_attr)
            edge_attr = attr[:E]
        return out, edge_attr
    n = int(count.item())
    if edge_attr is not None:
        # which input row each kept position takes: the inverse of newpos (dropped rows fall into a spare last slot)
        pos = newpos[:E].long()
        pos = torch.where(pos < 0, torch.full_like(pos, E), pos)
        sel = torch.zeros(E + 1, dtype=torch.int64, device=dev).index_copy_(0, pos, torch.arange(E, device=dev))
        edge_attr = edge_attr.index_select(0, sel[:n])
    return out[:, :n], edge_attr


class DropEdge(nn.Module):
    """``DropEdge(p, seed=0, undirected=False)``: ``forward(graph)`` is ``graph.drop_edges(p, seed, draw)`` with ``draw`` the module's
    counter, which every training-mode call counts up (readable and settable, as ``GATConv.draw``: set it back to replay a step);
    in ``eval()`` the identity.  ``graph``: a ``CSRGraph``, a ``BipartiteGraph`` or a ``GraphBatch`` (its ``.graph()``).  ``tick``: the
    device word of a captured step.  Call it once per layer for independent masks per layer."""

    def __init__(self, p: float = 0.5, seed: int = 0, undirected: bool = False):
        super().__init__()
        self.p = check_p(p, "DropEdge")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"DropEdge: seed must be an int, got {seed!r}")
        self.seed, self.undirected = seed, bool(undirected)
        self.draw = 0

    def forward(self, graph, tick: Optional[torch.Tensor] = None, out=None):
        if isinstance(graph, GraphBatch):
            graph = graph.graph()
        if not isinstance(graph, (CSRGraph, BipartiteGraph)):
            raise TypeError("DropEdge: a CSRGraph, a BipartiteGraph or a GraphBatch")
        if not self.training or self.p == 0.0:
            return graph
        return graph.drop_edges(self.p, seed=self.seed, draw=next_draw(self, None), tick=tick, undirected=self.undirected, out=out)

    def extra_repr(self):
        return f"p={self.p}, seed={self.seed}, undirected={self.undirected}"
