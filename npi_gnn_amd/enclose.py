"""Enclosing subgraphs of candidate links, extracted, labelled and collated on the MI355X (Rule H of ``include/npi_gnn.h``).

``InteractionGraph.batch`` restates the reference's sample: a one-hop star around the target pair, labelled 0 / 1.  SEAL, the method
the reference follows, classifies the *enclosing subgraph*: every node within ``h`` hops of either target, EVERY edge among them
(the partner-to-partner edges are the length-3 paths that tell a true link from a false one), the target link itself removed, and
every node labelled by its distances to both targets (DRNL).  ``EnclosingSubgraphs.batch(keys)`` builds that batch for any list of
target pairs directly in HBM -- one workgroup per sample, bitmaps instead of frontier lists, nothing sorted -- ready for the layers
and for ``global_sort_pool``, SEAL's readout.  It follows Rule H, not the reference's own h-hop class (dead code with a by-value
counter bug).

Everything is integer work and a pure function of the inputs; ``tests/_enclose_ref.py`` restates the rule with Python sets.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib
from . import graph as _graph
from ._lib import check, load, ptr, require_gpu, stream_ptr
from .graph import CSRGraph, GraphBatch, build_side

#: the largest bitmap workspace a call may ask for (four bitmaps of ``num_nodes`` bits per key)
WORKSPACE_CAP = 1 << 30

_LABELS = {None: _lib.NPI_ENCLOSE_LABEL_NONE, "drnl": _lib.NPI_ENCLOSE_LABEL_DRNL, "targets": _lib.NPI_ENCLOSE_LABEL_TARGETS}
_TARGET_EDGE = {"remove": 0, "add": _lib.NPI_ENCLOSE_ADD_TARGET_EDGE}


def workspace_bytes(num_nodes: int, num_keys: int) -> int:
    """Bytes of bitmap workspace ``num_keys`` samples over ``num_nodes`` nodes need (``npi_enclose_workspace_bytes``, restated on the
    host so that the cap below is decided before the device is touched): four bitmaps' worth per sample."""
    return (int(num_keys) * 4 * ((int(num_nodes) + 31) // 32) * 4 + 15) // 16 * 16


def check_workspace(num_nodes: int, num_keys: int) -> int:
    """``workspace_bytes``, or a ``ValueError`` when it exceeds ``WORKSPACE_CAP``."""
    need = workspace_bytes(num_nodes, num_keys)
    if need > WORKSPACE_CAP:
        raise ValueError(f"EnclosingSubgraphs: {num_keys} keys over {num_nodes} nodes need {need} bytes of bitmaps, more than the cap of "
                         f"{WORKSPACE_CAP}; pass fewer keys per call (at most {max_keys(num_nodes)})")
    return need


def max_keys(num_nodes: int) -> int:
    """keys per call that fit ``WORKSPACE_CAP``"""
    return WORKSPACE_CAP // max(workspace_bytes(num_nodes, 1), 1)


class EnclosingBatch:
    """What ``EnclosingSubgraphs.batch`` returns.

    graph_batch  ``GraphBatch(x, edge_index, batch, B, graph_ptr=, sizes=, symmetric=True)``: what the layers take
    node_id      int64 [n]      the global id of every row (local 0 / 1 of a sample: its targets u / v, then ascending ids)
    z            int64 [n]      DRNL label
    dist         int32 [n, 2]   distances to u (v removed) and to v (u removed); -1: unreachable, or the other target
    e_id         int64 [e]      the column of ``edge_index`` every emitted entry is; -1 for an added target edge
    graph_ptr, edge_ptr  int32 [B + 1]  first row / first entry of every sample
    local_rowptr, local_col  int32 [n + 1] / [e]  the emitted entries as a by-target CSR over the batch's rows (no loops)"""

    __slots__ = ("graph_batch", "node_id", "z", "dist", "e_id", "graph_ptr", "edge_ptr", "local_rowptr", "local_col")

    def __init__(self, graph_batch, node_id, z, dist, e_id, graph_ptr, edge_ptr, local_rowptr, local_col):
        self.graph_batch, self.node_id, self.z, self.dist, self.e_id = graph_batch, node_id, z, dist, e_id
        self.graph_ptr, self.edge_ptr, self.local_rowptr, self.local_col = graph_ptr, edge_ptr, local_rowptr, local_col

    @property
    def num_graphs(self) -> int:
        return int(self.graph_ptr.numel()) - 1

    def __repr__(self):
        return f"EnclosingBatch({self.graph_batch!r})"


def _label(rowptr, col, n, nnz, src, dst, graph_ptr, B, z, dist, dev) -> None:
    check(load().npi_drnl_label(ptr(rowptr), ptr(col), n, nnz, ptr(src), ptr(dst), ptr(graph_ptr), B, ptr(z), ptr(dist),
                                stream_ptr(dev)), "npi_drnl_label")


class EnclosingSubgraphs:
    """The h-hop enclosing subgraphs of an undirected graph in one id space (the bipartite ncRNA-protein graphs in their serial
    numbering included), resident on the GPU.

    ``edge_index [2, E]`` int64 holds every edge in both directions; ``edge_mask [E]`` bool (``False``: the column does not exist --
    a fold's test links, say) is equal on both directions.  ``feat [N, F]`` float32 or None.  ``target_edge``: ``"remove"`` (SEAL:
    the target link is never walked and never emitted) or ``"add"`` (the same, then one ``(1 -> 0)`` and one ``(0 -> 1)`` column
    with ``e_id = -1`` in front of rows 0 and 1 of every sample: the reference's convention, positives and negatives both carry
    their target edge).  ``label``: the first column of ``x`` -- ``"drnl"``: ``float(z)``; ``"targets"``: the reference's 0 for the
    two targets and 1 elsewhere; ``None``: no column.  ``check_input``: verify once, with torch ops, that ids are in range and
    that the edge list and the mask are symmetric (a ``ValueError`` otherwise)."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, num_hops: int = 2, feat: Optional[torch.Tensor] = None,
                 edge_mask: Optional[torch.Tensor] = None, target_edge: str = "remove", label: Optional[str] = "drnl",
                 check_input: bool = True):
        if target_edge not in _TARGET_EDGE:
            raise ValueError(f"EnclosingSubgraphs: target_edge must be 'remove' or 'add', got {target_edge!r}")
        if label not in _LABELS:
            raise ValueError(f"EnclosingSubgraphs: label must be 'drnl', 'targets' or None, got {label!r}")
        if int(num_hops) < 1:
            raise ValueError(f"EnclosingSubgraphs: num_hops must be at least 1, got {num_hops}")
        self.num_nodes = N = int(num_nodes)
        if N < 1 or N >= 2 ** 31 - 1:
            raise ValueError(f"EnclosingSubgraphs: num_nodes must lie in [1, 2^31 - 1), got {N}")
        check_workspace(N, 1)
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("EnclosingSubgraphs: edge_index must be a LongTensor of shape [2, E]")
        E = int(edge_index.size(1))
        if edge_mask is not None and (edge_mask.dtype != torch.bool or edge_mask.dim() != 1 or int(edge_mask.numel()) != E):
            raise ValueError("EnclosingSubgraphs: edge_mask must be a bool tensor of E elements")
        if feat is not None:
            if feat.dtype != torch.float32 or feat.dim() != 2:
                raise TypeError("EnclosingSubgraphs: feat must be a float32 matrix")
            if feat.size(0) < N:
                raise ValueError("EnclosingSubgraphs: feat has fewer rows than num_nodes")
        self.num_hops, self.target_edge, self.label = int(num_hops), target_edge, label
        self._flags, self._label_mode = _TARGET_EDGE[target_edge], _LABELS[label]
        dev = require_gpu(edge_index, edge_mask, feat)
        self.device = dev
        src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
        if check_input and E:
            lo, hi = torch.stack([edge_index.min(), edge_index.max()]).tolist()
            if lo < 0 or hi >= N:
                raise ValueError("EnclosingSubgraphs: edge_index holds a node id outside [0, num_nodes)")
            fwd, bwd = src * N + dst, dst * N + src
            if not torch.equal(torch.sort(fwd).values, torch.sort(bwd).values):
                raise ValueError("EnclosingSubgraphs: edge_index is not symmetric (every edge must be there in both directions)")
            if edge_mask is not None and not torch.equal(torch.sort(fwd[edge_mask]).values, torch.sort(bwd[edge_mask]).values):
                raise ValueError("EnclosingSubgraphs: edge_mask differs on the two directions of an edge")
        # the parent graph: by-target CSR without loops, (i, i) columns dropped, a row's entries in (source id, column number) order
        self.side = build_side(dst, src, N, N, self_loops=False, drop_equal=True, sort_columns=True)
        self.mask = None if edge_mask is None else edge_mask.to(torch.uint8).contiguous()
        self.feat = None if feat is None else feat.contiguous()
        self.num_edges = E

    # ---- the two launches every call shares ------------------------------------------------------------------------------------------
    def _keys(self, keys: torch.Tensor) -> torch.Tensor:
        if keys.dim() != 2 or keys.size(1) != 2:
            raise ValueError("EnclosingSubgraphs: keys must have shape [K, 2]")
        # (ids beyond int32 stay out of range instead of wrapping into it)
        return keys.to(self.device).clamp(min=-1, max=self.num_nodes).to(torch.int32).contiguous()

    def _sizes(self, keys: torch.Tensor, status: torch.Tensor):
        lib, dev, s = load(), self.device, self.side
        B = int(keys.size(0))
        nbytes = check_workspace(self.num_nodes, B)
        i32 = dict(dtype=torch.int32, device=dev)
        counts, node_off, edge_off = torch.empty(max(2 * B, 1), **i32), torch.empty(B + 1, **i32), torch.empty(B + 1, **i32)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.npi_enclose_sizes(ptr(s.rowptr), ptr(s.col), ptr(s.eid), ptr(self.mask), self.num_nodes, ptr(keys), B, self.num_hops,
                                    self._flags, ptr(counts), ptr(node_off), ptr(edge_off), ptr(ws), int(ws.numel()), ptr(status),
                                    stream_ptr(dev)), "npi_enclose_sizes")
        return counts, node_off, edge_off, ws

    def sizes(self, keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(nodes, directed edges) per sample of ``keys [K, 2]`` as HOST int64 tensors -- ONE device read for the whole key list (the
        list is worked through in chunks that fit ``WORKSPACE_CAP``).  A sample's size depends on its key only, so a loader that keeps
        them (``net1.KeyLoader``) can tell ``batch`` the totals of every batch it asks for."""
        keys = self._keys(keys)
        K = int(keys.size(0))
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        step = max(1, max_keys(self.num_nodes))
        parts = [self._sizes(keys[i:i + step], status)[0][: 2 * min(step, K - i)].view(2, -1) for i in range(0, K, step)]
        pending = _graph.pending_status(self.device)
        flat = torch.cat([p.reshape(-1) for p in parts] + [status] + pending).cpu()
        _graph.raise_on_status(flat[2 * K:].tolist())
        nodes, edges, at = [], [], 0
        for p in parts:
            k = int(p.size(1))
            nodes.append(flat[at:at + k])
            edges.append(flat[at + k:at + 2 * k])
            at += 2 * k
        z64 = torch.zeros(0, dtype=torch.int64)
        return (torch.cat(nodes).to(torch.int64) if nodes else z64), (torch.cat(edges).to(torch.int64) if edges else z64.clone())

    def batch(self, keys: torch.Tensor, n_nodes=None, n_edges=None, pad_features: bool = True) -> EnclosingBatch:
        """``keys [B, 2]`` -> the ``EnclosingBatch`` of their B enclosing subgraphs.

        ``n_nodes`` / ``n_edges``: the batch's totals as ints, or the per-key host tensors ``sizes`` returned for exactly these keys
        (then ``GraphBatch.sizes`` is set and ``TopKPooling`` needs no read-back either).  With them nothing is read back and the
        call may run inside a stream capture.  The fill kernel compares them with the device's own totals: on a mismatch the batch
        holds placeholders only (node 0 / graph 0 rows, ``(-1, -1)`` columns, zero features) and a status bit is raised that the
        next device read of this package reports as a ``ValueError`` (``graph.check_pending``; at once under
        ``graph.set_debug(True)``).  A bad key (``u == v``, an id out of range) gives an empty sample and the same kind of error.
        ``pad_features``: as ``InteractionGraph.batch`` -- ``x`` with a row pitch of the next multiple of 128 and zero pad columns
        when that costs less than half as much again."""
        lib, dev, s = load(), self.device, self.side
        keys = self._keys(keys)
        B = int(keys.size(0))
        st = stream_ptr(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        status = torch.zeros(1, **i32)
        counts, node_off, edge_off, ws = self._sizes(keys, status)
        host_sizes = None
        if n_nodes is not None and n_edges is not None:
            if isinstance(n_nodes, torch.Tensor):
                if n_nodes.is_cuda or int(n_nodes.numel()) != B:
                    raise ValueError("EnclosingSubgraphs.batch: n_nodes must be an int or the HOST tensor of sizes() for these keys")
                host_sizes = n_nodes.to(torch.int64)
                n_nodes = int(host_sizes.sum())
            if isinstance(n_edges, torch.Tensor):
                n_edges = int(n_edges.sum())
            n, e = int(n_nodes), int(n_edges)
            known = True
        elif n_nodes is None and n_edges is None:
            n, e = (int(v) for v in torch.stack([node_off[-1], edge_off[-1]]).tolist())   # the one device read of the call
            known = False
            if n < 0:
                raise OverflowError("EnclosingSubgraphs.batch: the batch has more than 2^31 - 2 rows or edges; use fewer keys per call")
        else:
            raise ValueError("EnclosingSubgraphs.batch: pass both n_nodes and n_edges, or neither")
        if n < 0 or e < 0 or n >= 2 ** 31 - 1 or e >= 2 ** 31 - 1:
            raise OverflowError("EnclosingSubgraphs.batch: the batch has more than 2^31 - 2 rows or edges; use fewer keys per call")
        node_id = torch.empty(max(n, 1), **i32)
        bvec = torch.empty(max(n, 1), **i64)[:n]
        ei = torch.empty((2, max(e, 1)), **i64)[:, :e]
        e_id = torch.empty(max(e, 1), **i64)[:e]
        lrowptr, lcol = torch.empty(n + 1, **i32), torch.empty(max(e, 1), **i32)
        graph_ptr, edge_ptr = torch.empty(B + 1, **i32), torch.empty(B + 1, **i32)
        check(lib.npi_enclose_fill(ptr(s.rowptr), ptr(s.col), ptr(s.eid), ptr(self.mask), self.num_nodes, ptr(keys), B, self._flags,
                                   ptr(node_off), ptr(edge_off), ptr(ws), int(ws.numel()), ptr(node_id), bvec.data_ptr(),
                                   ei.data_ptr(), ei.data_ptr() + 8 * ei.stride(0), e_id.data_ptr(), ptr(lrowptr), ptr(lcol),
                                   ptr(graph_ptr), ptr(edge_ptr), n, e, ptr(status), st), "npi_enclose_fill")
        z = torch.empty(max(n, 1), **i64)[:n]
        dist = torch.empty((max(n, 1), 2), **i32)[:n]
        _label(lrowptr, lcol, n, e, None, None, graph_ptr, B, z, dist, dev)
        Ff = 0 if self.feat is None else int(self.feat.size(1))
        Fx = Ff + (0 if self.label is None else 1)
        ld = (Fx + 127) // 128 * 128
        if not pad_features or 2 * ld > 3 * Fx:
            ld = Fx
        full = torch.empty((n, ld), dtype=torch.float32, device=dev)
        if Fx > 0:
            check(lib.npi_enclose_features(ptr(self.feat), 0 if self.feat is None else self.feat.stride(0), Ff, ptr(node_id), z.data_ptr(),
                                           bvec.data_ptr(), ptr(node_off), ptr(edge_off), B, n, e, self._label_mode, full.data_ptr(),
                                           max(full.stride(0), Fx), st), "npi_enclose_features")
        _graph.note_status(status)                             # read now under set_debug, else at the next device read; never in a capture
        if not known:
            _graph.check_pending()                             # (this call has read from the device already)
        # the emitted entries are symmetric: the parent holds both directions, the mask and the target rule treat them alike
        gb = GraphBatch(full if ld == Fx else full[:, :Fx], ei, bvec, B, sizes=host_sizes, graph_ptr=graph_ptr, symmetric=True,
                        pad_base=None if ld == Fx else full)
        return EnclosingBatch(gb, node_id[:n].to(torch.int64), z, dist, e_id, graph_ptr, edge_ptr, lrowptr, lcol[:e])


def drnl_node_labeling(graph_or_edge_index: Union[CSRGraph, EnclosingBatch, torch.Tensor], src: torch.Tensor, dst: torch.Tensor,
                       graph_ptr: torch.Tensor, num_nodes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """DRNL labels of any batch of graphs -- Rule H 5, the label kernel alone: ``(z int64 [n], dist int32 [n, 2])``.

    ``graph_or_edge_index``: a ``CSRGraph`` over the batch's rows (its by-target side is walked; entries with source equal to target,
    such as its self loops, are skipped), an ``EnclosingBatch``, or an ``edge_index [2, E]`` tensor (a CSR is built; ``num_nodes``
    defaults to ``graph_ptr[-1]``, one device read).  ``src`` / ``dst [B]``: one target row id per graph; ``graph_ptr [B + 1]``: the
    graphs' first rows.  ``dist[:, 0]`` is the BFS distance from ``src`` with ``dst`` removed, ``dist[:, 1]`` from ``dst`` with ``src``
    removed (-1: unreachable, or the other target); ``z`` is SEAL's label, 1 for the targets and 0 where a distance is -1.  Rows
    outside every graph get ``z = 0`` and ``dist = -1``."""
    g = graph_or_edge_index
    dev = require_gpu(src, dst, graph_ptr)
    if isinstance(g, EnclosingBatch):
        rowptr, col, n = g.local_rowptr, g.local_col, int(g.z.numel())
    else:
        if not isinstance(g, CSRGraph):
            if num_nodes is None:
                num_nodes = int(graph_ptr[-1])
            g = CSRGraph(g, int(num_nodes), self_loops=False)
        rowptr, col, n = g.by_dst.rowptr, g.by_dst.col, g.num_nodes
    B = int(graph_ptr.numel()) - 1
    if int(src.numel()) != B or int(dst.numel()) != B:
        raise ValueError("drnl_node_labeling: src and dst hold one row id per graph")
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()            # noqa: E731
    z = torch.zeros(n, dtype=torch.int64, device=dev)
    dist = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
    if B > 0 and n > 0:
        _label(rowptr, col, n, int(col.numel()), i32(src), i32(dst), i32(graph_ptr), B, z, dist, dev)
    return z, dist
