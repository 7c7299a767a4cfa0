"""Device-resident adjacency for the conv hot path: destination-sorted CSR (+ its transpose).

Takes the ``edge_index`` LongTensor ``[2, E]`` exactly as PyG's ``Batch`` collate hands it to the
conv (row 0 = source j, row 1 = target i; reference ``src/classes.py:701-704`` emits both
directions) and builds, on the GPU, what PyG 1.4.2's ``add_remaining_self_loops`` + scatter would
produce implicitly.  A ``CSRGraph`` may be passed to the convs in place of ``edge_index`` so that a
static full-batch graph (BASELINE.json configs 3-5) is sorted once instead of once per layer call.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import check, load, ptr, require_gpu, stream_ptr

_DEBUG = False

# Status words of graph builds that nobody has looked at yet.  A build never synchronises, so an out-of-range node id
# (which the build DROPS, where PyG's index_select / scatter raise) is reported at the next point that reads from the
# device anyway: TopKPooling's size read, InteractionGraph.batch, CSRGraph.nnz(), the metrics read -- or after
# _PENDING_MAX unchecked builds (one extra device read per that many builds).  set_debug(True) checks every build at once.
_PENDING = []
_PENDING_MAX = 256


def set_debug(flag: bool) -> None:
    """When on, every graph build synchronises and raises on out-of-range node ids
    (PyG/torch raise IndexError/RuntimeError there)."""
    global _DEBUG
    _DEBUG = bool(flag)


def pending_status(device=None) -> list:
    """Device status words not yet checked (callers that are about to read from the device append them to their read and
    hand the values to ``raise_on_status``).  ``device``: only that GPU's words are taken; the others stay pending."""
    if device is None:
        out = list(_PENDING)
        _PENDING.clear()
        return out
    out = [t for t in _PENDING if t.device == device]
    _PENDING[:] = [t for t in _PENDING if t.device != device]
    return out


class BadSourceIdError(IndexError, ValueError):
    """A source id outside its table, reported by a status word: an ``IndexError`` to the samplers' callers (torch's indexing raises
    one there) and a ``ValueError`` to ``topk_links``' (a bad value in ``rows``)."""


def raise_on_status(values) -> None:
    if any(int(v) & 1 for v in values):
        raise IndexError("edge_index holds a node id outside [0, num_nodes): the edges were dropped by the graph build "
                         "(PyG's index_select / scatter raise here)")
    if any(int(v) & _lib.NPI_STATUS_BAD_ROW_ID for v in values):
        raise IndexError("res_n_id holds a row id outside [0, N_src): the row was gathered as zeros (npi_rows_gather; torch's "
                         "index_select raises here)")
    if any(int(v) & _lib.NPI_STATUS_BAD_TARGET_ID for v in values):
        raise IndexError("NeighborSampler: a target id outside [0, num_nodes): it was dropped (no entry sampled for it; "
                         "npi_sample_counts)")
    if any(int(v) & _lib.NPI_STATUS_BAD_SAMPLE_SIZES for v in values):
        raise ValueError("npi_sample_select / npi_sample_relabel: the offsets or counts they were given belong to another call; "
                         "the entries concerned were not written")
    if any(int(v) & _lib.NPI_STATUS_BAD_SOURCE_ID for v in values):
        raise BadSourceIdError("NegativeSampler.corrupt / RandomWalker.walks / topk_links: a source id outside [0, n_src): its slot "
                               "(its whole walk, its whole row of results) holds -1 (npi_negative_targets / npi_random_walk / "
                               "npi_topk_links)")
    if any(int(v) & _lib.NPI_STATUS_NO_NEGATIVE for v in values):
        raise ValueError("NegativeSampler.corrupt: a source found no non-edge target within its tries (it is joined to every "
                         "target, or tries ran out): its slot holds -1 (npi_negative_targets)")
    if any(int(v) & _lib.NPI_STATUS_WALK_TRIES for v in values):
        raise ValueError("RandomWalker.walks: a step had every one of its tries rejected and took the last candidate "
                         "(npi_random_walk): raise tries, or choose p and q less far apart")
    if any(int(v) & _lib.NPI_STATUS_BAD_PAIR_ID for v in values):
        raise IndexError("pair_scores / link_loss: a pair holds an id outside its embedding table: its logit, coefficient and loss "
                         "term are 0 (npi_pair_score; torch's indexing raises here) -- or EdgeSplitter / to_undirected: a column "
                         "holds an id outside its range: it was dropped (npi_split_permute / npi_split_undirected) -- or link_ranks: "
                         "a query pair holds an id outside its table: its counts are -1 (npi_link_ranks) -- or link_log_softmax / "
                         "listwise_loss: such a pair has lp = 0 and adds to no sum or gradient (npi_softmax_link_fwd)")
    if any(int(v) & _lib.NPI_STATUS_BAD_SCORE for v in values):
        raise ValueError("Input contains NaN: rank_metrics / roc_auc_score and their kin were given a NaN score; the metrics and "
                         "the curve of that call are undefined (npi_rank_metrics; sklearn raises here) -- or topk_links / link_ranks "
                         "met a NaN score: it was not returned or counted, a NaN target's counts are -1 (npi_topk_links / npi_link_ranks) "
                         "-- or link_log_softmax / listwise_loss met one among the candidates of a query: its lp is NaN "
                         "(npi_softmax_link_fwd)")
    if any(int(v) & _lib.NPI_STATUS_BAD_LABEL for v in values):
        raise ValueError("rank_metrics / roc_auc_score and their kin: a label other than 0 / 1; it counted as 0 "
                         "(npi_rank_metrics; sklearn's binary metrics raise here)")
    if any(int(v) & _lib.NPI_STATUS_BAD_ENCLOSE_KEY for v in values):
        raise ValueError("EnclosingSubgraphs: a key with u == v or an id outside [0, num_nodes): its sample is empty -- 0 nodes, 0 edges "
                         "(npi_enclose_sizes)")
    if any(int(v) & _lib.NPI_STATUS_BAD_ENCLOSE_TOTALS for v in values):
        raise ValueError("EnclosingSubgraphs.batch: the n_nodes / n_edges it was given do not belong to its keys (the device counted "
                         "other totals); that batch holds placeholders only (node 0 / graph 0 rows, (-1, -1) edges, zero features).  "
                         "Totals must come from sizes() of the same keys")
    if any(int(v) & 4 for v in values):
        raise ValueError("InteractionGraph.batch: the n_nodes / n_pairs it was given do not belong to its keys (the device counted "
                         "other totals); that batch holds placeholders only (node 0 / graph 0 rows, padding edges, zero features).  "
                         "Totals must come from sizes() of the same keys")


def note_status(status: torch.Tensor) -> None:
    """File a device status word: checked at once under ``set_debug(True)``, otherwise at the next device read of this package
    (or after ``_PENDING_MAX`` unchecked words); never during a HIP-graph capture."""
    if torch.cuda.is_current_stream_capturing():
        return                                # no reads inside a capture, and the word lives in the graph's pool
    if _DEBUG:
        raise_on_status([status.item()])
        return
    _PENDING.append(status)
    if len(_PENDING) > _PENDING_MAX:
        check_pending()


def check_pending() -> None:
    """Read and check every outstanding status word now (synchronises)."""
    st = pending_status()
    if st:
        by_dev = {}
        for t in st:
            by_dev.setdefault(t.device, []).append(t)
        for ts in by_dev.values():
            raise_on_status(torch.cat(ts).tolist())


#: aggregation scratch buffers kept per side (one per (width, stream) pair in use: launch stream, side stream, partial stream, a capture's)
CARRY_SLOTS = 6


@dataclass
class CSRSide:
    """One orientation.  ``rowptr[N+1]``, ``col/eid/rowidx[nnz_max]`` int32 in entry order;
    ``item_row`` maps every item of ``item`` entries (64 or 256: fixed when the side is built, and handed to every kernel that
    walks ``item_row`` -- no process-wide setting can change the meaning of an existing side) to its first row;
    ``rowptr[N]`` is nnz on device."""
    rowptr: torch.Tensor
    col: torch.Tensor
    eid: torch.Tensor
    rowidx: torch.Tensor
    item_row: torch.Tensor
    status: torch.Tensor
    nnz_max: int
    n_items: int
    _inv_cnt: Optional[torch.Tensor] = None
    _carry: Dict[tuple, torch.Tensor] = field(default_factory=dict)
    n_rows: int = -1          # output rows (key id space)
    n_cols: int = -1          # rows of the feature table the entries index (== n_rows unless sharded)
    item: int = 0             # entries per item this side was cut with
    _hub: Optional["HubPlan"] = None      # the streaming path for the heaviest rows (``hub_plan()``), None: none / not asked yet
    _hub_asked: bool = False
    rect_hub: bool = False    # a side of a BipartiteGraph: n_rows and n_cols are independent id spaces and the side may still get a hub plan

    def inv_count(self) -> torch.Tensor:
        """1 / max(row length, 1): the scatter_mean divisor (count includes the self loop)."""
        if self._inv_cnt is None:
            dev = self.rowptr.device
            out = torch.empty(self.n_rows, dtype=torch.float32, device=dev)
            check(load().npi_row_inv_count(ptr(self.rowptr), self.n_rows, ptr(out), stream_ptr(dev)),
                  "npi_row_inv_count")
            self._inv_cnt = out
        return self._inv_cnt

    def hub_plan(self) -> Optional["HubPlan"]:
        """The plan for aggregating this side's heaviest rows by streaming the table (``build_hub_plan``), made on first use and
        kept; None when the side has no such rows (then the plain launch is all there is).  One device read, once per side --
        so never inside a capture: a side first met there is walked the plain way until somebody asks again outside."""
        if not self._hub_asked:
            if (self.n_rows != self.n_cols and not self.rect_hub) or self.n_cols < HUB_MIN_COLS or self.nnz_max <= 0:
                self._hub_asked = True
            elif not torch.cuda.is_current_stream_capturing():
                self._hub = build_hub_plan(self)
                self._hub_asked = True
        return self._hub

    def carry(self, F: int) -> torch.Tensor:
        """f32 scratch of the aggregation launches (partial sums of rows cut by a workgroup boundary + their arrival
        counters); reused across calls of the same width ON THE SAME STREAM.  ZEROED once, here: every launch leaves its
        counters at zero again (``npi_segsum_carry_elems``).  One buffer per (side, width, current stream): launches of one
        stream are ordered, so they may share it; two modules that walk the same side at the same width on two streams
        (possibly concurrently) get a buffer each.  ``reset_carry()`` after a launch that did not run to its end."""
        dev = self.rowptr.device
        key = (F, _lib.stream_ptr(dev))
        buf = self._carry.pop(key, None)
        if buf is None:
            n = int(load().npi_segsum_carry_elems(self.nnz_max, self.item, F))
            buf = torch.zeros(n, dtype=torch.float32, device=dev)
            # at most CARRY_SLOTS buffers per side (at the C5 size one is ~200 MB): the least recently used one goes when a new
            # (width, stream) pair appears -- every fresh stream of a capture or a bench run used to leave its own behind for the
            # side's lifetime.  A dropped buffer was allocated and used on ITS stream only, so the caching allocator's stream-
            # ordered reuse keeps a launch that is still in flight on it safe; never during a capture (the graph owns its memory).
            if len(self._carry) >= CARRY_SLOTS and not torch.cuda.is_current_stream_capturing():
                self._carry.pop(next(iter(self._carry)))
        elif _DEBUG and not torch.cuda.is_current_stream_capturing():
            self._check_counters(buf)
        self._carry[key] = buf                              # (re-inserted: dicts keep insertion order, the first key is the LRU)
        return buf

    def _check_counters(self, buf: torch.Tensor) -> None:
        """``set_debug(True)``: the arrival counters at the head of ``buf`` must be zero between launches (synchronises)"""
        n_wg = -(-self.n_items // 4)
        n = n_wg + 2 * (-(-n_wg // 64))
        if n and int(buf[:n].view(torch.int32).abs().max()) != 0:
            raise _lib.NpiError("aggregation scratch: an arrival counter is not zero between launches -- two launches shared the "
                                "buffer concurrently or one was aborted; call reset_carry() on this side")

    def reset_carry(self) -> None:
        """Drop every scratch buffer of this side (after an aborted launch or a failed ``check()``): the next launch of each
        (width, stream) gets a freshly zeroed one."""
        self._carry.clear()


#: A side gets a hub plan only when its table is larger than the 256 MB Infinity Cache (262,144 rows of 256 f32): a smaller table
#: is gathered from cache, and streaming it saves no HBM traffic.  Every small batched configuration stops here, at no cost.
HUB_MIN_COLS = 262_144
#: A row qualifies as a hub from ``n_cols / HUB_DEGREE_DIV`` entries on.  In bytes any row pays once the table is streamed anyway
#: (its bit rides in a mask word that is read regardless); the bound keeps the candidates few and the rows long enough that the
#: scalar mask test per (source row, hub) stays small beside the row's 1 KiB.
HUB_DEGREE_DIV = 512
#: ... and the plan is empty unless the hubs' entries together are at least this many times the rows that have to be streamed:
#: 1 is break-even in bytes (entries x 1 KiB gathered against n_cols x 1 KiB streamed); the second launch, its tail and the
#: partial sums have to be paid for as well.
HUB_ENTRIES_PER_STREAMED_ROW = 2


@dataclass
class HubPlan:
    """The heaviest rows of one ``CSRSide`` and what the streaming aggregation needs (``npi_hub_plan`` / ``npi_segsum_hub``):
    ``hub_rows[NPI_HUB_MAX]`` int32 (the first ``H`` valid, by descending degree), ``mask[n_cols, NPI_HUB_MAX / 32]`` (bit j of
    source row r: the side has an entry (hub j, r)), and ``light``: the same side with the hub rows empty."""
    H: int
    n_entries: int                     # entries of the hub rows (what the light side no longer holds)
    hub_rows: torch.Tensor
    mask: torch.Tensor
    light: CSRSide
    _partial: Dict[int, torch.Tensor] = field(default_factory=dict)

    def partial(self) -> torch.Tensor:
        """scratch of the streaming launch (one partial sum per slab and hub), by the rules of ``CSRSide.carry``: one buffer per
        stream in use, the least recently used one dropped beyond ``CARRY_SLOTS`` -- never during a capture, whose graph replays
        the launch on the buffer it saw.  Needs no clearing."""
        dev = self.mask.device
        key = _lib.stream_ptr(dev)
        buf = self._partial.pop(key, None)
        if buf is None:
            buf = torch.empty(int(load().npi_segsum_hub_partial_elems(self.mask.size(0))), dtype=torch.float32, device=dev)
            if len(self._partial) >= CARRY_SLOTS and not torch.cuda.is_current_stream_capturing():
                self._partial.pop(next(iter(self._partial)))
        self._partial[key] = buf
        return buf


def build_hub_plan(side: CSRSide, h_max: int = _lib.NPI_HUB_MAX, min_degree: Optional[int] = None,
                   min_entries: Optional[int] = None) -> Optional[HubPlan]:
    """``npi_hub_plan`` + ``npi_hub_light_side`` for one side (a one-table side, ``n_cols == n_rows``, or a side of a
    ``BipartiteGraph``, whose thresholds then follow ``n_cols``: the rows of the table that would be streamed); None when the plan comes
    out empty.  Reads four words back from the device.  ``min_degree`` / ``min_entries``: the two thresholds (defaults: the
    module's policy, ``HUB_DEGREE_DIV`` / ``HUB_ENTRIES_PER_STREAMED_ROW``)."""
    if side.n_rows != side.n_cols and not side.rect_hub:
        raise ValueError("build_hub_plan: one-table sides with n_cols == n_rows, or the sides of a BipartiteGraph, only")
    lib = load()
    dev = side.rowptr.device
    N = side.n_rows
    if N <= 0 or side.nnz_max <= 0:
        return None
    if min_degree is None:
        min_degree = max(-(-side.n_cols // HUB_DEGREE_DIV), 2)
    if min_entries is None:
        min_entries = HUB_ENTRIES_PER_STREAMED_ROW * side.n_cols
    i32 = dict(dtype=torch.int32, device=dev)
    hub_rows = torch.empty(_lib.NPI_HUB_MAX, **i32)
    mask = torch.empty((side.n_cols, _lib.NPI_HUB_MAX // 32), **i32)
    info = torch.empty(4, **i32)
    ws = torch.empty(int(lib.npi_hub_plan_workspace_elems()), **i32)
    s = stream_ptr(dev)
    check(lib.npi_hub_plan(ptr(side.rowptr), ptr(side.col), N, side.n_cols, side.nnz_max, int(h_max), int(min_degree), int(min_entries),
                           ptr(hub_rows), ptr(mask), ptr(info), ptr(ws), s), "npi_hub_plan")
    H, n_entries = info.tolist()[:2]
    if H == 0:
        return None
    nnz_max = side.nnz_max - n_entries
    n_items = int(lib.npi_num_items(nnz_max, side.item))
    rowptr = torch.empty(N + 1, **i32)
    col = torch.empty(max(nnz_max, 1), **i32)
    eid = torch.empty(max(nnz_max, 1), **i32)
    rowidx = torch.empty(max(nnz_max, 1), **i32)
    item_row = torch.empty(n_items + 1, **i32)
    check(lib.npi_hub_light_side(ptr(side.rowptr), ptr(side.col), ptr(side.eid), ptr(side.rowidx), N, side.nnz_max, ptr(hub_rows), H,
                                 nnz_max, side.item, ptr(rowptr), ptr(col), ptr(eid), ptr(rowidx), ptr(item_row), s),
          "npi_hub_light_side")
    light = CSRSide(rowptr, col, eid, rowidx, item_row, side.status, nnz_max, n_items)
    light.n_rows, light.n_cols, light.item, light.rect_hub = N, side.n_cols, side.item, side.rect_hub
    light._hub_asked = True                                   # (the light side has no plan of its own)
    return HubPlan(H, n_entries, hub_rows, mask, light)


def item_hint(nnz_max: int) -> int:
    """Recommended item size for a new CSR of this capacity (``npi_item_edges``, a pure function: 64 below 2^22 entries, else
    256).  Asked ONCE, when a side is built without ``item=``; the side then carries its own value.  Neither the library nor this
    module keeps a threshold that could move (``CSRGraph(item=)`` / ``build_side(item=)`` name another size explicitly)."""
    return int(load().npi_item_edges(int(nnz_max)))


def build_side(key: torch.Tensor, val: torch.Tensor, n_rows: int, n_cols: int, self_loops: bool = True,
               loop_col_offset: int = 0, drop_equal: bool = True, item: Optional[int] = None,
               sort_columns: bool = False) -> CSRSide:
    """CSR over ``n_rows`` key rows whose entries index a table of ``n_cols`` rows
    (``npi_csr_build_ex``); with ``n_cols == n_rows`` and the defaults this is the plain build.  ``item``: entries per
    item (64 or 256; default: ``item_hint``).  ``sort_columns``: a row's entries ordered by column instead of list order
    (``NPI_CSR_SORT_COLUMNS``; the appended self loop stays last)."""
    lib = load()
    dev = require_gpu(key, val)
    E, N = int(key.numel()), int(n_rows)
    nnz_max = E + (N if self_loops else 0)
    item = item_hint(nnz_max) if item is None else int(item)
    n_items = int(lib.npi_num_items(nnz_max, item))
    if n_items < 0:
        raise ValueError(f"build_side: item must be 64 or 256 (got {item})")
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr = torch.empty(N + 1, **i32)
    col = torch.empty(max(nnz_max, 1), **i32)
    eid = torch.empty(max(nnz_max, 1), **i32)
    rowidx = torch.empty(max(nnz_max, 1), **i32)
    item_row = torch.empty(n_items + 1, **i32)
    status = torch.empty(1, **i32)
    ws_bytes = int(lib.npi_csr_workspace_bytes(E, N))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib.npi_csr_build_ex(ptr(key), ptr(val), E, N, int(n_cols), 1 if self_loops else 0,
                               int(loop_col_offset), (1 if drop_equal else 0) | (2 if sort_columns else 0), ptr(rowptr), ptr(col), ptr(eid),
                               ptr(rowidx), ptr(item_row), item, ptr(status), ptr(ws), ws_bytes, stream_ptr(dev)),
          "npi_csr_build_ex")
    note_status(status)
    side = CSRSide(rowptr, col, eid, rowidx, item_row, status, nnz_max, n_items)
    side.n_rows, side.n_cols, side.item = N, int(n_cols), item
    return side


class CSRGraph:
    """Self-loop-augmented adjacency of one (batched) graph on one GPU.

    ``by_dst`` groups entries by target node (forward aggregation, PyG flow ``source_to_target``);
    ``by_src`` groups them by source node (backward: dX = A^T ...), built lazily."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, self_loops: bool = True, by_dst: Optional[CSRSide] = None,
                 symmetric: bool = False, item: Optional[int] = None, sort_columns: bool = False, keep_equal: bool = False,
                 hub_stream: bool = True):
        """``item``: entries per item of both sides (64 or 256; default: the hint for this capacity, ``item_hint``).
        ``sort_columns``: both sides with every row's entries in column order (a second key for the build's sort: at 4M nodes /
        100M edges 3 ms more per side, once, for 1.2 % of every GATConv layer step and 0.6 % of every SAGEConv one -- the
        4-byte gathers of per-node scalars walk ascending addresses; EXPERIMENTS A22).  The sums are the same in another order.
        ``self_loops=False, keep_equal=True``: the edge list exactly as it is -- no loop appended, existing ``(i, i)`` columns kept
        as ordinary entries (what PyG's ``SAGEConv(concat=True)`` aggregates over; the default drops them first, as
        ``add_remaining_self_loops`` does).
        ``hub_stream``: SAGEConv (f32, 256 features, no edge weights) aggregates the heaviest rows of a side that has a hub plan
        (``CSRSide.hub_plan``) by streaming the table once (``npi_segsum_hub``) beside the plain launch over the rest; False: the
        plain launch alone, as for a side without such rows.  A plain attribute: both paths can be run over one graph and compared.
        ``by_dst``: a by-target side somebody already derived for this very edge list (``filtered_side``): not rebuilt.
        ``symmetric``: the producer of the edge list vouches that it holds every edge in both directions (the device-side
        subgraph extraction emits both, src/classes.py:701-704, and filter_adj keeps the property; ``GraphBatch.symmetric``).
        Then row j of the by-source CSR holds the same neighbours as row j of the by-target CSR -- in another order -- and an
        UNWEIGHTED transposed aggregation can walk the by-target side: no second sort (functional._AggProjectFn)."""
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError("edge_index must be a LongTensor of shape [2, E]")
        require_gpu(edge_index)
        self.num_nodes = int(num_nodes)
        self.num_edges = int(edge_index.size(1))
        self.self_loops = bool(self_loops)
        self.device = edge_index.device
        # what this CSR was built from: a GraphBatch reuses it only for THIS tensor in THIS state (an in-place edit of the
        # edge list bumps ``_version`` and the next conv call sorts again -- ``built_from``)
        self._ei_version = edge_index._version
        self._ei_ptr = edge_index.data_ptr()
        self.symmetric = bool(symmetric)
        # rows of a [2,E] tensor are contiguous when the tensor is; otherwise copy (index plumbing)
        self._src = edge_index[0].contiguous()
        self._dst = edge_index[1].contiguous()
        self._item = item if by_dst is None else by_dst.item
        self.sort_columns = bool(sort_columns)
        self.keep_equal = bool(keep_equal)
        self.hub_stream = bool(hub_stream)
        if self.keep_equal and self.self_loops:
            raise ValueError("CSRGraph: keep_equal=True (existing self loops stay ordinary entries) needs self_loops=False")
        self.by_dst = by_dst if by_dst is not None else \
            build_side(self._dst, self._src, self.num_nodes, self.num_nodes, self.self_loops, drop_equal=not self.keep_equal,
                       item=self._item, sort_columns=self.sort_columns)
        self._by_src: Optional[CSRSide] = None
        self.dropped_from: Optional["CSRGraph"] = None      # the graph whose edges ``drop_edges`` dropped to make this one

    @property
    def by_src(self) -> CSRSide:
        if self._by_src is None:
            self._by_src = build_side(self._src, self._dst, self.num_nodes, self.num_nodes, self.self_loops,
                                      drop_equal=not self.keep_equal, item=self.by_dst.item, sort_columns=self.sort_columns)
        return self._by_src

    def drop_edges(self, p: float, seed: int = 0, draw: int = 0, tick: Optional[torch.Tensor] = None, undirected: bool = False,
                   training: bool = True, out: Optional["CSRGraph"] = None) -> "CSRGraph":
        """DropEdge (PyG's ``dropout_adj`` in front of a conv) WITHOUT a sort: a new ``CSRGraph`` over the same ``edge_index`` whose two
        sides are this graph's with the dropped entries removed (``npi_csr_drop_side``, Rule E of ``include/npi_gnn.h``: column e is
        dropped iff a word that is a pure function of ``(seed, draw, tick, e)`` lies below ``floor(p 2^64)``).  The kept entries keep
        their order and THIS graph's column numbers, so an ``[E]``-long ``edge_weight`` still lines up (the gradient w.r.t. a dropped
        edge's weight is 0), ``segmax``'s ``arg`` names the same columns and a GATConv's Rule D mask of an edge is unchanged.  Nothing
        is read back; both sides keep this graph's capacity and item size and never get a hub plan.

        ``p`` in ``[0, 1)`` (PyG's ``p = 1`` is refused); ``p == 0`` or ``training=False``: this graph itself.  ``tick``: None, or a
        one-element int64 DEVICE tensor the kernels read -- a captured step draws a new mask per replay by counting it up.
        ``undirected``: the rule is keyed on the column's unordered pair of ends, so ``(u, v)``, ``(v, u)`` and parallel duplicates
        go together; ``symmetric`` stays True only then.  ``out``: a graph an earlier ``drop_edges`` of this very graph returned --
        its arrays are reused and what was derived from them is dropped.  Existing ``(i, i)`` columns have no entry on either side
        (the build drops them), so they are not subject to DropEdge: their weight remains the node's loop weight."""
        from .dropedge import drop_edges_csr
        return drop_edges_csr(self, p, seed, draw, tick, undirected, training, out)

    def built_from(self, edge_index: torch.Tensor, num_nodes: Optional[int] = None) -> bool:
        """True while ``edge_index`` is still the tensor this CSR was built from: same storage, same shape and, above all,
        the same ``_version`` (every in-place write bumps it)."""
        return (self.num_edges == edge_index.size(1) and self._ei_version == edge_index._version
                and self._ei_ptr == edge_index.data_ptr() and (num_nodes is None or self.num_nodes == int(num_nodes)))

    def inv_count(self, side: CSRSide) -> torch.Tensor:
        return side.inv_count()

    def carry(self, side: CSRSide, F: int) -> torch.Tensor:
        return side.carry(F)

    def nnz(self) -> int:
        """Entries incl. self loops (device read; synchronises -- and reports dropped out-of-range ids)."""
        n = int(self.by_dst.rowptr[-1].item())
        check_pending()
        return n


class BipartiteGraph:
    """Adjacency between TWO id spaces on one GPU: ``edge_index[0]`` indexes a source table of ``size[0]`` rows, ``edge_index[1]``
    the ``size[1]`` target rows (PyG 1.4.2 ``MessagePassing.propagate(edge_index, size=(N_src, N_dst))``, flow ``source_to_target``)
    -- what ``SAGEConv`` / ``GATConv`` aggregate over when ``x`` is a pair ``(x_src, x_dst)``.  The edge list as it is: no self loop
    is added or removed (a ``(k, k)`` column is an ordinary edge from source k to target k); out-of-range and ``(-1, -1)`` columns
    are dropped and reported exactly as by ``CSRGraph`` (``note_status``).

    ``by_dst`` groups the entries by target (``n_rows = N_dst`` over a table of ``n_cols = N_src`` rows: the forward aggregation),
    ``by_src`` -- built lazily -- by source (the transposed aggregation of the backward).  ``item`` / ``sort_columns``: as
    ``CSRGraph``.  ``hub_stream``: the heaviest rows of a side whose TABLE is larger than the Infinity Cache (``HUB_MIN_COLS`` and
    the degree / entry thresholds apply to ``n_cols``) are aggregated by streaming that table (``CSRSide.hub_plan``)."""

    def __init__(self, edge_index: torch.Tensor, size, item: Optional[int] = None, sort_columns: bool = False, hub_stream: bool = True):
        if not isinstance(edge_index, torch.Tensor) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError("edge_index must be a LongTensor of shape [2, E]")
        if not isinstance(size, (tuple, list)) or len(size) != 2 or size[0] is None or size[1] is None or int(size[0]) < 0 or int(size[1]) < 0:
            raise ValueError("BipartiteGraph: size must be (N_src, N_dst)")
        require_gpu(edge_index)
        self.size = (int(size[0]), int(size[1]))
        self.num_src, self.num_dst = self.size
        self.num_edges = int(edge_index.size(1))
        self.self_loops = False                 # (never appended: the layers' helpers ask)
        self.symmetric = False
        self.device = edge_index.device
        self._ei_version = edge_index._version
        self._ei_ptr = edge_index.data_ptr()
        self._src = edge_index[0].contiguous()
        self._dst = edge_index[1].contiguous()
        self.sort_columns = bool(sort_columns)
        self.hub_stream = bool(hub_stream)
        self.by_dst = build_side(self._dst, self._src, self.num_dst, self.num_src, self_loops=False, drop_equal=False, item=item,
                                 sort_columns=self.sort_columns)
        self.by_dst.rect_hub = True
        self._by_src: Optional[CSRSide] = None
        self._root = None                       # (res_n_id storage, _version, shape) -> the combined by-source side (root_side)
        self._pair = None                       # the one-id-space side of the list read as pairs (pair_side)
        self.dropped_from: Optional["BipartiteGraph"] = None     # the graph whose edges ``drop_edges`` dropped to make this one

    def drop_edges(self, p: float, seed: int = 0, draw: int = 0, tick: Optional[torch.Tensor] = None, undirected: bool = False,
                   training: bool = True, out: Optional["BipartiteGraph"] = None) -> "BipartiteGraph":
        """``CSRGraph.drop_edges`` for two id spaces (directed mode only: ``undirected=True`` is a ``ValueError``).  ``root_side`` of
        the result is the drop of this graph's ``root_side`` -- the root entries are never dropped --, its ``pair_side`` raises."""
        from .dropedge import drop_edges_bipartite
        return drop_edges_bipartite(self, p, seed, draw, tick, undirected, training, out)

    @property
    def by_src(self) -> CSRSide:
        if self._by_src is None:
            self._by_src = build_side(self._src, self._dst, self.num_src, self.num_dst, self_loops=False, drop_equal=False,
                                      item=self.by_dst.item, sort_columns=self.sort_columns)
            self._by_src.rect_hub = True
        return self._by_src

    def built_from(self, edge_index: torch.Tensor, size=None) -> bool:
        """True while ``edge_index`` is still the tensor this structure was built from (storage, shape, ``_version``) -- and
        ``size``, when given, is its size."""
        return (self.num_edges == edge_index.size(1) and self._ei_version == edge_index._version
                and self._ei_ptr == edge_index.data_ptr() and (size is None or (int(size[0]), int(size[1])) == self.size))

    def inv_count(self, side: Optional[CSRSide] = None) -> torch.Tensor:
        """1 / max(in-edge count, 1) per TARGET (``by_dst``; another side: its rows')"""
        return (self.by_dst if side is None else side).inv_count()

    def carry(self, side: CSRSide, F: int) -> torch.Tensor:
        return side.carry(F)

    def root_side(self, res_n_id: torch.Tensor) -> CSRSide:
        """The by-source side of the backward of ``SAGEConv(concat=True)``: the entries of ``by_src`` over the two-part table
        ``[dAgg ; dRoot]`` (``N_dst`` rows each) plus ONE entry ``(res_n_id[i], N_dst + i)`` per target i -- the root term
        ``x_src[res_n_id]`` of the forward, so that ``dX_src`` is one deterministic segmented sum (duplicates in ``res_n_id``
        accumulate; no float atomics).  Kept for as long as ``res_n_id`` is the same tensor in the same state.  ``eid``: the edge's
        column for an edge entry, ``num_edges + i`` for the root entry of target i."""
        key = (res_n_id.data_ptr(), res_n_id._version, tuple(res_n_id.shape))
        if self._root is None or self._root[0] != key:
            nd = self.num_dst
            keys = torch.cat([self._src, res_n_id.reshape(-1)])
            vals = torch.cat([self._dst, torch.arange(nd, 2 * nd, dtype=torch.int64, device=self.device)])
            side = build_side(keys, vals, self.num_src, 2 * nd, self_loops=False, drop_equal=False, item=self.by_dst.item,
                              sort_columns=self.sort_columns)
            self._root = (key, side, res_n_id)            # (the tensor is held: its storage cannot be reused under the key)
        return self._root[1]

    def pair_side(self) -> CSRSide:
        """The list read as PAIRS over ONE id space (``size = (N, N)``): the side of ``pair_list_side`` -- both ends of every pair
        as keys -- built on first use and kept (the backward of ``functional.pair_scores`` / ``link_loss`` with one table)."""
        if self._pair is None:
            if self.num_src != self.num_dst:
                raise ValueError(f"BipartiteGraph.pair_side: one id space needs size (N, N), this graph has {self.size}")
            self._pair = pair_list_side(self._src, self._dst, self.num_src, item=self.by_dst.item)
        return self._pair

    def nnz(self) -> int:
        """Entries (device read; synchronises -- and reports dropped out-of-range ids)."""
        n = int(self.by_dst.rowptr[-1].item())
        check_pending()
        return n


def pair_list_side(src: torch.Tensor, dst: torch.Tensor, num_nodes: int, item: Optional[int] = None) -> CSRSide:
    """The side over which ``dZ[v] = sum_{m: src_m = v} g_m z[dst_m] + sum_{m: dst_m = v} g_m z[src_m]`` -- the gradient of pair
    scores ``<z[src_m], z[dst_m]>`` taken from ONE table -- is a single deterministic segmented sum: keys ``cat(src, dst)``, values
    ``cat(dst, src)`` (``BipartiteGraph.root_side`` is the precedent for a concatenated side).  ``eid``: ``m`` for the entry that
    pair m files under its source, ``M + m`` for the one under its target, so the per-entry weights come from ``cat(g, g)``."""
    return build_side(torch.cat([src, dst]), torch.cat([dst, src]), num_nodes, num_nodes, self_loops=False, drop_equal=False, item=item)


@dataclass
class CSRRecipe:
    """How to obtain the by-target CSR of the graph a pooling layer leaves WITHOUT sorting: the parent's side filtered by the
    kept nodes (``filtered_side``).  Made by ``pool.topk_pool``, consumed -- at most once, and only if a conv asks -- by
    ``GraphBatch.graph``."""
    parent: CSRSide
    perm: torch.Tensor            # int32 [n_out]  new -> old node id
    remap: torch.Tensor           # int32 [N]      old -> new node id or -1
    newpos: torch.Tensor          # int32 [E]      where filter_adj put every input edge
    n_out: int
    num_edges_out: int
    ei_version: int               # ``edge_index._version`` of the pooled edge list when the recipe was written


class GraphBatch:
    """One batch of graphs as the layers of ``Net_1`` hand it to one another: the node features
    and everything this package knows about the structure they live on, in ONE explicit object -- nothing rides on tensor
    attributes.  ``SAGEConv`` / ``GCNConv`` / ``GATConv`` map a ``GraphBatch`` to a ``GraphBatch`` (new ``x``, same structure),
    ``TopKPooling`` to the pooled one, ``global_max_mean_pool`` reads its segments.  The layers still take PyG's plain
    ``(x, edge_index[, batch])`` tensors; what they then cannot know is exactly the optional part below.

    x           [n, F] float32 node features
    edge_index  [2, E] int64, PyG layout (row 0 = source, row 1 = target); may end in (-1, -1) padding columns when it comes
                from ``TopKPooling(padded_edges=True)`` -- every consumer in this package drops them
    batch       [n] int64 graph id per node, non-decreasing (None: one graph)
    num_graphs  B (None: read from ``batch`` when needed)
    sizes       host LongTensor [B], nodes per graph, when known WITHOUT a device read (``net1.KeyLoader``: a sample's
                size depends on its key only; a pooling layer: ceil(ratio n_g)) -- lets TopKPooling run without a read-back
    graph_ptr   device int32 [B+1] segment starts of ``batch`` (``segment_ptr()`` builds them on first use)
    symmetric   the edge list holds every edge in both directions (``CSRGraph.symmetric``)
    pad_base    ``x`` is the leading columns of this wider buffer whose other columns are zero (``InteractionGraph.batch``:
                178 -> 256): the first conv runs its GEMMs on the padded width
    The CSR of ``edge_index`` is built by ``graph()`` on first use and kept for as long as the tensor is unchanged
    (``CSRGraph.built_from``: storage, shape and ``_version``); a pooled batch may carry a ``CSRRecipe`` instead."""

    __slots__ = ("x", "edge_index", "batch", "num_graphs", "sizes", "graph_ptr", "symmetric", "pad_base", "_csr", "_recipe")

    def __init__(self, x: torch.Tensor, edge_index: torch.Tensor, batch: Optional[torch.Tensor] = None,
                 num_graphs: Optional[int] = None, *, sizes: Optional[torch.Tensor] = None,
                 graph_ptr: Optional[torch.Tensor] = None, symmetric: bool = False, pad_base: Optional[torch.Tensor] = None,
                 csr: Optional[CSRGraph] = None, recipe: Optional[CSRRecipe] = None):
        if isinstance(edge_index, CSRGraph):
            raise TypeError("GraphBatch: edge_index is the [2, E] tensor; pass a prebuilt CSRGraph as csr=")
        self.x, self.edge_index, self.batch = x, edge_index, batch
        if num_graphs is None and sizes is not None:
            num_graphs = int(sizes.numel())
        if num_graphs is None and graph_ptr is not None:
            num_graphs = int(graph_ptr.numel()) - 1
        if num_graphs is None and batch is None:
            num_graphs = 1
        self.num_graphs = None if num_graphs is None else int(num_graphs)
        if sizes is not None and self.num_graphs is not None and int(sizes.numel()) != self.num_graphs:
            raise ValueError(f"GraphBatch: sizes has {int(sizes.numel())} entries for {self.num_graphs} graphs")
        self.sizes, self.graph_ptr = sizes, graph_ptr
        self.symmetric, self.pad_base = bool(symmetric), pad_base
        self._csr, self._recipe = csr, recipe

    # ---- unpacking as PyG's (x, edge_index, batch) ----------------------------------------------------------------------------
    def __iter__(self):
        return iter((self.x, self.edge_index, self.batch))

    @property
    def num_nodes(self) -> int:
        return int(self.x.size(0))

    def to(self, device):
        """The reference's ``data = data.to(device)`` (src/train_with_twoDataset.PY:50).  Batches of this package are born on
        the device (``InteractionGraph.batch``): then this is the object itself.  Otherwise the tensors are moved; what was
        built for the old device (CSR, recipe, padded buffer) is dropped, the host-side knowledge (``sizes``) stays."""
        device = torch.device(device) if device is not None else self.x.device
        if device.type == "cuda" and device.index is None and self.x.is_cuda:
            device = self.x.device
        if device == self.x.device:
            return self
        mv = lambda t: None if t is None else t.to(device)                      # noqa: E731
        other = object.__new__(type(self))
        GraphBatch.__init__(other, mv(self.x), mv(self.edge_index), mv(self.batch), self.num_graphs, sizes=self.sizes,
                            graph_ptr=mv(self.graph_ptr), symmetric=self.symmetric)
        for klass in type(self).__mro__:                                       # subclasses' own fields (net1.Batch.y)
            for name in getattr(klass, "__slots__", ()):
                if name not in GraphBatch.__slots__ and hasattr(self, name):
                    v = getattr(self, name)
                    setattr(other, name, v.to(device) if isinstance(v, torch.Tensor) else v)
        return other

    def with_x(self, x: torch.Tensor) -> "GraphBatch":
        """The same graphs with other node features (what a conv returns); the structure, incl. a CSR already built, is shared."""
        return GraphBatch(x, self.edge_index, self.batch, self.num_graphs, sizes=self.sizes, graph_ptr=self.graph_ptr,
                          symmetric=self.symmetric, pad_base=None, csr=self._csr, recipe=self._recipe)

    # ---- structure, built on demand ------------------------------------------------------------------------------------------------
    def peek_graph(self) -> Optional[CSRGraph]:
        """The CSR if one was built AND ``edge_index`` has not been written to since; never builds."""
        g = self._csr
        if g is not None and g.built_from(self.edge_index, self.num_nodes):
            return g
        return None

    def graph(self) -> CSRGraph:
        """CSR of ``edge_index`` (+ self loops).  Reused while the edge list is untouched; an in-place edit (``_version``)
        makes the next call sort again, so a stale adjacency is never served."""
        g = self.peek_graph()
        if g is not None:
            return g
        n, ei = self.num_nodes, self.edge_index
        r, self._recipe = self._recipe, None                   # consumed either way: the parent's arrays are not kept alive
        g = None
        if r is not None and r.ei_version == ei._version and r.n_out == n and r.num_edges_out == ei.size(1):
            side = filtered_side(r.parent, r.perm, r.remap, r.newpos, r.n_out, r.num_edges_out)
            if side is not None:
                g = CSRGraph(ei, n, by_dst=side, symmetric=self.symmetric)
        if g is None:
            g = CSRGraph(ei, n, symmetric=self.symmetric)
        self._csr = g
        return g

    def segment_ptr(self) -> torch.Tensor:
        """int32 ``[B+1]`` segment starts of ``batch`` on the device (kept)."""
        if self.graph_ptr is None:
            dev = self.x.device
            if self.batch is None:
                self.graph_ptr = torch.tensor([0, self.num_nodes], dtype=torch.int32, device=dev)
            else:
                from .pool import graph_ptr as _graph_ptr
                self.graph_ptr = _graph_ptr(self.batch, self.num_graphs)
            if self.num_graphs is None:
                self.num_graphs = int(self.graph_ptr.numel()) - 1
        return self.graph_ptr

    def batch_vector(self) -> torch.Tensor:
        if self.batch is None:
            self.batch = torch.zeros(self.num_nodes, dtype=torch.int64, device=self.x.device)
        return self.batch

    def __repr__(self):
        return (f"GraphBatch(nodes={self.num_nodes}, edges={int(self.edge_index.size(1))}, graphs={self.num_graphs}, "
                f"F={int(self.x.size(1)) if self.x.dim() == 2 else '?'})")


def as_graph(edge_index_or_graph, num_nodes: int) -> CSRGraph:
    """What the convs aggregate over: a prebuilt ``CSRGraph``, a ``GraphBatch`` (its cached / derived CSR) or a plain
    ``edge_index`` tensor (sorted here, every call: a tensor carries no state)."""
    if isinstance(edge_index_or_graph, GraphBatch):
        edge_index_or_graph = edge_index_or_graph.graph()
    if isinstance(edge_index_or_graph, CSRGraph):
        g = edge_index_or_graph
        if g.num_nodes != num_nodes:
            raise ValueError(f"CSRGraph was built for {g.num_nodes} nodes, x has {num_nodes}")
        return g
    return CSRGraph(edge_index_or_graph, num_nodes)


def filtered_side(parent: CSRSide, perm: torch.Tensor, remap: torch.Tensor, newpos: torch.Tensor, n_out: int,
                  num_edges_out: int) -> Optional[CSRSide]:
    """By-target side of the graph TopKPooling leaves -- nodes ``perm`` (int32, new -> old) of the parent, renumbered by
    ``remap``, edges filtered in order (``newpos``: where ``npi_filter_adj`` put every input edge) -- derived from the
    parent's side without a sort (``npi_csr_filter``: three launches).  Identical to ``build_side`` on the filtered edge list of length
    ``num_edges_out`` (the padded length when the list is padded).  None when the shape is outside the kernel's range."""
    lib = load()
    dev = parent.rowptr.device
    n_out = int(n_out)
    if n_out > int(lib.npi_csr_filter_max_rows()) or parent.n_rows != parent.n_cols:
        return None
    nnz_max = int(num_edges_out) + n_out
    item = item_hint(nnz_max)
    n_items = int(lib.npi_num_items(nnz_max, item))
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr = torch.empty(n_out + 1, **i32)
    col = torch.empty(max(nnz_max, 1), **i32)
    eid = torch.empty(max(nnz_max, 1), **i32)
    rowidx = torch.empty(max(nnz_max, 1), **i32)
    item_row = torch.empty(n_items + 1, **i32)
    status = torch.empty(1, **i32)
    ws = torch.empty(int(lib.npi_csr_filter_workspace_elems(n_out)), **i32)
    check(lib.npi_csr_filter(ptr(parent.rowptr), ptr(parent.col), ptr(parent.eid), ptr(perm), ptr(remap), ptr(newpos), n_out,
                             nnz_max, ptr(rowptr), ptr(col), ptr(eid), ptr(rowidx), ptr(item_row), item, ptr(status), ptr(ws),
                             stream_ptr(dev)), "npi_csr_filter")
    side = CSRSide(rowptr, col, eid, rowidx, item_row, status, nnz_max, n_items)
    side.n_rows = side.n_cols = n_out
    side.item = item
    return side
