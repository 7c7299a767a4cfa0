#!/usr/bin/env python3
"""Timings of ``npi.NeighborSampler`` on one MI355X (EXPERIMENTS.md): one epoch-shaped run on the benchmark's synthetic C4 graph
(``npi_gnn_amd/synth.py``: 1M nodes, 20M directed edges, Zipf hubs), 1024 targets per batch, ``size=[25, 10]``, two hops,
``add_self_loops=True``, 100 batches after a warm-up.

Per batch it reports the device time of each entry point (HIP events around the call, summed over the two hops: counts, select,
relabel = relabel_count + relabel) and the wall time of the whole ``DataFlow`` (host clock around ``sampler.sample`` ending in a
synchronise: it includes the host reads that size the tensors).

Beside it: the numpy restatement of the sampling rule of ``include/npi_gnn.h`` on the first ``--numpy-batches`` of the same batches
(host, one Python iteration per target; its blocks are compared with the device's while it is at it).  There is NO torch-ops
composition on the GPU to put beside it: a draw without replacement per row needs a ``randperm`` per row, which torch does not
have -- the numpy figure is the comparison.

``--subgraph``: the one-id-space flow instead (``sampler.sample_subgraph``), same graph, batches and sizes.  Per batch: the device
time of ``npi_sample_union`` and ``npi_sample_coalesce`` (HIP events around each call), the wall time of the stage
``union_subgraph`` (both calls, the host read of the two sizes and the trim; ending in a synchronise) and of the whole
``sample_subgraph`` (hops included).  Beside it, on the same hop outputs and alternating with it: the same algorithm composed from
torch device ops -- PyG's formula (``unique`` of all ids, ``tmp[n_id] = arange``, ``idx = src * num_nodes + dst``,
``idx.unique(return_inverse=True)``, a ``scatter_reduce`` minimum for ``e_id``) -- by the same host clock; its result is compared with
the stage's while it is at it.

usage: python tools/sampler_time.py [--batches 100] [--numpy-batches 3] [--subgraph] [--json OUT]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import sampler as S                          # noqa: E402
from npi_gnn_amd.synth import bipartite_edge_index            # noqa: E402
from _timing import TimedLib, dump_json, row_summary, wall    # noqa: E402

U64 = np.uint64
GAMMA = U64(0x9E3779B97F4A7C15)


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def numpy_hop(rowptr, col, eid, targets, k, hop, seed, loops):
    """one block by the rule, in numpy: (n_id, e_id, edge_index)"""
    one = lambda i: np.array([int(i) & ((1 << 64) - 1)], dtype=U64)            # noqa: E731
    with np.errstate(over="ignore"):
        hop_base = mix64(one(seed) + GAMMA * one(hop + 1))
    src, e_id, tgt = [], [], []
    for t, v in enumerate(targets):
        s, d = int(rowptr[v]), int(rowptr[v + 1] - rowptr[v])
        if d <= k:
            pos = np.arange(d)
        else:
            p = np.arange(d, dtype=U64)
            with np.errstate(over="ignore"):
                base = mix64(hop_base ^ (one(v) * U64(0xD6E8FEB86659FD93)))
                keys = ((mix64(base + GAMMA * (p + U64(1))) >> U64(32)) << U64(32)) | p
            pos = np.sort(np.argpartition(keys, k)[:k])
        src.append(col[s + pos])
        e_id.append(eid[s + pos])
        tgt.append(np.full(len(pos), t, dtype=np.int64))
    src, e_id, tgt = np.concatenate(src), np.concatenate(e_id), np.concatenate(tgt)
    n_id = np.unique(np.concatenate([src, targets]) if loops else src)
    return n_id, e_id, np.stack([np.searchsorted(n_id, src), tgt])


def torch_union_coalesce(b_id, src_g, dst_g, eid, tmp):
    """PyG 1.4.2 ``__produce_subgraph__`` behind the hops, composed from torch ops on the device (``tmp``: an N-entry LongTensor kept
    between calls, as PyG's ``self.tmp``); the minimum instead of ``scatter_``'s whichever-comes-last, so that the result is defined"""
    n_id = torch.unique(torch.cat([b_id, src_g, dst_g]))
    U = n_id.numel()
    tmp[n_id] = torch.arange(U, device=n_id.device)
    idx = tmp[src_g] * U + tmp[dst_g]
    idx, inv = idx.unique(return_inverse=True)
    edge_index = torch.stack([idx // U, idx % U])
    e_id = torch.full((idx.numel(),), 2 ** 62, dtype=torch.int64, device=idx.device).scatter_reduce_(0, inv, eid, "amin")
    return edge_index, e_id, n_id, tmp[b_id], U


def subgraph_mode(args, sampler, timed, order, seed, dev):
    """the ``--subgraph`` run (module docstring)"""
    tmp = torch.empty(args.nodes, dtype=torch.int64, device=dev)
    rows = []
    for i, pos in enumerate(order):
        b_id = pos.to(dev)
        _, whole = wall(lambda: sampler.sample_subgraph(b_id, seed))
        timed.take()
        src_g, dst_g, eid = sampler.hop_entries(b_id, seed)
        src64, dst64, eid64 = src_g.long(), dst_g.long(), eid.long()
        timed.take()
        sub, stage = wall(lambda: sampler.union_subgraph(b_id, src_g, dst_g, eid))
        ev = timed.take()
        ref, composed = wall(lambda: torch_union_coalesce(b_id, src64, dst64, eid64, tmp))
        same = (torch.equal(ref[0], sub.edge_index) and torch.equal(ref[1], sub.e_id) and torch.equal(ref[2], sub.n_id)
                and torch.equal(ref[3], sub.sub_b_id) and ref[4] == sub.num_nodes)
        if not same:
            raise SystemExit("the stage's subgraph differs from the torch composition")
        if i >= args.warmup:
            rows.append({"union_ms": ev["npi_sample_union"], "coalesce_ms": ev["npi_sample_coalesce"], "stage_wall_ms": stage,
                         "torch_composed_wall_ms": composed, "sample_subgraph_wall_ms": whole, "entries": int(src_g.numel()),
                         "num_nodes": sub.num_nodes, "edges": int(sub.e_id.numel())})
    res = row_summary(rows)
    res["batches"] = len(rows)
    print(json.dumps(res, indent=1), flush=True)
    print("(every subgraph equal to the torch composition's)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numpy-batches", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--subgraph", action="store_true", help="time the one-id-space flow (sample_subgraph) instead")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    sizes, bs = [25, 10], 1024
    ei_host = bipartite_edge_index(args.nodes, args.edges, seed=20260310)
    ei = ei_host.to(dev)
    t0 = time.perf_counter()
    sampler = npi.NeighborSampler(ei, args.nodes, size=sizes, num_hops=2, batch_size=bs, shuffle=True, add_self_loops=True, seed=0)
    torch.cuda.synchronize()
    print(f"sampler construction (one CSR build of {args.edges} edges): {1e3 * (time.perf_counter() - t0):.1f} ms", flush=True)
    deg = (sampler.side.rowptr[1:] - sampler.side.rowptr[:-1])
    print(f"in-degree: max {int(deg.max())}, rows above 2048 entries {int((deg > 2048).sum())}", flush=True)
    seed = S.epoch_seed(0, 0)
    order = S.epoch_batches(args.nodes, bs, True, False, 0, 0)[: args.warmup + args.batches]
    timed = TimedLib(S.load(), "npi_sample_")
    S.load = lambda: timed                                   # the sampler module's handle on the library, for this process only
    if args.subgraph:
        dump_json(subgraph_mode(args, sampler, timed, order, seed, dev), args.json)
        return
    rows, flows = [], []
    for i, pos in enumerate(order):
        targets = pos.to(dev)
        flow, flow_ms = wall(lambda: sampler.sample(targets, seed))
        ev = timed.take()
        if i >= args.warmup:
            rows.append({"counts_ms": ev["npi_sample_counts"], "select_ms": ev["npi_sample_select"],
                         "relabel_ms": ev["npi_sample_relabel_count"] + ev["npi_sample_relabel"], "data_flow_wall_ms": flow_ms,
                         "sources_outer": flow[0].size[0], "edges": sum(int(b.e_id.numel()) for b in flow)})
            if len(flows) < args.numpy_batches:
                flows.append((pos.numpy(), flow))
    res = row_summary(rows)
    res["batches"] = len(rows)
    print(json.dumps(res, indent=1), flush=True)
    # the numpy restatement on the same batches
    dst = ei_host[1].numpy()
    t0 = time.perf_counter()
    perm = np.argsort(dst, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=args.nodes))])
    col = ei_host[0].numpy()[perm]
    print(f"numpy: by-target CSR (stable argsort) {time.perf_counter() - t0:.1f} s", flush=True)
    np_ms = []
    for targets, flow in flows:
        t0 = time.perf_counter()
        n_id = targets
        blocks = []
        for hop, k in enumerate(sizes):
            blk = numpy_hop(rowptr, col, perm, n_id, k, hop, seed, True)
            blocks.append(blk)
            n_id = blk[0]
        np_ms.append(1e3 * (time.perf_counter() - t0))
        for blk, dev_blk in zip(blocks, [flow[1], flow[0]]):
            same = (np.array_equal(blk[0], dev_blk.n_id.cpu().numpy()) and np.array_equal(blk[1], dev_blk.e_id.cpu().numpy())
                    and np.array_equal(blk[2], dev_blk.edge_index.cpu().numpy()))
            if not same:
                raise SystemExit("the device's block differs from the numpy restatement")
    if np_ms:
        res["numpy_data_flow_ms"] = {"median": statistics.median(np_ms), "batches": len(np_ms)}
        print(f"numpy restatement, whole DataFlow: median {statistics.median(np_ms):.0f} ms over {len(np_ms)} batches "
              "(blocks equal to the device's)", flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
