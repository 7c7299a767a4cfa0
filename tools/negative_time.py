#!/usr/bin/env python3
"""Timings of ``npi.NegativeSampler`` on one MI355X (EXPERIMENTS.md A45): the benchmark's synthetic C4 graph
(``npi_gnn_amd/synth.py``: 1M nodes in one id space, 20M directed edges, Zipf hubs), ``M = E`` distinct non-edge pairs per draw,
and one ``corrupt`` of ``edge_index[0]`` (``K = E`` slots).

Per draw it reports the device time of each entry point (HIP events around the call: ``npi_negative_candidates``,
``npi_negative_distinct``, ``npi_negative_targets``) and the wall time of ``pairs`` (host clock around the call ending in a
synchronise: it includes the host read of ``info``).

Beside it, alternating with it: the same draw composed from torch device ops -- ``randint`` candidates over a window of the same
length, ``isin`` on ``src * n_dst + dst`` codes against the sorted edge codes, ``unique(return_inverse=True)`` and a
``scatter_reduce`` minimum of the positions to keep the first occurrence of every pair, the first ``M`` in position order -- by the
same host clock.  Its random bits are torch's, so the two results are not compared element for element; each is checked to be
``M`` distinct non-edges.

usage: python tools/negative_time.py [--draws 10] [--warmup 2] [--nodes N --edges E] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import negative as NEG                       # noqa: E402
from npi_gnn_amd.synth import bipartite_edge_index            # noqa: E402
from _timing import TimedLib, dump_json, row_summary, wall    # noqa: E402


def torch_pairs(edge_codes, n_src, n_dst, M, W, gen):
    """the same draw from torch device ops: the first ``M`` distinct non-edges of ``W`` uniform candidates, in candidate order"""
    dev = edge_codes.device
    while True:
        c = torch.randint(n_src, (W,), device=dev, generator=gen) * n_dst + torch.randint(n_dst, (W,), device=dev, generator=gen)
        c = c[~torch.isin(c, edge_codes, assume_unique=False)]
        u, inv = torch.unique(c, return_inverse=True)
        if u.numel() >= M:                                   # (the host read of the composition: its unique is one already)
            first = torch.full((u.numel(),), W, dtype=torch.int64, device=dev)
            first.scatter_reduce_(0, inv, torch.arange(c.numel(), device=dev), "amin")
            c = c[first.sort().values[:M]]
            return torch.stack([c // n_dst, c % n_dst])
        W *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    N = args.nodes
    ei = bipartite_edge_index(N, args.edges, seed=20260310).to(dev)
    E = int(ei.size(1))
    neg, build_ms = wall(lambda: npi.NegativeSampler(ei, size=N, seed=0, allow_loops=False))
    print(f"sampler construction (one column-sorted CSR build of {E} edges + the non-edge count): {build_ms:.1f} ms; {neg}", flush=True)
    edge_codes = torch.unique(ei[0] * N + ei[1])
    timed = TimedLib(NEG.load(), "npi_negative_")
    NEG.load = lambda: timed                                  # the module's handle on the library, for this process only
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    src = ei[0].contiguous()
    rows = []

    def check(p, what):
        codes = p[0] * N + p[1]
        ok = tuple(p.shape) == (2, E) and not bool(torch.isin(codes, edge_codes).any()) and int(torch.unique(codes).numel()) == E \
            and bool((p[0] != p[1]).all() if what == "pairs" else True)
        if not ok:
            raise SystemExit(f"{what}: not {E} distinct non-edges")
    for i in range(args.warmup + args.draws):
        p, pairs_ms = wall(lambda: neg.pairs(draw=i))
        ev = timed.take()
        W = neg.last_window
        q, torch_ms = wall(lambda: torch_pairs(edge_codes, N, N, E, W, gen))
        k, corrupt_ms = wall(lambda: neg.corrupt(src, draw=i))
        ev.update(timed.take())
        if i == 0:
            check(p, "pairs")
            check(q, "torch composition")
            if bool((k < 0).any()) or bool(torch.isin(src * N + k, edge_codes).any()):
                raise SystemExit("corrupt: a slot holds an edge or -1")
        if i >= args.warmup:
            rows.append({"candidates_ms": ev["npi_negative_candidates"], "distinct_ms": ev["npi_negative_distinct"],
                         "pairs_wall_ms": pairs_ms, "torch_composed_wall_ms": torch_ms, "targets_ms": ev["npi_negative_targets"],
                         "corrupt_wall_ms": corrupt_ms, "window": W, "consumed": neg.last_consumed})
    res = row_summary(rows)
    res.update(draws=len(rows), nodes=N, edges=E, pairs_per_draw=E, non_edges=neg.num_non_edges, construction_ms=build_ms)
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
