#!/usr/bin/env python3
"""Timings of ``npi.EdgeSplitter`` on one MI355X (EXPERIMENTS.md A50): one id space, a random edge list given in both orientations
that is already on the device, ``E`` = 41,648 over 5,085 nodes (NPInter2's size) and 20M over 1M nodes (C4's).

Per case it reports, alternating call by call, all by a host clock that ends in a synchronise (every one of them reads a size back):
  * ``permutation``: Rule S 1-2 (keep flags, scan, partition, two 32-bit sorts, gather; one host read),
  * ``split``: ``permutation``, the undirected form of the train slice and ``0.15 K`` held-out negatives from the splitter's sampler,
    which is built before the clock starts (its build -- the undirected form of the whole list and a CSR of it -- is timed once, as
    ``sampler_build``),
  * ``to_undirected`` of the whole list,
  * the torch device composition of the order: ``row < col`` mask, ``torch.randperm`` and indexing of both rows,
  * the torch device composition of the undirected form: ``torch.unique`` of the 64-bit codes of both orientations, then ``//``, ``%``.
PyG's held-out negatives need a dense [N, N] mask (1 TB of bytes at 1M nodes): not run.

usage: python tools/split_time.py [--steps 10] [--warmup 3] [--cases 41648:5085 20000000:1000000] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from _timing import dump_json, row_summary, wall              # noqa: E402


def torch_order(ei):
    mask = ei[0] < ei[1]
    row, col = ei[0][mask], ei[1][mask]
    perm = torch.randperm(row.numel(), device=ei.device)
    return torch.stack([row[perm], col[perm]])


def torch_undirected(ei, N):
    codes = torch.unique(torch.cat([ei[0] * N + ei[1], ei[1] * N + ei[0]]))
    return torch.stack([codes // N, codes % N])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=["41648:5085", "20000000:1000000"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"steps": args.steps, "cases": {}}
    for case in args.cases:
        E, N = (int(v) for v in case.split(":"))
        half = torch.randint(0, N, (2, E // 2), device=dev, generator=gen)
        ei = torch.cat([half, half.flip(0)], dim=1).contiguous()
        sp = npi.EdgeSplitter(ei, N, seed=0)
        _, build_ms = wall(lambda: sp.split(0.05, 0.1, draw=0))                 # builds the sampler over the whole list
        und = npi.to_undirected(ei, N)
        assert torch.equal(und, torch_undirected(ei, N)), "to_undirected differs from torch.unique"
        rows = []
        for i in range(args.warmup + args.steps):
            (edges, _), perm_ms = wall(lambda: sp.permutation(draw=i))
            s, split_ms = wall(lambda: sp.split(0.05, 0.1, draw=i))
            _, und_ms = wall(lambda: npi.to_undirected(ei, N))
            t_edges, t_order_ms = wall(lambda: torch_order(ei))
            _, t_und_ms = wall(lambda: torch_undirected(ei, N))
            assert edges.shape == t_edges.shape
            if i >= args.warmup:
                rows.append({"permutation_ms": perm_ms, "split_ms": split_ms, "to_undirected_ms": und_ms,
                             "torch_randperm_index_ms": t_order_ms, "torch_unique_codes_ms": t_und_ms})
        npi.graph.check_pending()
        out = row_summary(rows)
        out["first_split_with_sampler_build_ms"] = build_ms
        out["kept"], out["held_out_negatives"] = int(edges.shape[1]), int(s.val_neg_edge_index.shape[1] + s.test_neg_edge_index.shape[1])
        res["cases"][case] = out
        print(f"E={E} N={N}: " + ", ".join(f"{k} {v['median']:.3f}" for k, v in out.items() if isinstance(v, dict))
              + f", first split {build_ms:.1f}", flush=True)
    res["not_measured"] = ["kernel times from a profiler", "kfold", "two id spaces", "PyG's dense-mask negatives (cannot run at 1M nodes)"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
