#!/usr/bin/env python3
"""Timings of the bipartite form on one MI355X (EXPERIMENTS.md): same process, the variants alternating round by round, warm,
HIP events around every call, the median per variant.

  gather   npi_rows_gather at n = 1M, F = 256, f32, into the left half of a [n, 512] buffer, against index_select + copy_
  layers   the two directed half-layers of the benchmark's C4 graph (ncRNA -> protein, size (900k, 100k), and protein -> ncRNA,
           size (100k, 900k); F = 256, one weight each), fwd + bwd, hub streaming on and off for the rectangular sides, beside the
           square SAGEConv layer on the same graph.  A record, not a comparison: the two forms compute different things.

usage: python tools/bipartite_time.py [--rounds 20] [--json OUT]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import functional as NF                      # noqa: E402
from npi_gnn_amd.synth import bipartite_edge_index            # noqa: E402


def alternate(variants: dict, rounds: int, warmup: int = 3) -> dict:
    """median ms per variant; one call of every variant per round, in turn"""
    times = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def gather(dev, rounds):
    n, F = 1_000_000, 256
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, F, generator=g).to(dev)
    idx = torch.randperm(n, generator=g).to(dev)
    buf = torch.empty(n, 2 * F, device=dev)
    left = buf[:, :F]
    return alternate({"npi_rows_gather": lambda: NF.rows_gather(x, idx, left),
                      "index_select+copy_": lambda: left.copy_(x.index_select(0, idx))}, rounds)


def layers(dev, rounds):
    n_rna, n_pro, F = 900_000, 100_000, 256
    ei = bipartite_edge_index(n_rna + n_pro, 20_000_000, seed=20260310).to(dev)      # the benchmark's C4 graph: every edge both ways
    fwd = ei[:, ei[0] < n_rna]                                                       # ncRNA -> protein (synth: ncRNA ids come first)
    if fwd.numel() == 0 or int(fwd[1].min()) < n_rna:
        raise SystemExit("synth.bipartite_edge_index no longer puts the 900k side first: adapt the split")
    a2b = torch.stack([fwd[0], fwd[1] - n_rna])
    b2a = a2b.flip(0)
    g = torch.Generator().manual_seed(1)
    x_all = torch.randn(n_rna + n_pro, F, generator=g).to(dev)
    W1, W2 = ((torch.randn(F, F, generator=g) / 16).to(dev).requires_grad_(True) for _ in range(2))
    b1, b2 = (torch.zeros(F, device=dev, requires_grad=True) for _ in range(2))
    go = torch.randn(n_rna + n_pro, F, generator=g).to(dev)
    sq = npi.CSRGraph(ei, n_rna + n_pro)
    variants = {}

    def step(fn, x, grad):
        def run():
            xg = x.detach().requires_grad_(True)
            fn(xg).backward(grad)
        return run
    variants["square SAGEConv (1M, 20M entries + loops)"] = step(lambda xg: npi.sage_conv(xg, sq, W1, b1), x_all, go)
    for hub in (True, False):
        ga = npi.BipartiteGraph(a2b, (n_rna, n_pro), hub_stream=hub)
        gb = npi.BipartiteGraph(b2a, (n_pro, n_rna), hub_stream=hub)
        tag = "hub streaming on" if hub else "hub streaming off"
        variants[f"ncRNA->protein (900k, 100k), {tag}"] = step(
            lambda xg, ga=ga: npi.sage_conv_bipartite((xg, None), ga, W1, b1), x_all[:n_rna], go[:n_pro])
        variants[f"protein->ncRNA (100k, 900k), {tag}"] = step(
            lambda xg, gb=gb: npi.sage_conv_bipartite((xg, None), gb, W2, b2), x_all[n_rna:], go[:n_rna])
        for gr in (ga, gb):
            for side in (gr.by_dst, gr.by_src):
                plan = side.hub_plan() if hub else None
                print(f"   {tag}: side {side.n_rows} x {side.n_cols}: hubs {plan.H if plan is not None else 0}", flush=True)
    out = alternate(variants, rounds)
    out["_edges_per_direction"] = int(a2b.size(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"gather": gather(dev, args.rounds)}
    print(json.dumps(res["gather"], indent=1), flush=True)
    res["layers"] = layers(dev, args.rounds)
    print(json.dumps(res["layers"], indent=1), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
