#!/usr/bin/env python3
"""HIP-event time of one GATConv training step (forward + backward) with and without attention dropout, on the synthetic bipartite
graph (default: the C4 size, 1M nodes / 20M edges, 256 input features), for the two flagship shapes H = 1, C = 256 and H = 4, C = 64:
    plain     the dropout-free layer
    composed  the composed variant with a mask from torch's generator (functional._GatDropoutFn: alpha, keep, e, dz as [nnz, H]
              arrays, one aggregation launch per head and direction)
    seeded    AttentionDropout(p, seed, draw): the mask recomputed per entry inside the fused kernels (a fresh draw per step)
Every mode is timed `repeats` times, the modes alternating inside a repeat (same box, same process); a tree without the seeded
path (an earlier commit: copy this file into its tools/) runs with --modes plain,composed.
usage: tools/gat_dropout_time.py [--nodes N --edges E --features F --p P --steps K --warmup W --repeats R --modes a,b,c --json FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                            # noqa: E402
from npi_gnn_amd import functional as NF                            # noqa: E402
from npi_gnn_amd.synth import bipartite_edge_index_device           # noqa: E402
from _timing import dump_json, summary                              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--edges", type=int, default=20_000_000)
ap.add_argument("--features", type=int, default=256)
ap.add_argument("--p", type=float, default=0.6)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--modes", default="plain,composed,seeded")
ap.add_argument("--shapes", default="1x256,4x64")
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
modes = args.modes.split(",")


def stage(m):
    torch.cuda.synchronize()
    print("  ..", m, file=sys.stderr, flush=True)


stage("start")
graph = npi.CSRGraph(bipartite_edge_index_device(args.nodes, args.edges, dev, seed=2), args.nodes, sort_columns=True)
graph.by_src
stage("graph")
gen = torch.Generator(device=dev).manual_seed(1)
x = torch.randn(args.nodes, args.features, device=dev, generator=gen).requires_grad_(True)
res = {"nodes": args.nodes, "edges": args.edges, "features": args.features, "p": args.p, "steps": args.steps,
       "lib": os.path.basename(os.environ.get("NPI_GNN_LIB", "default")), "shapes": {}}
for shape in args.shapes.split(","):
    H, C = (int(v) for v in shape.split("x"))
    W = (torch.randn(args.features, H * C, device=dev, generator=gen) / args.features ** 0.5).requires_grad_(True)
    att = (torch.randn(1, H, 2 * C, device=dev, generator=gen) / C ** 0.5).requires_grad_(True)
    b = torch.zeros(H * C, device=dev).requires_grad_(True)
    go = torch.randn(args.nodes, H * C, device=dev, generator=gen)
    draw = [0]

    def step(mode):
        kw = {}
        if mode == "composed":
            kw["keep"] = NF.gat_dropout_keep(graph, H, args.p)
        elif mode == "seeded":
            kw["dropout"] = NF.AttentionDropout(args.p, 0, draw[0])
            draw[0] += 1
        out = npi.gat_conv(x, graph, W, att, b, heads=H, **kw)
        out.backward(go)
        x.grad = W.grad = att.grad = b.grad = None

    times = {m: [] for m in modes}
    for rep in range(args.repeats):
        for m in modes:
            for _ in range(args.warmup):
                step(m)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(m)
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1) / args.steps)
            stage(f"H={H} C={C} repeat {rep} {m}: {times[m][-1]:.3f} ms per step")
    res["shapes"][shape] = {m: dict(summary(v), repeats=v) for m, v in times.items()}
    print(res["lib"], args.nodes, args.edges, f"H={H} C={C} |",
          "  ".join(f"{m} " + " / ".join(f"{t:.3f}" for t in v) + " ms" for m, v in times.items()))
dump_json(res, args.json)
