#!/usr/bin/env python3
"""What the gradient w.r.t. edge_weight costs (EXPERIMENTS: "d edge_weight"), on the synthetic bipartite graph:

  * HIP-event time of the dot launch (``npi_edge_dot``, by-target side, F columns) against the WEIGHTED aggregation launch
    (``npi_segsum_ex``) over the same side in the same process, alternated -- both gather the same E F 4 bytes;
  * the whole SAGEConv step (forward + backward, x / W / b gradients) with a constant weight and with a weight that requires grad;
  * peak memory of both steps (the weight gradient keeps x alive and forms dAgg).

usage: tools/edge_dot_time.py [nodes edges [F]]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi
from npi_gnn_amd import functional as NF
from npi_gnn_amd.synth import bipartite_edge_index_device
dev = torch.device("cuda:0")
N, E = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1_000_000, 20_000_000)
F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
REPS, ROUNDS = 10, 3


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


graph = npi.CSRGraph(bipartite_edge_index_device(N, E, dev, seed=2), N, sort_columns=True)
side = graph.by_dst
torch.manual_seed(0)
x = torch.randn(N, F, device=dev)
dagg = torch.randn(N, F, device=dev)
ew = torch.rand(E, device=dev) + 0.5
w_entry = NF.entry_weights(graph, ew, 1.0)
out = torch.empty(N, F, device=dev)
d_edge, d_loop = torch.zeros(E, device=dev), torch.zeros(N, device=dev)
inv = graph.inv_count(side)
launches = (("segsum_weighted", lambda: NF.segsum(graph, side, x, w=w_entry[0], mean=True, out=out)),
            ("edge_dot", lambda: NF.edge_dot(side, dagg, x, E, row_scale=inv, d_edge=d_edge, d_loop=d_loop)))
for _, fn in launches:
    for _ in range(3):
        fn()
res = {name: [] for name, _ in launches}
for _ in range(ROUNDS):                                              # alternated: A B A B A B
    for name, fn in launches:
        res[name].append(timed(fn))
for name, v in res.items():
    print(f"{name:16s} F={F}: " + "  ".join(f"{t:.3f}" for t in v) + f" ms  (median {sorted(v)[len(v) // 2]:.3f})")
ratio = sorted(res["edge_dot"])[ROUNDS // 2] / sorted(res["segsum_weighted"])[ROUNDS // 2]
print(f"edge_dot / segsum_weighted = {ratio:.2f}   (gathered bytes {E * F * 4 / 1e9:.1f} GB each)")
del out, dagg, d_edge, d_loop
torch.cuda.empty_cache()

W = (torch.randn(F, F, device=dev) / F ** 0.5).requires_grad_(True)
b = torch.randn(F, device=dev).requires_grad_(True)
xg = x.requires_grad_(True)
go = torch.randn(N, F, device=dev)


def step(w):
    npi.sage_conv(xg, graph, W, b, edge_weight=w).backward(go)
    xg.grad = W.grad = b.grad = None
    if w.requires_grad:
        w.grad = None


steps = (("step_constant_weight", ew), ("step_weight_gradient", ew.clone().requires_grad_(True)))
peak = {}
for name, w in steps:
    for _ in range(2):
        step(w)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    step(w)
    torch.cuda.synchronize()
    peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
res = {name: [] for name, _ in steps}
for _ in range(ROUNDS):
    for name, w in steps:
        res[name].append(timed(lambda: step(w), 5))
for name, v in res.items():
    print(f"{name:22s}: " + "  ".join(f"{t:.3f}" for t in v) + f" ms  (median {sorted(v)[len(v) // 2]:.3f}), peak above the inputs {peak[name]:.0f} MiB")
