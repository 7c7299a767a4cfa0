#!/usr/bin/env python3
"""GATConv with H heads at the C4 shape (H x C = 256): ms per layer step; under rocprofv3 --kernel-trace its kernels.
usage: tools/gat_heads_probe.py [heads] [steps] [fwd]
fwd: instead, the FORWARD alone (relu=True, no autograd) with the statistics inside the aggregation launch against
Schedule(gat_fused_stats=False) -- statistics pass + aggregation (+ ReLU pass for several heads) --, alternating, median of `steps`."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi
from npi_gnn_amd.synth import bipartite_edge_index
dev = torch.device("cuda:0")
H = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N, E, F = 1_000_000, 20_000_000, 256
g = npi.CSRGraph(bipartite_edge_index(N, E).to(dev), N); _ = g.by_src
conv = npi.GATConv(F, F // H, heads=H).to(dev)
x = torch.randn(N, F, device=dev).requires_grad_(True)
go = torch.randn(N, F, device=dev)
if len(sys.argv) > 3 and sys.argv[3] == "fwd":
    from npi_gnn_amd.schedule import DEFAULT
    convs = {k: npi.GATConv(F, F // H, heads=H, schedule=DEFAULT.but(gat_fused_stats=k)).to(dev) for k in (True, False)}
    convs[False].load_state_dict(convs[True].state_dict())
    times = {True: [], False: []}
    with torch.no_grad():
        for i in range(3 + n):
            for k in (True, False):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); convs[k](x, g, relu=True); b.record(); torch.cuda.synchronize()
                if i >= 3: times[k].append(a.elapsed_time(b))
    for k in (True, False):
        print(f"GATConv {H} heads forward, gat_fused_stats={k}: median {sorted(times[k])[len(times[k]) // 2]:.3f} ms  min {min(times[k]):.3f} ms")
    sys.exit(0)
def step():
    for p in conv.parameters(): p.grad = None
    x.grad = None
    conv(x, g).backward(go)
for _ in range(3): step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(n): step()
torch.cuda.synchronize()
print(f"GATConv {H} heads: {(time.perf_counter() - t0) / n * 1e3:.3f} ms per step")
