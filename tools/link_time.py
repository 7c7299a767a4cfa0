#!/usr/bin/env python3
"""Timings of ``npi.link_loss`` on one MI355X (EXPERIMENTS.md A46): the benchmark's synthetic C4 graph (``npi_gnn_amd/synth.py``:
1M nodes, 20M directed edges, Zipf hubs) read as a bipartite pair -- two embedding tables ``[N, 256]`` float32 --, ``M = 2 x
1,048,576`` pairs: 1,048,576 columns of the edge list as positives (a fixed random subset, so the hubs keep their share) and as
many uniform random pairs as negatives.

Per step and loss form it reports
  * the forward launch alone (HIP events around ``link_loss`` under ``torch.no_grad()``: ``npi_pair_score`` plus the one-workgroup
    sum of the partials),
  * forward + backward of ``link_loss`` with both tables requiring grad, INCLUDING the build of both sides of the pair list (two
    sorts of M pairs) and the two aggregations (host clock around the step, ending in a synchronise),
and, alternating with it call by call, the same step from torch device ops: two ``[M, 256]`` gathers, their product, the row sum,
``binary_cross_entropy_with_logits`` or the GAE expression, and autograd's backward (two ``index_add_`` scatters with float atomics)
-- forward alone under ``no_grad`` and forward + backward, by the same clocks.  The first step checks the two losses and gradients
against each other.

usage: python tools/link_time.py [--steps 10] [--warmup 2] [--nodes N --edges E --pairs P --features F] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd.synth import bipartite_edge_index            # noqa: E402
from _timing import device_ms, dump_json, row_summary, wall   # noqa: E402

EPS = 1e-15


def torch_loss(zs, zd, ei, n_pos, kind):
    x = (zs[ei[0]] * zd[ei[1]]).sum(1)
    if kind == "gae":
        return -torch.log(torch.sigmoid(x[:n_pos]) + EPS).mean() - torch.log(1 - torch.sigmoid(x[n_pos:]) + EPS).mean()
    y = (torch.arange(x.numel(), device=x.device) < n_pos).float()
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--pairs", type=int, default=1_048_576, help="positives; as many negatives")
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    N, F, P = args.nodes, args.features, args.pairs
    ei = bipartite_edge_index(N, args.edges, seed=20260310).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    pos = ei[:, torch.randperm(ei.size(1), device=dev, generator=gen)[:P]].contiguous()
    P = int(pos.size(1))
    scale = 0.7 * F ** -0.25                                   # logits of standard deviation 0.49, as in the tests
    zs = (torch.randn(N, F, device=dev, generator=gen) * scale).requires_grad_(True)
    zd = (torch.randn(N, F, device=dev, generator=gen) * scale).requires_grad_(True)
    rows = {"gae": [], "bce": []}

    def step_npi(neg, kind):
        zs.grad = zd.grad = None
        loss = npi.link_loss((zs, zd), pos, neg, loss=kind)
        loss.backward()
        return loss.detach(), zs.grad, zd.grad

    def step_torch(both, kind):
        zs.grad = zd.grad = None
        loss = torch_loss(zs, zd, both, P, kind)
        loss.backward()
        return loss.detach(), zs.grad, zd.grad

    for i in range(args.warmup + args.steps):
        neg = torch.stack([torch.randint(N, (P,), device=dev, generator=gen), torch.randint(N, (P,), device=dev, generator=gen)])
        both = torch.cat([pos, neg], 1)
        for kind in ("gae", "bce"):
            with torch.no_grad():
                _, fwd_ms = device_ms(lambda: npi.link_loss((zs, zd), pos, neg, loss=kind))
                _, torch_fwd_ms = device_ms(lambda: torch_loss(zs, zd, both, P, kind))
            (l0, a0, b0), step_ms = wall(lambda: step_npi(neg, kind))
            (l1, a1, b1), torch_step_ms = wall(lambda: step_torch(both, kind))
            if i == 0:
                for name, u, v in (("loss", l0, l1), ("dZ_src", a0, a1), ("dZ_dst", b0, b1)):
                    err = float((u.double() - v.double()).abs().max() / v.double().abs().max())
                    print(f"{kind}: {name} against the torch composition (float32, atomics): max |diff| / max |ref| = {err:.2e}", flush=True)
                    if not err <= 1e-4:
                        raise SystemExit(f"{kind}: {name} differs from the torch composition")
            if i >= args.warmup:
                rows[kind].append({"forward_ms": fwd_ms, "step_wall_ms": step_ms, "torch_forward_ms": torch_fwd_ms,
                                   "torch_step_wall_ms": torch_step_ms})
    npi.graph.check_pending()
    res = {kind: row_summary(rs) for kind, rs in rows.items()}
    res.update(steps=args.steps, nodes=N, edges=int(ei.size(1)), features=F, pairs=2 * P,
               not_measured=["the pair-graph build and the two aggregations separately", "kernel times from a profiler",
                             "a prebuilt BipartiteGraph of the pairs", "one id space", "widths other than --features",
                             "NegativeSampler negatives (uniform random pairs stand in)"])
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
