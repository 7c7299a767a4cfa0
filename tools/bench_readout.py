#!/usr/bin/env python3
"""Timings of the Rule O readouts on one MI355X (EXPERIMENTS.md A60): ``global_add_pool``, ``global_sort_pool(k)`` and
``attention_readout`` against the torch compositions they replace, in one process, the two forms alternating call by call, HIP events
around each call; forward alone (no autograd) and forward + backward.

Shapes:
  * net1   200 graphs of 60 .. 364 rows (about 42.4k rows, the batch of the reference's train loop), F = 128
  * many   16,658 graphs of the same size distribution, F = 128
  * one    one graph of 1,000,000 rows, F = 256
Compositions (the literal PyG 1.4.2 code on torch ops):
  * add        ``zeros.index_add_(0, batch, x)``
  * sort       ``to_dense_batch`` (fill ``x.min() - 1``) + ``sort(descending=True)`` of the last column + gather + truncate / pad
  * attention  ``exp(gate - scatter_max[batch]) / (scatter_add[batch] + 1e-16)``, then ``zeros.index_add_(0, batch, alpha * x)``
The first step of every case checks the fused result against the composition evaluated in fp64 (1e-5 of the largest magnitude; it
prints the f32 composition's own error beside it) and the gradient of x against the f32 composition's; the sort pool is compared on
inputs without ties, where PyG's order and the rule's agree.

usage: python tools/bench_readout.py [--steps 10] [--warmup 3] [--shapes net1 many one] [--k 30] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from npi_gnn_amd import graph as NG                           # noqa: E402
from npi_gnn_amd import pool as NP                            # noqa: E402
from _timing import device_ms, dump_json, row_summary         # noqa: E402


def shapes(names):
    g = torch.Generator().manual_seed(0)
    out = []
    for name in names:
        if name == "net1":
            out.append((name, torch.randint(60, 365, (200,), generator=g), 128))
        elif name == "many":
            out.append((name, torch.randint(60, 365, (16658,), generator=g), 128))
        elif name == "one":
            out.append((name, torch.tensor([1_000_000]), 256))
        else:
            raise SystemExit(f"unknown shape {name}")
    return out


def composed_add(x, batch, B):
    return torch.zeros((B, x.size(1)), dtype=x.dtype, device=x.device).index_add_(0, batch, x)


def composed_sort(x, batch, B, k, ptr, n_max):
    fill = x.detach().min() - 1                               # (PyG reads it back with .item(); kept on the device here)
    idx = torch.arange(batch.numel(), device=x.device) - ptr[batch] + batch * n_max
    dense = (torch.zeros((B * n_max, x.size(1)), device=x.device) + fill).index_put((idx,), x).view(B, n_max, -1)
    _, perm = dense[:, :, -1].sort(dim=-1, descending=True)
    perm = perm + (torch.arange(B, device=x.device) * n_max).view(-1, 1)
    dense = dense.view(B * n_max, -1)[perm.view(-1)].view(B, n_max, -1)
    if n_max >= k:
        dense = dense[:, :k].contiguous()
    else:
        dense = torch.cat([dense, (torch.zeros((B, k - n_max, dense.size(2)), device=x.device) + fill)], dim=1)
    dense = torch.where(dense == fill, torch.zeros_like(dense), dense)
    return dense.view(B, -1)


def composed_attention(gate, x, batch, B):
    mx = torch.full((B,), -float("inf"), dtype=x.dtype, device=x.device).scatter_reduce(0, batch, gate, "amax")
    e = (gate - mx[batch]).exp()
    alpha = e / (torch.zeros(B, dtype=x.dtype, device=x.device).index_add(0, batch, e)[batch] + 1e-16)
    return torch.zeros((B, x.size(1)), dtype=x.dtype, device=x.device).index_add_(0, batch, alpha[:, None] * x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["net1", "many", "one"])
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"steps": args.steps, "warmup": args.warmup, "k": args.k, "cases": []}
    for name, sizes, F in shapes(args.shapes):
        B, N, n_max = sizes.numel(), int(sizes.sum()), int(sizes.max())
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        x = torch.randn(N, F, device=dev, generator=gen)
        gate = 3 * torch.randn(N, device=dev, generator=gen)
        batch = torch.repeat_interleave(torch.arange(B), sizes).to(dev)
        ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]).to(dev)
        gb = NG.GraphBatch(x, torch.zeros((2, 0), dtype=torch.int64, device=dev), batch, B, sizes=sizes)
        gb.segment_ptr()
        k = args.k
        cases = {
            "add": (lambda xx, gg: NP.global_add_pool(gb.with_x(xx)), lambda xx, gg: composed_add(xx, batch, B), F),
            "sort": (lambda xx, gg: NP.global_sort_pool(gb.with_x(xx), k=k), lambda xx, gg: composed_sort(xx, batch, B, k, ptr, n_max), k * F),
            "attention": (lambda xx, gg: NP.attention_readout(gg, gb.with_x(xx)), lambda xx, gg: composed_attention(gg, xx, batch, B), F),
        }
        for what, (fused, composed, width) in cases.items():
            dout = torch.randn(B, width, device=dev, generator=gen)
            rows = []
            for i in range(args.warmup + args.steps):
                r = {}
                with torch.no_grad():
                    a, r["fused_forward_ms"] = device_ms(lambda: fused(x, gate))
                    b, r["torch_forward_ms"] = device_ms(lambda: composed(x, gate))
                grads = []
                for key, fn in (("fused", fused), ("torch", composed)):
                    xx, gg = x.clone().requires_grad_(True), gate.clone().requires_grad_(True)

                    def step():
                        fn(xx, gg).backward(dout)
                        return xx.grad
                    g, r[f"{key}_forward_backward_ms"] = device_ms(step)
                    grads.append(g)
                if i == 0:
                    # the composition in fp64 is the yardstick of both f32 forms (a million-term f32 sum by atomics has an error of its own)
                    with torch.no_grad():
                        want = composed(x.double(), gate.double()) if what != "sort" else b.double()
                    err, err_t = (float((v.double() - want).abs().max() / want.abs().max()) for v in (a, b))
                    err_g = float((grads[0] - grads[1]).abs().max() / grads[1].abs().max())
                    print(f"{name} {what}: against the composition in fp64: fused {err:.2e}, torch f32 {err_t:.2e}; dx fused against torch "
                          f"{err_g:.2e} of the largest", flush=True)
                    r0 = {"fused_rel_err_fp64": err, "torch_rel_err_fp64": err_t, "dx_fused_vs_torch": err_g}
                    if not (err <= 1e-5 and err_g <= 1e-5):
                        raise SystemExit(f"{name} {what}: the fused readout differs from the composition")
                    del want
                if i >= args.warmup:
                    rows.append(r)
                del a, b, grads
            o = row_summary(rows)
            o.update(r0, shape=name, readout=what, graphs=B, rows=N, features=F)
            for way in ("forward", "forward_backward"):
                f, t = o[f"fused_{way}_ms"]["median"], o[f"torch_{way}_ms"]["median"]
                o[f"fused_over_torch_{way}"] = f / t
                o[f"fused_{way}_spread"] = (o[f"fused_{way}_ms"]["max"] - o[f"fused_{way}_ms"]["min"]) / f
            o["fused_forward_TBps_of_x"] = 4.0 * N * F / o["fused_forward_ms"]["median"] / 1e9
            res["cases"].append(o)
            print(json.dumps(o), flush=True)
            dump_json(res, args.json)
        del x, gate, batch, gb
    res["not_measured"] = ["kernel times from a profiler (the events include the segment scan, the merge launch and torch's allocations)",
                           "bf16 storage", "the readouts inside a model step", "pitched or misaligned tables"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
