#!/usr/bin/env python3
"""Timings of ``npi.ranking_loss`` on one MI355X (EXPERIMENTS.md A56): ``P`` positives with uniform random ends in two embedding
tables ``[N, F]`` float32 (1M rows each, so the gathers miss the caches) and ``K`` uniform random corrupted targets each.

Per shape ``(F, K)`` it reports, alternating call by call,
  * fused: ``npi.ranking_loss`` -- one ``npi_group_score`` launch plus the one-workgroup sum;
  * (a) torch: the composition from device ops -- a ``[P, F]`` and a ``[P, 1 + K, F]`` gather, their product, the row sum, the
    loss from the logits, and autograd's backward (``index_add_`` scatters with float atomics).  Skipped, and reported as not
    measured, where its tensors would not fit ``--torch-gb``;
  * (b) expanded: what the package offered before ``ranking_loss`` -- ``npi.pair_scores`` over the expanded list of ``P (1 + K)``
    pairs (the list is built outside the timed region) plus the same torch loss from the logits,
each as the forward alone (HIP events, under ``torch.no_grad()``) and as forward + backward with both tables requiring grad (host
clock around the step, ending in a synchronise; for fused and (b) this includes the build of both sides of the expanded list and
the two aggregations, which the two share).  The first step of every shape checks the three losses against each other.

usage: python tools/group_loss_time.py [--steps 5] [--warmup 2] [--rows N --groups P] [--features 64 256] [--negatives 1 8 63]
                                       [--loss softmax] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from _timing import device_ms, dump_json, row_summary, wall   # noqa: E402


def loss_from_logits(x, kind, margin, scale):
    """the torch loss of logits ``x [P, 1 + K]`` without empty slots (then the slot-count divisors are ``mean()``'s)"""
    if kind == "softmax":
        return torch.nn.functional.cross_entropy(scale * x, torch.zeros(x.size(0), dtype=torch.int64, device=x.device))
    d = scale * (x[:, 1:] - x[:, :1])
    return torch.nn.functional.softplus(d).mean() if kind == "bpr" else (margin + d).clamp(min=0).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of each table")
    ap.add_argument("--groups", type=int, default=1_048_576, help="positives")
    ap.add_argument("--features", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--negatives", type=int, nargs="+", default=[1, 8, 63])
    ap.add_argument("--loss", default="softmax", choices=sorted(npi.functional.GROUP_LOSSES))
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--torch-gb", type=float, default=100.0, help="largest footprint of the torch composition that is still run")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    N, P, kind, margin, scale = args.rows, args.groups, args.loss, args.margin, args.scale
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"loss": kind, "rows": N, "groups": P, "steps": args.steps, "shapes": []}
    for F in args.features:
        s = 0.7 * F ** -0.25                                   # logits of standard deviation 0.49, as in the tests
        zs = (torch.randn(N, F, device=dev, generator=gen) * s).requires_grad_(True)
        zd = (torch.randn(N, F, device=dev, generator=gen) * s).requires_grad_(True)
        for K in args.negatives:
            C = 1 + K
            # two gathers, their product and its gradient, each P C F floats
            torch_gb = 4.0 * P * C * F * 4 / 2 ** 30
            run_torch = torch_gb <= args.torch_gb
            rows = []

            def fused(pos, neg):
                return npi.ranking_loss((zs, zd), pos, neg, loss=kind, margin=margin, scale=scale)

            def composed(pos, neg):
                x = (zs[pos[0]][:, None, :] * zd[torch.cat([pos[1][:, None], neg], 1)]).sum(-1)
                return loss_from_logits(x, kind, margin, scale)

            def expanded(flat):
                return loss_from_logits(npi.pair_scores((zs, zd), flat).view(P, C), kind, margin, scale)

            def step(fn, *a):
                zs.grad = zd.grad = None
                loss = fn(*a)
                loss.backward()
                return loss.detach()

            for i in range(args.warmup + args.steps):
                pos = torch.stack([torch.randint(N, (P,), device=dev, generator=gen), torch.randint(N, (P,), device=dev, generator=gen)])
                neg = torch.randint(N, (P, K), device=dev, generator=gen)
                flat = torch.stack([pos[0].repeat_interleave(C), torch.cat([pos[1][:, None], neg], 1).flatten()])
                row = {}
                with torch.no_grad():
                    l0, row["fused_forward_ms"] = device_ms(lambda: fused(pos, neg))
                    l2, row["expanded_forward_ms"] = device_ms(lambda: expanded(flat))
                    if run_torch:
                        l1, row["torch_forward_ms"] = device_ms(lambda: composed(pos, neg))
                _, row["fused_step_wall_ms"] = wall(lambda: step(fused, pos, neg))
                _, row["expanded_step_wall_ms"] = wall(lambda: step(expanded, flat))
                if run_torch:
                    _, row["torch_step_wall_ms"] = wall(lambda: step(composed, pos, neg))
                if i == 0:
                    for name, other in (("expanded", l2),) + ((("torch", l1),) if run_torch else ()):
                        err = abs(float(l0) - float(other)) / max(abs(float(other)), 1e-30)
                        print(f"F={F} K={K}: fused loss {float(l0):.6f} against {name}: relative difference {err:.2e}", flush=True)
                        if not err <= 1e-4:
                            raise SystemExit(f"F={F} K={K}: the fused loss differs from the {name} composition")
                if i >= args.warmup:
                    rows.append(row)
                del flat
            out = row_summary(rows)
            out.update(features=F, negatives=K, slots=P * C, torch_composition="timed" if run_torch else
                       f"not measured: about {torch_gb:.0f} GiB of gathered rows")
            out["fused_over_expanded_forward"] = out["fused_forward_ms"]["median"] / out["expanded_forward_ms"]["median"]
            res["shapes"].append(out)
            print(json.dumps(out), flush=True)
            dump_json(res, args.json)
        del zs, zd
    npi.graph.check_pending()
    res["not_measured"] = ["kernel times from a profiler", "sixteen target rows in flight per lane", "one id space",
                           "the build of the sides and the aggregations separately", "NegativeSampler.corrupt targets (uniform ids stand in)"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
