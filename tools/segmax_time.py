#!/usr/bin/env python3
"""Timings of the max aggregation on one MI355X (EXPERIMENTS.md A57): ``N`` nodes, ``E`` edges with uniform random ends plus the
appended self loops, a float32 table ``[N, F]`` -- and the same with one hub row of ``--hub`` further in-edges.

Per shape it reports, forward and backward apart, HIP events around each call, the forms alternating call by call:
  * (f) ``npi_segmax`` / ``npi_segmax_bwd`` (``functional.segmax_side`` / ``segmax_bwd_side``);
  * (a) the torch composition: ``x.index_select(0, col)`` + ``scatter_reduce_("amax")`` forward, autograd's backward of exactly that
        (the forward graph is rebuilt outside the timed region before every backward);
  * (m) ``segsum(mean=True)`` over the by-target side and the plain transposed aggregation ``segsum(mean=False)`` over the
        by-source side: what the mean aggregator moves over the same two sides.
The first step of every shape checks (f): the maxima bit for bit against (a); the gradient to 1e-5 of its largest magnitude against
the scatter of ``dout`` to the winners ``arg`` names, and against autograd's unless the inputs hold tied maxima (autograd splits a
tied cell's gradient evenly, Rule X gives it to one entry; the tool counts the tied cells).
Next to the medians it prints the byte model's prediction of (f) / (m) and, for the hub shape, the ratio to the uniform shape
beside the ratio of their entry counts and the run-to-run spread of (f).

usage: python tools/segmax_time.py [--steps 5] [--warmup 2] [--nodes N --edges E] [--hub 400000] [--features 64 256] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import functional as NF                      # noqa: E402
from _timing import device_ms, dump_json, row_summary         # noqa: E402


def byte_model(nnz, N, F):
    """bytes the three forward / backward forms have to move (ids and rows gathered once, outputs written once)"""
    return {"max_forward": nnz * (4 * F + 8) + 8 * N * F, "max_backward": nnz * (8 * F + 12) + 4 * N * F,
            "mean_forward": nnz * (4 * F + 4) + 4 * N * F, "mean_backward": nnz * (4 * F + 4) + 4 * N * F}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=262_144)
    ap.add_argument("--edges", type=int, default=5_242_880)
    ap.add_argument("--hub", type=int, default=400_000, help="in-edges of the one hub row of the second shape (0: no hub shape)")
    ap.add_argument("--features", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    N, E = args.nodes, args.edges
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    base = torch.stack([torch.randint(N, (E,), device=dev, generator=gen), torch.randint(N, (E,), device=dev, generator=gen)])
    shapes = [("uniform", base)]
    if args.hub > 0:
        extra = torch.stack([torch.randint(1, N, (args.hub,), device=dev, generator=gen), torch.zeros(args.hub, dtype=torch.int64, device=dev)])
        shapes.append(("hub", torch.cat([base, extra], dim=1)))
    res = {"nodes": N, "edges": E, "hub": args.hub, "steps": args.steps, "warmup": args.warmup, "shapes": []}
    uniform_ms = {}
    for name, ei in shapes:
        g = npi.CSRGraph(ei, N)
        d, t = g.by_dst, g.by_src
        keep = ei[0] != ei[1]                                  # what the build keeps; then the loops
        loop = torch.arange(N, device=dev)
        col = torch.cat([ei[0][keep], loop])
        row = torch.cat([ei[1][keep], loop])
        nnz = int(col.numel())
        for F in args.features:
            x = torch.randn(N, F, device=dev, generator=gen)
            dout = torch.randn(N, F, device=dev, generator=gen)
            idx = row[:, None].expand(-1, F)

            def composed(xx):
                return torch.zeros((N, F), device=dev).scatter_reduce_(0, idx, xx.index_select(0, col), "amax", include_self=False)

            rows = []
            for i in range(args.warmup + args.steps):
                r = {}
                with torch.no_grad():
                    (out, arg), r["f_forward_ms"] = device_ms(lambda: NF.segmax_side(d, x))
                    ref, r["a_forward_ms"] = device_ms(lambda: composed(x))
                    _, r["m_forward_ms"] = device_ms(lambda: NF.segsum(g, d, x, mean=True))
                    dx, r["f_backward_ms"] = device_ms(lambda: NF.segmax_bwd_side(t, dout, arg))
                    _, r["m_backward_ms"] = device_ms(lambda: NF.segsum(g, t, dout, mean=False))
                xa = x.clone().requires_grad_(True)
                ya = composed(xa)
                (da,), r["a_backward_ms"] = device_ms(lambda: torch.autograd.grad(ya, xa, dout))
                if i == 0:
                    if not torch.equal(out, ref):
                        raise SystemExit(f"{name} F={F}: npi_segmax differs from the torch composition")
                    owner = torch.where(arg >= 0, ei[0][arg.clamp(min=0).long()], loop[:, None])
                    want = torch.zeros((N, F), device=dev).index_put_((owner, torch.arange(F, device=dev).expand(N, F)), dout, accumulate=True)
                    hits = torch.zeros((N, F), device=dev).scatter_add_(0, idx, (x.index_select(0, col) == out.index_select(0, row)).float())
                    ties = int((hits > 1).sum())
                    err, err_a = (float((dx - w).abs().max() / w.abs().max()) for w in (want, da))
                    print(f"{name} F={F}: maxima equal bit for bit; gradient against the winners' scatter {err:.2e} of the largest, against "
                          f"autograd {err_a:.2e} with {ties} tied maxima among {N * F} cells", flush=True)
                    if not err <= 1e-5 or (ties == 0 and not err_a <= 1e-5):
                        raise SystemExit(f"{name} F={F}: npi_segmax_bwd differs from the reference gradient")
                    del owner, want, hits
                if i >= args.warmup:
                    rows.append(r)
                del xa, ya, da, ref
            o = row_summary(rows)
            m = byte_model(nnz, N, F)
            o.update(shape=name, features=F, entries=nnz, bytes=m)
            for way in ("forward", "backward"):
                f, a, mm = (o[f"{k}_{way}_ms"]["median"] for k in "fam")
                o[f"f_over_a_{way}"] = f / a
                o[f"f_over_m_{way}"] = f / mm
                o[f"model_f_over_m_{way}"] = m[f"max_{way}"] / m[f"mean_{way}"]
                o[f"f_{way}_TBps_of_model_bytes"] = m[f"max_{way}"] / f / 1e9
                o[f"f_{way}_spread"] = (o[f"f_{way}_ms"]["max"] - o[f"f_{way}_ms"]["min"]) / f
                if name == "uniform":
                    uniform_ms[(F, way)] = (f, nnz)
                elif (F, way) in uniform_ms:
                    uf, un = uniform_ms[(F, way)]
                    o[f"hub_over_uniform_{way}"] = f / uf
                    o[f"hub_over_uniform_entries"] = nnz / un
            res["shapes"].append(o)
            print(json.dumps(o), flush=True)
            dump_json(res, args.json)
            del x, dout, idx
        del g, d, t
    npi.graph.check_pending()
    res["not_measured"] = ["kernel times from a profiler (the events include the empty-row fill and the chain launch)",
                           "bf16 storage", "item sizes other than the hint's", "the layer around the aggregation"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
