#!/usr/bin/env python3
"""Timings of the listwise link loss on one MI355X (EXPERIMENTS.md A58): ``Q`` positive pairs, float32 tables ``z_src [n_src, F]``
and ``z_dst [n_dst, F]``, the positives themselves as the known edges (a ``KnownLinks`` built beforehand).

Per shape it reports, forward and backward apart, HIP events around each call, the forms alternating call by call:
  * (f) ``npi.listwise_loss`` and its backward (to both tables), and inside them the three scans of ``npi_softmax_link_*`` one by
        one (events around each entry point: ``_timing.TimedLib``) with their f32 flop rates -- ``2 Q n_dst F`` for the scores of
        every scan, as much again for the second stage of the two backward scans;
  * (a) the torch composition: ``scale * z_src[src] @ z_dst.t()`` plus a dense additive mask (built beforehand, outside the timed
        region), ``F.cross_entropy`` against the targets, and autograd's backward of exactly that.
The first step of every shape checks (f) against (a): the loss and both gradients to 1e-4 of their largest magnitude (torch's
product rounds in another order and its backward adds with float atomics).  Next to the medians it prints (a)'s peak memory beside
(f)'s workspace.

usage: python tools/softmax_link_time.py [--steps 5] [--warmup 2] [--shapes npinter2-64 npinter2-256 wide] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import softmax_link as SL                    # noqa: E402
from _timing import TimedLib, device_ms, dump_json, row_summary         # noqa: E402

SHAPES = {"npinter2-64": (4636, 449, 16658, 64), "npinter2-256": (4636, 449, 16658, 256), "wide": (4096, 100_000, 4096, 128)}
SCALE = 0.125
PEAK_TF = 157.0                                               # f32, matrix and vector alike


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    lib = TimedLib(npi.load(), "npi_softmax_link")
    SL.load = lambda: lib
    res = {"steps": args.steps, "warmup": args.warmup, "scale": SCALE, "shapes": []}
    for name in args.shapes:
        n_src, n_dst, Q, F = SHAPES[name]
        zs = torch.randn(n_src, F, device=dev, generator=gen)
        zd = torch.randn(n_dst, F, device=dev, generator=gen)
        pos = torch.stack([torch.randint(n_src, (Q,), device=dev, generator=gen), torch.randint(n_dst, (Q,), device=dev, generator=gen)])
        known = npi.KnownLinks(pos, (n_src, n_dst))
        mask = torch.zeros((n_src, n_dst), device=dev)
        mask[pos[0], pos[1]] = float("-inf")
        mask = mask[pos[0]]                                    # [Q, n_dst]: the other known partners of every query's source ...
        mask[torch.arange(Q, device=dev), pos[1]] = 0.0        # ... the target itself stays in
        workspace = int(npi.load().npi_softmax_link_workspace_bytes(Q, n_src, n_dst, F, 0))
        rows, peak_a = [], 0
        for i in range(args.warmup + args.steps):
            r = {}
            a, b = zs.clone().requires_grad_(True), zd.clone().requires_grad_(True)
            lib.take()
            loss_f, r["f_forward_ms"] = device_ms(lambda: npi.listwise_loss((a, b), pos, exclude=known, scale=SCALE))
            (ds, dd), r["f_backward_ms"] = device_ms(lambda: torch.autograd.grad(loss_f, (a, b)))
            for entry, ms in lib.take().items():
                r[entry.replace("npi_softmax_link_", "scan_") + "_ms"] = ms
            a2, b2 = zs.clone().requires_grad_(True), zd.clone().requires_grad_(True)
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            loss_a, r["a_forward_ms"] = device_ms(
                lambda: torch.nn.functional.cross_entropy(SCALE * (a2[pos[0]] @ b2.t()) + mask, pos[1]))
            (ds_a, dd_a), r["a_backward_ms"] = device_ms(lambda: torch.autograd.grad(loss_a, (a2, b2)))
            peak_a = max(peak_a, torch.cuda.max_memory_allocated(dev) - before)
            if i == 0:
                errs = {"loss": abs(float(loss_f.detach()) - float(loss_a.detach())) / abs(float(loss_a.detach())),
                        "dZ_src": float((ds - ds_a).abs().max() / ds_a.abs().max()),
                        "dZ_dst": float((dd - dd_a).abs().max() / dd_a.abs().max())}
                print(f"{name}: first step against the torch composition: {errs}", flush=True)
                if not all(e <= 1e-4 for e in errs.values()):
                    raise SystemExit(f"{name}: the listwise loss differs from the torch composition")
            if i >= args.warmup:
                rows.append(r)
            del a, b, a2, b2, loss_f, loss_a, ds, dd, ds_a, dd_a
        o = row_summary(rows)
        scores = 2.0 * Q * n_dst * F
        o.update(shape=name, n_src=n_src, n_dst=n_dst, Q=Q, features=F, first_step_parity=errs, score_flops_per_scan=scores,
                 a_peak_bytes=peak_a, a_matrix_bytes=4 * Q * n_dst, f_workspace_bytes=workspace)
        for scan, passes in (("scan_fwd", 1), ("scan_bwd_src", 2), ("scan_bwd_dst", 2)):
            ms = o[scan + "_ms"]["median"]
            o[scan + "_tflops"] = passes * scores / (ms * 1e-3) / 1e12
            o[scan + "_of_f32_peak"] = o[scan + "_tflops"] / PEAK_TF
        for way in ("forward", "backward"):
            f, a_ = o[f"f_{way}_ms"]["median"], o[f"a_{way}_ms"]["median"]
            o[f"f_over_a_{way}"] = f / a_
            o[f"f_{way}_spread"] = (o[f"f_{way}_ms"]["max"] - o[f"f_{way}_ms"]["min"]) / f
        res["shapes"].append(o)
        print(json.dumps(o), flush=True)
        dump_json(res, args.json)
        del zs, zd, mask, known
    npi.graph.check_pending()
    res["not_measured"] = ["kernel times from a profiler (the events of a scan include its split-sum launch)",
                           "an MFMA second stage (only the VALU form was built)", "queries grouped by source", "bf16 tables",
                           "building the dense mask of (a), which is left out of its time"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
