#!/usr/bin/env python3
"""HIP-event times of VGAE's reparametrisation + KL term (``functional.reparametrize_kl``: ``npi_gauss_sample_kl`` and its backward)
at ``[N, F]`` tables (default ``[1M, 64]`` and ``[1M, 256]``), beside the torch composition PyG runs and beside a plain device copy
that moves the same bytes:
    fused_fwd   one npi_gauss_sample_kl launch (NPI_GAUSS_SAMPLE | NPI_GAUSS_KL) plus the one-workgroup sum: 12 bytes per element
    fused_bwd   one npi_gauss_sample_kl_bwd launch with both upstream gradients: 20 bytes per element
    torch_fwd   mu + randn_like(logvar) * exp(0.5 * lv) and -0.5 * mean(sum(1 + lv - mu**2 - lv.exp(), 1)), lv = logvar.clamp(max=10)
    torch_bwd   autograd's backward of that, under the same two upstream gradients
    copy_fwd / copy_bwd   Tensor.copy_ over half of 12 / 20 bytes per element (a copy reads and writes each byte it moves)
The modes alternate inside a repeat (same box, same process).
usage: tools/bench_gauss.py [--shapes 1048576x64,1048576x256 --steps K --warmup W --repeats R --json FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from npi_gnn_amd import _lib                                         # noqa: E402
from npi_gnn_amd import functional as NF                            # noqa: E402
from _timing import dump_json, summary                              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1048576x64,1048576x256")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = _lib.load()
res = {"steps": args.steps, "repeats": args.repeats, "shapes": {}}
for shape in args.shapes.split(","):
    N, F = (int(v) for v in shape.split("x"))
    gen = torch.Generator(device=dev).manual_seed(1)
    mu = torch.randn(N, F, device=dev, generator=gen)
    logvar = torch.rand(N, F, device=dev, generator=gen) * 9 - 6
    g_z = torch.randn(N, F, device=dev, generator=gen)
    g_kl = torch.ones(1, device=dev)
    d_mu, d_lv = torch.empty_like(mu), torch.empty_like(mu)
    rule = NF.GaussianNoise(0, 0)
    src = {k: torch.empty(N * F * b // 8, dtype=torch.float32, device=dev) for k, b in (("copy_fwd", 12), ("copy_bwd", 20))}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    mu_t, lv_t = mu.clone().requires_grad_(True), logvar.clone().requires_grad_(True)
    state = {}

    def torch_fwd(grad):
        with torch.set_grad_enabled(grad):
            lv = lv_t.clamp(max=10.0)
            z = mu_t + torch.randn_like(lv) * torch.exp(0.5 * lv)
            kl = -0.5 * torch.mean(torch.sum(1 + lv - mu_t ** 2 - lv.exp(), dim=1))
        return z, kl

    def fused_bwd():
        _lib.check(lib.npi_gauss_sample_kl_bwd(mu.data_ptr(), F, logvar.data_ptr(), F, N, F, N, 10.0, rule.key, 0, 0,
                                               _lib.NPI_GAUSS_SAMPLE | _lib.NPI_GAUSS_KL, g_z.data_ptr(), F, g_kl.data_ptr(),
                                               d_mu.data_ptr(), F, d_lv.data_ptr(), F, _lib.stream_ptr(dev)), "npi_gauss_sample_kl_bwd")

    def torch_bwd_prepare():
        state["out"] = torch_fwd(True)

    def torch_bwd():
        z, kl = state["out"]
        torch.autograd.backward([z, kl], [g_z, g_kl[0]], retain_graph=True)
        mu_t.grad = lv_t.grad = None

    def fused_fwd():
        with torch.no_grad():
            NF.reparametrize_kl(mu, logvar, rule)

    modes = {"fused_fwd": fused_fwd, "fused_bwd": fused_bwd, "torch_fwd": lambda: torch_fwd(False), "torch_bwd": torch_bwd,
             "copy_fwd": lambda: dst["copy_fwd"].copy_(src["copy_fwd"]), "copy_bwd": lambda: dst["copy_bwd"].copy_(src["copy_bwd"])}
    torch_bwd_prepare()
    times = {m: [] for m in modes}
    for rep in range(args.repeats):
        for m, fn in modes.items():
            for _ in range(args.warmup):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1) / args.steps)
    bytes_of = {"fused_fwd": 12, "fused_bwd": 20, "copy_fwd": 12, "copy_bwd": 20}
    out = {m: dict(summary(v), repeats=v) for m, v in times.items()}
    for m, b in bytes_of.items():
        out[m]["GB_per_s"] = N * F * b / (out[m]["median"] * 1e-3) / 1e9
    res["shapes"][shape] = out
    state.clear()
    print(f"[{N}, {F}] |", "  ".join(f"{m} {out[m]['median']:.3f} ms" + (f" ({out[m]['GB_per_s']:.0f} GB/s)" if "GB_per_s" in out[m] else "")
                                      for m in modes))
dump_json(res, args.json)
print("RESULT " + __import__("json").dumps({s: {m: round(v["median"], 4) for m, v in o.items()} for s, o in res["shapes"].items()}))
