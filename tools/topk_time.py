#!/usr/bin/env python3
"""Timings of ``npi.topk_links`` on one MI355X (EXPERIMENTS.md A52): for every query row the ``k`` best targets without its known
edges, on

  * ``large``:    65,536 queries x 1,048,576 targets, ``F = 64``, ``k = 32``, 20 excluded targets per query (``randn`` tables),
  * ``npinter2``: the NPInter2 graph of ``tests/golden`` -- every ncRNA (4,636) against every protein (449) on fold 0's node2vec
    embeddings (``F = 64``), the positive pairs excluded, ``k = 32``.

Per shape it reports, alternating call by call,
  * the device call (HIP events around ``topk_links`` with a ``KnownLinks`` built beforehand: the tile kernel and the merge, its
    workspace allocation from torch's cache included) and the f32 TFLOP/s that time means (``2 R n_dst F`` flops),
  * the torch composition on the same tables: chunked ``z_src[chunk] @ z_dst.T``, ``index_put_`` of ``-inf`` at the known edges,
    ``torch.topk`` -- HIP events around all chunks, for every chunk size of ``--chunks``; the fastest chunk size is the one quoted.
The first call checks the two against each other: the scores position by position, and how many rows have the same ids (torch's
product rounds in another order and breaks ties its own way, so near-ties may swap).

usage: python tools/topk_time.py [--steps 5] [--warmup 1] [--shapes large npinter2] [--chunks 512 2048 8192] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import npi_gnn_amd as npi                                     # noqa: E402
from _timing import device_ms, dump_json, row_summary         # noqa: E402


def torch_topk(z_src, z_dst, k, ex_src, ex_dst, ex_ptr, chunk):
    """chunked dense scores -> -inf at the known edges (sorted by source: ex_ptr[i] is the first edge of source i) -> torch.topk"""
    out_s, out_i = [], []
    zt = z_dst.t()
    for a in range(0, z_src.size(0), chunk):
        b = min(a + chunk, z_src.size(0))
        s = z_src[a:b] @ zt
        lo, hi = int(ex_ptr[a]), int(ex_ptr[b])
        if hi > lo:
            s.index_put_((ex_src[lo:hi] - a, ex_dst[lo:hi]), s.new_tensor(float("-inf")))
        v, i = torch.topk(s, k, dim=1)
        out_s.append(v)
        out_i.append(i)
    return torch.cat(out_s), torch.cat(out_i)


def make(shape, dev):
    """``(z_src, z_dst, known edges [2, E] sorted by source, k)``"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    if shape == "large":
        R, n_dst, F, k, deg = 65536, 1 << 20, 64, 32, 20
        z_src = torch.randn(R, F, device=dev, generator=gen)
        z_dst = torch.randn(n_dst, F, device=dev, generator=gen)
        src = torch.arange(R, device=dev).repeat_interleave(deg)
        dst = torch.randint(0, n_dst, (R * deg,), device=dev, generator=gen)
        return z_src, z_dst, torch.stack([src, dst]), k
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "npinter2_folds.pt"), map_location="cpu", weights_only=False)
    pairs, label = fx["pairs"].long(), fx["label"].long()
    rna, protein = torch.unique(pairs[:, 0]), torch.unique(pairs[:, 1])
    z = fx["fold0"]["node2vec"].float()
    local = torch.full((int(fx["num_nodes"]),), -1, dtype=torch.int64)
    local[rna] = torch.arange(rna.numel())
    local_p = torch.full_like(local, -1)
    local_p[protein] = torch.arange(protein.numel())
    pos = pairs[label == 1]
    e = torch.stack([local[pos[:, 0]], local_p[pos[:, 1]]])
    e = e[:, torch.argsort(e[0], stable=True)]
    return z[rna].contiguous().to(dev), z[protein].contiguous().to(dev), e.to(dev), 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", nargs="+", default=["large", "npinter2"], choices=["large", "npinter2"])
    ap.add_argument("--chunks", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"steps": args.steps, "cases": {}}
    for shape in args.shapes:
        z_src, z_dst, e, k = make(shape, dev)
        R, n_dst, F = z_src.size(0), z_dst.size(0), z_src.size(1)
        known = npi.KnownLinks(e, (R, n_dst))
        ex_ptr = torch.searchsorted(e[0].contiguous(), torch.arange(R + 1, device=dev)).cpu()
        chunks = [c for c in args.chunks if c * n_dst * 4 <= 48 * 2 ** 30] or [min(args.chunks)]
        rows = []
        for i in range(args.warmup + args.steps):
            (s, ids), ms = device_ms(lambda: npi.topk_links((z_src, z_dst), k, exclude=known))
            row = {"topk_links_ms": ms, "topk_links_tflops": 2.0 * R * n_dst * F / (ms * 1e-3) / 1e12}
            for c in chunks:
                (ts, ti), row[f"torch_chunk_{c}_ms"] = device_ms(lambda: torch_topk(z_src, z_dst, k, e[0], e[1], ex_ptr, c))
                if i == 0:
                    same = (ti == ids).all(dim=1)
                    d = float((ts - s).abs().max())
                    print(f"{shape}: rows with the same ids as torch (chunk {c}): {int(same.sum())} of {R}; largest score difference "
                          f"{d:.2e}", flush=True)
                    if not d <= 1e-3:                 # (both lists are sorted: near-ties swap ids, not the scores of a position)
                        raise SystemExit(f"{shape}: differs from the torch composition")
                del ts, ti
            if i >= args.warmup:
                rows.append(row)
        npi.graph.check_pending()
        summ = row_summary(rows)
        best = min((c for c in chunks), key=lambda c: summ[f"torch_chunk_{c}_ms"]["median"])
        summ["fastest_torch_chunk"] = best
        res["cases"][shape] = dict(summ, R=R, n_dst=n_dst, F=F, k=k, excluded=int(e.size(1)))
        print(f"{shape}: " + ", ".join(f"{key} {v['median']:.3f} [{v['min']:.3f}, {v['max']:.3f}]" for key, v in summ.items()
                                       if isinstance(v, dict)) + f"; fastest torch chunk {best}", flush=True)
        del z_src, z_dst, known, s, ids
        torch.cuda.empty_cache()
    res["not_measured"] = ["kernel times from a profiler", "the edge-list form of exclude (a sort per call)", "other k, F and splits",
                           "GAE.predict / InnerProductDecoder.topk (a sigmoid more)"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
