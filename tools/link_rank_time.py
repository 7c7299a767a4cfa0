#!/usr/bin/env python3
"""Timings of ``npi.link_ranks`` on one MI355X (EXPERIMENTS.md A53): for every query pair the filtered counts of Rule F, on the two
shapes of ``tools/topk_time.py`` (A52)

  * ``large``:    65,536 queries (source ``i`` with a random target) x 1,048,576 targets, ``F = 64``, 20 excluded targets per source
    (``randn`` tables),
  * ``npinter2``: the NPInter2 graph of ``tests/golden`` -- every positive pair (10,412) ranked against every protein (449) on fold
    0's node2vec embeddings (``F = 64``), the positive pairs excluded.

Per shape it reports, alternating call by call,
  * ``link_ranks`` (HIP events around the call with a ``KnownLinks`` built beforehand: the tile kernel and the finishing kernel, the
    workspace allocation from torch's cache included) and the f32 TFLOP/s that time means (``2 Q n_dst F`` flops),
  * ``topk_links(k=32)`` on the same tables, with the queries' sources as its rows: the same scan with the selecting consumer,
  * the torch composition: chunked ``z_src[src[chunk]] @ z_dst.T``, ``index_put_`` of ``-inf`` at the known edges and at the target,
    compare-and-sum against the gathered target score -- HIP events around all chunks, for every chunk size of ``--chunks``.
The first call checks ``link_ranks`` against the composition: torch's product rounds in another order, so ``greater`` may differ
where a competitor scores within rounding of the target; the number of such queries is printed.

The criterion (``large``): the median of ``link_ranks`` does not exceed the median of ``topk_links`` of the same run by more than the
wider of the two min-max ranges.  ``npinter2`` is recorded, not judged (A52: launch-bound).

usage: python tools/link_rank_time.py [--steps 5] [--warmup 1] [--shapes large npinter2] [--chunks 2048 8192] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import npi_gnn_amd as npi                                     # noqa: E402
from _timing import device_ms, dump_json, row_summary         # noqa: E402
from topk_time import make                                    # noqa: E402


def torch_ranks(z_src, z_dst, src, dst, ex_row, ex_dst, ex_ptr, chunk):
    """chunked dense scores of the queries' sources -> -inf at the known edges (one entry per (query, known edge of its source),
    sorted by query: ex_ptr[i] is the first entry of query i) and at the target -> how many scores lie above / equal the target's"""
    greater, equal = [], []
    zt = z_dst.t()
    for a in range(0, src.numel(), chunk):
        b = min(a + chunk, src.numel())
        s = z_src[src[a:b]] @ zt
        mine = s.gather(1, dst[a:b, None])
        lo, hi = int(ex_ptr[a]), int(ex_ptr[b])
        if hi > lo:
            s.index_put_((ex_row[lo:hi] - a, ex_dst[lo:hi]), s.new_tensor(float("-inf")))
        s.scatter_(1, dst[a:b, None], float("-inf"))
        greater.append((s > mine).sum(1))
        equal.append((s == mine).sum(1))
    return torch.cat(greater), torch.cat(equal)


def queries(shape, e, R, n_dst, dev):
    """``[2, Q]`` query pairs"""
    if shape == "large":
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        return torch.stack([torch.arange(R, device=dev), torch.randint(0, n_dst, (R,), device=dev, generator=gen)])
    return e.clone()                                           # the positives themselves: known edges ranked against the non-edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", nargs="+", default=["large", "npinter2"], choices=["large", "npinter2"])
    ap.add_argument("--chunks", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"steps": args.steps, "cases": {}}
    for shape in args.shapes:
        z_src, z_dst, e, k = make(shape, dev)
        R, n_dst, F = z_src.size(0), z_dst.size(0), z_src.size(1)
        known = npi.KnownLinks(e, (R, n_dst))
        q = queries(shape, e, R, n_dst, dev)
        Q = int(q.size(1))
        src, dst = q[0].contiguous(), q[1].contiguous()
        # the known edges of the sources of query rows a .. b - 1, as (row within the queries, column): one entry per (query, edge)
        deg = torch.bincount(e[0], minlength=R)
        first = torch.cumsum(deg, 0) - deg
        per_q = deg[src]
        ex_ptr = torch.cat([per_q.new_zeros(1), torch.cumsum(per_q, 0)])
        owner = torch.repeat_interleave(torch.arange(Q, device=dev), per_q)
        ex_dst = e[1][first[src][owner] + (torch.arange(owner.numel(), device=dev) - ex_ptr[owner])]
        ex_ptr_h = ex_ptr.cpu()
        chunks = [c for c in args.chunks if c * n_dst * 4 <= 48 * 2 ** 30] or [min(args.chunks)]
        rows = []
        for i in range(args.warmup + args.steps):
            r, ms = device_ms(lambda: npi.link_ranks((z_src, z_dst), q, exclude=known))
            row = {"link_ranks_ms": ms, "link_ranks_tflops": 2.0 * Q * n_dst * F / (ms * 1e-3) / 1e12}
            _, row["topk_links_ms"] = device_ms(lambda: npi.topk_links((z_src, z_dst), k, exclude=known, rows=src))
            for c in chunks:
                (tg, te), row[f"torch_chunk_{c}_ms"] = device_ms(lambda: torch_ranks(z_src, z_dst, src, dst, owner, ex_dst, ex_ptr_h, c))
                if i == 0:
                    off = (tg != r.greater) | (te != r.equal)
                    far = ((tg + te - r.greater - r.equal).abs() > 3) | ((tg - r.greater).abs() > 3)
                    print(f"{shape}: queries whose counts differ from torch's (chunk {c}): {int(off.sum())} of {Q}, by more than 3: "
                          f"{int(far.sum())}", flush=True)
                    if int(far.sum()):
                        raise SystemExit(f"{shape}: differs from the torch composition")
                del tg, te
            if i >= args.warmup:
                rows.append(row)
        npi.graph.check_pending()
        summ = row_summary(rows)
        best = min((c for c in chunks), key=lambda c: summ[f"torch_chunk_{c}_ms"]["median"])
        summ["fastest_torch_chunk"] = best
        lr, tk = summ["link_ranks_ms"], summ["topk_links_ms"]
        slack = max(lr["max"] - lr["min"], tk["max"] - tk["min"])
        summ["ratio_to_topk_links"] = lr["median"] / tk["median"]
        summ["criterion_met"] = bool(lr["median"] <= tk["median"] + slack)
        res["cases"][shape] = dict(summ, Q=Q, n_dst=n_dst, F=F, k=k, excluded=int(e.size(1)))
        print(f"{shape}: " + ", ".join(f"{key} {v['median']:.3f} [{v['min']:.3f}, {v['max']:.3f}]" for key, v in summ.items()
                                       if isinstance(v, dict)) + f"; fastest torch chunk {best}; link_ranks / topk_links "
              f"{summ['ratio_to_topk_links']:.3f}; criterion met: {summ['criterion_met']}", flush=True)
        del z_src, z_dst, known, r
        torch.cuda.empty_cache()
    res["not_measured"] = ["kernel times from a profiler", "the edge-list form of exclude (a sort per call)", "other F and splits",
                           "GAE.test_ranking / ranking_metrics (a handful of reductions over [Q] more)"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
