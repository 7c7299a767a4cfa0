#!/usr/bin/env python3
"""Timings of DropEdge on one MI355X (EXPERIMENTS.md A59): ``N`` nodes, ``E`` edges with uniform random ends plus the appended self
loops -- and the same with one hub row of ``--hub`` further in-edges -- at ``F`` float32 features.

Per shape and ``p`` it reports, HIP events around each form, the forms alternating step by step:
  * (f)   ``CSRGraph.drop_edges`` of both sides (``npi_csr_drop_side`` twice, into the arrays of the previous step: ``out=``);
  * (t)   the torch route: ``rand`` mask, ``edge_index[:, mask]`` and the ``CSRGraph`` rebuild of both sides (two radix sorts);
  * (s)   one ``SAGEConv`` forward + backward (dX, dW, db) on the parent;
  * (s_p) the same step on the dropped graph;
  * (c)   a ``copy_`` that reads and writes as many bytes as the byte model of (f) says the compaction moves (half of them read, half
          written): the yardstick for (f).
The byte model of one side with ``nnz`` entries of which ``kept`` stay, over ``N`` rows: the count pass reads ``eid`` (4 B an entry;
12 B undirected), the write pass reads ``eid``, ``rowidx``, ``col`` (12 B) and writes the three kept arrays (12 B a kept entry), the
row passes read ``rowptr`` twice and write ``rowptr_o`` once (12 B a row), ``item_row`` and the tile counts are below 0.1 B an entry.
The first step checks (f) against the reference mask: the kept count of both sides.

usage: python tools/dropedge_time.py [--steps 5] [--warmup 2] [--nodes N --edges E] [--hub 400000] [--features 256] [--p 0.2 0.5]
                                     [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from _timing import device_ms, dump_json, row_summary         # noqa: E402


def model_bytes(nnz, kept, N, undirected=False):
    """bytes one ``npi_csr_drop_side`` call has to move"""
    return nnz * ((12 if undirected else 4) + 12) + kept * 12 + (N + 1) * 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--hub", type=int, default=400_000, help="in-edges of the one hub row of the second shape (0: no hub shape)")
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--p", type=float, nargs="+", default=[0.2, 0.5])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    N, E, F = args.nodes, args.edges, args.features
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    base = torch.stack([torch.randint(N, (E,), device=dev, generator=gen), torch.randint(N, (E,), device=dev, generator=gen)])
    shapes = [("uniform", base)]
    if args.hub > 0:
        extra = torch.stack([torch.randint(1, N, (args.hub,), device=dev, generator=gen), torch.zeros(args.hub, dtype=torch.int64, device=dev)])
        shapes.append(("hub", torch.cat([base, extra], dim=1)))
    res = {"nodes": N, "edges": E, "hub": args.hub, "features": F, "steps": args.steps, "warmup": args.warmup, "rows": []}
    conv = npi.SAGEConv(F, F).to(dev)
    x = torch.randn(N, F, device=dev, generator=gen).requires_grad_(True)
    go = torch.randn(N, F, device=dev, generator=gen)

    def step(graph):
        x.grad = None
        conv.zero_grad(set_to_none=True)
        conv(x, graph).backward(go)

    for name, ei in shapes:
        parent = npi.CSRGraph(ei, N)
        parent.by_src
        nnz = parent.nnz()
        hub = parent.by_dst.hub_plan() is not None
        for p in args.p:
            prev, rows = None, []
            buf = None
            for i in range(args.warmup + args.steps):
                r = {}
                prev, r["f_ms"] = device_ms(lambda: parent.drop_edges(p, seed=0, draw=i, out=prev))

                def torch_route():
                    mask = torch.rand(ei.size(1), device=dev) >= p
                    g = npi.CSRGraph(ei[:, mask], N)
                    g.by_src
                    return g
                fresh, r["t_ms"] = device_ms(torch_route)
                del fresh
                _, r["s_ms"] = device_ms(lambda: step(parent))
                _, r["sp_ms"] = device_ms(lambda: step(prev))
                if buf is None:
                    kept = int(prev.by_dst.rowptr[-1])
                    assert kept == int(prev.by_src.rowptr[-1])
                    mask = npi.drop_edge_mask(ei, p, seed=0, draw=i)
                    want = int((mask & (ei[0] != ei[1])).sum()) + N
                    if kept != want:
                        raise SystemExit(f"{name} p={p}: drop_edges kept {kept} entries, the mask says {want}")
                    total = 2 * model_bytes(nnz, kept, N)
                    buf = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)
                    print(f"{name} p={p}: {nnz} entries, {kept} kept (checked against drop_edge_mask); model {total / 1e6:.1f} MB for both sides",
                          flush=True)
                _, r["c_ms"] = device_ms(lambda: buf[0].copy_(buf[1]))
                if i >= args.warmup:
                    rows.append(r)
            o = row_summary(rows)
            f, s, sp, c = (o[k]["median"] for k in ("f_ms", "s_ms", "sp_ms", "c_ms"))
            o.update(shape=name, p=p, entries=nnz, kept=kept, parent_has_hub_plan=hub, model_bytes_both_sides=total,
                     f_GBps_of_model_bytes=total / f / 1e6, f_over_copy=f / c, f_over_t=f / o["t_ms"]["median"],
                     sp_plus_f_ms=sp + f, sp_plus_f_below_s=bool(sp + f < s), f_spread=(o["f_ms"]["max"] - o["f_ms"]["min"]) / f)
            res["rows"].append(o)
            print(json.dumps(o), flush=True)
            dump_json(res, args.json)
            del prev, buf
        del parent
    npi.graph.check_pending()
    res["not_measured"] = ["kernel times from a profiler (the events include the scan's three launches and write_item_rows)",
                           "undirected mode", "64-entry items at this size", "GATConv / GCNConv / max steps on the dropped graph"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
