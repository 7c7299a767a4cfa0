#!/usr/bin/env python3
"""Timings of the enclosing-subgraph extraction on one MI355X (EXPERIMENTS.md A61): ``--keys`` positive columns of the NPInter2 graph
(``tests/golden/npinter2_graph.pt``: 5,085 nodes, 41,648 directed columns), drawn with ``default_rng(0)``, at ``h = 1`` and ``h = 2``.

Per ``h`` it reports, the forms alternating step by step:
  * (r)  ``EnclosingSubgraphs.batch(keys)``: with its one device read of the totals -- host clock, the read synchronises;
  * (k)  ``batch(keys, n_nodes=, n_edges=)``: the totals passed, nothing read back -- HIP events and host clock; and the HIP events of
         its entry points one by one (``npi_enclose_sizes``, ``npi_enclose_fill``, ``npi_drnl_label``, ``npi_enclose_features``);
  * (s)  ``InteractionGraph.batch`` over the same keys with its totals passed: the reference's one-hop star, so less output -- context,
         not a bar;
  * (n)  one ``Net_1`` training step (forward, loss, backward) on the batch of (k);
  * (p)  the host reference of Rule H (``tests/_enclose_ref.py``) over the same keys, once.
The first step checks (k) against (p): node ids, edges, labels.

usage: python tools/enclose_time.py [--steps 10] [--warmup 3] [--keys 200] [--hops 1 2] [--json OUT]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import enclose as NE                         # noqa: E402
from npi_gnn_amd import net1 as N1                            # noqa: E402
from npi_gnn_amd.subgraph import InteractionGraph             # noqa: E402
import _enclose_ref as ref                                    # noqa: E402
from _timing import TimedLib, device_ms, dump_json, row_summary, wall   # noqa: E402


def two_colouring(ei, N):
    """0 / 1 per node such that every column joins the two colours (an isolated node: 0), or None when the graph has an odd cycle"""
    nbrs = [[] for _ in range(N)]
    for j, i in zip(ei[0].tolist(), ei[1].tolist()):
        nbrs[i].append(j)
    colour = np.full(N, -1, dtype=np.int64)
    for root in range(N):
        if colour[root] >= 0:
            continue
        colour[root] = 0
        level = [root]
        while level:
            nxt = []
            for w in level:
                for j in nbrs[w]:
                    if colour[j] < 0:
                        colour[j] = 1 - colour[w]
                        nxt.append(j)
                    elif colour[j] == colour[w]:
                        return None
            level = nxt
    return colour


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keys", type=int, default=200)
    ap.add_argument("--hops", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "npinter2_graph.pt"), map_location="cpu", weights_only=False)
    ei, feat = fx["edge_index"].long(), fx["x"].float()
    N, E = int(feat.size(0)), int(ei.size(1))
    cols = np.random.default_rng(0).choice(E, size=args.keys, replace=False)
    keys = ei[:, torch.from_numpy(cols)].t().contiguous()
    res = {"nodes": N, "columns": E, "keys": args.keys, "steps": args.steps, "warmup": args.warmup, "rows": []}

    # the star over the same keys: it wants (rna, protein) pairs, i.e. a two-colouring of the graph
    star = None
    colour = two_colouring(ei.numpy(), N)
    if colour is not None:
        colour = torch.from_numpy(colour)
        pairs = ei[:, colour[ei[0]] == 0].t().contiguous()
        ig = InteractionGraph(pairs.to(dev), torch.ones(pairs.size(0), dtype=torch.bool, device=dev), feat.to(dev), N)
        skeys = torch.where((colour[keys[:, 0]] == 0).view(-1, 1), keys, keys.flip(1))
        sn, sp = ig.sizes(skeys)
        star = (ig, skeys.to(dev), int(sn.sum()), int(sp.sum()))
        res["star"] = {"rows": int(sn.sum()), "directed_edges": 2 * int(sp.sum())}

    plain_load = NE.load
    timed = TimedLib(plain_load(), "npi_")
    for h in args.hops:
        enc = npi.EnclosingSubgraphs(ei.to(dev), N, num_hops=h, feat=feat.to(dev), target_edge="add")
        nodes, edges = enc.sizes(keys)
        n, e = int(nodes.sum()), int(edges.sum())
        dkeys = keys.to(dev)
        t0 = time.perf_counter()
        want = ref.extract(ei.numpy(), N, keys.numpy(), h, None, "add")
        p_ms = 1e3 * (time.perf_counter() - t0)
        model = N1.Net_1(1 + feat.size(1)).to(dev).train()
        y = (torch.arange(args.keys, device=dev) % 2).long()

        def net_step(gb):
            model.zero_grad(set_to_none=True)
            torch.nn.functional.nll_loss(model(gb), y).backward()

        rows, parts = [], []
        for i in range(args.warmup + args.steps):
            r = {}
            _, r["r_wall_ms"] = wall(lambda: enc.batch(dkeys))
            (b, r["k_ms"]) = device_ms(lambda: enc.batch(dkeys, n_nodes=nodes, n_edges=edges))
            _, r["k_wall_ms"] = wall(lambda: enc.batch(dkeys, n_nodes=nodes, n_edges=edges))
            NE.load = lambda: timed                             # events around every entry point of this one call
            enc.batch(dkeys, n_nodes=nodes, n_edges=edges)
            NE.load = plain_load
            part = {k: v for k, v in timed.take().items() if "enclose" in k or "drnl" in k}
            if star is not None:
                _, r["s_ms"] = device_ms(lambda: star[0].batch(star[1], n_nodes=star[2], n_pairs=star[3]))
            _, r["n_ms"] = device_ms(lambda: net_step(b.graph_batch))
            if i == 0:
                for name in ("node_id", "z", "dist", "e_id"):
                    if not torch.equal(getattr(b, name).cpu(), torch.from_numpy(want[name])):
                        raise SystemExit(f"h={h}: {name} differs from the host reference")
                if not torch.equal(b.graph_batch.edge_index.cpu(), torch.from_numpy(want["edge_index"])):
                    raise SystemExit(f"h={h}: edge_index differs from the host reference")
                print(f"h={h}: {n} rows, {e} directed edges in {args.keys} samples (checked against the host reference)", flush=True)
            if i >= args.warmup:
                rows.append(r)
                parts.append(part)
        o = row_summary(rows)
        o.update(hops=h, rows=n, directed_edges=e, max_rows=int(nodes.max()), max_edges=int(edges.max()), host_reference_ms=p_ms,
                 entry_points_ms=row_summary(parts), workspace_bytes=NE.workspace_bytes(N, args.keys),
                 extraction_slower_than_net1_step=bool(o["k_ms"]["median"] > o["n_ms"]["median"]),
                 host_reference_over_k=p_ms / o["k_wall_ms"]["median"])
        res["rows"].append(o)
        print(json.dumps(o), flush=True)
        dump_json(res, args.json)
    npi.graph.check_pending()
    res["not_measured"] = ["kernel times from a profiler", "graphs other than NPInter2", "h = 3", "an LDS-resident bitmap path",
                           "Net_1 accuracy on these batches"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
