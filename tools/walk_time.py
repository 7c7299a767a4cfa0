#!/usr/bin/env python3
"""Timings of ``npi.RandomWalker`` / ``npi_walk_pairs`` / ``npi.Node2Vec.loss`` on one MI355X (EXPERIMENTS.md A48), on the NPInter2
interaction graph (``tests/golden/npinter2_folds.pt``: 5,085 nodes, every interaction in both directions) and on the benchmark's
synthetic C4 graph (``npi_gnn_amd/synth.py``: 1M nodes, 20M directed edges, Zipf hubs), for ``(p, q) = (1, 1)`` and ``(0.5, 2)``:

  * ``walks``: one walk per node, L = 80 (HIP events around the call), and the gathers per second it stands for -- three dependent
    loads per step (two of ``rowptr``, one of ``col``), the searches of the p/q bias NOT counted;
  * ``npi_walk_pairs`` over the walks of ``--pair-walks`` nodes with c = 10, S = 9 (HIP events);
  * one ``Node2Vec.loss`` forward + backward, D = 64, L = 80, c = 10, ``subset`` = 4,096 nodes (host clock ending in a synchronise;
    it includes the walks, the pair list, the pair-graph build of the backward and the aggregation).

Beside each, call by call, the same from torch device ops: for the uniform walk one ``randint`` + three gathers per step (no torch
composition of the p/q bias is timed), PyG's slicing for the pair list, and for the loss PyG's slicing + ``randint`` negatives + the
torch composition of A46 (two gathers, product, row sum, the GAE expression, autograd's ``index_add_`` backward) on given walks.

usage: python tools/walk_time.py [--steps 10] [--warmup 2] [--json OUT] [--small-only]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import npi_gnn_amd as npi                                     # noqa: E402
from npi_gnn_amd import walk as npi_walk                      # noqa: E402
from npi_gnn_amd.sampler import epoch_seed                    # noqa: E402
from npi_gnn_amd.synth import bipartite_edge_index            # noqa: E402
from _timing import device_ms, dump_json, summary, wall       # noqa: E402

EPS = 1e-15
L, C, S, D, SUBSET = 80, 10, 9, 64, 4096


def torch_walk(rowptr, col, start, length):
    """the uniform walk from torch device ops: per step one ``randint`` and the gathers of ``rowptr[v]``, ``rowptr[v + 1]``, ``col``"""
    cur, out = start, [start]
    for _ in range(length):
        lo = rowptr[cur]
        d = rowptr[cur + 1] - lo
        r = torch.randint(2 ** 31 - 1, cur.shape, device=cur.device) % d.clamp(min=1)
        cur = torch.where(d > 0, col[(lo + r).clamp(max=col.numel() - 1)], cur)
        out.append(cur)
    return torch.stack(out, 1)


def torch_windows(rw, c):
    return torch.cat([rw[:, j:j + c] for j in range(rw.size(1) + 1 - c)], dim=0)


def torch_pairs(rw, c, s, n):
    walk = torch_windows(rw, c)
    start = walk[:, 0]
    pos = torch.stack([start.view(-1, 1).expand(-1, c - 1).reshape(-1), walk[:, 1:].reshape(-1)])
    neg = torch.stack([start.view(-1, 1).expand(-1, s).reshape(-1), torch.randint(n, (walk.size(0) * s,), device=rw.device)])
    return torch.cat([pos, neg], 1), pos.size(1)


def torch_loss(z, rw, c, s, n):
    both, n_pos = torch_pairs(rw, c, s, n)
    x = (z[both[0]] * z[both[1]]).sum(1)
    return -torch.log(torch.sigmoid(x[:n_pos]) + EPS).mean() - torch.log(1 - torch.sigmoid(x[n_pos:]) + EPS).mean()


def measure(name, ei, N, args, dev):
    res = {"nodes": N, "directed_edges": int(ei.size(1))}
    every = torch.arange(N, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    subset = torch.randperm(N, device=dev, generator=gen)[:min(SUBSET, N)]
    pw = every[:min(args.pair_walks, N)]
    for p, q in ((1.0, 1.0), (0.5, 2.0)):
        _, build_ms = wall(lambda: npi.RandomWalker(ei, N, p=p, q=q))
        rw = npi.RandomWalker(ei, N, p=p, q=q, tries=args.tries)
        side = rw.side
        rowptr, col = side.rowptr.long(), side.col[:max(int(ei.size(1)), 1)].long()
        model = npi.Node2Vec(N, D, L, C, p=p, q=q).to(dev)
        with torch.no_grad():
            model.embedding.weight.mul_(0.25)
        z = model.embedding.weight
        rows = {k: [] for k in ("walks_ms", "pairs_ms", "loss_step_wall_ms", "torch_walks_ms", "torch_pairs_ms", "torch_loss_step_wall_ms")}

        def step_npi():
            model.zero_grad(set_to_none=True)
            loss = model.loss(ei, subset)
            loss.backward()
            return loss.detach()

        def step_torch(walks_sub):
            model.zero_grad(set_to_none=True)
            loss = torch_loss(z, walks_sub, C, S, N)
            loss.backward()
            return loss.detach()

        for i in range(args.warmup + args.steps):
            walks, walks_ms = device_ms(lambda: rw.walks(every, L))
            small = rw.walks(pw, L, draw=i)
            (pairs, n_pos), pairs_ms = device_ms(lambda: npi_walk.walk_pairs(small, C, S, N, epoch_seed(0, i)))
            _, loss_ms = wall(step_npi)
            t = {}
            if p == 1.0 and q == 1.0:
                _, t["torch_walks_ms"] = device_ms(lambda: torch_walk(rowptr, col, every, L))
            _, t["torch_pairs_ms"] = device_ms(lambda: torch_pairs(small, C, S, N))
            sub_walks = rw.walks(subset, L, draw=i)
            _, t["torch_loss_step_wall_ms"] = wall(lambda: step_torch(sub_walks))
            if i == 0:                                         # what was timed is a walk: every step an edge or a stay, ids in range
                a, b = walks[:, :-1].reshape(-1), walks[:, 1:].reshape(-1)
                codes = torch.unique(ei[0] * N + ei[1])
                ok = torch.isin(a * N + b, codes) | ((a == b) & (rowptr[a + 1] == rowptr[a]))
                if not bool(ok.all()) or pairs.size(1) != small.size(0) * (L + 2 - C) * (C - 1 + S):
                    raise SystemExit(f"{name}: a step of a timed walk is no edge, or the pair count is off")
            if i >= args.warmup:
                for k, v in dict(walks_ms=walks_ms, pairs_ms=pairs_ms, loss_step_wall_ms=loss_ms, **t).items():
                    rows[k].append(v)
        npi.graph.check_pending()
        out = {k: summary(v) for k, v in rows.items() if v}
        out["walker_build_wall_ms"] = build_ms
        out["walk_steps"] = N * L
        out["gathers_per_s_at_median"] = 3.0 * N * L / (out["walks_ms"]["median"] * 1e-3)
        out["pairs"] = int(pw.numel()) * (L + 2 - C) * (C - 1 + S)
        out["loss_pairs"] = int(subset.numel()) * (L + 2 - C) * (C - 1 + S)
        res[f"p={p},q={q}"] = out
        print(name, f"p={p} q={q}", json.dumps(out), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pair-walks", type=int, default=65536, help="walks whose pair list is timed (the first ids; clamped to N)")
    ap.add_argument("--tries", type=int, default=128,
                    help="of the timed walker: with p = 0.5, q = 2 a step far from the previous node accepts 1 attempt in 4, so 64 tries "
                         "run out once in 1e8 steps -- about once per call at 80M steps -- and the status word reports it")
    ap.add_argument("--small-only", action="store_true", help="the NPInter2 graph only")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "npinter2_folds.pt"), map_location="cpu", weights_only=False)
    pairs = fx["pairs"].long()[fx["label"].long() == 1].t().contiguous()
    ei = torch.cat([pairs, pairs.flip(0)], 1).to(dev)
    res = {"npinter2": measure("npinter2", ei, int(fx["num_nodes"]), args, dev)}
    if not args.small_only:
        res["c4"] = measure("c4", bipartite_edge_index(1_000_000, 20_000_000, seed=20260310).to(dev), 1_000_000, args, dev)
    res.update(steps=args.steps, walk_length=L, context_size=C, num_negative_samples=S, embedding_dim=D, subset=SUBSET,
               not_measured=["kernel times from a profiler", "the memory traffic of the walk kernel", "a torch composition of the p/q bias",
                             "walks_per_node > 1", "another box"])
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
