#!/usr/bin/env python3
"""Timings of ``npi.rank_metrics`` on one MI355X (EXPERIMENTS.md A49): ROC-AUC and average precision of ``M`` float32 scores that
are already on the device, ``M = 2^20`` and ``2^24``, about 30 % positives, with

  * ``distinct``: ``M`` different scores (a shuffled ramp: every tie group has one member, the curve has ``M`` points),
  * ``tied``:     float32 ``sigmoid(8 randn)`` quantised to 1,024 levels (heavy ties: the curve has about a thousand points).

Per case it reports, alternating call by call,
  * the device call (HIP events around ``rank_metrics``: the key kernel, the sort, the two passes, the curve's reduction; its
    workspace allocation from torch's cache included),
  * a composition of torch device ops for the same two numbers -- ``sort(descending)``, ``cumsum`` of the gathered labels, the group
    ends by comparing neighbours, ``nonzero`` (a host read inside), then the trapezoid and the precision / recall sum in float64 --
    by a host clock around it, ending in a synchronise,
  * sklearn on the host, INCLUDING the copy of scores and labels (``roc_auc_score`` + ``average_precision_score``: two sorts), by a
    host clock; ``--no-sklearn`` or a missing sklearn leaves it out and the output says so.
The first call of every case checks the three against each other.

usage: python tools/rank_time.py [--steps 10] [--warmup 2] [--sizes 1048576 16777216] [--no-sklearn] [--json OUT]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npi_gnn_amd as npi                                     # noqa: E402
from _timing import device_ms, dump_json, row_summary, wall   # noqa: E402


def torch_metrics(scores, y):
    """the same two numbers from torch device ops (sklearn's algorithm line by line)"""
    s, order = torch.sort(scores, descending=True, stable=True)
    tp_all = torch.cumsum(y[order], 0)
    end = torch.ones_like(s, dtype=torch.bool)
    end[:-1] = s[:-1] != s[1:]
    idx = end.nonzero().squeeze(1)
    tps = tp_all[idx].double()
    fps = (idx + 1).double() - tps
    P, N = tps[-1], fps[-1]
    zero = tps.new_zeros(1)
    tpr, fpr = torch.cat([zero, tps]) / P, torch.cat([zero, fps]) / N
    auc = torch.trapz(tpr, fpr)
    recall = tps / P
    ap = ((recall - torch.cat([zero, recall[:-1]])) * (tps / (tps + fps))).sum()
    return auc, ap


def make(kind, M, dev, gen):
    if kind == "distinct":
        scores = (torch.randperm(M, device=dev, generator=gen).float() - M / 2) / M        # M <= 2^24: exact in float32
    else:
        scores = torch.round(torch.sigmoid(8 * torch.randn(M, device=dev, generator=gen)) * 1023) / 1023
    y = (torch.rand(M, device=dev, generator=gen) < 0.3 + 0.2 * scores).long()              # the labels lean on the scores
    return scores.contiguous(), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    skm = None
    if not args.no_sklearn:
        try:
            import sklearn.metrics as skm
        except ImportError:
            print("sklearn is not importable here: the host baseline is left out", flush=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"steps": args.steps, "sklearn": bool(skm), "cases": {}}
    for M in args.sizes:
        for kind in ("distinct", "tied"):
            scores, y = make(kind, M, dev, gen)
            rows = []
            for i in range(args.warmup + args.steps):
                (auc, ap_), ms = device_ms(lambda: npi.rank_metrics(scores, y))
                (t_auc, t_ap), torch_ms = wall(lambda: torch_metrics(scores, y))
                row = {"rank_metrics_ms": ms, "torch_sort_cumsum_wall_ms": torch_ms}
                if skm is not None:
                    def host():
                        s, l = scores.cpu().numpy(), y.cpu().numpy()
                        return skm.roc_auc_score(l, s), skm.average_precision_score(l, s)
                    (s_auc, s_ap), row["sklearn_with_copy_wall_ms"] = wall(host)
                if i == 0:
                    pairs = [("torch", float(t_auc), float(t_ap))] + ([("sklearn", s_auc, s_ap)] if skm is not None else [])
                    for name, a, p in pairs:
                        da, dp = abs(float(auc) - a), abs(float(ap_) - p)
                        print(f"M={M} {kind}: auc {float(auc):.12f} ap {float(ap_):.12f}; against {name}: |d auc| = {da:.1e}, "
                              f"|d ap| = {dp:.1e}", flush=True)
                        if not (da <= 1e-9 and dp <= 1e-9):
                            raise SystemExit(f"M={M} {kind}: differs from {name}")
                if i >= args.warmup:
                    rows.append(row)
            npi.graph.check_pending()
            res["cases"][f"{kind}_{M}"] = row_summary(rows)
            print(f"M={M} {kind}: " + ", ".join(f"{k} {v['median']:.3f}" for k, v in res["cases"][f"{kind}_{M}"].items()), flush=True)
    res["not_measured"] = ["kernel times from a profiler", "the curve functions (roc_curve / precision_recall_curve)", "GAE.test",
                           "sizes other than --sizes", "the n_pos form"]
    print(json.dumps(res, indent=1), flush=True)
    dump_json(res, args.json)


if __name__ == "__main__":
    main()
