"""What the ``*_time.py`` tools share: the two clocks, the per-entry-point event wrapper and the shape of a result."""
import json
import os
import statistics
import time

import torch


def wall(fn):
    """``(fn(), ms)`` by the host clock, between two synchronises"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def device_ms(fn):
    """``(fn(), ms)`` by HIP events around the call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def summary(vals):
    vals = list(vals)
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def row_summary(rows):
    """a list of per-step dicts with the same keys -> ``{key: summary}``"""
    return {k: summary(r[k] for r in rows) for k in rows[0]}


def dump_json(res, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)


class TimedLib:
    """the C-ABI library with HIP events around the entry points whose names start with ``prefix`` (the size queries excepted);
    put in place of a module's ``load`` for one process"""

    def __init__(self, lib, prefix):
        self._lib, self._prefix, self.events = lib, prefix, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(self._prefix) or name.endswith(("_elems", "_bytes")):
            return fn

        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            self.events.append((name, e0, e1))
            return rc
        return timed

    def take(self):
        """ms per entry point since the last take (summed over its calls)"""
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.events:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        self.events = []
        return out
