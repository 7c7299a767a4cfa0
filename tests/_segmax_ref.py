"""Rule X (``include/npi_gnn.h``) restated on the host, the backward in fp64, the literal torch composition and the input builders
of the max-aggregation tests.  Everything here is numpy / torch on the CPU and is computed once per argument set (``lru_cache``):
the tests share the results and leave them unchanged."""
from functools import lru_cache

import numpy as np
import torch

QNAN = np.uint32(0x7FC00000)
SIGN = np.uint32(0x80000000)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def key(v: np.ndarray) -> np.ndarray:
    """ascending-orderable uint32 of float32 values: NaN -> the quiet NaN (above +inf), -0.0 -> +0.0"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    b[(b & ~SIGN) > np.uint32(0x7F800000)] = QNAN
    b[b == SIGN] = 0
    return np.where(b & SIGN, ~b, b | SIGN).astype(np.uint32)


def value_of_key(u: np.ndarray) -> np.ndarray:
    u = u.astype(np.uint32)
    return np.where(u & SIGN, u ^ SIGN, ~u).astype(np.uint32).view(np.float32)


def entries(src, dst, n_dst: int, self_loops: bool):
    """(row, col, eid) of the by-target side's entries, rows ascending: the edge list's columns (with ``self_loops`` the ``(i, i)``
    columns dropped, as ``add_remaining_self_loops`` does) and then one loop entry per node with eid -1"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    eid = np.arange(src.size, dtype=np.int64)
    if self_loops:
        keep = src != dst
        src, dst, eid = src[keep], dst[keep], eid[keep]
        loop = np.arange(n_dst, dtype=np.int64)
        src, dst, eid = np.concatenate([src, loop]), np.concatenate([dst, loop]), np.concatenate([eid, np.full(n_dst, -1)])
    order = np.argsort(dst, kind="stable")
    return dst[order], src[order], eid[order]


def rule_x(x: torch.Tensor, src, dst, n_dst: int, self_loops: bool):
    """``(out f32 [n_dst, F], arg int32 [n_dst, F])``: per cell the largest word (key of the value, ~uint32(eid)) of the row's entries"""
    xn = x.detach().cpu().numpy().astype(np.float32)
    row, col, eid = entries(src, dst, n_dst, self_loops)
    F = xn.shape[1]
    out = np.zeros((n_dst, F), dtype=np.float32)
    arg = np.full((n_dst, F), -2, dtype=np.int32)
    if row.size:
        word = (key(xn[col]).astype(np.uint64) << np.uint64(32)) | (~eid.astype(np.uint32)).astype(np.uint64)[:, None]
        rows, starts = np.unique(row, return_index=True)
        best = np.maximum.reduceat(word, starts, axis=0)
        out[rows] = value_of_key((best >> np.uint64(32)).astype(np.uint32))
        arg[rows] = (~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)).view(np.int32)
    return torch.from_numpy(out), torch.from_numpy(arg)


def rule_x_loop(x: torch.Tensor, src, dst, n_dst: int, self_loops: bool):
    """the same rule as a literal loop over rows, columns and entries with float comparisons (small inputs only)"""
    xn = x.detach().cpu().numpy().astype(np.float32)
    row, col, eid = entries(src, dst, n_dst, self_loops)
    F = xn.shape[1]
    out = np.zeros((n_dst, F), dtype=np.float32)
    arg = np.full((n_dst, F), -2, dtype=np.int32)
    for i in range(n_dst):
        ps = np.nonzero(row == i)[0]
        for c in range(F):
            best = None
            for p in ps:
                v, e = xn[col[p], c], int(np.uint32(np.int32(eid[p])))
                if best is None:
                    best = (v, e)
                    continue
                bv, be = best
                if np.isnan(v) or np.isnan(bv):
                    better = (np.isnan(v) and not np.isnan(bv)) or (np.isnan(v) and np.isnan(bv) and e < be)
                else:
                    better = v > bv or (v == bv and e < be)                # -0.0 == +0.0 here, as the rule wants
                if better:
                    best = (v, e)
            if best is not None:
                v = best[0]
                out[i, c] = np.float32(np.nan) if np.isnan(v) else (np.float32(0.0) if v == 0 else v)
                arg[i, c] = np.int32(np.uint32(best[1]))
    out_bits = out.view(np.uint32)
    out_bits[np.isnan(out)] = QNAN
    return torch.from_numpy(out), torch.from_numpy(arg)


def rule_x_bwd(dout: torch.Tensor, arg: torch.Tensor, src, n_src: int) -> torch.Tensor:
    """fp64 ``dX [n_src, F]``: ``dout[i, c]`` goes to the source of edge ``arg[i, c]``, to node i itself for the loop (-1), nowhere for -2"""
    d = dout.detach().cpu().double().numpy()
    a = arg.cpu().numpy().astype(np.int64)
    src = np.asarray(src, dtype=np.int64)
    n_dst, F = d.shape
    dx = np.zeros((n_src, F), dtype=np.float64)
    cols = np.broadcast_to(np.arange(F), (n_dst, F))
    owner = np.where(a >= 0, src[np.clip(a, 0, max(src.size - 1, 0))] if src.size else 0, np.arange(n_dst)[:, None])
    live = a >= -1
    np.add.at(dx, (owner[live], cols[live]), d[live])
    return torch.from_numpy(dx)


def torch_amax(x: torch.Tensor, src, dst, n_dst: int, self_loops: bool) -> torch.Tensor:
    """the literal composition the kernels replace: ``zeros.scatter_reduce(0, idx, x[src], 'amax', include_self=False)``"""
    row, col, _ = entries(src, dst, n_dst, self_loops)
    idx = torch.from_numpy(row)[:, None].expand(-1, x.size(1))
    return torch.zeros((n_dst, x.size(1)), dtype=x.dtype).scatter_reduce(0, idx, x[torch.from_numpy(col)], "amax", include_self=False)


def tied_fraction(x: torch.Tensor, src, dst, n_dst: int, self_loops: bool) -> float:
    """share of the non-empty (row, column) cells whose maximum is attained by more than one entry"""
    xn = x.detach().cpu().numpy().astype(np.float32)
    row, col, _ = entries(src, dst, n_dst, self_loops)
    k = key(xn[col])
    rows, starts = np.unique(row, return_index=True)
    best = np.maximum.reduceat(k, starts, axis=0)
    hits = np.add.reduceat((k == best[np.searchsorted(rows, row)]).astype(np.int64), starts, axis=0)
    return float((hits > 1).mean())


# ---- inputs ------------------------------------------------------------------------------------------------------------------
N_STRESS = 300
EMPTY_ROWS = (0, 17, N_STRESS - 1)
SIZED_ROWS = {3: 1, 5: 63, 7: 64, 9: 65, 11: 255, 13: 256, 15: 257}
HUB_ROW, HUB_SRC, HUB = 20, 25, 1500


@lru_cache(maxsize=None)
def stress_edges(seed: int = 0) -> torch.Tensor:
    """``edge_index [2, E]`` over ``N_STRESS`` nodes, no ``(i, i)`` column, columns in random order (a row's list order is not its
    eid order).  Rows 0, 17 and N-1 have no in-edge; rows 3 .. 15 have exactly 1, 63, 64, 65, 255, 256 and 257; row 20 is a hub of
    1,500 in-edges and node 25 a hub SOURCE of at least 1,500 out-edges -- 700 of them repeated ``25 -> 20`` columns (ties between eids),
    the other 800 spread over the remaining rows, which besides have a random 0 - 12 in-edges each."""
    rng = np.random.default_rng(seed)
    N = N_STRESS
    fixed = set(EMPTY_ROWS) | set(SIZED_ROWS) | {HUB_ROW}
    free = np.array([i for i in range(N) if i not in fixed])

    def sources(i, n):
        s = rng.integers(0, N - 1, size=n)
        return s + (s >= i)                                                # any node but i

    src, dst = [], []
    for i in free:
        n = int(rng.integers(0, 13))
        src.append(sources(i, n)), dst.append(np.full(n, i))
    for i, n in SIZED_ROWS.items():
        src.append(sources(i, n)), dst.append(np.full(n, i))
    src.append(np.full(700, HUB_SRC)), dst.append(np.full(700, HUB_ROW))
    src.append(sources(HUB_ROW, HUB - 700)), dst.append(np.full(HUB - 700, HUB_ROW))
    spread = rng.choice(free[free != HUB_SRC], size=HUB - 700)
    src.append(np.full(HUB - 700, HUB_SRC)), dst.append(spread)
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(src.size)
    return torch.from_numpy(np.stack([src[perm], dst[perm]]).astype(np.int64))


@lru_cache(maxsize=None)
def int_table(rows: int, F: int, lo: int, hi: int, seed: int) -> torch.Tensor:
    """integer-valued f32 in ``[lo, hi]``: maxima tie all the time, sums of them are exact in f32 in any order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (rows, F), generator=g).float()


@lru_cache(maxsize=None)
def randn_table(rows: int, F: int, seed: int) -> torch.Tensor:
    return torch.randn((rows, F), generator=torch.Generator().manual_seed(seed))


@lru_cache(maxsize=None)
def stress_reference(F: int, self_loops: bool, integer: bool = True):
    """``(x, dout, out, arg, dx64)`` of the stress graph at width F: the tables, Rule X and its fp64 backward"""
    ei = stress_edges()
    N = N_STRESS
    x = int_table(N, F, -2, 2, 100 + F) if integer else randn_table(N, F, 100 + F)
    dout = int_table(N, F, -3, 3, 200 + F) if integer else randn_table(N, F, 200 + F)
    out, arg = rule_x(x, ei[0].numpy(), ei[1].numpy(), N, self_loops)
    return x, dout, out, arg, rule_x_bwd(dout, arg, ei[0].numpy(), N)
