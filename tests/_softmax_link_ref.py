"""Rule L of ``include/npi_gnn.h`` (``npi_softmax_link_*``) restated in torch on the CPU, in the dtype of the tables it is given:
the candidate mask of ``_topk_ref.allowed`` with the target's own column forced in, ``logsumexp``, ``lp``, autograd for the
gradients; a bad pair is dropped (``lp = 0``, no gradient) -- and the inputs the CPU and GPU tests share."""
import functools

import torch

import _topk_ref as tref

BAD_PAIR, BAD_SCORE = 256, 1024              # NPI_STATUS_BAD_PAIR_ID, NPI_STATUS_BAD_SCORE
SCALE = 0.125                                # of the parity inputs (unit randn tables: |x| stays near F^(1/2) / 8)

# (n_src, n_dst, F) and Q of the parity cases (tests/test_gpu_softmax_link.py)
SHAPES = [(63, 127, 64), (65, 129, 65), (130, 1000, 260), (130, 300, 100), (1, 1000, 3), (40, 449, 256)]
QS = (1, 63, 65, 200)


def link_log_softmax(z_src, z_dst, edge_index, exclude=None, allow_loops=True, scale=1.0, u=None):
    """``(lp [Q], dZ_src, dZ_dst, status)``; ``z_dst`` None: one id space (``dZ_src`` is then the gradient of the one table and
    ``dZ_dst`` None).  ``u``: the upstream ``d L / d lp`` (None: no gradients).  ``loss(lp, Q)`` is Rule L 6."""
    zs = z_src.detach().clone().requires_grad_(u is not None)
    zd = zs if z_dst is None else z_dst.detach().clone().requires_grad_(u is not None)
    n_src, n_dst = zs.size(0), zd.size(0)
    s, t = edge_index[0], edge_index[1]
    Q = s.numel()
    good = (s >= 0) & (s < n_src) & (t >= 0) & (t < n_dst)
    sg, tg = s[good], t[good]
    at = torch.arange(sg.numel())
    mask = torch.from_numpy(tref.allowed(n_src, n_dst, exclude, allow_loops))[sg]
    mask[at, tg] = True                                                    # the target is always a candidate
    x = (scale * (zs[sg] @ zd.t())).masked_fill(~mask, float("-inf"))
    lp = torch.zeros(Q, dtype=zs.dtype)
    lp[good] = x[at, tg] - torch.logsumexp(x, 1)
    status = (0 if bool(good.all()) else BAD_PAIR) | (BAD_SCORE if bool(torch.isnan(lp).any()) else 0)
    if u is None:
        return lp.detach(), None, None, status
    (lp * u.to(zs.dtype)).sum().backward()
    return lp.detach(), zs.grad, (None if z_dst is None else zd.grad), status


def loss(lp: torch.Tensor, Q: int) -> torch.Tensor:
    return -lp.double().sum() / Q if Q else torch.zeros((), dtype=torch.float64)


def queries(n_src, n_dst, Q, seed=0):
    """``[2, Q]`` pairs drawn with repeats: sources occur several times, many sources and targets never"""
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.stack([torch.randint(0, n_src, (Q,), generator=g), torch.randint(0, n_dst, (Q,), generator=g)])


def upstream(Q, seed=0):
    """``randn`` with negative entries and, at every fifth place, zeros"""
    g = torch.Generator().manual_seed(5000 + seed)
    u = torch.randn(Q, generator=g)
    u[::5] = 0.0
    return u


@functools.lru_cache(maxsize=None)
def inputs(shape, Q):
    """the parity input of a (shape, Q) case: ``(z_src, z_dst, exclude [2, 3 n_src], queries [2, Q], u [Q])``, float32 on the host"""
    n_src, n_dst, F = shape
    zs, zd = tref.real_tables(n_src, n_dst, F, seed=F + Q)
    return zs, zd, tref.edges(n_src, n_dst, 3 * n_src, seed=F), queries(n_src, n_dst, Q, seed=Q + F), upstream(Q, seed=Q)


@functools.lru_cache(maxsize=None)
def expected(shape, Q, excluded: bool, dtype=torch.float64):
    """the restatement on ``inputs(shape, Q)`` in ``dtype``, computed once and shared: ``(lp, dZ_src, dZ_dst)``"""
    zs, zd, ex, q, u = inputs(shape, Q)
    return link_log_softmax(zs.to(dtype), zd.to(dtype), q, ex if excluded else None, True, SCALE, u)[:3]
