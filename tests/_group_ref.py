"""Rule G (``include/npi_gnn.h``: ``npi_group_score``) restated in torch on the CPU: the logits of every positive and of its own
corrupted targets, the three ranking losses, ``d loss / d logit`` and the gradients of both tables as explicit formulas -- no autograd
-- in the dtype asked for (the tests evaluate it in fp64 as the reference, and in float32 to see what that precision alone costs).
Shared by ``tests/test_group_loss_cpu.py`` and ``tests/test_gpu_group_loss.py``, with the inputs both use."""
import functools

import torch

import _link_ref as link
from _link_ref import F_CASES, N_DST, N_SRC, extreme_tables, tables  # noqa: F401  (re-exported to the tests)

# (P, K): the smallest shapes that reach each way the slot -> lane mapping can go wrong (a wavefront owns 64 // (1 + K) whole groups,
# a workgroup four wavefronts; slots are scored in batches of eight)
SHAPES = ((5, 0),                                            # no corrupted target at all
          (1, 1), (31, 1), (32, 1), (33, 1), (129, 1),       # 32 groups per wave: its tails, a second wave, a second workgroup
          (22, 2),                                           # 21 groups per wave and one idle lane
          (9, 3),
          (21, 7),                                           # groups aligned to the batch of eight
          (9, 8),                                            # groups straddling batches
          (5, 15),
          (9, 31),                                           # 2 groups per wave: 9 groups need a second workgroup
          (5, 32),                                           # one group per wave, 31 idle lanes
          (6, 63))                                           # a full wave per group, second workgroup
HINGE_GAP = 1e-3                                             # every valid |margin + d_c| of a margin parity case is at least this


def cases():
    """(loss, margin, scale) of the parity cases"""
    return (("bpr", 1.0, 1.0), ("bpr", 1.0, 2.5), ("margin", 1.0, 1.0), ("softmax", 1.0, 1.0), ("softmax", 1.0, 2.5))


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def slots(src, dst, neg, n_src, n_dst):
    """(targets [P, C], keep [P], valid [P, C]): a group is kept when both ids of its positive are in range; a slot is valid -- it
    reads rows -- when its group is kept and its target lies in [0, n_dst) (-1 is the empty slot, anything else out of range a bad one)"""
    tgt = torch.cat([dst[:, None], neg], 1)
    keep = (src >= 0) & (src < n_src) & (dst >= 0) & (dst < n_dst)
    valid = keep[:, None] & (tgt >= 0) & (tgt < n_dst)
    return tgt, keep, valid


def logits(z_src, z_dst, src, dst, neg):
    """[P, 1 + K]: <z_src[src_p], z_dst[target]>; -inf at an empty or bad slot of a kept group, 0 all over a dropped group"""
    n_src, n_dst = z_src.size(0), z_dst.size(0)
    tgt, keep, valid = slots(src, dst, neg, n_src, n_dst)
    a = z_src[src.clamp(0, n_src - 1)]
    b = z_dst[tgt.clamp(0, n_dst - 1)]
    x = (a[:, None, :] * b).sum(-1)
    ninf = torch.full_like(x, float("-inf"))
    return torch.where(valid, x, torch.where(keep[:, None], ninf, torch.zeros_like(x))), valid


def loss_and_coef(x, valid, kind, margin=1.0, scale=1.0):
    """(loss, d loss / d x [P, C]) of logits ``x`` whose valid slots are ``valid``; d_c = scale (x_c - x_0) over the valid negatives V:
    bpr:     sum_V softplus(d_c) / (P K), softplus(d) = max(d, 0) + log1p(exp(-|d|));   coef_c = scale sigmoid(d_c) / (P K)
    margin:  sum_V max(0, margin + d_c) / (P K);                                         coef_c = scale [margin + d_c > 0] / (P K)
    softmax: sum_p (m + log(exp(-m) + sum_V exp(d_c - m))) / P, m = max(0, max_V d_c);   coef_c = scale exp(d_c - m) / den / P
    coef_0 = -sum_{c >= 1} coef_c.  The divisors count slots, not valid slots."""
    P, C = x.shape
    K = C - 1
    V = valid.clone()
    V[:, 0] = False
    zero = torch.zeros_like(x)
    d = torch.where(V, scale * (torch.where(valid, x, zero) - torch.where(valid[:, :1], x[:, :1], zero[:, :1])), zero)   # 0 outside V
    if kind == "bpr":
        div = max(P * K, 1)
        term = torch.where(V, d.clamp(min=0) + torch.log1p(torch.exp(-d.abs())), zero)
        coef = torch.where(V, scale * torch.sigmoid(d), zero) / div
        loss = term.sum() / div
    elif kind == "margin":
        div = max(P * K, 1)
        h = margin + d
        term = torch.where(V, h.clamp(min=0), zero)
        coef = torch.where(V & (h > 0), torch.full_like(x, scale), zero) / div
        loss = term.sum() / div
    elif kind == "softmax":
        div = max(P, 1)
        m = torch.where(V, d, zero).max(dim=1).values.clamp(min=0)                # max(0, max_V d_c): the zeros outside V stand for it
        e = torch.where(V, torch.exp(d - m[:, None]), zero)
        den = torch.exp(-m) + e.sum(1)
        coef = scale * e / den[:, None] / div
        loss = (m + torch.log(den)).sum() / div
    else:
        raise ValueError(kind)
    coef[:, 0] = -coef[:, 1:].sum(1)
    return loss, coef


def table_grads(z_src, z_dst, src, dst, neg, g):
    """(dZ_src, dZ_dst) for d loss / d logit = g [P, C] (zero at every slot that is not valid): the sums of ``_link_ref.table_grads``
    over the expanded list"""
    C = 1 + neg.size(1)
    tgt = torch.cat([dst[:, None], neg], 1).clamp(0, z_dst.size(0) - 1).flatten()
    return link.table_grads(z_src, z_dst, src.clamp(0, z_src.size(0) - 1).repeat_interleave(C), tgt, g.flatten())


def evaluate(z_src, z_dst, src, dst, neg, kind, margin=1.0, scale=1.0, upstream=1.0, dtype=torch.float64):
    """everything the tests compare, in ``dtype``: dict(logits, loss, coef, d_src, d_dst, valid); gradients of ``upstream * loss``"""
    zs, zd = z_src.to(dtype), z_dst.to(dtype)
    x, valid = logits(zs, zd, src, dst, neg)
    loss, coef = loss_and_coef(x, valid, kind, margin, scale)
    d_src, d_dst = table_grads(zs, zd, src, dst, neg, coef * upstream)
    return dict(logits=x, loss=loss, coef=coef, d_src=d_src, d_dst=d_dst, valid=valid)


def rel_finite(got, want):
    """``_util.rel_max`` over the finite entries of ``want``; the -inf entries (empty slots) must sit at the same places in both"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    inf = torch.isinf(want)
    assert torch.equal(inf, torch.isinf(got)) and bool((got[inf] == want[inf]).all()), "the -inf slots differ"
    zero = torch.zeros_like(want)
    return float((torch.where(inf, zero, got) - torch.where(inf, zero, want)).abs().max() / torch.where(inf, zero, want).abs().max().clamp(min=1e-300))


# ---- the inputs of the parity cases --------------------------------------------------------------------------------------------------
def groups(P, K, n_src=N_SRC, n_dst=N_DST, seed=0):
    """(src [P], dst [P], neg [P, K]): uniform ids; about 10 % of the corrupted slots are empty (-1), and with three groups or more the
    middle group's corrupted slots are ALL empty"""
    g = torch.Generator().manual_seed(7919 * P + 131 * K + seed)
    src = torch.randint(0, n_src, (P,), generator=g)
    dst = torch.randint(0, n_dst, (P,), generator=g)
    neg = torch.randint(0, n_dst, (P, K), generator=g)
    neg[torch.rand(P, K, generator=g) < 0.1] = -1
    if P >= 3:
        neg[P // 2] = -1
    return src, dst, neg


def hinge_gap(zs, zd, src, dst, neg, margin, scale):
    """the smallest |margin + d_c| over the valid corrupted slots, in fp64 (inf when there is none)"""
    x, valid = logits(zs.double(), zd.double(), src, dst, neg)
    V = valid.clone()
    V[:, 0] = False
    if not bool(V.any()):
        return float("inf")
    h = margin + scale * (x - x[:, :1])
    return float(h[V].abs().min())


@functools.lru_cache(maxsize=None)
def _seed(P, K, F, kind, margin, scale, n_src, n_dst):
    """the seed of ``groups`` a parity case uses: 0 -- for ``margin`` the first of 0 .. 31 whose inputs keep every valid hinge at
    least HINGE_GAP away from its kink (an f32 logit on these tables is off by less than 1e-5 absolute, so no kink can flip between
    the device and the fp64 reference); None when there is none"""
    if kind != "margin":
        return 0
    zs, zd = tables(F, n_src, n_dst)
    for seed in range(32):
        if hinge_gap(zs, zd, *groups(P, K, n_src, n_dst, seed), margin, scale) >= HINGE_GAP:
            return seed
    return None


def inputs(P, K, F, kind, margin=1.0, scale=1.0, n_src=N_SRC, n_dst=N_DST):
    """(z_src, z_dst, src, dst, neg) of a parity case; float32 tables of ``_link_ref.tables``"""
    seed = _seed(P, K, F, kind, float(margin), float(scale), n_src, n_dst)
    assert seed is not None, ("no seed in 0..31 keeps every hinge off its kink", P, K, F, margin, scale)
    zs, zd = tables(F, n_src, n_dst)
    return (zs, zd) + groups(P, K, n_src, n_dst, seed)


ONE_SPACE = (40, 5, 30)                      # (P, K, N) of the one-id-space case: both ends read one table of N rows


def one_space_inputs(kind, margin=1.0, scale=1.0, F=64):
    P, K, N = ONE_SPACE
    zs, _, src, dst, neg = inputs(P, K, F, kind, margin, scale, N, N)
    src[:3] = dst[:3]                        # loops (v, v) among the positives
    if kind == "margin":
        assert hinge_gap(zs, zs, src, dst, neg, margin, scale) >= HINGE_GAP
    return zs, src, dst, neg


def extreme_groups(F=64):
    """``_link_ref.extreme_tables`` as groups: every source with target 0 as its positive and every other target of the +-60
    construction as a corrupted one -- all of its pairs, so the logits span exactly [-60, 60]: (z_src, z_dst, src, dst, neg)"""
    zs, zd, _, _ = extreme_tables(F)
    n_src, n_even = zs.size(0), zd.size(0) // 2 * 2
    src = torch.arange(n_src)
    return zs, zd, src, torch.zeros(n_src, dtype=torch.int64), torch.arange(1, n_even).repeat(n_src, 1)


def upstream_of(P, K, F):
    """the upstream factor of a parity case: a fixed 'random' number in [-3, 3] that is never near 0"""
    u = ((37 * P + 11 * K + F) % 25) / 10.0 + 0.5
    return -u if (P + K + F) % 2 else u


def parity_inputs():
    """every (F, P, K, kind, margin, scale) the GPU parity tests run"""
    for F in F_CASES:
        for P, K in SHAPES:
            for kind, margin, scale in cases():
                yield F, P, K, kind, margin, scale
