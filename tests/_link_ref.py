"""The link-prediction stage restated in torch on the CPU, from PyG 1.4.2's expressions (``nn/models/autoencoder.py``): pair logits,
both losses, ``d loss / d logit`` and the gradients of both tables as explicit formulas -- no autograd -- in the dtype of the inputs
(the tests evaluate it in fp64 as the reference, and in float32 to see what that precision alone costs).  Shared by
``tests/test_link_cpu.py`` and ``tests/test_gpu_link.py``, with the inputs both use."""
import torch

EPS = 1e-15            # torch_geometric.nn.models.autoencoder.EPS

F_CASES = (1, 3, 64, 256, 257, 260)          # scalar and 16-byte lanes, partial and full chunks, rows of more than one chunk
M_CASES = (1, 7, 8, 9, 64, 65, 1000)         # the tails of the group of eight and of the block of 64; four workgroups
N_SRC, N_DST = 37, 23                        # few rows: every id repeats, the backward accumulates


def n_pos_cases(M):
    return sorted({0, M, M // 3})


def logits(z_src, z_dst, src, dst):
    """InnerProductDecoder.forward(sigmoid=False): (z[edge_index[0]] * z[edge_index[1]]).sum(dim=1)"""
    return (z_src[src] * z_dst[dst]).sum(dim=1)


def loss_and_coef(x, n_pos, kind):
    """(loss, d loss / d x) of logits ``x`` whose first ``n_pos`` are positives.
    gae: -log(s + EPS).mean() over the positives + -log(1 - s + EPS).mean() over the negatives, s = sigmoid(x); the derivative of
         exactly these: -s (1 - s) / (s + EPS) / n_pos and s (1 - s) / (1 - s + EPS) / n_neg.  An empty part adds 0.
    bce: binary_cross_entropy_with_logits(x, y).mean(): max(x, 0) - x y + log1p(exp(-|x|)); derivative (s - y) / M."""
    M = x.numel()
    pos = torch.arange(M) < n_pos
    if kind == "gae":
        s = torch.sigmoid(x)
        q = 1 - s
        n = torch.where(pos, torch.tensor(float(max(n_pos, 1))), torch.tensor(float(max(M - n_pos, 1)))).to(x.dtype)
        term = -torch.log(torch.where(pos, s, q) + EPS)
        coef = torch.where(pos, -(s * q) / (s + EPS), (s * q) / (q + EPS)) / n
        return (term / n).sum(), coef
    if kind == "bce":
        y = pos.to(x.dtype)
        term = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
        # s - y without cancellation: -sigmoid(-x) for a positive
        coef = torch.where(pos, -torch.sigmoid(-x), torch.sigmoid(x)) / max(M, 1)
        return term.sum() / max(M, 1), coef
    raise ValueError(kind)


def table_grads(z_src, z_dst, src, dst, g):
    """(dZ_src, dZ_dst) for d loss / d logit = g: dZ_src[i] = sum_{m: src_m = i} g_m z_dst[dst_m], dZ_dst[j] likewise"""
    d_src = torch.zeros_like(z_src).index_add_(0, src, g[:, None] * z_dst[dst])
    d_dst = torch.zeros_like(z_dst).index_add_(0, dst, g[:, None] * z_src[src])
    return d_src, d_dst


def evaluate(z_src, z_dst, src, dst, n_pos, kind, upstream=1.0, dtype=torch.float64):
    """everything the tests compare, in ``dtype``: dict(logits, loss, coef, d_src, d_dst); gradients of ``upstream * loss``"""
    zs, zd = z_src.to(dtype), z_dst.to(dtype)
    x = logits(zs, zd, src, dst)
    loss, coef = loss_and_coef(x, n_pos, kind)
    d_src, d_dst = table_grads(zs, zd, src, dst, coef * upstream)
    return dict(logits=x, loss=loss, coef=coef, d_src=d_src, d_dst=d_dst)


# ---- the inputs of the parity cases --------------------------------------------------------------------------------------------------
def tables(F, n_src=N_SRC, n_dst=N_DST, seed=0):
    """float32 embeddings drawn so that the logits stay within +-4 (randn F^-1/4 0.7: a logit has standard deviation 0.49): beyond
    that ``1 - s`` loses digits in float32, a property of PyG's formula and not of the kernel"""
    g = torch.Generator().manual_seed(1000 * F + seed)
    scale = 0.7 * F ** -0.25
    return torch.randn(n_src, F, generator=g) * scale, torch.randn(n_dst, F, generator=g) * scale


def pair_list(M, n_src=N_SRC, n_dst=N_DST, seed=0):
    g = torch.Generator().manual_seed(77 * M + seed)
    return torch.randint(0, n_src, (M,), generator=g), torch.randint(0, n_dst, (M,), generator=g)


def hub_pairs(n_src=N_SRC, n_dst=N_DST):
    """300 pairs that share source 5 (targets cycling: every pair many times) followed by 100 spread ones"""
    src = torch.cat([torch.full((300,), 5, dtype=torch.int64), torch.arange(100) % n_src])
    dst = torch.cat([torch.arange(300) % 7, (torch.arange(100) * 3) % n_dst])
    return src, dst


def extreme_tables(F=64, n_src=N_SRC, n_dst=N_DST):
    """tables and a pair list whose logits span exactly [-60, 60]: every odd target row is minus the even one before it, the list is
    every source with each of those targets (in a shuffled order), and the source table is scaled so that the largest |logit| is 60"""
    zs, zd = tables(F, n_src, n_dst, seed=5)
    n_even = n_dst // 2 * 2
    zd[1:n_even:2] = -zd[0:n_even:2]
    zs = zs * float(60.0 / (zs.double() @ zd[:n_even].double().t()).abs().max())
    perm = torch.randperm(n_src * n_even, generator=torch.Generator().manual_seed(9))
    return zs, zd, (perm // n_even), (perm % n_even)
