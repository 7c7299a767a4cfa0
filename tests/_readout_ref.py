"""Rule O (include/npi_gnn.h) restated in torch, for any dtype and device: what the fused readouts are tested against.  The sums are
plain torch sums (in fp64 when the inputs are): the reference fixes the VALUES, not the order of summation."""
import torch

CHUNK = 1024                     # NPI_READOUT_CHUNK
# graph sizes around every boundary of the kernels (a wave, a chunk), empty graphs first, in the middle and last
SIZES = [0, 1, 2, 63, 0, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 0]
WIDTHS = [1, 3, 6, 64, 100, 256, 260]


def graph_ptr(sizes, first=0):
    return torch.tensor([first] + sizes, dtype=torch.int64).cumsum(0).to(torch.int32)


def batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64))


def _owner(gp, N):
    """graph of every row (-1: a row outside every graph) and the rows' positions inside their graphs"""
    gp = gp.long()
    rows = torch.arange(N, device=gp.device)
    g = torch.searchsorted(gp, rows, right=True) - 1
    inside = (rows >= gp[0]) & (rows < gp[-1])
    g = torch.where(inside, g, torch.full_like(g, -1))
    return g, inside


def key_bits(v):
    """ascending-orderable uint32 (as int64) of float32 keys after the rule's NaN canonicalisation: NaN above +inf, +0.0 above -0.0"""
    v = v.float()
    bits = v.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    bits = torch.where(torch.isnan(v), torch.full_like(bits, 0x7FC00000), bits)
    return torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits | 0x80000000)


# ---- O-add ---------------------------------------------------------------------------------------------------------------------
def add(x, gp):
    g, inside = _owner(gp, x.size(0))
    out = torch.zeros((gp.numel() - 1, x.size(1)), dtype=x.dtype, device=x.device)
    return out.index_add(0, g[inside], x[inside])


def add_bwd(dout, gp, N):
    g, inside = _owner(gp, N)
    dx = torch.zeros((N, dout.size(1)), dtype=dout.dtype, device=dout.device)
    dx[inside] = dout[g[inside]]
    return dx


# ---- O-sort --------------------------------------------------------------------------------------------------------------------
def ranks(x, gp):
    """rank of every row inside its graph (-1: outside every graph): last column descending in the rule's bit order, ties by index"""
    N = x.size(0)
    g, inside = _owner(gp, N)
    comp = (torch.where(inside, g, torch.full_like(g, gp.numel())) << 32) | (0xFFFFFFFF - key_bits(x[:, -1].detach()))
    order = torch.argsort(comp, stable=True)                  # graph-major, key descending, index ascending
    pos = torch.empty(N, dtype=torch.int64, device=x.device)
    pos[order] = torch.arange(N, device=x.device)
    n_before = gp.long()[0]                                    # rows in front of the first graph sort behind everything (g = B)
    rank = pos - (gp.long()[g.clamp(min=0)] - n_before)
    return torch.where(inside, rank, torch.full_like(rank, -1)), g


def sort_pool(x, gp, k):
    B, F = gp.numel() - 1, x.size(1)
    rank, g = ranks(x, gp)
    sel = (rank >= 0) & (rank < k)
    out = torch.zeros((B, k, F), dtype=x.dtype, device=x.device)
    out = out.index_put((g[sel], rank[sel]), x[sel])
    return out.view(B, k * F)


def sort_pool_bwd(dout, x, gp, k):
    F = x.size(1)
    rank, g = ranks(x, gp)
    sel = (rank >= 0) & (rank < k)
    dx = torch.zeros((x.size(0), F), dtype=dout.dtype, device=dout.device)
    dx[sel] = dout.view(-1, k, F)[g[sel], rank[sel]]
    return dx


# ---- O-att ---------------------------------------------------------------------------------------------------------------------
def alpha(gate, gp):
    g, inside = _owner(gp, gate.numel())
    B = gp.numel() - 1
    gi = g[inside]
    m = torch.full((B,), -float("inf"), dtype=gate.dtype, device=gate.device).scatter_reduce(0, gi, gate[inside], "amax")
    e = torch.zeros_like(gate)
    e[inside] = torch.exp(gate[inside] - m[gi])
    s = torch.zeros(B, dtype=gate.dtype, device=gate.device).index_add(0, gi, e[inside])
    a = torch.zeros_like(gate)
    a[inside] = e[inside] / (s[gi] + 1e-16)
    return a, g, inside


def attention(gate, x, gp):
    a, g, inside = alpha(gate.reshape(-1), gp)
    out = torch.zeros((gp.numel() - 1, x.size(1)), dtype=x.dtype, device=x.device)
    return out.index_add(0, g[inside], a[inside, None] * x[inside])


def attention_bwd(gate, x, gp, dout):
    """the rule's backward formulas: dx_i = alpha_i dout_g, dgate_i = alpha_i (<dout_g, x_i> - <dout_g, out_g>)"""
    a, g, inside = alpha(gate.reshape(-1), gp)
    out = attention(gate, x, gp)
    c = (dout * out).sum(1)
    gi = g.clamp(min=0)
    dx = torch.where(inside[:, None], a[:, None] * dout[gi], torch.zeros_like(x))
    dgate = torch.where(inside, a * ((dout[gi] * x).sum(1) - c[gi]), torch.zeros_like(a))
    return dx, dgate


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def randn_table(n, F, seed):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed))


def int_table(n, F, lo, hi, seed):
    return torch.randint(lo, hi + 1, (n, F), generator=torch.Generator().manual_seed(seed)).float()


def tied_keys(n, seed):
    """a last column where ties are the rule: a few small integers, with NaNs of both signs, -0.0 and +0.0 among them"""
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, float("nan"), float("inf")])
    col = pool[torch.randint(0, pool.numel(), (n,), generator=g)]
    bits = col.view(torch.int32).clone()
    flip = torch.isnan(col) & (torch.rand(n, generator=g) < 0.5)
    bits[flip] |= -0x80000000                                  # NaNs with the sign bit set
    return bits.view(torch.float32)
