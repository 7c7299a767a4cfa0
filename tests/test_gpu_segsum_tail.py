"""The aggregation kernel's ragged tail, batch boundary and cut row in every weight mode (csrc/segsum.hip).

A 64-entry block is consumed in batches of U gathered rows (U = 8, 4 or 2 for 1, 2 or 4 chunks per lane) and, in the LAST item
of a CSR only, entry by entry for what is left when the block is no multiple of U.  Every mode runs both, so every mode is run
here on CSRs whose last block holds r = nnz % 64 entries for r around every U: no tail (0), a tail alone (1), a full tail
(U - 1), exactly one batch (U), a batch and a tail (U + 1), and 63.  Each CSR has 64-entry items, a row of more than 128 entries
(a tail part, a head part that spans a whole item, a head part that closes) and two empty rows, on BOTH sides of the bipartite
graph.  Every operator is compared with its definition, a few lines of torch in float64 on the same device, at the tolerances
tests/test_gpu_gat.py and test_gpu_parity.py::test_segsum_widths use for the same operator."""
import pytest
import torch

import npi_gnn_amd as npi

N_SRC, N_DST = 50, 40
REMAINDERS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63)       # {0, 1, U - 1, U, U + 1, 63} for U = 8, 4 and 2
ATOL, RTOL = 1e-4, 1e-4                            # test_segsum_widths; the GAT forward (test_gat_conv_fwd_bwd_matches_oracle)
BWD_ATOL, BWD_RTOL = 2e-4, 1e-3                    # the GAT backward (the same test's gradient)
SLOPE = 0.2


def _edges(r, g):
    """E = 192 + r edges (255 for r = 63): 110 copies of 5 -> 3 plus 20 more into target 3 and 20 more out of source 5 (130 entries
    each: the long row of either side), the rest random; targets 11 and 39 and sources 7 and 49 stay empty (others may)"""
    E = 255 if r == 63 else 192 + r
    assert E % 64 == r and 130 <= E <= 260
    src_ok = torch.tensor([j for j in range(N_SRC) if j not in (5, 7, 49)])
    dst_ok = torch.tensor([i for i in range(N_DST) if i not in (3, 11, 39)])
    n = E - 150
    src = torch.cat([torch.full((110,), 5), src_ok[torch.randint(0, len(src_ok), (20,), generator=g)], torch.full((20,), 5),
                     src_ok[torch.randint(0, len(src_ok), (n,), generator=g)]])
    dst = torch.cat([torch.full((110,), 3), torch.full((20,), 3), dst_ok[torch.randint(0, len(dst_ok), (20,), generator=g)],
                     dst_ok[torch.randint(0, len(dst_ok), (n,), generator=g)]])
    perm = torch.randperm(E, generator=g)
    return torch.stack([src[perm], dst[perm]])


class _Case:
    """one graph and the entry lists of its two sides (row and column of every entry, int64)"""

    def __init__(self, r, dev):
        self.g = torch.Generator().manual_seed(100 + r)
        ei = _edges(r, self.g)
        self.E = ei.size(1)
        self.graph = npi.BipartiteGraph(ei.to(dev), (N_SRC, N_DST), item=64)
        self.dev = dev
        for side in (self.graph.by_dst, self.graph.by_src):
            assert side.item == 64 and int(side.rowptr[-1]) == self.E        # no self loop added: nnz is exactly E
            cnt = (side.rowptr[1:] - side.rowptr[:-1])
            assert int(cnt.max()) > 128 and int((cnt == 0).sum()) >= 2

    def entries(self, side):
        return side.rowidx[:self.E].long(), side.col[:self.E].long()

    def randn(self, *shape, scale=1.0):
        return (torch.randn(*shape, generator=self.g) * scale).to(self.dev)

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g).to(self.dev)


@pytest.fixture(scope="module", params=REMAINDERS)
def case(request, dev):
    return _Case(request.param, dev)


def _rowsum(row, vals, n_rows):
    """sum of the float64 entry values over every row"""
    return torch.zeros((n_rows,) + vals.shape[1:], dtype=torch.float64, device=vals.device).index_add_(0, row, vals)


def _close(got, want, atol, rtol):
    return torch.allclose(got.double(), want, atol=atol, rtol=rtol)


def _softmax_stats(row, e, n_rows):
    """(m, s) of the float64 scores e [E, H] over every row; an empty row has m = s = 0"""
    H = e.size(1)
    m = torch.full((n_rows, H), float("-inf"), dtype=torch.float64, device=e.device)
    m = m.scatter_reduce(0, row.view(-1, 1).expand(-1, H), e, "amax")
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return m, _rowsum(row, (e - m[row]).exp(), n_rows)


def _lrelu(z):
    return torch.where(z > 0, z, SLOPE * z)


@pytest.mark.gpu
# unguarded; guarded, one chunk (100: two entries per instruction, 200: one); two chunks; four chunks; four entries per instruction
@pytest.mark.parametrize("F", [256, 100, 200, 300, 1000, 8])
def test_segsum_plain_and_weighted_mean_and_sum(case, F):
    from npi_gnn_amd import functional as NF
    for side, n_rows, n_cols in ((case.graph.by_dst, N_DST, N_SRC), (case.graph.by_src, N_SRC, N_DST)):
        row, col = case.entries(side)
        x = case.randn(n_cols, F)
        w = case.rand(side.nnz_max)
        cnt = torch.bincount(row, minlength=n_rows).clamp(min=1).double().view(-1, 1)
        for wt in (None, w):
            vals = x.double()[col] if wt is None else wt[:case.E].double().view(-1, 1) * x.double()[col]
            want = _rowsum(row, vals, n_rows)
            for mean in (False, True):
                out = NF.segsum(case.graph, side, x, w=wt, mean=mean)
                assert _close(out, want / cnt if mean else want, ATOL * (1 if mean else 30), RTOL), (F, wt is not None, mean)


@pytest.mark.gpu
def test_segsum_bf16(case):
    """bf16 storage, f32 accumulation: the float64 sum of the same bf16 values, rounded once to bf16 (2^-9 relative; 2^-8 allowed)"""
    from npi_gnn_amd import functional as NF
    side = case.graph.by_dst
    row, col = case.entries(side)
    x = case.randn(N_SRC, 256).bfloat16()
    w = case.rand(side.nnz_max)
    for wt in (None, w):
        vals = x.double()[col] if wt is None else wt[:case.E].double().view(-1, 1) * x.double()[col]
        want = _rowsum(row, vals, N_DST)
        out = NF.segsum(case.graph, side, x, w=wt)
        assert out.dtype == torch.bfloat16
        assert bool(((out.double() - want).abs() <= 2.0 ** -8 * want.abs() + ATOL * 30).all())


@pytest.mark.gpu
@pytest.mark.parametrize("H,C", [(1, 256), (2, 80)])
def test_gat_aggregate_by_target_and_by_source(case, H, C):
    from npi_gnn_amd import functional as NF
    d, s_ = case.graph.by_dst, case.graph.by_src
    a_dst, a_src = case.randn(N_DST, H, scale=2.0), case.randn(N_SRC, H, scale=2.0)
    row, col = case.entries(d)
    e = _lrelu(a_dst.double()[row] + a_src.double()[col])
    m64, s64 = _softmax_stats(row, e, N_DST)
    m, s = m64.float(), s64.float()
    # by target: out[i] = sum_p alpha_p x[col p], alpha_p = exp(e_p - m[i]) / (s[i] + 1e-16) per head
    x = case.randn(N_SRC, H * C)
    alpha = (e - m.double()[row]).exp() / (s.double()[row] + 1e-16)                                    # [E, H]
    want = _rowsum(row, (alpha.view(-1, H, 1) * x.double()[col].view(-1, H, C)).reshape(-1, H * C), N_DST)
    assert _close(NF._gat_aggregate(None, d, x, H, C, a_dst, a_src, m, s, SLOPE, False), want, ATOL, RTOL)
    if H == 1:                     # one head: the same launch also leaves alpha of every entry
        a_out = torch.empty(d.nnz_max, device=case.dev)
        assert _close(NF._gat_aggregate(None, d, x, H, C, a_dst, a_src, m, s, SLOPE, False, alpha=a_out), want, ATOL, RTOL)
        assert _close(a_out[:case.E], alpha.view(-1), ATOL, RTOL)
    # by source: out[j] = sum_q alpha_q y[col q] over the entries of SOURCE j (col = the target, whose a_dst / m / s make alpha),
    # plus the rank-1 terms g_dst[j] att[:C] + g_src[j] att[C:]
    row, col = case.entries(s_)
    y = case.randn(N_DST, H * C)
    alpha = (_lrelu(a_dst.double()[col] + a_src.double()[row]) - m.double()[col]).exp() / (s.double()[col] + 1e-16)
    want = _rowsum(row, (alpha.view(-1, H, 1) * y.double()[col].view(-1, H, C)).reshape(-1, H * C), N_SRC)
    assert _close(NF._gat_aggregate(None, s_, y, H, C, a_dst, a_src, m, s, SLOPE, True), want, BWD_ATOL, BWD_RTOL)
    g_dst, g_src, att = case.randn(N_SRC, H), case.randn(N_SRC, H), case.randn(H, 2 * C)
    rank1 = g_dst.double().view(-1, H, 1) * att.double()[:, :C] + g_src.double().view(-1, H, 1) * att.double()[:, C:]
    got = NF._gat_aggregate(None, s_, y, H, C, a_dst, a_src, m, s, SLOPE, True, g_dst=g_dst, g_src=g_src, att=att)
    assert _close(got, want + rank1.reshape(-1, H * C), BWD_ATOL, BWD_RTOL)
    if H == 1:                     # alpha read back through a map instead of recomputed: out[j] = sum_q alpha[map[q]] y[col q]
        a_in = case.rand(d.nnz_max)
        amap = torch.randint(0, case.E, (s_.nnz_max,), generator=case.g).to(torch.int32).to(case.dev)
        want = _rowsum(row, a_in.double()[amap[:case.E].long()].view(-1, 1) * y.double()[col], N_SRC)
        got = NF._gat_aggregate(None, s_, y, H, C, a_dst, a_src, m, s, SLOPE, True, alpha=a_in, alpha_map=amap)
        assert _close(got, want, BWD_ATOL, BWD_RTOL)
        got = NF._gat_aggregate(None, s_, y, H, C, a_dst, a_src, m, s, SLOPE, True, alpha=a_in, alpha_map=amap, g_dst=g_dst, g_src=g_src,
                                att=att)
        assert _close(got, want + rank1.reshape(-1, C), BWD_ATOL, BWD_RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [256, 100])
def test_gat_aggregate_on_read_back_scores_and_fused_forward(case, C):
    from npi_gnn_amd import functional as NF
    d = case.graph.by_dst
    row, col = case.entries(d)
    h = case.randn(N_SRC, C)
    bias = case.randn(C)
    # read-back scores: out[r] = sum_p exp(scores[p] - m[r]) / (s[r] + 1e-16) h[col p] + bias
    sc = case.randn(d.nnz_max, 1, scale=3.0)
    m64, s64 = _softmax_stats(row, sc[:case.E].double(), N_DST)
    m, s = m64.float(), s64.float()
    wgt = (sc[:case.E].double() - m.double()[row]).exp() / (s.double()[row] + 1e-16)
    want = _rowsum(row, wgt * h.double()[col], N_DST) + bias.double()
    assert _close(NF.gat_aggregate_scores(d, h, None, C, sc, m, s, bias=bias), want, ATOL, RTOL)
    # fused forward: the scores e_p = leaky_relu(a_dst[row] + <h[col p], att[C:]>) and the rows' (m, s) come out of the same launch
    att = case.randn(1, 2 * C, scale=6.0 / C ** 0.5)                  # scores spread over about +-20
    a_dst = case.randn(N_DST, scale=3.0)
    e = _lrelu(a_dst.double()[row] + (h.double() @ att.double()[0, C:])[col]).view(-1, 1)
    m64, s64 = _softmax_stats(row, e, N_DST)
    want = _rowsum(row, (e - m64[row]).exp() / (s64[row] + 1e-16) * h.double()[col], N_DST) + bias.double()
    out, m, s = NF.gat_aggregate_fused(d, h, None, C, a_dst, att, SLOPE, bias=bias)
    tol = 4e-6 * max(1.0, float(e.abs().max()))                     # test_fused_forward_statistics_equal_the_statistics_pass
    assert float((m.double() - m64).abs().max()) <= tol
    assert float(((s.double() - s64).abs() / s64.clamp(min=1e-30)).max()) <= 10 * tol + 2e-5
    assert float((out.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    empty = s64.view(-1) == 0
    assert int(empty.sum()) >= 2 and float(m[empty].abs().max()) == 0.0 and float(s[empty].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("H,C", [(1, 256), (1, 64), (2, 32), (4, 32), (8, 32)])
def test_gat_backward_fused(case, H, C):
    """out[j] = sum_q alpha_q dout[col q] and dz[q] = alpha_q (<dout[col q], hrow[j]> - D) leaky_relu'(z_q) per head, with
    (a_dst, m, 1 / s, D) = tpack[col q, head], z_q = a_dst + a_src[j], alpha_q = exp(leaky_relu(z_q) - m) / s; one head: also
    the row sums of dz"""
    from npi_gnn_amd import functional as NF
    side = case.graph.by_src
    row, col = case.entries(side)
    dout, hrow = case.randn(N_DST, H * C), case.randn(N_SRC, H * C)
    tpack = torch.randn(N_DST * H, 4, generator=case.g)
    tpack[:, 2] = tpack[:, 2].abs() * 0.1 + 0.01                    # 1 / s > 0
    tpack[:, 1] = tpack[:, 1].abs() + 2.0                           # the "row max": keeps exp(. - m) bounded
    tpack = tpack.to(case.dev)
    a_src = case.randn(N_SRC, H)
    t = tpack.double().view(N_DST, H, 4)[col]                       # [E, H, 4]
    z = t[:, :, 0] + a_src.double()[row]
    alpha = (_lrelu(z) - t[:, :, 1]).exp() * t[:, :, 2]
    dots = (dout.double()[col].view(-1, H, C) * hrow.double()[row].view(-1, H, C)).sum(-1)
    want_dz = alpha * (dots - t[:, :, 3]) * torch.where(z > 0, 1.0, SLOPE)
    want = _rowsum(row, (alpha.view(-1, H, 1) * dout.double()[col].view(-1, H, C)).reshape(-1, H * C), N_SRC)
    out, dz = NF.gat_backward_fused_packed(side, dout, None, hrow, C, tpack, a_src, SLOPE, H=H)
    assert _close(out, want, BWD_ATOL, BWD_RTOL)
    assert _close(dz[:case.E * H].view(-1, H), want_dz, BWD_ATOL, BWD_RTOL)
    if H == 1:
        gs = torch.full((N_SRC,), float("nan"), device=case.dev)
        out2, dz2 = NF.gat_backward_fused_packed(side, dout, None, hrow, C, tpack, a_src, SLOPE, H=H, rowsum_out=gs)
        assert torch.equal(out2, out) and torch.equal(dz2[:case.E], dz[:case.E])
        sums = _rowsum(row, dz[:case.E].double(), N_SRC)
        # test_fused_backward_pass_also_leaves_the_row_sums_of_dz
        tol = 2e-6 * max(1.0, float(sums.abs().max())) * max(1.0, (case.E / N_SRC) ** 0.5)
        assert not bool(torch.isnan(gs).any()) and float((gs.double() - sums).abs().max()) < tol
