"""The power-of-two scales behind the fp16 x 2 arithmetic (NPI_GEMM_SPLIT_F16X2) on the data this project's gradients really are:
zero rows (TopK-dropped nodes, masked losses, ReLU-dead rows, empty CSR rows), tiny magnitudes, non-finite rows.  Every expected
scale comes from the definition, evaluated on the host in fp64: the power of two s with max |row| s in [2^14, 2^15), clamped to
[2^-126, 2^126]; NaN elements skipped; a row with no magnitude (all zero, all NaN, or holding an Inf) takes 2^126 (include/npi_gnn.h,
npi_row_scales).  The column scale derived from row scales (npi_col_scales with A == NULL) is the smallest of them: the scale of the
largest finite magnitude of the matrix, 2^126 when every row is zero, 1 when there is no row.  Products are checked against fp64
at GRAD_REL, and the layer path (GATConv's exposed dW GEMM) is checked to be the one actually taken."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import functional as NF
from npi_gnn_amd._lib import ptr, stream_ptr
from npi_gnn_amd.schedule import DEFAULT
from _util import GRAD_REL, rel_max
from oracle import ref_conv as R

pytestmark = pytest.mark.gpu

NO_MAGNITUDE = 2.0 ** 126           # the scale of a row with no finite magnitude (the clamp maximum)


def _scale_of(m: np.ndarray) -> np.ndarray:
    """the definition, in fp64: m = f 2^e with f in [0.5, 1) -> s = 2^(15 - e), so that m s is in [2^14, 2^15)"""
    m = np.asarray(m, dtype=np.float64)
    out = np.full(m.shape, NO_MAGNITUDE)
    ok = np.isfinite(m) & (m > 0)
    _, e = np.frexp(m[ok])
    out[ok] = np.ldexp(1.0, np.clip(15 - e, -126, 126))
    return out


def _row_max(a: torch.Tensor) -> np.ndarray:
    """largest |element| of every row, NaN skipped (an Inf stays: such a row has no finite scale)"""
    x = np.abs(a.detach().double().cpu().numpy())
    return np.where(np.isnan(x), 0.0, x).max(axis=1) if x.shape[0] else np.zeros(0)


def _ref_row_scales(a: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(_scale_of(_row_max(a))).float()


def _ref_uniform_col_scale(a: torch.Tensor) -> float:
    """the scale of the largest finite row maximum (rows holding an Inf contribute none); 1 without rows"""
    if a.size(0) == 0:
        return 1.0
    m = _row_max(a)
    m = m[np.isfinite(m)]
    return float(_scale_of(np.array([m.max() if m.size else 0.0]))[0])


def _matrix(case: str, M: int, K: int, dev, seed: int) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K, device=dev, generator=g)
    if M == 0:
        return a
    perm = torch.randperm(M, device=dev, generator=g)
    if case == "one_zero_row":
        a[M - 1] = 0                                              # the last row: the ragged tail of the partial minima
    elif case == "99pct_zero":
        a[perm[: (99 * M) // 100]] = 0
    elif case == "all_zero":
        a.zero_()
    elif case == "non_finite":
        a[perm[: max(1, M // 100)]] = 0
        a[perm[-1]] = float("inf")                                # a row of Inf
        if M > 2:
            a[perm[-2], 0] = float("nan")                         # NaN among finite values: skipped
            a[perm[-3]] = float("nan")                            # a row of NaN: no magnitude
    elif case.startswith("mag"):                                  # global magnitudes 1e-30 .. 1e+30, with a zero row
        a *= float(case[3:])
        a[perm[0]] = 0
    elif case == "ambiguous":
        # non-zero rows whose maximum is in [2^14, 2^15), plus zero rows: the column scale is 1 (2 would overflow fp16)
        a *= (1.5 * 2.0 ** 14) / a.abs().amax(dim=1, keepdim=True)
        a[perm[: M // 2]] = 0
    return a


_CASES = ["dense", "one_zero_row", "99pct_zero", "all_zero", "non_finite", "mag1e-30", "mag1e-10", "mag1e+10", "mag1e+30",
          "ambiguous"]


@pytest.mark.parametrize("M", [0, 1, 255, 256, 65_535, 65_537, 300_000])       # both launch shapes of the partial minima
@pytest.mark.parametrize("case", _CASES)
def test_col_scales_from_row_scales_follow_the_definition(dev, M, case):
    """npi_col_scales(A = NULL): one scale for every column -- that of the matrix's largest finite magnitude; a zero, NaN or Inf row
    never lowers it"""
    K = 8                                                         # (the row scales are what matters; cols is separate)
    a = _matrix(case, M, K, dev, seed=M + len(case))
    rs = NF.row_scales(a)
    for cols in (1, 256, 300):
        cs = NF.col_scales(row_scales=rs, cols=cols)
        want = _ref_uniform_col_scale(a)
        assert cs.shape == (cols,) and bool((cs == want).all()), (float(cs[0]), want)
    assert torch.equal(rs.cpu(), _ref_row_scales(a))
    if case == "all_zero" and M:
        assert float(cs[0]) == NO_MAGNITUDE
    if case == "ambiguous" and M > 1:
        assert float(cs[0]) == 1.0


def test_col_scales_of_a_matrix_follow_the_definition(dev):
    """npi_col_scales(A): per column, zero and Inf columns included"""
    g = torch.Generator(device=dev).manual_seed(31)
    a = torch.randn(5000, 384, device=dev, generator=g) * torch.pow(10.0, torch.linspace(-20, 20, 384, device=dev))
    a[::2] = 0
    a[:, 7] = 0
    a[:, 9] = 0
    a[3, 9] = float("inf")
    a[5, 11] = float("nan")
    cs = NF.col_scales(a)
    assert torch.equal(cs.cpu(), _ref_row_scales(a.t()))
    assert float(cs[7]) == NO_MAGNITUDE and float(cs[9]) == NO_MAGNITUDE


# ---- dW = A^T dC on two fp16 pieces per operand --------------------------------------------------------------------------------

def _zero_rows(x: torch.Tensor, perm: torch.Tensor, frac) -> None:
    n = 0 if frac == 0 else (1 if frac == "1row" else int(frac * x.size(0)))
    x[perm[:n]] = 0                                               # the same permutation for both operands: their non-zero rows overlap


def _dw_both_ways(a, dc):
    """(uniform column scales from the row scales, per-column scales from the column maxima)"""
    K, N = a.size(1), dc.size(1)
    assert NF.dw_f16x2_shape(a.size(0), K, N)
    uni = NF.linear_bwd_weight(a, dc, want_bias=False, a_cs=NF.col_scales(row_scales=NF.row_scales(a), cols=K),
                               dc_cs=NF.col_scales(row_scales=NF.row_scales(dc), cols=N))[0]
    col = NF.linear_bwd_weight(a, dc, want_bias=False, a_cs=NF.col_scales(a), dc_cs=NF.col_scales(dc))[0]
    return uni, col


@pytest.mark.parametrize("zeros", [(0, "1row"), ("1row", 0.5), (0.5, 0.99), (0.99, 0)])
@pytest.mark.parametrize("mag_dc", [1.0, 1e-3, 1e-6, 1e-8])
@pytest.mark.parametrize("mag_a", [1.0, 1e-3, 1e-6, 1e-8])
def test_weight_gradient_on_fp16x2_with_zero_rows_and_tiny_values(dev, mag_a, mag_dc, zeros):
    """linear_bwd_weight(a_cs=, dc_cs=) against fp64 at GRAD_REL: operands at 1 .. 1e-8, zero-row fractions 0 / one row / 50 % / 99 %
    (M >= 4096 with a ragged tail; K, N multiples of 128)"""
    M, K, N = 4133, 128, 256
    g = torch.Generator(device=dev).manual_seed(1000 + int(-np.log10(mag_a)) * 10 + int(-np.log10(mag_dc)))
    a = torch.randn(M, K, device=dev, generator=g) * mag_a
    dc = torch.randn(M, N, device=dev, generator=g) * mag_dc
    perm = torch.randperm(M, device=dev, generator=g)
    _zero_rows(a, perm, zeros[0])
    _zero_rows(dc, perm, zeros[1])
    ref = a.double().cpu().t() @ dc.double().cpu()
    assert float(ref.abs().max()) > 0
    for dw in _dw_both_ways(a, dc):
        assert rel_max(dw, ref) <= GRAD_REL, rel_max(dw, ref)


def test_weight_gradient_of_zero_operands_is_exactly_zero(dev):
    """every row zero: column scale 2^126 (no magnitude), and dW exactly zero; no row at all: scale 1"""
    M, K, N = 4100, 128, 128
    g = torch.Generator(device=dev).manual_seed(41)
    a = torch.zeros(M, K, device=dev)
    dc = torch.randn(M, N, device=dev, generator=g)
    for x, y in ((a, dc), (dc[:, :K].contiguous(), torch.zeros(M, N, device=dev)), (a, torch.zeros(M, N, device=dev))):
        assert float(NF.col_scales(row_scales=NF.row_scales(x), cols=K)[0]) == (NO_MAGNITUDE if not x.any() else
                                                                                 _ref_uniform_col_scale(x))
        for dw in _dw_both_ways(x, y):
            assert torch.isfinite(dw).all() and not dw.any()
    empty = torch.empty(0, device=dev)
    assert bool((NF.col_scales(row_scales=empty, cols=K) == 1.0).all())


def test_weight_gradient_in_the_ambiguous_case_stays_finite(dev):
    """rows with their maximum in [2^14, 2^15) next to zero rows: the uniform scale must be 1 -- a zero row must neither pull it
    below nor be skipped in a way that picks 2 (2^15 * 2 overflows fp16)"""
    M, K, N = 4133, 128, 128
    a = _matrix("ambiguous", M, K, dev, seed=51)
    dc = _matrix("ambiguous", M, N, dev, seed=52)
    dc[M // 2:] *= 2.0 ** -20                                      # (dC's non-zero rows at two levels)
    ref = a.double().cpu().t() @ dc.double().cpu()
    for dw in _dw_both_ways(a, dc):
        assert torch.isfinite(dw).all() and rel_max(dw, ref) <= GRAD_REL


@pytest.mark.parametrize("where", ["a_inf", "a_nan", "dc_inf", "dc_nan"])
def test_weight_gradient_with_a_non_finite_element(dev, where):
    """the entries of dW that an Inf / NaN operand element reaches are non-finite; every other entry stays at GRAD_REL"""
    M, K, N = 4133, 128, 256
    g = torch.Generator(device=dev).manual_seed(61)
    a = torch.randn(M, K, device=dev, generator=g) * 1e-3
    dc = torch.randn(M, N, device=dev, generator=g) * 1e-4
    a[::7] = 0
    dc[::5] = 0
    bad = float("inf") if where.endswith("inf") else float("nan")
    m0, k0, n0 = 1001, 17, 40
    if where.startswith("a"):
        a[m0, k0] = bad
    else:
        dc[m0 + 1, n0] = bad
    ref = a.double().cpu().t() @ dc.double().cpu()
    touched = torch.zeros(K, N, dtype=torch.bool)
    if where.startswith("a"):
        touched[k0] = True
    else:
        touched[:, n0] = True
    assert not torch.isfinite(ref[touched]).any() and torch.isfinite(ref[~touched]).all()
    for dw in _dw_both_ways(a, dc):
        dw = dw.cpu()
        assert not torch.isfinite(dw[touched]).any()
        assert torch.isfinite(dw[~touched]).all() and rel_max(dw[~touched], ref[~touched]) <= GRAD_REL


# ---- every producer of row scales agrees on zero rows --------------------------------------------------------------------------

def _check_scales_of(sc: torch.Tensor, out: torch.Tensor, zero_rows: torch.Tensor):
    assert torch.equal(sc, NF.row_scales(out))
    assert torch.equal(sc.cpu(), _ref_row_scales(out))
    assert bool(zero_rows.any()) and bool((sc[zero_rows] == NO_MAGNITUDE).all())


@pytest.mark.parametrize("item", [64, 256])
def test_aggregation_scales_of_empty_and_zero_rows(dev, item):
    """npi_segsum_ex(row_scales_out): empty rows (no self loops) and rows that gather only zero feature rows"""
    N, E, F = 6000, 30_000, 256
    g = torch.Generator().manual_seed(71)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei = ei[:, ei[1] % 10 != 3]                                   # a tenth of the rows receive nothing
    x = torch.randn(N, F, generator=g)
    dead = torch.randperm(N, generator=g)[: N // 5]
    x[dead] = 0
    gathers_dead = ei[1] % 10 == 5                                # these rows gather zero feature rows only
    ei[0, gathers_dead] = dead[torch.randint(0, dead.numel(), (int(gathers_dead.sum()),), generator=g)]
    graph = npi.CSRGraph(ei.to(dev), N, self_loops=False, item=item)
    xd = x.to(dev)
    for mean in (False, True):
        sc = torch.empty(N, device=dev)
        out = NF.segsum(graph, graph.by_dst, xd, mean=mean, scales_out=sc)
        zero = (out == 0).all(dim=1)
        assert bool(zero[torch.arange(3, N, 10, device=dev)].all()) and bool(zero[torch.arange(5, N, 10, device=dev)].all())
        _check_scales_of(sc, out, zero)


def _gat_inputs(N, E, C, dev, seed, isolated_frac=0.05):
    """features with ~10 % zero rows and some targets whose only entry is their (zero) self loop: with a negative bias and the
    fused ReLU those rows come out entirely zero"""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    iso = torch.randperm(N, generator=g)[: int(isolated_frac * N)]
    ei = ei[:, ~torch.isin(ei[1], iso)]
    x = torch.randn(N, C, generator=g)
    zero = torch.randperm(N, generator=g)[: N // 10]
    x[zero] = 0
    x[iso] = 0
    W = (torch.rand(C, C, generator=g) * 2 - 1) * (6.0 / (2 * C)) ** 0.5
    att = (torch.rand(1, 1, 2 * C, generator=g) * 2 - 1) * 0.3
    b = -(0.02 + 0.05 * torch.rand(C, generator=g))                 # every channel negative
    return ei, x, W, att, b, iso


@pytest.mark.parametrize("item", [64, 256])
def test_gat_fused_passes_write_the_scales_of_zero_rows(dev, item):
    """npi_gat_aggregate_fused(row_scales_out) with ReLU-dead rows, npi_gat_backward_fused_heads(row_scales_out) with sources that
    receive no gradient, and the entry-free side of gat_backward_fused_packed: bit-equal to npi_row_scales of the output and to the
    definition"""
    N, E, C = 5000, 40_000, 256
    ei, x, W, att, b, iso = _gat_inputs(N, E, C, dev, seed=80 + item)
    graph = npi.CSRGraph(ei.to(dev), N, item=item)
    att2 = att.view(1, 2 * C).to(dev)
    hfeat = (x @ W).to(dev)
    a_dst, a_src = NF.gat_scores(hfeat, att2, 1, C)
    sc = torch.empty(N, device=dev)
    out, m, s = NF.gat_aggregate_fused(graph.by_dst, hfeat, None, C, a_dst, att2, 0.2, bias=b.to(dev), relu=True, scales_out=sc)
    dead = (out == 0).all(dim=1)
    assert bool(dead[iso.to(dev)].all())
    _check_scales_of(sc, out, dead)
    # the backward's by-source pass: the gradient reaches ~2 % of the targets
    gm = torch.Generator().manual_seed(90 + item)
    go = torch.randn(N, C, generator=gm) * 1e-4
    go[torch.rand(N, generator=gm) > 0.02] = 0
    go = go.to(dev)
    D = NF.gat_rowdot(go, out, b.to(dev), 1, C)
    tpack = NF.gat_pack_targets(a_dst, m, s, D)
    sc2 = torch.empty(N, device=dev)
    dh, _ = NF.gat_backward_fused_packed(graph.by_src, go, None, hfeat, C, tpack, a_src, 0.2, scales_out=sc2)
    _check_scales_of(sc2, dh, (dh == 0).all(dim=1))
    # a side without entries: every row zero
    empty = npi.CSRGraph(torch.empty(2, 0, dtype=torch.int64, device=dev), N, self_loops=False, item=item)
    assert empty.by_src.nnz_max == 0
    sc3 = torch.full((N,), 5.0, device=dev)
    dh3, _ = NF.gat_backward_fused_packed(empty.by_src, go, None, hfeat, C, tpack, a_src, 0.2, scales_out=sc3)
    _check_scales_of(sc3, dh3, torch.ones(N, dtype=torch.bool, device=dev))


# ---- through the layer: GATConv's exposed dW GEMM ------------------------------------------------------------------------------

def _spy_dw(monkeypatch):
    calls = []
    real = NF.linear_bwd_weight

    def spy(a, dc, *args, **kw):
        calls.append((tuple(a.shape), tuple(dc.shape), kw.get("a_cs") is not None and kw.get("dc_cs") is not None))
        return real(a, dc, *args, **kw)
    monkeypatch.setattr(NF, "linear_bwd_weight", spy)
    return calls


def _assert_f16x2_dw_taken(calls, n_layers):
    taken = [c for c in calls if c[2] and NF.dw_f16x2_shape(c[0][0], c[0][1], c[1][1])]
    assert len(taken) == n_layers, calls


_SCH = DEFAULT.but(f16x2_min_rows=0, gat_rank2_min_rows=0)
_SCH_SIDE = _SCH.but(overlap_min_rows=0)          # (the HBM-bound passes on the side stream beside the dW GEMM, as at scale)


@pytest.mark.parametrize("sch", [_SCH, _SCH_SIDE], ids=["one_stream", "side_stream"])
@pytest.mark.parametrize("mag", [1e-4, 1e-6])
def test_gat_layer_dw_on_fp16x2_with_zero_rows_and_sparse_tiny_gradients(dev, monkeypatch, mag, sch):
    """one head, 256 channels, N >= 4096, x_scales = row_scales(x) with ~10 % zero feature rows, the gradient non-zero on ~2 % of the
    targets at 1e-4 / 1e-6 (most by-source rows of d hfeat are zero): dW, d att, db at GRAD_REL against the fp64 oracle, dX at the
    GAT tests' bar (on the gradient's own scale); the fp16 x 2 dW GEMM is the one that ran"""
    N, E, C = 12_000, 120_000, 256
    ei, x, W, att, b, _ = _gat_inputs(N, E, C, dev, seed=100)
    b = -b                                                        # (no ReLU here: a positive bias)
    g = torch.Generator().manual_seed(101)
    go = torch.randn(N, C, generator=g) * mag
    go[torch.rand(N, generator=g) > 0.02] = 0
    graph = npi.CSRGraph(ei.to(dev), N)
    calls = _spy_dw(monkeypatch)
    xd, Wd, ad, bd = (t.to(dev).requires_grad_(True) for t in (x, W, att, b))
    out = npi.gat_conv(xd, graph, Wd, ad, bd, heads=1, schedule=sch, x_scales=NF.row_scales(xd.detach()))
    out.backward(go.to(dev))
    _assert_f16x2_dw_taken(calls, 1)
    xr, Wr, ar, br = (t.clone().double().requires_grad_(True) for t in (x, W, att, b))
    ref = R.gat_conv(xr, ei, Wr, ar, br, heads=1)
    ref.backward(go.double())
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))
    for got, want in ((Wd.grad, Wr.grad), (ad.grad, ar.grad), (bd.grad, br.grad)):
        assert rel_max(got, want) <= GRAD_REL, rel_max(got, want)
    assert torch.allclose(xd.grad.cpu() / mag, xr.grad.float() / mag, atol=2e-4, rtol=1e-3)


def test_gat_stack_with_relu_dead_rows_hands_on_scales(dev, monkeypatch):
    """two layers, return_scales=True: layer 1's output has ReLU-dead rows (their scales 2^126), layer 2 takes them as its x_scales;
    a sparse gradient of 1e-5; every gradient at the stack bars of tests/test_gpu_f16x2.py against the fp64 oracle"""
    N, E, C = 12_000, 120_000, 256
    ei, x, W, att, b, iso = _gat_inputs(N, E, C, dev, seed=110)
    g = torch.Generator().manual_seed(111)
    W2 = (torch.rand(C, C, generator=g) * 2 - 1) * (6.0 / (2 * C)) ** 0.5
    att2 = (torch.rand(1, 1, 2 * C, generator=g) * 2 - 1) * 0.3
    b2 = torch.randn(C, generator=g) * 0.1
    go = torch.randn(N, C, generator=g) * 1e-5
    go[torch.rand(N, generator=g) > 0.02] = 0
    graph = npi.CSRGraph(ei.to(dev), N)
    calls = _spy_dw(monkeypatch)
    P = [t.to(dev).requires_grad_(True) for t in (W, W2, att, att2, b, b2)]
    xd = x.to(dev).requires_grad_(True)
    h1, s1 = npi.gat_conv(xd, graph, P[0], P[2], P[4], heads=1, relu=True, schedule=_SCH, x_scales=NF.row_scales(xd.detach()),
                          return_scales=True)
    dead = (h1.detach() == 0).all(dim=1)
    h2, _ = npi.gat_conv(h1, graph, P[1], P[3], P[5], heads=1, relu=True, schedule=_SCH, x_scales=s1, return_scales=True)
    h2.backward(go.to(dev))
    _assert_f16x2_dw_taken(calls, 2)
    P6 = [t.clone().double().requires_grad_(True) for t in (W, W2, att, att2, b, b2)]
    x6 = x.clone().double().requires_grad_(True)
    r1 = torch.relu(R.gat_conv(x6, ei, P6[0], P6[2], P6[4], heads=1))
    r2 = torch.relu(R.gat_conv(r1, ei, P6[1], P6[3], P6[5], heads=1))
    r2.backward(go.double())
    assert float((h2.detach().cpu().double() - r2.detach()).abs().max()) <= 1e-4 * max(1.0, float(r2.abs().max()))
    assert float((xd.grad.cpu().double() - x6.grad).abs().max()) <= 2e-4 * float(x6.grad.abs().max())
    for got, want in zip(P, P6):
        assert rel_max(got.grad, want.grad) <= 3 * GRAD_REL, rel_max(got.grad, want.grad)
    assert bool(dead[iso.to(dev)].all()) and bool((s1[dead] == NO_MAGNITUDE).all()) and torch.equal(s1, NF.row_scales(h1.detach()))


# ---- column scales are not kept between calls ----------------------------------------------------------------------------------

def test_col_scales_follow_a_scales_tensor_rewritten_by_a_library_launch(dev):
    """a kernel writes scales through a raw pointer (torch's version counter does not move): the next col_scales sees the new values"""
    N, F = 4096, 256
    g = torch.Generator(device=dev).manual_seed(121)
    a = torch.randn(N, F, device=dev, generator=g)
    sc = NF.row_scales(a)
    before = NF.col_scales(row_scales=sc, cols=F)
    assert float(before[0]) == _ref_uniform_col_scale(a)
    graph = npi.CSRGraph(torch.randint(0, N, (2, 20_000), device=dev, generator=g), N)
    out = NF.segsum(graph, graph.by_dst, a * 1e-3, mean=True, scales_out=sc)        # the same tensor, rewritten by the launch
    after = NF.col_scales(row_scales=sc, cols=F)
    assert float(after[0]) == _ref_uniform_col_scale(out) != float(before[0])


def _gat_step(x, graph, W, att, b, go, xs):
    xd, Wd, ad, bd = (t.clone().requires_grad_(True) for t in (x, W, att, b))
    npi.gat_conv(xd, graph, Wd, ad, bd, heads=1, schedule=_SCH_SIDE, x_scales=xs).backward(go)
    return [xd.grad, Wd.grad, ad.grad, bd.grad]


def test_gat_steps_with_x_scales_refreshed_in_place(dev, monkeypatch):
    """two steps that reuse ONE x_scales tensor, refreshed in place by npi_row_scales between them, equal runs with fresh scales bit
    for bit"""
    N, E, C = 6000, 50_000, 256
    ei, x, W, att, b, _ = _gat_inputs(N, E, C, dev, seed=130)
    x1, W, att, b = x.to(dev), W.to(dev), att.to(dev), b.to(dev)
    x2 = x1.flip(0) * 1e3
    g = torch.Generator().manual_seed(131)
    go = (torch.randn(N, C, generator=g) * 1e-3).to(dev)
    graph = npi.CSRGraph(ei.to(dev), N)
    calls = _spy_dw(monkeypatch)
    xs = NF.row_scales(x1)
    first = _gat_step(x1, graph, W, att, b, go, xs)
    assert NF.load().npi_row_scales(ptr(x2), x2.stride(0), N, C, ptr(xs), stream_ptr(dev)) == 0
    second = _gat_step(x2, graph, W, att, b, go, xs)
    _assert_f16x2_dw_taken(calls, 2)
    for got, want in zip(first + second, _gat_step(x1, graph, W, att, b, go, NF.row_scales(x1)) +
                         _gat_step(x2, graph, W, att, b, go, NF.row_scales(x2))):
        assert torch.equal(got, want)


def test_col_scales_under_capture_are_not_an_eager_result(dev):
    """inside torch.cuda.graph capture col_scales launches (its output belongs to the graph), whatever was computed eagerly"""
    g = torch.Generator(device=dev).manual_seed(141)
    a = torch.randn(4096, 128, device=dev, generator=g)
    sc = NF.row_scales(a)
    eager = NF.col_scales(row_scales=sc, cols=128)                 # kept alive
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        NF.col_scales(row_scales=sc, cols=128)
    torch.cuda.current_stream(dev).wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = NF.col_scales(row_scales=sc, cols=128)
    gr.replay()
    torch.cuda.synchronize(dev)
    assert cap.data_ptr() != eager.data_ptr() and torch.equal(cap, eager)


def test_replay_after_other_col_scales_calls_matches_eager(dev):
    """capture col_scales + the fp16 x 2 dW GEMM, then ask for the column scales of 8 other row-scale tensors, then replay: the
    replay reads nothing that was freed or rewritten since -- bit-equal to the eager result"""
    M, K, N = 4133, 128, 256
    g = torch.Generator(device=dev).manual_seed(151)
    a = torch.randn(M, K, device=dev, generator=g) * 1e-3
    dc = torch.randn(M, N, device=dev, generator=g) * 1e-5
    dc[::3] = 0
    sa, sd = NF.row_scales(a), NF.row_scales(dc)

    def dw():
        return NF.linear_bwd_weight(a, dc, want_bias=False, a_cs=NF.col_scales(row_scales=sa, cols=K),
                                    dc_cs=NF.col_scales(row_scales=sd, cols=N))[0]
    want = dw().clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        dw()
    torch.cuda.current_stream(dev).wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = dw()
    others = [NF.row_scales(torch.randn(M, K, device=dev, generator=g) * 10.0 ** (3 * i - 12)) for i in range(10)]
    kept = [NF.col_scales(row_scales=o, cols=n) for o in others for n in (K, N)]
    gr.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want)
    assert rel_max(want, a.double().cpu().t() @ dc.double().cpu()) <= GRAD_REL
    del kept
