"""One case per branch of the projection GEMMs' host dispatch (csrc/gemm_f32.hip: plan_gemm, npi_linear_bwd_weight_ex), through the
public ``functional`` wrappers against a float64 product.  The tolerances are the neighbours': ``ATOL`` / ``RTOL`` and the sqrt(M)
scaling of ``test_linear_fwd_bwd`` for the f32 kernels, the relative bound of ``test_split_bf16_gemm_is_f32_accurate`` for the split
kernels, the bf16-rounded-input comparisons of ``test_bf16_mfma_gemm_matches_f32_reference`` / ``test_bf16_dw_matches_f32_reference``
for bf16 storage.  ``CASES`` is importable: a script can run the same inputs through two builds of the library and compare bits."""
import pytest
import torch

from npi_gnn_amd import functional as NF
from npi_gnn_amd import _lib
from npi_gnn_amd._lib import NPI_GEMM_EXACT_F32, NpiError, ptr, stream_ptr

pytestmark = pytest.mark.gpu

ATOL = 1e-4
RTOL = 1e-4
EXACT = NPI_GEMM_EXACT_F32
F32, BF16 = torch.float32, torch.bfloat16

# (branch, call, (M, K, N), options).  Options: dtype, flags, ka (width of a zero-padded a), scales (fp16 x 2), reserve_cus,
# f16 (prepared planes of the fp16 x 2 kind), shared, bias
CASES = [
    ("split narrow, ragged last row tile", "fwd", (130, 64, 128), {}),
    ("guarded, output 64 wide", "bwd_data", (130, 64, 128), {}),
    ("split narrow (the output is K wide), ragged last row tile", "bwd_data", (130, 128, 64), {}),
    ("split wide, ragged last row tile", "fwd", (130, 64, 256), {}),
    ("guarded, output 64 wide, contraction 256", "bwd_data", (130, 64, 256), {}),
    ("split wide (the output is K wide), ragged last row tile", "bwd_data", (130, 256, 64), {}),
    ("split plus a right guarded strip", "fwd", (130, 64, 300), {}),
    ("exact fast kernel, no strips", "fwd", (256, 32, 128), {"flags": EXACT}),
    ("exact, one guarded launch", "fwd", (300, 128, 128), {"flags": EXACT}),
    ("exact, fast kernel plus bottom and right strips", "fwd", (2051, 32, 1924), {"flags": EXACT}),
    ("unvectorised", "fwd", (129, 65, 2), {}),
    ("unvectorised", "bwd_data", (129, 65, 2), {}),
    ("unvectorised", "bwd_weight", (129, 65, 2), {}),
    ("zero-padded a, split on the padded width", "fwd", (130, 178, 128), {"ka": 256}),
    ("zero-padded a, split dW on the padded width", "bwd_weight", (4103, 178, 128), {"ka": 256}),
    ("zero-padded a, back to k_valid: fewer than 128 rows", "fwd", (37, 178, 128), {"ka": 256}),
    ("zero-padded a, back to k_valid: exact", "fwd", (130, 178, 128), {"ka": 256, "flags": EXACT}),
    ("bf16 persistent narrow", "fwd", (130, 64, 128), {"dtype": BF16}),
    ("bf16 guarded, output 64 wide", "bwd_data", (130, 64, 128), {"dtype": BF16}),
    ("bf16 persistent narrow (the output is K wide)", "bwd_data", (130, 128, 64), {"dtype": BF16}),
    ("bf16 persistent wide", "fwd", (130, 64, 256), {"dtype": BF16}),
    ("bf16 guarded, output 64 wide, contraction 256", "bwd_data", (130, 64, 256), {"dtype": BF16}),
    ("bf16 persistent wide (the output is K wide)", "bwd_data", (130, 256, 64), {"dtype": BF16}),
    ("bf16 guarded only (K % 64 != 0)", "fwd", (130, 96, 128), {"dtype": BF16}),
    ("prepared forward equals unprepared (bwd_data 64 wide: guarded, reads no copy)", "prepared", (130, 64, 128), {}),
    ("prepared forward equals unprepared, fp16 x 2 (bwd_data guarded)", "prepared", (130, 64, 128), {"f16": True}),
    ("prepared forward and bwd_data equal unprepared", "prepared", (130, 128, 128), {}),
    ("prepared forward and bwd_data equal unprepared, fp16 x 2", "prepared", (130, 128, 128), {"f16": True}),
    ("prepared forward and bwd_data equal unprepared, bf16", "prepared", (130, 128, 128), {"dtype": BF16}),
    ("fp16 x 2", "fwd", (130, 128, 128), {"scales": True}),
    ("fp16 x 2", "bwd_data", (130, 128, 128), {"scales": True}),
    ("reserve_cus = 8", "fwd", (1000, 256, 256), {"reserve_cus": 8}),
    ("rank-2 epilogue, smallest", "rank2", (128, 128, 32), {}),
    ("row-dot epilogue, smallest", "scores", (128, 64, 128), {}),
    ("dW, fewer than 32 nodes", "bwd_weight", (20, 64, 64), {}),
    ("dW, fewer than 32 nodes, no bias", "bwd_weight", (20, 64, 64), {"bias": False}),
    ("dW, fewer than 32 nodes, bf16", "bwd_weight", (20, 64, 64), {"dtype": BF16}),
    ("dW, fewer than 32 nodes, bf16, no bias", "bwd_weight", (20, 64, 64), {"dtype": BF16, "bias": False}),
    ("dW, slabs plus trailing nodes in the finish launch", "bwd_weight", (33, 96, 130), {}),
    ("dW, slabs plus trailing nodes in the finish launch, bf16", "bwd_weight", (33, 96, 130), {"dtype": BF16}),
    ("dW split kernel, narrow", "bwd_weight", (4103, 128, 128), {}),
    ("dW split kernel, narrow, shared", "bwd_weight", (4103, 128, 128), {"shared": True}),
    ("dW split kernel, wide", "bwd_weight", (4103, 128, 256), {}),
    ("dW split kernel, wide, shared", "bwd_weight", (4103, 128, 256), {"shared": True}),
    ("dW split kernel, bf16 operands", "bwd_weight", (4103, 128, 128), {"dtype": BF16}),
    ("dW split kernel, fp16 x 2", "bwd_weight", (4103, 128, 128), {"scales": True}),
]
# (linear_bwd_data's output is K wide and its contraction runs over N: at K = 64 the output has no full 128-wide tile and the
# guarded kernel takes it, whatever N is.  Those shapes stay, named for what they run; the matrix-core kernels of bwd_data -- and
# with them the prepared copy of W^T -- are reached at (130, 128, 64), (130, 256, 64) and (130, 128, 128).)


def case_inputs(call, shape, opt):
    """the case's operands on the host, seeded by the case: ``randn``, the weight scaled by 1 / sqrt(K)"""
    M, K, N = shape
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N + len(call))
    dt = opt.get("dtype", F32)
    t = {"a": torch.randn(M, K, generator=g), "w": torch.randn(K, N, generator=g) / K ** 0.5, "b": torch.randn(N, generator=g),
         "dc": torch.randn(M, N, generator=g)}
    t = {k: v.to(dt) for k, v in t.items()}
    t["rs"] = torch.rand(M, generator=g) + 0.5
    for name, n in (("r0", M), ("r1", M), ("c0", K), ("c1", K)):
        t[name] = torch.randn(n, generator=g)
    t["att"] = torch.randn(2 * N, generator=g)
    if "ka" in opt:                                              # the zero pad columns of NPI_GEMM_A_ZERO_PADDED
        t["a_pad"] = torch.zeros(M, opt["ka"])
        t["a_pad"][:, :K] = t["a"]
    return t


def run_case(call, shape, opt, dev):
    """``(inputs on the host, {name: output on the device})`` of one case"""
    M, K, N = shape
    t = case_inputs(call, shape, opt)
    d = {k: v.to(dev) for k, v in t.items()}
    a = d.get("a_pad", d["a"])
    flags, out = opt.get("flags"), {}
    if call == "fwd":
        out["c"] = NF.linear_fwd(a, d["w"], d["b"], rowscale=d["rs"], relu=True, flags=flags, reserve_cus=opt.get("reserve_cus", 0),
                                 a_scales=NF.row_scales(a) if opt.get("scales") else None)
    elif call == "bwd_data":
        out["da"] = NF.linear_bwd_data(d["dc"], d["w"], d["rs"], flags=flags, dc_scales=NF.row_scales(d["dc"]) if opt.get("scales") else None)
    elif call == "bwd_weight":
        cs = (NF.col_scales(a), NF.col_scales(d["dc"])) if opt.get("scales") else (None, None)
        out["dw"], db = NF.linear_bwd_weight(a, d["dc"], opt.get("bias", True), shared=opt.get("shared", False), flags=flags,
                                             k_valid=K if "ka" in opt else None, a_cs=cs[0], dc_cs=cs[1])
        assert (db is None) == (not opt.get("bias", True))
        if db is not None:
            out["db"] = db
    elif call == "prepared":
        f16 = bool(opt.get("f16"))
        wsf, wsb = NF.prepare_weight(d["w"], f16=f16)
        sa, sdc = (NF.row_scales(a), NF.row_scales(d["dc"])) if f16 else (None, None)
        out["c"] = NF.linear_fwd(a, d["w"], d["b"], relu=True, a_scales=sa)
        out["c_prepared"] = NF.linear_fwd(a, d["w"], d["b"], relu=True, ws=wsf, a_scales=sa)
        out["da"] = NF.linear_bwd_data(d["dc"], d["w"], d["rs"], dc_scales=sdc)
        out["da_prepared"] = NF.linear_bwd_data(d["dc"], d["w"], d["rs"], ws=wsb, dc_scales=sdc)
    elif call == "rank2":
        out["da"] = NF.linear_bwd_data_rank2(d["dc"], d["w"], d["r0"], d["r1"], d["c0"], d["c1"])
    elif call == "scores":
        out["h"], out["s0"], out["s1"] = NF.linear_fwd_scores(a, d["w"], d["att"])
    return t, out


def reference(call, shape, opt, t):
    """float64 products of the operands as stored (bf16 storage: of the bf16-rounded values)"""
    N = shape[2]
    a, w, b, dc, rs = (t[k].double() for k in ("a", "w", "b", "dc", "rs"))
    fwd, bwd = a @ w, dc @ w.t()
    if call == "fwd":
        return {"c": torch.relu(rs[:, None] * fwd + b)}
    if call == "bwd_data":
        return {"da": rs[:, None] * bwd}
    if call == "bwd_weight":
        return {"dw": a.t() @ dc, "db": dc.sum(0)}
    if call == "prepared":
        return {"c": torch.relu(fwd + b), "da": rs[:, None] * bwd}
    if call == "rank2":
        return {"da": bwd + torch.outer(t["r0"].double(), t["c0"].double()) + torch.outer(t["r1"].double(), t["c1"].double())}
    att = t["att"].double()
    return {"h": fwd, "s0": (fwd @ att[:N])[:, None], "s1": (fwd @ att[N:])[:, None]}


def _split_shape(call, shape, opt):
    """does a forward / bwd_data call take a matrix-core split kernel on f32 storage (the bound of
    test_split_bf16_gemm_is_f32_accurate applies)?  dW has its own bounds in check_case."""
    M, K, N = shape
    if opt.get("flags") or opt.get("dtype", F32) != F32 or call == "bwd_weight":
        return False
    contraction, width = (N, K) if call in ("bwd_data", "rank2") else (opt.get("ka", K), N)
    return M >= 128 and contraction % 32 == 0 and width >= 128


def check_case(call, shape, opt, t, out):
    M = shape[0]
    ref = reference(call, shape, opt, t)
    bf16 = opt.get("dtype", F32) == BF16
    for name, got in out.items():
        assert bool(torch.isfinite(got).all()), name
        if name.endswith("_prepared"):                           # as test_prepared_weight_copies_give_the_same_bits
            assert torch.equal(got, out[name[:-len("_prepared")]]), name
            continue
        want = ref[name]
        got = got.double().cpu()
        err = (got - want).abs()
        rel = float(err.max() / want.abs().max())
        print(f"{call} {shape} {opt} {name}: max |err| {float(err.max()):.3e}, relative to max |ref| {rel:.3e}")
        if bf16 and call == "bwd_weight":
            assert float(err.max()) <= 2.0 ** -7 * float(want.abs().max()), name       # one bf16 rounding of the result
        elif bf16:
            assert float((err / (want.abs() + 1.0)).max()) < 1e-2, name                 # one bf16 rounding of the result (2^-8)
            assert float(err.mean()) < 2e-3 * max(1.0, float(want.abs().mean())), name
        elif _split_shape(call, shape, opt) and name not in ("s0", "s1", "db"):
            assert rel < 2e-6, name
        else:
            scale = 4 if call in ("bwd_data", "rank2") else max(1.0, M ** 0.5) if call == "bwd_weight" else 1
            assert torch.allclose(got, want, atol=ATOL * scale, rtol=RTOL), name
            if call == "bwd_weight" and name == "dw" and M >= 4096:  # the split dW kernel: test_linear_bwd_weight_large_m_split's bound
                assert rel <= 1e-5, name


@pytest.mark.parametrize("branch,call,shape,opt", CASES, ids=[f"{c[1]}-{c[0]}" for c in CASES])
def test_dispatch_branch(dev, branch, call, shape, opt):
    t, out = run_case(call, shape, opt, dev)
    check_case(call, shape, opt, t, out)


def test_argument_checks_of_the_data_gemms(dev):
    """the host-side refusals the four data-GEMM entry points share: nothing is launched"""
    lib = _lib.load()
    M, K, N = 130, 128, 128                                       # a shape all four entry points serve
    a = torch.randn(M, K, device=dev)
    w = torch.randn(K, N, device=dev)
    c = torch.empty(M, N, device=dev)
    att, s = torch.randn(2 * N, device=dev), torch.empty(M, device=dev)
    need = int(lib.npi_linear_workspace_bytes(K, N))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = stream_ptr(dev)

    def fwd(lda=K, nbytes=need, dtype=0, k=K):
        return lib.npi_linear_fwd_ex(ptr(a), lda, ptr(w), N, 0, 0, ptr(c), N, M, k, N, 0, dtype, 0, ptr(ws), nbytes, 0, st)

    def bwd(ldda=K, nbytes=need):
        return lib.npi_linear_bwd_data_ex(ptr(c), N, ptr(w), N, 0, ptr(a), ldda, M, K, N, 0, 0, ptr(ws), nbytes, 0, st)

    def scores(lda=K, nbytes=need, a_=a):
        return lib.npi_linear_fwd_scores(ptr(a_), lda, ptr(w), N, ptr(att), ptr(c), N, ptr(s), ptr(s), M, K, N, ptr(ws), nbytes, 0, st)

    def rank2(ldda=K, nbytes=need, row0=s):
        return lib.npi_linear_bwd_data_rank2(ptr(c), N, ptr(w), N, ptr(row0), ptr(s), ptr(a[0]), ptr(a[1]), ptr(a), ldda, M, K, N,
                                             ptr(ws), nbytes, 0, st)

    ARG, WORKSPACE = -1, -3
    for name, call in (("npi_linear_fwd_ex", fwd), ("npi_linear_bwd_data_ex", bwd), ("npi_linear_fwd_scores", scores),
                       ("npi_linear_bwd_data_rank2", rank2)):
        assert call(nbytes=need - 1) == WORKSPACE, name          # a workspace one byte short
        stem = name[:-3].encode() if name.endswith("_ex") else name.encode()
        assert stem in lib.npi_last_error() and b"workspace" in lib.npi_last_error()
        assert call(K - 4) == ARG, name                          # a leading dimension that does not cover the row
        assert stem in lib.npi_last_error() and b"leading dimension" in lib.npi_last_error()
    assert fwd(dtype=7) == ARG and b"bad dtype" in lib.npi_last_error()
    assert fwd(k=0) == ARG and b"bad size" in lib.npi_last_error()
    assert scores(a_=None) == ARG and b"null pointer" in lib.npi_last_error()
    assert rank2(row0=None) == ARG and b"null pointer" in lib.npi_last_error()
    with pytest.raises(NpiError):                                 # the wrappers turn a refusal into NpiError
        _lib.check(fwd(nbytes=need - 1), "npi_linear_fwd")
    with pytest.raises(ValueError):                               # out= of another shape never reaches the library
        NF.linear_fwd(a, w, out=torch.empty(M, N + 1, device=dev))
    with pytest.raises(ValueError):
        NF.linear_bwd_data(c, w, out=torch.empty(M + 1, K, device=dev))
