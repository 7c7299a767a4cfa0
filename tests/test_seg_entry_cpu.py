"""The entry points of the aggregation family without a GPU: for each, one baseline argument list and one argument perturbed at a time.
Every case returns BEFORE any launch -- a refusal (``NPI_ERR_ARG`` -1, ``NPI_ERR_WORKSPACE`` -3) or the early ``NPI_OK`` of an empty call --
because the pointers are integer stand-ins that no kernel may follow (a baseline that passes validation is therefore never called).  The
expected statuses are those of the library before the entry points were rewritten over one call description (``seg_call.h``); a refusal's
message names the function that was called.  ``npi_gat_pack_targets`` is the control: an entry point outside that rewrite."""
import pytest

from npi_gnn_amd import _lib

A = 0x10000                      # a 16-byte aligned stand-in for every pointer: never dereferenced by a call that returns early
N = None
KEY, THRESHOLD, SCALE = 12345, 1 << 62, 2.0


def _segsum_ex(lib, rowptr=A, col=A, item_row=A, item=64, w=N, n=100, nnz=1000, x=A, ldx=256, x2=N, split=0, out=A, ldo=256, F=256,
               dtype=_lib.NPI_F32, bias=N, carry=A, scales=N):
    return lib.npi_segsum_ex(rowptr, col, item_row, item, w, n, nnz, x, ldx, x2, split, out, ldo, F, dtype, 0, bias, carry, scales, N)


def _aggregate_ex(lib, rowptr=A, col=A, item_row=A, item=64, n=100, nnz=1000, x=A, ldx=48, x2=N, split=0, out=A, ldo=48, H=3, C=16,
                  a_dst=A, a_src=A, m=A, s=A, by_source=0, alpha=N, alpha_map=N, carry=A):
    return lib.npi_gat_aggregate_ex(rowptr, col, item_row, item, n, nnz, x, ldx, x2, split, out, ldo, H, C, a_dst, a_src, m, s, 0.2,
                                    by_source, N, N, N, N, alpha, alpha_map, carry, N)


def _aggregate_scores(lib, rowptr=A, col=A, item_row=A, item=64, n=100, nnz=1000, x=A, ldx=64, x2=N, split=0, out=A, ldo=64, C=64,
                      scores=A, m=A, s=A, carry=A):
    return lib.npi_gat_aggregate_scores(rowptr, col, item_row, item, n, nnz, x, ldx, x2, split, out, ldo, C, scores, m, s, N, 0, carry, N)


def _fused(lib, rowptr=A, col=A, rowidx=A, item_row=A, item=64, n=100, nnz=1000, x=A, ldx=N, x2=N, split=0, out=A, ldo=N, C=64,
           a_dst=A, att=A, m=A, s=A, carry=A, scales=N):
    ldx, ldo = (C if ldx is None else ldx), (C if ldo is None else ldo)
    return lib.npi_gat_aggregate_fused(rowptr, col, rowidx, item_row, item, n, nnz, x, ldx, x2, split, out, ldo, C, a_dst, att, 0.2, N, 0,
                                       m, s, carry, scales, N)


def _fused_heads(lib, rowptr=A, col=A, rowidx=A, item_row=A, item=64, n=100, nnz=1000, x=A, ldx=N, x2=N, split=0, out=A, ldo=N, H=4,
                 C=64, a_dst=A, att=A, m=A, s=A, carry=A, scales=N, eid=False):
    """``eid=False``: the plain entry point; anything else (``None`` included): the dropout sibling with that eid"""
    ldx, ldo = (H * C if ldx is None else ldx), (H * C if ldo is None else ldo)
    args = (rowptr, col, rowidx, item_row, item, n, nnz, x, ldx, x2, split, out, ldo, H, C, a_dst, att, 0.2, N, 0, m, s, carry, scales, N)
    if eid is False:
        return lib.npi_gat_aggregate_fused_heads(*args)
    return lib.npi_gat_aggregate_fused_heads_dropout(*args, eid, KEY, THRESHOLD, SCALE)


def _backward(lib, rowptr=A, col=A, rowidx=A, item_row=A, item=64, n=100, nnz=1000, x=A, ldx=N, x2=N, split=0, hfeat=A, ldh=N,
              out=A, ldo=N, H=4, C=64, tpack=A, a_src=A, dz=A, carry=A, scales=N, g_src=N, ws=N, ws_elems=0, eid=False):
    F = H * C
    ldx, ldh, ldo = (F if ldx is None else ldx), (F if ldh is None else ldh), (F if ldo is None else ldo)
    args = (rowptr, col, rowidx, item_row, item, n, nnz, x, ldx, x2, split, hfeat, ldh, out, ldo, H, C, tpack, a_src, 0.2, dz,
            carry, scales, g_src, ws, ws_elems, N)
    if eid is False:
        return lib.npi_gat_backward_fused_heads(*args)
    return lib.npi_gat_backward_fused_heads_dropout(*args, eid, KEY, THRESHOLD, SCALE)


def _edge_grad(lib, rowptr=A, col=A, rowidx=A, n=100, nnz=1000, hfeat=A, ldh=N, hfeat2=N, split=0, dout=A, ldd=N, H=2, C=32, a_dst=A,
               a_src=A, m=A, s=A, D=A, swap=0, dz=A, eid=False):
    ldh, ldd = (H * C if ldh is None else ldh), (H * C if ldd is None else ldd)
    args = (rowptr, col, rowidx, n, nnz, hfeat, ldh, hfeat2, split, dout, ldd, H, C, a_dst, a_src, m, s, D, 0.2, swap, dz, N, N)
    if eid is False:
        return lib.npi_gat_edge_grad_ex(*args)
    return lib.npi_gat_edge_grad_dropout(*args, eid, KEY, THRESHOLD, SCALE)


def _pack_targets(lib, a_dst=A, m=A, s=A, D=A, n=100, tpack=A):
    return lib.npi_gat_pack_targets(a_dst, m, s, D, n, tpack, N)


# what every member of the family takes: the CSR side, the two-part table, the output
COMMON = {
    "item size 100": (dict(item=100), -1),
    "x2 with split -5": (dict(x2=A, split=-5), -1),
    "N = -1": (dict(n=-1), -1),
    "nnz_max = 0": (dict(nnz=0), -1),
    "null rowptr": (dict(rowptr=N), -1),
    "null carry": (dict(carry=N), -1),
    "ldx < F": (dict(ldx=8), -1),
    "ldo < F": (dict(ldo=8), -1),
}
EMPTY = dict(rowptr=N, col=N, item_row=N, x=N, out=N, carry=N, n=0)           # every pointer null, no rows: nothing to do
FUSED = {      # the fused forward, whichever entry point
    "att misaligned by 4 bytes": (dict(att=A + 4), -1),
    "null att": (dict(att=N), -1),
    "C = 30": (dict(C=30), -1),
}
HEADS = {      # the shapes of the several-head kernels, forward and backward
    "three heads": (dict(H=3, C=32), -1),
    "C = 30": (dict(H=1, C=30), -1),
    "C = 48 with two heads": (dict(H=2, C=48), -1),
    "H C = 512": (dict(H=4, C=128), -1),
}
FUSED_HEADS = {
    **COMMON, **FUSED, **HEADS,
    "one head of 300": (dict(H=1, C=300), -1),
    "row_scales_out with two heads": (dict(H=2, C=128, scales=A), -1),
    "row_scales_out with C != 256": (dict(H=1, C=64, scales=A), -1),
    "row_scales_out with misaligned rows": (dict(H=1, C=256, scales=A, x=A + 4), -1),
    "two heads, rows misaligned by 4 bytes": (dict(H=2, C=64, x=A + 4), -1),
    "two heads, carry misaligned by 4 bytes": (dict(H=2, C=64, carry=A + 4), -1),
    "two heads, odd pitch": (dict(H=2, C=64, ldx=130), -1),
    "every pointer null with N == 0": (dict(EMPTY, rowidx=N, a_dst=N, att=N, m=N, s=N), 0),
    "every pointer null with N == 0, one head": (dict(EMPTY, rowidx=N, a_dst=N, att=N, m=N, s=N, H=1), 0),
}
BACKWARD = {
    **COMMON, **HEADS,
    "null rowidx": (dict(rowidx=N), -1),
    "null tpack": (dict(tpack=N), -1),
    "tpack misaligned by 4 bytes": (dict(tpack=A + 4), -1),
    "ldh < F": (dict(ldh=8), -1),
    "row_scales_out with H C != 256": (dict(H=2, C=64, scales=A), -1),
    "row_scales_out with misaligned rows": (dict(scales=A, out=A + 4), -1),
    "g_src_out with two heads": (dict(H=2, C=64, g_src=A, ws=A, ws_elems=1 << 20), -1),
    "g_src_out with a workspace of 0 elements": (dict(H=1, C=64, g_src=A, ws=A, ws_elems=0), -3),
    "g_src_out with no workspace": (dict(H=1, C=64, g_src=A, ws=N, ws_elems=1 << 20), -3),
    "every pointer null with N == 0": (dict(n=0, rowptr=N, col=N, rowidx=N, item_row=N, x=N, hfeat=N, out=N, tpack=N, a_src=N, dz=N,
                                            carry=N), 0),
}
EDGE_GRAD = {
    "x2 with split -5": (dict(hfeat2=A, split=-5), -1),
    "N = -1": (dict(n=-1), -1),
    "nnz_max = -1": (dict(nnz=-1), -1),
    "nnz_max = 0": (dict(nnz=0), 0),                    # served: there is nothing to do
    "nnz_max = 0 and every pointer null": (dict(nnz=0, rowptr=N, col=N, rowidx=N, hfeat=N, dout=N, a_dst=N, a_src=N, m=N, s=N, D=N, dz=N), 0),
    "null rowptr": (dict(rowptr=N), -1),
    "null rowidx": (dict(rowidx=N), -1),
    "null dz": (dict(dz=N), -1),
    "no heads": (dict(H=0), -1),
    "C = 30": (dict(H=1, C=30), -1),
    "H C = 2048": (dict(H=8, C=256), -1),
    "pitch % 4": (dict(H=1, C=64, ldh=66), -1),
    "table misaligned by 4 bytes": (dict(hfeat=A + 4), -1),
    "second part misaligned by 4 bytes": (dict(hfeat2=A + 4, split=50), -1),
    "every pointer null with N == 0": (dict(n=0, rowptr=N, col=N, rowidx=N, hfeat=N, dout=N, a_dst=N, a_src=N, m=N, s=N, D=N, dz=N), 0),
}


def _with_eid(table, eid=A):
    return {name: (dict(kw, eid=eid), status) for name, (kw, status) in table.items()}


NULL_EID = {"null eid, one head": (dict(H=1, C=64, eid=N), -1), "null eid, four heads": (dict(H=4, C=64, eid=N), -1)}

# entry point -> (caller, {case: (perturbed arguments, status)})
TABLE = {
    "npi_segsum_ex": (_segsum_ex, {
        **{k: v for k, v in COMMON.items() if k != "nnz_max = 0"},
        "nnz_max = -1": (dict(nnz=-1), -1),
        "nnz_max = 0 with a bias": (dict(nnz=0, bias=A), -1),
        "F = 0": (dict(F=0), -1),
        "no such dtype": (dict(dtype=7), -1),
        "null col": (dict(col=N), -1),
        "row_scales_out with F != 256": (dict(F=128, ldx=128, ldo=128, scales=A), -1),
        "row_scales_out with bf16 rows": (dict(dtype=_lib.NPI_BF16, scales=A), -1),
        "row_scales_out with misaligned rows": (dict(scales=A, x=A + 4), -1),
        "row_scales_out without entries": (dict(nnz=0, scales=A), -1),
        "every pointer null with N == 0": (dict(EMPTY), 0),
    }),
    "npi_gat_aggregate_ex": (_aggregate_ex, {
        **COMMON,
        "no heads": (dict(H=0), -1),
        "null a_src": (dict(a_src=N), -1),
        "stored alpha with three heads": (dict(alpha=A), -1),
        "alpha read back without its map": (dict(H=1, C=16, ldx=16, ldo=16, alpha=A, by_source=1), -1),
        "every pointer null with N == 0": (dict(EMPTY, a_dst=N, a_src=N, m=N, s=N), 0),
    }),
    "npi_gat_aggregate_scores": (_aggregate_scores, {
        **COMMON,
        "C = 0": (dict(C=0), -1),
        "null scores": (dict(scores=N), -1),
        "every pointer null with N == 0": (dict(EMPTY, scores=N, m=N, s=N), 0),
    }),
    "npi_gat_aggregate_fused": (_fused, {
        **COMMON, **FUSED,
        "C = 300": (dict(C=300), -1),
        "row_scales_out with C != 256": (dict(scales=A), -1),
        "row_scales_out with misaligned rows": (dict(C=256, scales=A, out=A + 4), -1),
        "every pointer null with N == 0": (dict(EMPTY, rowidx=N, a_dst=N, att=N, m=N, s=N), 0),
    }),
    "npi_gat_aggregate_fused_heads": (_fused_heads, FUSED_HEADS),
    "npi_gat_aggregate_fused_heads_dropout": (_fused_heads, {**_with_eid(FUSED_HEADS), **NULL_EID}),
    "npi_gat_backward_fused_heads": (_backward, BACKWARD),
    "npi_gat_backward_fused_heads_dropout": (_backward, {**_with_eid(BACKWARD), **NULL_EID}),
    "npi_gat_edge_grad_ex": (_edge_grad, EDGE_GRAD),
    "npi_gat_edge_grad_dropout": (_edge_grad, {**_with_eid(EDGE_GRAD), **NULL_EID}),
    "npi_gat_pack_targets": (_pack_targets, {
        "N = -1": (dict(n=-1), -1),
        "null a_dst": (dict(a_dst=N), -1),
        "tpack misaligned by 4 bytes": (dict(tpack=A + 4), -1),
        "every pointer null with N == 0": (dict(a_dst=N, m=N, s=N, D=N, n=0, tpack=N), 0),
    }),
}
CASES = [(entry, name) for entry, (_, cases) in TABLE.items() for name in cases]


def status_of(lib, entry, name):
    call, cases = TABLE[entry]
    return call(lib, **cases[name][0])


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e}-{n}" for e, n in CASES])
def test_returns_before_a_launch_with_the_status_it_always_had(entry, name):
    lib = _lib.load()
    want = TABLE[entry][1][name][1]
    assert status_of(lib, entry, name) == want
    if want != 0:
        msg = lib.npi_last_error().decode()
        assert entry in msg, msg


def test_the_table_covers_the_family():
    assert len(TABLE) == 11 and all(entry in _lib.PROTOTYPES for entry in TABLE)
    for entry in ("npi_gat_aggregate_fused_heads_dropout", "npi_gat_backward_fused_heads_dropout", "npi_gat_edge_grad_dropout"):
        assert {"null eid, one head", "null eid, four heads"} <= set(TABLE[entry][1])
