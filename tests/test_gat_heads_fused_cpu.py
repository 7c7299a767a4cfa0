"""``npi_gat_aggregate_fused_heads`` without a GPU: the symbol, the ABI version, and every shape outside its contract refused with
``NPI_ERR_ARG`` before anything is launched (the arguments are checked on the host; no pointer is followed)."""
import ctypes

from npi_gnn_amd import _lib

NPI_ERR_ARG = -1
A = 0x10000                      # a 16-byte aligned stand-in for every pointer: never dereferenced by a refused call


def _call(lib, H, C, att=A, row_scales=None, item=64):
    return lib.npi_gat_aggregate_fused_heads(A, A, A, A, item, 100, 1000, A, H * C, None, 0, A, H * C, H, C, A, att, 0.2, A, 0,
                                             A, A, A, row_scales, None)


def test_symbol_and_abi_version():
    lib = _lib.load()
    assert "npi_gat_aggregate_fused_heads" in _lib.PROTOTYPES
    assert isinstance(lib.npi_gat_aggregate_fused_heads, ctypes._CFuncPtr)
    assert lib.npi_abi_version() == 4                                   # an additive change


def test_shapes_outside_the_contract_are_refused_before_a_launch():
    lib = _lib.load()
    cases = {"three heads": dict(H=3, C=32), "48 channels": dict(H=2, C=48), "H C = 512": dict(H=4, C=128),
             "row scales with two heads": dict(H=2, C=128, row_scales=A), "misaligned att": dict(H=4, C=64, att=A + 4),
             "bad item size": dict(H=4, C=64, item=100)}
    for name, kw in cases.items():
        assert _call(lib, **kw) == NPI_ERR_ARG, name
        msg = lib.npi_last_error().decode()
        assert "npi_gat_aggregate_fused_heads" in msg, (name, msg)


def test_carry_size_query_is_unchanged_in_kind():
    lib = _lib.load()
    for item in (64, 256):
        for F in (64, 128, 256):
            assert lib.npi_segsum_carry_elems(100_000, item, F) > 0
    assert lib.npi_segsum_carry_elems(1000, 100, 256) == -1             # no such item size
    # the (max, sum exp) slots of every partial row: 8 heads x 2 floats, two partial rows per workgroup (4 items) and per span
    wg = (100_000 // 64 + 1 + 3) // 4
    assert lib.npi_segsum_carry_elems(100_000, 64, 256) >= 2 * wg * (256 + 16)
