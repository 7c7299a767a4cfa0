// Row gather into a column block of a wider buffer (include/npi_gnn.h: npi_rows_gather).
//
//     out[i, 0:F] = x[idx[i], 0:F]      i < n        (idx == NULL: the identity)
//
// The left half of the [N_dst, 2F] operand of the bipartite SAGEConv(concat=True) projection: PyG's
// `torch.cat([x[0][res_n_id], aggr_out], dim=-1)` reads x, writes the gathered copy, reads it again and writes the concatenation;
// here every row is read once and written once, straight into the GEMM operand.
//
// A pure streaming copy with one indirection per row, so the kernel is shaped for bytes in flight and nothing else: one wavefront
// owns RG_ROWS rows at a time, its lanes walk a row in consecutive 16-byte pieces (one fully coalesced 1 KiB access per wave and
// row at F = 256 f32), the RG_ROWS loads are issued before the first store, and the row index -- the same for every lane -- is
// read once per row through a wave-uniform address.  No LDS, a handful of registers: the CU keeps its full wave count, which is
// what hides the HBM latency of a copy.  Rows that are not 16-byte aligned (odd F, odd pitch or base) take the same loop on single
// elements.  An index outside [0, n_src) writes a ZERO row and raises NPI_STATUS_BAD_ROW_ID in the status word -- nothing is read
// out of bounds and the host learns of it at its next device read, without a synchronisation here.
#include "npi_common.h"

namespace npi {

constexpr int RG_WAVES = 4;      // wavefronts per workgroup
constexpr int RG_ROWS = 4;       // rows one wavefront keeps in flight

template <typename T> __device__ __forceinline__ T zero_piece() { return T(0); }
template <> __device__ __forceinline__ uint4 zero_piece<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }

// T: the piece one lane moves (uint4: 16 bytes; uint32_t / uint16_t: one f32 / bf16 element); width, ldx, ldo in pieces
template <typename T>
__global__ void __launch_bounds__(RG_WAVES * WAVE)
rows_gather_kernel(const T* __restrict__ x, int64_t ldx, int64_t n_src, const int64_t* __restrict__ idx, int64_t n, int width,
                   T* __restrict__ out, int64_t ldo, int32_t* __restrict__ status) {
    const int lane = lane_id();
    const int64_t r0 = ((int64_t)blockIdx.x * RG_WAVES + uniform_i(threadIdx.x >> 6)) * RG_ROWS;
    if (r0 >= n) return;
    int64_t src[RG_ROWS];                                      // first piece of the source row, -1: no row (a zero row / past n)
    bool bad = false;
#pragma unroll
    for (int q = 0; q < RG_ROWS; ++q) {
        const int64_t r = r0 + q;
        src[q] = -1;
        if (r < n) {
            const int64_t s = idx != nullptr ? idx[r] : r;
            if (s >= 0 && s < n_src) src[q] = s * ldx;
            else bad = true;
        }
    }
    if (bad && lane == 0 && status != nullptr) atomicOr(status, NPI_STATUS_BAD_ROW_ID);
    for (int c = lane; c < width; c += WAVE) {
        T v[RG_ROWS];
#pragma unroll
        for (int q = 0; q < RG_ROWS; ++q) v[q] = src[q] >= 0 ? x[src[q] + c] : zero_piece<T>();
#pragma unroll
        for (int q = 0; q < RG_ROWS; ++q)
            if (r0 + q < n) out[(r0 + q) * ldo + c] = v[q];
    }
}

template <typename T>
static int launch_rows_gather(const void* x, int64_t ldx, int64_t n_src, const int64_t* idx, int64_t n, int64_t width, void* out,
                              int64_t ldo, int32_t* status, hipStream_t stream) {
    const int64_t blocks = ceil_div(n, (int64_t)RG_WAVES * RG_ROWS);
    rows_gather_kernel<T><<<(unsigned)blocks, RG_WAVES * WAVE, 0, stream>>>(static_cast<const T*>(x), ldx, n_src, idx, n, (int)width,
                                                                           static_cast<T*>(out), ldo, status);
    return check_launch("npi_rows_gather");
}

}  // namespace npi

using namespace npi;

extern "C" int npi_rows_gather(const void* x, int64_t ldx, int64_t n_src, const int64_t* idx, int64_t n, int64_t F, void* out,
                               int64_t ldo, int dtype, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(dtype == NPI_F32 || dtype == NPI_BF16, "npi_rows_gather: dtype must be NPI_F32 or NPI_BF16");
    NPI_REQUIRE(n >= 0 && n_src >= 0 && F > 0 && F < ((int64_t)1 << 31) && ldx >= F && ldo >= F, "npi_rows_gather: bad size");
    NPI_REQUIRE(ceil_div(n, (int64_t)RG_WAVES * RG_ROWS) < ((int64_t)1 << 31), "npi_rows_gather: too many rows for one launch");
    if (n == 0) return NPI_OK;
    NPI_REQUIRE(out && (x || n_src == 0), "npi_rows_gather: null pointer");
    const int64_t es = dtype == NPI_F32 ? 4 : 2;               // bytes per element
    const int64_t per = 16 / es;                               // elements per 16-byte piece
    const bool v16 = F % per == 0 && ldx % per == 0 && ldo % per == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0;
    if (v16) return launch_rows_gather<uint4>(x, ldx / per, n_src, idx, n, F / per, out, ldo / per, status, stream);
    if (dtype == NPI_F32) return launch_rows_gather<uint32_t>(x, ldx, n_src, idx, n, F, out, ldo, status, stream);
    return launch_rows_gather<uint16_t>(x, ldx, n_src, idx, n, F, out, ldo, status, stream);
}
