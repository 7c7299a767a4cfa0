// Negative sampling on the device: the pairs a link-prediction loss is taken against.  Replaces the reference's offline loop
// src/generate_edgelist.py:108-139 (draw a uniform ncRNA and a uniform protein, redraw a positive or a repeat, stop at as many
// negatives as positives) and PyG 1.4.2 `torch_geometric.utils.negative_sampling` / `structured_negative_sampling` (Python
// `random.sample` + `isin` on the CPU).
//
// THE RULES (include/npi_gnn.h states them).  Wrapping uint64 throughout, mix64 the sampler's (sample.hip),
// G = 0x9E3779B97F4A7C15, C = 0xD6E8FEB86659FD93, mulhi(a, n) = the upper 64 bits of a * n:
//     Rule P:  base = mix64(mix64(key) + G);  candidate i = (mulhi(mix64(base + G (2i + 1)), n_src), mulhi(mix64(base + G (2i + 2)), n_dst))
//     Rule T:  base_k = mix64(mix64(mix64(key) + 2 G) ^ (k C));  try t of slot k = mulhi(mix64(base_k + G (t + 1)), n_dst)
// Both kernels answer "is (s, d) an edge" the same way: the two rowptr loads of row d of the by-target CSR with SORTED columns and a
// binary search of the row for s.  One lane per candidate / slot, grid-stride; a chain of dependent gathers, so the kernels keep
// few registers and no LDS and rely on occupancy.  npi_negative_distinct (csr_build.hip) turns a window of candidates into the
// first M distinct valid ones.
#include "npi_common.h"

namespace npi {

constexpr int NEG_BLOCK = 256;
constexpr uint64_t NEG_G = 0x9E3779B97F4A7C15ull;
constexpr uint64_t NEG_C = 0xD6E8FEB86659FD93ull;

__host__ __device__ __forceinline__ uint64_t neg_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ int32_t neg_below(uint64_t word, int64_t n) { return (int32_t)__umul64hi(word, (uint64_t)n); }

// is s a column of row d?  Rows ascend; empty rows, rows of one entry and rows with repeated columns all occur.
__device__ __forceinline__ bool is_edge(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t s, int32_t d) {
    int lo = rowptr[d], hi = rowptr[d + 1];
    while (lo < hi) {                                      // first position with col >= s
        const int mid = lo + ((hi - lo) >> 1);
        if (col[mid] < s) lo = mid + 1; else hi = mid;
    }
    return lo < rowptr[d + 1] && col[lo] == s;
}

__global__ void __launch_bounds__(NEG_BLOCK)
negative_candidates_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_dst, int64_t n_src,
                           uint64_t base, int64_t first, int64_t W, int no_loops, int32_t* __restrict__ cand_src,
                           int32_t* __restrict__ cand_dst) {
    const int64_t nt = (int64_t)gridDim.x * NEG_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * NEG_BLOCK + threadIdx.x; j < W; j += nt) {
        const uint64_t i = (uint64_t)(first + j);
        const int32_t s = neg_below(neg_mix64(base + NEG_G * (2 * i + 1)), n_src);
        const int32_t d = neg_below(neg_mix64(base + NEG_G * (2 * i + 2)), n_dst);
        const bool valid = !(no_loops && s == d) && !is_edge(rowptr, col, s, d);
        cand_src[j] = valid ? s : -1;
        cand_dst[j] = valid ? d : -1;
    }
}

__global__ void __launch_bounds__(NEG_BLOCK)
negative_targets_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_dst, int64_t n_src,
                        const int64_t* __restrict__ src, int64_t K, uint64_t key_base, int tries, int64_t* __restrict__ out_dst,
                        int32_t* __restrict__ status) {
    const int64_t nt = (int64_t)gridDim.x * NEG_BLOCK;
    int bits = 0;
    for (int64_t k = (int64_t)blockIdx.x * NEG_BLOCK + threadIdx.x; k < K; k += nt) {
        const int64_t s = src[k];
        int64_t out = -1;
        if (s < 0 || s >= n_src) {                         // reported, never dereferenced
            bits |= NPI_STATUS_BAD_SOURCE_ID;
        } else {
            const uint64_t base = neg_mix64(key_base ^ ((uint64_t)k * NEG_C));
            for (int t = 0; t < tries; ++t) {
                const int32_t d = neg_below(neg_mix64(base + NEG_G * (uint64_t)(t + 1)), n_dst);
                if (!is_edge(rowptr, col, (int32_t)s, d)) {
                    out = d;
                    break;
                }
            }
            if (out < 0) bits |= NPI_STATUS_NO_NEGATIVE;
        }
        out_dst[k] = out;
    }
    if (bits != 0 && status != nullptr) atomicOr(status, bits);
}

}  // namespace npi

using namespace npi;

// enough workgroups for 8 wavefronts on every SIMD of 256 CUs; more work than that strides
static unsigned neg_grid(int64_t work) {
    const int64_t g = ceil_div(work, NEG_BLOCK);
    return (unsigned)(g < 2048 ? g : 2048);
}

extern "C" int npi_negative_candidates(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t n_src, int64_t key,
                                       int64_t first, int64_t W, int flags, int32_t* cand_src, int32_t* cand_dst, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(W >= 0 && W < (int64_t)0x7fffffff, "npi_negative_candidates: bad window size");
    NPI_REQUIRE(n_src >= 1 && n_src < (int64_t)0x7fffffff && n_dst >= 1 && n_dst < (int64_t)0x7fffffff,
                "npi_negative_candidates: bad id bound");
    NPI_REQUIRE(first >= 0 && first <= (int64_t)1 << 40, "npi_negative_candidates: bad first candidate");
    NPI_REQUIRE((flags & ~1) == 0, "npi_negative_candidates: unknown flag");
    NPI_REQUIRE(rowptr && col, "npi_negative_candidates: null pointer");
    if (W == 0) return NPI_OK;
    NPI_REQUIRE(cand_src && cand_dst, "npi_negative_candidates: null pointer");
    const uint64_t base = neg_mix64(neg_mix64((uint64_t)key) + NEG_G);
    negative_candidates_kernel<<<neg_grid(W), NEG_BLOCK, 0, stream>>>(rowptr, col, n_dst, n_src, base, first, W, flags & 1, cand_src,
                                                                    cand_dst);
    return check_launch("npi_negative_candidates");
}

extern "C" int npi_negative_targets(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t n_src, const int64_t* src,
                                    int64_t K, int64_t key, int64_t tries, int64_t* out_dst, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(K >= 0 && K < (int64_t)0x7fffffff, "npi_negative_targets: bad slot count");
    NPI_REQUIRE(n_src >= 1 && n_src < (int64_t)0x7fffffff && n_dst >= 1 && n_dst < (int64_t)0x7fffffff,
                "npi_negative_targets: bad id bound");
    NPI_REQUIRE(tries >= 1 && tries < (int64_t)0x7fffffff, "npi_negative_targets: tries below 1");
    NPI_REQUIRE(rowptr && col, "npi_negative_targets: null pointer");
    if (K == 0) return NPI_OK;
    NPI_REQUIRE(src && out_dst, "npi_negative_targets: null pointer");
    if (status != nullptr) (void)hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    const uint64_t kb = neg_mix64(neg_mix64((uint64_t)key) + 2 * NEG_G);
    negative_targets_kernel<<<neg_grid(K), NEG_BLOCK, 0, stream>>>(rowptr, col, n_dst, n_src, src, K, kb, (int)tries, out_dst, status);
    return check_launch("npi_negative_targets");
}
