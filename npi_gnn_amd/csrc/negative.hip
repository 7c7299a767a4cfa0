// Negative sampling on the device: the pairs a link-prediction loss is taken against.  Replaces the reference's offline loop
// src/generate_edgelist.py:108-139 (draw a uniform ncRNA and a uniform protein, redraw a positive or a repeat, stop at as many
// negatives as positives) and PyG 1.4.2 `torch_geometric.utils.negative_sampling` / `structured_negative_sampling` (Python
// `random.sample` + `isin` on the CPU).
//
// THE RULES (include/npi_gnn.h states them).  Wrapping uint64 throughout; mix64, G, C and mulhi(a, n) = the upper
// 64 bits of a * n are draw.h's (draw_word, draw_stream, draw_below), and so is the row search both kernels share (row_has):
//     Rule P:  base = mix64(mix64(key) + G);  candidate i = (mulhi(mix64(base + G (2i + 1)), n_src), mulhi(mix64(base + G (2i + 2)), n_dst))
//     Rule T:  base_k = mix64(mix64(mix64(key) + 2 G) ^ (k C));  try t of slot k = mulhi(mix64(base_k + G (t + 1)), n_dst)
// Both kernels answer "is (s, d) an edge" the same way: the two rowptr loads of row d of the by-target CSR with SORTED columns and a
// binary search of the row for s.  One lane per candidate / slot, grid-stride; a chain of dependent gathers, so the kernels keep
// few registers and no LDS and rely on occupancy.  npi_negative_distinct (below, over sort.h's radix sort) turns a window of
// candidates into the first M distinct valid ones.
#include "draw.h"
#include "sort.h"

namespace npi {

constexpr int NEG_BLOCK = 256;

__global__ void __launch_bounds__(NEG_BLOCK)
negative_candidates_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_dst, int64_t n_src,
                           uint64_t base, int64_t first, int64_t W, int no_loops, int32_t* __restrict__ cand_src,
                           int32_t* __restrict__ cand_dst) {
    const int64_t nt = (int64_t)gridDim.x * NEG_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * NEG_BLOCK + threadIdx.x; j < W; j += nt) {
        const uint64_t i = (uint64_t)(first + j);
        const int32_t s = (int32_t)draw_below(draw_word(base, 2 * i + 1), (uint64_t)n_src);
        const int32_t d = (int32_t)draw_below(draw_word(base, 2 * i + 2), (uint64_t)n_dst);
        const bool valid = !(no_loops && s == d) && !row_has(rowptr, col, d, s);
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
            const uint64_t base = draw_stream(key_base, (uint64_t)k);
            for (int t = 0; t < tries; ++t) {
                const int32_t d = (int32_t)draw_below(draw_word(base, (uint64_t)(t + 1)), (uint64_t)n_dst);
                if (!row_has(rowptr, col, d, (int32_t)s)) {
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

// ---- the first M distinct valid pairs of a window of negative candidates (npi_negative_distinct; the sort and the scan: sort.h) ---------
// Replaces the `if (a, b) in positives or (a, b) in negatives: continue` of src/generate_edgelist.py:108-139 for the "already drawn"
// half.  The LSD scheme of npi_sample_coalesce (sample.hip) -- by target, then by source, val = the candidate's position -- with one
// more key bit in the second sort that puts the invalid candidates ((-1, -1), or an id out of range) behind every valid one.  The
// sorts are stable over the position, so the head of a run of equal pairs is its EARLIEST occurrence: it alone sets keep[position].
__global__ void negative_keys_kernel(const int32_t* __restrict__ cand_dst, int64_t W, int64_t n_dst, uint32_t* __restrict__ keys,
                                     int32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W) return;
    const int32_t d = cand_dst[i];
    keys[i] = (d < 0 || d >= n_dst) ? 0u : (uint32_t)d;
    vals[i] = (int32_t)i;
}
__global__ void negative_rekey_kernel(const int32_t* __restrict__ cand_src, const int32_t* __restrict__ cand_dst,
                                      const int32_t* __restrict__ vals, int64_t W, int64_t n_src, int64_t n_dst, uint32_t invalid,
                                      uint32_t* __restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W) return;
    const int32_t i = vals[p], s = cand_src[i], d = cand_dst[i];
    keys[p] = (s < 0 || s >= n_src || d < 0 || d >= n_dst) ? invalid : (uint32_t)s;
}
// keep / kept (both ALL ZERO on entry): 1 at the position of every first occurrence of a valid pair
__global__ void negative_heads_kernel(const uint32_t* __restrict__ src_s, const int32_t* __restrict__ vals, const int32_t* __restrict__ cand_dst,
                                      int64_t W, uint32_t invalid, int32_t* __restrict__ keep, int32_t* __restrict__ kept) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W) return;
    const uint32_t s = src_s[p];
    if (s == invalid) return;
    const int32_t i = vals[p];
    if (p == 0 || src_s[p - 1] != s || cand_dst[vals[p - 1]] != cand_dst[i]) {
        keep[i] = 1;
        kept[i] = 1;
    }
}
// pos = the exclusive scan of keep in position order; info (ALL ZERO on entry) = (distinct valid pairs, candidates consumed by the M-th)
__global__ void negative_compact_kernel(const int32_t* __restrict__ cand_src, const int32_t* __restrict__ cand_dst,
                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ kept, int64_t W, int64_t M,
                                        int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst, int32_t* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W) return;
    const int64_t q = pos[i];                                    // q <= i
    const bool on = kept[i] != 0;
    if (i == W - 1) info[0] = (int32_t)(q + (on ? 1 : 0));
    if (!on || q >= M) return;
    out_src[q] = cand_src[i];
    out_dst[q] = cand_dst[i];
    if (q == M - 1) info[1] = (int32_t)(i + 1);
}

}  // namespace npi

using namespace npi;

extern "C" int npi_negative_candidates(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t n_src, int64_t key,
                                       int64_t first, int64_t W, int flags, int32_t* cand_src, int32_t* cand_dst, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(W), "npi_negative_candidates: bad window size");
    NPI_REQUIRE(id_bound_ok(n_src) && id_bound_ok(n_dst), "npi_negative_candidates: bad id bound");
    NPI_REQUIRE(first >= 0 && first <= (int64_t)1 << 40, "npi_negative_candidates: bad first candidate");
    NPI_REQUIRE((flags & ~1) == 0, "npi_negative_candidates: unknown flag");
    NPI_REQUIRE(rowptr && col, "npi_negative_candidates: null pointer");
    if (W == 0) return NPI_OK;
    NPI_REQUIRE(cand_src && cand_dst, "npi_negative_candidates: null pointer");
    const uint64_t base = draw_root(key, DRAW_RULE_P);
    negative_candidates_kernel<<<stride_grid(W, NEG_BLOCK, 2048), NEG_BLOCK, 0, stream>>>(rowptr, col, n_dst, n_src, base, first, W,
                                                                                          flags & 1, cand_src, cand_dst);
    return check_launch("npi_negative_candidates");
}

extern "C" int npi_negative_targets(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t n_src, const int64_t* src,
                                    int64_t K, int64_t key, int64_t tries, int64_t* out_dst, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(K), "npi_negative_targets: bad slot count");
    NPI_REQUIRE(id_bound_ok(n_src) && id_bound_ok(n_dst), "npi_negative_targets: bad id bound");
    NPI_REQUIRE(tries >= 1 && tries < NPI_INDEX_LIMIT, "npi_negative_targets: tries below 1");
    NPI_REQUIRE(rowptr && col, "npi_negative_targets: null pointer");
    if (K == 0) return NPI_OK;
    NPI_REQUIRE(src && out_dst, "npi_negative_targets: null pointer");
    if (status != nullptr) (void)hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    const uint64_t kb = draw_root(key, DRAW_RULE_T);
    negative_targets_kernel<<<stride_grid(K, NEG_BLOCK, 2048), NEG_BLOCK, 0, stream>>>(rowptr, col, n_dst, n_src, src, K, kb, (int)tries,
                                                                                       out_dst, status);
    return check_launch("npi_negative_targets");
}

extern "C" int64_t npi_negative_distinct_workspace_bytes(int64_t W) {
    if (!count_ok(W)) return -1;
    return PairSort::bytes(W);
}

extern "C" int npi_negative_distinct(const int32_t* cand_src, const int32_t* cand_dst, int64_t W, int64_t n_src, int64_t n_dst, int64_t M,
                                     int64_t* out_src, int64_t* out_dst, int32_t* info, void* workspace, int64_t workspace_bytes,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(W) && M >= 0, "npi_negative_distinct: bad size");
    NPI_REQUIRE(id_bound_ok(n_src) && id_bound_ok(n_dst), "npi_negative_distinct: bad id bound");
    NPI_REQUIRE(info, "npi_negative_distinct: null pointer");
    if (W == 0) return NPI_OK;
    NPI_REQUIRE(cand_src && cand_dst && workspace && (M == 0 || (out_src && out_dst)), "npi_negative_distinct: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace & 15) == 0, "npi_negative_distinct: workspace must be 16-byte aligned");
    if (workspace_short("npi_negative_distinct", workspace_bytes, PairSort::bytes(W))) return NPI_ERR_ARG;
    PairSort ps;
    (void)ps.carve(workspace, workspace_bytes, W);           // (the length was checked above)
    const int sbits = key_bits(n_src);
    const uint32_t invalid = (uint32_t)1 << sbits;         // sbits <= 31: one bit above every source id
    const unsigned wb = (unsigned)ceil_div(W, 256);
    negative_keys_kernel<<<wb, 256, 0, stream>>>(cand_dst, W, n_dst, ps.keys_a, ps.vals_a);
    ps.sort(key_bits(n_dst), stream);
    negative_rekey_kernel<<<wb, 256, 0, stream>>>(cand_src, cand_dst, ps.vals_a, W, n_src, n_dst, invalid, ps.keys_a);
    ps.sort(sbits + 1, stream);
    // the sort's free buffers (PairSort): keep (scanned in place into the output positions), a copy of it and the scan's tile sums
    int32_t* keep = (int32_t*)ps.keys_b;
    int32_t* kept = ps.vals_b;
    (void)hipMemsetAsync(keep, 0, (size_t)W * sizeof(int32_t), stream);
    (void)hipMemsetAsync(kept, 0, (size_t)W * sizeof(int32_t), stream);
    (void)hipMemsetAsync(info, 0, 2 * sizeof(int32_t), stream);
    negative_heads_kernel<<<wb, 256, 0, stream>>>(ps.keys_a, ps.vals_a, cand_dst, W, invalid, keep, kept);
    exclusive_scan_i32(keep, W, ps.counts, stream);
    negative_compact_kernel<<<wb, 256, 0, stream>>>(cand_src, cand_dst, keep, kept, W, M, out_src, out_dst, info);
    return check_launch("npi_negative_distinct");
}
