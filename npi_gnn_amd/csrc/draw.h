// The counter-based generator behind every seeded result of the index kernels, stated ONCE (include/npi_gnn.h states the rules for a
// caller).  Wrapping uint64 throughout; no state, no float.  A rule is
//     root      = draw_root(key, rule)        mix64(mix64(key) + rule G): one root per (key, rule), so two rules never share a word
//     a stream  = draw_stream(root, k)        mix64(root ^ (k C)): one stream per slot / walk / target
//     a word    = draw_word(base, i)          mix64(base + G i), i = 1, 2, ...: the i-th output of splitmix64 started at base
//     an id     = draw_below(word, n)         the upper 64 bits of word * n: uniform over [0, n) without a division
// Everything here is forced inline, so the header has no translation unit of its own and its clients need no relocatable device code.
#pragma once
#include "npi_common.h"

namespace npi {

constexpr uint64_t DRAW_G = 0x9E3779B97F4A7C15ull;
constexpr uint64_t DRAW_C = 0xD6E8FEB86659FD93ull;

// The rules apart: the multiplier of G that draw_root adds.  The next feature takes the next number.
enum DrawRule : uint64_t {
    DRAW_RULE_P = 1,                                       // Rule P: candidate pairs                 (npi_negative_candidates)
    DRAW_RULE_T = 2,                                       // Rule T: corrupted targets, per slot     (npi_negative_targets)
    DRAW_RULE_W = 3,                                       // Rule W: walks, per walk                 (npi_random_walk)
    DRAW_RULE_W_NEG = 4,                                   // Rule W's negatives of the pair list     (npi_walk_pairs)
    DRAW_RULE_S = 5,                                       // Rule S: the order of a split            (npi_split_permute)
    DRAW_RULE_D = 6,                                       // Rule D: the attention-dropout mask      (npi_gat_*_dropout)
    DRAW_RULE_N = 7,                                       // Rule N: the standard normal, gauss.h      (npi_gauss_*)
    DRAW_RULE_E = 8,                                       // Rule E: DropEdge, per column / per pair (npi_csr_drop_side, npi_drop_edge_*)
};

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t draw_word(uint64_t base, uint64_t i) { return mix64(base + DRAW_G * i); }
__host__ __device__ __forceinline__ uint64_t draw_stream(uint64_t root, uint64_t k) { return mix64(root ^ (k * DRAW_C)); }
inline uint64_t draw_root(int64_t key, DrawRule rule) { return mix64(mix64((uint64_t)key) + (uint64_t)rule * DRAW_G); }
// (n is an id bound or a row length, below 2^31 - 1 at every caller: the result fits 32 bits, signed or not)
__device__ __forceinline__ uint32_t draw_below(uint64_t word, uint64_t n) { return (uint32_t)__umul64hi(word, n); }

// Rule D, the attention-dropout mask of GATConv: a pure function of (key, edge, head), the same on the by-target and the by-source
// side because both carry the entry's eid.  root = draw_root(key, DRAW_RULE_D); the slot of an entry is its eid (a column of
// edge_index, 0 <= eid < 2^31) or, for the self loop the CSR build appends at node i (eid < 0, rowidx == col == i), 2^32 + i;
// head h of slot k is DROPPED iff draw_word(draw_stream(root, k), h + 1) < threshold, threshold = floor(p 2^64) (the host rounds);
// a kept weight is scaled by float32(1 / (1 - p)).
__host__ __device__ __forceinline__ uint64_t drop_slot(int32_t eid, int32_t col) {
    return eid >= 0 ? (uint64_t)(uint32_t)eid : (1ull << 32) + (uint64_t)(uint32_t)col;
}
__host__ __device__ __forceinline__ bool drop_kept(uint64_t stream, int h, uint64_t threshold) {
    return draw_word(stream, (uint64_t)h + 1) >= threshold;
}
// bit h of the result: head h of the entry is kept (NH <= 32 heads)
template <int NH>
__host__ __device__ __forceinline__ int drop_keep_bits(uint64_t root, uint64_t threshold, int32_t eid, int32_t col) {
    const uint64_t stream = draw_stream(root, drop_slot(eid, col));
    int bits = 0;
#pragma unroll
    for (int h = 0; h < NH; ++h) bits |= drop_kept(stream, h, threshold) ? (1 << h) : 0;
    return bits;
}

// Rule E, DropEdge: a pure function of (key, tick, column) -- or, undirected, of (key, tick, the column's unordered pair of ends).
// root_t = draw_word(draw_root(key, DRAW_RULE_E), tick + 1), the tick word read as Rule N reads it.  Directed: slot e, word 1;
// undirected: slot 2^32 min(u, v) + max(u, v) (wrapping uint64 of the int64 ends), word 2.  DROPPED iff word < threshold.
__host__ __device__ __forceinline__ uint64_t edge_pair_slot(int64_t u, int64_t v) {
    const int64_t lo = u < v ? u : v, hi = u < v ? v : u;
    return ((uint64_t)lo << 32) + (uint64_t)hi;
}
__host__ __device__ __forceinline__ bool edge_dropped(uint64_t root_t, bool undirected, int64_t e, int64_t u, int64_t v, uint64_t threshold) {
    const uint64_t k = undirected ? edge_pair_slot(u, v) : (uint64_t)e;
    return draw_word(draw_stream(root_t, k), undirected ? 2 : 1) < threshold;
}

// is x a column of row `row`?  Rows ascend; empty rows, rows of one entry and rows with repeated columns all occur.
__device__ __forceinline__ bool row_has(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t row, int32_t x) {
    int lo = rowptr[row];
    const int end = rowptr[row + 1];
    int hi = end;
    while (lo < hi) {                                      // first position with col >= x
        const int mid = lo + ((hi - lo) >> 1);
        if (col[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < end && col[lo] == x;
}

// enough workgroups for 8 wavefronts on every SIMD of 256 CUs (cap 2048 at 256 threads); more work than the cap strides
inline unsigned stride_grid(int64_t work, int block, int64_t cap) {
    const int64_t g = ceil_div(work, block);
    return (unsigned)(g < cap ? g : cap);
}

}  // namespace npi
