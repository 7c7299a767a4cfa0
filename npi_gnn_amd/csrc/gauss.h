// Rule N, the seeded standard normal (include/npi_gnn.h states it for a caller): eps is a pure function of
// (key, tick, table, row, column).  The integer half is draw.h's generator and exact; the float half starts here.
//     root   = draw_root(key, DRAW_RULE_N)                          on the host, once per call
//     root_t = draw_word(root, tick + 1)                            tick: a device int64 word the kernel reads, 0 when there is none
//     stream = draw_stream(root_t, table 2^32 + row)                one stream per row of a table
//     w_p    = draw_word(stream, p + 1)                             one word per COLUMN PAIR p = column >> 1
//     u1 = float((w_p >> 40) + 1) 2^-24 in (0, 1];  u2 = float((w_p >> 16) & 0xFFFFFF) 2^-24 in [0, 1)      both exact
//     theta = float32(2 pi) u2 (ONE f32 multiply);  r = sqrt(-2 ln u1);  eps = r cos(theta) (even column), r sin(theta) (odd)
// logf / sincosf / sqrtf are the full-precision functions: |eps| <= sqrt(48 ln 2) = 5.77, and the tests' tolerance is theirs.
#pragma once
#include "draw.h"

namespace npi {

// one lane owns four columns of a row: two words.  A partial of the KL sum covers GAUSS_TILE_QUADS such groups in row-major order
// of (row, group): a function of N and F alone, so the sum does not depend on the grid, the pitch or the lane width.
constexpr int GAUSS_THREADS = 256;
constexpr int GAUSS_QUADS_PER_THREAD = NPI_GAUSS_TILE / 4 / GAUSS_THREADS;
constexpr int GAUSS_TILE_QUADS = NPI_GAUSS_TILE / 4;
static_assert(GAUSS_QUADS_PER_THREAD * GAUSS_THREADS * 4 == NPI_GAUSS_TILE, "a tile is a whole number of passes of the workgroup");

__device__ __forceinline__ uint64_t gauss_root_t(uint64_t root, const int64_t* __restrict__ tick) {
    return draw_word(root, (uint64_t)(tick ? tick[0] : 0) + 1);
}
__device__ __forceinline__ uint64_t gauss_stream(uint64_t root_t, int table, int row) {
    return draw_stream(root_t, ((uint64_t)table << 32) + (uint64_t)(uint32_t)row);
}
// the two values of column pair p: columns 2 p and 2 p + 1
__device__ __forceinline__ void gauss_pair(uint64_t stream, int p, float& even, float& odd) {
    const uint64_t w = draw_word(stream, (uint64_t)p + 1);
    const float u1 = (float)((uint32_t)(w >> 40) + 1u) * 0x1p-24f;
    const float u2 = (float)((uint32_t)(w >> 16) & 0xFFFFFFu) * 0x1p-24f;
    const float theta = __uint_as_float(0x40C90FDBu) * u2;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(theta, &s, &c);
    even = r * c;
    odd = r * s;
}

}  // namespace npi
