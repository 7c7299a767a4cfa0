// The descending-orderable key of an f32 score (include/npi_gnn.h: RULE R 1, RULE K 3), shared by the ranking metrics (rank.hip) and
// the top-k link selection (topk.hip).
#pragma once
#include "npi_common.h"

namespace npi {

// score bits -> key.  s = score + 0.0f, done on the bits (-0.0 is the one value the addition changes), then the complement of
// pool.hip's ascending-orderable transform: ascending key == descending score.  A NaN passes through as it is.
__device__ __forceinline__ uint32_t rank_key(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    const uint32_t u = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ~u;
}
__device__ __forceinline__ float rank_score(uint32_t key) {
    const uint32_t u = ~key;
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

}  // namespace npi
