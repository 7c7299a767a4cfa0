// What one lane carries of a row in the per-entry dot products (edge_dot.hip, pair_score.hip): a 16-byte piece when the rows allow
// it (F % 4 == 0, 16-byte aligned bases and pitches: rows16), one float otherwise.
#pragma once
#include "npi_common.h"

namespace npi {

template <bool VEC> struct Lanes;
template <> struct Lanes<true> {
    using T = float4;
    static constexpr int W = 4;
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ float dot(const T& u, const T& v, float acc) {
        return fmaf(u.w, v.w, fmaf(u.z, v.z, fmaf(u.y, v.y, fmaf(u.x, v.x, acc))));
    }
};
template <> struct Lanes<false> {
    using T = float;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T load(const float* p) { return *p; }
    static __device__ __forceinline__ float dot(const T& u, const T& v, float acc) { return fmaf(u, v, acc); }
};

// the eight partial dot products p[0..8) of a group of eight entries, reduce-SCATTERED over the wave: every xor step halves the
// number of entries a lane still carries (10 cross-lane steps for 8 entries instead of 48); afterwards the eight lanes
// 8 e .. 8 e + 7 all hold the sum of entry e (e = bits 5, 4, 3 of the lane read as 4, 2, 1: group_of_lane)
__device__ __forceinline__ int group_of_lane(int lane) { return ((lane & 32) ? 4 : 0) + ((lane & 16) ? 2 : 0) + ((lane & 8) ? 1 : 0); }
__device__ __forceinline__ float reduce_scatter8(const float (&p)[8], int lane) {
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    float w4[4], w2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = (b5 ? p[k + 4] : p[k]) + __shfl_xor(b5 ? p[k] : p[k + 4], 32, WAVE);
#pragma unroll
    for (int k = 0; k < 2; ++k) w2[k] = (b4 ? w4[k + 2] : w4[k]) + __shfl_xor(b4 ? w4[k] : w4[k + 2], 16, WAVE);
    float y = (b3 ? w2[1] : w2[0]) + __shfl_xor(b3 ? w2[0] : w2[1], 8, WAVE);
    y += __shfl_xor(y, 4, WAVE);
    y += __shfl_xor(y, 2, WAVE);
    y += __shfl_xor(y, 1, WAVE);
    return y;
}

inline bool rows16(const void* p, int64_t ld, int64_t F) { return F % 4 == 0 && ld % 4 == 0 && ((uintptr_t)p % 16) == 0; }

}  // namespace npi
