// The device sort and scans the index builders share (sort.hip holds the kernels: without relocatable device code a kernel is
// launched from the translation unit that defines it, so the clients reach them through the host functions below).
//
//   PairSort             stable LSD radix sort of n (uint32 key, int32 val) pairs inside a caller's workspace
//   exclusive_scan_i32   exclusive scan of an int32 array of any length, in place (three launches)
//   block_exclusive_scan exclusive scan over the threads of ONE workgroup (a device helper for a client's own kernels)
//   pool_vec             the load width of the row kernels that walk graphs by segment starts (pool.hip, readout.hip)
#pragma once
#include <initializer_list>
#include "npi_common.h"

namespace npi {

// bits that hold every id in [0, n); at least 1
int key_bits(int64_t n);

// floats per load of the row kernels of pool.hip and readout.hip: the widest of {4, 2, 1} that divides F and every leading dimension
// and keeps every base pointer aligned
inline int pool_vec(int64_t F, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs) {
    for (int v = 4; v > 1; v >>= 1) {
        bool ok = F % v == 0;
        for (int64_t l : lds) ok = ok && l % v == 0;
        for (const void* p : ptrs) ok = ok && ((uintptr_t)p % (v * sizeof(float))) == 0;
        if (ok) return v;
    }
    return 1;
}

// Every client: carve (a short workspace is the CALLER's error: it words the text and picks the status), write keys_a / vals_a with a
// kernel of its own, sort; then -- for a second key -- rewrite keys_a from vals_a and sort again.
struct PairSort {
    // The sorted pairs are in (keys_a, vals_a) after every sort (the pointers swap pass by pass).  Between sorts and after the last
    // one the other pair (keys_b, vals_b) is free: n words each, for whatever the client derives from the sorted stream (run heads,
    // sorted second keys, keep flags).  `counts` (the tile histograms: 256 words per 4,096 pairs = n / 16 words at least) is free
    // then as well and is large enough for the tile sums of exclusive_scan_i32 over n words (one word per 2,048).
    uint32_t *keys_a, *keys_b;
    int32_t *vals_a, *vals_b, *counts, *tiles;
    int64_t n;

    static int64_t bytes(int64_t n);                      // workspace for n pairs (n = 0 as n = 1); what the npi_*_workspace_bytes queries return
    bool carve(void* ws, int64_t ws_bytes, int64_t n);    // false: fewer than bytes(n)
    void sort(int bits, hipStream_t stream);              // on the low `bits` bits of the keys, 8 bits a pass
};

// data[i] = data[0] + ... + data[i - 1]; tile_sums: scratch of ceil(n / 2048) words.  n <= 0: nothing is launched
void exclusive_scan_i32(int32_t* data, int64_t n, int32_t* tile_sums, hipStream_t stream);

// v of every thread of a THREADS-wide workgroup -> the sum of the v of the threads in front of it; *total = the sum over all of them.
// Every thread calls it; lds[THREADS] may be used again right after the return.
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds /*[THREADS]*/, T* total) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {          // Hillis-Steele inclusive scan
        T t = (threadIdx.x >= off) ? lds[threadIdx.x - off] : 0;
        __syncthreads();
        lds[threadIdx.x] += t;
        __syncthreads();
    }
    T incl = lds[threadIdx.x];
    *total = lds[THREADS - 1];
    __syncthreads();
    return incl - v;
}

}  // namespace npi
