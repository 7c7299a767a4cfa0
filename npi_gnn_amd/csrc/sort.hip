// Stable LSD radix sort of (key, val) pairs (8-bit digits) and the exclusive scan of an int32 array: the kernels behind sort.h.
// The sort is stable, so pairs with equal keys keep the order they were written in: the CSR build's rows keep their edge_index
// order, and a client that sorts twice (second key first) gets a lexicographic order with ties in entry order.
#include "sort.h"

namespace npi {

constexpr int SORT_THREADS = 256;
constexpr int SORT_WAVES = SORT_THREADS / WAVE;
constexpr int SORT_ITEMS = 16;                       // keys per lane
constexpr int SORT_WAVE_TILE = WAVE * SORT_ITEMS;    // 1024 keys per wave, striped: key j*64+lane
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS; // 4096 keys per workgroup
constexpr int RADIX = 256;

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
static_assert(SCAN_THREADS == SORT_THREADS && SORT_THREADS == 256, "one thread per radix digit");

__global__ void __launch_bounds__(SORT_THREADS)
radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift, int nblocks,
                  int32_t* __restrict__ counts) {
    __shared__ int hist[RADIX];
    hist[threadIdx.x] = 0;
    __syncthreads();
    int64_t base = (int64_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        int64_t i = base + j * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&hist[(keys[i] >> shift) & (RADIX - 1)], 1);
    }
    __syncthreads();
    counts[(int64_t)threadIdx.x * nblocks + blockIdx.x] = hist[threadIdx.x];   // digit-major
}

// ---- exclusive scan of an int32 array (three launches) -------------------------------------
__global__ void __launch_bounds__(SCAN_THREADS)
scan_tiles_kernel(int32_t* __restrict__ data, int64_t n, int32_t* __restrict__ tile_sums) {
    __shared__ int lds[SCAN_THREADS];
    int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = (base + j < n) ? data[base + j] : 0;
        s += v[j];
    }
    int total;
    int excl = block_exclusive_scan<SCAN_THREADS>(s, lds, &total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (base + j < n) data[base + j] = excl;
        excl += v[j];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_THREADS)
scan_sums_kernel(int32_t* __restrict__ sums, int64_t n) {   // one workgroup
    __shared__ int lds[SCAN_THREADS];
    int carry = 0;
    for (int64_t base = 0; base < n; base += SCAN_THREADS) {
        int64_t i = base + threadIdx.x;
        int v = (i < n) ? sums[i] : 0;
        int total;
        int excl = block_exclusive_scan<SCAN_THREADS>(v, lds, &total);
        if (i < n) sums[i] = carry + excl;
        carry += total;
    }
}

__global__ void __launch_bounds__(SCAN_THREADS)
scan_add_kernel(int32_t* __restrict__ data, int64_t n, const int32_t* __restrict__ tile_sums) {
    int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int add = tile_sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (base + j < n) data[base + j] += add;
}

// ---- stable scatter of one radix pass ----------------------------------------------------------
// SCANNED: `offsets` is the exclusive scan of the digit-major tile histograms (three scan launches before this one).
// !SCANNED (at most SMALL_SORT_TILES tiles -- the reference's 200-subgraph batches, launch-bound): `offsets` holds the
// raw histograms and every workgroup derives its own start offsets from them, two launches per pass instead of five.
constexpr int SMALL_SORT_TILES = 64;
template <bool SCANNED>
__global__ void __launch_bounds__(SORT_THREADS)
radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in,
                     uint32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out,
                     int64_t n, int shift, int nblocks, const int32_t* __restrict__ offsets) {
    __shared__ int wcnt[SORT_WAVES][RADIX];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < SORT_WAVES * RADIX; i += SORT_THREADS) (&wcnt[0][0])[i] = 0;
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * SORT_TILE + (int64_t)wave * SORT_WAVE_TILE;
    uint32_t key[SORT_ITEMS];
    int32_t val[SORT_ITEMS];
    int rank[SORT_ITEMS];
    const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        int64_t i = base + j * WAVE + lane;
        bool valid = i < n;
        key[j] = valid ? keys_in[i] : 0xFFFFFFFFu;
        val[j] = valid ? vals_in[i] : 0;
        // tail lanes rank as digit 255 of the last tile: they sort behind everything and are not written
        int digit = valid ? (int)((key[j] >> shift) & (RADIX - 1)) : (RADIX - 1);
        uint64_t same = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            bool bit = (digit >> b) & 1;
            uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        int before = __popcll(same & lt_mask);
        int prev = wcnt[wave][digit];
        __builtin_amdgcn_wave_barrier();
        if (before == 0) wcnt[wave][digit] = prev + __popcll(same);
        __builtin_amdgcn_wave_barrier();
        rank[j] = prev + before;
    }
    __syncthreads();
    {   // thread d owns digit d: turn per-wave counts into global start offsets
        int d = threadIdx.x;
        int off;
        if (SCANNED) {
            off = offsets[(int64_t)d * nblocks + blockIdx.x];
        } else {
            __shared__ int scan_s[SCAN_THREADS];
            const int32_t* __restrict__ h = offsets + (int64_t)d * nblocks;
            int total = 0, before = 0;
            for (int t = 0; t < nblocks; ++t) {
                const int c = h[t];
                before += (t < (int)blockIdx.x) ? c : 0;
                total += c;
            }
            int all;
            off = block_exclusive_scan<SCAN_THREADS>(total, scan_s, &all) + before;   // keys with a smaller digit + same digit in earlier tiles
        }
#pragma unroll
        for (int w = 0; w < SORT_WAVES; ++w) {
            int c = wcnt[w][d];
            wcnt[w][d] = off;
            off += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        int64_t i = base + j * WAVE + lane;
        if (i < n) {
            int digit = (int)((key[j] >> shift) & (RADIX - 1));
            int pos = wcnt[wave][digit] + rank[j];
            keys_out[pos] = key[j];
            vals_out[pos] = val[j];
        }
    }
}

int key_bits(int64_t n) {
    int bits = 1;
    while (((int64_t)1 << bits) < n) ++bits;
    return bits;
}

static int64_t sort_tiles(int64_t n) { return ceil_div(n > 0 ? n : 1, SORT_TILE); }

int64_t PairSort::bytes(int64_t n) {
    const int64_t words = n > 0 ? n : 1, counts_len = sort_tiles(n) * RADIX;
    return 4 * align_up(words * 4, 256) + align_up(counts_len * 4, 256) + align_up(ceil_div(counts_len, SCAN_TILE) * 4, 256);
}

bool PairSort::carve(void* workspace, int64_t ws_bytes, int64_t n_) {
    if (ws_bytes < bytes(n_)) return false;
    n = n_;
    char* ws = (char*)workspace;
    const int64_t pitch = align_up((n > 0 ? n : 1) * 4, 256);
    keys_a = (uint32_t*)(ws + 0 * pitch);
    keys_b = (uint32_t*)(ws + 1 * pitch);
    vals_a = (int32_t*)(ws + 2 * pitch);
    vals_b = (int32_t*)(ws + 3 * pitch);
    counts = (int32_t*)(ws + 4 * pitch);
    tiles = (int32_t*)(ws + 4 * pitch + align_up(sort_tiles(n) * RADIX * 4, 256));
    return true;
}

void exclusive_scan_i32(int32_t* data, int64_t n, int32_t* tile_sums, hipStream_t stream) {
    if (n <= 0) return;
    const int64_t ntiles = ceil_div(n, SCAN_TILE);
    scan_tiles_kernel<<<(unsigned)ntiles, SCAN_THREADS, 0, stream>>>(data, n, tile_sums);
    scan_sums_kernel<<<1, SCAN_THREADS, 0, stream>>>(tile_sums, ntiles);
    scan_add_kernel<<<(unsigned)ntiles, SCAN_THREADS, 0, stream>>>(data, n, tile_sums);
}

void PairSort::sort(int bits, hipStream_t stream) {
    const int nblocks = (int)sort_tiles(n);
    const int passes = (bits + 7) / 8;
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p;
        radix_hist_kernel<<<(unsigned)nblocks, SORT_THREADS, 0, stream>>>(keys_a, n, shift, nblocks, counts);
        if (nblocks <= SMALL_SORT_TILES) {
            radix_scatter_kernel<false><<<(unsigned)nblocks, SORT_THREADS, 0, stream>>>(keys_a, vals_a, keys_b, vals_b, n, shift, nblocks, counts);
        } else {
            exclusive_scan_i32(counts, (int64_t)nblocks * RADIX, tiles, stream);
            radix_scatter_kernel<true><<<(unsigned)nblocks, SORT_THREADS, 0, stream>>>(keys_a, vals_a, keys_b, vals_b, n, shift, nblocks, counts);
        }
        uint32_t* tk = keys_a; keys_a = keys_b; keys_b = tk;
        int32_t* tv = vals_a; vals_a = vals_b; vals_b = tv;
    }
}

}  // namespace npi
