// Neighbour sampling on the device: the producer of the (x_src, None) / size= / res_n_id arguments of the bipartite SAGEConv and
// GATConv.  Replaces PyG 1.4.2 `torch_geometric.data.NeighborSampler.__produce_bipartite_data_flow__`, i.e. the CPU calls
// `torch_cluster.neighbor_sampler(start, cumdeg, size)` + `torch.unique` + the `tmp[n_id] = arange` relabelling, one hop per call.
//
// THE RULE (include/npi_gnn.h restates it; DESIGN.md "Neighbour sampling").  Over the by-target CSR of the edge list as it is, target
// v has the row [rowptr[v], rowptr[v + 1]) of d entries; position p in [0, d) gets the 64-bit key (h32(seed, hop, v, p) << 32) | p,
//     base      = draw_stream(mix64(seed + G (hop + 1)), v)        (mix64, G, draw_stream, draw_word: draw.h; uint64, wrapping)
//     h32       = draw_word(base, p + 1) >> 32
// (splitmix64: a stream per (seed, hop, v), its p-th output, upper half) and the sample is the k entries with the smallest keys,
// emitted in ascending p.  Keys are distinct (p is part of the key), so the sample is a pure function of (seed, hop, v, d, k): no
// launch geometry, batch composition or timing enters.  Everything below only finds T = the k-th smallest key of a row and then
// emits, in position order, the entries with key <= T.
//
// Rows of at most 64 entries: one wavefront, one key per lane, rank by 64 broadcasts.  Longer rows: the whole workgroup.  It keeps
// the keys it has to look at in LDS -- all of them for a row of up to SAMPLE_CAP entries; for a longer row only those whose h32
// lies under a threshold chosen so that about k + 8 sqrt(k) + 32 survive (ANY superset of the k smallest keys that is a lower set in
// h32 gives the same answer; fewer than k survivors: the threshold is doubled and the row hashed again) -- and finds T by a radix
// select over the 64-bit keys, 8 bits a pass, stopping at the first pass after which every remaining key is taken.  A budget too
// large for LDS (a fraction of a hub) runs the same select straight over the positions, hashing once per pass.  Entries (col, eid)
// are read for the winners only.  Integer LDS counters, no float anywhere except the fraction's ceil (in double, as the host's).
#include "draw.h"
#include "sort.h"

namespace npi {

constexpr int SAMPLE_BLOCK = 256;                 // 4 wavefronts: 4 light targets per workgroup, or the whole group on a heavy one
constexpr int SAMPLE_WAVES = SAMPLE_BLOCK / WAVE;
constexpr int SAMPLE_CAP = 2048;                  // keys kept in LDS (16 KiB)
static_assert(SAMPLE_BLOCK == 256, "the radix select keeps one histogram bin per thread");
constexpr int RELABEL_BLOCK = 256;
constexpr int RELABEL_CHUNK = 4 * RELABEL_BLOCK;  // scratch entries per workgroup of the relabelling scans
constexpr int STATUS_BAD_TARGET = NPI_STATUS_BAD_TARGET_ID;
constexpr int STATUS_BAD_OFFSETS = NPI_STATUS_BAD_SAMPLE_SIZES;

// the hop enters the UNMIXED seed (the rule is older than draw_root and part of the ABI as it is)
__host__ __device__ __forceinline__ uint64_t row_base(int64_t seed, int64_t hop, int64_t v) {
    return draw_stream(mix64((uint64_t)seed + DRAW_G * (uint64_t)(hop + 1)), (uint64_t)v);
}
__host__ __device__ __forceinline__ uint64_t key_of(uint64_t base, uint32_t p) {
    const uint64_t h = draw_word(base, (uint64_t)p + 1) >> 32;
    return (h << 32) | p;
}

// budget of a row of d entries: min(d, budget) for budget > 0, else min(d, ceil(frac * d)) in double (the host restates it so)
__device__ __forceinline__ int budget_of(int d, int64_t budget, float frac) {
    if (d <= 0) return 0;
    if (budget > 0) return (int)(budget < (int64_t)d ? budget : (int64_t)d);
    const double c = ceil((double)frac * (double)d);
    return c < (double)d ? (int)c : d;
}

__global__ void __launch_bounds__(256)
sample_counts_kernel(const int32_t* __restrict__ rowptr, int64_t N, const int64_t* __restrict__ targets, int64_t n, int64_t budget,
                     float frac, int32_t* __restrict__ cnt, int32_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t v = targets[t];
    if (v < 0 || v >= N) {                                   // dropped and reported, never dereferenced
        cnt[t] = 0;
        if (status != nullptr) atomicOr(status, STATUS_BAD_TARGET);
        return;
    }
    cnt[t] = budget_of(rowptr[v + 1] - rowptr[v], budget, frac);
}

struct SampleSmem {
    unsigned long long keys[SAMPLE_CAP];
    int hist[256];
    int wsum[SAMPLE_WAVES];
    int pick[3];
};

// position of this thread's flag among the workgroup's flags (thread order) and their number; two barriers
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
    const uint64_t m = __ballot(flag);
    const int lane = lane_id(), w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < SAMPLE_WAVES; ++i) {
        const int c = wsum[i];
        base += i < w ? c : 0;
        total += c;
    }
    __syncthreads();
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// T = the k-th smallest (k >= 1) of n distinct keys: those in sm.keys[0 .. n) (IN_LDS) or key_of(base, p) for p < n.  All threads of
// the workgroup call it with the same arguments and get the same value.
template <bool IN_LDS>
__device__ unsigned long long kth_smallest_key(SampleSmem& sm, uint64_t base, int n, int k) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    unsigned long long prefix = 0;
    int r = k;                                             // rank still wanted among the keys that match `prefix`
    for (int shift = 56; shift >= 0; shift -= 8) {
        sm.hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += SAMPLE_BLOCK) {
            const unsigned long long key = IN_LDS ? sm.keys[i] : key_of(base, (uint32_t)i);
            if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&sm.hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        const int x = sm.hist[tid];
        int incl = x;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == WAVE - 1) sm.wsum[w] = incl;
        __syncthreads();
        for (int i = 0; i < w; ++i) incl += sm.wsum[i];
        const int excl = incl - x;
        if (excl < r && r <= incl) {                       // exactly one bin holds the r-th key
            sm.pick[0] = tid;
            sm.pick[1] = excl;
            sm.pick[2] = x;
        }
        __syncthreads();
        const int bin = sm.pick[0], below = sm.pick[1], in_bin = sm.pick[2];
        __syncthreads();
        prefix = (prefix << 8) | (unsigned long long)bin;
        r -= below;
        if (r == in_bin)                                   // every key under this prefix is taken: the low bits no longer matter
            return shift == 0 ? prefix : ((prefix << shift) | ((1ull << shift) - 1ull));
    }
    return prefix;
}

// the workgroup emits, in position order, the entries of the row with key <= T
template <bool IN_LDS>
__device__ void emit_selected(SampleSmem& sm, uint64_t base, int n, unsigned long long T, int k, int row_start, int64_t out0, int t,
                              const int32_t* __restrict__ col, const int32_t* __restrict__ eid, int32_t* __restrict__ out_src,
                              int32_t* __restrict__ out_eid, int32_t* __restrict__ out_tgt) {
    int done = 0;
    for (int b = 0; b < n; b += SAMPLE_BLOCK) {
        const int i = b + (int)threadIdx.x;
        const unsigned long long key = i < n ? (IN_LDS ? sm.keys[i] : key_of(base, (uint32_t)i)) : ~0ull;
        const bool take = i < n && key <= T;
        int total;
        const int r = done + block_rank(take, sm.wsum, total);
        if (take && r < k) {                               // (r < k always: exactly k keys are <= T)
            const int e = row_start + (int)(key & 0xffffffffull);
            out_src[out0 + r] = col[e];
            out_eid[out0 + r] = eid[e];
            out_tgt[out0 + r] = t;
        }
        done += total;
    }
}

__device__ void sample_heavy_row(SampleSmem& sm, uint64_t base, int d, int k, int row_start, int64_t out0, int t,
                                 const int32_t* __restrict__ col, const int32_t* __restrict__ eid, int32_t* __restrict__ out_src,
                                 int32_t* __restrict__ out_eid, int32_t* __restrict__ out_tgt) {
    const int tid = threadIdx.x;
    if (k >= d) {                                          // every entry is taken
        for (int p = tid; p < d; p += SAMPLE_BLOCK) {
            out_src[out0 + p] = col[row_start + p];
            out_eid[out0 + p] = eid[row_start + p];
            out_tgt[out0 + p] = t;
        }
        return;
    }
    // how many keys to keep: all of a row that fits, else about k + 8 sqrt(k) + 32 (8 standard deviations of the binomial count above
    // k); a budget whose candidates would not fit runs the select over the positions themselves
    int n_lds = -1;
    if (d <= SAMPLE_CAP || (int64_t)k * 5 / 4 + 320 <= SAMPLE_CAP) {
        uint64_t want = d <= SAMPLE_CAP ? (uint64_t)d : (uint64_t)k + 8 * (uint64_t)sqrtf((float)k) + 32;
        for (int attempt = 0; attempt < 3 && n_lds < 0; ++attempt, want *= 2) {
            const uint64_t q = want >= (uint64_t)d ? 0xffffffffull : (want << 32) / (uint64_t)d;
            const uint32_t thr = q > 0xffffffffull ? 0xffffffffu : (uint32_t)q;
            int c = 0;
            for (int b = 0; b < d; b += SAMPLE_BLOCK) {
                const int p = b + tid;
                const unsigned long long key = p < d ? key_of(base, (uint32_t)p) : ~0ull;
                const bool keep = p < d && (uint32_t)(key >> 32) <= thr;
                int total;
                const int r = c + block_rank(keep, sm.wsum, total);
                if (keep && r < SAMPLE_CAP) sm.keys[r] = key;
                c += total;
            }
            __syncthreads();
            if (c > SAMPLE_CAP) break;                     // does not fit: the select over the positions is always right
            if (c >= k) n_lds = c;                         // the k smallest keys are all among the kept ones
        }
    }
    if (n_lds >= 0) {
        const unsigned long long T = kth_smallest_key<true>(sm, base, n_lds, k);
        emit_selected<true>(sm, base, n_lds, T, k, row_start, out0, t, col, eid, out_src, out_eid, out_tgt);
    } else {
        const unsigned long long T = kth_smallest_key<false>(sm, base, d, k);
        emit_selected<false>(sm, base, d, T, k, row_start, out0, t, col, eid, out_src, out_eid, out_tgt);
    }
}

// offsets[n + 1]: exclusive sums of npi_sample_counts' output; n_out: what the caller sized the outputs with
__global__ void __launch_bounds__(SAMPLE_BLOCK)
sample_select_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid, int64_t N,
                     const int64_t* __restrict__ targets, int64_t n, const int64_t* __restrict__ offsets, int64_t seed, int64_t hop,
                     int32_t* __restrict__ out_src, int32_t* __restrict__ out_eid, int32_t* __restrict__ out_tgt, int64_t n_out,
                     int32_t* __restrict__ status) {
    __shared__ SampleSmem sm;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * SAMPLE_WAVES;
    for (int j = 0; j < SAMPLE_WAVES; ++j) {
        // the four targets of this workgroup in turn; everything below up to the heavy-row call is the same in every thread
        const int64_t t = t0 + j;
        if (t >= n) break;
        const int64_t v = targets[t];
        if (v < 0 || v >= N) continue;                     // counted as 0 entries and reported by npi_sample_counts
        const int row_start = rowptr[v];
        const int d = rowptr[v + 1] - row_start;
        const int64_t out0 = offsets[t];
        const int64_t k64 = offsets[t + 1] - out0;
        if (k64 <= 0) continue;
        if (k64 > (int64_t)d || out0 < 0 || out0 + k64 > n_out) {   // offsets of another call: nothing is written for this target
            if (threadIdx.x == 0 && status != nullptr) atomicOr(status, STATUS_BAD_OFFSETS);
            continue;
        }
        const int k = (int)k64;
        const uint64_t base = row_base(seed, hop, v);
        if (d > WAVE) {
            sample_heavy_row(sm, base, d, k, row_start, out0, (int)t, col, eid, out_src, out_eid, out_tgt);
            continue;
        }
        if (w != j) continue;                              // a light row: wavefront j alone
        const uint64_t key = lane < d ? key_of(base, (uint32_t)lane) : ~0ull;
        bool take = lane < d;
        if (k < d) {
            const int hi = (int)(key >> 32), lo = (int)key;
            int rank = 0;
            const int du = uniform_i(d);
            for (int i = 0; i < du; ++i) {
                const uint64_t other = ((uint64_t)(uint32_t)bcast_i(hi, i) << 32) | (uint32_t)bcast_i(lo, i);
                rank += other < key ? 1 : 0;
            }
            take = take && rank < k;
        }
        const uint64_t m = __ballot(take);
        if (take) {
            const int64_t o = out0 + __popcll(m & ((1ull << lane) - 1ull));
            out_src[o] = col[row_start + lane];
            out_eid[o] = eid[row_start + lane];
            out_tgt[o] = (int32_t)t;
        }
    }
}

// ---- relabelling: mark -> count per chunk -> scan -> positions -> local ids ----------------------------------------------------------
__global__ void __launch_bounds__(256)
relabel_mark_kernel(const int32_t* __restrict__ src, const int64_t* __restrict__ offsets, int64_t n, int64_t n_out,
                    const int64_t* __restrict__ targets, int add_self_loops, int32_t* __restrict__ scratch, int64_t N) {
    int64_t E = offsets[n];
    E = E < n_out ? E : n_out;
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < E; i += nt) {
        const int32_t g = src[i];
        if (g >= 0 && g < N) scratch[g] = 1;
    }
    if (add_self_loops)
        for (int64_t i = i0; i < n; i += nt) {
            const int64_t v = targets[i];
            if (v >= 0 && v < N) scratch[v] = 1;
        }
}

// marks of this thread's 4 consecutive scratch entries as a bit mask
__device__ __forceinline__ int marks_of(const int32_t* __restrict__ scratch, int64_t i, int64_t N) {
    if (i + 3 < N) {
        const int4 q = *reinterpret_cast<const int4*>(scratch + i);
        return (q.x != 0) | ((q.y != 0) << 1) | ((q.z != 0) << 2) | ((q.w != 0) << 3);
    }
    int m = 0;
    for (int c = 0; c < 4; ++c)
        if (i + c < N && scratch[i + c] != 0) m |= 1 << c;
    return m;
}

__global__ void __launch_bounds__(RELABEL_BLOCK)
relabel_count_kernel(const int32_t* __restrict__ scratch, int64_t N, int32_t* __restrict__ chunk_cnt) {
    __shared__ int wsum[RELABEL_BLOCK / WAVE];
    const int64_t i = (int64_t)blockIdx.x * RELABEL_CHUNK + 4 * (int64_t)threadIdx.x;
    const int c = wave_sum(__popc(marks_of(scratch, i, N)));
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// chunk_cnt[0 .. nb) -> exclusive sums in place, chunk_cnt[nb] = their total; info = (unique ids, sampled entries); one workgroup
__global__ void __launch_bounds__(1024)
relabel_scan_kernel(int32_t* __restrict__ chunk_cnt, int64_t nb, const int64_t* __restrict__ offsets, int64_t n, int64_t n_out,
                    int32_t* __restrict__ info) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b = min(nb, t * per), e = min(nb, b + per);
    long long s = 0;
    for (int64_t g = b; g < e; ++g) s += chunk_cnt[g];
    long long all;
    long long run = block_exclusive_scan<1024>(s, part, &all);
    for (int64_t g = b; g < e; ++g) {
        const int c = chunk_cnt[g];
        chunk_cnt[g] = (int)run;
        run += c;
    }
    if (t == 1023) {
        chunk_cnt[nb] = (int)all;                          // at most N < 2^31 marks
        info[0] = (int)all;
        int64_t E = offsets != nullptr ? offsets[n] : n_out;       // (the union of the hops has no offsets: its entry count is n_out)
        E = E < n_out ? E : n_out;
        info[1] = (int)(E < 0 ? 0 : E);
    }
}

// scratch[i] = 1 + position of i among the marked ids (0: not marked); n_id[position] = i
__global__ void __launch_bounds__(RELABEL_BLOCK)
relabel_positions_kernel(int32_t* __restrict__ scratch, int64_t N, const int32_t* __restrict__ chunk_cnt, int64_t nb, int64_t U,
                         int64_t* __restrict__ n_id, int32_t* __restrict__ status) {
    __shared__ int wsum[RELABEL_BLOCK / WAVE];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0 && chunk_cnt[nb] != U && status != nullptr) atomicOr(status, STATUS_BAD_OFFSETS);
    const int64_t i = (int64_t)blockIdx.x * RELABEL_CHUNK + 4 * (int64_t)threadIdx.x;
    const int m = marks_of(scratch, i, N);
    const int c = __popc(m);
    int incl = c;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == WAVE - 1) wsum[w] = incl;
    __syncthreads();
    int64_t pos = (int64_t)chunk_cnt[blockIdx.x] + incl - c;
    for (int j = 0; j < w; ++j) pos += wsum[j];
    for (int q = 0; q < 4; ++q) {
        if (i + q >= N) break;
        const bool on = (m >> q) & 1;
        scratch[i + q] = on ? (int32_t)(pos + 1) : 0;
        if (on) {
            if (pos < U) n_id[pos] = i + q;
            ++pos;
        }
    }
}

__global__ void __launch_bounds__(256)
relabel_edges_kernel(const int32_t* __restrict__ scratch, int64_t N, const int32_t* __restrict__ src, const int32_t* __restrict__ eid,
                     const int32_t* __restrict__ tgt, int64_t E, const int64_t* __restrict__ targets, int64_t n,
                     int64_t* __restrict__ edge_src, int64_t* __restrict__ edge_dst, int64_t* __restrict__ e_id,
                     int64_t* __restrict__ res_n_id) {
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < E; i += nt) {
        const int32_t g = src[i];
        edge_src[i] = (g >= 0 && g < N) ? (int64_t)scratch[g] - 1 : -1;
        edge_dst[i] = tgt[i];
        e_id[i] = eid[i];
    }
    if (res_n_id != nullptr)
        for (int64_t i = i0; i < n; i += nt) {
            const int64_t v = targets[i];
            res_n_id[i] = (v >= 0 && v < N) ? (int64_t)scratch[v] - 1 : -1;
        }
}

// ---- the one-id-space flow: the union of the hops' entries and of the batch, relabelled on both ends -------------------------------------
// Replaces the `n_id.unique()` / `tmp[n_id] = arange` / `tmp[...]` lines of PyG 1.4.2 NeighborSampler.__produce_subgraph__.  Same scheme
// as a hop's relabelling (idempotent marks in the N-entry scratch, relabel_count / scan / positions as they are); only what is marked
// and what is looked up differ.
__global__ void __launch_bounds__(256)
union_mark_kernel(const int32_t* __restrict__ src_g, const int32_t* __restrict__ dst_g, int64_t E, const int64_t* __restrict__ b_id,
                  int64_t n, int32_t* __restrict__ scratch, int64_t N, int32_t* __restrict__ status) {
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    for (int64_t i = i0; i < E; i += nt) {
        const int32_t s = src_g[i], d = dst_g[i];
        if (s >= 0 && s < N) scratch[s] = 1; else bad = true;
        if (d >= 0 && d < N) scratch[d] = 1; else bad = true;
    }
    for (int64_t i = i0; i < n; i += nt) {
        const int64_t v = b_id[i];
        if (v >= 0 && v < N) scratch[v] = 1; else bad = true;       // dropped and reported, never dereferenced
    }
    if (bad && status != nullptr) atomicOr(status, STATUS_BAD_TARGET);
}

// after relabel_positions_kernel: scratch[g] - 1 = position of g in n_id
__global__ void __launch_bounds__(256)
union_local_kernel(const int32_t* __restrict__ scratch, int64_t N, const int32_t* __restrict__ src_g, const int32_t* __restrict__ dst_g,
                   int64_t E, const int64_t* __restrict__ b_id, int64_t n, const int32_t* __restrict__ chunk_cnt, int64_t nb, int64_t cap,
                   int32_t* __restrict__ src_l, int32_t* __restrict__ dst_l, int64_t* __restrict__ sub_b_id, int32_t* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && chunk_cnt[nb] > cap && status != nullptr) atomicOr(status, STATUS_BAD_OFFSETS);
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < E; i += nt) {
        const int32_t s = src_g[i], d = dst_g[i];
        src_l[i] = (s >= 0 && s < N) ? scratch[s] - 1 : -1;
        dst_l[i] = (d >= 0 && d < N) ? scratch[d] - 1 : -1;
    }
    for (int64_t i = i0; i < n; i += nt) {
        const int64_t v = b_id[i];
        sub_b_id[i] = (v >= 0 && v < N) ? (int64_t)scratch[v] - 1 : -1;
    }
}

// ---- merging the equal (source, target) pairs of a sampled subgraph (npi_sample_coalesce; the sort and the scan: sort.h) -------------------
// Replaces the `idx = src * num_nodes + dst; idx.unique()` + `scatter_` lines of PyG 1.4.2 NeighborSampler.__produce_subgraph__.  LSD over
// the pair: the stable sort by target first, then the stable sort by source; val = the entry's index, so equal pairs stay in entry order.
__global__ void coalesce_keys_kernel(const int32_t* __restrict__ dst_l, int64_t E, uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    keys[i] = (uint32_t)dst_l[i];
    vals[i] = (int32_t)i;
}
__global__ void coalesce_rekey_kernel(const int32_t* __restrict__ src_l, const int32_t* __restrict__ vals, int64_t E,
                                      uint32_t* __restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < E) keys[p] = (uint32_t)src_l[vals[p]];
}
// dst_s[p] = the target of the entry sorted to p (its source: the sort's key); head[p] = 1 where a run of equal pairs starts
__global__ void coalesce_heads_kernel(const uint32_t* __restrict__ src_s, const int32_t* __restrict__ vals, const int32_t* __restrict__ dst_l,
                                      int64_t E, int32_t* __restrict__ dst_s, int32_t* __restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const int32_t d = dst_l[vals[p]];
    dst_s[p] = d;
    head[p] = (p == 0 || src_s[p - 1] != src_s[p] || dst_l[vals[p - 1]] != d) ? 1 : 0;
}
// pos = the exclusive scan of head.  The head of a run writes the pair and the smallest eid of its run (runs are short: a pair
// repeats once per hop it was sampled in and once per parallel edge); info[0] = the number of runs
__global__ void coalesce_compact_kernel(const uint32_t* __restrict__ src_s, const int32_t* __restrict__ dst_s, const int32_t* __restrict__ vals,
                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ eid, int64_t E,
                                        int64_t* __restrict__ edge_src, int64_t* __restrict__ edge_dst, int64_t* __restrict__ e_id,
                                        int32_t* __restrict__ info) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const uint32_t s = src_s[p];
    const int32_t d = dst_s[p];
    const bool head = p == 0 || src_s[p - 1] != s || dst_s[p - 1] != d;
    const int64_t q = pos[p];                                    // q <= p < E: within the caller's bound
    if (p == E - 1) info[0] = (int32_t)(q + (head ? 1 : 0));
    if (!head) return;
    int32_t m = eid[vals[p]];
    for (int64_t r = p + 1; r < E && src_s[r] == s && dst_s[r] == d; ++r) {
        const int32_t e = eid[vals[r]];
        m = e < m ? e : m;
    }
    edge_src[q] = (int64_t)(int32_t)s;
    edge_dst[q] = d;
    e_id[q] = m;
}

}  // namespace npi

using namespace npi;

extern "C" int npi_sample_counts(const int32_t* rowptr, int64_t N, const int64_t* targets, int64_t n, int64_t budget, float frac,
                                 int32_t* cnt, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(n), "npi_sample_counts: bad size");
    NPI_REQUIRE(budget >= 0, "npi_sample_counts: a budget below 1");
    if (budget > 0) NPI_REQUIRE(frac == 0.f, "npi_sample_counts: a budget and a fraction together");
    else NPI_REQUIRE(frac > 0.f && frac <= 1.f, "npi_sample_counts: a budget below 1, or a fraction outside (0, 1]");
    if (n > 0) NPI_REQUIRE(rowptr && targets && cnt, "npi_sample_counts: null pointer");
    if (status != nullptr) (void)hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    if (n == 0) return NPI_OK;
    sample_counts_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, stream>>>(rowptr, N, targets, n, budget, frac, cnt, status);
    return check_launch("npi_sample_counts");
}

extern "C" int npi_sample_select(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t N, const int64_t* targets,
                                 int64_t n, const int64_t* offsets, int64_t seed, int64_t hop, int32_t* out_src, int32_t* out_eid,
                                 int32_t* out_tgt, int64_t n_out, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(n) && n_out >= 0 && n_out <= NPI_INDEX_LIMIT, "npi_sample_select: bad size");
    NPI_REQUIRE(count_ok(hop), "npi_sample_select: bad hop");
    if (n == 0) return NPI_OK;
    NPI_REQUIRE(rowptr && targets && offsets, "npi_sample_select: null pointer");
    if (n_out > 0) NPI_REQUIRE(col && eid && out_src && out_eid && out_tgt, "npi_sample_select: null pointer");
    sample_select_kernel<<<(unsigned)ceil_div(n, SAMPLE_WAVES), SAMPLE_BLOCK, 0, stream>>>(rowptr, col, eid, N, targets, n, offsets, seed,
                                                                                        hop, out_src, out_eid, out_tgt, n_out, status);
    return check_launch("npi_sample_select");
}

extern "C" int64_t npi_sample_workspace_elems(int64_t N) {
    if (!count_ok(N)) return -1;
    return ceil_div(N, RELABEL_CHUNK) + 1;
}

extern "C" int npi_sample_relabel_count(const int32_t* out_src, const int64_t* offsets, int64_t n, int64_t n_out, const int64_t* targets,
                                        int add_self_loops, int32_t* scratch, int64_t N, int32_t* workspace, int32_t* info,
                                        void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(n) && n_out >= 0 && n_out <= NPI_INDEX_LIMIT,
                "npi_sample_relabel_count: bad size");
    NPI_REQUIRE(offsets && workspace && info, "npi_sample_relabel_count: null pointer");
    NPI_REQUIRE(N == 0 || scratch, "npi_sample_relabel_count: null pointer");
    NPI_REQUIRE((n == 0 || targets) && (n_out == 0 || out_src), "npi_sample_relabel_count: null pointer");
    NPI_REQUIRE(((uintptr_t)scratch & 15) == 0, "npi_sample_relabel_count: scratch must be 16-byte aligned");
    const int64_t nb = ceil_div(N, RELABEL_CHUNK);
    if (N > 0 && (n_out > 0 || (add_self_loops && n > 0)))
        relabel_mark_kernel<<<stride_grid(n_out > n ? n_out : n, 256, 4096), 256, 0, stream>>>(out_src, offsets, n, n_out, targets,
                                                                                              add_self_loops, scratch, N);
    if (nb > 0) relabel_count_kernel<<<(unsigned)nb, RELABEL_BLOCK, 0, stream>>>(scratch, N, workspace);
    relabel_scan_kernel<<<1, 1024, 0, stream>>>(workspace, nb, offsets, n, n_out, info);
    return check_launch("npi_sample_relabel_count");
}

extern "C" int npi_sample_relabel(int32_t* scratch, int64_t N, const int32_t* workspace, const int32_t* out_src, const int32_t* out_eid,
                                  const int32_t* out_tgt, int64_t E, const int64_t* targets, int64_t n, int64_t U, int64_t* n_id,
                                  int64_t* edge_src, int64_t* edge_dst, int64_t* e_id, int64_t* res_n_id, int32_t* status,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(n) && E >= 0 && E <= NPI_INDEX_LIMIT && U >= 0 && U <= N,
                "npi_sample_relabel: bad size");
    NPI_REQUIRE(workspace && (N == 0 || scratch), "npi_sample_relabel: null pointer");
    NPI_REQUIRE(U == 0 || n_id, "npi_sample_relabel: null pointer");
    NPI_REQUIRE(E == 0 || (out_src && out_eid && out_tgt && edge_src && edge_dst && e_id), "npi_sample_relabel: null pointer");
    NPI_REQUIRE(res_n_id == nullptr || n == 0 || targets, "npi_sample_relabel: null pointer");
    NPI_REQUIRE(((uintptr_t)scratch & 15) == 0, "npi_sample_relabel: scratch must be 16-byte aligned");
    const int64_t nb = ceil_div(N, RELABEL_CHUNK);
    if (nb > 0) relabel_positions_kernel<<<(unsigned)nb, RELABEL_BLOCK, 0, stream>>>(scratch, N, workspace, nb, U, n_id, status);
    if (E > 0 || (res_n_id != nullptr && n > 0))
        relabel_edges_kernel<<<stride_grid(E > n ? E : n, 256, 4096), 256, 0, stream>>>(scratch, N, out_src, out_eid, out_tgt, E, targets, n,
                                                                                       edge_src, edge_dst, e_id, res_n_id);
    if (N > 0) (void)hipMemsetAsync(scratch, 0, (size_t)N * sizeof(int32_t), stream);   // the scratch is left as it was found
    return check_launch("npi_sample_relabel");
}

extern "C" int npi_sample_union(const int32_t* src_g, const int32_t* dst_g, int64_t E, const int64_t* b_id, int64_t n, int32_t* scratch,
                                int64_t N, int32_t* workspace, int64_t n_id_cap, int64_t* n_id, int32_t* src_l, int32_t* dst_l,
                                int64_t* sub_b_id, int32_t* info, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(n) && count_ok(E) && n_id_cap >= 0 && n_id_cap <= N,
                "npi_sample_union: bad size");
    if (E == 0 && n == 0) return NPI_OK;
    NPI_REQUIRE(workspace && info && (N == 0 || scratch) && (n_id_cap == 0 || n_id), "npi_sample_union: null pointer");
    NPI_REQUIRE((E == 0 || (src_g && dst_g && src_l && dst_l)) && (n == 0 || (b_id && sub_b_id)), "npi_sample_union: null pointer");
    NPI_REQUIRE(((uintptr_t)scratch & 15) == 0, "npi_sample_union: scratch must be 16-byte aligned");
    const int64_t nb = ceil_div(N, RELABEL_CHUNK);
    const unsigned grid = stride_grid(E > n ? E : n, 256, 4096);
    union_mark_kernel<<<grid, 256, 0, stream>>>(src_g, dst_g, E, b_id, n, scratch, N, status);
    if (nb > 0) relabel_count_kernel<<<(unsigned)nb, RELABEL_BLOCK, 0, stream>>>(scratch, N, workspace);
    relabel_scan_kernel<<<1, 1024, 0, stream>>>(workspace, nb, nullptr, 0, E, info);
    // (positions: n_id within the caller's capacity; more marks than that are reported by union_local_kernel)
    if (nb > 0) relabel_positions_kernel<<<(unsigned)nb, RELABEL_BLOCK, 0, stream>>>(scratch, N, workspace, nb, n_id_cap, n_id, nullptr);
    union_local_kernel<<<grid, 256, 0, stream>>>(scratch, N, src_g, dst_g, E, b_id, n, workspace, nb, n_id_cap, src_l, dst_l, sub_b_id,
                                                 status);
    if (N > 0) (void)hipMemsetAsync(scratch, 0, (size_t)N * sizeof(int32_t), stream);   // the scratch is left as it was found
    return check_launch("npi_sample_union");
}

extern "C" int64_t npi_sample_coalesce_workspace_bytes(int64_t E) {
    if (!count_ok(E)) return -1;
    return PairSort::bytes(E);
}

extern "C" int npi_sample_coalesce(const int32_t* src_l, const int32_t* dst_l, const int32_t* eid, int64_t E, int64_t U, int64_t* edge_src,
                                   int64_t* edge_dst, int64_t* e_id, int32_t* info, void* workspace, int64_t workspace_bytes,
                                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(E) && count_ok(U), "npi_sample_coalesce: bad size");
    if (E == 0) return NPI_OK;
    NPI_REQUIRE(src_l && dst_l && eid && edge_src && edge_dst && e_id && info && workspace, "npi_sample_coalesce: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace & 15) == 0, "npi_sample_coalesce: workspace must be 16-byte aligned");
    if (workspace_short("npi_sample_coalesce", workspace_bytes, PairSort::bytes(E))) return NPI_ERR_WORKSPACE;
    PairSort ps;
    (void)ps.carve(workspace, workspace_bytes, E);         // (the length was checked above)
    const int bits = key_bits(U);                        // local ids lie in [0, U)
    const unsigned eb = (unsigned)ceil_div(E, 256);
    coalesce_keys_kernel<<<eb, 256, 0, stream>>>(dst_l, E, ps.keys_a, ps.vals_a);
    ps.sort(bits, stream);
    coalesce_rekey_kernel<<<eb, 256, 0, stream>>>(src_l, ps.vals_a, E, ps.keys_a);
    ps.sort(bits, stream);
    // the sort's free buffers (PairSort): the sorted targets, the run heads and the scan's tile sums
    int32_t* dst_s = ps.vals_b;
    int32_t* head = (int32_t*)ps.keys_b;
    coalesce_heads_kernel<<<eb, 256, 0, stream>>>(ps.keys_a, ps.vals_a, dst_l, E, dst_s, head);
    exclusive_scan_i32(head, E, ps.counts, stream);
    coalesce_compact_kernel<<<eb, 256, 0, stream>>>(ps.keys_a, dst_s, ps.vals_a, head, eid, E, edge_src, edge_dst, e_id, info);
    return check_launch("npi_sample_coalesce");
}
