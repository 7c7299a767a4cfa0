// Per-graph readouts under Rule O (include/npi_gnn.h): PyG 1.4.2 `global_add_pool`, `global_sort_pool` and the softmax + weighted sum of
// `GlobalAttention`, forward and backward.  graph_ptr [B + 1] are the segment starts of a PyG batch (nodes contiguous per graph).
//
//   add / attention   a graph is cut into chunks of NPI_READOUT_CHUNK of its own rows; ONE workgroup reduces one chunk (and one block of
//                     64 columns), so a single graph of a million rows is ~1,000 workgroups and 200 graphs of 200 rows are 200.  The
//                     workgroup -> (graph, chunk) map is an exclusive scan of max(1, ceil(n_g / chunk)) (readout_map_kernel); a graph of
//                     one chunk is finished by the first launch, longer ones by a merge launch over their partials, ascending.
//   order of a sum    inside a chunk, row lane l of 16 adds rows l, l + 16, ... ascending; the 16 lanes are added ascending; the chunks are
//                     added ascending.  Columns always travel in groups of 4 (thread <-> columns 4q .. 4q + 3): the width of the loads
//                     (16 / 8 / 4 bytes, picked from F, the pitches and the base pointers) changes the instructions, never the sums.
//   sort pool         the order is npi_topk_select / npi_topk_select_sorted with ratio 1.0 over canonical keys (npi_sort_pool_keys); the
//                     kernels here copy rows into their slots and back.
// No float atomics; nothing is allocated or read back: every entry point may run inside a stream capture.
#include <algorithm>
#include <initializer_list>
#include "sort.h"

namespace npi {

constexpr int RO_CHUNK = NPI_READOUT_CHUNK;
constexpr int RO_THREADS = 256;
constexpr int RO_LANES = 16;                 // row lanes of a workgroup
constexpr int RO_GROUPS = 16;                // groups of 4 columns of a workgroup
constexpr int RO_COLS = RO_GROUPS * 4;       // columns per workgroup (blockIdx.y walks the rest)
constexpr int RO_STRIP = 16;                 // consecutive rows per wave in the row-parallel backward kernels
constexpr int RO_MAP_THREADS = 1024;
static_assert(RO_LANES * RO_GROUPS == RO_THREADS && RO_CHUNK % RO_THREADS == 0, "readout geometry");

// 4 adjacent columns of a row (nvalid of them exist, the rest read as 0 / are not written); VEC = floats per load
template <int VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int nvalid, float (&v)[4]) {
    if (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if (VEC == 2) {                                  // F is even: 2 or 4 columns
        const float2 a = *reinterpret_cast<const float2*>(p);
        v[0] = a.x; v[1] = a.y; v[2] = 0.f; v[3] = 0.f;
        if (nvalid > 2) {
            const float2 b = *reinterpret_cast<const float2*>(p + 2);
            v[2] = b.x; v[3] = b.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < nvalid ? p[k] : 0.f;
    }
}
template <int VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int nvalid, const float (&v)[4]) {
    if (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (VEC == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
        if (nvalid > 2) *reinterpret_cast<float2*>(p + 2) = make_float2(v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nvalid) p[k] = v[k];
    }
}

__device__ __forceinline__ int clamp_row(int v, int N) { return v < 0 ? 0 : (v > N ? N : v); }

// chunk_ptr[g] = sum over g' < g of max(1, ceil(n_g' / chunk)): an empty graph keeps one (empty) chunk, whose workgroup writes its zeros
__global__ void __launch_bounds__(RO_MAP_THREADS)
readout_map_kernel(const int32_t* __restrict__ graph_ptr, int B, int N, int32_t* __restrict__ chunk_ptr) {
    __shared__ int lds[RO_MAP_THREADS];
    int carry = 0;
    for (int base = 0; base < B; base += RO_MAP_THREADS) {
        const int g = base + threadIdx.x;
        int v = 0;
        if (g < B) {
            const int n = clamp_row(graph_ptr[g + 1], N) - clamp_row(graph_ptr[g], N);
            v = n > 0 ? (n - 1) / RO_CHUNK + 1 : 1;
        }
        int total;
        const int excl = block_exclusive_scan<RO_MAP_THREADS>(v, lds, &total);
        if (g < B) chunk_ptr[g] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) chunk_ptr[B] = carry;
}

// workgroup w -> its graph, its chunk of it, the number of chunks of that graph and the chunk's rows [b, e); false: no work
struct ChunkOf { int g, nch, b, e; };
__device__ __forceinline__ bool locate_chunk(const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ chunk_ptr, int B, int N,
                                             int w, ChunkOf& at) {
    if (w >= chunk_ptr[B]) return false;
    int lo = 0, hi = B;                                      // the largest g with chunk_ptr[g] <= w (strictly increasing)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_ptr[mid] <= w) lo = mid; else hi = mid;
    }
    at.g = lo;
    at.nch = chunk_ptr[lo + 1] - chunk_ptr[lo];
    const int gb = clamp_row(graph_ptr[lo], N), ge = clamp_row(graph_ptr[lo + 1], N);
    at.b = gb + (w - chunk_ptr[lo]) * RO_CHUNK;
    at.e = min(ge, at.b + RO_CHUNK);
    if (at.e < at.b) at.e = at.b;
    return true;
}

// ---- O-add -------------------------------------------------------------------------------------------------------------------------
template <int VEC>
__global__ void __launch_bounds__(RO_THREADS)
readout_add_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ graph_ptr,
                   const int32_t* __restrict__ chunk_ptr, int B, int F, int N, float* __restrict__ out, int64_t ldo,
                   float* __restrict__ part /* [workgroups, F] */) {
    __shared__ float sum_s[RO_LANES][RO_COLS];
    ChunkOf at;
    if (!locate_chunk(graph_ptr, chunk_ptr, B, N, blockIdx.x, at)) return;
    const int cgi = threadIdx.x % RO_GROUPS, rl = threadIdx.x / RO_GROUPS;
    const int c0 = blockIdx.y * RO_COLS + cgi * 4;
    const int nvalid = min(4, F - c0);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (nvalid > 0) {
#pragma unroll 4
        for (int i = at.b + rl; i < at.e; i += RO_LANES) {
            float v[4];
            load4<VEC>(x + (int64_t)i * ldx + c0, nvalid, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sum_s[rl][cgi * 4 + k] = acc[k];
    __syncthreads();
    const int col = blockIdx.y * RO_COLS + threadIdx.x;
    if (threadIdx.x < RO_COLS && col < F) {
        float t = sum_s[0][threadIdx.x];
#pragma unroll
        for (int r = 1; r < RO_LANES; ++r) t += sum_s[r][threadIdx.x];
        if (at.nch == 1) out[(int64_t)at.g * ldo + col] = t;
        else part[(int64_t)blockIdx.x * F + col] = t;
    }
}

// graphs of more than one chunk: the partials, ascending
__global__ void __launch_bounds__(64)
readout_add_merge_kernel(const int32_t* __restrict__ chunk_ptr, int F, const float* __restrict__ part, float* __restrict__ out,
                         int64_t ldo) {
    const int g = blockIdx.x;
    const int w0 = chunk_ptr[g], nch = chunk_ptr[g + 1] - w0;
    if (nch <= 1) return;
    const int col = blockIdx.y * 64 + threadIdx.x;
    if (col >= F) return;
    const float* __restrict__ p = part + (int64_t)w0 * F + col;
    float t = p[0];
#pragma unroll 16
    for (int c = 1; c < nch; ++c) t += p[(int64_t)c * F];
    out[(int64_t)g * ldo + col] = t;
}

// which graph owns row i, for a wave that walks consecutive rows: `find` once, then `advance` (empty graphs are stepped over)
struct GraphWalk {
    int g, gend;
    __device__ __forceinline__ void find(const int32_t* __restrict__ graph_ptr, int B, int i) {
        int lo = 0, hi = B;                                  // the largest g < B with graph_ptr[g] <= i: the one graph that holds row i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (graph_ptr[mid] <= i) lo = mid; else hi = mid;
        }
        g = lo;
        gend = graph_ptr[lo + 1];
    }
    // true when the graph changed
    __device__ __forceinline__ bool advance(const int32_t* __restrict__ graph_ptr, int B, int i) {
        if (i < gend) return false;
        do { ++g; } while (g + 1 < B && graph_ptr[g + 1] <= i);
        gend = graph_ptr[g + 1];
        return true;
    }
};

// dx[i] = dout[g(i)]; rows outside [graph_ptr[0], graph_ptr[B]) are written as zeros.  One wave per strip of RO_STRIP rows.
template <int VEC>
__global__ void __launch_bounds__(RO_THREADS)
readout_add_bwd_kernel(const float* __restrict__ dout, int64_t ldd, const int32_t* __restrict__ graph_ptr, int B, int F, int N,
                       float* __restrict__ dx, int64_t lddx) {
    const int lane = lane_id();
    const int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RO_STRIP, i1 = min(N, i0 + RO_STRIP);
    const int first = graph_ptr[0], last = graph_ptr[B];
    GraphWalk at;
    at.g = -1;
    for (int i = i0; i < i1; ++i) {
        const bool owned = i >= first && i < last;
        if (owned) {
            if (at.g < 0) at.find(graph_ptr, B, i); else at.advance(graph_ptr, B, i);
        }
        const float* __restrict__ src = dout + (int64_t)(owned ? at.g : 0) * ldd;
        float* __restrict__ dst = dx + (int64_t)i * lddx;
        for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) {
            const int nvalid = min(4, F - c0);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (owned) load4<VEC>(src + c0, nvalid, v);
            store4<VEC>(dst + c0, nvalid, v);
        }
    }
}

// ---- O-att -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

constexpr float RO_EPS = 1e-16f;                            // PyG's softmax: e / (sum + 1e-16)

template <int VEC>
__global__ void __launch_bounds__(RO_THREADS)
readout_att_kernel(const float* __restrict__ gate, const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ graph_ptr,
                   const int32_t* __restrict__ chunk_ptr, int B, int F, int N, float* __restrict__ out, int64_t ldo,
                   float* __restrict__ m_out, float* __restrict__ s_out, float* __restrict__ pm, float* __restrict__ ps,
                   float* __restrict__ pacc /* [workgroups, F] */) {
    __shared__ float e_s[RO_CHUNK];
    __shared__ float acc_s[RO_LANES][RO_COLS];
    __shared__ float sl_s[RO_LANES];
    __shared__ float max_s[RO_THREADS / WAVE];
    ChunkOf at;
    if (!locate_chunk(graph_ptr, chunk_ptr, B, N, blockIdx.x, at)) return;
    const int n = at.e - at.b;
    // the chunk's maximum (exact, any order), then e_j = exp(gate_j - max) once per row, in LDS
    constexpr int PER = RO_CHUNK / RO_THREADS;
    float gv[PER];
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = q * RO_THREADS + threadIdx.x;
        gv[q] = j < n ? gate[at.b + j] : -INFINITY;
        mx = fmaxf(mx, gv[q]);
    }
    mx = wave_max(mx);
    if (lane_id() == 0) max_s[threadIdx.x >> 6] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(max_s[0], max_s[1]), fmaxf(max_s[2], max_s[3]));
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = q * RO_THREADS + threadIdx.x;
        if (j < n) e_s[j] = expf(gv[q] - m);
    }
    __syncthreads();
    const int cgi = threadIdx.x % RO_GROUPS, rl = threadIdx.x / RO_GROUPS;
    const int c0 = blockIdx.y * RO_COLS + cgi * 4;
    const int nvalid = min(4, F - c0);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, sl = 0.f;
    if (nvalid > 0) {                                        // (column group 0 of a workgroup always exists: it also sums the e_j)
#pragma unroll 4
        for (int j = rl; j < n; j += RO_LANES) {
            const float ev = e_s[j];
            float v[4];
            load4<VEC>(x + (int64_t)(at.b + j) * ldx + c0, nvalid, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(ev, v[k], acc[k]);
            sl += ev;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc_s[rl][cgi * 4 + k] = acc[k];
    if (cgi == 0) sl_s[rl] = sl;
    __syncthreads();
    const int col = blockIdx.y * RO_COLS + threadIdx.x;
    if (threadIdx.x < RO_COLS) {
        float s = sl_s[0];
#pragma unroll
        for (int r = 1; r < RO_LANES; ++r) s += sl_s[r];
        const bool scalar = blockIdx.y == 0 && threadIdx.x == 0;
        if (col < F) {
            float t = acc_s[0][threadIdx.x];
#pragma unroll
            for (int r = 1; r < RO_LANES; ++r) t += acc_s[r][threadIdx.x];
            if (at.nch == 1) out[(int64_t)at.g * ldo + col] = t / (s + RO_EPS);       // an empty graph: 0 / 1e-16 = 0
            else pacc[(int64_t)blockIdx.x * F + col] = t;
        }
        if (scalar) {
            if (at.nch == 1) { m_out[at.g] = n > 0 ? m : 0.f; s_out[at.g] = s; }
            else { pm[blockIdx.x] = m; ps[blockIdx.x] = s; }
        }
    }
}

// graphs of more than one chunk: m = max_c m_c;  s = sum_c s_c exp(m_c - m);  acc = sum_c acc_c exp(m_c - m), both ascending
__global__ void __launch_bounds__(64)
readout_att_merge_kernel(const int32_t* __restrict__ chunk_ptr, int F, const float* __restrict__ pm, const float* __restrict__ ps,
                         const float* __restrict__ pacc, float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                         float* __restrict__ s_out) {
    const int g = blockIdx.x;
    const int w0 = chunk_ptr[g], nch = chunk_ptr[g + 1] - w0;
    if (nch <= 1) return;
    float m = pm[w0];
    for (int c = 1; c < nch; ++c) m = fmaxf(m, pm[w0 + c]);
    const int col = blockIdx.y * 64 + threadIdx.x;
    const bool live = col < F;
    const float* __restrict__ p = pacc + (int64_t)w0 * F + (live ? col : 0);
    float f = expf(pm[w0] - m);
    float s = ps[w0] * f, t = p[0] * f;
#pragma unroll 8
    for (int c = 1; c < nch; ++c) {
        f = expf(pm[w0 + c] - m);
        s = fmaf(ps[w0 + c], f, s);
        t = fmaf(p[(int64_t)c * F], f, t);
    }
    if (live) out[(int64_t)g * ldo + col] = t / (s + RO_EPS);
    if (blockIdx.y == 0 && threadIdx.x == 0) { m_out[g] = m; s_out[g] = s; }
}

// alpha_i = exp(gate_i - m_g) / (s_g + 1e-16);  dx_i = alpha_i dout_g;  dgate_i = alpha_i (<dout_g, x_i> - <dout_g, out_g>).
// One wave per strip of RO_STRIP rows; lane l owns the columns 4l .. 4l + 3 (+ 256 q): a fixed map, then the xor butterfly.
template <int VEC>
__global__ void __launch_bounds__(RO_THREADS)
readout_att_bwd_kernel(const float* __restrict__ gate, const float* __restrict__ x, int64_t ldx,
                       const int32_t* __restrict__ graph_ptr, int B, int F, int N, const float* __restrict__ out, int64_t ldo,
                       const float* __restrict__ m_in, const float* __restrict__ s_in, const float* __restrict__ dout, int64_t ldd,
                       float* __restrict__ dx, int64_t lddx, float* __restrict__ dgate) {
    const int lane = lane_id();
    const int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RO_STRIP, i1 = min(N, i0 + RO_STRIP);
    const int first = graph_ptr[0], last = graph_ptr[B];
    GraphWalk at;
    at.g = -1;
    float cg = 0.f, mg = 0.f, inv = 0.f;
    for (int i = i0; i < i1; ++i) {
        float* __restrict__ dst = dx + (int64_t)i * lddx;
        if (i < first || i >= last) {                        // a row of no graph
            const float z[4] = {0.f, 0.f, 0.f, 0.f};
            for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) store4<VEC>(dst + c0, min(4, F - c0), z);
            if (lane == 0) dgate[i] = 0.f;
            continue;
        }
        bool fresh;
        if (at.g < 0) { at.find(graph_ptr, B, i); fresh = true; }
        else fresh = at.advance(graph_ptr, B, i);
        const float* __restrict__ dg = dout + (int64_t)at.g * ldd;
        if (fresh) {
            const float* __restrict__ og = out + (int64_t)at.g * ldo;
            float c = 0.f;
            for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) {
                const int nvalid = min(4, F - c0);
                float a[4], b[4];
                load4<VEC>(dg + c0, nvalid, a);
                load4<VEC>(og + c0, nvalid, b);
#pragma unroll
                for (int k = 0; k < 4; ++k) c = fmaf(a[k], b[k], c);
            }
            cg = wave_sum(c);
            mg = m_in[at.g];
            inv = 1.f / (s_in[at.g] + RO_EPS);
        }
        const float* __restrict__ xr = x + (int64_t)i * ldx;
        float d = 0.f;
        for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) {
            const int nvalid = min(4, F - c0);
            float a[4], b[4];
            load4<VEC>(dg + c0, nvalid, a);
            load4<VEC>(xr + c0, nvalid, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) d = fmaf(a[k], b[k], d);
        }
        d = wave_sum(d);
        const float alpha = expf(gate[i] - mg) * inv;
        for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) {
            const int nvalid = min(4, F - c0);
            float a[4];
            load4<VEC>(dg + c0, nvalid, a);
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] *= alpha;
            store4<VEC>(dst + c0, nvalid, a);
        }
        if (lane == 0) dgate[i] = alpha * (d - cg);
    }
}

// ---- O-sort ------------------------------------------------------------------------------------------------------------------------
// keys[i] = x[i, F - 1] with every NaN written as 0x7fc00000
__global__ void sort_pool_keys_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int F, float* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float v = x[i * ldx + (F - 1)];
    keys[i] = (v != v) ? __uint_as_float(0x7fc00000u) : v;
}

// slot (g, r) of out <- row order[graph_ptr[g] + r] of x, or zeros when the graph has no rank r; one wave per slot
template <int VEC>
__global__ void __launch_bounds__(RO_THREADS)
sort_pool_gather_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ order,
                        const int32_t* __restrict__ graph_ptr, int N, int B, int F, int k, float* __restrict__ out, int64_t ldo) {
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= (int64_t)B * k) return;
    const int g = (int)(q / k), r = (int)(q % k);
    const int b = graph_ptr[g], n = graph_ptr[g + 1] - b;
    int node = r < n ? order[b + r] : -1;
    if (node >= N) node = -1;                                // (an order of another batch: nothing is read out of bounds)
    float* __restrict__ dst = out + (int64_t)g * ldo + (int64_t)r * F;
    const float* __restrict__ src = x + (int64_t)(node < 0 ? 0 : node) * ldx;
    for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) {
        const int nvalid = min(4, F - c0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (node >= 0) load4<VEC>(src + c0, nvalid, v);
        store4<VEC>(dst + c0, nvalid, v);
    }
}

// dx[i] = the slot row i was copied to, or zeros; remap[i] = graph_ptr[g] + rank (-1: a row of no graph); one wave per row
template <int VEC>
__global__ void __launch_bounds__(RO_THREADS)
sort_pool_bwd_kernel(const float* __restrict__ dout, int64_t ldd, const int32_t* __restrict__ remap,
                     const int32_t* __restrict__ graph_ptr, int N, int B, int F, int k, float* __restrict__ dx, int64_t lddx) {
    const int lane = lane_id();
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int p = remap[i];
    const float* __restrict__ src = dout;
    bool ranked = false;
    if (p >= graph_ptr[0] && p < graph_ptr[B]) {
        GraphWalk at;
        at.find(graph_ptr, B, p);
        const int r = p - graph_ptr[at.g];
        ranked = r < k;
        if (ranked) src = dout + (int64_t)at.g * ldd + (int64_t)r * F;
    }
    float* __restrict__ dst = dx + (int64_t)i * lddx;
    for (int c0 = lane * 4; c0 < F; c0 += WAVE * 4) {
        const int nvalid = min(4, F - c0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (ranked) load4<VEC>(src + c0, nvalid, v);
        store4<VEC>(dst + c0, nvalid, v);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// workspace: chunk_ptr int32 [B + 1] | pm f32 [W] | ps f32 [W] | pacc f32 [W, F], W = N / chunk + B workgroups at most (each 16-byte aligned)
struct ReadoutWorkspace {
    int32_t* chunk_ptr;
    float *pm, *ps, *pacc;
    static int64_t workgroups(int64_t N, int64_t B) { return N / RO_CHUNK + B; }
    static int64_t bytes(int64_t N, int64_t B, int64_t F, bool attention) {
        const int64_t W = workgroups(N, B);
        return align_up((B + 1) * 4, 16) + (attention ? 2 * align_up(W * 4, 16) : 0) + align_up(W * F * 4, 16);
    }
    void carve(void* ws, int64_t N, int64_t B, bool attention) {
        const int64_t W = workgroups(N, B);
        char* p = (char*)ws;
        chunk_ptr = (int32_t*)p; p += align_up((B + 1) * 4, 16);
        pm = ps = nullptr;
        if (attention) { pm = (float*)p; p += align_up(W * 4, 16); ps = (float*)p; p += align_up(W * 4, 16); }
        pacc = (float*)p;
    }
};
static bool readout_sizes_ok(int64_t N, int64_t B, int64_t F) {
    return count_ok(N) && count_ok(B) && F > 0 && F < NPI_INDEX_LIMIT && ReadoutWorkspace::workgroups(N, B) < NPI_INDEX_LIMIT &&
           ceil_div(F, RO_COLS) <= 65535;
}

#define RO_DISPATCH(vec, kernel, grid, block, ...)                                            \
    do {                                                                                      \
        if ((vec) == 4) kernel<4><<<grid, block, 0, stream>>>(__VA_ARGS__);                   \
        else if ((vec) == 2) kernel<2><<<grid, block, 0, stream>>>(__VA_ARGS__);              \
        else kernel<1><<<grid, block, 0, stream>>>(__VA_ARGS__);                              \
    } while (0)

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_readout_add_workspace_bytes(int64_t N, int64_t B, int64_t F) {
    if (!readout_sizes_ok(N, B, F)) return -1;
    return ReadoutWorkspace::bytes(N, B, F, false);
}
extern "C" int64_t npi_readout_attention_workspace_bytes(int64_t N, int64_t B, int64_t F) {
    if (!readout_sizes_ok(N, B, F)) return -1;
    return ReadoutWorkspace::bytes(N, B, F, true);
}

extern "C" int npi_readout_add(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t N, int64_t B, int64_t F, float* out,
                               int64_t ldo, void* workspace, int64_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(readout_sizes_ok(N, B, F) && workspace_bytes >= 0, "npi_readout_add: bad size");
    NPI_REQUIRE(ldx >= F && ldo >= F, "npi_readout_add: a pitch below F");
    if (N == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(x && graph_ptr && out && workspace, "npi_readout_add: null pointer");
    NPI_REQUIRE((uintptr_t)workspace % 16 == 0, "npi_readout_add: workspace not 16-byte aligned");
    if (workspace_short("npi_readout_add", workspace_bytes, ReadoutWorkspace::bytes(N, B, F, false))) return NPI_ERR_ARG;
    ReadoutWorkspace ws;
    ws.carve(workspace, N, B, false);
    readout_map_kernel<<<1, RO_MAP_THREADS, 0, stream>>>(graph_ptr, (int)B, (int)N, ws.chunk_ptr);
    const int vec = pool_vec(F, {ldx}, {x});
    const dim3 grid((unsigned)ReadoutWorkspace::workgroups(N, B), (unsigned)ceil_div(F, RO_COLS));
    RO_DISPATCH(vec, readout_add_kernel, grid, RO_THREADS, x, ldx, graph_ptr, ws.chunk_ptr, (int)B, (int)F, (int)N, out, ldo, ws.pacc);
    if (N > RO_CHUNK)                                        // otherwise no graph has a second chunk
        readout_add_merge_kernel<<<dim3((unsigned)B, (unsigned)ceil_div(F, 64)), 64, 0, stream>>>(ws.chunk_ptr, (int)F, ws.pacc, out, ldo);
    return check_launch("npi_readout_add");
}

extern "C" int npi_readout_add_bwd(const float* dout, int64_t ldd, const int32_t* graph_ptr, int64_t N, int64_t B, int64_t F,
                                   float* dx, int64_t lddx, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(readout_sizes_ok(N, B, F), "npi_readout_add_bwd: bad size");
    NPI_REQUIRE(ldd >= F && lddx >= F, "npi_readout_add_bwd: a pitch below F");
    if (N == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(dout && graph_ptr && dx, "npi_readout_add_bwd: null pointer");
    const int vec = pool_vec(F, {ldd, lddx}, {dout, dx});
    const unsigned grid = (unsigned)ceil_div(N, 4 * RO_STRIP);
    RO_DISPATCH(vec, readout_add_bwd_kernel, grid, RO_THREADS, dout, ldd, graph_ptr, (int)B, (int)F, (int)N, dx, lddx);
    return check_launch("npi_readout_add_bwd");
}

extern "C" int npi_readout_attention(const float* gate, const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t N, int64_t B,
                                     int64_t F, float* out, int64_t ldo, float* m, float* s, void* workspace,
                                     int64_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(readout_sizes_ok(N, B, F) && workspace_bytes >= 0, "npi_readout_attention: bad size");
    NPI_REQUIRE(ldx >= F && ldo >= F, "npi_readout_attention: a pitch below F");
    if (N == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(gate && x && graph_ptr && out && m && s && workspace, "npi_readout_attention: null pointer");
    NPI_REQUIRE((uintptr_t)workspace % 16 == 0, "npi_readout_attention: workspace not 16-byte aligned");
    if (workspace_short("npi_readout_attention", workspace_bytes, ReadoutWorkspace::bytes(N, B, F, true))) return NPI_ERR_ARG;
    ReadoutWorkspace ws;
    ws.carve(workspace, N, B, true);
    readout_map_kernel<<<1, RO_MAP_THREADS, 0, stream>>>(graph_ptr, (int)B, (int)N, ws.chunk_ptr);
    const int vec = pool_vec(F, {ldx}, {x});
    const dim3 grid((unsigned)ReadoutWorkspace::workgroups(N, B), (unsigned)ceil_div(F, RO_COLS));
    RO_DISPATCH(vec, readout_att_kernel, grid, RO_THREADS, gate, x, ldx, graph_ptr, ws.chunk_ptr, (int)B, (int)F, (int)N, out, ldo, m, s,
                ws.pm, ws.ps, ws.pacc);
    if (N > RO_CHUNK)
        readout_att_merge_kernel<<<dim3((unsigned)B, (unsigned)ceil_div(F, 64)), 64, 0, stream>>>(ws.chunk_ptr, (int)F, ws.pm, ws.ps, ws.pacc,
                                                                                                  out, ldo, m, s);
    return check_launch("npi_readout_attention");
}

extern "C" int npi_readout_attention_bwd(const float* gate, const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t N, int64_t B,
                                         int64_t F, const float* out, int64_t ldo, const float* m, const float* s, const float* dout,
                                         int64_t ldd, float* dx, int64_t lddx, float* dgate, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(readout_sizes_ok(N, B, F), "npi_readout_attention_bwd: bad size");
    NPI_REQUIRE(ldx >= F && ldo >= F && ldd >= F && lddx >= F, "npi_readout_attention_bwd: a pitch below F");
    if (N == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(gate && x && graph_ptr && out && m && s && dout && dx && dgate, "npi_readout_attention_bwd: null pointer");
    const int vec = pool_vec(F, {ldx, ldo, ldd, lddx}, {x, out, dout, dx});
    const unsigned grid = (unsigned)ceil_div(N, 4 * RO_STRIP);
    RO_DISPATCH(vec, readout_att_bwd_kernel, grid, RO_THREADS, gate, x, ldx, graph_ptr, (int)B, (int)F, (int)N, out, ldo, m, s, dout, ldd,
                dx, lddx, dgate);
    return check_launch("npi_readout_attention_bwd");
}

extern "C" int npi_sort_pool_keys(const float* x, int64_t ldx, int64_t N, int64_t F, float* keys, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && F > 0 && F < NPI_INDEX_LIMIT, "npi_sort_pool_keys: bad size");
    NPI_REQUIRE(ldx >= F, "npi_sort_pool_keys: a pitch below F");
    if (N == 0) return NPI_OK;
    NPI_REQUIRE(x && keys, "npi_sort_pool_keys: null pointer");
    sort_pool_keys_kernel<<<(unsigned)ceil_div(N, 256), 256, 0, stream>>>(x, ldx, N, (int)F, keys);
    return check_launch("npi_sort_pool_keys");
}

static bool sort_pool_sizes_ok(int64_t N, int64_t B, int64_t F, int64_t k) {
    return count_ok(N) && count_ok(B) && F > 0 && F < NPI_INDEX_LIMIT && k > 0 && k < NPI_INDEX_LIMIT && k * F < NPI_INDEX_LIMIT &&
           B * k < NPI_INDEX_LIMIT;
}

extern "C" int npi_sort_pool_gather(const float* x, int64_t ldx, const int32_t* order, const int32_t* graph_ptr, int64_t N, int64_t B,
                                    int64_t F, int64_t k, float* out, int64_t ldo, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(B) && F > 0 && F < NPI_INDEX_LIMIT, "npi_sort_pool_gather: bad size");
    NPI_REQUIRE(k > 0, "npi_sort_pool_gather: k must be positive");
    NPI_REQUIRE(sort_pool_sizes_ok(N, B, F, k), "npi_sort_pool_gather: bad size (B k or k F beyond int32)");
    NPI_REQUIRE(ldx >= F && ldo >= k * F, "npi_sort_pool_gather: a pitch below F (out: below k F)");
    if (N == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(x && order && graph_ptr && out, "npi_sort_pool_gather: null pointer");
    const int vec = pool_vec(F, {ldx, ldo}, {x, out});
    const unsigned grid = (unsigned)ceil_div(B * k, 4);
    RO_DISPATCH(vec, sort_pool_gather_kernel, grid, RO_THREADS, x, ldx, order, graph_ptr, (int)N, (int)B, (int)F, (int)k, out, ldo);
    return check_launch("npi_sort_pool_gather");
}

extern "C" int npi_sort_pool_bwd(const float* dout, int64_t ldd, const int32_t* remap, const int32_t* graph_ptr, int64_t N, int64_t B,
                                 int64_t F, int64_t k, float* dx, int64_t lddx, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(B) && F > 0 && F < NPI_INDEX_LIMIT, "npi_sort_pool_bwd: bad size");
    NPI_REQUIRE(k > 0, "npi_sort_pool_bwd: k must be positive");
    NPI_REQUIRE(sort_pool_sizes_ok(N, B, F, k), "npi_sort_pool_bwd: bad size (B k or k F beyond int32)");
    NPI_REQUIRE(ldd >= k * F && lddx >= F, "npi_sort_pool_bwd: a pitch below F (dout: below k F)");
    if (N == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(dout && remap && graph_ptr && dx, "npi_sort_pool_bwd: null pointer");
    const int vec = pool_vec(F, {ldd, lddx}, {dout, dx});
    RO_DISPATCH(vec, sort_pool_bwd_kernel, (unsigned)ceil_div(N, 4), RO_THREADS, dout, ldd, remap, graph_ptr, (int)N, (int)B, (int)F, (int)k,
                dx, lddx);
    return check_launch("npi_sort_pool_bwd");
}
