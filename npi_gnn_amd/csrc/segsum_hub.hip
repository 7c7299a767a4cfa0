// The heaviest rows of a CSR side ("hubs", picked by npi_hub_plan at the end of this file) aggregated by STREAMING the source table once instead of
// gathering it: a hub whose row touches a sizeable fraction of all source rows re-reads the table row by row, and no cache holds a
// table of a million 1 KiB rows.  Here every source row is fetched once per launch and added into the accumulators of the hubs its
// mask word names (bit j of mask[r]: the side has an entry (hub j, r)).  f32, 256 columns, one table; deterministic: no float
// atomics, every hub row is summed in a fixed order (source rows ascending inside a slab, slabs in groups of ascending order).
//
//   hub_stream_kernel   one workgroup per slab of HUB_SLAB consecutive source rows.  Its 8 waves deal the hubs round-robin (wave w
//                       owns hubs w, w + 8, ...: contiguous ranges would hand the first wave the heaviest rows) and keep their
//                       partial sums in registers (16 hubs x 4 VGPRs).  Tiles of HUB_TILE rows go through LDS: every needed row is
//                       loaded once per workgroup (rows whose mask is zero are not loaded), the next tile's loads are in flight
//                       while the waves add the current one.  Which rows of a tile a hub takes is one scalar word (a ballot over
//                       the mask rows), so the tests are wave-uniform and a hub without entries in the tile costs one of them.
//   hub_finish_kernel   one workgroup per hub: 16 waves each add a contiguous group of slabs in slab order, wave 0 adds the 16
//                       group sums in order, applies the mean's divisor of the ORIGINAL row and writes the row and its
//                       power-of-two scale (pow2_scale_of) exactly as the main kernel's finish_row does.
#include "npi_common.h"

namespace npi {

constexpr int HUB_WAVES = 8;
constexpr int HUB_PER_WAVE = NPI_HUB_MAX / HUB_WAVES;
constexpr int HUB_THREADS = HUB_WAVES * WAVE;
constexpr int HUB_TILE = 32;                 // source rows per LDS tile (32 KiB); one mask row per lane of the lower half wave
constexpr int HUB_TILE_LOADS = HUB_TILE / HUB_WAVES;
constexpr int HUB_SLAB = 2048;               // source rows per workgroup: 489 slabs at a million rows, two resident per CU
constexpr int HUB_F = 256;
constexpr int HUB_MASK_WORDS = NPI_HUB_MAX / 32;
constexpr int FIN_WAVES = 16;
static_assert(HUB_PER_WAVE == 16 && HUB_MASK_WORDS == 4, "the wave's 16 mask bits are cut out of four 32-bit words");
static_assert(HUB_TILE == 32 && HUB_TILE % HUB_WAVES == 0, "one mask row per lane of a half wave");

// the 16 hubs of wave w as one word: hub (4 q + i) * 8 + w of mask word ... -- local hub k = 4 q + i sits in word q at bit 8 i + w,
// and lands at bit 8 i + q of the pattern
__device__ __forceinline__ uint32_t wave_pattern(const uint4& m, int w) {
    return ((m.x >> w) & 0x01010101u) | (((m.y >> w) & 0x01010101u) << 1) | (((m.z >> w) & 0x01010101u) << 2) |
           (((m.w >> w) & 0x01010101u) << 3);
}
constexpr uint32_t pattern_bit(int k) { return 1u << (8 * (k & 3) + (k >> 2)); }
// global hub index of wave w's local hub k
__device__ __forceinline__ int hub_of(int k, int w) { return ((k >> 2) * 32) + (k & 3) * 8 + w; }

// the loads of the tile at t0: its mask rows (lane l: row t0 + l), and this wave's share of the rows somebody needs
__device__ __forceinline__ void hub_prefetch(const float* __restrict__ x, int64_t ldx, const uint4* __restrict__ mask,
                                             const float* __restrict__ col_scale, int t0, int r1, int w, int lane,
                                             float4 (&pre)[HUB_TILE_LOADS], uint32_t& pat_n, uint32_t& need_n, float& cs_n) {
    const int row = t0 + lane;
    const bool valid = lane < HUB_TILE && row < r1;
    uint4 m = make_uint4(0u, 0u, 0u, 0u);
    if (valid) m = mask[row];
    cs_n = (valid && col_scale != nullptr) ? col_scale[row] : 1.f;
    pat_n = wave_pattern(m, w);
    need_n = (uint32_t)__ballot((m.x | m.y | m.z | m.w) != 0u);
#pragma unroll
    for (int t = 0; t < HUB_TILE_LOADS; ++t) {
        const int i = w + HUB_WAVES * t;
        if ((need_n >> i) & 1u)                              // (implies t0 + i < r1)
            pre[t] = *reinterpret_cast<const float4*>(x + (int64_t)(t0 + i) * ldx + lane * 4);
    }
}

__global__ void __launch_bounds__(HUB_THREADS, 4)
hub_stream_kernel(const float* __restrict__ x, int64_t ldx, const uint4* __restrict__ mask, const float* __restrict__ col_scale,
                  int n_cols, int H, float* __restrict__ partial) {
    __shared__ float4 tile[HUB_TILE][WAVE];
    const int lane = lane_id();
    const int w = uniform_i(threadIdx.x >> 6);
    const int r0 = blockIdx.x * HUB_SLAB;
    const int r1 = min(r0 + HUB_SLAB, n_cols);

    float4 acc[HUB_PER_WAVE];
#pragma unroll
    for (int k = 0; k < HUB_PER_WAVE; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 pre[HUB_TILE_LOADS];
#pragma unroll
    for (int t = 0; t < HUB_TILE_LOADS; ++t) pre[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t pat_n = 0, need_n = 0;
    float cs_n = 1.f;
    if (r0 < r1) hub_prefetch(x, ldx, mask, col_scale, r0, r1, w, lane, pre, pat_n, need_n, cs_n);
    for (int t0 = r0; t0 < r1; t0 += HUB_TILE) {
        __syncthreads();                                     // the previous tile has been added by every wave
#pragma unroll
        for (int t = 0; t < HUB_TILE_LOADS; ++t) {
            const int i = w + HUB_WAVES * t;
            if ((need_n >> i) & 1u) tile[i][lane] = pre[t];
        }
        const uint32_t pat = pat_n;
        const float cs = cs_n;
        __syncthreads();
        if (t0 + HUB_TILE < r1) hub_prefetch(x, ldx, mask, col_scale, t0 + HUB_TILE, r1, w, lane, pre, pat_n, need_n, cs_n);
        // hub by hub: the rows of this tile with an entry of hub k as one scalar word (most are zero: one test per hub and tile,
        // not one per hub and row), walked in ascending row order
#pragma unroll
        for (int k = 0; k < HUB_PER_WAVE; ++k) {
            uint32_t m = (uint32_t)__ballot((pat & pattern_bit(k)) != 0u);
            while (m != 0u) {
                const int i = uniform_i(__builtin_ctz(m));
                m &= m - 1u;
                const float s = bcast_f(cs, i);
                const float4 v = tile[i][lane];
                acc[k].x = fmaf(v.x, s, acc[k].x);
                acc[k].y = fmaf(v.y, s, acc[k].y);
                acc[k].z = fmaf(v.z, s, acc[k].z);
                acc[k].w = fmaf(v.w, s, acc[k].w);
            }
        }
    }
    float4* __restrict__ dst = reinterpret_cast<float4*>(partial) + (int64_t)blockIdx.x * NPI_HUB_MAX * WAVE;
#pragma unroll
    for (int k = 0; k < HUB_PER_WAVE; ++k) {
        const int j = hub_of(k, w);
        if (j < H) dst[(int64_t)j * WAVE + lane] = acc[k];
    }
}

__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__global__ void __launch_bounds__(FIN_WAVES * WAVE)
hub_finish_kernel(const float* __restrict__ partial, int n_slabs, const int32_t* __restrict__ hub_rows, const int32_t* __restrict__ rowptr,
                  int mean, float* __restrict__ out, int64_t ldo, float* __restrict__ scale_out) {
    __shared__ float4 part[FIN_WAVES][WAVE];
    const int lane = lane_id();
    const int w = uniform_i(threadIdx.x >> 6);
    const int j = blockIdx.x;
    const int chunk = (n_slabs + FIN_WAVES - 1) / FIN_WAVES;
    const int s0 = w * chunk, s1 = min(s0 + chunk, n_slabs);
    const float4* __restrict__ src = reinterpret_cast<const float4*>(partial) + (int64_t)j * WAVE + lane;
    const int64_t step = (int64_t)NPI_HUB_MAX * WAVE;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = s0;
    for (; s + 8 <= s1; s += 8) {                            // eight loads in flight, added in slab order
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(s + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) a = add4(a, v[u]);
    }
    for (; s < s1; ++s) a = add4(a, src[(int64_t)s * step]);
    part[w][lane] = a;
    __syncthreads();
    if (w != 0) return;
    a = part[0][lane];
#pragma unroll
    for (int g = 1; g < FIN_WAVES; ++g) a = add4(a, part[g][lane]);
    const int r = hub_rows[j];
    float sc = 1.f;
    if (mean) sc = 1.f / (float)max(rowptr[r + 1] - rowptr[r], 1);
    const float4 t = make_float4(fmaf(a.x, sc, 0.f), fmaf(a.y, sc, 0.f), fmaf(a.z, sc, 0.f), fmaf(a.w, sc, 0.f));
    *reinterpret_cast<float4*>(out + (int64_t)r * ldo + lane * 4) = t;
    if (scale_out != nullptr) {
        float m = fmaxf(fmaxf(fabsf(t.x), fabsf(t.y)), fmaxf(fabsf(t.z), fabsf(t.w)));
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) scale_out[r] = pow2_scale_of(m);
    }
}

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_segsum_hub_slabs(int64_t n_cols) { return n_cols <= 0 ? 0 : ceil_div(n_cols, HUB_SLAB); }

extern "C" int64_t npi_segsum_hub_partial_elems(int64_t n_cols) {
    return n_cols < 0 ? -1 : (npi_segsum_hub_slabs(n_cols) > 0 ? npi_segsum_hub_slabs(n_cols) : 1) * NPI_HUB_MAX * HUB_F;
}

extern "C" int npi_segsum_hub(const int32_t* hub_rows, int64_t H, const uint32_t* mask, const int32_t* rowptr, int64_t N, int64_t n_cols,
                              const float* col_scale, const float* x, int64_t ldx, float* out, int64_t ldo, int64_t F, int mean,
                              float* partial, float* row_scales_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(H >= 0 && H <= NPI_HUB_MAX, "npi_segsum_hub: H must be in [0, NPI_HUB_MAX]");
    NPI_REQUIRE(F == HUB_F, "npi_segsum_hub: f32 rows of 256 columns only");
    NPI_REQUIRE(N >= 0 && n_cols >= 0 && n_cols < ((int64_t)1 << 31) - HUB_SLAB, "npi_segsum_hub: bad size");
    if (H == 0) return NPI_OK;
    NPI_REQUIRE(hub_rows && mask && rowptr && x && out && partial, "npi_segsum_hub: null pointer");
    NPI_REQUIRE(ldx >= F && ldo >= F && ldx % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                    ((uintptr_t)partial % 16) == 0 && ((uintptr_t)mask % 16) == 0,
                "npi_segsum_hub: rows and masks must be 16-byte aligned");
    const int64_t n_slabs = npi_segsum_hub_slabs(n_cols);
    if (n_slabs > 0) {
        hipLaunchKernelGGL(hub_stream_kernel, dim3((unsigned)n_slabs), dim3(HUB_THREADS), 0, stream, x, ldx,
                           reinterpret_cast<const uint4*>(mask), col_scale, (int)n_cols, (int)H, partial);
        int rc = check_launch("npi_segsum_hub(stream)");
        if (rc != NPI_OK) return rc;
    }
    hipLaunchKernelGGL(hub_finish_kernel, dim3((unsigned)H), dim3(FIN_WAVES * WAVE), 0, stream, partial, (int)n_slabs, hub_rows, rowptr,
                       mean, out, ldo, row_scales_out);
    return check_launch("npi_segsum_hub(finish)");
}

// ---- hub plan: the heaviest rows of a side, for the streaming aggregation above ---------------------------------------------------
// npi_hub_plan picks the up to h_max rows with the most entries among those with at least min_degree entries (ties: the lower row
// first), writes bit j of mask[c] for every entry (hub j, c), drops hubs that hold a column twice (a bit cannot count twice) and
// leaves the plan EMPTY (info[0] = 0) unless the remaining hubs' entries add up to min_entries.  npi_hub_light_side writes the same
// side without the hub rows' entries.  All of it once per graph and side; integer atomics only.
namespace npi {

constexpr int HUB_CAND_CAP = 4096;           // rows with >= min_degree entries the selection looks at (more: the plan is empty)
constexpr int HUB_WS_CNT = 0, HUB_WS_IDENT = 1, HUB_WS_PRELIM = 8, HUB_WS_BAD = HUB_WS_PRELIM + NPI_HUB_MAX,
              HUB_WS_REMAP = HUB_WS_BAD + NPI_HUB_MAX, HUB_WS_CAND = HUB_WS_REMAP + NPI_HUB_MAX, HUB_WS_ELEMS = HUB_WS_CAND + HUB_CAND_CAP;
constexpr int HUB_WORDS = HUB_MASK_WORDS;

__global__ void hub_candidates_kernel(const int32_t* __restrict__ rowptr, int64_t N, int32_t min_degree, int32_t* __restrict__ ws) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N || rowptr[r + 1] - rowptr[r] < min_degree) return;
    const int i = atomicAdd(&ws[HUB_WS_CNT], 1);
    if (i < HUB_CAND_CAP) ws[HUB_WS_CAND + i] = (int32_t)r;
}

// rank of every candidate by (degree descending, row ascending); the first h_max are the preliminary hubs, in that order
__global__ void __launch_bounds__(1024)
hub_select_kernel(const int32_t* __restrict__ rowptr, int h_max, int32_t* __restrict__ ws, int32_t* __restrict__ info) {
    __shared__ int32_t rows[HUB_CAND_CAP], degs[HUB_CAND_CAP];
    const int seen = ws[HUB_WS_CNT];
    const int n = seen > HUB_CAND_CAP ? 0 : seen;
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
        const int32_t r = ws[HUB_WS_CAND + c];
        rows[c] = r;
        degs[c] = rowptr[r + 1] - rowptr[r];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
        const int32_t r = rows[c], d = degs[c];
        int rank = 0;
        for (int o = 0; o < n; ++o) rank += (degs[o] > d || (degs[o] == d && rows[o] < r)) ? 1 : 0;
        if (rank < h_max) ws[HUB_WS_PRELIM + rank] = r;
    }
    if (threadIdx.x == 0) {
        info[2] = seen;
        info[3] = n < h_max ? n : h_max;
    }
    if (threadIdx.x < NPI_HUB_MAX) ws[HUB_WS_BAD + threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256)
hub_mask_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_cols, int32_t* __restrict__ ws,
                const int32_t* __restrict__ info, uint32_t* __restrict__ mask) {
    const int j = blockIdx.y;
    if (j >= info[3]) return;
    const int32_t r = ws[HUB_WS_PRELIM + j];
    const uint32_t bit = 1u << (j & 31);
    const int64_t p1 = rowptr[r + 1];
    for (int64_t p = (int64_t)rowptr[r] + blockIdx.x * 256 + threadIdx.x; p < p1; p += (int64_t)gridDim.x * 256) {
        const int32_t c = col[p];
        if (c < 0 || c >= n_cols) { ws[HUB_WS_BAD + j] = 1; continue; }
        const uint32_t old = atomicOr(&mask[(int64_t)c * HUB_WORDS + (j >> 5)], bit);
        if (old & bit) ws[HUB_WS_BAD + j] = 1;                 // the column a second time: this row cannot be a hub
    }
}

__global__ void hub_finalize_kernel(const int32_t* __restrict__ rowptr, int64_t min_entries, int32_t* __restrict__ ws,
                                    int32_t* __restrict__ info, int32_t* __restrict__ hub_rows) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int h0 = info[3];
    int h = 0;
    int64_t total = 0;
    for (int j = 0; j < NPI_HUB_MAX; ++j) {
        int m = -1;
        if (j < h0 && ws[HUB_WS_BAD + j] == 0) {
            const int32_t r = ws[HUB_WS_PRELIM + j];
            hub_rows[h] = r;
            total += rowptr[r + 1] - rowptr[r];
            m = h++;
        }
        ws[HUB_WS_REMAP + j] = m;
    }
    if (total < min_entries || total >= ((int64_t)1 << 31)) h = 0;
    for (int j = h; j < NPI_HUB_MAX; ++j) hub_rows[j] = -1;
    ws[HUB_WS_IDENT] = (h == h0) ? 1 : 0;
    info[0] = h;
    info[1] = h > 0 ? (int32_t)total : 0;
}

// the bits of the dropped hubs leave the masks, the others move down (only when a hub was dropped)
__global__ void hub_mask_remap_kernel(int64_t n_cols, const int32_t* __restrict__ ws, const int32_t* __restrict__ info,
                                      uint32_t* __restrict__ mask) {
    if (ws[HUB_WS_IDENT] != 0 || info[0] == 0) return;
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    uint32_t out[HUB_WORDS] = {};
    bool any = false;
    for (int q = 0; q < HUB_WORDS; ++q) {
        uint32_t m = mask[c * HUB_WORDS + q];
        any |= m != 0u;
        while (m != 0u) {
            const int b = __builtin_ctz(m);
            m &= m - 1u;
            const int nj = ws[HUB_WS_REMAP + q * 32 + b];
            if (nj >= 0) out[nj >> 5] |= 1u << (nj & 31);
        }
    }
    if (!any) return;
    for (int q = 0; q < HUB_WORDS; ++q) mask[c * HUB_WORDS + q] = out[q];
}

__global__ void __launch_bounds__(256)
hub_light_rowptr_kernel(const int32_t* __restrict__ rowptr, int64_t N, const int32_t* __restrict__ hub_rows, int H,
                        int32_t* __restrict__ rowptr_l) {
    __shared__ int32_t hr[NPI_HUB_MAX], hd[NPI_HUB_MAX];
    if (threadIdx.x < H) {
        const int32_t r = hub_rows[threadIdx.x];
        hr[threadIdx.x] = r;
        hd[threadIdx.x] = rowptr[r + 1] - rowptr[r];
    }
    __syncthreads();
    int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > N) return;
    int32_t removed = 0;
    for (int j = 0; j < H; ++j) removed += (hr[j] < r) ? hd[j] : 0;
    rowptr_l[r] = rowptr[r] - removed;
}

__global__ void hub_light_entries_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                         const int32_t* __restrict__ eid, const int32_t* __restrict__ rowidx, int64_t N, int64_t nnz_max,
                                         const int32_t* __restrict__ rowptr_l, int64_t nnz_max_l, int32_t* __restrict__ col_l,
                                         int32_t* __restrict__ eid_l, int32_t* __restrict__ rowidx_l) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz_max || p >= rowptr[N]) return;
    const int32_t r = rowidx[p];
    if (r < 0 || r >= N || rowptr_l[r + 1] == rowptr_l[r]) return;      // an entry of a hub row
    const int64_t q = p - (rowptr[r] - rowptr_l[r]);
    if (q < 0 || q >= nnz_max_l) return;
    col_l[q] = col[p];
    eid_l[q] = eid[p];
    rowidx_l[q] = r;
}

}  // namespace npi

extern "C" int64_t npi_hub_plan_workspace_elems(void) { return HUB_WS_ELEMS; }

extern "C" int npi_hub_plan(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t n_cols, int64_t nnz_max, int64_t h_max,
                            int64_t min_degree, int64_t min_entries, int32_t* hub_rows, uint32_t* mask, int32_t* info,
                            int32_t* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(N > 0 && n_cols > 0 && nnz_max > 0 && N < ((int64_t)1 << 31) && n_cols < ((int64_t)1 << 31), "npi_hub_plan: bad size");
    NPI_REQUIRE(h_max >= 1 && h_max <= NPI_HUB_MAX, "npi_hub_plan: h_max must be in [1, NPI_HUB_MAX]");
    NPI_REQUIRE(min_degree >= 1 && min_degree < ((int64_t)1 << 31) && min_entries >= 0, "npi_hub_plan: bad threshold");
    NPI_REQUIRE(rowptr && col && hub_rows && mask && info && workspace, "npi_hub_plan: null pointer");
    (void)hipMemsetAsync(workspace, 0, HUB_WS_CAND * sizeof(int32_t), stream);
    (void)hipMemsetAsync(info, 0, 4 * sizeof(int32_t), stream);
    (void)hipMemsetAsync(mask, 0, (size_t)n_cols * HUB_WORDS * sizeof(uint32_t), stream);
    hub_candidates_kernel<<<(unsigned)ceil_div(N, 256), 256, 0, stream>>>(rowptr, N, (int32_t)min_degree, workspace);
    hub_select_kernel<<<1, 1024, 0, stream>>>(rowptr, (int)h_max, workspace, info);
    hub_mask_kernel<<<dim3(64, NPI_HUB_MAX), 256, 0, stream>>>(rowptr, col, n_cols, workspace, info, mask);
    hub_finalize_kernel<<<1, 64, 0, stream>>>(rowptr, min_entries, workspace, info, hub_rows);
    hub_mask_remap_kernel<<<(unsigned)ceil_div(n_cols, 256), 256, 0, stream>>>(n_cols, workspace, info, mask);
    return check_launch("npi_hub_plan");
}

extern "C" int npi_hub_light_side(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t N,
                                  int64_t nnz_max, const int32_t* hub_rows, int64_t H, int64_t nnz_max_light, int64_t item_edges,
                                  int32_t* rowptr_l, int32_t* col_l, int32_t* eid_l, int32_t* rowidx_l, int32_t* item_row_l,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(N > 0 && nnz_max > 0 && nnz_max_light >= 0 && nnz_max_light <= nnz_max, "npi_hub_light_side: bad size");
    NPI_REQUIRE(H >= 1 && H <= NPI_HUB_MAX, "npi_hub_light_side: H must be in [1, NPI_HUB_MAX]");
    NPI_REQUIRE(item_edges_ok(item_edges), "npi_hub_light_side: item_edges must be 64 or NPI_ITEM_EDGES");
    NPI_REQUIRE(rowptr && col && eid && rowidx && hub_rows && rowptr_l && col_l && eid_l && rowidx_l && item_row_l,
                "npi_hub_light_side: null pointer");
    hub_light_rowptr_kernel<<<(unsigned)ceil_div(N + 1, 256), 256, 0, stream>>>(rowptr, N, hub_rows, (int)H, rowptr_l);
    hub_light_entries_kernel<<<(unsigned)ceil_div(nnz_max, 256), 256, 0, stream>>>(rowptr, col, eid, rowidx, N, nnz_max, rowptr_l,
                                                                                 nnz_max_light, col_l, eid_l, rowidx_l);
    write_item_rows(rowptr_l, N, nnz_max_light, item_edges, item_row_l, stream);
    return check_launch("npi_hub_light_side");
}
