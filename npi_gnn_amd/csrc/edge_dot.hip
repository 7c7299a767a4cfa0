// Gradients w.r.t. edge_weight of the aggregate-and-project layers (SAGEConv, GCNConv): what autograd computes for
// `edge_weight.view(-1, 1) * x_j` in front of a scatter -- one dot product per entry of the CSR,
//   g[p] = row_scale[i] * <a[i, :], b[col[p], :]>        (i = the row of entry p; a = dAgg or dOut, b = x or xW)
// -- and, for GCNConv(normalize=True), the chain through norm = deg^-1/2[j] w deg^-1/2[i] (npi_gcn_norm_bwd).
// The general form of gat.hip's by-target SDDMM (gat_edge_grad_kernel), without the softmax chain behind it.
// No float atomics: every entry is summed by one wavefront in a fixed order, every output element has one writer.
#include "dot_lanes.h"

namespace npi {

// One wavefront per item of `item_edges` entries (64 or 256, picked per call by the rule of npi_item_edges), walked in blocks of
// 64: columns, rows and edge ids of a block are fetched lane-parallel, the entries go eight at a time -- eight gathered rows of b
// in flight per lane, the eight partial dot products reduce-SCATTERED over the wave (10 cross-lane steps for 8 entries instead of
// 48) -- and the 64 results are parked in LDS, so that scaling and the (scattered) stores are lane-parallel again.
//   VEC: 16-byte lanes (F % 4 == 0, 16-byte aligned rows), a chunk is 256 columns; otherwise one float per lane, 64 columns.
//   ONE: the row fits one chunk -- its a-row stays in registers and is reloaded only when the row changes.  Wider rows walk the
//        chunks inside the group of eight and read a's chunk with each entry (from cache: consecutive entries share the row).
template <bool VEC, bool ONE>
__global__ void __launch_bounds__(256)
edge_dot_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ rowidx,
                const int32_t* __restrict__ eid, int N, int n_cols, int n_edges, int n_items, int item_edges,
                const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int F,
                const float* __restrict__ row_scale, const float* __restrict__ mul, float* __restrict__ g_entry,
                float* __restrict__ gm_entry, float* __restrict__ d_edge, float* __restrict__ d_loop) {
    using L = Lanes<VEC>;
    using T = typename L::T;
    constexpr int CW = WAVE * L::W;
    const int lane = lane_id();
    const int item = uniform_i(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (item >= n_items) return;
    const int nnz = rowptr[N];
    const int64_t k0 = (int64_t)item * item_edges;
    if (k0 >= nnz) return;
    const int k1 = (int)min(k0 + item_edges, (int64_t)nnz);
    __shared__ float pbuf[4][WAVE];
    float* __restrict__ pb = pbuf[threadIdx.x >> 6];
    const int e_of_lane = group_of_lane(lane);
    T ar = L::zero();
    int cur = -1;
    for (int kb = (int)k0; kb < k1; kb += WAVE) {
        const int nb = min(WAVE, k1 - kb);
        int cv = (lane < nb) ? col[kb + lane] : 0;
        int rv = (lane < nb) ? rowidx[kb + lane] : 0;
        // an index outside its table contributes nothing and is never dereferenced (a CSR from npi_csr_build has none)
        const bool inside = (unsigned)cv < (unsigned)n_cols && (unsigned)rv < (unsigned)N;
        if (!inside) { cv = 0; rv = 0; }
        for (int j = 0; j < nb; j += 8) {
            float p[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = 0.f;
            if (ONE) {
                const int off = lane * L::W;
                const bool act = off < F;
                T hv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int cu = bcast_i(cv, min(j + u, nb - 1));
                    hv[u] = act ? L::load(b + (int64_t)cu * ldb + off) : L::zero();
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (j + u < nb) {                                  // wave-uniform
                        const int i = bcast_i(rv, j + u);
                        if (i != cur) {
                            cur = i;
                            ar = act ? L::load(a + (int64_t)i * lda + off) : L::zero();
                        }
                        p[u] = L::dot(ar, hv[u], 0.f);
                    }
                }
            } else {
                for (int c0 = 0; c0 < F; c0 += CW) {
                    const int off = c0 + lane * L::W;
                    const bool act = off < F;
                    T hv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int cu = bcast_i(cv, min(j + u, nb - 1));
                        hv[u] = act ? L::load(b + (int64_t)cu * ldb + off) : L::zero();
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        if (j + u < nb) {
                            const int i = bcast_i(rv, j + u);
                            const T av = act ? L::load(a + (int64_t)i * lda + off) : L::zero();
                            p[u] = L::dot(av, hv[u], p[u]);
                        }
                    }
                }
            }
            const float y = reduce_scatter8(p, lane);          // the eight lanes of group e_of_lane hold entry j + e_of_lane
            if ((lane & 7) == 0 && j + e_of_lane < nb) pb[j + e_of_lane] = y;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < nb) {
            const int p = kb + lane;
            float g = inside ? pb[lane] : 0.f;
            if (row_scale) g *= row_scale[rv];
            if (g_entry) g_entry[p] = g;
            if (gm_entry) gm_entry[p] = g * mul[p];
            if (d_edge || d_loop) {
                const int e = eid[p];
                if (e >= 0) {
                    if (d_edge && e < n_edges) d_edge[e] = g;
                } else if (d_loop && inside) {
                    d_loop[rv] = g;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ float inv_sqrt_or_zero_(float d) { return d > 0.f ? 1.0f / sqrtf(d) : 0.f; }

// d w_p = g_p dis[j] dis[i] - s[j] / (2 deg[j])   (i = row = target, j = column = source of by-target entry p; dis = deg^-1/2,
// 0 where deg <= 0 -- then both terms are 0);  s = s_a + s_b: the row sums of g norm over both orientations
__global__ void gcn_norm_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                    const int32_t* __restrict__ rowidx, const int32_t* __restrict__ eid, int N, int64_t nnz_max,
                                    int n_edges, const float* __restrict__ g_entry, const float* __restrict__ deg,
                                    const float* __restrict__ s_a, const float* __restrict__ s_b, float* __restrict__ d_edge,
                                    float* __restrict__ d_loop) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz_max || p >= rowptr[N]) return;
    const int i = rowidx[p], j = col[p];
    if ((unsigned)i >= (unsigned)N || (unsigned)j >= (unsigned)N) return;
    const float di = deg[i], dj = deg[j];
    const float s = s_a[j] + (s_b ? s_b[j] : 0.f);
    const float v = g_entry[p] * inv_sqrt_or_zero_(dj) * inv_sqrt_or_zero_(di) - (dj > 0.f ? s / (2.f * dj) : 0.f);
    const int e = eid[p];
    if (e >= 0) {
        if (d_edge && e < n_edges) d_edge[e] = v;
    } else if (d_loop) {
        d_loop[i] = v;
    }
}

}  // namespace npi

using namespace npi;

extern "C" int npi_edge_dot(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* eid, int64_t N,
                            int64_t n_cols, int64_t nnz_max, int64_t n_edges, const float* a, int64_t lda, const float* b,
                            int64_t ldb, int64_t F, const float* row_scale, const float* mul, float* g_entry, float* gm_entry,
                            float* d_edge, float* d_loop, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(N >= 0 && n_cols >= 0 && nnz_max >= 0 && n_edges >= 0 && F > 0 && N < 0x7fffffff && n_cols < 0x7fffffff &&
                    nnz_max < 0x7fffffff && n_edges < 0x7fffffff && F < 0x7fffffff && lda >= F && ldb >= F,
                "npi_edge_dot: bad size");
    NPI_REQUIRE((gm_entry == nullptr) == (mul == nullptr), "npi_edge_dot: the per-entry multiplier and its output come together");
    if (nnz_max == 0 || N == 0 || n_cols == 0) return NPI_OK;
    NPI_REQUIRE(rowptr && col && rowidx && a && b && (g_entry || gm_entry || d_edge || d_loop), "npi_edge_dot: null pointer");
    NPI_REQUIRE(eid || !(d_edge || d_loop), "npi_edge_dot: null pointer (eid)");
    const int item = item_edges_for(nnz_max);
    const int64_t n_items = num_items_of(nnz_max, item);
    const unsigned grid = (unsigned)ceil_div(n_items, 4);
    const bool vec = rows16(a, lda, F) && rows16(b, ldb, F);
    const bool one = F <= (vec ? 4 * WAVE : WAVE);
#define NPI_EDGE_DOT(V, O)                                                                                                      \
    edge_dot_kernel<V, O><<<grid, 256, 0, stream>>>(rowptr, col, rowidx, eid, (int)N, (int)n_cols, (int)n_edges, (int)n_items, \
                                                    item, a, lda, b, ldb, (int)F, row_scale, mul, g_entry, gm_entry, d_edge,   \
                                                    d_loop)
    if (vec) { if (one) NPI_EDGE_DOT(true, true); else NPI_EDGE_DOT(true, false); }
    else     { if (one) NPI_EDGE_DOT(false, true); else NPI_EDGE_DOT(false, false); }
#undef NPI_EDGE_DOT
    return check_launch("npi_edge_dot");
}

extern "C" int npi_gcn_norm_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* eid, int64_t N,
                                int64_t nnz_max, int64_t n_edges, const float* g_entry, const float* deg, const float* s_a,
                                const float* s_b, float* d_edge, float* d_loop, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(N >= 0 && nnz_max >= 0 && n_edges >= 0 && N < 0x7fffffff && n_edges < 0x7fffffff, "npi_gcn_norm_bwd: bad size");
    if (nnz_max == 0 || N == 0) return NPI_OK;
    NPI_REQUIRE(rowptr && col && rowidx && eid && g_entry && deg && s_a && (d_edge || d_loop), "npi_gcn_norm_bwd: null pointer");
    gcn_norm_bwd_kernel<<<(unsigned)ceil_div(nnz_max, 256), 256, 0, stream>>>(rowptr, col, rowidx, eid, (int)N, nnz_max,
                                                                              (int)n_edges, g_entry, deg, s_a, s_b, d_edge, d_loop);
    return check_launch("npi_gcn_norm_bwd");
}
