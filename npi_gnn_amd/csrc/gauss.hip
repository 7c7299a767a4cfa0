// The variational half of PyG 1.4.2 `torch_geometric/nn/models/autoencoder.py` (include/npi_gnn.h: npi_gauss_*): VGAE's
//     z  = mu + randn_like(logvar) * exp(0.5 * logvar)                                   reparametrize
//     kl = -0.5 * mean(sum(1 + logvar - mu**2 - logvar.exp(), dim=1))                    kl_loss, logvar clamped at MAX_LOGVAR
// in ONE launch forward and ONE backward.  The noise is Rule N (gauss.h), recomputed in the backward: no eps, no sigma array.
// A lane owns four columns of a row -- two words of the rule -- as one 16-byte piece when the rows allow it (rows16), else as four
// guarded floats; the lane -> element map is the same either way.  The KL sum follows pair_score.hip's scheme: f32 terms, one fp64
// partial per FIXED tile of NPI_GAUSS_TILE element slots (whatever the grid), a second one-workgroup launch that adds the partials
// in a fixed order.  No float atomics; every output element has one writer.
#include "dot_lanes.h"
#include "gauss.h"

namespace npi {

// the tables one launch walks: N rows of F columns cut into Q = ceil(F / 4) groups of four; group g = row Q + j is column 4 j of row
struct GaussShape {
    int F, Q;
    int64_t n_quads, n_tiles;
    uint64_t root;
    int table;
};

// (row, first column) of the k-th group this thread takes of the tile that starts at group q0 = r0 Q + j0; false: past the end
__device__ __forceinline__ bool gauss_quad(const GaussShape& s, int64_t q0, int64_t r0, int j0, int k, int& row, int& c0) {
    const int off = k * GAUSS_THREADS + (int)threadIdx.x;
    if (q0 + off >= s.n_quads) return false;
    const uint32_t jj = (uint32_t)j0 + (uint32_t)off;          // < Q + 1024: 32-bit division per group, the 64-bit one per tile
    const uint32_t dr = jj / (uint32_t)s.Q;
    row = (int)(r0 + dr);
    c0 = (int)(jj - dr * (uint32_t)s.Q) * 4;
    return true;
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int c0, int F, float (&v)[4]) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(p + c0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = c0 + u < F ? p[c0 + u] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int c0, int F, const float (&v)[4]) {
    if (VEC) {
        *reinterpret_cast<float4*>(p + c0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c0 + u < F) p[c0 + u] = v[u];
    }
}
// eps of columns c0 .. c0 + 3 of `row` (the second word only when one of its columns exists)
template <bool VEC>
__device__ __forceinline__ void noise4(uint64_t root_t, int table, int row, int c0, int F, float (&e)[4]) {
    const uint64_t stream = gauss_stream(root_t, table, row);
    gauss_pair(stream, c0 >> 1, e[0], e[1]);
    e[2] = e[3] = 0.f;
    if (VEC || c0 + 2 < F) gauss_pair(stream, (c0 >> 1) + 1, e[2], e[3]);
}

// sum of `acc` over the workgroup in a fixed order (a butterfly per wave, the four waves in order), valid in thread 0
__device__ __forceinline__ double gauss_block_sum(double acc, double* wsum) {
    acc = wave_sum(acc);
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

//   SAMPLE: z = fmaf(eps, expf(0.5 lv), mu);   KL: partials[tile] = sum of the f32 terms 1 + lv - mu^2 - expf(lv) of the tile, in fp64
template <bool VEC, bool SAMPLE, bool KL>
__global__ void __launch_bounds__(GAUSS_THREADS)
gauss_sample_kl_kernel(GaussShape s, const int64_t* __restrict__ tick, const float* __restrict__ mu, int64_t ld_mu,
                       const float* __restrict__ logvar, int64_t ld_lv, float max_logvar, float* __restrict__ z, int64_t ld_z,
                       double* __restrict__ partials) {
    __shared__ double wsum[GAUSS_THREADS / WAVE];
    const uint64_t root_t = gauss_root_t(s.root, tick);
    for (int64_t tile = blockIdx.x; tile < s.n_tiles; tile += gridDim.x) {
        const int64_t q0 = tile * GAUSS_TILE_QUADS, r0 = q0 / s.Q;
        const int j0 = (int)(q0 - r0 * s.Q);
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < GAUSS_QUADS_PER_THREAD; ++k) {
            int row, c0;
            if (!gauss_quad(s, q0, r0, j0, k, row, c0)) continue;
            float m[4], l[4], e[4], out[4], t[4];
            load4<VEC>(mu + (int64_t)row * ld_mu, c0, s.F, m);
            load4<VEC>(logvar + (int64_t)row * ld_lv, c0, s.F, l);
            if (SAMPLE) noise4<VEC>(root_t, s.table, row, c0, s.F, e);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float lv = fminf(l[u], max_logvar);
                if (SAMPLE) out[u] = fmaf(e[u], expf(0.5f * lv), m[u]);
                if (KL) t[u] = (VEC || c0 + u < s.F) ? fmaf(-m[u], m[u], 1.0f + lv) - expf(lv) : 0.f;
            }
            if (SAMPLE) store4<VEC>(z + (int64_t)row * ld_z, c0, s.F, out);
            if (KL) acc += (((double)t[0] + (double)t[1]) + (double)t[2]) + (double)t[3];
        }
        if (KL) {
            const double total = gauss_block_sum(acc, wsum);
            if (threadIdx.x == 0) partials[tile] = total;
            __syncthreads();                                   // wsum is written again in the next tile
        }
    }
}

// kl[0] = scale * sum of partials[0 .. n) in a fixed order: thread t adds t, t + 256, ... in fp64, then a fixed tree
__global__ void __launch_bounds__(GAUSS_THREADS)
gauss_kl_sum_kernel(const double* __restrict__ partials, int64_t n, double scale, float* __restrict__ kl) {
    __shared__ double acc[GAUSS_THREADS];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += GAUSS_THREADS) v += partials[i];
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int st = GAUSS_THREADS / 2; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) acc[threadIdx.x] += acc[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) kl[0] = (float)(acc[0] * scale);
}

//   d_mu = g_z + c mu,  d_logvar = [logvar <= max_logvar] (g_z 0.5 eps sigma - 0.5 c (1 - exp(lv))),  c = g_kl[0] / n_total;
//   GZ / GKL: which upstream gradients exist (an absent one contributes 0).  eps is Rule N again: what the forward drew.
template <bool VEC, bool GZ, bool GKL>
__global__ void __launch_bounds__(GAUSS_THREADS)
gauss_sample_kl_bwd_kernel(GaussShape s, const int64_t* __restrict__ tick, const float* __restrict__ mu, int64_t ld_mu,
                           const float* __restrict__ logvar, int64_t ld_lv, float max_logvar, float inv_n,
                           const float* __restrict__ g_z, int64_t ld_gz, const float* __restrict__ g_kl, float* __restrict__ d_mu,
                           int64_t ld_dmu, float* __restrict__ d_logvar, int64_t ld_dlv) {
    const uint64_t root_t = gauss_root_t(s.root, tick);
    const float c = GKL ? g_kl[0] * inv_n : 0.f;
    for (int64_t tile = blockIdx.x; tile < s.n_tiles; tile += gridDim.x) {
        const int64_t q0 = tile * GAUSS_TILE_QUADS, r0 = q0 / s.Q;
        const int j0 = (int)(q0 - r0 * s.Q);
#pragma unroll
        for (int k = 0; k < GAUSS_QUADS_PER_THREAD; ++k) {
            int row, c0;
            if (!gauss_quad(s, q0, r0, j0, k, row, c0)) continue;
            float g[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
            if (GZ) load4<VEC>(g_z + (int64_t)row * ld_gz, c0, s.F, g);
            if (d_mu) {
                if (GKL) {
                    float m[4];
                    load4<VEC>(mu + (int64_t)row * ld_mu, c0, s.F, m);
#pragma unroll
                    for (int u = 0; u < 4; ++u) out[u] = fmaf(c, m[u], g[u]);
                    store4<VEC>(d_mu + (int64_t)row * ld_dmu, c0, s.F, out);
                } else {
                    store4<VEC>(d_mu + (int64_t)row * ld_dmu, c0, s.F, g);
                }
            }
            if (d_logvar) {
                float l[4], e[4] = {0.f, 0.f, 0.f, 0.f};
                load4<VEC>(logvar + (int64_t)row * ld_lv, c0, s.F, l);
                if (GZ) noise4<VEC>(root_t, s.table, row, c0, s.F, e);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float lv = fminf(l[u], max_logvar);
                    const float a = GZ ? (0.5f * g[u]) * (e[u] * expf(0.5f * lv)) : 0.f;
                    const float d = GKL ? fmaf(-0.5f * c, 1.0f - expf(lv), a) : a;
                    out[u] = l[u] <= max_logvar ? d : 0.f;
                }
                store4<VEC>(d_logvar + (int64_t)row * ld_dlv, c0, s.F, out);
            }
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(GAUSS_THREADS)
gauss_noise_kernel(GaussShape s, const int64_t* __restrict__ tick, float* __restrict__ eps, int64_t ld) {
    const uint64_t root_t = gauss_root_t(s.root, tick);
    for (int64_t tile = blockIdx.x; tile < s.n_tiles; tile += gridDim.x) {
        const int64_t q0 = tile * GAUSS_TILE_QUADS, r0 = q0 / s.Q;
        const int j0 = (int)(q0 - r0 * s.Q);
#pragma unroll
        for (int k = 0; k < GAUSS_QUADS_PER_THREAD; ++k) {
            int row, c0;
            if (!gauss_quad(s, q0, r0, j0, k, row, c0)) continue;
            float e[4];
            noise4<VEC>(root_t, s.table, row, c0, s.F, e);
            store4<VEC>(eps + (int64_t)row * ld, c0, s.F, e);
        }
    }
}

}  // namespace npi

using namespace npi;

// tiles of N x F, or -1 when a size is outside its range (the tile count itself stays a count)
static int64_t gauss_tiles(int64_t N, int64_t F) {
    if (!count_ok(N) || F < 1 || F >= NPI_INDEX_LIMIT) return -1;
    const int64_t tiles = ceil_div(N * ceil_div(F, 4), (int64_t)GAUSS_TILE_QUADS);
    return count_ok(tiles) ? tiles : -1;
}

static GaussShape gauss_shape(int64_t N, int64_t F, int64_t key, int table) {
    GaussShape s;
    s.F = (int)F;
    s.Q = (int)ceil_div(F, 4);
    s.n_quads = N * s.Q;
    s.n_tiles = gauss_tiles(N, F);
    s.root = draw_root(key, DRAW_RULE_N);
    s.table = table;
    return s;
}

static unsigned gauss_grid(const GaussShape& s) { return stride_grid(s.n_tiles * GAUSS_THREADS, GAUSS_THREADS, 2048); }

static bool gauss_flags_ok(int flags) { return flags != 0 && (flags & ~(NPI_GAUSS_SAMPLE | NPI_GAUSS_KL)) == 0; }

extern "C" int64_t npi_gauss_workspace_bytes(int64_t N, int64_t F) {
    const int64_t tiles = gauss_tiles(N, F);
    return tiles < 0 ? -1 : align_up(max(tiles, (int64_t)1) * (int64_t)sizeof(double), 16);
}

extern "C" int npi_gauss_sample_kl(const float* mu, int64_t ld_mu, const float* logvar, int64_t ld_lv, int64_t N, int64_t F,
                                   int64_t n_total, float max_logvar, int64_t key, const int64_t* tick, int table, int flags, float* z,
                                   int64_t ld_z, float* kl, void* partials, int64_t partials_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const bool sample = (flags & NPI_GAUSS_SAMPLE) != 0, want_kl = (flags & NPI_GAUSS_KL) != 0;
    NPI_REQUIRE(gauss_flags_ok(flags), "npi_gauss_sample_kl: flags must be NPI_GAUSS_SAMPLE, NPI_GAUSS_KL or both");
    NPI_REQUIRE(gauss_tiles(N, F) >= 0 && ld_mu >= F && ld_lv >= F && (!sample || ld_z >= F) && count_ok(n_total) && n_total >= N &&
                    (N == 0 || n_total >= 1),
                "npi_gauss_sample_kl: bad size");
    NPI_REQUIRE(table == 0 || table == 1, "npi_gauss_sample_kl: table must be 0 or 1");
    if (want_kl) {
        NPI_REQUIRE(kl && partials, "npi_gauss_sample_kl: null pointer (NPI_GAUSS_KL needs kl and the partials workspace)");
        NPI_REQUIRE(((uintptr_t)partials % 16) == 0 && partials_bytes >= npi_gauss_workspace_bytes(N, F),
                    "npi_gauss_sample_kl: the partials workspace is misaligned or shorter than npi_gauss_workspace_bytes(N, F)");
    }
    NPI_REQUIRE(!sample || z || N == 0, "npi_gauss_sample_kl: null pointer (NPI_GAUSS_SAMPLE needs z)");
    if (N == 0) {                                              // no row, no kernel: the empty sum, written by the runtime
        const hipError_t e = want_kl ? hipMemsetAsync(kl, 0, sizeof(float), stream) : hipSuccess;
        if (e != hipSuccess) {
            set_error("npi_gauss_sample_kl: %s", hipGetErrorString(e));
            return NPI_ERR_LAUNCH;
        }
        return NPI_OK;
    }
    NPI_REQUIRE(mu && logvar, "npi_gauss_sample_kl: null pointer");
    const GaussShape s = gauss_shape(N, F, key, table);
    const unsigned grid = gauss_grid(s);
    const bool vec = rows16(mu, ld_mu, F) && rows16(logvar, ld_lv, F) && (!sample || rows16(z, ld_z, F));
    double* part = static_cast<double*>(partials);
#define NPI_GAUSS_FWD(V, S, K) \
    gauss_sample_kl_kernel<V, S, K><<<grid, GAUSS_THREADS, 0, stream>>>(s, tick, mu, ld_mu, logvar, ld_lv, max_logvar, z, ld_z, part)
    if (sample && want_kl) { if (vec) NPI_GAUSS_FWD(true, true, true); else NPI_GAUSS_FWD(false, true, true); }
    else if (sample) { if (vec) NPI_GAUSS_FWD(true, true, false); else NPI_GAUSS_FWD(false, true, false); }
    else { if (vec) NPI_GAUSS_FWD(true, false, true); else NPI_GAUSS_FWD(false, false, true); }
#undef NPI_GAUSS_FWD
    int rc = check_launch("npi_gauss_sample_kl");
    if (rc != NPI_OK || !want_kl) return rc;
    gauss_kl_sum_kernel<<<1, GAUSS_THREADS, 0, stream>>>(part, s.n_tiles, -0.5 / (double)n_total, kl);
    return check_launch("npi_gauss_sample_kl");
}

extern "C" int npi_gauss_sample_kl_bwd(const float* mu, int64_t ld_mu, const float* logvar, int64_t ld_lv, int64_t N, int64_t F,
                                       int64_t n_total, float max_logvar, int64_t key, const int64_t* tick, int table, int flags,
                                       const float* g_z, int64_t ld_gz, const float* g_kl, float* d_mu, int64_t ld_dmu,
                                       float* d_logvar, int64_t ld_dlv, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(gauss_flags_ok(flags), "npi_gauss_sample_kl_bwd: flags must be NPI_GAUSS_SAMPLE, NPI_GAUSS_KL or both");
    const bool gz = (flags & NPI_GAUSS_SAMPLE) != 0 && g_z, gkl = (flags & NPI_GAUSS_KL) != 0 && g_kl;
    NPI_REQUIRE(gauss_tiles(N, F) >= 0 && ld_mu >= F && ld_lv >= F && (!gz || ld_gz >= F) && (!d_mu || ld_dmu >= F) &&
                    (!d_logvar || ld_dlv >= F) && count_ok(n_total) && n_total >= N && (N == 0 || n_total >= 1),
                "npi_gauss_sample_kl_bwd: bad size");
    NPI_REQUIRE(table == 0 || table == 1, "npi_gauss_sample_kl_bwd: table must be 0 or 1");
    if (N == 0) return NPI_OK;
    NPI_REQUIRE(mu && logvar && (d_mu || d_logvar), "npi_gauss_sample_kl_bwd: null pointer (mu, logvar and one of d_mu, d_logvar)");
    const GaussShape s = gauss_shape(N, F, key, table);
    const unsigned grid = gauss_grid(s);
    const bool vec = rows16(mu, ld_mu, F) && rows16(logvar, ld_lv, F) && (!gz || rows16(g_z, ld_gz, F)) &&
                     (!d_mu || rows16(d_mu, ld_dmu, F)) && (!d_logvar || rows16(d_logvar, ld_dlv, F));
    const float inv_n = (float)(1.0 / (double)n_total);
#define NPI_GAUSS_BWD(V, Z, K)                                                                                                      \
    gauss_sample_kl_bwd_kernel<V, Z, K><<<grid, GAUSS_THREADS, 0, stream>>>(s, tick, mu, ld_mu, logvar, ld_lv, max_logvar, inv_n, g_z, ld_gz, \
                                                                            g_kl, d_mu, ld_dmu, d_logvar, ld_dlv)
    if (gz && gkl) { if (vec) NPI_GAUSS_BWD(true, true, true); else NPI_GAUSS_BWD(false, true, true); }
    else if (gz) { if (vec) NPI_GAUSS_BWD(true, true, false); else NPI_GAUSS_BWD(false, true, false); }
    else if (gkl) { if (vec) NPI_GAUSS_BWD(true, false, true); else NPI_GAUSS_BWD(false, false, true); }
    else { if (vec) NPI_GAUSS_BWD(true, false, false); else NPI_GAUSS_BWD(false, false, false); }
#undef NPI_GAUSS_BWD
    return check_launch("npi_gauss_sample_kl_bwd");
}

extern "C" int npi_gauss_noise(int64_t N, int64_t F, int64_t key, const int64_t* tick, int table, float* eps, int64_t ld,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(gauss_tiles(N, F) >= 0 && ld >= F, "npi_gauss_noise: bad size");
    NPI_REQUIRE(table == 0 || table == 1, "npi_gauss_noise: table must be 0 or 1");
    if (N == 0) return NPI_OK;
    NPI_REQUIRE(eps, "npi_gauss_noise: null pointer");
    const GaussShape s = gauss_shape(N, F, key, table);
    if (rows16(eps, ld, F)) gauss_noise_kernel<true><<<gauss_grid(s), GAUSS_THREADS, 0, stream>>>(s, tick, eps, ld);
    else gauss_noise_kernel<false><<<gauss_grid(s), GAUSS_THREADS, 0, stream>>>(s, tick, eps, ld);
    return check_launch("npi_gauss_noise");
}
