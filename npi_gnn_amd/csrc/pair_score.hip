// Scores of a list of (source, target) pairs from two embedding tables and the link-prediction loss over them (include/npi_gnn.h:
// npi_pair_score) -- PyG 1.4.2 `InnerProductDecoder.forward` (`(z[edge_index[0]] * z[edge_index[1]]).sum(dim=1)`) and
// `GAE.recon_loss`, or `binary_cross_entropy_with_logits`, in ONE launch over the list as it is: no CSR, no sort, no [M, F] gather
// written to memory, no logits written when only the loss is wanted.
//   logit_m = <z_src[src_m], z_dst[dst_m]>;  the first n_pos pairs are positives, the rest negatives (`torch.cat([pos, neg], 1)`)
// The shape of edge_dot_kernel with BOTH operands gathered: one wavefront per block of 64 pairs, ids fetched lane-parallel, the pairs
// eight at a time -- sixteen gathered rows in flight per lane -- the eight partial dots reduce-scattered over the wave, the 64 logits
// parked in LDS so that the loss terms, the coefficients d loss / d logit and the stores are lane-parallel again.
// No float atomics: a wave sums its 64 loss terms in a fixed tree, a workgroup its four waves in order into ONE fp64 partial, and a
// second, one-workgroup launch (loss_sum.h) adds the partials in a fixed order.  Every output element has one writer.
#include "dot_lanes.h"
#include "loss_sum.h"

namespace npi {

constexpr int PS_WAVES = 4;                    // wavefronts (blocks of 64 pairs) per workgroup: one partial per 256 pairs

// Loss term and d term / d logit of one pair, before the 1 / count of its part.  s = sigmoid(x) in f32 throughout.
//   GAE: PyG's expressions literally, EPS = 1e-15: a positive -log(s + EPS), a negative -log(1 - s + EPS), and what autograd
//        gives for exactly those: -s q / (s + EPS) and s q / (q + EPS) with ONE q = 1 - s in numerator and denominator.
//   BCE: max(x, 0) - x y + log1p(exp(-|x|)) and s - y, the latter as -sigmoid(-x) for y = 1 so that neither cancels: one
//        e = exp(-|x|) <= 1 serves both, finite at any x.
template <int MODE>
__device__ __forceinline__ void pair_term(float x, bool pos, float& term, float& d) {
    if (MODE == NPI_PAIR_LOSS_GAE) {
        constexpr float EPS = 1e-15f;
        const float s = 1.0f / (1.0f + expf(-x));
        const float q = 1.0f - s;
        term = -logf((pos ? s : q) + EPS);
        d = pos ? -(s * q) / (s + EPS) : (s * q) / (q + EPS);
    } else {
        const float e = expf(-fabsf(x));
        const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);         // sigmoid(|x|), sigmoid(-|x|)
        term = fmaxf(x, 0.f) - (pos ? x : 0.f) + log1pf(e);
        d = pos ? -(x >= 0.f ? small : big) : (x >= 0.f ? big : small);
    }
}

//   VEC : 16-byte lanes (F % 4 == 0, 16-byte aligned rows of both tables), a chunk is 256 columns; otherwise one float per lane,
//         64 columns.  A row wider than one chunk walks the chunks inside the group of eight.
//   MODE: NPI_PAIR_LOGITS writes logits only; the loss modes write any of logits / coef / partials[blockIdx.x].
// A pair with an id outside its table: logit 0, coefficient 0, loss term 0, its rows never read, the status bit raised.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(PS_WAVES * WAVE)
pair_score_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int M, int n_pos, const float* __restrict__ zs,
                  int64_t lds, int n_src, const float* __restrict__ zd, int64_t ldd, int n_dst, int F, float inv_pos, float inv_neg,
                  float* __restrict__ logits, float* __restrict__ coef, double* __restrict__ partials, int32_t* __restrict__ status) {
    using L = Lanes<VEC>;
    using T = typename L::T;
    constexpr int CW = WAVE * L::W;
    const int lane = lane_id();
    const int wv = uniform_i(threadIdx.x >> 6);
    const int64_t kb = ((int64_t)blockIdx.x * PS_WAVES + wv) * WAVE;
    const int nb = uniform_i((int)max((int64_t)0, min((int64_t)WAVE, (int64_t)M - kb)));      // 0: a wave past the list (it still meets the barrier)
    __shared__ float pbuf[PS_WAVES][WAVE];
    __shared__ double wsum[PS_WAVES];
    float* __restrict__ pb = pbuf[wv];
    const int e_of_lane = group_of_lane(lane);
    int sv = 0, dv = 0;
    bool inside = false;
    if (lane < nb) {
        const int64_t s = src[kb + lane], d = dst[kb + lane];
        inside = (uint64_t)s < (uint64_t)n_src && (uint64_t)d < (uint64_t)n_dst;
        if (inside) { sv = (int)s; dv = (int)d; }
    }
    const uint64_t ok = __ballot(inside);                                                    // wave-uniform: which pairs read rows at all
    if (status != nullptr && lane == 0 && nb > 0 && ok != (~(uint64_t)0 >> (WAVE - nb))) atomicOr(status, NPI_STATUS_BAD_PAIR_ID);
    for (int j = 0; j < nb; j += 8) {
        float p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = 0.f;
        for (int c0 = 0; c0 < F; c0 += CW) {
            const int off = c0 + lane * L::W;
            const bool act = off < F;
            T a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int m = j + u;                                                         // < 64; past nb: no bit in `ok`
                const bool rd = act && ((ok >> m) & 1) != 0;
                const int su = bcast_i(sv, m), du = bcast_i(dv, m);
                a[u] = rd ? L::load(zs + (int64_t)su * lds + off) : L::zero();
                b[u] = rd ? L::load(zd + (int64_t)du * ldd + off) : L::zero();
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = L::dot(a[u], b[u], p[u]);
        }
        const float y = reduce_scatter8(p, lane);
        if ((lane & 7) == 0 && j + e_of_lane < nb) pb[j + e_of_lane] = y;
    }
    __builtin_amdgcn_wave_barrier();
    double t = 0.0;
    if (lane < nb) {
        const float x = inside ? pb[lane] : 0.f;
        if (logits) logits[kb + lane] = x;
        if (MODE != NPI_PAIR_LOGITS) {
            const bool pos = kb + lane < n_pos;
            const float inv = pos ? inv_pos : inv_neg;
            float term = 0.f, d = 0.f;
            if (inside) pair_term<MODE>(x, pos, term, d);
            if (coef) coef[kb + lane] = d * inv;
            t = (double)term * (double)inv;
        }
    }
    if (MODE != NPI_PAIR_LOGITS) {
        if (partials == nullptr) return;                                                     // (uniform over the workgroup)
        t = wave_sum(t);
        if (lane == 0) wsum[wv] = t;
        __syncthreads();
        if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

}  // namespace npi

using namespace npi;

static bool pair_size_ok(int64_t M) { return M >= 0 && M < 0x7fffffff; }

extern "C" int64_t npi_pair_score_workspace_bytes(int64_t M) {
    if (!pair_size_ok(M)) return -1;
    return align_up(max(ceil_div(M, (int64_t)PS_WAVES * WAVE), (int64_t)1) * (int64_t)sizeof(double), 16);
}

extern "C" int npi_pair_score(const int64_t* src, const int64_t* dst, int64_t M, int64_t n_pos, const float* z_src, int64_t ld_src,
                              int64_t n_src, const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F, int mode, float* logits,
                              float* coef, float* loss, void* partials, int64_t partials_bytes, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(mode == NPI_PAIR_LOGITS || mode == NPI_PAIR_LOSS_GAE || mode == NPI_PAIR_LOSS_BCE,
                "npi_pair_score: mode must be NPI_PAIR_LOGITS, NPI_PAIR_LOSS_GAE or NPI_PAIR_LOSS_BCE");
    NPI_REQUIRE(pair_size_ok(M) && F > 0 && F < 0x7fffffff && n_src >= 0 && n_src < 0x7fffffff && n_dst >= 0 && n_dst < 0x7fffffff &&
                    n_pos >= 0 && n_pos <= M && ld_src >= F && ld_dst >= F,
                "npi_pair_score: bad size");
    NPI_REQUIRE(logits || coef || loss, "npi_pair_score: null pointer (at least one of logits, coef, loss is required)");
    NPI_REQUIRE(mode != NPI_PAIR_LOGITS || (!coef && !loss), "npi_pair_score: coef and loss belong to the loss modes");
    if (loss) {
        NPI_REQUIRE(partials, "npi_pair_score: null pointer (loss needs the partials workspace)");
        NPI_REQUIRE(((uintptr_t)partials % 16) == 0 && partials_bytes >= npi_pair_score_workspace_bytes(M),
                    "npi_pair_score: the partials workspace is misaligned or shorter than npi_pair_score_workspace_bytes(M)");
    }
    if (M == 0) {                                              // no pair, no kernel: the empty sum, written by the runtime
        const hipError_t e = loss ? hipMemsetAsync(loss, 0, sizeof(float), stream) : hipSuccess;
        if (e != hipSuccess) {
            set_error("npi_pair_score: %s", hipGetErrorString(e));
            return NPI_ERR_LAUNCH;
        }
        return NPI_OK;
    }
    NPI_REQUIRE(src && dst && z_src && z_dst, "npi_pair_score: null pointer");
    const int64_t n_wg = ceil_div(M, (int64_t)PS_WAVES * WAVE);
    const unsigned grid = (unsigned)n_wg;
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    // a part without a pair contributes 0 (torch's mean() of an empty tensor is NaN: a deliberate deviation, see the header)
    const int64_t n_neg = M - n_pos;
    float inv_pos, inv_neg;
    if (mode == NPI_PAIR_LOSS_BCE) {
        inv_pos = inv_neg = (float)(1.0 / (double)M);
    } else {
        inv_pos = n_pos > 0 ? (float)(1.0 / (double)n_pos) : 0.f;
        inv_neg = n_neg > 0 ? (float)(1.0 / (double)n_neg) : 0.f;
    }
    double* part = loss ? static_cast<double*>(partials) : nullptr;
#define NPI_PAIR_SCORE(V, MODE)                                                                                                   \
    pair_score_kernel<V, MODE><<<grid, PS_WAVES * WAVE, 0, stream>>>(src, dst, (int)M, (int)n_pos, z_src, ld_src, (int)n_src, z_dst, \
                                                                     ld_dst, (int)n_dst, (int)F, inv_pos, inv_neg, logits, coef,  \
                                                                     part, status)
    if (mode == NPI_PAIR_LOGITS) { if (vec) NPI_PAIR_SCORE(true, NPI_PAIR_LOGITS); else NPI_PAIR_SCORE(false, NPI_PAIR_LOGITS); }
    else if (mode == NPI_PAIR_LOSS_GAE) { if (vec) NPI_PAIR_SCORE(true, NPI_PAIR_LOSS_GAE); else NPI_PAIR_SCORE(false, NPI_PAIR_LOSS_GAE); }
    else { if (vec) NPI_PAIR_SCORE(true, NPI_PAIR_LOSS_BCE); else NPI_PAIR_SCORE(false, NPI_PAIR_LOSS_BCE); }
#undef NPI_PAIR_SCORE
    int rc = check_launch("npi_pair_score");
    if (rc != NPI_OK || !loss) return rc;
    pair_loss_sum_kernel<<<1, PS_SUM_THREADS, 0, stream>>>(part, (int)n_wg, loss);
    return check_launch("npi_pair_score");
}
