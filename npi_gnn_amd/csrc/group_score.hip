// Ranking losses over corrupted targets (include/npi_gnn.h: npi_group_score, Rule G): every positive (src_p, dst_p) scored against its
// own K corrupted targets neg[p, 0 .. K) -- a GROUP of C = 1 + K slots that share ONE source row -- and reduced to BPR, a margin
// hinge or the sampled softmax in ONE launch over src / dst / neg as they are: no expanded pair list, no logits written when only
// the loss is wanted.
// The shape of pair_score_kernel (dot_lanes.h, four waves per workgroup, one fp64 partial per workgroup, the sum of loss_sum.h) with
// two differences that are the reason for a kernel of its own:
//   * a wavefront owns G = 64 / C WHOLE groups, i.e. G C <= 64 flat slots (lanes past that idle), so that everything a group needs
//     -- its positive logit, the softmax maximum and denominator, coef_0 -- is in this wave's LDS;
//   * within a batch of eight slots the source chunk of slot u is loaded only when u == 0 or its group differs from that of slot
//     u - 1 (wave-uniform); otherwise the register of slot u - 1 is reused: one source load per distinct group of a batch, not eight.
// Per-group quantities are formed by the group's head lane in a serial ascending loop over its <= 63 LDS slots: a fixed order, so
// the value of a slot and of its coefficient depends only on the rows of its group, never on where the group sits in the list.
// No float atomics; every output element has one writer.
#include "dot_lanes.h"
#include "loss_sum.h"

namespace npi {

constexpr int GS_WAVES = 4;                    // wavefronts per workgroup: one partial per 4 * (64 / C) groups
constexpr int GS_MAX_K = 63;                   // a group fits one wavefront

static __host__ __device__ __forceinline__ int groups_per_wave(int C) { return WAVE / C; }

//   VEC : as in pair_score_kernel (16-byte lanes and 256-column chunks, or one float per lane and 64-column chunks)
//   MODE: NPI_GROUP_LOGITS writes logits only; the loss modes write any of logits / coef / partials[blockIdx.x]
// inv = 1 / (P K) (bpr, margin; 0 for K = 0) or 1 / P (softmax): the divisors count SLOTS, whatever their validity.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(GS_WAVES * WAVE, 5)
group_score_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int P, const int64_t* __restrict__ neg,
                   int64_t ld_neg, int C, const float* __restrict__ zs, int64_t lds, int n_src, const float* __restrict__ zd,
                   int64_t ldd, int n_dst, int F, float margin, float scale, float inv, float* __restrict__ logits,
                   float* __restrict__ coef, double* __restrict__ partials, int32_t* __restrict__ status) {
    using L = Lanes<VEC>;
    using T = typename L::T;
    constexpr int CW = WAVE * L::W;
    constexpr float NINF = -__builtin_huge_valf();
    const int lane = lane_id();
    const int wv = uniform_i(threadIdx.x >> 6);
    const int G = groups_per_wave(C);
    const int64_t gb = ((int64_t)blockIdx.x * GS_WAVES + wv) * G;                             // this wave's first group
    const int ng = uniform_i((int)max((int64_t)0, min((int64_t)G, (int64_t)P - gb)));         // 0: a wave past the list
    const int ns = ng * C;                                                                   // its flat slots, <= 64
    __shared__ float xbuf[GS_WAVES][WAVE];     // logits
    __shared__ float dbuf[GS_WAVES][WAVE];     // d_c of the valid negative slots, -inf elsewhere; a head's slot: the group's m
    __shared__ float ebuf[GS_WAVES][WAVE];     // a head's slot: the group's denominator
    __shared__ float cbuf[GS_WAVES][WAVE];     // coefficients of the negative slots
    __shared__ double wsum[GS_WAVES];
    float* __restrict__ xb = xbuf[wv];
    float* __restrict__ db = dbuf[wv];
    float* __restrict__ eb = ebuf[wv];
    float* __restrict__ cb = cbuf[wv];
    const int e_of_lane = group_of_lane(lane);
    const int g = lane / C, c = lane - g * C;                                                // group within the wave, slot within it
    const int head = g * C;
    int sv = 0, tv = 0;
    bool group_ok = false, slot_ok = false, bad = false;
    if (lane < ns) {
        const int64_t p = gb + g;
        const int64_t s = src[p], d = dst[p];
        group_ok = (uint64_t)s < (uint64_t)n_src && (uint64_t)d < (uint64_t)n_dst;
        const int64_t t = c == 0 ? d : neg[p * ld_neg + (c - 1)];
        const bool t_in = (uint64_t)t < (uint64_t)n_dst;
        slot_ok = group_ok && t_in;
        bad = !group_ok || (!t_in && t != -1);                                               // -1: an empty slot, no status
        if (group_ok) sv = (int)s;
        if (slot_ok) tv = (int)t;
    }
    const uint64_t gok = __ballot(group_ok);                                                 // wave-uniform: whose source row is read
    const uint64_t ok = __ballot(slot_ok);                                                   //               whose target row is read
    if (status != nullptr && __ballot(bad) != 0 && lane == 0) atomicOr(status, NPI_STATUS_BAD_PAIR_ID);
    for (int j = 0; j < ns; j += 8) {
        float p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = 0.f;
        for (int c0 = 0; c0 < F; c0 += CW) {
            const int off = c0 + lane * L::W;
            const bool act = off < F;
            T a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int m = j + u;                                                         // < 64; past ns: no bit in `gok` / `ok`
                const bool fresh = u == 0 || bcast_i(g, m) != bcast_i(g, m - 1);              // wave-uniform
                if (fresh) {
                    const int su = bcast_i(sv, m);
                    a[u] = (act && ((gok >> m) & 1) != 0) ? L::load(zs + (int64_t)su * lds + off) : L::zero();
                } else {
                    a[u] = a[u > 0 ? u - 1 : 0];
                }
                const int tu = bcast_i(tv, m);
                b[u] = (act && ((ok >> m) & 1) != 0) ? L::load(zd + (int64_t)tu * ldd + off) : L::zero();
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = L::dot(a[u], b[u], p[u]);
        }
        const float y = reduce_scatter8(p, lane);
        if ((lane & 7) == 0 && j + e_of_lane < ns) xb[j + e_of_lane] = y;
    }
    __builtin_amdgcn_wave_barrier();
    const bool live = lane < ns;
    const bool vneg = live && slot_ok && c > 0;                                              // a valid negative slot
    // a dropped group: all logits 0;  an empty or bad slot of a kept group: -inf
    const float x = !live ? 0.f : (slot_ok ? xb[lane] : (group_ok ? NINF : 0.f));
    if (live && logits) logits[gb * C + lane] = x;
    if (MODE == NPI_GROUP_LOGITS) return;
    const float x0 = live ? xb[head] : 0.f;
    const float d = vneg ? scale * (x - x0) : NINF;
    float term = 0.f, cf = 0.f;
    if (MODE == NPI_GROUP_LOSS_SOFTMAX) {
        db[lane] = d;
        __builtin_amdgcn_wave_barrier();
        float m = 0.f, den = 1.f;
        if (live && c == 0) {                                                                // the head: max and denominator, ascending
            for (int k = 1; k < C; ++k) m = fmaxf(m, db[lane + k]);
            den = expf(-m);
            for (int k = 1; k < C; ++k) {
                const float v = db[lane + k];
                if (v > NINF) den += expf(v - m);
            }
            term = m + logf(den);
        }
        __builtin_amdgcn_wave_barrier();                                                     // every head has read its d's
        if (live && c == 0) { db[lane] = m; eb[lane] = den; }
        __builtin_amdgcn_wave_barrier();
        if (vneg) cf = scale * (expf(d - db[head]) / eb[head]) * inv;
    } else if (vneg) {
        if (MODE == NPI_GROUP_LOSS_BPR) {
            const float e = expf(-fabsf(d));
            term = fmaxf(d, 0.f) + log1pf(e);
            cf = scale * (d >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e)) * inv;
        } else {
            const float h = margin + d;
            term = fmaxf(h, 0.f);
            cf = h > 0.f ? scale * inv : 0.f;
        }
    }
    if (coef) {                                                                              // (uniform over the workgroup)
        cb[lane] = cf;
        __builtin_amdgcn_wave_barrier();
        if (live && c == 0) {                                                                // coef_0 = -(sum in ascending slot order)
            float sum = 0.f;
            for (int k = 1; k < C; ++k) sum += cb[lane + k];
            cf = -sum;
        }
        if (live) coef[gb * C + lane] = cf;
    }
    if (partials == nullptr) return;                                                         // (uniform over the workgroup)
    double t = wave_sum((double)term * (double)inv);
    if (lane == 0) wsum[wv] = t;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

}  // namespace npi

using namespace npi;

static bool group_sizes_ok(int64_t P, int64_t K) {
    return P >= 0 && P < 0x7fffffff && K >= 0 && K <= GS_MAX_K && P * (1 + K) < 0x7fffffff;
}

extern "C" int64_t npi_group_score_workspace_bytes(int64_t P, int64_t K) {
    if (!group_sizes_ok(P, K)) return -1;
    const int64_t per_wg = (int64_t)GS_WAVES * groups_per_wave((int)(1 + K));
    return align_up(max(ceil_div(P, per_wg), (int64_t)1) * (int64_t)sizeof(double), 16);
}

extern "C" int npi_group_score(const int64_t* src, const int64_t* dst, int64_t P, const int64_t* neg, int64_t ld_neg, int64_t K,
                               const float* z_src, int64_t ld_src, int64_t n_src, const float* z_dst, int64_t ld_dst, int64_t n_dst,
                               int64_t F, int mode, float margin, float scale, float* logits, float* coef, float* loss, void* partials,
                               int64_t partials_bytes, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(mode == NPI_GROUP_LOGITS || mode == NPI_GROUP_LOSS_BPR || mode == NPI_GROUP_LOSS_MARGIN || mode == NPI_GROUP_LOSS_SOFTMAX,
                "npi_group_score: mode must be NPI_GROUP_LOGITS, NPI_GROUP_LOSS_BPR, NPI_GROUP_LOSS_MARGIN or NPI_GROUP_LOSS_SOFTMAX");
    NPI_REQUIRE(group_sizes_ok(P, K) && ld_neg >= K && F > 0 && F < 0x7fffffff && n_src >= 0 && n_src < 0x7fffffff && n_dst >= 0 &&
                    n_dst < 0x7fffffff && ld_src >= F && ld_dst >= F,
                "npi_group_score: bad size");
    NPI_REQUIRE(margin - margin == 0.f && scale - scale == 0.f && scale > 0.f,
                "npi_group_score: margin and scale must be finite, scale > 0");
    NPI_REQUIRE(logits || coef || loss, "npi_group_score: null pointer (at least one of logits, coef, loss is required)");
    NPI_REQUIRE(mode != NPI_GROUP_LOGITS || (!coef && !loss), "npi_group_score: coef and loss belong to the loss modes");
    if (loss) {
        NPI_REQUIRE(partials, "npi_group_score: null pointer (loss needs the partials workspace)");
        NPI_REQUIRE(((uintptr_t)partials % 16) == 0 && partials_bytes >= npi_group_score_workspace_bytes(P, K),
                    "npi_group_score: the partials workspace is misaligned or shorter than npi_group_score_workspace_bytes(P, K)");
    }
    if (P == 0) {                                              // no group, no kernel: the empty sum, written by the runtime
        const hipError_t e = loss ? hipMemsetAsync(loss, 0, sizeof(float), stream) : hipSuccess;
        if (e != hipSuccess) {
            set_error("npi_group_score: %s", hipGetErrorString(e));
            return NPI_ERR_LAUNCH;
        }
        return NPI_OK;
    }
    NPI_REQUIRE(src && dst && z_src && z_dst && (neg || K == 0), "npi_group_score: null pointer");
    const int C = (int)(1 + K);
    const int64_t n_wg = ceil_div(P, (int64_t)GS_WAVES * groups_per_wave(C));
    const unsigned grid = (unsigned)n_wg;
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    // the divisors count slots, not valid slots: no host read of a device count (a deliberate deviation, see the header)
    const float inv = mode == NPI_GROUP_LOSS_SOFTMAX ? (float)(1.0 / (double)P) : (K > 0 ? (float)(1.0 / ((double)P * (double)K)) : 0.f);
    double* part = loss ? static_cast<double*>(partials) : nullptr;
#define NPI_GROUP_SCORE(V, MODE)                                                                                                   \
    group_score_kernel<V, MODE><<<grid, GS_WAVES * WAVE, 0, stream>>>(src, dst, (int)P, neg, ld_neg, C, z_src, ld_src, (int)n_src,    \
                                                                      z_dst, ld_dst, (int)n_dst, (int)F, margin, scale, inv, logits, \
                                                                      coef, part, status)
#define NPI_GROUP_SCORE_V(MODE) do { if (vec) NPI_GROUP_SCORE(true, MODE); else NPI_GROUP_SCORE(false, MODE); } while (0)
    if (mode == NPI_GROUP_LOGITS) NPI_GROUP_SCORE_V(NPI_GROUP_LOGITS);
    else if (mode == NPI_GROUP_LOSS_BPR) NPI_GROUP_SCORE_V(NPI_GROUP_LOSS_BPR);
    else if (mode == NPI_GROUP_LOSS_MARGIN) NPI_GROUP_SCORE_V(NPI_GROUP_LOSS_MARGIN);
    else NPI_GROUP_SCORE_V(NPI_GROUP_LOSS_SOFTMAX);
#undef NPI_GROUP_SCORE_V
#undef NPI_GROUP_SCORE
    int rc = check_launch("npi_group_score");
    if (rc != NPI_OK || !loss) return rc;
    pair_loss_sum_kernel<<<1, PS_SUM_THREADS, 0, stream>>>(part, (int)n_wg, loss);
    return check_launch("npi_group_score");
}
