// Listwise link loss (include/npi_gnn.h: npi_softmax_link_*, RULE L): for every positive pair (s, t) the log-probability of t under
// the softmax over ALL candidate targets of s -- the known partners of s filtered out, t itself always in -- forward and backward,
// without the score matrix or the probability matrix ever leaving the chip.  The scan is score_tile.h's, the one topk.hip and
// link_rank.hip walk; what is new here are three consumers and a second stage.
//   softmax_link_tiles_kernel   grid (blocks of 64 queries) x (S column splits).  Per tile the 64 x 128 scores as KEYS in LDS, the
//                               excluded columns and the loop column marked; the consumer puts the target's own key (from the
//                               gathered tile, the same fmaf chain) BACK into column t_q, so that the target is a candidate in its
//                               own column position whatever the exclusion set says, then every lane folds its two keys of the row
//                               into an online (max, sum exp) of its own, kept in registers for the wavefront's 16 rows across all
//                               tiles of the split.  Which lane sees which column depends on the column alone, so a query's value
//                               does not depend on its slot.  One wave reduction per row at the end; each (query, split) writes a
//                               partial (m, s).
//   softmax_link_finish_kernel  one thread per query: the S partials merged in ascending split order, lse_q and lp_q written, and the
//                               workgroup's fp64 share of the loss (loss_sum.h adds the shares).
//   softmax_link_bwd_src_kernel grid (blocks of 64 queries) x (S column splits) x (chunks of 256 feature columns): the forward's scan
//                               again; the consumer turns the keys into w_qj = -u_q scale exp(x_qj - lse_q) (0 at a non-candidate and
//                               at t_q, whose term is the sparse part the caller adds) in place, and after the 16 rows of a tile the
//                               second stage adds sum_j w_qj z_dst[j, :] to the wavefront's 16 x 256 accumulators: a lane owns four
//                               columns, one 16-byte load of the partner's row per 64 fmaf, ascending j -- an fmaf chain per element.
//   softmax_link_bwd_dst_kernel the roles swapped: a workgroup owns 64 TARGETS (the A rows) and walks the QUERIES in tiles of 128, the
//                               B rows gathered as z_src[s_q] (score_tile.h: GATHER_B).  a . b = b . a term by term, so the score
//                               bits are the forward's.  Per tile a lane takes its two queries' (s, t, lse, u) and, by one binary
//                               search into s_q's sorted exclusion segment and a walk of at most the wavefront's 16 targets, a
//                               16-bit mask of the non-candidates among them (the loop and t_q included).  Second stage as above
//                               with z_src[s_q] as the partner row, ascending q.
//   split_sum_kernel            the S partial results of either backward scan added in ascending split order.
// No float atomics; every sum has one order.  LDS: ScoreTileShared alone, 89.25 KiB, one workgroup per CU.
#include <float.h>
#include "loss_sum.h"
#include "rank_key.h"
#include "score_tile.h"

namespace npi {

constexpr int SL_CHUNK = 4 * WAVE;                       // feature columns per pass of a backward scan at most: four per lane
constexpr int SL_MAX_CHUNKS = 65535;                     // gridDim.z
// lane groups of the second stage (SecondStage) for a table of F columns, and the columns one pass then covers
static int second_stage_groups(int64_t F) { return F <= SL_CHUNK / 4 ? 4 : (F <= SL_CHUNK / 2 ? 2 : 1); }

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}
__device__ __forceinline__ float neg_inf() { return __uint_as_float(0xff800000u); }
// RULE L 1: one f32 multiply, never contracted into what follows
__device__ __forceinline__ float scaled_score(float scale, uint32_t key) { return __fmul_rn(scale, rank_score(key)); }

// ---- forward: the online (max, sum exp) of every row
struct SoftmaxAcc {
    static constexpr bool UNROLL_ROWS = true;
    uint32_t v_thr;                                      // lane rr (mod 16): the target's key of the wavefront's row rr ...
    int v_tid;                                           // ... and its target id
    float scale;
    float m[TK_ROWS_PER_WAVE], s[TK_ROWS_PER_WAVE];      // this lane's share of the wavefront's rows
    int bad_score;

    __device__ __forceinline__ void threshold(const ScoreTileShared& sh, int wave, int lane) {
        const int r = wave * TK_ROWS_PER_WAVE + (lane & (TK_ROWS_PER_WAVE - 1));
        v_thr = sh.keys[r * TK_SPITCH + r];
        v_tid = sh.tid[r];
    }
    __device__ __forceinline__ void row(int rr, int, uint32_t* krow, int c0, int cn, int lane) {
        const int tq = __builtin_amdgcn_readlane(v_tid, rr);
        const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)v_thr, rr);
        if (lane == 0 && tq - c0 >= 0 && tq - c0 < cn) krow[tq - c0] = th;                // the target is always a candidate
        const uint32_t k0 = krow[lane], k1 = krow[WAVE + lane];
        const bool ok0 = k0 <= TK_KEY_LAST, ok1 = k1 <= TK_KEY_LAST;
        const bool nan = k0 == TK_KEY_NAN || k1 == TK_KEY_NAN;
        bad_score |= nan ? 1 : 0;
        const float x0 = ok0 ? scaled_score(scale, k0) : neg_inf();
        const float x1 = ok1 ? scaled_score(scale, k1) : neg_inf();
        const float mn = fmaxf(m[rr], fmaxf(x0, x1));
        if (mn > neg_inf()) {                                                             // column h * 64 + lane, h ascending
            float acc = s[rr] * expf(m[rr] - mn);
            acc += ok0 ? expf(x0 - mn) : 0.f;
            acc += ok1 ? expf(x1 - mn) : 0.f;
            s[rr] = acc;
            m[rr] = mn;
        }
        if (nan) s[rr] = __uint_as_float(0x7fc00000u);
    }
};

template <bool VEC>
__global__ void __launch_bounds__(TK_THREADS, 1)
softmax_link_tiles_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int Q, const float* __restrict__ zs,
                          int64_t lds_, int n_src, const float* __restrict__ zd, int64_t ldd, int n_dst, int F,
                          const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int no_loops, int tiles_per_split,
                          float scale, float2* __restrict__ partial, uint32_t* __restrict__ tkey, int32_t* __restrict__ status) {
    __shared__ ScoreTileShared sh;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int S = gridDim.y, split = blockIdx.y;

    const ScoreTileArgs args{src, dst, Q, zs, lds_, n_src, zd, ldd, n_dst, F, ex_rowptr, ex_col, no_loops, tiles_per_split, status};
    SoftmaxAcc acc;
    acc.v_thr = TK_KEY_OUT;
    acc.v_tid = -1;
    acc.scale = scale;
    acc.bad_score = 0;
#pragma unroll
    for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) {
        acc.m[rr] = neg_inf();
        acc.s[rr] = 0.f;
    }
    score_tiles<VEC, true>(args, sh, acc);
    if (status != nullptr && __any(acc.bad_score) && lane == 0) atomicOr(status, NPI_STATUS_BAD_SCORE);

    // ---- one reduction per row: partial[row * S + split] = (m, s); split 0 also leaves the row's key (TK_KEY_OUT: a bad pair)
#pragma unroll
    for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) {
        const float mw = wave_max_f(acc.m[rr]);
        const float mine = acc.m[rr] > neg_inf() ? acc.s[rr] * expf(acc.m[rr] - mw) : (acc.s[rr] != acc.s[rr] ? acc.s[rr] : 0.f);
        const float sw = wave_sum(mine);
        const int r = wave * TK_ROWS_PER_WAVE + rr;
        if (m0 + r < Q && lane == 0) partial[(m0 + r) * S + split] = make_float2(mw, sw);
    }
    if (split == 0 && lane < TK_ROWS_PER_WAVE) {
        const int r = wave * TK_ROWS_PER_WAVE + lane;
        if (m0 + r < Q) tkey[m0 + r] = sh.qid[r] >= 0 ? acc.v_thr : TK_KEY_OUT;
    }
}

__global__ void __launch_bounds__(TK_THREADS)
softmax_link_finish_kernel(const float2* __restrict__ partial, const uint32_t* __restrict__ tkey, int Q, int S, float scale,
                           double neg_inv_q, float* __restrict__ lp, float* __restrict__ lse, double* __restrict__ loss_part,
                           int32_t* __restrict__ status) {
    __shared__ double wsum[TK_THREADS / WAVE];
    const int64_t q = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
    double term = 0.0;
    if (q < Q) {
        const uint32_t key = tkey[q];
        float l = 0.f, e = 0.f;                                                           // a bad pair: RULE L 4
        if (key <= TK_KEY_LAST) {
            const float xt = scaled_score(scale, key);
            float m = neg_inf(), tot = 0.f;
            for (int s = 0; s < S; ++s) m = fmaxf(m, partial[q * S + s].x);
            for (int s = 0; s < S; ++s) {                                                 // ascending split order
                const float2 p = partial[q * S + s];
                if (p.x > neg_inf() || p.y != p.y) tot += p.y * expf(p.x - m);
            }
            e = m + logf(tot);                                                            // (the target is in: tot >= 1 up to rounding)
            l = xt - e;
            term = (double)l * neg_inv_q;                                                 // (a NaN score among the candidates: NaN)
        } else if (key == TK_KEY_NAN) {
            l = e = __uint_as_float(0x7fc00000u);
            term = (double)l;
            if (status != nullptr) atomicOr(status, NPI_STATUS_BAD_SCORE);
        }
        lp[q] = l;
        lse[q] = e;
    }
    if (loss_part == nullptr) return;
    term = wave_sum(term);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) loss_part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ---- backward: what both scans share
// four columns col .. col + 3 of a contiguous result row (F columns)
template <bool VEC>
__device__ __forceinline__ void store_k4(float* __restrict__ row, int col, int F, const float4& v) {
    if (VEC) {
        if (col < F) *reinterpret_cast<float4*>(row + col) = v;
    } else {
        if (col + 0 < F) row[col + 0] = v.x;
        if (col + 1 < F) row[col + 1] = v.y;
        if (col + 2 < F) row[col + 2] = v.z;
        if (col + 3 < F) row[col + 3] = v.w;
    }
}

// The second stage of a backward scan: acc[row, col] += sum over the tile's partners j of w[row][j] * partner_j[col], j ascending --
// one fmaf chain per element.  The wavefront's 16 rows are shared by GROUPS lane groups: a group owns 16 / GROUPS rows and each of
// its 64 / GROUPS lanes four feature columns, so that narrow tables (F <= 64: four groups, F <= 128: two) leave no lane idle; a
// wider table is walked in chunks of 256 columns by gridDim.z.  The partner rows of the next step of four are loaded before the
// 16-byte LDS reads and the fmaf of this one.  Which lane adds an element changes nothing about the order it is added in.
template <bool VEC, int GROUPS>
struct SecondStage {
    static constexpr int ROWS = TK_ROWS_PER_WAVE / GROUPS;
    static constexpr int LANES = WAVE / GROUPS;
    static constexpr int CHUNK = 4 * LANES;
    int col, row0;                                       // this lane's first column; the first of its rows among the wavefront's 16
    float4 acc[ROWS];

    __device__ __forceinline__ void init(int chunk, int lane) {
        col = chunk * CHUNK + 4 * (lane % LANES);
        row0 = (lane / LANES) * ROWS;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // load(j): columns col .. col + 3 of partner j's row (zeros for a partner that does not exist); rowmask: the rows row() has left
    // weights in -- the others still hold keys and are cleared first
    template <class Load>
    __device__ __forceinline__ void run(ScoreTileShared& sh, int wave, int lane, int cn, uint32_t rowmask, Load load) {
        if (rowmask == 0u) return;
        uint32_t* kw = sh.keys + wave * TK_ROWS_PER_WAVE * TK_SPITCH;
        if (rowmask != 0xffffu) {
#pragma unroll
            for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr)
                if (!((rowmask >> rr) & 1u)) kw[rr * TK_SPITCH + lane] = kw[rr * TK_SPITCH + WAVE + lane] = 0u;
        }
        const uint32_t* kl = kw + row0 * TK_SPITCH;
        float4 zn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) zn[e] = load(e);
        for (int j = 0; j < cn; j += 4) {
            float4 zr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) zr[e] = zn[e];
            if (j + 4 < cn) {
#pragma unroll
                for (int e = 0; e < 4; ++e) zn[e] = load(j + 4 + e);
            }
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const uint4 wb = *reinterpret_cast<const uint4*>(kl + i * TK_SPITCH + j);   // row() left the weights' bits there
                const float wx = __uint_as_float(wb.x), wy = __uint_as_float(wb.y), wz = __uint_as_float(wb.z), ww = __uint_as_float(wb.w);
                float4 a = acc[i];
                a.x = fmaf(wx, zr[0].x, a.x); a.y = fmaf(wx, zr[0].y, a.y); a.z = fmaf(wx, zr[0].z, a.z); a.w = fmaf(wx, zr[0].w, a.w);
                a.x = fmaf(wy, zr[1].x, a.x); a.y = fmaf(wy, zr[1].y, a.y); a.z = fmaf(wy, zr[1].z, a.z); a.w = fmaf(wy, zr[1].w, a.w);
                a.x = fmaf(wz, zr[2].x, a.x); a.y = fmaf(wz, zr[2].y, a.y); a.z = fmaf(wz, zr[2].z, a.z); a.w = fmaf(wz, zr[2].w, a.w);
                a.x = fmaf(ww, zr[3].x, a.x); a.y = fmaf(ww, zr[3].y, a.y); a.z = fmaf(ww, zr[3].z, a.z); a.w = fmaf(ww, zr[3].w, a.w);
                acc[i] = a;
            }
        }
    }
    // rows[(first + row) * F + col ..] for this lane's rows below `limit`: first = the id of the wavefront's row 0
    __device__ __forceinline__ void store(float* __restrict__ rows, int64_t first, int64_t limit, int F) const {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int64_t r = first + row0 + i;
            if (r < limit) store_k4<VEC>(rows + r * F, col, F, acc[i]);
        }
    }
};

// ---- backward, query-major: dq[q, :] = sum over the candidates j != t_q of w_qj z_dst[j, :]
template <bool VEC, int GROUPS>
struct SoftmaxGradSrc {
    static constexpr bool UNROLL_ROWS = true;
    static constexpr bool TILE_HOOKS = true;
    static constexpr bool GATHER_B = false;
    int v_tid;                                           // lane rr (mod 16): the target id of the wavefront's row rr ...
    float v_lse, v_c;                                    // ... its lse and -u_q * scale
    float scale;
    const float* __restrict__ zd;
    int64_t ldd;
    int F;
    uint32_t rowmask;                                    // the rows of the wavefront that row() has visited in this tile
    SecondStage<VEC, GROUPS> st;

    __device__ __forceinline__ void threshold(const ScoreTileShared& sh, int wave, int lane) {
        v_tid = sh.tid[wave * TK_ROWS_PER_WAVE + (lane & (TK_ROWS_PER_WAVE - 1))];
    }
    __device__ __forceinline__ void tile_begin(int, int, int, int) { rowmask = 0u; }
    __device__ __forceinline__ void row(int rr, int, uint32_t* krow, int c0, int cn, int lane) {
        const int tq = __builtin_amdgcn_readlane(v_tid, rr);
        const float lse = bcast_f(v_lse, rr), c = bcast_f(v_c, rr);
        if (lane == 0 && tq - c0 >= 0 && tq - c0 < cn) krow[tq - c0] = TK_KEY_OUT;        // the target's term is the sparse part
        rowmask |= 1u << rr;
#pragma unroll
        for (int h = 0; h < TK_BN / WAVE; ++h) {
            const uint32_t key = krow[h * WAVE + lane];
            const float w = key <= TK_KEY_LAST ? c * expf(scaled_score(scale, key) - lse) : 0.f;
            krow[h * WAVE + lane] = __float_as_uint(w);
        }
    }
    __device__ __forceinline__ void tile_end(ScoreTileShared& sh, int c0, int cn, int wave, int lane) {
        st.run(sh, wave, lane, cn, rowmask, [&](int j) {
            return j < cn ? load_k4<VEC>(zd + (int64_t)(c0 + j) * ldd, st.col, F) : make_float4(0.f, 0.f, 0.f, 0.f);
        });
    }
};

template <bool VEC, int GROUPS>
__global__ void __launch_bounds__(TK_THREADS, 1)
softmax_link_bwd_src_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int Q, const float* __restrict__ zs,
                            int64_t lds_, int n_src, const float* __restrict__ zd, int64_t ldd, int n_dst, int F,
                            const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int no_loops, int tiles_per_split,
                            float scale, const float* __restrict__ lse, const float* __restrict__ u, float* __restrict__ out) {
    __shared__ ScoreTileShared sh;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int split = blockIdx.y;

    const ScoreTileArgs args{src, dst, Q, zs, lds_, n_src, zd, ldd, n_dst, F, ex_rowptr, ex_col, no_loops, tiles_per_split, nullptr};
    SoftmaxGradSrc<VEC, GROUPS> g;
    const int64_t ql = m0 + wave * TK_ROWS_PER_WAVE + (lane & (TK_ROWS_PER_WAVE - 1));
    g.v_tid = -1;
    g.v_lse = ql < Q ? lse[ql] : 0.f;
    g.v_c = ql < Q ? -u[ql] * scale : 0.f;
    g.scale = scale;
    g.zd = zd;
    g.ldd = ldd;
    g.F = F;
    g.rowmask = 0u;
    g.st.init(blockIdx.z, lane);
    score_tiles<VEC, true>(args, sh, g);
    // ---- out[(split * Q + q) * F + col ..]: the split's share of dq (zeros for a bad pair)
    g.st.store(out + (int64_t)split * Q * F, m0 + wave * TK_ROWS_PER_WAVE, Q, F);
}

// ---- backward, target-major: dz_dst[j, :] = sum over the queries q that j is a candidate of, j != t_q, of w_qj z_src[s_q, :]
template <bool VEC, int GROUPS>
struct SoftmaxGradDst {
    static constexpr bool UNROLL_ROWS = true;
    static constexpr bool TILE_HOOKS = true;
    static constexpr bool GATHER_B = true;
    const int64_t* __restrict__ src;
    const int64_t* __restrict__ dst;
    const float* __restrict__ lse;
    const float* __restrict__ u;
    const int32_t* __restrict__ ex_rowptr;
    const int32_t* __restrict__ ex_col;
    const float* __restrict__ zs;
    int64_t lds;
    int n_src, n_dst, no_loops, F, j_wave;               // j_wave: the first target of this wavefront's 16
    float scale;
    // this lane's two queries of the tile (columns lane and 64 + lane): lse, -u scale (0: no query, or a bad pair), and the
    // wavefront's targets that are NOT candidates of the query, as bits
    float q_lse[2], q_c[2];
    uint32_t q_out[2];
    uint32_t rowmask;
    SecondStage<VEC, GROUPS> st;

    __device__ __forceinline__ void tile_begin(int c0, int cn, int, int lane) {
        rowmask = 0u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            q_lse[h] = 0.f;
            q_c[h] = 0.f;
            q_out[h] = 0xffffu;
            const int jq = h * WAVE + lane;
            if (jq >= cn) continue;
            const int64_t s = src[c0 + jq], tg = dst[c0 + jq];
            if ((uint64_t)s >= (uint64_t)n_src || (uint64_t)tg >= (uint64_t)n_dst) continue;
            uint32_t out = 0u;
            if (ex_rowptr != nullptr) {
                int lo = ex_rowptr[s];
                const int end = ex_rowptr[s + 1];
                int hi = end;
                while (lo < hi) {                                                         // first entry with column >= j_wave
                    const int mid = lo + ((hi - lo) >> 1);
                    if (ex_col[mid] < j_wave) lo = mid + 1; else hi = mid;
                }
                for (; lo < end; ++lo) {                                                  // sorted: at most this wavefront's 16, repeats aside
                    const int d = ex_col[lo] - j_wave;
                    if (d >= TK_ROWS_PER_WAVE) break;
                    out |= 1u << d;
                }
            }
            const int64_t dl = s - j_wave, dt = tg - j_wave;
            if (no_loops && dl >= 0 && dl < TK_ROWS_PER_WAVE) out |= 1u << (int)dl;
            if (dt >= 0 && dt < TK_ROWS_PER_WAVE) out |= 1u << (int)dt;                   // the target's term is the sparse part
            q_out[h] = out;
            q_lse[h] = lse[c0 + jq];
            q_c[h] = -u[c0 + jq] * scale;
        }
    }
    __device__ __forceinline__ void row(int rr, int, uint32_t* krow, int, int, int lane) {
        rowmask |= 1u << rr;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t key = krow[h * WAVE + lane];
            const bool cand = key <= TK_KEY_LAST && !((q_out[h] >> rr) & 1u);
            const float w = cand ? q_c[h] * expf(scaled_score(scale, key) - q_lse[h]) : 0.f;
            krow[h * WAVE + lane] = __float_as_uint(w);
        }
    }
    __device__ __forceinline__ void tile_end(ScoreTileShared& sh, int c0, int cn, int wave, int lane) {
        st.run(sh, wave, lane, cn, rowmask, [&](int j) {
            const int64_t id = j < cn ? src[c0 + j] : -1;                                 // wave-uniform
            return (uint64_t)id < (uint64_t)n_src ? load_k4<VEC>(zs + id * lds, st.col, F) : make_float4(0.f, 0.f, 0.f, 0.f);
        });
    }
};

template <bool VEC, int GROUPS>
__global__ void __launch_bounds__(TK_THREADS, 1)
softmax_link_bwd_dst_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int Q, const float* __restrict__ zs,
                            int64_t lds_, int n_src, const float* __restrict__ zd, int64_t ldd, int n_dst, int F,
                            const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int no_loops, int tiles_per_split,
                            float scale, const float* __restrict__ lse, const float* __restrict__ u, float* __restrict__ out) {
    __shared__ ScoreTileShared sh;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int split = blockIdx.y;

    // the targets are the rows (A = z_dst, ids 0 .. n_dst - 1), the queries the columns (B = z_src[s_q]); the candidate test is the
    // consumer's, so the producer gets no exclusion set
    ScoreTileArgs args{nullptr, nullptr, n_dst, zd, ldd, n_dst, zs, lds_, Q, F, nullptr, nullptr, 0, tiles_per_split, nullptr};
    args.brows = src;
    args.n_b = n_src;
    SoftmaxGradDst<VEC, GROUPS> g;
    g.src = src;
    g.dst = dst;
    g.lse = lse;
    g.u = u;
    g.ex_rowptr = ex_rowptr;
    g.ex_col = ex_col;
    g.zs = zs;
    g.lds = lds_;
    g.n_src = n_src;
    g.n_dst = n_dst;
    g.no_loops = no_loops;
    g.F = F;
    g.j_wave = (int)min(m0 + wave * TK_ROWS_PER_WAVE, (int64_t)n_dst);
    g.scale = scale;
    g.rowmask = 0u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        g.q_lse[h] = 0.f;
        g.q_c[h] = 0.f;
        g.q_out[h] = 0xffffu;
    }
    g.st.init(blockIdx.z, lane);
    score_tiles<VEC, false>(args, sh, g);
    // ---- out[(split * n_dst + j) * F + col ..]: the split's share of dz_dst
    g.st.store(out + (int64_t)split * n_dst * F, m0 + wave * TK_ROWS_PER_WAVE, n_dst, F);
}

// out[i] = p[i] + p[n + i] + ... + p[(S - 1) n + i], in that order
__global__ void __launch_bounds__(TK_THREADS)
split_sum_kernel(const float* __restrict__ p, int64_t n, int S, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
    if (i >= n) return;
    float v = p[i];
    for (int s = 1; s < S; ++s) v += p[(int64_t)s * n + i];
    out[i] = v;
}

// (host) the larger of two byte or row counts: spelled out, so that no overload of max() narrower than int64 can be picked
static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// tiles per split and the number of splits that have a tile, for `rows` query rows against `cols` columns
static void split_plan(int64_t rows, int64_t cols, int64_t splits, int64_t* per, int64_t* S) {
    *per = max64(ceil_div(topk_tiles(cols), topk_splits(rows, cols, splits)), (int64_t)1);
    *S = max64(ceil_div(topk_tiles(cols), *per), (int64_t)1);
}

static int64_t fwd_part_bytes(int64_t Q, int64_t S) { return align_up(max64(Q, (int64_t)1) * S * (int64_t)sizeof(float2), 16); }
static int64_t fwd_key_bytes(int64_t Q) { return align_up(max64(Q, (int64_t)1) * (int64_t)sizeof(uint32_t), 16); }
static int64_t fwd_loss_bytes(int64_t Q) { return align_up(max64(ceil_div(Q, TK_THREADS), (int64_t)1) * (int64_t)sizeof(double), 16); }

static bool softmax_link_sizes_ok(int64_t Q, int64_t n_src, int64_t n_dst, int64_t F) {
    return count_ok(Q) && count_ok(n_src) && count_ok(n_dst) && F > 0 && F < NPI_INDEX_LIMIT;
}

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_softmax_link_workspace_bytes(int64_t Q, int64_t n_src, int64_t n_dst, int64_t F, int64_t splits) {
    if (!softmax_link_sizes_ok(Q, n_src, n_dst, F) || splits < 0) return -1;
    const int64_t s_src = topk_splits(Q, n_dst, splits), s_dst = topk_splits(n_dst, Q, splits);
    const int64_t fwd = fwd_part_bytes(Q, s_src) + fwd_key_bytes(Q) + fwd_loss_bytes(Q);
    int64_t bwd_src, bwd_dst;                                  // rows (< 2^31) * splits (<= 64) fits; times 4 F may not: -1 then
    if (__builtin_mul_overflow(max64(Q, (int64_t)1) * s_src, F * (int64_t)sizeof(float), &bwd_src) ||
        __builtin_mul_overflow(max64(n_dst, (int64_t)1) * s_dst, F * (int64_t)sizeof(float), &bwd_dst) ||
        max64(bwd_src, bwd_dst) > INT64_MAX - 16)
        return -1;
    return align_up(max64(fwd, max64(bwd_src, bwd_dst)), 16);
}

// what the three entry points refuse alike, before the GPU is touched
#define NPI_SOFTMAX_LINK_REQUIRE(who)                                                                                                  \
    NPI_REQUIRE(softmax_link_sizes_ok(Q, n_src, n_dst, F) && ld_src >= F && ld_dst >= F,                                               \
                who ": bad size (Q, n_src, n_dst in [0, 2^31 - 1), F in [1, 2^31 - 1), pitches >= F)");                                \
    NPI_REQUIRE((flags & ~NPI_SOFTMAX_LINK_NO_LOOPS) == 0, who ": unknown flag");                                                      \
    NPI_REQUIRE(!(flags & NPI_SOFTMAX_LINK_NO_LOOPS) || n_src == n_dst,                                                                \
                who ": NPI_SOFTMAX_LINK_NO_LOOPS belongs to one id space (n_src == n_dst)");                                           \
    NPI_REQUIRE((ex_rowptr == nullptr) == (ex_col == nullptr), who ": the exclusion set is ex_rowptr and ex_col together, or both NULL"); \
    NPI_REQUIRE(splits >= 0, who ": splits must be 0 (choose) or positive");                                                           \
    NPI_REQUIRE(scale > 0.f && scale <= FLT_MAX, who ": scale must be positive and finite")

#define NPI_SOFTMAX_LINK_WORKSPACE(who)                                                                                                \
    NPI_REQUIRE(((uintptr_t)workspace % 16) == 0 && npi_softmax_link_workspace_bytes(Q, n_src, n_dst, F, splits) >= 0 &&               \
                    workspace_bytes >= npi_softmax_link_workspace_bytes(Q, n_src, n_dst, F, splits),                                   \
                who ": the workspace is misaligned or shorter than npi_softmax_link_workspace_bytes(Q, n_src, n_dst, F, splits)")

extern "C" int npi_softmax_link_fwd(const int64_t* src, const int64_t* dst, int64_t Q, const float* z_src, int64_t ld_src, int64_t n_src,
                                    const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F, const int32_t* ex_rowptr,
                                    const int32_t* ex_col, int flags, float scale, int64_t splits, float* lp, float* lse, float* loss,
                                    void* workspace, int64_t workspace_bytes, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_SOFTMAX_LINK_REQUIRE("npi_softmax_link_fwd");
    if (Q == 0) {                                              // no pair, no kernel: the empty sum, written by the runtime
        const hipError_t e = loss ? hipMemsetAsync(loss, 0, sizeof(float), stream) : hipSuccess;
        if (e != hipSuccess) {
            set_error("npi_softmax_link_fwd: %s", hipGetErrorString(e));
            return NPI_ERR_LAUNCH;
        }
        return NPI_OK;
    }
    NPI_REQUIRE(src && dst && lp && lse && workspace && (z_src || n_src == 0) && (z_dst || n_dst == 0), "npi_softmax_link_fwd: null pointer");
    NPI_SOFTMAX_LINK_WORKSPACE("npi_softmax_link_fwd");
    int64_t per, S;
    split_plan(Q, n_dst, splits, &per, &S);
    const dim3 grid((unsigned)ceil_div(Q, TK_BM), (unsigned)S);
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    char* base = static_cast<char*>(workspace);
    float2* partial = reinterpret_cast<float2*>(base);
    uint32_t* tkey = reinterpret_cast<uint32_t*>(base + fwd_part_bytes(Q, S));
    double* loss_part = loss ? reinterpret_cast<double*>(base + fwd_part_bytes(Q, S) + fwd_key_bytes(Q)) : nullptr;
#define NPI_SOFTMAX_LINK_TILES(V)                                                                                                     \
    softmax_link_tiles_kernel<V><<<grid, TK_THREADS, 0, stream>>>(src, dst, (int)Q, z_src, ld_src, (int)n_src, z_dst, ld_dst,         \
                                                                  (int)n_dst, (int)F, ex_rowptr, ex_col,                              \
                                                                  flags & NPI_SOFTMAX_LINK_NO_LOOPS, (int)per, scale, partial, tkey,  \
                                                                  status)
    if (vec) NPI_SOFTMAX_LINK_TILES(true); else NPI_SOFTMAX_LINK_TILES(false);
#undef NPI_SOFTMAX_LINK_TILES
    int rc = check_launch("npi_softmax_link_fwd");
    if (rc != NPI_OK) return rc;
    const int64_t n_wg = ceil_div(Q, TK_THREADS);
    // the divisor counts pairs, not good pairs: no host read of a device count (RULE L 6)
    softmax_link_finish_kernel<<<(unsigned)n_wg, TK_THREADS, 0, stream>>>(partial, tkey, (int)Q, (int)S, scale, -1.0 / (double)Q, lp,
                                                                          lse, loss_part, status);
    rc = check_launch("npi_softmax_link_fwd");
    if (rc != NPI_OK || !loss) return rc;
    pair_loss_sum_kernel<<<1, PS_SUM_THREADS, 0, stream>>>(loss_part, (int)n_wg, loss);
    return check_launch("npi_softmax_link_fwd");
}

// the split results of a backward scan: straight into `out` when there is one split and the rows allow it, else through the workspace
static float* bwd_target(float* out, void* workspace, int64_t S, bool vec) {
    return S == 1 && (!vec || ((uintptr_t)out % 16) == 0) ? out : static_cast<float*>(workspace);
}

extern "C" int npi_softmax_link_bwd_src(const int64_t* src, const int64_t* dst, int64_t Q, const float* z_src, int64_t ld_src,
                                        int64_t n_src, const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                                        const int32_t* ex_rowptr, const int32_t* ex_col, int flags, float scale, int64_t splits,
                                        const float* lse, const float* u, float* dq, void* workspace, int64_t workspace_bytes,
                                        void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_SOFTMAX_LINK_REQUIRE("npi_softmax_link_bwd_src");
    NPI_REQUIRE(ceil_div(F, SL_CHUNK) <= SL_MAX_CHUNKS, "npi_softmax_link_bwd_src: F above 65535 * 256");
    if (Q == 0) return NPI_OK;
    NPI_REQUIRE(src && dst && lse && u && dq && workspace && (z_src || n_src == 0) && (z_dst || n_dst == 0),
                "npi_softmax_link_bwd_src: null pointer");
    NPI_SOFTMAX_LINK_WORKSPACE("npi_softmax_link_bwd_src");
    int64_t per, S;
    split_plan(Q, n_dst, splits, &per, &S);
    const int groups = second_stage_groups(F);
    const dim3 grid((unsigned)ceil_div(Q, TK_BM), (unsigned)S, (unsigned)ceil_div(F, SL_CHUNK / groups));
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    float* part = bwd_target(dq, workspace, S, vec);
#define NPI_SOFTMAX_LINK_BWD_SRC(V, G)                                                                                                \
    softmax_link_bwd_src_kernel<V, G><<<grid, TK_THREADS, 0, stream>>>(src, dst, (int)Q, z_src, ld_src, (int)n_src, z_dst, ld_dst,    \
                                                                       (int)n_dst, (int)F, ex_rowptr, ex_col,                         \
                                                                       flags & NPI_SOFTMAX_LINK_NO_LOOPS, (int)per, scale, lse, u,    \
                                                                       part)
#define NPI_SOFTMAX_LINK_BWD_SRC_V(G) do { if (vec) NPI_SOFTMAX_LINK_BWD_SRC(true, G); else NPI_SOFTMAX_LINK_BWD_SRC(false, G); } while (0)
    if (groups == 4) NPI_SOFTMAX_LINK_BWD_SRC_V(4);
    else if (groups == 2) NPI_SOFTMAX_LINK_BWD_SRC_V(2);
    else NPI_SOFTMAX_LINK_BWD_SRC_V(1);
#undef NPI_SOFTMAX_LINK_BWD_SRC_V
#undef NPI_SOFTMAX_LINK_BWD_SRC
    const int rc = check_launch("npi_softmax_link_bwd_src");
    if (rc != NPI_OK || part == dq) return rc;
    const int64_t n = Q * F;
    split_sum_kernel<<<(unsigned)ceil_div(n, TK_THREADS), TK_THREADS, 0, stream>>>(part, n, (int)S, dq);
    return check_launch("npi_softmax_link_bwd_src");
}

extern "C" int npi_softmax_link_bwd_dst(const int64_t* src, const int64_t* dst, int64_t Q, const float* z_src, int64_t ld_src,
                                        int64_t n_src, const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                                        const int32_t* ex_rowptr, const int32_t* ex_col, int flags, float scale, int64_t splits,
                                        const float* lse, const float* u, float* dz_dst, void* workspace, int64_t workspace_bytes,
                                        void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_SOFTMAX_LINK_REQUIRE("npi_softmax_link_bwd_dst");
    NPI_REQUIRE(ceil_div(F, SL_CHUNK) <= SL_MAX_CHUNKS, "npi_softmax_link_bwd_dst: F above 65535 * 256");
    if (n_dst == 0) return NPI_OK;
    NPI_REQUIRE(dz_dst, "npi_softmax_link_bwd_dst: null pointer");
    if (Q == 0) {                                              // no pair: the zero gradient, written by the runtime
        const hipError_t e = hipMemsetAsync(dz_dst, 0, (size_t)(n_dst * F) * sizeof(float), stream);
        if (e != hipSuccess) {
            set_error("npi_softmax_link_bwd_dst: %s", hipGetErrorString(e));
            return NPI_ERR_LAUNCH;
        }
        return NPI_OK;
    }
    NPI_REQUIRE(src && dst && lse && u && workspace && (z_src || n_src == 0) && z_dst, "npi_softmax_link_bwd_dst: null pointer");
    NPI_SOFTMAX_LINK_WORKSPACE("npi_softmax_link_bwd_dst");
    int64_t per, S;
    split_plan(n_dst, Q, splits, &per, &S);                    // the splits cut the QUERY list here
    const int groups = second_stage_groups(F);
    const dim3 grid((unsigned)ceil_div(n_dst, TK_BM), (unsigned)S, (unsigned)ceil_div(F, SL_CHUNK / groups));
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    float* part = bwd_target(dz_dst, workspace, S, vec);
#define NPI_SOFTMAX_LINK_BWD_DST(V, G)                                                                                                \
    softmax_link_bwd_dst_kernel<V, G><<<grid, TK_THREADS, 0, stream>>>(src, dst, (int)Q, z_src, ld_src, (int)n_src, z_dst, ld_dst,    \
                                                                       (int)n_dst, (int)F, ex_rowptr, ex_col,                         \
                                                                       flags & NPI_SOFTMAX_LINK_NO_LOOPS, (int)per, scale, lse, u,    \
                                                                       part)
#define NPI_SOFTMAX_LINK_BWD_DST_V(G) do { if (vec) NPI_SOFTMAX_LINK_BWD_DST(true, G); else NPI_SOFTMAX_LINK_BWD_DST(false, G); } while (0)
    if (groups == 4) NPI_SOFTMAX_LINK_BWD_DST_V(4);
    else if (groups == 2) NPI_SOFTMAX_LINK_BWD_DST_V(2);
    else NPI_SOFTMAX_LINK_BWD_DST_V(1);
#undef NPI_SOFTMAX_LINK_BWD_DST_V
#undef NPI_SOFTMAX_LINK_BWD_DST
    const int rc = check_launch("npi_softmax_link_bwd_dst");
    if (rc != NPI_OK || part == dz_dst) return rc;
    const int64_t n = n_dst * F;
    split_sum_kernel<<<(unsigned)ceil_div(n, TK_THREADS), TK_THREADS, 0, stream>>>(part, n, (int)S, dz_dst);
    return check_launch("npi_softmax_link_bwd_dst");
}
