// The tile producer of the all-targets scans (include/npi_gnn.h: RULE K 1 - 3), shared by the top-k selection (topk.hip), the
// filtered link ranks (link_rank.hip) and the listwise link loss (softmax_link.hip).  A workgroup of 256 threads owns 64 query
// rows and walks its split's z_dst rows in tiles of 128, ascending.
// Per tile: the 64 x 128 scores on v_mfma_f32_32x32x2_f32 (both operands K-contiguous, the A . B^T form of
// gemm_f32.hip's edge kernel: [row][BK + 4] LDS images, double-buffered k-steps of 32, the next tile's first k-step already in
// flight), the accumulators go to LDS as KEYS (rank_key.h), and every wavefront takes 16 rows: it marks the row's excluded columns
// (a cursor into the row's sorted CSR segment, placed by one binary search at the split's first column, moving forward only) and
// the loop column, then hands the row's 128 keys to the CONSUMER -- what the files differ in.
// The k order of the products: the LDS image of a k-step stores column 8 g + e of a row at position 8 g + 4 (e & 1) + (e >> 1),
// so that the 16-byte fragment of lane half h holds columns 8 g + h, 8 g + 2 + h, 8 g + 4 + h, 8 g + 6 + h and MFMA s of a group
// multiplies columns 8 g + 2 s (half 0) and 8 g + 2 s + 1 (half 1): an ascending fmaf chain per output element, whatever tile,
// split or position in the query list the pair falls into (columns past F are zeros in both operands: fmaf(0, 0, acc) = acc).
// PAIRS (link_rank.hip): a query is a pair (source, target).  Before its first tile the workgroup runs the same k-loop on the 64
// gathered rows z_dst[target] as a B tile of their own; element (r, r) of that tile is the key of row r's target -- the same
// chain as every other element, so it equals the key the pair has in the tile its column falls into.
//
// A consumer provides
//   static constexpr bool UNROLL_ROWS           the 16 rows of a wavefront as straight-line code (state per row in registers)
//   void threshold(sh, wave, lane)              PAIRS only: sh.keys holds the gathered tile; a wavefront takes what it needs of its
//                                               rows 16 wave .. 16 wave + 15 into registers
//   void row(rr, r, krow, c0, cn, lane)         row r = 16 wave + rr of the workgroup (a good id), its keys of the tile's columns
//                                               c0 .. c0 + cn - 1 in krow[0 .. cn) (TK_KEY_OUT: no candidate; also past cn)
// and may provide (softmax_link.hip; a consumer without the constant compiles to what it compiled to before)
//   static constexpr bool TILE_HOOKS = true     void tile_begin(c0, cn, wave, lane) before the rows of a tile and
//                                               void tile_end(sh, c0, cn, wave, lane) after them: a second stage over what row()
//                                               left in the wavefront's own 16 rows of sh.keys
//   static constexpr bool GATHER_B = true       the B row of column j is zd[brows[j]] (zeros for an id outside [0, n_b)), not
//                                               zd[j]: the columns are a list, n_dst its length
#pragma once
#include <type_traits>
#include "dot_lanes.h"
#include "rank_key.h"

namespace npi {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TK_THREADS = 256;
constexpr int TK_BM = 64;                                // query rows per workgroup: 2 x 2 wavefronts of 32 rows x 64 columns
constexpr int TK_BN = 128;                               // target rows per tile
constexpr int TK_BK = 32;
constexpr int TK_KPITCH = TK_BK + 4;                     // [row][k] image, fragment reads free of bank conflicts (gemm_f32.hip)
constexpr int TK_AF = TK_BM * TK_KPITCH, TK_BF = TK_BN * TK_KPITCH;
constexpr int TK_SPITCH = TK_BN + 8;                     // key tile: rows r and r + 4 of one accumulator store 32 banks apart
constexpr int TK_ROWS_PER_WAVE = TK_BM / (TK_THREADS / WAVE);
constexpr int TK_MAX_SPLITS = 64;
constexpr int TK_TARGET_WORKGROUPS = 512;                // two per CU of an MI355X: what the default split count aims at

// keys no score has (both are bit patterns of negative NaNs under rank_key): not a candidate / a NaN score
constexpr uint32_t TK_KEY_OUT = 0xffffffffu, TK_KEY_NAN = 0xfffffffeu, TK_KEY_LAST = 0xff800000u /* -inf */;

// the optional constants of a consumer (file header)
template <class C, class = void> struct tile_hooks : std::false_type {};
template <class C> struct tile_hooks<C, std::void_t<decltype(C::TILE_HOOKS)>> : std::bool_constant<C::TILE_HOOKS> {};
template <class C, class = void> struct gather_b : std::false_type {};
template <class C> struct gather_b<C, std::void_t<decltype(C::GATHER_B)>> : std::bool_constant<C::GATHER_B> {};

// four columns k .. k + 3 of a table row (zeros past F); VEC: one 16-byte load (F % 4 == 0, aligned rows)
template <bool VEC>
__device__ __forceinline__ float4 load_k4(const float* __restrict__ row, int k, int F) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
        if (k < F) v = *reinterpret_cast<const float4*>(row + k);
    } else {
        if (k + 0 < F) v.x = row[k + 0];
        if (k + 1 < F) v.y = row[k + 1];
        if (k + 2 < F) v.z = row[k + 2];
        if (k + 3 < F) v.w = row[k + 3];
    }
    return v;
}

// the queries (PAIRS: rows = the sources, never NULL, targets = their partners), the tables and the exclusion set of one scan
struct ScoreTileArgs {
    const int64_t* __restrict__ rows;
    const int64_t* __restrict__ targets;
    int R;
    const float* __restrict__ zs;
    int64_t lds;
    int n_src;
    const float* __restrict__ zd;
    int64_t ldd;
    int n_dst, F;
    const int32_t* __restrict__ ex_rowptr;
    const int32_t* __restrict__ ex_col;
    int no_loops, tiles_per_split;
    int32_t* __restrict__ status;
    const int64_t* __restrict__ brows = nullptr;         // GATHER_B consumers only: the B row id of every column, ids in [0, n_b)
    int n_b = 0;
};

// the producer's LDS: 2 x 27 KiB staging + 34 KiB keys + 1.25 KiB row state
struct ScoreTileShared {
    __attribute__((aligned(16))) float stage[2][TK_AF + TK_BF];
    uint32_t keys[TK_BM * TK_SPITCH];
    int qid[TK_BM], ex_cur[TK_BM], ex_end[TK_BM], ex_next[TK_BM];
    int tid[TK_BM];                                      // PAIRS: the row's target id (-1 with a bad pair)
};

// the whole scan of one workgroup: blockIdx.x = its 64 queries, blockIdx.y = its split of gridDim.y.  The caller has initialised
// its consumer's LDS, if any; the first barrier in here covers it.
template <bool VEC, bool PAIRS, class Consumer>
__device__ __forceinline__ void score_tiles(const ScoreTileArgs& a, ScoreTileShared& sh, Consumer& consumer) {
    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int split = blockIdx.y;
    const int n_dst = a.n_dst, F = a.F;
    const int n_tiles = (int)(((int64_t)n_dst + TK_BN - 1) / TK_BN);
    const int tile_beg = min((int)min((int64_t)split * a.tiles_per_split, (int64_t)n_tiles), n_tiles);
    const int tile_end = (int)min((int64_t)tile_beg + a.tiles_per_split, (int64_t)n_tiles);
    const int tile_first = PAIRS ? tile_beg - 1 : tile_beg;                       // PAIRS: tile_beg - 1 stands for the gathered tile
    const int nk = (F + TK_BK - 1) / TK_BK;

    // ---- the rows of this workgroup: ids, exclusion cursors at the split's first column
    if (t < TK_BM) {
        const int64_t r = m0 + t;
        int q = -1, tq = -1, cur = 0, end = 0, next = 0x7fffffff;
        if (r < a.R) {
            const int64_t id = a.rows != nullptr ? a.rows[r] : r;
            bool ok = (uint64_t)id < (uint64_t)a.n_src;
            if (PAIRS) {
                const int64_t tj = a.targets[r];
                ok = ok && (uint64_t)tj < (uint64_t)n_dst;
                if (ok) tq = (int)tj;
            }
            if (ok) q = (int)id;
            else if (a.status != nullptr && split == 0) atomicOr(a.status, PAIRS ? NPI_STATUS_BAD_PAIR_ID : NPI_STATUS_BAD_SOURCE_ID);
        }
        if (q >= 0 && a.ex_rowptr != nullptr) {
            const int cbeg = (int)min((int64_t)tile_beg * TK_BN, (int64_t)n_dst);
            int lo = a.ex_rowptr[q];
            end = a.ex_rowptr[q + 1];
            int hi = end;
            while (lo < hi) {                                                     // first entry with column >= cbeg
                const int mid = lo + ((hi - lo) >> 1);
                if (a.ex_col[mid] < cbeg) lo = mid + 1; else hi = mid;
            }
            cur = lo;
            if (cur < end) next = a.ex_col[cur];
        }
        sh.qid[t] = q;
        sh.ex_cur[t] = cur;
        sh.ex_end[t] = end;
        sh.ex_next[t] = next;
        if (PAIRS) sh.tid[t] = tq;
    }
    __syncthreads();

    // ---- staging: thread t moves float4 #(t & 7) of rows (t >> 3) + 32 p: two of the query tile, four of the target tile
    const int srow = t >> 3, sk = (t & 7) * 4;
    const int soff = ((t & 7) >> 1) * 8 + (t & 1) * 2;                            // the permuted image (file header)
    const int qa0 = sh.qid[srow], qa1 = sh.qid[srow + 32];
    const float* __restrict__ pa0 = a.zs + (int64_t)max(qa0, 0) * a.lds;
    const float* __restrict__ pa1 = a.zs + (int64_t)max(qa1, 0) * a.lds;
    const float* __restrict__ zd = a.zd;
    const int64_t ldd = a.ldd;
    float4 ra0, ra1, rb0, rb1, rb2, rb3;
    auto gload = [&](int tile, int kt) {
        const int kk = kt * TK_BK + sk;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        ra0 = qa0 >= 0 ? load_k4<VEC>(pa0, kk, F) : z;
        ra1 = qa1 >= 0 ? load_k4<VEC>(pa1, kk, F) : z;
        if (PAIRS && tile < tile_beg) {                                           // the targets of the 64 queries, gathered
            const int t0 = sh.tid[srow], t1 = sh.tid[srow + 32];
            rb0 = t0 >= 0 ? load_k4<VEC>(zd + (int64_t)t0 * ldd, kk, F) : z;
            rb1 = t1 >= 0 ? load_k4<VEC>(zd + (int64_t)t1 * ldd, kk, F) : z;
            rb2 = z;
            rb3 = z;
            return;
        }
        const int64_t j0 = (int64_t)tile * TK_BN + srow;
        if constexpr (gather_b<Consumer>::value) {
            auto brow = [&](int64_t j) {
                const int64_t id = j < n_dst ? a.brows[j] : -1;
                return (uint64_t)id < (uint64_t)a.n_b ? load_k4<VEC>(zd + id * ldd, kk, F) : z;
            };
            rb0 = brow(j0);
            rb1 = brow(j0 + 32);
            rb2 = brow(j0 + 64);
            rb3 = brow(j0 + 96);
            return;
        }
        rb0 = j0 + 0 < n_dst ? load_k4<VEC>(zd + (j0 + 0) * ldd, kk, F) : z;
        rb1 = j0 + 32 < n_dst ? load_k4<VEC>(zd + (j0 + 32) * ldd, kk, F) : z;
        rb2 = j0 + 64 < n_dst ? load_k4<VEC>(zd + (j0 + 64) * ldd, kk, F) : z;
        rb3 = j0 + 96 < n_dst ? load_k4<VEC>(zd + (j0 + 96) * ldd, kk, F) : z;
    };
    auto put = [&](float* img, int row, const float4& v) {
        float* d = img + row * TK_KPITCH + soff;
        *reinterpret_cast<float2*>(d) = make_float2(v.x, v.z);
        *reinterpret_cast<float2*>(d + 4) = make_float2(v.y, v.w);
    };
    auto lstore = [&](int buf) {
        put(sh.stage[buf], srow, ra0);
        put(sh.stage[buf], srow + 32, ra1);
        put(sh.stage[buf] + TK_AF, srow, rb0);
        put(sh.stage[buf] + TK_AF, srow + 32, rb1);
        put(sh.stage[buf] + TK_AF, srow + 64, rb2);
        put(sh.stage[buf] + TK_AF, srow + 96, rb3);
    };

    // a wavefront's 16 rows across 16 lanes: what the row loop needs wave-uniform comes from a register (v_readlane), not from an
    // LDS round trip per row (EXPERIMENTS.md A53)
    const int rl = wave * TK_ROWS_PER_WAVE + (lane & (TK_ROWS_PER_WAVE - 1));
    const int v_qid = sh.qid[rl];

    int buf = 0;
    if (tile_first < tile_end) {
        gload(tile_first, 0);
        lstore(0);
    }
    __syncthreads();
    for (int tile = tile_first; tile < tile_end; ++tile) {
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        for (int kt = 0; kt < nk; ++kt) {
            const bool last = kt + 1 == nk;
            const bool more = !last || tile + 1 < tile_end;
            if (more) gload(last ? tile + 1 : tile, last ? 0 : kt + 1);
            const float* as = sh.stage[buf] + (wm * 32 + li) * TK_KPITCH + lh * 4;
            const float* bs = sh.stage[buf] + TK_AF + (wn * 64 + li) * TK_KPITCH + lh * 4;
#pragma unroll
            for (int g = 0; g < TK_BK / 8; ++g) {
                const float4 a4 = *reinterpret_cast<const float4*>(as + g * 8);
                const float4 b0 = *reinterpret_cast<const float4*>(bs + g * 8);
                const float4 b1 = *reinterpret_cast<const float4*>(bs + 32 * TK_KPITCH + g * 8);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b1.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b0.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b0.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b1.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b0.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b1.w, acc[1], 0, 0, 0);
            }
            if (more) lstore(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }

        // ---- the tile's scores as keys: C/D map of the 32x32 MFMA, col = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
        const bool gathered = PAIRS && tile < tile_beg;
        const int c0 = gathered ? 0 : tile * TK_BN;                               // < n_dst
        const int cn = gathered ? TK_BM : (int)min((int64_t)TK_BN, (int64_t)n_dst - c0);      // columns of this tile that exist
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wn * 64 + j * 32 + li;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
                const float v = acc[j][q];
                const uint32_t key = col < cn ? (v != v ? TK_KEY_NAN : rank_key(__float_as_uint(v))) : TK_KEY_OUT;
                sh.keys[row * TK_SPITCH + col] = key;
            }
        }
        __syncthreads();
        if constexpr (PAIRS) {
            if (gathered) {
                consumer.threshold(sh, wave, lane);
                continue;
            }
        }

        // ---- every wavefront its 16 rows: exclusions and the loop column, then the consumer
        if constexpr (tile_hooks<Consumer>::value) consumer.tile_begin(c0, cn, wave, lane);
        const int v_next = sh.ex_next[rl];                                        // (row r's is written in row r's turn only)
        auto one_row = [&](int rr) {
            const int r = wave * TK_ROWS_PER_WAVE + rr;
            const int q = __builtin_amdgcn_readlane(v_qid, rr);
            if (q < 0) return;                                                    // a bad id, or past R: nothing to consume
            uint32_t* __restrict__ krow = sh.keys + r * TK_SPITCH;
            if (__builtin_amdgcn_readlane(v_next, rr) - c0 < cn) {                // (sorted columns: ex_next >= c0)
                int cur = uniform_i(sh.ex_cur[r]);
                const int end = uniform_i(sh.ex_end[r]);
                for (;;) {
                    const int idx = cur + lane;
                    const int col = idx < end ? a.ex_col[idx] - c0 : 0x7fffffff;
                    const bool in = col < cn;
                    if (in && col >= 0) krow[col] = TK_KEY_OUT;
                    const int n = __popcll(__ballot(in));                         // a prefix of the lanes
                    cur += n;
                    if (n < WAVE) break;
                }
                if (lane == 0) {
                    sh.ex_cur[r] = cur;
                    sh.ex_next[r] = cur < end ? a.ex_col[cur] : 0x7fffffff;
                }
            }
            if (a.no_loops && lane == 0 && q - c0 >= 0 && q - c0 < cn) krow[q - c0] = TK_KEY_OUT;
            consumer.row(rr, r, krow, c0, cn, lane);
        };
        if constexpr (Consumer::UNROLL_ROWS) {
#pragma unroll
            for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) one_row(rr);
        } else {
            for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) one_row(rr);
        }
        if constexpr (tile_hooks<Consumer>::value) consumer.tile_end(sh, c0, cn, wave, lane);
        // (the next write of `keys` comes after the barriers of the next tile's k-steps: nk >= 1)
    }
}

static int64_t topk_tiles(int64_t n_dst) { return ceil_div(n_dst, TK_BN); }
// S: the caller's, or enough splits for TK_TARGET_WORKGROUPS workgroups; never more than there are tiles, or than TK_MAX_SPLITS
static int64_t topk_splits(int64_t R, int64_t n_dst, int64_t splits) {
    int64_t s = splits > 0 ? splits : ceil_div(TK_TARGET_WORKGROUPS, max(ceil_div(R, TK_BM), (int64_t)1));
    s = min(s, min(topk_tiles(n_dst), (int64_t)TK_MAX_SPLITS));
    return max(s, (int64_t)1);
}

}  // namespace npi
