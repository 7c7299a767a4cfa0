// Top-k link prediction (include/npi_gnn.h: npi_topk_links, RULE K): for every query row the k best-scoring target rows that are
// not excluded -- what a user of PyG 1.4.2 gets from `InnerProductDecoder.forward_all` (a dense [N, N] product), a mask and
// `torch.topk`, and the reference from its per-case loops on the host (src/case_study*.py) -- without the score matrix ever
// leaving the chip.  Two kernels:
//   topk_tiles_kernel  grid (blocks of 64 query rows) x (S column splits).  A workgroup walks its split's z_dst rows in tiles of
//                      128, ascending.  Per tile: the 64 x 128 scores on v_mfma_f32_32x32x2_f32 (both operands K-contiguous, the
//                      A . B^T form of gemm_f32.hip's edge kernel: [row][BK + 4] LDS images, double-buffered k-steps of 32, the
//                      next tile's first k-step already in flight), the accumulators go to LDS as KEYS (rank_key.h), and every
//                      wavefront takes 16 rows: it marks the row's excluded columns (a cursor into the row's sorted CSR segment,
//                      placed by one binary search at the split's first column, moving forward only), compares the row's 128
//                      keys with the row's current k-th best lane-parallel (__ballot) and inserts the survivors into the row's
//                      sorted list of 128 (key << 32 | id) words -- two registers per lane while the row is being worked on, LDS
//                      otherwise.  After the first tiles almost nothing survives.  At the end each (row, split) writes its k
//                      best to the workspace.
//   topk_merge_kernel  one wavefront per query row: the S partial lists merged under the same order, scores (rebuilt from the
//                      key) and ids written.
// The k order of the products: the LDS image of a k-step stores column 8 g + e of a row at position 8 g + 4 (e & 1) + (e >> 1),
// so that the 16-byte fragment of lane half h holds columns 8 g + h, 8 g + 2 + h, 8 g + 4 + h, 8 g + 6 + h and MFMA s of a group
// multiplies columns 8 g + 2 s (half 0) and 8 g + 2 s + 1 (half 1): an ascending fmaf chain per output element, whatever tile,
// split or position in the query list the pair falls into (columns past F are zeros in both operands: fmaf(0, 0, acc) = acc).
// The (key, id) words are distinct within a row and totally ordered, so the k smallest of a row do not depend on the order in
// which they are met: no float atomics, no atomics at all but the status OR.  LDS: 2 x 27 KiB staging + 34 KiB keys + 64 KiB
// lists + 1 KiB row state = 153 KiB, one workgroup per CU.
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
constexpr int TK_LIST = NPI_TOPK_MAX;                    // list positions kept per row (the first k are the answer)
constexpr int TK_ROWS_PER_WAVE = TK_BM / (TK_THREADS / WAVE);
constexpr int TK_MAX_SPLITS = 64;
constexpr int TK_TARGET_WORKGROUPS = 512;                // two per CU of an MI355X: what the default split count aims at
static_assert(TK_LIST == 2 * WAVE, "a row's list is two words per lane");

// keys no score has (both are bit patterns of negative NaNs under rank_key): not a candidate / a NaN score
constexpr uint32_t TK_KEY_OUT = 0xffffffffu, TK_KEY_NAN = 0xfffffffeu, TK_KEY_LAST = 0xff800000u /* -inf */;
constexpr uint64_t TK_EMPTY = ~(uint64_t)0;              // key TK_KEY_OUT, id -1: an unused list slot

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1, WAVE);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

// A row's sorted list (ascending words = Rule K's order) spread over a wavefront: lane l holds positions l and 64 + l.
struct TopList {
    uint64_t a0, a1;
    __device__ __forceinline__ uint64_t kth(int k) const {                        // position k - 1 (k wave-uniform)
        return k <= WAVE ? readlane64(a0, k - 1) : readlane64(a1, k - 1 - WAVE);
    }
    // x (wave-uniform, > 0, not in the list) takes its place; what falls off position 127 is gone
    __device__ __forceinline__ void insert(uint64_t x, int lane) {
        uint64_t p0 = shfl_up64(a0), p1 = shfl_up64(a1);
        const uint64_t l0 = readlane64(a0, WAVE - 1);
        if (lane == 0) { p0 = 0; p1 = l0; }
        a0 = a0 < x ? a0 : (p0 < x ? x : p0);
        a1 = a1 < x ? a1 : (p1 < x ? x : p1);
    }
    // every lane offers one word (ok: it is a candidate); those below the k-th best go in, one at a time.  true: the list changed
    __device__ __forceinline__ bool offer(uint64_t x, bool ok, int k, int lane) {
        uint64_t thr = kth(k);
        uint64_t m = __ballot(ok && x < thr);
        const bool any = m != 0;
        while (m != 0) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const uint64_t xb = readlane64(x, b);
            if (xb < thr) {
                insert(xb, lane);
                thr = kth(k);
            }
        }
        return any;
    }
};

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

template <bool VEC>
__global__ void __launch_bounds__(TK_THREADS, 1)
topk_tiles_kernel(const int64_t* __restrict__ rows, int R, const float* __restrict__ zs, int64_t lds_, int n_src,
                  const float* __restrict__ zd, int64_t ldd, int n_dst, int F, int k, const int32_t* __restrict__ ex_rowptr,
                  const int32_t* __restrict__ ex_col, int no_loops, int tiles_per_split, uint64_t* __restrict__ ws,
                  int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float stage[2][TK_AF + TK_BF];
    __shared__ uint32_t keys[TK_BM * TK_SPITCH];
    __shared__ uint64_t lists[TK_BM * TK_LIST];
    __shared__ int qid[TK_BM], ex_cur[TK_BM], ex_end[TK_BM], ex_next[TK_BM];

    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int S = gridDim.y, split = blockIdx.y;
    const int n_tiles = (int)(((int64_t)n_dst + TK_BN - 1) / TK_BN);
    const int tile_beg = min((int)min((int64_t)split * tiles_per_split, (int64_t)n_tiles), n_tiles);
    const int tile_end = (int)min((int64_t)tile_beg + tiles_per_split, (int64_t)n_tiles);
    const int nk = (F + TK_BK - 1) / TK_BK;

    // ---- the rows of this workgroup: ids, exclusion cursors at the split's first column, empty lists
    for (int i = t; i < TK_BM * TK_LIST; i += TK_THREADS) lists[i] = TK_EMPTY;
    if (t < TK_BM) {
        const int64_t r = m0 + t;
        int q = -1, cur = 0, end = 0, next = 0x7fffffff;
        if (r < R) {
            const int64_t id = rows != nullptr ? rows[r] : r;
            if ((uint64_t)id < (uint64_t)n_src) q = (int)id;
            else if (status != nullptr && split == 0) atomicOr(status, NPI_STATUS_BAD_SOURCE_ID);
        }
        if (q >= 0 && ex_rowptr != nullptr) {
            const int cbeg = (int)min((int64_t)tile_beg * TK_BN, (int64_t)n_dst);
            int lo = ex_rowptr[q];
            end = ex_rowptr[q + 1];
            int hi = end;
            while (lo < hi) {                                                     // first entry with column >= cbeg
                const int mid = lo + ((hi - lo) >> 1);
                if (ex_col[mid] < cbeg) lo = mid + 1; else hi = mid;
            }
            cur = lo;
            if (cur < end) next = ex_col[cur];
        }
        qid[t] = q;
        ex_cur[t] = cur;
        ex_end[t] = end;
        ex_next[t] = next;
    }
    __syncthreads();

    // ---- staging: thread t moves float4 #(t & 7) of rows (t >> 3) + 32 p: two of the query tile, four of the target tile
    const int srow = t >> 3, sk = (t & 7) * 4;
    const int soff = ((t & 7) >> 1) * 8 + (t & 1) * 2;                            // the permuted image (file header)
    const int qa0 = qid[srow], qa1 = qid[srow + 32];
    const float* __restrict__ pa0 = zs + (int64_t)max(qa0, 0) * lds_;
    const float* __restrict__ pa1 = zs + (int64_t)max(qa1, 0) * lds_;
    float4 ra0, ra1, rb0, rb1, rb2, rb3;
    auto gload = [&](int tile, int kt) {
        const int kk = kt * TK_BK + sk;
        const int64_t j0 = (int64_t)tile * TK_BN + srow;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        ra0 = qa0 >= 0 ? load_k4<VEC>(pa0, kk, F) : z;
        ra1 = qa1 >= 0 ? load_k4<VEC>(pa1, kk, F) : z;
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
        put(stage[buf], srow, ra0);
        put(stage[buf], srow + 32, ra1);
        put(stage[buf] + TK_AF, srow, rb0);
        put(stage[buf] + TK_AF, srow + 32, rb1);
        put(stage[buf] + TK_AF, srow + 64, rb2);
        put(stage[buf] + TK_AF, srow + 96, rb3);
    };

    int buf = 0;
    if (tile_beg < tile_end) {
        gload(tile_beg, 0);
        lstore(0);
    }
    __syncthreads();
    int bad_score = 0;
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        for (int kt = 0; kt < nk; ++kt) {
            const bool last = kt + 1 == nk;
            const bool more = !last || tile + 1 < tile_end;
            if (more) gload(last ? tile + 1 : tile, last ? 0 : kt + 1);
            const float* as = stage[buf] + (wm * 32 + li) * TK_KPITCH + lh * 4;
            const float* bs = stage[buf] + TK_AF + (wn * 64 + li) * TK_KPITCH + lh * 4;
#pragma unroll
            for (int g = 0; g < TK_BK / 8; ++g) {
                const float4 a = *reinterpret_cast<const float4*>(as + g * 8);
                const float4 b0 = *reinterpret_cast<const float4*>(bs + g * 8);
                const float4 b1 = *reinterpret_cast<const float4*>(bs + 32 * TK_KPITCH + g * 8);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc[1], 0, 0, 0);
            }
            if (more) lstore(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }

        // ---- the tile's scores as keys: C/D map of the 32x32 MFMA, col = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
        const int c0 = tile * TK_BN;                                              // < n_dst
        const int cn = (int)min((int64_t)TK_BN, (int64_t)n_dst - c0);             // columns of this tile that exist
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wn * 64 + j * 32 + li;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
                const float v = acc[j][q];
                const uint32_t key = col < cn ? (v != v ? TK_KEY_NAN : rank_key(__float_as_uint(v))) : TK_KEY_OUT;
                keys[row * TK_SPITCH + col] = key;
            }
        }
        __syncthreads();

        // ---- every wavefront its 16 rows: exclusions, then the filter against the row's k-th best
        for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) {
            const int r = wave * TK_ROWS_PER_WAVE + rr;
            const int q = uniform_i(qid[r]);
            if (q < 0) continue;                                                  // a bad id, or past R: nothing is selected
            uint32_t* __restrict__ krow = keys + r * TK_SPITCH;
            if (uniform_i(ex_next[r]) - c0 < cn) {                                // (sorted columns: ex_next >= c0)
                int cur = uniform_i(ex_cur[r]);
                const int end = uniform_i(ex_end[r]);
                for (;;) {
                    const int idx = cur + lane;
                    const int col = idx < end ? ex_col[idx] - c0 : 0x7fffffff;
                    const bool in = col < cn;
                    if (in && col >= 0) krow[col] = TK_KEY_OUT;
                    const int n = __popcll(__ballot(in));                         // a prefix of the lanes
                    cur += n;
                    if (n < WAVE) break;
                }
                if (lane == 0) {
                    ex_cur[r] = cur;
                    ex_next[r] = cur < end ? ex_col[cur] : 0x7fffffff;
                }
            }
            if (no_loops && lane == 0 && q - c0 >= 0 && q - c0 < cn) krow[q - c0] = TK_KEY_OUT;
            TopList L;
            L.a0 = lists[r * TK_LIST + lane];
            L.a1 = lists[r * TK_LIST + WAVE + lane];
            bool changed = false;
#pragma unroll
            for (int h = 0; h < TK_BN / WAVE; ++h) {
                const uint32_t key = krow[h * WAVE + lane];
                bad_score |= key == TK_KEY_NAN ? 1 : 0;
                const uint64_t x = ((uint64_t)key << 32) | ((uint32_t)c0 + (uint32_t)(h * WAVE + lane));
                changed |= L.offer(x, key <= TK_KEY_LAST, k, lane);
            }
            if (changed) {
                lists[r * TK_LIST + lane] = L.a0;
                lists[r * TK_LIST + WAVE + lane] = L.a1;
            }
        }
        // (the next write of `keys` comes after the barriers of the next tile's k-steps: nk >= 1)
    }
    if (status != nullptr && __any(bad_score) && lane == 0) atomicOr(status, NPI_STATUS_BAD_SCORE);

    // ---- the partial lists: ws[(row * S + split) * k + p]
    for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) {
        const int r = wave * TK_ROWS_PER_WAVE + rr;
        if (m0 + r >= R) break;
        uint64_t* __restrict__ out = ws + ((m0 + r) * S + split) * (int64_t)k;
        if (lane < k) out[lane] = lists[r * TK_LIST + lane];
        if (WAVE + lane < k) out[WAVE + lane] = lists[r * TK_LIST + WAVE + lane];
    }
}

// one wavefront per query row: its S lists of k words (each ascending) -> the k best of all, as scores and ids
__global__ void __launch_bounds__(TK_THREADS)
topk_merge_kernel(const uint64_t* __restrict__ ws, int R, int S, int k, float* __restrict__ scores, int64_t* __restrict__ ids) {
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * (TK_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= R) return;
    const uint64_t* __restrict__ in = ws + row * S * (int64_t)k;
    TopList L;
    L.a0 = lane < k ? in[lane] : TK_EMPTY;
    L.a1 = WAVE + lane < k ? in[WAVE + lane] : TK_EMPTY;
    for (int s = 1; s < S; ++s) {
        const uint64_t* __restrict__ p = in + (int64_t)s * k;
        const uint64_t x0 = lane < k ? p[lane] : TK_EMPTY;
        const uint64_t x1 = WAVE + lane < k ? p[WAVE + lane] : TK_EMPTY;
        (void)L.offer(x0, x0 != TK_EMPTY, k, lane);
        (void)L.offer(x1, x1 != TK_EMPTY, k, lane);
    }
    const float ninf = __uint_as_float(0xff800000u);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = h * WAVE + lane;
        const uint64_t e = h == 0 ? L.a0 : L.a1;
        if (p < k) {
            const uint32_t key = (uint32_t)(e >> 32);
            const bool real = key != TK_KEY_OUT;
            scores[row * k + p] = real ? rank_score(key) : ninf;
            ids[row * k + p] = real ? (int64_t)(uint32_t)e : (int64_t)-1;
        }
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

using namespace npi;

extern "C" int64_t npi_topk_links_workspace_bytes(int64_t R, int64_t n_dst, int64_t k, int64_t splits) {
    if (!count_ok(R) || !count_ok(n_dst) || k < 1 || k > NPI_TOPK_MAX || splits < 0) return -1;
    return align_up(max(R, (int64_t)1) * topk_splits(R, n_dst, splits) * k * (int64_t)sizeof(uint64_t), 16);
}

extern "C" int npi_topk_links(const int64_t* rows, int64_t R, const float* z_src, int64_t ld_src, int64_t n_src, const float* z_dst,
                              int64_t ld_dst, int64_t n_dst, int64_t F, int64_t k, const int32_t* ex_rowptr, const int32_t* ex_col,
                              int flags, int64_t splits, float* scores, int64_t* ids, void* workspace, int64_t workspace_bytes,
                              int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(R) && count_ok(n_src) && count_ok(n_dst) && F > 0 && F < NPI_INDEX_LIMIT && ld_src >= F && ld_dst >= F,
                "npi_topk_links: bad size (R, n_src, n_dst in [0, 2^31 - 1), F in [1, 2^31 - 1), pitches >= F)");
    NPI_REQUIRE(k >= 1 && k <= NPI_TOPK_MAX, "npi_topk_links: k must lie in [1, NPI_TOPK_MAX]");
    NPI_REQUIRE((flags & ~NPI_TOPK_NO_LOOPS) == 0, "npi_topk_links: unknown flag");
    NPI_REQUIRE(!(flags & NPI_TOPK_NO_LOOPS) || n_src == n_dst, "npi_topk_links: NPI_TOPK_NO_LOOPS belongs to one id space (n_src == n_dst)");
    NPI_REQUIRE((ex_rowptr == nullptr) == (ex_col == nullptr), "npi_topk_links: the exclusion set is ex_rowptr and ex_col together, or both NULL");
    NPI_REQUIRE(splits >= 0, "npi_topk_links: splits must be 0 (choose) or positive");
    if (R == 0) return NPI_OK;
    NPI_REQUIRE(scores && ids && workspace && (z_src || n_src == 0) && (z_dst || n_dst == 0), "npi_topk_links: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace % 16) == 0 && workspace_bytes >= npi_topk_links_workspace_bytes(R, n_dst, k, splits),
                "npi_topk_links: the workspace is misaligned or shorter than npi_topk_links_workspace_bytes(R, n_dst, k, splits)");
    const int64_t per = max(ceil_div(topk_tiles(n_dst), topk_splits(R, n_dst, splits)), (int64_t)1);     // tiles per split
    const int64_t S = max(ceil_div(topk_tiles(n_dst), per), (int64_t)1);                                  // no split without a tile
    const dim3 grid((unsigned)ceil_div(R, TK_BM), (unsigned)S);
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    uint64_t* ws = static_cast<uint64_t*>(workspace);
#define NPI_TOPK_TILES(V)                                                                                                           \
    topk_tiles_kernel<V><<<grid, TK_THREADS, 0, stream>>>(rows, (int)R, z_src, ld_src, (int)n_src, z_dst, ld_dst, (int)n_dst, (int)F, \
                                                          (int)k, ex_rowptr, ex_col, flags & NPI_TOPK_NO_LOOPS, (int)per, ws, status)
    if (vec) NPI_TOPK_TILES(true); else NPI_TOPK_TILES(false);
#undef NPI_TOPK_TILES
    const int rc = check_launch("npi_topk_links");
    if (rc != NPI_OK) return rc;
    topk_merge_kernel<<<(unsigned)ceil_div(R, TK_THREADS / WAVE), TK_THREADS, 0, stream>>>(ws, (int)R, (int)S, (int)k, scores, ids);
    return check_launch("npi_topk_links");
}
