// Top-k link prediction (include/npi_gnn.h: npi_topk_links, RULE K): for every query row the k best-scoring target rows that are
// not excluded -- what a user of PyG 1.4.2 gets from `InnerProductDecoder.forward_all` (a dense [N, N] product), a mask and
// `torch.topk`, and the reference from its per-case loops on the host (src/case_study*.py) -- without the score matrix ever
// leaving the chip.  Two kernels:
//   topk_tiles_kernel  grid (blocks of 64 query rows) x (S column splits).  The scan is score_tile.h's: per tile of 128 targets
//                      the 64 x 128 scores on v_mfma_f32_32x32x2_f32 as KEYS (rank_key.h) in LDS, the excluded columns marked.
//                      The consumer here is the SELECTION: every wavefront compares a row's 128 keys with the row's current k-th
//                      best lane-parallel (__ballot) and inserts the survivors into the row's sorted list of 128 (key << 32 | id)
//                      words -- two registers per lane while the row is being worked on, LDS otherwise.  After the first tiles
//                      almost nothing survives.  At the end each (row, split) writes its k best to the workspace.
//   topk_merge_kernel  one wavefront per query row: the S partial lists merged under the same order, scores (rebuilt from the
//                      key) and ids written.
// The (key, id) words are distinct within a row and totally ordered, so the k smallest of a row do not depend on the order in
// which they are met: no float atomics, no atomics at all but the status OR.  LDS: 2 x 27 KiB staging + 34 KiB keys + 64 KiB
// lists + 1.25 KiB row state = 153 KiB, one workgroup per CU.
#include "rank_key.h"
#include "score_tile.h"

namespace npi {

constexpr int TK_LIST = NPI_TOPK_MAX;                    // list positions kept per row (the first k are the answer)
static_assert(TK_LIST == 2 * WAVE, "a row's list is two words per lane");
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

// the selection consumer of score_tile.h's scan: a row's candidates of one tile offered to the row's list
struct TopkSelect {
    static constexpr bool UNROLL_ROWS = false;
    uint64_t* __restrict__ lists;
    int k, bad_score;
    __device__ __forceinline__ void row(int, int r, const uint32_t* krow, int c0, int, int lane) {
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
};

template <bool VEC>
__global__ void __launch_bounds__(TK_THREADS, 1)
topk_tiles_kernel(const int64_t* __restrict__ rows, int R, const float* __restrict__ zs, int64_t lds_, int n_src,
                  const float* __restrict__ zd, int64_t ldd, int n_dst, int F, int k, const int32_t* __restrict__ ex_rowptr,
                  const int32_t* __restrict__ ex_col, int no_loops, int tiles_per_split, uint64_t* __restrict__ ws,
                  int32_t* __restrict__ status) {
    __shared__ ScoreTileShared sh;
    __shared__ uint64_t lists[TK_BM * TK_LIST];

    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int S = gridDim.y, split = blockIdx.y;

    for (int i = t; i < TK_BM * TK_LIST; i += TK_THREADS) lists[i] = TK_EMPTY;
    const ScoreTileArgs args{rows, nullptr, R, zs, lds_, n_src, zd, ldd, n_dst, F, ex_rowptr, ex_col, no_loops, tiles_per_split, status};
    TopkSelect select{lists, k, 0};
    score_tiles<VEC, false>(args, sh, select);
    if (status != nullptr && __any(select.bad_score) && lane == 0) atomicOr(status, NPI_STATUS_BAD_SCORE);

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
