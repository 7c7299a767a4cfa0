// Filtered link ranks (include/npi_gnn.h: npi_link_ranks, RULE F): for every query pair (source, target) how many of the targets
// the source has no known edge to score above the true one, how many tie with it and how many there are -- what MRR, Hits@K and
// mean rank in the filtered setting are made of -- without the score matrix ever leaving the chip.  Two kernels:
//   link_rank_tiles_kernel   grid (blocks of 64 queries) x (S column splits).  The scan is score_tile.h's, the one topk.hip
//                            walks: per tile of 128 targets the 64 x 128 scores on v_mfma_f32_32x32x2_f32 as KEYS (rank_key.h) in
//                            LDS, the excluded columns and the loop column marked.  Before its first tile the workgroup runs the
//                            same k-loop on the 64 gathered rows z_dst[target]: element (r, r) is row r's THRESHOLD key, from the
//                            matrix cores like every key it is compared with; a wavefront keeps the keys and targets of its 16
//                            rows across 16 lanes of two registers (v_readlane per row, no LDS round trip).  The consumer here
//                            COUNTS: a wavefront marks column `target` of its row, then each lane compares its two keys of the
//                            row with the threshold and adds to the row's four counters (greater, equal, equal with a smaller
//                            id, candidates), kept in registers for the wavefront's 16 rows across all tiles of the split.  One
//                            wave reduction per row and counter at the end; each (row, split) writes four int32 partial counts
//                            to the workspace.
//   link_rank_finish_kernel  one thread per query: the S partial counts summed in int64, the score rebuilt from the key.
// Counts are integers: exact, order-free, no atomics but the status OR.  LDS: 2 x 27 KiB staging + 34 KiB keys + 1.25 KiB row
// state = 89.25 KiB, one workgroup per CU.
#include "rank_key.h"
#include "score_tile.h"

namespace npi {

constexpr int LR_COUNTS = 4;                             // greater, equal, equal_before, candidates

// the counting consumer of score_tile.h's scan
struct LinkRankCount {
    static constexpr bool UNROLL_ROWS = true;
    uint32_t v_thr;                                      // lane rr (mod 16): the threshold key of the wavefront's row rr ...
    int v_tid;                                           // ... and its target id: wave-uniform per row by v_readlane, no LDS round trip
    uint32_t n[TK_ROWS_PER_WAVE][LR_COUNTS];             // this lane's share of the counts of the wavefront's rows
    int bad_score;

    __device__ __forceinline__ void threshold(const ScoreTileShared& sh, int wave, int lane) {
        const int r = wave * TK_ROWS_PER_WAVE + (lane & (TK_ROWS_PER_WAVE - 1));
        v_thr = sh.keys[r * TK_SPITCH + r];
        v_tid = sh.tid[r];
    }
    __device__ __forceinline__ void row(int rr, int, uint32_t* krow, int c0, int cn, int lane) {
        const int tq = __builtin_amdgcn_readlane(v_tid, rr);
        const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)v_thr, rr);
        if (lane == 0 && tq - c0 >= 0 && tq - c0 < cn) krow[tq - c0] = TK_KEY_OUT;        // the target is no competitor of its own
#pragma unroll
        for (int h = 0; h < TK_BN / WAVE; ++h) {
            const uint32_t key = krow[h * WAVE + lane];
            const bool eq = key == th;
            bad_score |= key == TK_KEY_NAN ? 1 : 0;
            n[rr][0] += key < th ? 1u : 0u;
            n[rr][1] += eq ? 1u : 0u;
            n[rr][2] += eq && c0 + h * WAVE + lane < tq ? 1u : 0u;
            n[rr][3] += key <= TK_KEY_LAST ? 1u : 0u;
        }
    }
};

template <bool VEC>
__global__ void __launch_bounds__(TK_THREADS, 1)
link_rank_tiles_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int Q, const float* __restrict__ zs,
                       int64_t lds_, int n_src, const float* __restrict__ zd, int64_t ldd, int n_dst, int F,
                       const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int no_loops, int tiles_per_split,
                       uint32_t* __restrict__ partial, uint32_t* __restrict__ tkey, int32_t* __restrict__ status) {
    __shared__ ScoreTileShared sh;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = uniform_i(t >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * TK_BM;
    const int S = gridDim.y, split = blockIdx.y;

    const ScoreTileArgs args{src, dst, Q, zs, lds_, n_src, zd, ldd, n_dst, F, ex_rowptr, ex_col, no_loops, tiles_per_split, status};
    LinkRankCount count;
    count.v_thr = TK_KEY_OUT;
    count.v_tid = -1;
    count.bad_score = 0;
#pragma unroll
    for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr)
#pragma unroll
        for (int c = 0; c < LR_COUNTS; ++c) count.n[rr][c] = 0u;
    score_tiles<VEC, true>(args, sh, count);
    if (status != nullptr && __any(count.bad_score) && lane == 0) atomicOr(status, NPI_STATUS_BAD_SCORE);

    // ---- the partial counts: partial[(row * S + split) * 4 + c]; split 0 also leaves the row's key (TK_KEY_OUT: a bad pair)
#pragma unroll
    for (int rr = 0; rr < TK_ROWS_PER_WAVE; ++rr) {
        uint32_t mine = 0u;                                                       // lane c keeps counter c
#pragma unroll
        for (int c = 0; c < LR_COUNTS; ++c) {
            const uint32_t sum = wave_sum(count.n[rr][c]);
            if (lane == c) mine = sum;
        }
        const int r = wave * TK_ROWS_PER_WAVE + rr;
        if (m0 + r < Q) {
            if (lane < LR_COUNTS) partial[((m0 + r) * S + split) * LR_COUNTS + lane] = mine;
        }
    }
    if (split == 0 && lane < TK_ROWS_PER_WAVE) {
        const int r = wave * TK_ROWS_PER_WAVE + lane;
        if (m0 + r < Q) tkey[m0 + r] = sh.qid[r] >= 0 ? count.v_thr : TK_KEY_OUT;
    }
}

__global__ void __launch_bounds__(TK_THREADS)
link_rank_finish_kernel(const uint32_t* __restrict__ partial, const uint32_t* __restrict__ tkey, int Q, int S,
                        int64_t* __restrict__ counts, float* __restrict__ scores, int32_t* __restrict__ status) {
    const int64_t q = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
    if (q >= Q) return;
    const uint32_t key = tkey[q];
    int64_t n[LR_COUNTS] = {-1, -1, -1, -1};
    float score = __uint_as_float(0xff800000u);
    if (key <= TK_KEY_LAST) {
#pragma unroll
        for (int c = 0; c < LR_COUNTS; ++c) n[c] = 0;
        for (int s = 0; s < S; ++s) {
            const uint4 p = *reinterpret_cast<const uint4*>(partial + (q * S + s) * LR_COUNTS);
            n[0] += p.x;
            n[1] += p.y;
            n[2] += p.z;
            n[3] += p.w;
        }
        score = rank_score(key);
    } else if (key == TK_KEY_NAN && status != nullptr) {
        atomicOr(status, NPI_STATUS_BAD_SCORE);                                   // a NaN target score: the row of a bad pair
    }
#pragma unroll
    for (int c = 0; c < LR_COUNTS; ++c) counts[q * LR_COUNTS + c] = n[c];
    scores[q] = score;
}

// the partial counts of every (query, split), then the queries' keys
static int64_t link_rank_partial_bytes(int64_t Q, int64_t S) { return max(Q, (int64_t)1) * S * LR_COUNTS * (int64_t)sizeof(uint32_t); }

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_link_ranks_workspace_bytes(int64_t Q, int64_t n_dst, int64_t splits) {
    if (!count_ok(Q) || !count_ok(n_dst) || splits < 0) return -1;
    return align_up(link_rank_partial_bytes(Q, topk_splits(Q, n_dst, splits)) + max(Q, (int64_t)1) * (int64_t)sizeof(uint32_t), 16);
}

extern "C" int npi_link_ranks(const int64_t* src, const int64_t* dst, int64_t Q, const float* z_src, int64_t ld_src, int64_t n_src,
                              const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F, const int32_t* ex_rowptr,
                              const int32_t* ex_col, int flags, int64_t splits, int64_t* counts, float* scores, void* workspace,
                              int64_t workspace_bytes, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(Q) && count_ok(n_src) && count_ok(n_dst) && F > 0 && F < NPI_INDEX_LIMIT && ld_src >= F && ld_dst >= F,
                "npi_link_ranks: bad size (Q, n_src, n_dst in [0, 2^31 - 1), F in [1, 2^31 - 1), pitches >= F)");
    NPI_REQUIRE((flags & ~NPI_LINK_RANK_NO_LOOPS) == 0, "npi_link_ranks: unknown flag");
    NPI_REQUIRE(!(flags & NPI_LINK_RANK_NO_LOOPS) || n_src == n_dst,
                "npi_link_ranks: NPI_LINK_RANK_NO_LOOPS belongs to one id space (n_src == n_dst)");
    NPI_REQUIRE((ex_rowptr == nullptr) == (ex_col == nullptr), "npi_link_ranks: the exclusion set is ex_rowptr and ex_col together, or both NULL");
    NPI_REQUIRE(splits >= 0, "npi_link_ranks: splits must be 0 (choose) or positive");
    if (Q == 0) return NPI_OK;
    NPI_REQUIRE(src && dst && counts && scores && workspace && (z_src || n_src == 0) && (z_dst || n_dst == 0), "npi_link_ranks: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace % 16) == 0 && workspace_bytes >= npi_link_ranks_workspace_bytes(Q, n_dst, splits),
                "npi_link_ranks: the workspace is misaligned or shorter than npi_link_ranks_workspace_bytes(Q, n_dst, splits)");
    const int64_t per = max(ceil_div(topk_tiles(n_dst), topk_splits(Q, n_dst, splits)), (int64_t)1);     // tiles per split
    const int64_t S = max(ceil_div(topk_tiles(n_dst), per), (int64_t)1);                                  // no split without a tile
    const dim3 grid((unsigned)ceil_div(Q, TK_BM), (unsigned)S);
    const bool vec = rows16(z_src, ld_src, F) && rows16(z_dst, ld_dst, F);
    uint32_t* partial = static_cast<uint32_t*>(workspace);
    uint32_t* tkey = partial + link_rank_partial_bytes(Q, S) / (int64_t)sizeof(uint32_t);
#define NPI_LINK_RANK_TILES(V)                                                                                                        \
    link_rank_tiles_kernel<V><<<grid, TK_THREADS, 0, stream>>>(src, dst, (int)Q, z_src, ld_src, (int)n_src, z_dst, ld_dst, (int)n_dst, \
                                                               (int)F, ex_rowptr, ex_col, flags & NPI_LINK_RANK_NO_LOOPS, (int)per,   \
                                                               partial, tkey, status)
    if (vec) NPI_LINK_RANK_TILES(true); else NPI_LINK_RANK_TILES(false);
#undef NPI_LINK_RANK_TILES
    const int rc = check_launch("npi_link_ranks");
    if (rc != NPI_OK) return rc;
    link_rank_finish_kernel<<<(unsigned)ceil_div(Q, TK_THREADS), TK_THREADS, 0, stream>>>(partial, tkey, (int)Q, (int)S, counts, scores,
                                                                                            status);
    return check_launch("npi_link_ranks");
}
