// Ranking metrics of M scored, labelled examples (include/npi_gnn.h: npi_rank_metrics, RULE R) -- sklearn's `_binary_clf_curve`,
// `roc_auc_score` and `average_precision_score`, what PyG 1.4.2 `GAE.test` calls on the host -- as one more client of the shared
// sorter (sort.h) and six kernels of its own:
//   rank_keys_kernel    score, label -> (descending-orderable key, label) pairs; NaN scores and labels other than 0 / 1 reported
//   PairSort::sort      all 32 key bits
//   rank_totals_kernel  pass 1 over the sorted stream: positives and tie-group ends per tile of 1,024, packed into one int64
//   rank_offsets_kernel ONE workgroup: exclusive scan of the tile totals in place; the grand total (P, G) behind them
//   rank_curve_kernel   pass 2: the same tile scanned (block_exclusive_scan over the packed pair) on top of its offset; every group
//                       end writes its (threshold, TP, FP) at its group number -- the compaction
//   rank_terms_kernel   the curve read once: the U2 terms in int64, the AP terms in fp64, one partial of each per workgroup
//   rank_finish_kernel  ONE workgroup: the partials in a fixed order, then auc, ap and the four counts
// The sorted stream is read twice (16-byte lanes, plus the one key behind each lane's four), the curve written once and read once.
// No float atomics, no atomics at all but the status OR; every sum has a fixed order that depends on M alone, so the result is a
// pure function of the multiset of (score, label) pairs.  Nothing allocates or reads back.
#include "sort.h"
#include "rank_key.h"

namespace npi {

constexpr int RANK_THREADS = 256;
constexpr int RANK_WAVES = RANK_THREADS / WAVE;
constexpr int RANK_ITEMS = 4;                                   // one 16-byte lane of keys and one of labels per thread
constexpr int RANK_TILE = RANK_THREADS * RANK_ITEMS;            // 1,024 positions of the sorted stream (or of the curve) per workgroup

// rank_key / rank_score: rank_key.h (shared with topk.hip)

__global__ void __launch_bounds__(RANK_THREADS)
rank_keys_kernel(const float* __restrict__ scores, const int64_t* __restrict__ y, int M, int n_pos, uint32_t* __restrict__ keys,
                 int32_t* __restrict__ labels, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    int bad = 0;
    if (i < M) {
        const float s = scores[i];
        if (s != s) bad |= NPI_STATUS_BAD_SCORE;
        int32_t label;
        if (y != nullptr) {
            const int64_t v = y[i];
            if (v != 0 && v != 1) bad |= NPI_STATUS_BAD_LABEL;
            label = v == 1 ? 1 : 0;
        } else {
            label = i < n_pos ? 1 : 0;
        }
        keys[i] = rank_key(__float_as_uint(s));
        labels[i] = label;
    }
    if (status != nullptr) {                                    // one OR per wavefront that saw either
        const int any_score = __any(bad & NPI_STATUS_BAD_SCORE), any_label = __any(bad & NPI_STATUS_BAD_LABEL);
        const int bits = (any_score ? NPI_STATUS_BAD_SCORE : 0) | (any_label ? NPI_STATUS_BAD_LABEL : 0);
        if (bits != 0 && lane_id() == 0) atomicOr(status, bits);
    }
}

// The four positions of one thread: base = tile * RANK_TILE + 4 * thread.  pos[j] = the label, end[j] = "position base + j ends its
// tie group" (the last position, or a different key behind it); both 0 past M.  key[j] is read for the threshold.
struct RankLane {
    uint32_t key[RANK_ITEMS];
    int pos[RANK_ITEMS], end[RANK_ITEMS];
};
__device__ __forceinline__ RankLane rank_load(const uint32_t* __restrict__ keys, const int32_t* __restrict__ labels, int M, int64_t base) {
    RankLane r;
    uint32_t k[RANK_ITEMS + 1];
    int l[RANK_ITEMS];
    if (base + RANK_ITEMS <= M) {                               // 16-byte lanes: the arrays are 256-byte aligned, base a multiple of 4
        const uint4 kv = *reinterpret_cast<const uint4*>(keys + base);
        const int4 lv = *reinterpret_cast<const int4*>(labels + base);
        k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
        l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
    } else {
#pragma unroll
        for (int j = 0; j < RANK_ITEMS; ++j) {
            const bool in = base + j < M;
            k[j] = in ? keys[base + j] : 0u;
            l[j] = in ? labels[base + j] : 0;
        }
    }
    k[RANK_ITEMS] = base + RANK_ITEMS < M ? keys[base + RANK_ITEMS] : 0u;
#pragma unroll
    for (int j = 0; j < RANK_ITEMS; ++j) {
        const int64_t i = base + j;
        r.key[j] = k[j];
        r.pos[j] = i < M ? l[j] : 0;
        r.end[j] = i < M && (i == (int64_t)M - 1 || k[j] != k[j + 1]) ? 1 : 0;
    }
    return r;
}
// (positives << 32) | group ends of the four: both below 2^31, so the packed sums never carry from one half into the other
__device__ __forceinline__ long long rank_pack(const RankLane& r) {
    int p = 0, e = 0;
#pragma unroll
    for (int j = 0; j < RANK_ITEMS; ++j) { p += r.pos[j]; e += r.end[j]; }
    return ((long long)p << 32) | (long long)e;
}

__global__ void __launch_bounds__(RANK_THREADS)
rank_totals_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ labels, int M, long long* __restrict__ tile_tot) {
    __shared__ long long wsum[RANK_WAVES];
    const int64_t base = (int64_t)blockIdx.x * RANK_TILE + (int64_t)threadIdx.x * RANK_ITEMS;
    const long long v = wave_sum(rank_pack(rank_load(keys, labels, M, base)));
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tile_tot[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// tile_tot[0 .. n) -> its exclusive scan, in place; tile_tot[n] = the sum of all: (P << 32) | G
__global__ void __launch_bounds__(RANK_THREADS)
rank_offsets_kernel(long long* __restrict__ tile_tot, int n) {
    __shared__ long long lds[RANK_THREADS];
    long long carry = 0;
    for (int base = 0; base < n; base += RANK_THREADS) {
        const int i = base + (int)threadIdx.x;
        const long long v = i < n ? tile_tot[i] : 0;
        long long total;
        const long long excl = block_exclusive_scan<RANK_THREADS>(v, lds, &total);
        if (i < n) tile_tot[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) tile_tot[n] = carry;
}

// Group g = the number of group ends in front of a position; its end writes thr[g] / tps[g] / fps[g].  thr may be NULL (the
// entry point's own curve: the metrics need the counts only).
__global__ void __launch_bounds__(RANK_THREADS)
rank_curve_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ labels, int M, const long long* __restrict__ tile_off,
                  float* __restrict__ thr, int32_t* __restrict__ tps, int32_t* __restrict__ fps) {
    __shared__ long long lds[RANK_THREADS];
    const int64_t base = (int64_t)blockIdx.x * RANK_TILE + (int64_t)threadIdx.x * RANK_ITEMS;
    const RankLane r = rank_load(keys, labels, M, base);
    long long total;
    const long long before = tile_off[blockIdx.x] + block_exclusive_scan<RANK_THREADS>(rank_pack(r), lds, &total);
    int tp = (int)(before >> 32), g = (int)(before & 0xffffffffll);
#pragma unroll
    for (int j = 0; j < RANK_ITEMS; ++j) {
        tp += r.pos[j];
        if (r.end[j]) {                                         // g < G <= M: inside the caller's capacity
            if (thr != nullptr) thr[g] = rank_score(r.key[j]);
            tps[g] = tp;
            fps[g] = (int)(base + j + 1) - tp;
            ++g;
        }
    }
}

// Workgroup b takes curve entries [b * RANK_TILE, (b + 1) * RANK_TILE) below G, entry c * 256 + thread in its round c:
//   u2 += (FP_g - FP_{g-1}) * (TP_g + TP_{g-1})                       int64, exact
//   ap += ((TP_g - TP_{g-1}) / P) * (TP_g / (TP_g + FP_g))            fp64, each lane its rounds in order
// then a wavefront its 64 lanes in a fixed tree and the workgroup its four wavefronts in order (pair_score.hip's scheme).
__global__ void __launch_bounds__(RANK_THREADS)
rank_terms_kernel(const int32_t* __restrict__ tps, const int32_t* __restrict__ fps, const long long* __restrict__ grand,
                  double* __restrict__ ap_part, long long* __restrict__ u2_part) {
    __shared__ double wap[RANK_WAVES];
    __shared__ long long wu2[RANK_WAVES];
    const long long pg = grand[0];
    const int G = (int)(pg & 0xffffffffll);
    const double P = (double)(int)(pg >> 32);
    double ap = 0.0;
    long long u2 = 0;
#pragma unroll
    for (int c = 0; c < RANK_ITEMS; ++c) {
        const int64_t g = (int64_t)blockIdx.x * RANK_TILE + c * RANK_THREADS + threadIdx.x;
        if (g < G) {
            const int tp = tps[g], fp = fps[g];
            const int tp0 = g > 0 ? tps[g - 1] : 0, fp0 = g > 0 ? fps[g - 1] : 0;
            u2 += (long long)(fp - fp0) * ((long long)tp + (long long)tp0);
            ap += ((double)(tp - tp0) / P) * ((double)tp / ((double)tp + (double)fp));
        }
    }
    ap = wave_sum(ap);
    u2 = wave_sum(u2);
    if (lane_id() == 0) { wap[threadIdx.x >> 6] = ap; wu2[threadIdx.x >> 6] = u2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ap_part[blockIdx.x] = ((wap[0] + wap[1]) + wap[2]) + wap[3];
        u2_part[blockIdx.x] = ((wu2[0] + wu2[1]) + wu2[2]) + wu2[3];
    }
}

// thread t adds partials t, t + 256, ... in order, then a fixed tree over the workgroup; result = (auc, ap), counts = (P, N, G, U2)
__global__ void __launch_bounds__(RANK_THREADS)
rank_finish_kernel(const double* __restrict__ ap_part, const long long* __restrict__ u2_part, int n, const long long* __restrict__ grand,
                   int M, double* __restrict__ result, int64_t* __restrict__ counts) {
    __shared__ double sap[RANK_THREADS];
    __shared__ long long su2[RANK_THREADS];
    double ap = 0.0;
    long long u2 = 0;
    for (int i = threadIdx.x; i < n; i += RANK_THREADS) { ap += ap_part[i]; u2 += u2_part[i]; }
    sap[threadIdx.x] = ap;
    su2[threadIdx.x] = u2;
    __syncthreads();
    for (int s = RANK_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) { sap[threadIdx.x] += sap[threadIdx.x + s]; su2[threadIdx.x] += su2[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long pg = grand[0];
        const long long P = pg >> 32, G = pg & 0xffffffffll, N = (long long)M - P;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        result[0] = (P == 0 || N == 0) ? nan : (double)su2[0] / (2.0 * (double)P * (double)N);
        result[1] = P == 0 ? nan : sap[0];
        counts[0] = P; counts[1] = N; counts[2] = G; counts[3] = su2[0];
    }
}

static int64_t rank_tiles(int64_t M) { return ceil_div(M > 0 ? M : 1, RANK_TILE); }
// behind the sorter's part: tile totals [tiles + 1] int64, AP partials [tiles] fp64, U2 partials [tiles] int64
static int64_t rank_tail_bytes(int64_t M) { return align_up((rank_tiles(M) + 1) * 8, 256) + 2 * align_up(rank_tiles(M) * 8, 256); }

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_rank_workspace_bytes(int64_t M) {
    if (!count_ok(M)) return -1;
    return align_up(PairSort::bytes(M), 256) + rank_tail_bytes(M);
}

extern "C" int npi_rank_metrics(const float* scores, const int64_t* y, int64_t M, int64_t n_pos, double* result, int64_t* counts,
                                float* thr, int32_t* tps, int32_t* fps, int32_t* status, void* workspace, int64_t workspace_bytes,
                                void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(M), "npi_rank_metrics: bad size (M must lie in [0, 2^31 - 1))");
    NPI_REQUIRE(y != nullptr || (n_pos >= 0 && n_pos <= M), "npi_rank_metrics: n_pos outside [0, M] (it names the positives when y is NULL)");
    NPI_REQUIRE(result && counts, "npi_rank_metrics: null pointer (result and counts are required)");
    NPI_REQUIRE((thr && tps && fps) || (!thr && !tps && !fps), "npi_rank_metrics: the curve is thr, tps and fps together, or all three NULL");
    if (M == 0) {                                               // no example, no kernel: NaN, NaN (all bits set) and zero counts by the runtime
        hipError_t e = hipMemsetAsync(result, 0xff, 2 * sizeof(double), stream);
        if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), stream);
        if (e != hipSuccess) {
            set_error("npi_rank_metrics: %s", hipGetErrorString(e));
            return NPI_ERR_LAUNCH;
        }
        return NPI_OK;
    }
    NPI_REQUIRE(scores && workspace, "npi_rank_metrics: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace % 16) == 0 && workspace_bytes >= npi_rank_workspace_bytes(M),
                "npi_rank_metrics: the workspace is misaligned or shorter than npi_rank_workspace_bytes(M)");
    PairSort ps;
    const int64_t sort_bytes = align_up(PairSort::bytes(M), 256);
    (void)ps.carve(workspace, sort_bytes, M);                   // (the length was checked above)
    const int64_t nt = rank_tiles(M);
    char* tail = (char*)workspace + sort_bytes;
    long long* tile_tot = (long long*)tail;
    double* ap_part = (double*)(tail + align_up((nt + 1) * 8, 256));
    long long* u2_part = (long long*)(tail + align_up((nt + 1) * 8, 256) + align_up(nt * 8, 256));
    const unsigned tiles = (unsigned)nt;

    rank_keys_kernel<<<(unsigned)ceil_div(M, RANK_THREADS), RANK_THREADS, 0, stream>>>(scores, y, (int)M, (int)n_pos, ps.keys_a, ps.vals_a,
                                                                                      status);
    ps.sort(32, stream);
    // the sorter's free pair: the curve's counts when the caller takes no curve
    int32_t* ctps = tps ? tps : ps.vals_b;
    int32_t* cfps = fps ? fps : (int32_t*)ps.keys_b;
    rank_totals_kernel<<<tiles, RANK_THREADS, 0, stream>>>(ps.keys_a, ps.vals_a, (int)M, tile_tot);
    rank_offsets_kernel<<<1, RANK_THREADS, 0, stream>>>(tile_tot, (int)nt);
    rank_curve_kernel<<<tiles, RANK_THREADS, 0, stream>>>(ps.keys_a, ps.vals_a, (int)M, tile_tot, thr, ctps, cfps);
    rank_terms_kernel<<<tiles, RANK_THREADS, 0, stream>>>(ctps, cfps, tile_tot + nt, ap_part, u2_part);
    rank_finish_kernel<<<1, RANK_THREADS, 0, stream>>>(ap_part, u2_part, (int)nt, tile_tot + nt, (int)M, result, counts);
    return check_launch("npi_rank_metrics");
}
