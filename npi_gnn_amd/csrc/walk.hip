// Random walks on the device and the pair list of the skip-gram loss over them.  Replaces the reference's offline feature step
// node2vec-master/src/main.py (alias-sampled walks, then gensim) and PyG 1.4.2 `torch_geometric.nn.models.Node2Vec` over
// `torch_cluster.random_walk`: the walks by rejection (no alias tables), the pairs in the layout npi_pair_score takes.
//
// RULE W (include/npi_gnn.h states it).  Wrapping uint64 throughout; mix64, G, C, mulhi and the row search are draw.h's:
//     root = mix64(mix64(key) + 3 G);  base_w = mix64(root ^ (w C));  word(i) = mix64(base_w + G i),  i = 1, 2, ...
// Attempt n (counted over the WHOLE walk) draws pick = word(2n + 1), accept = word(2n + 2); the candidate col[rowptr[v] + mulhi(pick, d)]
// is accepted iff (accept >> 32) < thr, thr one of three integers in [0, 2^32] chosen by where the candidate lies relative to the
// previous node (the same node / a neighbour of it: a binary search of its SORTED by-source row / neither).  No float anywhere.
// One lane per walk, grid-stride: a chain of dependent gathers, few registers, no LDS; the kernel relies on occupancy.
#include "draw.h"

namespace npi {

constexpr int WALK_BLOCK = 256;
constexpr uint64_t WALK_ONE = (uint64_t)1 << 32;           // the threshold that accepts every word

// UNIFORM: all three thresholds are 2^32 -- every first attempt is accepted, so neither the accept word nor the search is needed
// and step t uses word(2t - 1): the same walks as the general kernel gives for these thresholds.
template <bool UNIFORM>
__global__ void __launch_bounds__(WALK_BLOCK)
random_walk_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, const int64_t* __restrict__ start,
                   int64_t W, int64_t L, uint64_t root, uint64_t thr_ret, uint64_t thr_nbr, uint64_t thr_far, int tries,
                   int64_t* __restrict__ walks, int32_t* __restrict__ status) {
    const int64_t nt = (int64_t)gridDim.x * WALK_BLOCK;
    const bool search = thr_nbr != thr_far;                // equal thresholds: membership does not change the verdict
    int bits = 0;
    for (int64_t w = (int64_t)blockIdx.x * WALK_BLOCK + threadIdx.x; w < W; w += nt) {
        int64_t* __restrict__ row = walks + w * (L + 1);
        const int64_t s = start[w];
        if (s < 0 || s >= N) {                             // reported, never dereferenced
            bits |= NPI_STATUS_BAD_SOURCE_ID;
            for (int64_t t = 0; t <= L; ++t) row[t] = -1;
            continue;
        }
        const uint64_t base = draw_stream(root, (uint64_t)w);
        uint64_t n = 0;                                    // attempts made so far, over the whole walk
        int32_t prev = -1, v = (int32_t)s;
        row[0] = s;
        for (int64_t t = 1; t <= L; ++t) {
            const int lo = rowptr[v];
            const int d = rowptr[v + 1] - lo;
            int32_t x = v;                                 // a dead end: the walk stays, no word is consumed
            if (d > 0) {
                if constexpr (UNIFORM) {
                    x = col[lo + (int)draw_below(draw_word(base, 2 * n + 1), (uint64_t)d)];
                    ++n;
                } else {
                    bool ok = false;
                    for (int a = 0; a < tries && !ok; ++a, ++n) {
                        const uint64_t pick = draw_word(base, 2 * n + 1);
                        const uint64_t accept = draw_word(base, 2 * n + 2);
                        x = col[lo + (int)draw_below(pick, (uint64_t)d)];
                        uint64_t thr = WALK_ONE;
                        if (t > 1) {
                            if (x == prev) thr = thr_ret;
                            else thr = (search && row_has(rowptr, col, prev, x)) ? thr_nbr : thr_far;
                        }
                        ok = (accept >> 32) < thr;
                    }
                    if (!ok) bits |= NPI_STATUS_WALK_TRIES;    // the last candidate is taken
                }
            }
            prev = v;
            v = x;
            row[t] = x;
        }
    }
    if (bits != 0 && status != nullptr) atomicOr(status, bits);
}

// One lane per pair m of the M = R (c - 1 + S) pairs, R = J W window rows, row r = j W + w (PyG's torch.cat(walks, dim=0) order).
// Every count here stays below 2^31 - 1 (checked by the entry point), so the divisions are 32-bit.
__global__ void __launch_bounds__(WALK_BLOCK)
walk_pairs_kernel(const int64_t* __restrict__ walks, uint32_t W, int64_t L, uint32_t c1, uint32_t S, int64_t N, uint64_t nbase,
                  uint32_t n_pos, uint32_t M, int64_t* __restrict__ src, int64_t* __restrict__ dst) {
    const uint32_t nt = gridDim.x * WALK_BLOCK;
    for (uint32_t m = blockIdx.x * WALK_BLOCK + threadIdx.x; m < M; m += nt) {
        uint32_t r, k = 0;
        const bool pos = m < n_pos;
        if (pos) {
            r = m / c1;
            k = m - r * c1 + 1;
        } else {
            r = (m - n_pos) / S;
        }
        const uint32_t j = r / W, w = r - j * W;
        const int64_t* __restrict__ row = walks + (int64_t)w * (L + 1) + j;
        src[m] = row[0];
        dst[m] = pos ? row[k] : (int64_t)draw_below(draw_word(nbase, (uint64_t)(m - n_pos + 1)), (uint64_t)N);
    }
}

}  // namespace npi

using namespace npi;

extern "C" int npi_random_walk(const int32_t* rowptr, const int32_t* col, int64_t N, const int64_t* start, int64_t W, int64_t L,
                               int64_t key, int64_t thr_ret, int64_t thr_nbr, int64_t thr_far, int64_t tries, int64_t* walks,
                               int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(W), "npi_random_walk: bad walk count");
    NPI_REQUIRE(count_ok(L), "npi_random_walk: bad walk length");
    NPI_REQUIRE(id_bound_ok(N), "npi_random_walk: bad id bound");
    NPI_REQUIRE(tries >= 1 && tries < NPI_INDEX_LIMIT, "npi_random_walk: tries below 1");
    NPI_REQUIRE((uint64_t)thr_ret <= WALK_ONE && (uint64_t)thr_nbr <= WALK_ONE && (uint64_t)thr_far <= WALK_ONE,
                "npi_random_walk: a threshold outside [0, 2^32]");
    NPI_REQUIRE(rowptr && col, "npi_random_walk: null pointer");
    if (W == 0) return NPI_OK;
    NPI_REQUIRE(start && walks, "npi_random_walk: null pointer");
    const uint64_t root = draw_root(key, DRAW_RULE_W);
    const unsigned grid = stride_grid(W, WALK_BLOCK, 2048);
    if ((uint64_t)thr_ret == WALK_ONE && (uint64_t)thr_nbr == WALK_ONE && (uint64_t)thr_far == WALK_ONE)
        random_walk_kernel<true><<<grid, WALK_BLOCK, 0, stream>>>(rowptr, col, N, start, W, L, root, thr_ret, thr_nbr, thr_far, (int)tries,
                                                                  walks, status);
    else
        random_walk_kernel<false><<<grid, WALK_BLOCK, 0, stream>>>(rowptr, col, N, start, W, L, root, thr_ret, thr_nbr, thr_far, (int)tries,
                                                                   walks, status);
    return check_launch("npi_random_walk");
}

extern "C" int npi_walk_pairs(const int64_t* walks, int64_t W, int64_t L, int64_t c, int64_t S, int64_t N, int64_t key, int64_t* src,
                              int64_t* dst, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(W), "npi_walk_pairs: bad walk count");
    NPI_REQUIRE(count_ok(L) && count_ok(S), "npi_walk_pairs: bad size");
    NPI_REQUIRE(id_bound_ok(N), "npi_walk_pairs: bad id bound");
    NPI_REQUIRE(c >= 2 && c <= L + 1, "npi_walk_pairs: the context size lies in [2, L + 1]");
    // M = J W (c - 1 + S): every factor is below 2^31, so the two products are taken one at a time in 64 bits
    const int64_t R = (L + 2 - c) * W;
    NPI_REQUIRE(R < NPI_INDEX_LIMIT && R * (c - 1 + S) < NPI_INDEX_LIMIT, "npi_walk_pairs: more than 2^31 - 2 pairs");
    if (W == 0) return NPI_OK;
    NPI_REQUIRE(walks && src && dst, "npi_walk_pairs: null pointer");
    const int64_t M = R * (c - 1 + S);
    const uint64_t nbase = draw_root(key, DRAW_RULE_W_NEG);
    walk_pairs_kernel<<<stride_grid(M, WALK_BLOCK, 2048), WALK_BLOCK, 0, stream>>>(walks, (uint32_t)W, L, (uint32_t)(c - 1), (uint32_t)S, N,
                                                                                   nbase, (uint32_t)(R * (c - 1)), (uint32_t)M, src, dst);
    return check_launch("npi_walk_pairs");
}
