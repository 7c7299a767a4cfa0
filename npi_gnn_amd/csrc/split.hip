// Edge splits on the device: one edge list -> a random order of its kept columns, whose contiguous ranges are the train / val / test
// parts or the k folds of a link-prediction run, and the undirected form a training graph is handed over in.  Replaces PyG 1.4.2
// `train_test_split_edges` (host `torch.randperm`, a dense [N, N] mask for the held-out negatives, `to_undirected` through
// `torch_sparse.coalesce`) and the reference's 5-fold key split (src/generate_edgelist.py:460-494, src/train.py:108-184).
//
// RULE S (include/npi_gnn.h states it).  Wrapping uint64, mix64 / G are draw.h's:
//     base = mix64(mix64(mix64(key) + 5 G));   r_e = mix64(base + G (e + 1)),   e = the column's index in the INPUT
// The kept columns (both ids in range; with `upper` also src < dst) come out in ascending (r_e, e).  npi_split_permute:
//   split_keep_kernel     keep flag per column; an id out of range is reported, never dereferenced
//   exclusive_scan_i32    the flags -> positions (E + 1 words: the last one is K)
//   split_compact_kernel  a stable partition: kept column e -> pair (low 32 bits of r_e, e) at its position, a dropped one -> a
//                         padding pair (0xFFFFFFFF, -1) behind all K kept ones.  The host does not know K, so the sorter runs over all
//                         E pairs; padding that STARTS behind the kept pairs and carries the largest key in both rounds STAYS behind
//                         them (the sorts are stable), whatever r_e the kept ones have
//   PairSort::sort        32 bits;  split_rekey_kernel: the high 32 bits of r_e from the carried e;  PairSort::sort, 32 bits
//   split_gather_kernel   position p < K: out_src / out_dst / e_id[p], three coalesced int64 stores
// npi_split_canonical rewrites Rule P's candidates (s, d) as (min, max) for the held-out negatives of one id space;
// npi_split_undirected writes both orientations as int32 pairs and hands them to npi_sample_coalesce (sample.hip).
// One lane per entry, grid-stride; integers only; the one atomic is the status OR.  Nothing allocates or keeps state.
#include "draw.h"
#include "sort.h"

namespace npi {

constexpr int SPLIT_BLOCK = 256;

__device__ __forceinline__ uint64_t split_word(uint64_t base, int32_t e) { return draw_word(base, (uint64_t)e + 1); }

__device__ __forceinline__ bool split_in_range(int64_t s, int64_t d, int64_t n_src, int64_t n_dst) {
    return s >= 0 && s < n_src && d >= 0 && d < n_dst;
}

// flag[e] = 1 for a kept column, flag[E] = 0: the exclusive scan over E + 1 words then ends in K
__global__ void __launch_bounds__(SPLIT_BLOCK)
split_keep_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, int64_t n_src, int64_t n_dst, int upper,
                  int32_t* __restrict__ flag, int32_t* __restrict__ status) {
    const int64_t nt = (int64_t)gridDim.x * SPLIT_BLOCK;
    int bad = 0;
    for (int64_t e = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x; e <= E; e += nt) {
        int keep = 0;
        if (e < E) {
            const int64_t s = src[e], d = dst[e];
            const bool in = split_in_range(s, d, n_src, n_dst);
            if (!in) bad = NPI_STATUS_BAD_PAIR_ID;
            keep = in && !(upper && s >= d) ? 1 : 0;
        }
        flag[e] = keep;
    }
    if (bad != 0 && status != nullptr) atomicOr(status, bad);
}

// pos = the scanned flags (pos[E] = K).  Column e is kept iff pos[e + 1] != pos[e]; the dropped ones keep their order behind K
__global__ void __launch_bounds__(SPLIT_BLOCK)
split_compact_kernel(const int32_t* __restrict__ pos, int64_t E, uint64_t base, uint32_t* __restrict__ keys, int32_t* __restrict__ vals,
                     int32_t* __restrict__ info) {
    const int64_t nt = (int64_t)gridDim.x * SPLIT_BLOCK;
    const int32_t K = pos[E];
    for (int64_t e = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x; e < E; e += nt) {
        const int32_t q = pos[e];
        const bool kept = pos[e + 1] != q;
        const int64_t p = kept ? (int64_t)q : (int64_t)K + (e - q);          // p < E either way
        keys[p] = kept ? (uint32_t)split_word(base, (int32_t)e) : 0xFFFFFFFFu;
        vals[p] = kept ? (int32_t)e : -1;
        if (e == 0) info[0] = K;
    }
}

__global__ void __launch_bounds__(SPLIT_BLOCK)
split_rekey_kernel(const int32_t* __restrict__ vals, int64_t E, uint64_t base, uint32_t* __restrict__ keys) {
    const int64_t nt = (int64_t)gridDim.x * SPLIT_BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x; p < E; p += nt) {
        const int32_t e = vals[p];
        keys[p] = e >= 0 ? (uint32_t)(split_word(base, e) >> 32) : 0xFFFFFFFFu;
    }
}

// the padding pairs lie behind the K kept ones: every p with vals[p] >= 0 is below K, inside what the caller sized with the bound E
__global__ void __launch_bounds__(SPLIT_BLOCK)
split_gather_kernel(const int32_t* __restrict__ vals, int64_t E, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                    int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst, int64_t* __restrict__ e_id) {
    const int64_t nt = (int64_t)gridDim.x * SPLIT_BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x; p < E; p += nt) {
        const int32_t e = vals[p];
        if (e < 0) continue;
        out_src[p] = src[e];
        out_dst[p] = dst[e];
        e_id[p] = e;
    }
}

// (s, d) -> (min, max); an invalid candidate (-1, -1) stays as it is
__global__ void __launch_bounds__(SPLIT_BLOCK)
split_canonical_kernel(int32_t* __restrict__ cand_src, int32_t* __restrict__ cand_dst, int64_t W) {
    const int64_t nt = (int64_t)gridDim.x * SPLIT_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x; j < W; j += nt) {
        const int32_t s = cand_src[j], d = cand_dst[j];
        if (s > d) {
            cand_src[j] = d;
            cand_dst[j] = s;
        }
    }
}

// entries 2e and 2e + 1 = column e as it is and turned round, both carrying e.  A column with an id outside [0, N) becomes the pair
// (N, N) twice: one id above every real one, so it sorts last and split_trim_kernel takes it off again
__global__ void __launch_bounds__(SPLIT_BLOCK)
split_orient_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, int64_t N, int32_t* __restrict__ row,
                    int32_t* __restrict__ col, int32_t* __restrict__ eid, int32_t* __restrict__ status) {
    const int64_t nt = (int64_t)gridDim.x * SPLIT_BLOCK;
    int bad = 0;
    for (int64_t e = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x; e < E; e += nt) {
        const int64_t s = src[e], d = dst[e];
        const bool in = split_in_range(s, d, N, N);
        if (!in) bad = NPI_STATUS_BAD_PAIR_ID;
        const int32_t a = in ? (int32_t)s : (int32_t)N, b = in ? (int32_t)d : (int32_t)N;
        *reinterpret_cast<int2*>(row + 2 * e) = make_int2(a, b);
        *reinterpret_cast<int2*>(col + 2 * e) = make_int2(b, a);
        *reinterpret_cast<int2*>(eid + 2 * e) = make_int2((int32_t)e, (int32_t)e);
    }
    if (bad != 0 && status != nullptr) atomicOr(status, bad);
}
__global__ void split_trim_kernel(const int64_t* __restrict__ out_src, int64_t N, int32_t* __restrict__ info) {
    const int32_t n = info[0];
    if (threadIdx.x == 0 && blockIdx.x == 0 && n > 0 && out_src[n - 1] == N) info[0] = n - 1;
}

// the flags / positions behind the sorter's part of the workspace
static int64_t split_sort_bytes(int64_t E) { return align_up(PairSort::bytes(E), 256); }
static int64_t split_words_bytes(int64_t n) { return align_up((n > 0 ? n : 1) * 4, 256); }

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_split_workspace_bytes(int64_t E) {
    if (!count_ok(E)) return -1;
    return split_sort_bytes(E) + split_words_bytes(E + 1);
}

extern "C" int npi_split_permute(const int64_t* src, const int64_t* dst, int64_t E, int64_t n_src, int64_t n_dst, int64_t key, int flags,
                                 int64_t* out_src, int64_t* out_dst, int64_t* e_id, int32_t* info, int32_t* status, void* workspace,
                                 int64_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(E), "npi_split_permute: bad size (E must lie in [0, 2^31 - 1))");
    NPI_REQUIRE(id_bound_ok(n_src) && id_bound_ok(n_dst), "npi_split_permute: bad id bound");
    NPI_REQUIRE((flags & ~NPI_SPLIT_UPPER) == 0, "npi_split_permute: unknown flag");
    NPI_REQUIRE(info, "npi_split_permute: null pointer (info is required)");
    if (E == 0) {
        if (hipMemsetAsync(info, 0, sizeof(int32_t), stream) != hipSuccess) return check_launch("npi_split_permute");
        return NPI_OK;
    }
    NPI_REQUIRE(src && dst && out_src && out_dst && e_id && workspace, "npi_split_permute: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace & 15) == 0, "npi_split_permute: workspace must be 16-byte aligned");
    if (workspace_short("npi_split_permute", workspace_bytes, npi_split_workspace_bytes(E))) return NPI_ERR_ARG;
    PairSort ps;
    (void)ps.carve(workspace, split_sort_bytes(E), E);          // (the length was checked above)
    int32_t* pos = (int32_t*)((char*)workspace + split_sort_bytes(E));
    const uint64_t base = mix64(draw_root(key, DRAW_RULE_S));     // Rule S alone mixes its root once more
    const unsigned grid = stride_grid(E + 1, SPLIT_BLOCK, 2048);

    split_keep_kernel<<<grid, SPLIT_BLOCK, 0, stream>>>(src, dst, E, n_src, n_dst, flags & NPI_SPLIT_UPPER, pos, status);
    exclusive_scan_i32(pos, E + 1, ps.counts, stream);          // (the sorter's histograms are free until the first sort)
    split_compact_kernel<<<grid, SPLIT_BLOCK, 0, stream>>>(pos, E, base, ps.keys_a, ps.vals_a, info);
    ps.sort(32, stream);
    split_rekey_kernel<<<grid, SPLIT_BLOCK, 0, stream>>>(ps.vals_a, E, base, ps.keys_a);
    ps.sort(32, stream);
    split_gather_kernel<<<grid, SPLIT_BLOCK, 0, stream>>>(ps.vals_a, E, src, dst, out_src, out_dst, e_id);
    return check_launch("npi_split_permute");
}

extern "C" int npi_split_canonical(int32_t* cand_src, int32_t* cand_dst, int64_t W, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(W), "npi_split_canonical: bad window size");
    if (W == 0) return NPI_OK;
    NPI_REQUIRE(cand_src && cand_dst, "npi_split_canonical: null pointer");
    split_canonical_kernel<<<stride_grid(W, SPLIT_BLOCK, 2048), SPLIT_BLOCK, 0, stream>>>(cand_src, cand_dst, W);
    return check_launch("npi_split_canonical");
}

// 2 E entries go through the coalesce: both have to stay below 2^31 - 1, and so has the id N of the placeholder pair
static bool undirected_size_ok(int64_t E) { return E >= 0 && 2 * E < NPI_INDEX_LIMIT; }

extern "C" int64_t npi_split_undirected_workspace_bytes(int64_t E) {
    if (!undirected_size_ok(E)) return -1;
    return 3 * split_words_bytes(2 * E) + npi_sample_coalesce_workspace_bytes(2 * E);
}

extern "C" int npi_split_undirected(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int64_t* out_src, int64_t* out_dst,
                                    int64_t* e_id, int32_t* info, int32_t* status, void* workspace, int64_t workspace_bytes,
                                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(undirected_size_ok(E), "npi_split_undirected: bad size (2 E must lie in [0, 2^31 - 1))");
    NPI_REQUIRE(N >= 1 && N < NPI_INDEX_LIMIT - 1, "npi_split_undirected: bad id bound");
    NPI_REQUIRE(info, "npi_split_undirected: null pointer (info is required)");
    if (E == 0) {
        if (hipMemsetAsync(info, 0, sizeof(int32_t), stream) != hipSuccess) return check_launch("npi_split_undirected");
        return NPI_OK;
    }
    NPI_REQUIRE(src && dst && out_src && out_dst && e_id && workspace, "npi_split_undirected: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace & 15) == 0, "npi_split_undirected: workspace must be 16-byte aligned");
    if (workspace_short("npi_split_undirected", workspace_bytes, npi_split_undirected_workspace_bytes(E))) return NPI_ERR_ARG;
    const int64_t pitch = split_words_bytes(2 * E);
    char* ws = (char*)workspace;
    int32_t *row = (int32_t*)ws, *col = (int32_t*)(ws + pitch), *eid = (int32_t*)(ws + 2 * pitch);
    split_orient_kernel<<<stride_grid(E, SPLIT_BLOCK, 2048), SPLIT_BLOCK, 0, stream>>>(src, dst, E, N, row, col, eid, status);
    if (check_launch("npi_split_undirected") != NPI_OK) return NPI_ERR_LAUNCH;
    const int rc = npi_sample_coalesce(row, col, eid, 2 * E, N + 1, out_src, out_dst, e_id, info, ws + 3 * pitch,
                                       workspace_bytes - 3 * pitch, stream_);
    if (rc != NPI_OK) return rc;
    split_trim_kernel<<<1, 64, 0, stream>>>(out_src, N, info);
    return check_launch("npi_split_undirected");
}
