// DropEdge (Rule E, include/npi_gnn.h): seeded edge dropout as a sort-free stream compaction.
//
// A CSR side is ordered by (row, list order) and dropping entries keeps that order, so the dropped graph's two sides are the parent's
// two sides with entries removed -- no sort.  Both sides carry eid (and a symmetric (rowidx, col) pair), so the rule makes the same
// decision on both.  The compaction is parallel over ENTRIES: one wavefront per tile of DROP_TILE entries,
//   1. count      kept entries per tile (ballots)                                   -> tiles[n_tiles + 1], the last word 0
//   2. scan       exclusive_scan_i32 over the tile counts (sort.h); tiles[n_tiles] = the number kept
//   3. write      the decisions recomputed; a kept entry goes to tile base + its rank among the tile's kept entries (ballot +
//                 mbcnt, round by round), and the FIRST entry of every row -- kept or not -- leaves its new position in rowptr_o
//   4. empty rows and the tail of rowptr_o (one thread per row): an empty row takes the value of the row that owns the entry at
//                 its position, a row at or behind nnz takes the total.  Runs of empty rows of any length cost one read each.
//   5. write_item_rows
// No flag or newpos array is kept between 1 and 3: three mix64 per entry are cheaper than 4 bytes written and read back.
// npi_drop_edge_list is the same compaction over the columns of an edge list, npi_drop_edge_keep the decision itself.
#include "draw.h"
#include "sort.h"

namespace npi {

constexpr int DROP_TILE = 256;                             // entries one wavefront compacts
constexpr int DROP_ROUNDS = DROP_TILE / WAVE;              // ... in rounds of one entry per lane
constexpr int DROP_THREADS = 256;
constexpr int DROP_WAVES = DROP_THREADS / WAVE;

struct DropRule {
    uint64_t root, threshold;
    int undirected;
};

__device__ __forceinline__ uint64_t drop_root_t(uint64_t root, const int64_t* __restrict__ tick) {
    return draw_word(root, (uint64_t)(tick ? tick[0] : 0) + 1);
}
// entries of the side as the device knows them, never beyond the capacity the caller vouches for
__device__ __forceinline__ int64_t side_nnz(const int32_t* __restrict__ rowptr, int64_t N, int64_t nnz_max) {
    const int64_t n = rowptr[N];
    return n < 0 ? 0 : (n > nnz_max ? nnz_max : n);
}
// only a column of edge_index is subject to the rule: the appended self loop (eid < 0) and root entries (eid >= n_edges) stay
__device__ __forceinline__ bool side_entry_kept(uint64_t root_t, const DropRule& rule, int32_t e, int32_t r, int32_t c, int64_t n_edges) {
    if (e < 0 || e >= n_edges) return true;
    return !edge_dropped(root_t, rule.undirected != 0, e, r, c, rule.threshold);
}
__device__ __forceinline__ int lanes_before(uint64_t mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
inline int64_t drop_tiles(int64_t n) { return ceil_div(n > 0 ? n : 0, DROP_TILE); }
inline unsigned drop_grid(int64_t tiles) { return (unsigned)ceil_div(tiles, DROP_WAVES); }

// ---- a CSR side ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DROP_THREADS)
drop_side_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
                       const int32_t* __restrict__ rowidx, int64_t N, int64_t nnz_max, int64_t n_edges, DropRule rule,
                       const int64_t* __restrict__ tick, int64_t n_tiles, int32_t* __restrict__ tiles) {
    const int64_t tile = (int64_t)blockIdx.x * DROP_WAVES + (threadIdx.x >> 6);
    if (tile > n_tiles) return;
    const int lane = lane_id();
    if (tile == n_tiles) {                                 // the word behind the counts: the total, once scanned
        if (lane == 0) tiles[tile] = 0;
        return;
    }
    const int64_t nnz = side_nnz(rowptr, N, nnz_max);
    const uint64_t root_t = drop_root_t(rule.root, tick);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < DROP_ROUNDS; ++j) {
        const int64_t p = tile * DROP_TILE + j * WAVE + lane;
        bool keep = false;
        if (p < nnz) {
            const int32_t e = eid[p];
            int32_t r = 0, c = 0;
            if (rule.undirected) { r = rowidx[p]; c = col[p]; }
            keep = side_entry_kept(root_t, rule, e, r, c, n_edges);
        }
        cnt += __popcll(__ballot(keep));
    }
    if (lane == 0) tiles[tile] = cnt;
}

__global__ void __launch_bounds__(DROP_THREADS)
drop_side_write_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
                       const int32_t* __restrict__ rowidx, int64_t N, int64_t nnz_max, int64_t n_edges, DropRule rule,
                       const int64_t* __restrict__ tick, int64_t n_tiles, const int32_t* __restrict__ tiles, int64_t nnz_max_out,
                       int32_t* __restrict__ rowptr_o, int32_t* __restrict__ col_o, int32_t* __restrict__ eid_o,
                       int32_t* __restrict__ rowidx_o) {
    const int64_t tile = (int64_t)blockIdx.x * DROP_WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int lane = lane_id();
    const int64_t nnz = side_nnz(rowptr, N, nnz_max);
    if (tile * DROP_TILE >= nnz) return;
    const uint64_t root_t = drop_root_t(rule.root, tick);
    int64_t base = tiles[tile];
#pragma unroll
    for (int j = 0; j < DROP_ROUNDS; ++j) {
        const int64_t p = tile * DROP_TILE + j * WAVE + lane;
        const bool in = p < nnz;
        int32_t e = -1, r = -1, c = 0, r_prev = -1;
        if (in) {
            e = eid[p];
            r = rowidx[p];
            c = col[p];
            r_prev = p > 0 ? rowidx[p - 1] : -1;
        }
        const bool keep = in && side_entry_kept(root_t, rule, e, r, c, n_edges);
        const uint64_t mask = __ballot(keep);
        const int64_t q = base + lanes_before(mask);       // kept entries in front of p: where p goes, and where its row starts
        if (in && r != r_prev && r >= 0 && r < N) rowptr_o[r] = (int32_t)q;
        if (keep && q < nnz_max_out) {
            col_o[q] = c;
            eid_o[q] = e;
            rowidx_o[q] = r;
        }
        base += __popcll(mask);
    }
}

// rows without a first entry: empty ones (the value of the row that owns the entry at their position) and those at or behind nnz
// (the total; row N among them).  rowptr_o is read and written here: an empty row reads a NON-empty one, which pass 3 wrote.
__global__ void __launch_bounds__(256)
drop_side_rows_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rowidx, int64_t N, int64_t nnz_max,
                      const int32_t* __restrict__ tiles, int64_t n_tiles, int32_t* rowptr_o) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    const int64_t nnz = side_nnz(rowptr, N, nnz_max);
    const int32_t total = tiles[n_tiles];
    const int64_t p = rowptr[i];
    if (i == N || p < 0 || p >= nnz) { rowptr_o[i] = total; return; }
    if ((int64_t)rowptr[i + 1] != p) return;
    const int32_t r = rowidx[p];
    rowptr_o[i] = (r > i && r < N) ? rowptr_o[r] : total;
}

// ---- an edge list ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DROP_THREADS)
drop_list_count_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, DropRule rule,
                       const int64_t* __restrict__ tick, int64_t n_tiles, int32_t* __restrict__ tiles) {
    const int64_t tile = (int64_t)blockIdx.x * DROP_WAVES + (threadIdx.x >> 6);
    if (tile > n_tiles) return;
    const int lane = lane_id();
    if (tile == n_tiles) {
        if (lane == 0) tiles[tile] = 0;
        return;
    }
    const uint64_t root_t = drop_root_t(rule.root, tick);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < DROP_ROUNDS; ++j) {
        const int64_t e = tile * DROP_TILE + j * WAVE + lane;
        bool keep = false;
        if (e < E) {
            int64_t u = 0, v = 0;
            if (rule.undirected) { u = src[e]; v = dst[e]; }
            keep = !edge_dropped(root_t, rule.undirected != 0, e, u, v, rule.threshold);
        }
        cnt += __popcll(__ballot(keep));
    }
    if (lane == 0) tiles[tile] = cnt;
}

// launched over n_tiles + 1 tiles, so that the count word is written for an empty list as well
__global__ void __launch_bounds__(DROP_THREADS)
drop_list_write_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, DropRule rule,
                       const int64_t* __restrict__ tick, int64_t n_tiles, const int32_t* __restrict__ tiles,
                       int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst, int32_t* __restrict__ newpos,
                       int32_t* __restrict__ count, int pad_tail) {
    const int64_t tile = (int64_t)blockIdx.x * DROP_WAVES + (threadIdx.x >> 6);
    if (tile > n_tiles) return;
    const int lane = lane_id();
    const int64_t total = tiles[n_tiles];
    if (tile == 0 && lane == 0) count[0] = (int32_t)total;
    if (tile == n_tiles) return;
    const uint64_t root_t = drop_root_t(rule.root, tick);
    int64_t base = tiles[tile];
#pragma unroll
    for (int j = 0; j < DROP_ROUNDS; ++j) {
        const int64_t e = tile * DROP_TILE + j * WAVE + lane;
        const bool in = e < E;
        int64_t u = 0, v = 0;
        if (in) { u = src[e]; v = dst[e]; }
        const bool keep = in && !edge_dropped(root_t, rule.undirected != 0, e, u, v, rule.threshold);
        const uint64_t mask = __ballot(keep);
        const int64_t q = base + lanes_before(mask);
        if (keep && q < E) {
            out_src[q] = u;
            out_dst[q] = v;
        }
        if (in && newpos) newpos[e] = keep ? (int32_t)q : -1;
        if (in && pad_tail && e >= total) {                // no kept column lands at or behind `total`
            out_src[e] = -1;
            out_dst[e] = -1;
        }
        base += __popcll(mask);
    }
}

__global__ void __launch_bounds__(256)
drop_keep_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, DropRule rule,
                 const int64_t* __restrict__ tick, uint8_t* __restrict__ keep) {
    const uint64_t root_t = drop_root_t(rule.root, tick);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        int64_t u = 0, v = 0;
        if (rule.undirected) { u = src[e]; v = dst[e]; }
        keep[e] = edge_dropped(root_t, rule.undirected != 0, e, u, v, rule.threshold) ? 0 : 1;
    }
}

static DropRule drop_rule(int64_t key, int64_t threshold, int flags) {
    return DropRule{draw_root(key, DRAW_RULE_E), (uint64_t)threshold, (flags & NPI_DROP_UNDIRECTED) ? 1 : 0};
}
static int64_t drop_ws_elems(int64_t n) {
    const int64_t words = drop_tiles(n) + 1;               // the tile counts and the total; then the scan's own tile sums
    return words + ceil_div(words, 2048);
}
static bool drop_ws_ok(const void* ws, int64_t have, int64_t n) {
    return ws != nullptr && (reinterpret_cast<uintptr_t>(ws) % sizeof(int32_t)) == 0 && have >= drop_ws_elems(n);
}

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_drop_edges_workspace_elems(int64_t n) { return count_ok(n) ? drop_ws_elems(n) : -1; }

extern "C" int npi_csr_drop_side(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t N,
                                 int64_t nnz_max, int64_t n_edges, int64_t key, const int64_t* tick, int64_t threshold, int flags,
                                 int64_t nnz_max_out, int64_t item_edges, int32_t* rowptr_o, int32_t* col_o, int32_t* eid_o,
                                 int32_t* rowidx_o, int32_t* item_row_o, int32_t* workspace, int64_t workspace_elems, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(N) && count_ok(nnz_max) && count_ok(n_edges) && count_ok(nnz_max_out), "npi_csr_drop_side: bad size");
    NPI_REQUIRE(nnz_max_out >= nnz_max, "npi_csr_drop_side: nnz_max_out is below the parent's nnz_max");
    NPI_REQUIRE(item_edges_ok(item_edges), "npi_csr_drop_side: item_edges must be 64 or NPI_ITEM_EDGES");
    NPI_REQUIRE((flags & ~NPI_DROP_UNDIRECTED) == 0, "npi_csr_drop_side: unknown flag");
    NPI_REQUIRE(rowptr && col && eid && rowidx && rowptr_o && col_o && eid_o && rowidx_o && item_row_o, "npi_csr_drop_side: null pointer");
    NPI_REQUIRE(rowptr_o != rowptr && col_o != col && eid_o != eid && rowidx_o != rowidx, "npi_csr_drop_side: the output arrays are the input's");
    NPI_REQUIRE(drop_ws_ok(workspace, workspace_elems, nnz_max),
                "npi_csr_drop_side: workspace null, not aligned to 4 bytes or shorter than npi_drop_edges_workspace_elems(nnz_max)");
    const DropRule rule = drop_rule(key, threshold, flags);
    const int64_t n_tiles = drop_tiles(nnz_max);
    int32_t* tiles = workspace;
    drop_side_count_kernel<<<drop_grid(n_tiles + 1), DROP_THREADS, 0, stream>>>(rowptr, col, eid, rowidx, N, nnz_max, n_edges, rule, tick,
                                                                                  n_tiles, tiles);
    exclusive_scan_i32(tiles, n_tiles + 1, tiles + n_tiles + 1, stream);
    if (n_tiles > 0)
        drop_side_write_kernel<<<drop_grid(n_tiles), DROP_THREADS, 0, stream>>>(rowptr, col, eid, rowidx, N, nnz_max, n_edges, rule, tick,
                                                                                  n_tiles, tiles, nnz_max_out, rowptr_o, col_o, eid_o,
                                                                                  rowidx_o);
    drop_side_rows_kernel<<<(unsigned)ceil_div(N + 1, 256), 256, 0, stream>>>(rowptr, rowidx, N, nnz_max, tiles, n_tiles, rowptr_o);
    write_item_rows(rowptr_o, N, nnz_max_out, item_edges, item_row_o, stream);
    return check_launch("npi_csr_drop_side");
}

extern "C" int npi_drop_edge_list(const int64_t* src, const int64_t* dst, int64_t E, int64_t key, const int64_t* tick, int64_t threshold,
                                  int flags, int64_t* out_src, int64_t* out_dst, int32_t* newpos, int32_t* count, int pad_tail,
                                  int32_t* workspace, int64_t workspace_elems, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(E), "npi_drop_edge_list: bad size");
    NPI_REQUIRE((flags & ~NPI_DROP_UNDIRECTED) == 0, "npi_drop_edge_list: unknown flag");
    NPI_REQUIRE(count && (E == 0 || (src && dst && out_src && out_dst)), "npi_drop_edge_list: null pointer");
    NPI_REQUIRE(E == 0 || (out_src != src && out_dst != dst && out_src != dst && out_dst != src), "npi_drop_edge_list: not in place");
    NPI_REQUIRE(drop_ws_ok(workspace, workspace_elems, E),
                "npi_drop_edge_list: workspace null, not aligned to 4 bytes or shorter than npi_drop_edges_workspace_elems(E)");
    const DropRule rule = drop_rule(key, threshold, flags);
    const int64_t n_tiles = drop_tiles(E);
    int32_t* tiles = workspace;
    drop_list_count_kernel<<<drop_grid(n_tiles + 1), DROP_THREADS, 0, stream>>>(src, dst, E, rule, tick, n_tiles, tiles);
    exclusive_scan_i32(tiles, n_tiles + 1, tiles + n_tiles + 1, stream);
    drop_list_write_kernel<<<drop_grid(n_tiles + 1), DROP_THREADS, 0, stream>>>(src, dst, E, rule, tick, n_tiles, tiles, out_src, out_dst,
                                                                                  newpos, count, pad_tail);
    return check_launch("npi_drop_edge_list");
}

extern "C" int npi_drop_edge_keep(const int64_t* src, const int64_t* dst, int64_t E, int64_t key, const int64_t* tick, int64_t threshold,
                                  int flags, uint8_t* keep, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(E), "npi_drop_edge_keep: bad size");
    NPI_REQUIRE((flags & ~NPI_DROP_UNDIRECTED) == 0, "npi_drop_edge_keep: unknown flag");
    NPI_REQUIRE(E == 0 || (keep && (!(flags & NPI_DROP_UNDIRECTED) || (src && dst))), "npi_drop_edge_keep: null pointer");
    if (E == 0) return NPI_OK;
    drop_keep_kernel<<<stride_grid(E, 256, 2048), 256, 0, stream>>>(src, dst, E, drop_rule(key, threshold, flags), tick, keep);
    return check_launch("npi_drop_edge_keep");
}
