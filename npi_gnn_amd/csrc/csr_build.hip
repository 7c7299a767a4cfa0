// COO (int64, as PyG hands it over) -> destination-sorted CSR (int32) with the self loop of
// add_remaining_self_loops appended as the LAST entry of every row.
//
// Replaces, for reference src/classes.py:62,66,70 (SAGEConv.forward -> PyG 1.4.2
// utils.add_remaining_self_loops + the per-target grouping torch_scatter does with atomics).
//
// Stable LSD radix sort on the key node id (8-bit digits, ceil(log2(N+1)/8) passes):
// entries of a row keep their edge_index order, so the reduction order equals the
// reference's CPU scatter order and every run is bitwise identical.  The sort itself: sort.h.
//
// Here: the key kernels, fill_csr_kernel, item_rows_kernel (write_item_rows for the other files), npi_csr_build_ex, npi_csr_filter
// (the CSR of a pooled graph from its parent's, no sort) with its kernels, npi_edge_positions and the item-size queries.
#include "sort.h"

namespace npi {

// key = key node, or N (sentinel, sorts behind every row) for dropped columns
__global__ void make_keys_kernel(const int64_t* __restrict__ key_nodes,
                                 const int64_t* __restrict__ val_nodes, int64_t E, int64_t N,
                                 int64_t n_cols, int drop_equal,
                                 uint32_t* __restrict__ keys, int32_t* __restrict__ vals,
                                 int32_t* __restrict__ status) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int64_t k = key_nodes[e], v = val_nodes[e];
    // (-1, -1) is a PADDING column: npi_filter_adj(pad_tail) keeps its output at the input's length and fills the tail with it,
    // so that the edge count never has to be read back; dropped without raising the out-of-range flag
    const bool pad = (k == -1) & (v == -1);
    bool bad = !pad & ((k < 0) | (k >= N) | (v < 0) | (v >= n_cols));
    if (bad) atomicOr(status, 1);
    keys[e] = (pad || bad || (drop_equal && k == v)) ? (uint32_t)N : (uint32_t)k;
    vals[e] = (int32_t)e;
}

// NPI_CSR_SORT_COLUMNS, first sort: key = the column node (out-of-range columns: n_cols, behind everything; make_keys_kernel's
// rules decide later what becomes of them), val = the entry's position in the caller's list
__global__ void col_keys_kernel(const int64_t* __restrict__ val_nodes, int64_t E, int64_t n_cols,
                                uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t v = val_nodes[e];
    keys[e] = (v < 0 || v >= n_cols) ? (uint32_t)n_cols : (uint32_t)v;
    vals[e] = (int32_t)e;
}

// ... second sort's keys: make_keys_kernel's rule for the entry that the column sort left at position i
__global__ void rekey_kernel(const int64_t* __restrict__ key_nodes, const int64_t* __restrict__ val_nodes,
                             const int32_t* __restrict__ vals, int64_t E, int64_t N, int64_t n_cols, int drop_equal,
                             uint32_t* __restrict__ keys, int32_t* __restrict__ status) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const int64_t e = vals[i];
    const int64_t k = key_nodes[e], v = val_nodes[e];
    const bool pad = (k == -1) & (v == -1);
    const bool bad = !pad & ((k < 0) | (k >= N) | (v < 0) | (v >= n_cols));
    if (bad) atomicOr(status, 1);
    keys[i] = (pad || bad || (drop_equal && k == v)) ? (uint32_t)N : (uint32_t)k;
}

__device__ __forceinline__ int64_t first_key_at_least(const uint32_t* __restrict__ keys, int64_t E, int64_t r) {
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < (uint32_t)r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One launch writes the whole CSR from the sorted (key, column) stream.
// Workgroups [0, entry_blocks): entry p of the sorted stream lands at p (+ key when every row gets a self loop behind it).
// Workgroups behind them: row r -- rowptr[r] = first sorted position with key >= r (+ r), and the appended self loop.
__global__ void __launch_bounds__(256)
fill_csr_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals,
                const int64_t* __restrict__ val_nodes, int64_t E, int64_t N, int loops, int32_t loop_col_offset,
                unsigned entry_blocks, int32_t* __restrict__ rowptr, int32_t* __restrict__ col,
                int32_t* __restrict__ eid, int32_t* __restrict__ rowidx) {
    if (blockIdx.x < entry_blocks) {
        int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (p >= E) return;
        uint32_t k = keys[p];
        if (k >= (uint32_t)N) return;
        int32_t e = vals[p];
        int64_t q = p + (loops ? (int64_t)k : 0);
        col[q] = (int32_t)val_nodes[e];
        if (eid) eid[q] = e;
        if (rowidx) rowidx[q] = (int32_t)k;
        return;
    }
    // row r starts at the first sorted position with key >= r; its end is the next thread's start (one search per
    // row, the workgroup's last thread searches once more)
    __shared__ int64_t lb_s[257];
    int64_t r = (int64_t)(blockIdx.x - entry_blocks) * 256 + threadIdx.x;
    const bool have = r <= N;
    const int64_t lb = have ? first_key_at_least(keys, E, r) : E;
    lb_s[threadIdx.x] = lb;
    if (threadIdx.x == 255) lb_s[256] = (r + 1 <= N) ? first_key_at_least(keys, E, r + 1) : E;
    __syncthreads();
    if (!have) return;
    rowptr[r] = (int32_t)(lb + (loops ? r : 0));
    if (loops && r < N) {
        int64_t q = lb_s[threadIdx.x + 1] + r;                  // behind the last entry of row r
        col[q] = (int32_t)r + loop_col_offset;
        if (eid) eid[q] = -1;
        if (rowidx) rowidx[q] = (int32_t)r;
    }
}

// item_row[i] = row holding entry i*item (item 0 starts at row 0 so that leading empty
// rows get written); N for items past nnz.
__global__ void item_rows_kernel(const int32_t* __restrict__ rowptr, int64_t N, int64_t n_items, int item,
                                 int32_t* __restrict__ item_row) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_items) return;
    int64_t nnz = rowptr[N];
    int64_t k = i * item;
    if (i == 0) { item_row[0] = 0; return; }
    if (k >= nnz) { item_row[i] = (int32_t)N; return; }
    // upper_bound(rowptr[0..N], k) - 1
    int64_t lo = 0, hi = N + 1;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rowptr[mid] <= k) lo = mid + 1; else hi = mid;
    }
    item_row[i] = (int32_t)(lo - 1);
}
void write_item_rows(const int32_t* rowptr, int64_t N, int64_t nnz_max, int64_t item_edges, int32_t* item_row, hipStream_t stream) {
    const int64_t n_items = num_items_of(nnz_max, item_edges);
    item_rows_kernel<<<(unsigned)ceil_div(n_items + 1, 256), 256, 0, stream>>>(rowptr, N, n_items, (int)item_edges, item_row);
}

__global__ void edge_positions_kernel(const int32_t* __restrict__ eid, const int32_t* __restrict__ rowptr,
                                      int64_t N, int64_t nnz_max, int32_t* __restrict__ pos_of) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz_max || p >= rowptr[N]) return;
    int32_t e = eid[p];
    if (e >= 0) pos_of[e] = (int32_t)p;
}

__global__ void fill_i32_kernel(int32_t* __restrict__ p, int64_t n, int32_t v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_csr_workspace_bytes(int64_t E, int64_t N) {
    if (E < 0 || N < 0) return -1;
    return PairSort::bytes(E);
}

extern "C" int64_t npi_item_edges(int64_t nnz_max) { return npi::item_edges_for(nnz_max); }

extern "C" int64_t npi_num_items(int64_t nnz_max, int64_t item_edges) {
    if (!npi::item_edges_ok(item_edges)) return -1;
    return npi::num_items_of(nnz_max, item_edges);
}

extern "C" int npi_csr_build_ex(const int64_t* key_nodes, const int64_t* val_nodes, int64_t E, int64_t N,
                                int64_t n_cols, int add_self_loops, int64_t loop_col_offset, int build_flags,
                                int32_t* rowptr, int32_t* col, int32_t* eid,
                                int32_t* rowidx, int32_t* item_row, int64_t item_edges, int32_t* status,
                                void* workspace, int64_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(E >= 0 && N >= 0 && n_cols >= 0, "npi_csr_build: negative size");
    NPI_REQUIRE((build_flags & ~(NPI_CSR_DROP_EQUAL | NPI_CSR_SORT_COLUMNS)) == 0, "npi_csr_build: unknown build flag");
    NPI_REQUIRE(item_edges_ok(item_edges), "npi_csr_build: item_edges must be 64 or NPI_ITEM_EDGES (npi_item_edges gives the hint)");
    NPI_REQUIRE(E + N + 1 < NPI_INDEX_LIMIT, "npi_csr_build: E + N does not fit int32");
    NPI_REQUIRE(n_cols < NPI_INDEX_LIMIT && loop_col_offset >= 0 && loop_col_offset + N <= (n_cols > N ? n_cols : N),
                "npi_csr_build: column range does not fit");
    NPI_REQUIRE(rowptr && item_row && status && workspace, "npi_csr_build: null output");
    NPI_REQUIRE(E == 0 || (key_nodes && val_nodes && col), "npi_csr_build: null edge arrays");
    if (workspace_short("npi_csr_build", workspace_bytes, PairSort::bytes(E))) return NPI_ERR_WORKSPACE;
    PairSort ps;
    (void)ps.carve(workspace, workspace_bytes, E);         // (the length was checked above)
    (void)hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    const int drop_equal = build_flags & NPI_CSR_DROP_EQUAL;
    if (E > 0) {
        const unsigned eb = (unsigned)ceil_div(E, 256);
        if (build_flags & NPI_CSR_SORT_COLUMNS) {
            // LSD over the pair (row, column): the stable sort by column first, then the stable sort by row keeps it inside a row
            col_keys_kernel<<<eb, 256, 0, stream>>>(val_nodes, E, n_cols, ps.keys_a, ps.vals_a);
            ps.sort(key_bits(n_cols + 1), stream);      // keys lie in [0, n_cols]
            rekey_kernel<<<eb, 256, 0, stream>>>(key_nodes, val_nodes, ps.vals_a, E, N, n_cols, drop_equal, ps.keys_a, status);
        } else {
            make_keys_kernel<<<eb, 256, 0, stream>>>(key_nodes, val_nodes, E, N, n_cols, drop_equal, ps.keys_a, ps.vals_a, status);
        }
        ps.sort(key_bits(N + 1), stream);               // keys lie in [0, N]
    }
    const unsigned entry_blocks = (unsigned)ceil_div(E, 256);
    fill_csr_kernel<<<entry_blocks + (unsigned)ceil_div(N + 1, 256), 256, 0, stream>>>(
        ps.keys_a, ps.vals_a, val_nodes, E, N, add_self_loops, (int32_t)loop_col_offset, entry_blocks, rowptr, col, eid, rowidx);
    write_item_rows(rowptr, N, E + (add_self_loops ? N : 0), item_edges, item_row, stream);
    return check_launch("npi_csr_build");
}

// ---- the CSR of a pooled graph from the CSR of its parent: no sort ------------------------------------------------------
// TopKPooling keeps a subset of the nodes, renumbers them (perm: new -> old, remap: old -> new or -1) and filter_adj drops
// every edge that lost an endpoint while keeping the edge order.  The by-target CSR of the result is therefore the parent's,
// row perm[r'] for new row r', with the entries whose source survived, in the same order (the self loop still last):
// count per new row, ordered fill (offsets from per-tile totals), item rows -- three launches instead of the eight of a fresh radix sort.
namespace npi {
// Tiles of 256 new rows, one thread per row: the enclosing subgraphs are double stars, so almost every row has two or three
// entries and a lane walks its own row; the few long rows (the two centres of a subgraph, hundreds of entries) are taken by
// the whole wave, one after the other.  count: per-row counts and the tile's total.  fill: the tile's base is the sum of the
// totals in front of it (a few hundred integers), the rows' offsets an exclusive scan inside the tile -- no scan launch.
constexpr int CF_SHORT = 8;
__global__ void __launch_bounds__(256)
csr_filter_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ perm,
                        const int32_t* __restrict__ remap, int n_out, int32_t* __restrict__ cnt, int32_t* __restrict__ tile_total) {
    __shared__ int wtot[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r2 = blockIdx.x * 256 + t;
    const bool valid = r2 < n_out;
    const int r = valid ? perm[r2] : 0;
    const int b = valid ? rowptr[r] : 0, e = valid ? rowptr[r + 1] : 0;
    const bool is_long = e - b > CF_SHORT;
    int c = 0;
    if (!is_long) for (int p = b; p < e; ++p) c += remap[col[p]] >= 0 ? 1 : 0;
    uint64_t m = __ballot(is_long);
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int bb = __shfl(b, l, WAVE), ee = __shfl(e, l, WAVE);
        int cc = 0;
        for (int p = bb + lane; p < ee; p += WAVE) cc += remap[col[p]] >= 0 ? 1 : 0;
        cc = wave_sum(cc);
        if (lane == l) c = cc;
    }
    if (valid) cnt[r2] = c;
    const int ws_ = wave_sum(c);
    if (lane == 0) wtot[wave] = ws_;
    __syncthreads();
    if (t == 0) tile_total[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}
__global__ void __launch_bounds__(256)
csr_filter_fill_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
                       const int32_t* __restrict__ perm, const int32_t* __restrict__ remap, const int32_t* __restrict__ newpos,
                       int n_out, const int32_t* __restrict__ cnt, const int32_t* __restrict__ tile_total,
                       int32_t* __restrict__ rowptr_o, int32_t* __restrict__ col_o, int32_t* __restrict__ eid_o,
                       int32_t* __restrict__ rowidx_o) {
    __shared__ int wtot[4], base_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // entries in front of this tile
    int s = 0;
    for (int i = t; i < (int)blockIdx.x; i += 256) s += tile_total[i];
    s = wave_sum(s);
    if (lane == 0) wtot[wave] = s;
    __syncthreads();
    if (t == 0) base_s = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    const int base = base_s;
    const int r2 = blockIdx.x * 256 + t;
    const bool valid = r2 < n_out;
    const int c = valid ? cnt[r2] : 0;
    int x = c;                                               // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, WAVE);
        if (lane >= off) x += y;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wtot[w];
    const int start = base + woff + x - c;
    if (valid) {
        rowptr_o[r2] = start;
        if (r2 == n_out - 1) rowptr_o[n_out] = start + c;
    }
    const int r = valid ? perm[r2] : 0;
    const int b = valid ? rowptr[r] : 0, e = valid ? rowptr[r + 1] : 0;
    const bool is_long = e - b > CF_SHORT;
    if (!is_long) {
        int pos = start;
        for (int p = b; p < e; ++p) {
            const int c2 = remap[col[p]];
            if (c2 >= 0) {
                const int e0 = eid[p];
                col_o[pos] = c2;
                eid_o[pos] = e0 >= 0 ? newpos[e0] : -1;      // the self loop keeps -1
                rowidx_o[pos] = r2;
                ++pos;
            }
        }
    }
    uint64_t m = __ballot(is_long);
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int bb = __shfl(b, l, WAVE), ee = __shfl(e, l, WAVE), rr = __shfl(r2, l, WAVE);
        int out = __shfl(start, l, WAVE);
        for (int pb = bb; pb < ee; pb += WAVE) {
            const int p = pb + lane;
            int c2 = -1;
            if (p < ee) c2 = remap[col[p]];
            const uint64_t k = __ballot(c2 >= 0);
            if (c2 >= 0) {
                const int pos = out + __popcll(k & ((1ull << lane) - 1ull));
                const int e0 = eid[p];
                col_o[pos] = c2;
                eid_o[pos] = e0 >= 0 ? newpos[e0] : -1;
                rowidx_o[pos] = rr;
            }
            out += __popcll(k);
        }
    }
}
}  // namespace npi

extern "C" int64_t npi_csr_filter_max_rows(void) { return (int64_t)1 << 24; }      // tile totals summed per tile: above this, sort afresh
extern "C" int64_t npi_csr_filter_workspace_elems(int64_t n_out) { return n_out < 0 ? -1 : n_out + ceil_div(n_out > 0 ? n_out : 1, 256) + 1; }

extern "C" int npi_csr_filter(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* perm,
                              const int32_t* remap, const int32_t* newpos, int64_t n_out, int64_t nnz_max_out,
                              int32_t* rowptr_o, int32_t* col_o, int32_t* eid_o, int32_t* rowidx_o, int32_t* item_row_o,
                              int64_t item_edges, int32_t* status_o, int32_t* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(n_out >= 0 && n_out <= npi_csr_filter_max_rows() && nnz_max_out >= n_out, "npi_csr_filter: bad size");
    NPI_REQUIRE(item_edges_ok(item_edges), "npi_csr_filter: item_edges must be 64 or NPI_ITEM_EDGES");
    NPI_REQUIRE(rowptr_o && item_row_o && status_o && (n_out == 0 || (rowptr && col && eid && perm && remap && newpos && col_o &&
                eid_o && rowidx_o && workspace)), "npi_csr_filter: null pointer");
    (void)hipMemsetAsync(status_o, 0, sizeof(int32_t), stream);            // ids were checked when the parent was built
    if (n_out == 0) {
        (void)hipMemsetAsync(rowptr_o, 0, sizeof(int32_t), stream);
    } else {
        const unsigned tiles = (unsigned)ceil_div(n_out, 256);
        int32_t* cnt = workspace;
        int32_t* tile_total = workspace + n_out;
        csr_filter_count_kernel<<<tiles, 256, 0, stream>>>(rowptr, col, perm, remap, (int)n_out, cnt, tile_total);
        csr_filter_fill_kernel<<<tiles, 256, 0, stream>>>(rowptr, col, eid, perm, remap, newpos, (int)n_out, cnt, tile_total,
                                                          rowptr_o, col_o, eid_o, rowidx_o);
    }
    write_item_rows(rowptr_o, n_out, nnz_max_out, item_edges, item_row_o, stream);
    return check_launch("npi_csr_filter");
}

extern "C" int npi_edge_positions(const int32_t* eid, const int32_t* rowptr, int64_t N, int64_t nnz_max,
                                  int64_t E, int32_t* pos_of, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(E >= 0 && nnz_max >= 0, "npi_edge_positions: negative size");
    if (E > 0) fill_i32_kernel<<<(unsigned)ceil_div(E, 256), 256, 0, stream>>>(pos_of, E, -1);
    if (nnz_max > 0)
        edge_positions_kernel<<<(unsigned)ceil_div(nnz_max, 256), 256, 0, stream>>>(eid, rowptr, N, nnz_max, pos_of);
    return check_launch("npi_edge_positions");
}
