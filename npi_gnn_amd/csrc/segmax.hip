// Max aggregation over the CSR (include/npi_gnn.h: RULE X, npi_segmax / npi_segmax_bwd) -- PyG 1.4.2 `scatter_('max', x[col], row)`
// inside `MessagePassing.propagate(aggr='max')` and its backward, without the [nnz, F] gather written to memory and without a
// float atomic.
//
// Forward and backward stream the ENTRIES, as segscan.hip's seg_items_kernel and the aggregation kernel do: a wavefront takes one
// item (64 or 256 consecutive entries, whatever rows they belong to), the lanes are spread over the COLUMNS (a 16-byte piece per
// lane when the rows allow it, dot_lanes.h: rows16; one float otherwise; a row wider than one chunk walks the chunks), the ids of
// a block of 64 entries are fetched lane-parallel and broadcast, and eight gathered rows are in flight per lane (pair_score.hip).
//   * a row that begins and ends inside the item is written at once,
//   * the part of a row that began in an earlier item goes to head[item], the part of a row that runs on into the next item to
//     tail[item]; segmax_chain_kernel folds tail[i], head[i + 1], ... into the row.
// The forward's state per column is ONE 64-bit word (key of the value, ~eid): the larger word wins, which is RULE X literally --
// larger value first (NaN above +inf, -0 == +0), then the smaller uint32(eid) -- so merging is order-free.  The backward's state
// is a sum, added in ascending entry order inside the item and in a fixed order over the chain.
// A hub row is shared among the wavefronts of all the items it covers, and its chain among the sixteen wavefronts of a workgroup
// and the column blocks of the grid: no row is walked by one wavefront alone.
#include "dot_lanes.h"
#include "rank_key.h"

namespace npi {

namespace {

constexpr int SM_FLIGHT = 8;              // gathered rows in flight per lane
constexpr int CHAIN_SHORT = 4;            // a chain of up to this many heads is folded by ONE wavefront, in ascending order
constexpr int CHAIN_WAVES = 16;           // wavefronts of a chain workgroup: a longer chain is cut over all of them
constexpr uint32_t QUIET_NAN = 0x7fc00000u;

struct SegmaxArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* eid;
    const int32_t* rowidx;
    const float* tab;         // forward: x; backward: dOut -- the table the entries' columns index
    int64_t ldt;
    const int32_t* garg;      // backward: arg of the forward, gathered with dOut
    int64_t ldg;
    float* out;               // forward: out; backward: dX -- one row per CSR row
    int64_t ldo;
    int32_t* arg;             // forward only
    int64_t lda;
    float* head_v;            // [n_items, F] partial rows: the values (forward) / sums (backward) ...
    float* tail_v;
    int32_t* head_e;          // ... and, forward only, the winners' eid
    int32_t* tail_e;
    int32_t* tail_row;        // [n_items]: row of the item's tail partial, -1 = none
    int N, F, n_items, item, nnz_max;
};

// RULE X as one unsigned comparison: (ascending-orderable key of the value with NaN -> the quiet NaN and -0 -> +0, ~eid)
__device__ __forceinline__ uint64_t max_word(uint32_t bits, int32_t eid) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) bits = QUIET_NAN;
    return ((uint64_t)(~rank_key(bits)) << 32) | (uint32_t)(~(uint32_t)eid);
}
__device__ __forceinline__ float word_value(uint64_t w) { return rank_score(~(uint32_t)(w >> 32)); }
__device__ __forceinline__ int32_t word_eid(uint64_t w) { return (int32_t)(~(uint32_t)w); }

template <bool VEC> struct ArgLanes;
template <> struct ArgLanes<true> {
    using T = int4;
    static __device__ __forceinline__ T none() { return make_int4(-2, -2, -2, -2); }
    static __device__ __forceinline__ T load(const int32_t* p) { return *reinterpret_cast<const int4*>(p); }
};
template <> struct ArgLanes<false> {
    using T = int32_t;
    static __device__ __forceinline__ T none() { return -2; }
    static __device__ __forceinline__ T load(const int32_t* p) { return *p; }
};

__device__ __forceinline__ float comp(const float4& v, int w) { return w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w; }
__device__ __forceinline__ float comp(const float& v, int) { return v; }
__device__ __forceinline__ int32_t comp(const int4& v, int w) { return w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w; }
__device__ __forceinline__ int32_t comp(const int32_t& v, int) { return v; }

template <bool VEC> __device__ __forceinline__ void store_f(float* p, const float (&v)[VEC ? 4 : 1]);
template <> __device__ __forceinline__ void store_f<true>(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store_f<false>(float* p, const float (&v)[1]) { *p = v[0]; }
template <bool VEC> __device__ __forceinline__ void store_i(int32_t* p, const int32_t (&v)[VEC ? 4 : 1]);
template <> __device__ __forceinline__ void store_i<true>(int32_t* p, const int32_t (&v)[4]) {
    *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store_i<false>(int32_t* p, const int32_t (&v)[1]) { *p = v[0]; }

// What a lane has of the open row: BWD the running sums of its columns, otherwise their RULE X words (0 = no entry yet: below
// every word of an entry, whose key is at least that of -inf)
template <int W, bool BWD> struct RowState {
    uint64_t word[BWD ? 1 : W];
    float sum[BWD ? W : 1];
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if constexpr (BWD) sum[w] = 0.f;
            else word[w] = 0;
        }
    }
};

// The open row `cur` is complete as far as this item sees it.  `ended`: its last entry lies in this item.  Where it goes: a row
// that began in an earlier item -> head[item] (also when the whole item lies inside it), one that runs on -> tail[item], any
// other row is finished: out (and arg).  Returns true when the tail was written.
template <bool VEC, bool BWD>
__device__ __forceinline__ bool flush_row(const SegmaxArgs& A, const RowState<VEC ? 4 : 1, BWD>& st, int item, int cur, int prev_row,
                                          bool ended, int off, bool act) {
    constexpr int W = VEC ? 4 : 1;
    float* vp;
    int32_t* ep;
    bool tail = false;
    if (cur == prev_row) {
        vp = A.head_v + (int64_t)item * A.F;
        ep = BWD ? nullptr : A.head_e + (int64_t)item * A.F;
    } else if (ended) {
        vp = A.out + (int64_t)cur * A.ldo;
        ep = BWD ? nullptr : A.arg + (int64_t)cur * A.lda;
    } else {
        vp = A.tail_v + (int64_t)item * A.F;
        ep = BWD ? nullptr : A.tail_e + (int64_t)item * A.F;
        tail = true;
    }
    if (act) {
        float v[W];
        if constexpr (BWD) {
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = st.sum[w];
            store_f<VEC>(vp + off, v);
        } else {
            int32_t e[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                v[w] = word_value(st.word[w]);
                e[w] = word_eid(st.word[w]);
            }
            store_f<VEC>(vp + off, v);
            store_i<VEC>(ep + off, e);
        }
    }
    return tail;
}

//   VEC : 16-byte lanes (F > 64, F % 4 == 0 and every table, output and partial row 16-byte aligned), a chunk is 256 columns;
//         otherwise one float per lane, 64 columns
//   BWD : dX[row] = sum over the row's entries q of dOut[col[q], c] where arg[col[q], c] == eid[q] -- two gathered rows per entry
template <bool VEC, bool BWD>
__global__ void __launch_bounds__(256)
segmax_items_kernel(SegmaxArgs A) {
    using L = Lanes<VEC>;
    using T = typename L::T;
    using G = ArgLanes<VEC>;
    constexpr int W = L::W;
    constexpr int CW = WAVE * W;
    const int lane = lane_id();
    const int item = uniform_i(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (item >= A.n_items) return;
    const int nnz = min(uniform_i(A.rowptr[A.N]), A.nnz_max);                  // entries behind it are padding: never read
    const int k0 = item * A.item;
    if (k0 >= nnz) {
        if (lane == 0) A.tail_row[item] = -1;
        return;
    }
    const int k1 = min(k0 + A.item, nnz);
    const int prev_row = k0 > 0 ? uniform_i(A.rowidx[k0 - 1]) : -1;            // the row that may run INTO this item
    const int next_row = k1 < nnz ? uniform_i(A.rowidx[k1]) : -2;              // the row of the first entry behind it
    int tail_r = -1;
    for (int c0 = 0; c0 < A.F; c0 += CW) {
        const int off = c0 + lane * W;
        const bool act = off < A.F;
        RowState<W, BWD> st;
        st.reset();
        int cur = uniform_i(A.rowidx[k0]);
        for (int kb = k0; kb < k1; kb += WAVE) {
            const int nb = min(WAVE, k1 - kb);
            int cv = 0, ev = -1, rv = 0;
            if (lane < nb) {
                cv = A.col[kb + lane];
                ev = A.eid[kb + lane];
                rv = A.rowidx[kb + lane];
            }
            if (ev < 0) ev = -1;                                               // the appended loop
            for (int j = 0; j < nb; j += SM_FLIGHT) {
                T x[SM_FLIGHT];
                typename G::T g[SM_FLIGHT];
#pragma unroll
                for (int u = 0; u < SM_FLIGHT; ++u) {
                    const int m = j + u;                                       // < 64 (j a multiple of eight below nb)
                    const bool rd = act && m < nb;
                    const int cu = bcast_i(cv, m);
                    x[u] = rd ? L::load(A.tab + (int64_t)cu * A.ldt + off) : L::zero();
                    if constexpr (BWD) g[u] = rd ? G::load(A.garg + (int64_t)cu * A.ldg + off) : G::none();
                }
#pragma unroll
                for (int u = 0; u < SM_FLIGHT; ++u) {
                    const int m = j + u;
                    if (m < nb) {                                              // (wave-uniform)
                        const int r = bcast_i(rv, m), e = bcast_i(ev, m);
                        if (r != cur) {                                        // the open row ended with the entry before
                            flush_row<VEC, BWD>(A, st, item, cur, prev_row, true, off, act);
                            st.reset();
                            cur = r;
                        }
#pragma unroll
                        for (int w = 0; w < W; ++w) {
                            if constexpr (BWD) {
                                st.sum[w] += comp(g[u], w) == e ? comp(x[u], w) : 0.f;
                            } else {
                                const uint64_t k = max_word(__float_as_uint(comp(x[u], w)), e);
                                if (k > st.word[w]) st.word[w] = k;
                            }
                        }
                    }
                }
            }
        }
        if (flush_row<VEC, BWD>(A, st, item, cur, prev_row, next_row != cur, off, act)) tail_r = cur;
    }
    if (lane == 0) A.tail_row[item] = tail_r;
}

// Row r = tail_row[i] of every item i that ends inside a row: tail[i] (+) head[i + 1] (+) ... (+) head[i + n].  A workgroup of
// sixteen wavefronts takes sixteen items and 64 columns (blockIdx.y): a wavefront folds the chain of ITS item when that has at
// most CHAIN_SHORT heads (nearly all: rows are tens of entries), in ascending order.  The longer chains -- the 400k-entry hub
// row: 1,600 heads -- are then taken one after the other by the whole workgroup: wavefront w folds the heads t = w, w + 16, ...
// in ascending t, and the sixteen partial results are added to the tail in the order 0 .. 15.  The forward's merge is order-free
// anyway; the backward's sum has this one fixed order.  No atomics.
template <bool BWD> struct ChainOp;
template <> struct ChainOp<false> {
    using V = uint64_t;
    static __device__ __forceinline__ V identity() { return 0; }
    static __device__ __forceinline__ V load(const float* v, const int32_t* e, int64_t i) { return max_word(__float_as_uint(v[i]), e[i]); }
    static __device__ __forceinline__ V merge(V a, V b) { return a > b ? a : b; }
};
template <> struct ChainOp<true> {
    using V = float;
    static __device__ __forceinline__ V identity() { return 0.f; }
    static __device__ __forceinline__ V load(const float* v, const int32_t*, int64_t i) { return v[i]; }
    static __device__ __forceinline__ V merge(V a, V b) { return a + b; }       // a = the EARLIER part
};

template <bool BWD>
__global__ void __launch_bounds__(CHAIN_WAVES * WAVE)
segmax_chain_kernel(SegmaxArgs A) {
    using Op = ChainOp<BWD>;
    using V = typename Op::V;
    __shared__ V part[CHAIN_WAVES][WAVE];
    const int lane = lane_id();
    const int wv = uniform_i(threadIdx.x >> 6);
    const int c = blockIdx.y * WAVE + lane;
    const bool act = c < A.F;
    const int base = blockIdx.x * CHAIN_WAVES;
    const int F = A.F;
    // lane l < 16 of EVERY wavefront: row and chain length of item base + l
    int r = -1, n = 0;
    if (lane < CHAIN_WAVES && base + lane < A.n_items) {
        r = A.tail_row[base + lane];
        if (r >= A.N) r = -1;
        if (r >= 0) n = min((A.rowptr[r + 1] - 1) / A.item, A.n_items - 1) - (base + lane);
    }
    auto write_row = [&](int row, V acc) {
        if constexpr (BWD) {
            A.out[(int64_t)row * A.ldo + c] = acc;
        } else {
            A.out[(int64_t)row * A.ldo + c] = word_value(acc);
            A.arg[(int64_t)row * A.lda + c] = word_eid(acc);
        }
    };
    const int my_r = bcast_i(r, wv), my_n = bcast_i(n, wv);
    if (my_r >= 0 && my_n <= CHAIN_SHORT && act) {
        const int64_t it = base + wv;
        V acc = Op::load(A.tail_v, A.tail_e, it * F + c);
        for (int t = 1; t <= my_n; ++t) acc = Op::merge(acc, Op::load(A.head_v, A.head_e, (it + t) * F + c));
        write_row(my_r, acc);
    }
    uint64_t todo = __ballot(r >= 0 && n > CHAIN_SHORT);                       // the same word in every wavefront of the workgroup
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t it = base + l;
        const int nn = bcast_i(n, l), rr = bcast_i(r, l);
        V acc = Op::identity();
        if (act) {
#pragma unroll 4
            for (int t = wv; t < nn; t += CHAIN_WAVES) acc = Op::merge(acc, Op::load(A.head_v, A.head_e, (it + 1 + t) * F + c));
        }
        part[wv][lane] = acc;
        __syncthreads();
        if (wv == 0 && act) {
            V a = Op::load(A.tail_v, A.tail_e, it * F + c);
#pragma unroll
            for (int w = 0; w < CHAIN_WAVES; ++w) a = Op::merge(a, part[w][lane]);
            write_row(rr, a);
        }
        __syncthreads();
    }
}

// rows without an entry: out = +0.0 (PyG's fill of scatter_('max')), arg = -2; the backward: dX = 0.  A wavefront looks at 64 rows
// lane-parallel and writes the empty ones among them one after the other, coalesced.
__global__ void __launch_bounds__(256)
segmax_empty_rows_kernel(const int32_t* __restrict__ rowptr, int N, int F, float* __restrict__ out, int64_t ldo,
                         int32_t* __restrict__ arg, int64_t lda) {
    const int lane = lane_id();
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * WAVE;
    const int64_t r = r0 + lane;
    uint64_t m = __ballot(r < N && rowptr[r] == rowptr[r + 1]);
    while (m) {
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int64_t rr = r0 + l;
        for (int c = lane; c < F; c += WAVE) {
            out[rr * ldo + c] = 0.f;
            if (arg) arg[rr * lda + c] = -2;
        }
    }
}

struct Workspace {
    float *head_v, *tail_v;
    int32_t *head_e, *tail_e, *tail_row;
};
// 16-byte lanes put F / 4 lanes of a wavefront to work: up to 64 columns one float per lane keeps all of them busy (the per-element
// compare, not the gather, bounds a table that narrow -- EXPERIMENTS.md A57)
bool wide_lanes(int64_t F) { return F > WAVE; }
int64_t plane_bytes(int64_t n_items, int64_t F) { return align_up(n_items * F * 4, 16); }
int64_t workspace_bytes(int64_t nnz_max, int64_t item, int64_t F) {
    const int64_t n_items = num_items_of(nnz_max, item);
    return 4 * plane_bytes(n_items, F) + align_up(n_items * 4, 16);
}

// the launches both directions share: empty rows, the items, the chains
template <bool BWD>
int segmax_run(SegmaxArgs A, bool vec, void* workspace, hipStream_t stream, const char* what) {
    if (A.N == 0) return NPI_OK;
    segmax_empty_rows_kernel<<<(unsigned)ceil_div(A.N, 4 * WAVE), 256, 0, stream>>>(A.rowptr, A.N, A.F, A.out, A.ldo, BWD ? nullptr : A.arg,
                                                                                   A.lda);
    const int64_t n_items = num_items_of(A.nnz_max, A.item);
    if (n_items > 0) {
        const int64_t pb = plane_bytes(n_items, A.F);
        char* ws = static_cast<char*>(workspace);
        A.head_v = reinterpret_cast<float*>(ws);
        A.tail_v = reinterpret_cast<float*>(ws + pb);
        A.head_e = reinterpret_cast<int32_t*>(ws + 2 * pb);
        A.tail_e = reinterpret_cast<int32_t*>(ws + 3 * pb);
        A.tail_row = reinterpret_cast<int32_t*>(ws + 4 * pb);
        A.n_items = (int)n_items;
        const unsigned grid = (unsigned)ceil_div(n_items, 4);
        if (vec) segmax_items_kernel<true, BWD><<<grid, 256, 0, stream>>>(A);
        else segmax_items_kernel<false, BWD><<<grid, 256, 0, stream>>>(A);
        const dim3 cgrid((unsigned)ceil_div(n_items, CHAIN_WAVES), (unsigned)ceil_div(A.F, WAVE));
        segmax_chain_kernel<BWD><<<cgrid, CHAIN_WAVES * WAVE, 0, stream>>>(A);
    }
    return check_launch(what);
}

}  // namespace

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_segmax_workspace_bytes(int64_t nnz_max, int64_t item_edges, int64_t F) {
    if (!count_ok(nnz_max) || !item_edges_ok(item_edges) || F <= 0 || F >= NPI_INDEX_LIMIT) return -1;
    return workspace_bytes(nnz_max, item_edges, F);
}

// the checks both entry points share; `t` / `ldt`: the gathered table, `o` / `ldo`: the per-row output, `a` / `lda`: arg
#define NPI_SEGMAX_CHECK(WHAT, t, ldt, o, ldo, a, lda)                                                                               \
    NPI_REQUIRE(count_ok(N) && count_ok(n_cols) && count_ok(nnz_max), WHAT ": bad size (N, n_cols, nnz_max in [0, 2^31 - 1))");        \
    NPI_REQUIRE(F > 0 && F < NPI_INDEX_LIMIT, WHAT ": F must be positive");                                                           \
    NPI_REQUIRE(item_edges_ok(item_edges), WHAT ": item_edges must be 64 or 256 (the size the side was built with)");                \
    NPI_REQUIRE(ldt >= F && ldo >= F && lda >= F, WHAT ": a row pitch is below F");                                                   \
    if (N == 0) return NPI_OK;                                                                                                       \
    NPI_REQUIRE(rowptr && col && eid && rowidx && t && o && a, WHAT ": null pointer (rowptr, col, eid, rowidx and the tables are required)"); \
    NPI_REQUIRE(nnz_max == 0 || (workspace && ((uintptr_t)workspace % 16) == 0 &&                                                     \
                                 workspace_bytes_ >= workspace_bytes(nnz_max, item_edges, F)),                                         \
                WHAT ": the workspace is null, misaligned (16 bytes) or shorter than npi_segmax_workspace_bytes(nnz_max, item_edges, F)")

extern "C" int npi_segmax(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t item_edges,
                          int64_t N, int64_t n_cols, int64_t nnz_max, const float* x, int64_t ldx, int64_t F, float* out, int64_t ldo,
                          int32_t* arg, int64_t lda, void* workspace, int64_t workspace_bytes_, void* stream) {
    NPI_SEGMAX_CHECK("npi_segmax", x, ldx, out, ldo, arg, lda);
    SegmaxArgs A{};
    A.rowptr = rowptr; A.col = col; A.eid = eid; A.rowidx = rowidx;
    A.tab = x; A.ldt = ldx; A.out = out; A.ldo = ldo; A.arg = arg; A.lda = lda;
    A.N = (int)N; A.F = (int)F; A.item = (int)item_edges; A.nnz_max = (int)nnz_max;
    const bool vec = wide_lanes(F) && rows16(x, ldx, F) && rows16(out, ldo, F) && rows16(arg, lda, F);
    return segmax_run<false>(A, vec, workspace, (hipStream_t)stream, "npi_segmax");
}

extern "C" int npi_segmax_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t item_edges,
                              int64_t N, int64_t n_cols, int64_t nnz_max, const float* dout, int64_t ldd, const int32_t* arg,
                              int64_t lda, int64_t F, float* dx, int64_t ldx, void* workspace, int64_t workspace_bytes_, void* stream) {
    NPI_SEGMAX_CHECK("npi_segmax_bwd", dout, ldd, dx, ldx, arg, lda);
    SegmaxArgs A{};
    A.rowptr = rowptr; A.col = col; A.eid = eid; A.rowidx = rowidx;
    A.tab = dout; A.ldt = ldd; A.garg = arg; A.ldg = lda; A.out = dx; A.ldo = ldx;
    A.N = (int)N; A.F = (int)F; A.item = (int)item_edges; A.nnz_max = (int)nnz_max;
    const bool vec = wide_lanes(F) && rows16(dout, ldd, F) && rows16(arg, lda, F) && rows16(dx, ldx, F);
    return segmax_run<true>(A, vec, workspace, (hipStream_t)stream, "npi_segmax_bwd");
}
#undef NPI_SEGMAX_CHECK
