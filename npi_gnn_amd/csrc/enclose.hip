// h-hop enclosing subgraphs of target pairs, induced, with SEAL's DRNL labels, extracted and collated on the device (Rule H of
// include/npi_gnn.h).  Where subgraph.hip restates the reference's one-hop star, this is SEAL's data construction: the nodes within
// h hops of either target, EVERY edge among them, the target link itself never walked, and per node the two distances the label is
// made of.
//
// The parent graph is a by-target CSR over one id space with sorted columns (rowptr[N + 1], col, eid: npi_csr_build_ex with
// NPI_CSR_SORT_COLUMNS, no loops); it holds every edge in both directions, so row w lists the neighbours of w.  One workgroup per
// sample; what a sample has reached lives in bitmaps of W = ceil(N / 32) words in the caller's workspace -- visited, current level,
// next level and the exclusive popcount prefix of visited -- so the node order of the output (ascending id) is the bitmap's own and
// the order of discovery never matters: integer atomicOr only, no frontier lists, no synchronisation between workgroups.
//
// Rows are walked by the thread that finds their bit; a row of ROW_LONG entries or more (the hub protein has 1,121 partners) is set
// aside in an LDS list and walked by a whole wavefront afterwards, 64 entries a step.
#include "sort.h"

namespace npi {

constexpr int ENC_THREADS = 256;
constexpr int ENC_WAVES = ENC_THREADS / WAVE;
constexpr int ROW_LONG = 64;             // entries from which a row goes to a wavefront
constexpr int LONG_CAP = 512;            // rows the LDS list holds; what does not fit is walked by its own thread

struct Parent {
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ col;
    const int32_t* __restrict__ eid;
    const uint8_t* __restrict__ mask;    // by column number; nullptr: every column exists
    int N, W;
};

// the bitmaps of sample g
struct Maps {
    uint32_t *vis, *cur, *nxt, *prefix;
};
__device__ __forceinline__ Maps maps_of(uint32_t* ws, int W, int g) {
    uint32_t* base = ws + (int64_t)g * 4 * W;
    return Maps{base, base + W, base + 2 * (int64_t)W, base + 3 * (int64_t)W};
}

__device__ __forceinline__ bool bit_of(const uint32_t* bm, int w) { return (bm[w >> 5] >> (w & 31)) & 1u; }

// Rule H 1: entry k of row w (source j) may be walked
__device__ __forceinline__ bool walkable(const Parent& P, int w, int j, int k, int u, int v) {
    if ((w == u && j == v) || (w == v && j == u)) return false;
    return P.mask == nullptr || P.mask[P.eid[k]] != 0;
}

// Every set bit w of bm[0 .. W): body.serial(w, b, e) by one thread, or body.wave(w, b, e, lane) by the 64 lanes of a wavefront, with
// [b, e) the entries of row w.  Every thread of the workgroup calls it; it ends with a barrier.
template <typename Body>
__device__ __forceinline__ void walk_rows(const Parent& P, const uint32_t* bm, int* s_list, int* s_cnt, Body& body) {
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    for (int wi = threadIdx.x; wi < P.W; wi += ENC_THREADS) {
        uint32_t bits = bm[wi];
        while (bits) {
            const int w = wi * 32 + (__ffs((int)bits) - 1);
            bits &= bits - 1;
            const int b = P.rowptr[w], e = P.rowptr[w + 1];
            if (e - b >= ROW_LONG) {
                const int slot = atomicAdd(s_cnt, 1);
                if (slot < LONG_CAP) { s_list[slot] = w; continue; }
            }
            body.serial(w, b, e);
        }
    }
    __syncthreads();
    const int nl = min(*s_cnt, LONG_CAP);
    for (int i = threadIdx.x >> 6; i < nl; i += ENC_WAVES) {
        const int w = s_list[i];
        body.wave(w, P.rowptr[w], P.rowptr[w + 1], lane_id());
    }
    __syncthreads();
}

// one BFS level: the unvisited neighbours of the current level go into nxt
struct MarkBody {
    const Parent& P;
    Maps M;
    int u, v;
    __device__ __forceinline__ void entry(int w, int k) {
        const int j = P.col[k];
        if (walkable(P, w, j, k, u, v) && !bit_of(M.vis, j)) atomicOr(&M.nxt[j >> 5], 1u << (j & 31));
    }
    __device__ __forceinline__ void serial(int w, int b, int e) { for (int k = b; k < e; ++k) entry(w, k); }
    __device__ __forceinline__ void wave(int w, int b, int e, int lane) { for (int k = b + lane; k < e; k += WAVE) entry(w, k); }
};

// entries of the induced subgraph: walkable, source visited
struct CountBody {
    const Parent& P;
    Maps M;
    int u, v;
    int total;
    __device__ __forceinline__ bool take(int w, int k) {
        const int j = P.col[k];
        return walkable(P, w, j, k, u, v) && bit_of(M.vis, j);
    }
    __device__ __forceinline__ void serial(int w, int b, int e) { for (int k = b; k < e; ++k) total += take(w, k) ? 1 : 0; }
    __device__ __forceinline__ void wave(int w, int b, int e, int lane) { for (int k = b + lane; k < e; k += WAVE) total += take(w, k) ? 1 : 0; }
};

// Mark + count of one sample: cnt[g] = n_g, cnt[B + g] = e_g (the two added target columns included); the workspace keeps visited and
// its popcount prefix for npi_enclose_fill
__global__ void __launch_bounds__(ENC_THREADS)
enclose_mark_kernel(Parent P, const int32_t* __restrict__ keys, int B, int hops, int add, uint32_t* ws, int32_t* __restrict__ cnt,
                    int32_t* status) {
    __shared__ int s_list[LONG_CAP];
    __shared__ int s_cnt, s_flag, s_edges;
    __shared__ int s_part[ENC_THREADS];
    const int g = blockIdx.x, t = threadIdx.x;
    const Maps M = maps_of(ws, P.W, g);
    const int u = keys[2 * g], v = keys[2 * g + 1];
    const bool bad = u == v || u < 0 || v < 0 || u >= P.N || v >= P.N;
    for (int wi = t; wi < P.W; wi += ENC_THREADS) {
        uint32_t s = 0;
        if (!bad) s = ((u >> 5) == wi ? 1u << (u & 31) : 0u) | ((v >> 5) == wi ? 1u << (v & 31) : 0u);
        M.vis[wi] = s; M.cur[wi] = s; M.nxt[wi] = 0; M.prefix[wi] = 0;
    }
    if (t == 0) s_edges = 0;
    if (bad) {                                              // Rule H: an empty sample
        if (t == 0) {
            cnt[g] = 0; cnt[B + g] = 0;
            if (status != nullptr) atomicOr(status, NPI_STATUS_BAD_ENCLOSE_KEY);
        }
        return;
    }
    __syncthreads();
    MarkBody mark{P, M, u, v};
    for (int level = 0; level < hops; ++level) {
        if (t == 0) s_flag = 0;
        walk_rows(P, M.cur, s_list, &s_cnt, mark);
        bool any = false;
        for (int wi = t; wi < P.W; wi += ENC_THREADS) {
            // (the bits were set by atomics of this workgroup: read where the atomics ran)
            const uint32_t nw = __hip_atomic_load(&M.nxt[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~M.vis[wi];
            if (nw) { M.vis[wi] |= nw; any = true; }
            M.cur[wi] = nw;
            M.nxt[wi] = 0;
        }
        if (any) s_flag = 1;
        __syncthreads();
        if (!s_flag) break;                                 // nothing new: the component is exhausted
        __syncthreads();                                    // (s_flag is cleared at the top of the next level)
    }
    // n_g and the exclusive popcount prefix per word: local(w) = 2 + rank(w) - [u < w] - [v < w]
    const int per = (P.W + ENC_THREADS - 1) / ENC_THREADS;
    const int wb = min(P.W, t * per), we = min(P.W, wb + per);
    int mine = 0;
    for (int wi = wb; wi < we; ++wi) mine += __popc(M.vis[wi]);
    int all;
    int run = block_exclusive_scan<ENC_THREADS>(mine, s_part, &all);
    for (int wi = wb; wi < we; ++wi) { M.prefix[wi] = (uint32_t)run; run += __popc(M.vis[wi]); }
    CountBody count{P, M, u, v, 0};
    walk_rows(P, M.vis, s_list, &s_cnt, count);
    if (count.total) atomicAdd(&s_edges, count.total);
    __syncthreads();
    if (t == 0) { cnt[g] = all; cnt[B + g] = s_edges + (add ? 2 : 0); }
}

// node_off / edge_off = exclusive prefix sums of cnt[0 .. B) / cnt[B .. 2B); one workgroup.  Both totals are -1 when either passes 2^31 - 1
__global__ void __launch_bounds__(1024)
enclose_scan_kernel(const int32_t* __restrict__ cnt, int B, int32_t* __restrict__ node_off, int32_t* __restrict__ edge_off) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int b = min(B, t * per), e = min(B, b + per);
    long long sn = 0, se = 0;
    for (int g = b; g < e; ++g) { sn += cnt[g]; se += cnt[B + g]; }
    long long alln, alle;
    long long rn = block_exclusive_scan<1024>(sn, part, &alln);
    long long re = block_exclusive_scan<1024>(se, part, &alle);
    const bool fits = alln < NPI_INDEX_LIMIT && alle < NPI_INDEX_LIMIT;
    for (int g = b; g < e; ++g) {
        node_off[g] = fits ? (int)rn : 0;
        edge_off[g] = fits ? (int)re : 0;
        rn += cnt[g];
        re += cnt[B + g];
    }
    if (t == 1023) {
        node_off[B] = fits ? (int)alln : -1;
        edge_off[B] = fits ? (int)alle : -1;
    }
}

struct Out {
    int32_t* node_id;
    int64_t* batch;
    int64_t *esrc, *edst, *e_id;
    int32_t *lrowptr, *lcol;
    int32_t *graph_ptr, *edge_ptr;       // the offsets as the consumers get them: the device's, or on a mismatch one graph of the caller's size
};

__device__ __forceinline__ int local_of(const Maps& M, int w, int u, int v) {
    if (w == u) return 0;
    if (w == v) return 1;
    const int rank = (int)M.prefix[w >> 5] + __popc(M.vis[w >> 5] & ((1u << (w & 31)) - 1u));
    return 2 + rank - (u < w ? 1 : 0) - (v < w ? 1 : 0);
}

// a row's place in the batch, and its number of emitted entries into lrowptr (scanned afterwards)
struct RowBody {
    const Parent& P;
    Maps M;
    Out O;
    int u, v, g, n0, add;
    __device__ __forceinline__ bool take(int w, int k) {
        const int j = P.col[k];
        return walkable(P, w, j, k, u, v) && bit_of(M.vis, j);
    }
    __device__ __forceinline__ void head(int w, int c) {
        const int a = local_of(M, w, u, v);
        O.node_id[n0 + a] = w;
        O.batch[n0 + a] = g;
        O.lrowptr[n0 + a] = c + (add && a < 2 ? 1 : 0);
    }
    __device__ __forceinline__ void serial(int w, int b, int e) {
        int c = 0;
        for (int k = b; k < e; ++k) c += take(w, k) ? 1 : 0;
        head(w, c);
    }
    __device__ __forceinline__ void wave(int w, int b, int e, int lane) {
        int c = 0;
        for (int k0 = b; k0 < e; k0 += WAVE) c += __popcll(__ballot(k0 + lane < e && take(w, k0 + lane)));
        if (lane == 0) head(w, c);
    }
};

// the entries of a row, in the parent's order, at the row's scanned offset
struct EmitBody {
    const Parent& P;
    Maps M;
    Out O;
    int u, v, n0, add;
    __device__ __forceinline__ void put(int64_t pos, int w_row, int k) {
        const int src = n0 + local_of(M, P.col[k], u, v);
        O.esrc[pos] = src; O.edst[pos] = w_row; O.e_id[pos] = P.eid[k]; O.lcol[pos] = src;
    }
    // the added target column in front of rows 0 and 1: (1 -> 0) and (0 -> 1), e_id -1
    __device__ __forceinline__ int64_t target_edge(int64_t pos, int a) {
        if (!(add && a < 2)) return pos;
        O.esrc[pos] = n0 + 1 - a; O.edst[pos] = n0 + a; O.e_id[pos] = -1; O.lcol[pos] = n0 + 1 - a;
        return pos + 1;
    }
    __device__ __forceinline__ bool take(int w, int k) {
        const int j = P.col[k];
        return walkable(P, w, j, k, u, v) && bit_of(M.vis, j);
    }
    __device__ __forceinline__ void serial(int w, int b, int e) {
        const int a = local_of(M, w, u, v);
        int64_t pos = target_edge(O.lrowptr[n0 + a], a);
        for (int k = b; k < e; ++k)
            if (take(w, k)) put(pos++, n0 + a, k);
    }
    __device__ __forceinline__ void wave(int w, int b, int e, int lane) {
        const int a = local_of(M, w, u, v);
        int64_t pos = O.lrowptr[n0 + a];
        if (lane == 0) target_edge(pos, a);
        pos += (add && a < 2) ? 1 : 0;
        for (int k0 = b; k0 < e; k0 += WAVE) {
            const int k = k0 + lane;
            const bool tk = k < e && take(w, k);
            const uint64_t m = __ballot(tk);
            if (tk) put(pos + __popcll(m & ((1ull << lane) - 1ull)), n0 + a, k);
            pos += __popcll(m);
        }
    }
};

__global__ void __launch_bounds__(ENC_THREADS)
enclose_fill_kernel(Parent P, const int32_t* __restrict__ keys, int B, int add, uint32_t* ws, const int32_t* __restrict__ node_off,
                    const int32_t* __restrict__ edge_off, Out O, int n_nodes, int n_edges, int32_t* status) {
    __shared__ int s_list[LONG_CAP];
    __shared__ int s_cnt;
    __shared__ int s_part[ENC_THREADS];
    const int g = blockIdx.x, t = threadIdx.x;
    // the arrays were sized from the CALLER's totals, the offsets are the device's (subgraph.hip's convention): on a mismatch nothing
    // is written through them -- node 0 / graph 0 rows, (-1, -1) columns and empty local rows within the caller's sizes, and a status bit
    if (node_off[B] != n_nodes || edge_off[B] != n_edges) {
        if (g == 0 && t == 0 && status != nullptr) atomicOr(status, NPI_STATUS_BAD_ENCLOSE_TOTALS);
        const int64_t nt = (int64_t)gridDim.x * ENC_THREADS;
        const int64_t first = (int64_t)g * ENC_THREADS + t;
        for (int64_t i = first; i < n_nodes; i += nt) { O.node_id[i] = 0; O.batch[i] = 0; }
        for (int64_t i = first; i <= n_nodes; i += nt) O.lrowptr[i] = 0;
        for (int64_t i = first; i <= B; i += nt) { O.graph_ptr[i] = i == 0 ? 0 : n_nodes; O.edge_ptr[i] = i == 0 ? 0 : n_edges; }
        for (int64_t i = first; i < n_edges; i += nt) { O.esrc[i] = -1; O.edst[i] = -1; O.e_id[i] = -1; O.lcol[i] = 0; }
        return;
    }
    const int n0 = node_off[g], ng = node_off[g + 1] - n0, e0 = edge_off[g];
    if (t == 0) {
        O.graph_ptr[g] = n0; O.edge_ptr[g] = e0;
        if (g == B - 1) { O.graph_ptr[B] = n_nodes; O.edge_ptr[B] = n_edges; O.lrowptr[n_nodes] = n_edges; }
    }
    if (ng == 0) return;                                    // a bad key
    const Maps M = maps_of(ws, P.W, g);
    const int u = keys[2 * g], v = keys[2 * g + 1];
    RowBody rows{P, M, O, u, v, g, n0, add};
    walk_rows(P, M.vis, s_list, &s_cnt, rows);
    // lrowptr[n0 .. n0 + ng): counts -> e0 + their exclusive prefix, in place
    const int per = (ng + ENC_THREADS - 1) / ENC_THREADS;
    const int rb = min(ng, t * per), re = min(ng, rb + per);
    int mine = 0;
    for (int a = rb; a < re; ++a) mine += O.lrowptr[n0 + a];
    int all;
    int run = e0 + block_exclusive_scan<ENC_THREADS>(mine, s_part, &all);
    for (int a = rb; a < re; ++a) {
        const int c = O.lrowptr[n0 + a];
        O.lrowptr[n0 + a] = run;
        run += c;
    }
    __syncthreads();
    EmitBody emit{P, M, O, u, v, n0, add};
    walk_rows(P, M.vis, s_list, &s_cnt, emit);
}

// Rule H 5 over any batch of graphs given as a by-target CSR over the batch's rows: graph g is the rows [graph_ptr[g], graph_ptr[g + 1]),
// its targets src[g] / dst[g] (nullptr: its first two rows).  Two pull-style BFS at once, one workgroup per graph: at level L a row not
// yet reached takes L + 1 from any source that holds L.  Every index is clamped to the arrays (n rows, nnz entries) and an entry whose
// source is outside the graph, or the row itself, is skipped, so the kernel is safe on any input.
__global__ void __launch_bounds__(ENC_THREADS)
drnl_label_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n, int nnz, const int32_t* __restrict__ src,
                  const int32_t* __restrict__ dst, const int32_t* __restrict__ graph_ptr, int64_t* __restrict__ z, int32_t* dist) {
    __shared__ int s_list[LONG_CAP];
    __shared__ int s_cnt, s_changed;
    const int g = blockIdx.x, t = threadIdx.x, lane = lane_id();
    const int b = min(max(graph_ptr[g], 0), n), e = min(max(graph_ptr[g + 1], b), n);
    if (e <= b) return;
    int s = src ? src[g] : b, d = dst ? dst[g] : b + 1;
    const bool ok = s >= b && s < e && d >= b && d < e && s != d;
    for (int a = b + t; a < e; a += ENC_THREADS) {
        dist[2 * (int64_t)a] = (ok && a == s) ? 0 : -1;
        dist[2 * (int64_t)a + 1] = (ok && a == d) ? 0 : -1;
        if (!ok) z[a] = 0;
    }
    if (!ok) return;
    __syncthreads();
    for (int L = 0; L < e - b; ++L) {                       // a distance is below n_g: the loop ends for any input
        if (t == 0) { s_changed = 0; s_cnt = 0; }
        __syncthreads();
        bool changed = false;
        for (int a = b + t; a < e; a += ENC_THREADS) {
            const bool need0 = dist[2 * (int64_t)a] < 0 && a != d;        // from src with dst removed
            const bool need1 = dist[2 * (int64_t)a + 1] < 0 && a != s;    // from dst with src removed
            if (!need0 && !need1) continue;
            const int kb = min(max(rowptr[a], 0), nnz), ke = min(max(rowptr[a + 1], kb), nnz);
            if (ke - kb >= ROW_LONG) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < LONG_CAP) { s_list[slot] = a; continue; }
            }
            bool f0 = false, f1 = false;
            for (int k = kb; k < ke; ++k) {
                const int j = col[k];
                if (j < b || j >= e || j == a) continue;
                f0 = f0 || (need0 && dist[2 * (int64_t)j] == L);
                f1 = f1 || (need1 && dist[2 * (int64_t)j + 1] == L);
                if ((f0 || !need0) && (f1 || !need1)) break;
            }
            if (f0) dist[2 * (int64_t)a] = L + 1;
            if (f1) dist[2 * (int64_t)a + 1] = L + 1;
            changed = changed || f0 || f1;
        }
        __syncthreads();
        const int nl = min(s_cnt, LONG_CAP);
        for (int i = t >> 6; i < nl; i += ENC_WAVES) {
            const int a = s_list[i];
            const bool need0 = dist[2 * (int64_t)a] < 0 && a != d;
            const bool need1 = dist[2 * (int64_t)a + 1] < 0 && a != s;
            const int kb = min(max(rowptr[a], 0), nnz), ke = min(max(rowptr[a + 1], kb), nnz);
            bool f0 = false, f1 = false;
            for (int k0 = kb; k0 < ke; k0 += WAVE) {
                const int k = k0 + lane;
                const int j = k < ke ? col[k] : -1;
                const bool in = j >= b && j < e && j != a;
                f0 = f0 || __ballot(in && need0 && dist[2 * (int64_t)(in ? j : b)] == L) != 0;
                f1 = f1 || __ballot(in && need1 && dist[2 * (int64_t)(in ? j : b) + 1] == L) != 0;
                if ((f0 || !need0) && (f1 || !need1)) break;
            }
            if (lane == 0) {
                if (f0) dist[2 * (int64_t)a] = L + 1;
                if (f1) dist[2 * (int64_t)a + 1] = L + 1;
            }
            changed = changed || f0 || f1;
        }
        if (changed) s_changed = 1;
        __syncthreads();
        if (!s_changed) break;
        __syncthreads();
    }
    for (int a = b + t; a < e; a += ENC_THREADS) {
        const int du = dist[2 * (int64_t)a], dv = dist[2 * (int64_t)a + 1];
        int64_t lab;
        if (a == s || a == d) lab = 1;
        else if (du < 0 || dv < 0) lab = 0;
        else {
            const int64_t dd = (int64_t)du + dv, half = dd / 2;
            lab = 1 + min(du, dv) + half * (half + dd % 2 - 1);
        }
        z[a] = lab;
    }
}

// x[row] = [label | feat[node_id[row]]]; label: float(z) (NPI_ENCLOSE_LABEL_DRNL), 0 for a sample's two targets and 1 elsewhere
// (NPI_ENCLOSE_LABEL_TARGETS) or no column; the pad columns up to ldx are set to zero
__global__ void __launch_bounds__(256)
enclose_features_kernel(const float* __restrict__ feat, int64_t ldf, int Ff, const int32_t* __restrict__ node_id,
                        const int64_t* __restrict__ z, const int64_t* __restrict__ batch, const int32_t* __restrict__ node_off,
                        const int32_t* __restrict__ edge_off, int B, int64_t n, int64_t e, int label, float* __restrict__ x, int64_t ldx) {
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    float* __restrict__ out = x + row * ldx;
    if (node_off[B] != n || edge_off[B] != e) {            // npi_enclose_fill raised the status bit: node_id is a placeholder -- zero rows
        for (int c = lane; c < ldx; c += WAVE) out[c] = 0.f;
        return;
    }
    const int lc = label == NPI_ENCLOSE_LABEL_NONE ? 0 : 1;
    if (lc && lane == 0)
        out[0] = label == NPI_ENCLOSE_LABEL_DRNL ? (float)z[row] : ((row - node_off[batch[row]] < 2) ? 0.f : 1.f);
    const float* __restrict__ in = feat + (int64_t)node_id[row] * ldf;
    for (int c = lane; lc + c < ldx; c += WAVE) out[lc + c] = c < Ff ? in[c] : 0.f;
}

static bool parent_ok(const int32_t* rowptr, const int32_t* col, const int32_t* eid) { return rowptr && col && eid; }

}  // namespace npi

using namespace npi;

extern "C" int64_t npi_enclose_workspace_bytes(int64_t N, int64_t B) {
    if (!id_bound_ok(N) || B < 0 || B >= 0x3fffffff) return -1;
    const int64_t W = ceil_div(N, 32);
    return align_up(B * 4 * W * (int64_t)sizeof(uint32_t), 16);
}

extern "C" int npi_enclose_sizes(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const uint8_t* mask, int64_t N,
                                 const int32_t* keys, int64_t B, int64_t hops, int flags, int32_t* counts, int32_t* node_off,
                                 int32_t* edge_off, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(id_bound_ok(N) && B >= 0 && B < 0x3fffffff, "npi_enclose_sizes: bad size");
    NPI_REQUIRE(hops >= 1 && hops < NPI_INDEX_LIMIT, "npi_enclose_sizes: hops must be at least 1");
    NPI_REQUIRE((flags & ~NPI_ENCLOSE_ADD_TARGET_EDGE) == 0, "npi_enclose_sizes: unknown flag");
    NPI_REQUIRE(workspace_bytes >= 0, "npi_enclose_sizes: negative workspace length");
    NPI_REQUIRE(node_off && edge_off, "npi_enclose_sizes: null pointer");
    if (B > 0) {
        NPI_REQUIRE(parent_ok(rowptr, col, eid) && keys && counts && workspace, "npi_enclose_sizes: null pointer");
        NPI_REQUIRE(((uintptr_t)workspace & 3) == 0, "npi_enclose_sizes: misaligned workspace");
        if (workspace_short("npi_enclose_sizes", workspace_bytes, npi_enclose_workspace_bytes(N, B))) return NPI_ERR_ARG;
        const Parent P{rowptr, col, eid, mask, (int)N, (int)ceil_div(N, 32)};
        enclose_mark_kernel<<<(unsigned)B, ENC_THREADS, 0, stream>>>(P, keys, (int)B, (int)hops, flags & NPI_ENCLOSE_ADD_TARGET_EDGE ? 1 : 0,
                                                                     (uint32_t*)workspace, counts, status);
    }
    enclose_scan_kernel<<<1, 1024, 0, stream>>>(counts, (int)B, node_off, edge_off);
    return check_launch("npi_enclose_sizes");
}

extern "C" int npi_enclose_fill(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const uint8_t* mask, int64_t N,
                                const int32_t* keys, int64_t B, int flags, const int32_t* node_off, const int32_t* edge_off,
                                void* workspace, int64_t workspace_bytes, int32_t* node_id, int64_t* batch, int64_t* edge_src,
                                int64_t* edge_dst, int64_t* e_id, int32_t* local_rowptr, int32_t* local_col, int32_t* graph_ptr,
                                int32_t* edge_ptr, int64_t n_nodes, int64_t n_edges, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(id_bound_ok(N) && B >= 0 && B < 0x3fffffff, "npi_enclose_fill: bad size");
    NPI_REQUIRE(count_ok(n_nodes) && count_ok(n_edges), "npi_enclose_fill: bad totals");
    NPI_REQUIRE((flags & ~NPI_ENCLOSE_ADD_TARGET_EDGE) == 0, "npi_enclose_fill: unknown flag");
    NPI_REQUIRE(workspace_bytes >= 0, "npi_enclose_fill: negative workspace length");
    NPI_REQUIRE(local_rowptr && graph_ptr && edge_ptr, "npi_enclose_fill: null pointer");
    if (B == 0) {
        (void)hipMemsetAsync(local_rowptr, 0, sizeof(int32_t), stream);
        (void)hipMemsetAsync(graph_ptr, 0, sizeof(int32_t), stream);
        (void)hipMemsetAsync(edge_ptr, 0, sizeof(int32_t), stream);
        return check_launch("npi_enclose_fill");
    }
    NPI_REQUIRE(parent_ok(rowptr, col, eid) && keys && node_off && edge_off && workspace, "npi_enclose_fill: null pointer");
    NPI_REQUIRE(n_nodes == 0 || (node_id && batch), "npi_enclose_fill: null pointer");
    NPI_REQUIRE(n_edges == 0 || (edge_src && edge_dst && e_id && local_col), "npi_enclose_fill: null pointer");
    NPI_REQUIRE(((uintptr_t)workspace & 3) == 0, "npi_enclose_fill: misaligned workspace");
    if (workspace_short("npi_enclose_fill", workspace_bytes, npi_enclose_workspace_bytes(N, B))) return NPI_ERR_ARG;
    const Parent P{rowptr, col, eid, mask, (int)N, (int)ceil_div(N, 32)};
    const Out O{node_id, batch, edge_src, edge_dst, e_id, local_rowptr, local_col, graph_ptr, edge_ptr};
    enclose_fill_kernel<<<(unsigned)B, ENC_THREADS, 0, stream>>>(P, keys, (int)B, flags & NPI_ENCLOSE_ADD_TARGET_EDGE ? 1 : 0,
                                                                 (uint32_t*)workspace, node_off, edge_off, O, (int)n_nodes, (int)n_edges,
                                                                 status);
    return check_launch("npi_enclose_fill");
}

extern "C" int npi_drnl_label(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const int32_t* src, const int32_t* dst,
                              const int32_t* graph_ptr, int64_t B, int64_t* z, int32_t* dist, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(count_ok(n) && count_ok(nnz) && B >= 0 && B < 0x3fffffff, "npi_drnl_label: bad size");
    NPI_REQUIRE((src == nullptr) == (dst == nullptr), "npi_drnl_label: src and dst go together");
    if (n == 0 || B == 0) return NPI_OK;
    NPI_REQUIRE(rowptr && graph_ptr && z && dist && (nnz == 0 || col), "npi_drnl_label: null pointer");
    drnl_label_kernel<<<(unsigned)B, ENC_THREADS, 0, stream>>>(rowptr, col, (int)n, (int)nnz, src, dst, graph_ptr, z, dist);
    return check_launch("npi_drnl_label");
}

extern "C" int npi_enclose_features(const float* feat, int64_t ldf, int64_t Ff, const int32_t* node_id, const int64_t* z,
                                    const int64_t* batch, const int32_t* node_off, const int32_t* edge_off, int64_t B, int64_t n,
                                    int64_t e, int label, float* x, int64_t ldx, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NPI_REQUIRE(label == NPI_ENCLOSE_LABEL_NONE || label == NPI_ENCLOSE_LABEL_DRNL || label == NPI_ENCLOSE_LABEL_TARGETS,
                "npi_enclose_features: unknown label");
    const int64_t lc = label == NPI_ENCLOSE_LABEL_NONE ? 0 : 1;
    NPI_REQUIRE(n >= 0 && n < NPI_INDEX_LIMIT && e >= 0 && e < NPI_INDEX_LIMIT && B >= 0 && B < 0x3fffffff && Ff >= 0 && Ff < NPI_INDEX_LIMIT && Ff + lc > 0 && ldf >= Ff &&
                ldx >= Ff + lc && ldx < NPI_INDEX_LIMIT, "npi_enclose_features: bad size");
    if (n == 0) return NPI_OK;
    NPI_REQUIRE(node_id && batch && node_off && edge_off && x && (Ff == 0 || feat) && (label != NPI_ENCLOSE_LABEL_DRNL || z),
                "npi_enclose_features: null pointer");
    enclose_features_kernel<<<(unsigned)ceil_div(n, 4), 256, 0, stream>>>(feat, ldf, (int)Ff, node_id, z, batch, node_off, edge_off, (int)B,
                                                                          n, e, label, x, ldx);
    return check_launch("npi_enclose_features");
}
