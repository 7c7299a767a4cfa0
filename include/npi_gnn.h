/*
 * npi_gnn.h -- C ABI of the MI355X (gfx950) message-passing engine for NPI-GNN's conv hot path.
 *
 * Drop-in boundary: the reference reaches this path through the PyG
 * `nn.Conv` module interface -- `SAGEConv(in,128)` constructed at reference src/classes.py:48,50,52
 * and called as `conv(x, edge_index)` at src/classes.py:62,66,70; backward through autograd at
 * src/train_with_twoDataset.PY:54.  The arithmetic lives in torch-geometric 1.4.2 / torch-scatter
 * (un-vendored, reference README.md:11).  The reference has no FFI of its own for this path; the
 * entry points below are what a ctypes binding inside a PyG-style `MessagePassing.propagate`
 * replacement binds.  Each entry point names the PyG-1.4.2 op it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (PyTorch's caching allocator);
 *     the library never frees or retains the caller's memory and NO entry point allocates (ABI 3: the library
 *     imports no hipMalloc* / hipFree*): every scratch buffer is a caller workspace with a size query next to it;
 *   - the library keeps NO process-wide state and reads no environment variable (ABI 3: the setters npi_gemm_mode,
 *     npi_dw_shared, npi_small_graph_entries of ABI 2 and the entry points that consulted them are gone): the GEMM
 *     arithmetic, the dW grid regime and the item size of a CSR are arguments of the calls they concern; calls on
 *     different streams from different threads are independent.  npi_item_edges() is a pure function of its argument;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call is asynchronous on it and performs no host synchronisation;
 *   - return value: 0 = ok, <0 = error (text via npi_last_error(), thread-local); no C++
 *     exception crosses the ABI, nothing calls exit();
 *   - node ids in CSR arrays are int32 (N + E + 1 < 2^31); the COO input is int64 as PyG hands it
 *     over (`edge_index` LongTensor [2,E], row 0 = source j, row 1 = target i);
 *   - ABI 4 (npi_abi_version() == 4): ONE entry point per operation.  The `_ex2` forms of ABI 3 (their `_ex` / plain twins plus one
 *     optional pointer: row scales in or out) and the plain forms of npi_topk_select / npi_topk_gather / npi_filter_adj are folded
 *     into the base names, which now take that pointer / flag (NULL / 0 = the old behaviour); npi_entry_col_scale is new.
 */
#ifndef NPI_GNN_H
#define NPI_GNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPI_OK 0
#define NPI_ERR_ARG (-1)      /* bad argument (null pointer, negative size, unsupported width) */
#define NPI_ERR_LAUNCH (-2)   /* HIP launch / runtime error */
#define NPI_ERR_WORKSPACE (-3)/* workspace too small */

/* entries of the self-loop-augmented CSR that one wavefront ("item") reduces: a property of each CSR, 64 or NPI_ITEM_EDGES,
 * chosen by whoever builds it (npi_item_edges(nnz_max) = the recommended value) and passed as `item_edges` to the build and
 * to every entry point that takes `item_row` */
#ifndef NPI_ITEM_EDGES
#define NPI_ITEM_EDGES 256
#endif

/* data types of feature matrices */
#define NPI_F32 0
#define NPI_BF16 1

const char* npi_last_error(void);
int npi_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Graph build.  Replaces PyG `add_remaining_self_loops` (SAGEConv.forward / GCNConv.norm) and
 * the implicit "group messages by target" that torch_scatter does with atomics: a STABLE LSD
 * radix sort of the COO columns by `key` node, so that within one row the entries keep their
 * edge_index order and the appended self loop comes last -- exactly the accumulation order of
 * the reference's CPU scatter.
 *
 *   key_nodes[E], val_nodes[E] : int64 device arrays.  CSR-by-target: key = edge_index[1],
 *                                val = edge_index[0].  CSR-by-source (transpose, for backward):
 *                                swap them.
 *   Columns with key == val (existing self loops) and columns with an id outside [0,N) are
 *   dropped; the latter also set bit 0 of status[0] -- except the padding column (-1, -1) of
 *   npi_filter_adj, which is dropped silently.
 *   add_self_loops != 0 appends (i,i) as the LAST entry of every row.
 *
 *   rowptr[N+1]  : int32, rowptr[N] = nnz (device-side; nnz <= E + N)
 *   col[E+N]     : int32 neighbour (val) node per entry
 *   eid[E+N]     : int32 original column in edge_index, -1 for an appended self loop (may be NULL)
 *   rowidx[E+N]  : int32 key node per entry, i.e. the sorted COO row (may be NULL)
 *   item_row[npi_num_items(E+N, item_edges)+1] : int32 first row of every item of item_edges entries
 *   item_edges   : 64 or NPI_ITEM_EDGES -- the item size of THIS CSR; hand the same value to every call that takes item_row
 *   status[1]    : int32 device word, bit 0 = out-of-range id seen
 * ------------------------------------------------------------------------------------------ */
int64_t npi_csr_workspace_bytes(int64_t E, int64_t N);
/* recommended item size for a new CSR of capacity nnz_max: 64 below 2^22 entries, NPI_ITEM_EDGES from there on.  A pure
 * function and a hint only -- nothing that consumes a CSR calls it; a caller that wants the other size passes it. */
int64_t npi_item_edges(int64_t nnz_max);
int64_t npi_num_items(int64_t nnz_max, int64_t item_edges);   /* ceil(nnz_max / item_edges); -1 for an item size that does not exist */

/* Same build with separate row and column id spaces, for a destination-row SHARD of the graph on
 * one GPU: keys are local row ids in [0, N), values index a feature table of
 * n_cols rows (e.g. the all-gathered x of every rank); the appended self loop of row r gets
 * column r + loop_col_offset.  build_flags: NPI_CSR_DROP_EQUAL drops key == val columns (0: the caller has
 * already removed the global self loops); NPI_CSR_SORT_COLUMNS orders the entries of a row by column
 * (ties: list order) instead of list order -- a second key for the build's sort, for graphs whose rows are
 * long: the 4-byte gathers of per-node scalars (GATConv) then walk ascending addresses.  The SUMS are the
 * same in another association. */
#define NPI_CSR_DROP_EQUAL 1
#define NPI_CSR_SORT_COLUMNS 2
int npi_csr_build_ex(const int64_t* key_nodes, const int64_t* val_nodes, int64_t E, int64_t N,
                     int64_t n_cols, int add_self_loops, int64_t loop_col_offset, int build_flags,
                     int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* rowidx,
                     int32_t* item_row, int64_t item_edges, int32_t* status,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* inverse map for per-edge data that lives in one CSR's entry order and is needed in the other's:
 * pos_of[e] for e in [0,E) = entry index of edge column e in the CSR given by (eid, nnz_max), or -1 */
int npi_edge_positions(const int32_t* eid, const int32_t* rowptr, int64_t N, int64_t nnz_max,
                       int64_t E, int32_t* pos_of, void* stream);

/* ------------------------------------------------------------------------------------------
 * Segmented row reduction over a CSR -- replaces `torch.index_select(x, 0, edge_index[0])`
 * followed by `torch_scatter.scatter_{add,mean}(x_j, edge_index[1], dim_size=N)`
 * (PyG MessagePassing.propagate, reached from reference src/classes.py:62,66,70), without
 * materialising the [E+N, F] message tensor and without float atomics:
 *
 *     out[i, :] = scale_i * sum_{p in [rowptr[i], rowptr[i+1])}  w[p] * x[col[p], :]  (+ bias[:])
 *
 *   mean != 0  : scale_i = 1 / max(rowptr[i+1]-rowptr[i], 1)   (scatter_mean)
 *   w == NULL  : all ones (SAGE);  otherwise one f32 per CSR entry (GCN norm / GAT alpha)
 *   x, out     : [N, F] row-major, leading dimension ldx / ldo (elements), dtype f32 or bf16
 *                (bf16 storage, f32 accumulation)
 *   item_row, item_edges : as the CSR was built (npi_csr_build_ex / npi_csr_filter)
 *   carry      : f32 scratch, npi_segsum_carry_elems(nnz_max, item_edges, F) elements: the partial sums of rows cut by a
 *                workgroup boundary and the agent-scope arrival counters through which the LAST workgroup to deliver a
 *                partial of a row sums that row's chain inside the same launch (in a fixed order => bitwise reproducible;
 *                no second launch).  ZERO IT ONCE after allocating it: every launch resets the counters it used, so the
 *                buffer can be reused launch after launch (any width F' <= F, this CSR or another of no larger capacity);
 *                two launches that may run CONCURRENTLY need two buffers.
 * ------------------------------------------------------------------------------------------ */
int64_t npi_segsum_carry_elems(int64_t nnz_max, int64_t item_edges, int64_t F);
/* x2 != NULL: a TWO-PART feature table -- an entry with col[p] < split reads row col[p] of x, any other entry row
 * col[p] - split of x2 (same leading dimension and dtype).  One rank of the sharded layers (npi_gnn_amd/dist.py, SURVEY.md
 * 8(e)) gathers from [hub rows received from all ranks ; its own rows] without copying its own rows behind the received
 * ones.  x2 == NULL (split ignored): one table. */
/* row_scales_out != NULL: the launch also writes, for every finished row, the power-of-two scale the projection GEMM behind the
 * aggregation takes as `a_scales` (NPI_GEMM_SPLIT_F16X2; the same values npi_row_scales would compute from `out` in a pass of its
 * own): a wave maximum and one 4-byte store per row.  [N] or NULL.  Only f32 rows of 256 columns, 16-byte aligned, on a graph
 * with entries: npi_segsum_scales_supported(F, dtype).  (ABI 4: the separate scales-writing twin of ABI 3, folded.) */
int npi_segsum_scales_supported(int64_t F, int dtype);
int npi_segsum_ex(const int32_t* rowptr, const int32_t* col, const int32_t* item_row, int64_t item_edges,
                   const float* w, int64_t N, int64_t nnz_max, const void* x, int64_t ldx,
                   const void* x2, int64_t split, void* out, int64_t ldo, int64_t F, int dtype, int mean,
                   const float* bias, float* carry, float* row_scales_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The heaviest rows of a side ("hubs") aggregated by streaming the source table once instead of gathering it.
 * A row that holds a sizeable fraction of all columns re-reads a table no cache can hold; streamed, every source row is
 * fetched once and added into the accumulators of the hubs its mask names.  f32, F = 256; N rows over a table of n_cols rows
 * (N == n_cols for the sides of a square graph; the two id spaces of a bipartite side are independent: every kernel below walks
 * rows with N and masks / table rows with n_cols).
 *
 * npi_hub_plan (once per graph and side): the up to h_max <= NPI_HUB_MAX rows with the most entries among the rows with at
 * least min_degree entries (ties: the lower row first), minus rows that hold a column twice (a mask bit cannot count twice).
 *   hub_rows[NPI_HUB_MAX]   : int32, the hubs by descending degree; -1 behind the last
 *   mask[n_cols][NPI_HUB_MAX / 32] : uint32, bit j of mask[c] set iff the side has an entry (hub j, c) -- a self loop included
 *   info[4]                 : int32 device words: [0] H, the number of hubs -- 0 (plan EMPTY: use npi_segsum_ex alone) when their
 *                             entries add up to less than min_entries or more than 4,096 rows reach min_degree; [1] the entries of
 *                             the hub rows; [2] rows with >= min_degree entries; [3] hubs before the duplicate check
 *   workspace               : int32, npi_hub_plan_workspace_elems() elements
 * npi_hub_light_side: the same side with the hub rows EMPTY and every other entry in its order (arrays as npi_csr_build_ex writes
 * them, capacity nnz_max_light >= nnz - info[1]); npi_segsum_ex walks it unchanged and leaves zeros in the hub rows.
 * npi_segsum_hub (same stream, BEHIND the light side's npi_segsum_ex on the same `out`): for every hub j
 *     out[hub_rows[j], :] = scale_j * sum_{c : bit j of mask[c]} col_scale[c] * x[c, :]
 *   mean != 0   : scale_j = 1 / max(length of the ORIGINAL row, 1) (rowptr: the original side's); col_scale == NULL: ones
 *   partial     : f32 scratch, npi_segsum_hub_partial_elems(n_cols) elements, no need to clear; two launches that may run
 *                 concurrently need two buffers
 *   row_scales_out : as npi_segsum_ex (the hub rows' elements are overwritten)
 * No float atomics: every hub row is summed in a fixed order, bitwise reproducible from launch to launch.
 * ------------------------------------------------------------------------------------------ */
#define NPI_HUB_MAX 128
int64_t npi_hub_plan_workspace_elems(void);
int npi_hub_plan(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t n_cols, int64_t nnz_max, int64_t h_max,
                 int64_t min_degree, int64_t min_entries, int32_t* hub_rows, uint32_t* mask, int32_t* info, int32_t* workspace,
                 void* stream);
int npi_hub_light_side(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t N,
                       int64_t nnz_max, const int32_t* hub_rows, int64_t H, int64_t nnz_max_light, int64_t item_edges,
                       int32_t* rowptr_l, int32_t* col_l, int32_t* eid_l, int32_t* rowidx_l, int32_t* item_row_l, void* stream);
int64_t npi_segsum_hub_slabs(int64_t n_cols);
int64_t npi_segsum_hub_partial_elems(int64_t n_cols);
int npi_segsum_hub(const int32_t* hub_rows, int64_t H, const uint32_t* mask, const int32_t* rowptr, int64_t N, int64_t n_cols,
                   const float* col_scale, const float* x, int64_t ldx, float* out, int64_t ldo, int64_t F, int mean,
                   float* partial, float* row_scales_out, void* stream);

/* GCNConv.norm (PyG 1.4.2): deg[j] = sum of weights of entries in row j of the BY-SOURCE CSR
 * (deg == NULL: unweighted, the row lengths of deg_rowptr are used);
 * norm[p] = deg^-1/2[rowidx[p]] * w[p] * deg^-1/2[col[p]] for the entries of either CSR
 * (w == NULL: ones; deg^-1/2 of 0 is 0 as PyG masks inf). */
int npi_row_weight_sum(const int32_t* rowptr, const float* w, int64_t N, float* deg, void* stream);
int npi_gcn_norm(const int32_t* rowidx, const int32_t* col, const int32_t* rowptr, const float* w,
                 const float* deg, const int32_t* deg_rowptr, int64_t N, int64_t nnz_max, float* norm,
                 void* stream);
/* inv_cnt[i] = 1 / max(rowptr[i+1] - rowptr[i], 1): the scatter_mean divisor, needed again by the
 * backward (dX = A^T D^-1 dAgg) */
/* w_out[p] = table[col[p]] * w_in[p] (w_in == NULL: ones) for the entries p of one CSR, 0 behind its last entry: a per-NODE factor of
 * the gathered row as a per-entry weight.  The layers' backward uses it with table = npi_row_inv_count of the by-target CSR over the
 * by-source side: scatter_mean's divisor belongs to the TARGET, so dX = (A^T D^-1 dOut) W^T aggregates dOut itself with these
 * weights and projects afterwards (autograd of `scatter_mean` + `torch.matmul`, reference src/train_with_twoDataset.PY:54). */
int npi_entry_col_scale(const int32_t* col, const int32_t* rowptr, const float* table, const float* w_in, int64_t N, int64_t n_cols,
                        int64_t nnz_max, float* w_out, void* stream);
int npi_row_inv_count(const int32_t* rowptr, int64_t N, float* inv_cnt, void* stream);
/* per-entry weights from per-edge weights: w_entry[p] = eid[p] >= 0 ? edge_w[eid[p]] : loop_w
 * (loop weight of node i = loop_w_node[i] if given else fill) */
int npi_entry_weights(const int32_t* eid, const int32_t* rowidx, const int32_t* rowptr,
                      const float* edge_w, const float* loop_w_node, float fill,
                      int64_t N, int64_t nnz_max, float* w_entry, void* stream);
/* Gradients w.r.t. edge_weight of SAGEConv / GCNConv: what autograd computes for `edge_weight.view(-1, 1) * x_j` in front of the
 * scatter (PyG 1.4.2 SAGEConv.message / GCNConv.message: the backward of the broadcast multiply, a row-wise sum of
 * grad * x_j per edge) -- one dot product per entry p of one CSR side (i = rowidx[p]):
 *   g[p] = row_scale[i] * <a[i, :], b[col[p], :]>      a [N, F] (lda), read once per row; b [n_cols, F] (ldb), gathered
 * f32, any F; 16-byte lanes when F % 4 == 0 and both tables have 16-byte aligned rows.  row_scale [N] may be NULL (ones).
 * Outputs, each optional (NULL: not written; at least one):
 *   g_entry  [nnz_max]  g in entry order
 *   gm_entry [nnz_max]  g[p] * mul[p] (mul [nnz_max]: both or neither) -- g norm for npi_gcn_norm_bwd's row sums
 *   d_edge   [n_edges]  d_edge[eid[p]] = g[p] for eid[p] >= 0: every edge owns one entry of a side, so plain stores; elements of
 *                       edges without an entry (existing self loops, dropped or padding columns) are NOT written
 *   d_loop   [N]        d_loop[i] = g[p] for the implicit self loop of row i (eid[p] < 0)
 * No float atomics, fixed summation order: bitwise reproducible from launch to launch.  Nothing is allocated. */
int npi_edge_dot(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* eid, int64_t N, int64_t n_cols,
                 int64_t nnz_max, int64_t n_edges, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t F,
                 const float* row_scale, const float* mul, float* g_entry, float* gm_entry, float* d_edge, float* d_loop,
                 void* stream);
/* Backward of GCNConv.norm (PyG 1.4.2: deg = scatter_add(edge_weight, row); norm = deg^-1/2[row] * edge_weight * deg^-1/2[col];
 * autograd through the pow, the two gathers and the scatter_add) over the BY-TARGET CSR, g_entry = d loss / d norm per entry:
 *   d w_p = g_p deg^-1/2[j] deg^-1/2[i] - (s_a[j] + s_b[j]) / (2 deg[j])        i = rowidx[p] (target), j = col[p] (source)
 * s_a + s_b [N]: the sum of g norm over the entries whose source is k plus that over the entries whose target is k
 * (npi_seg_rowsum_ex over both orientations of npi_edge_dot's gm_entry; s_b may be NULL).  deg <= 0: both terms are 0.
 * Stored like npi_edge_dot's d_edge / d_loop (either may be NULL, not both). */
int npi_gcn_norm_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* eid, int64_t N,
                     int64_t nnz_max, int64_t n_edges, const float* g_entry, const float* deg, const float* s_a, const float* s_b,
                     float* d_edge, float* d_loop, void* stream);
/* Backward of the ReLU that SAGEConv(..., relu=True) applies in its projection epilogue (autograd's threshold_backward):
 * dz[r, c] = y[r, c] > 0 ? dy[r, c] : 0 over M rows of F floats, y = the layer's (post-ReLU) output. */
/* Measurement support (no reference counterpart): `workgroups` workgroups that each hold 64 KB of a CU's LDS for `nanoseconds` --
 * a stand-in for the resident kernel of a collective, launched by npi_gnn_amd.virtual.StubCollectives beside a rank's step so
 * that a one-GPU run has the duration of an exchange and the CUs it sits on.  `start_word` (device memory, ZERO before the
 * launch; may be null): the time runs from the moment the first workgroup got a CU -- one that waited for a wave slot leaves
 * with the others; null: every workgroup times its own start.  Computes nothing; <= 256 workgroups, <= 100 ms. */
int npi_hold_cus(int workgroups, int64_t nanoseconds, uint64_t* start_word, void* stream);
int npi_relu_backward(const float* dy, int64_t ldd, const float* y, int64_t ldy, int64_t M, int64_t F, float* dz, int64_t ldz,
                      void* stream);

/* Row gather into a column block of a wider buffer -- replaces the left half of `torch.cat([x[0][res_n_id], aggr_out], dim=-1)`
 * (PyG 1.4.2 SAGEConv.update, the bipartite `(x_src, x_dst)` form with concat=True): where torch gathers `x[0][res_n_id]` into a
 * tensor of its own and copies it again into the concatenation, this writes every gathered row once, straight into the left
 * half of the [n, 2F] operand of the projection GEMM (npi_segsum_ex writes the mean into the right half):
 *     out[i, 0:F] = x[idx[i], 0:F]     i < n;  x [n_src, F] (ldx), out [n, F] (ldo), leading dimensions in elements
 *   idx    : int64 [n] row ids (`res_n_id` as PyG hands it over) or NULL: the identity (then n <= n_src is expected)
 *   dtype  : NPI_F32 or NPI_BF16.  16-byte lanes when F % 4 == 0 (f32) / F % 8 == 0 (bf16) and both bases and pitches are
 *            16-byte aligned; a guarded per-element path otherwise
 *   status : int32 device word as npi_csr_build_ex's (may be NULL): an id outside [0, n_src) writes a ZERO row and ORs
 *            NPI_STATUS_BAD_ROW_ID into it (torch's index_select raises there); the word is never cleared here
 * One pass, no synchronisation, nothing allocated. */
#define NPI_STATUS_BAD_ROW_ID 8
int npi_rows_gather(const void* x, int64_t ldx, int64_t n_src, const int64_t* idx, int64_t n, int64_t F, void* out, int64_t ldo,
                    int dtype, int32_t* status, void* stream);

/* SAGEConv(normalize=True): y_i = x_i / max(||x_i||_2, eps) -- torch.nn.functional.normalize(out, p=2, dim=-1) at the end of
 * PyG 1.4.2 SAGEConv.update (the reference constructs its layers with the default normalize=False, src/classes.py:48-52; the
 * option is part of the layer's signature).  norm [M] receives ||x_i|| for the backward:
 * dx_i = (dy_i - y_i <dy_i, y_i>) / ||x_i||, and dy_i / eps where the norm was clamped.  One wavefront per row, fixed
 * reduction tree (bitwise reproducible); rows with pitches, 16-byte lanes when aligned. */
int npi_l2_normalize_rows(const float* x, int64_t ldx, int64_t M, int64_t F, float eps, float* y, int64_t ldy, float* norm,
                          void* stream);
int npi_l2_normalize_rows_bwd(const float* dy, int64_t ldd, const float* y, int64_t ldy, const float* norm, int64_t M, int64_t F,
                              float eps, float* dx, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense projection on the matrix cores -- replaces `torch.matmul(aggr_out, self.weight) + bias`
 * (SAGEConv.update / GCNConv.forward) and its autograd backward.  f32 in, f32 out, f32 accumulate on
 * the matrix cores, error at f32-rounding level in both arithmetics (the `flags` of the entry points below).
 *
 *   npi_linear_fwd_ex       : C[M,N]  = act( rowscale_m * (A[M,K] @ W[K,N]) + bias[N] )
 *   npi_linear_bwd_data_ex  : dA[M,K] = rowscale_m * (dC[M,N] @ W[K,N]^T)
 *   npi_linear_bwd_weight_ex: dW[K,N] = A[M,K]^T @ dC[M,N],  db[N] = colsum(dC)   (db may be NULL)
 *                             deterministic split over M; workspace f32
 * GEMM arithmetic of f32 storage: the default (flags 0) is the 3-way bf16 split of both operands on the bf16 matrix cores (six
 * v_mfma_f32_32x32x16_bf16 per product tile, f32 accumulate, error at f32-rounding level; csrc/gemm_f32.hip) -- used by
 * fwd / bwd_data on full 128 x 128 tiles when K % 32 == 0 and rows are 16-byte aligned, and by bwd_weight when K % 128 == 0,
 * N % 128 == 0, M >= 4096 (both operands split on the fly, gemm_dw_split_kernel); everything else (ragged strips, other
 * shapes) and every call with NPI_GEMM_EXACT_F32 runs the exact-f32 kernels (v_mfma_f32_32x32x2_f32).
 * ------------------------------------------------------------------------------------------ */

/* out[N] = column sums of X[M,N] (GCNConv / GATConv bias gradient).  workspace f32: npi_colsum_workspace_elems(M, N)
 * elements for the finest row chunking; ceil(M/2048)*N is the minimum that is accepted (coarser chunks, slower on
 * small M). */
int64_t npi_colsum_workspace_elems(int64_t M, int64_t N);
int npi_colsum(const float* X, int64_t ldx, int64_t M, int64_t N, float* out, float* workspace,
               int64_t workspace_elems, void* stream);
int64_t npi_linear_bwd_weight_workspace_elems(int64_t M, int64_t K, int64_t N);

/* The arithmetic and the grid regime are ARGUMENTS, the scratch for the re-laid weight matrix is a caller workspace -- no
 * process-wide switch exists, nothing is allocated.
 *   flags     : 0 = the default arithmetic (3-way bf16 split for f32 storage); NPI_GEMM_EXACT_F32 forces the exact-f32 kernels
 *               for this call (NPI_GEMM_SPLIT_BF16 names the default explicitly)
 *   workspace : npi_linear_workspace_bytes(K, N) bytes, 16-byte aligned, REQUIRED (NPI_ERR_WORKSPACE otherwise)
 *   shared    : npi_linear_bwd_weight_ex: 1 = the GEMM shares the CUs with an HBM-bound kernel on another stream
 *               (about 3 workgroups per 4 CUs), 0 = it has the GPU to itself (~4 workgroups per CU)
 *
 * NON-FINITE OPERANDS (what replaces torch.matmul at PyG 1.4.2 SAGEConv.update / its autograd):
 *   NPI_GEMM_EXACT_F32  is an fp32 fmaf chain: an Inf operand gives +-Inf in the products it takes part in (NaN against a
 *                       zero or an opposing Inf), exactly like torch.matmul.
 *   NPI_GEMM_SPLIT_BF16 (the default for f32) writes every operand as x0 + x1 + x2 with x1 = bf16(x - x0): for x = +-Inf,
 *                       and for finite |x| > 3.3895e38 (beyond the largest bf16, x0 rounds to Inf), x - x0 is NaN, so every
 *                       output element that operand takes part in is NaN -- the whole output ROW for an element of A / dC,
 *                       the whole output COLUMN for an element of W -- where fp32 matmul gives +-Inf (or, for a finite
 *                       |x| > 3.3895e38 against small weights, a finite number).  NaN operands give
 *                       NaN in both.  Finite results are unaffected (error <= 3 * 2^-24 |a||b| per product).  A model that
 *                       has diverged therefore reads NaN instead of Inf; callers that test `isinf` on activations must
 *                       test `!isfinite`, or pass NPI_GEMM_EXACT_F32.
 *                       Pinned by tests/test_gpu_parity.py::test_non_finite_operands_of_the_projection_gemms. */
#define NPI_GEMM_EXACT_F32 1
#define NPI_GEMM_SPLIT_BF16 2
/* npi_linear_fwd_ex / npi_linear_bwd_weight_ex, f32: A is stored with lda >= Kp (K rounded up to a multiple of 128) and its
 * columns K .. Kp-1 are ZERO (W and dW keep K rows): the matrix-core kernels then run on Kp instead of the guarded kernel on
 * an odd K (178 features in the reference's first layer).  Workspaces are queried with Kp. */
#define NPI_GEMM_A_ZERO_PADDED 4
/* npi_linear_fwd_ex / npi_linear_bwd_data_ex: `workspace` already holds the re-laid copy of THIS weight matrix that the call
 * would otherwise prepare in a launch of its own -- written by npi_linear_prepare (set 0 for fwd, set 1 for bwd_data) from the
 * same W / ldw / K / N / dtype, W unchanged since.  A layer prepares both copies in one launch and runs its forward GEMM,
 * its backward GEMM and any row-block split of them (dist.py: light rows / hub rows) without a preparation launch each.  Not
 * together with NPI_GEMM_A_ZERO_PADDED.  A call whose shape does not take the matrix-core kernels ignores the workspace. */
#define NPI_GEMM_WORKSPACE_PREPARED 8
/* npi_linear_fwd_ex / npi_linear_bwd_data_ex: the persistent matrix-core kernels (one workgroup per CU, a static walk over the
 * tiles) take n workgroups fewer than the chip has CUs (n a multiple of 8, at most 128).  For a GEMM launched while another
 * kernel holds CUs -- a collective's workgroups on a multi-GPU node: a workgroup that finds its CU taken starts late and
 * still owns its share of the tiles, so the launch ends when the other kernel does (measured with a stand-in that holds 16
 * CUs: 0.107 -> 0.15 ms for 125 k rows).  Costs n / 256 more tiles per workgroup when nothing else runs. */
#define NPI_GEMM_RESERVE_CUS(n) ((((n) / 8) & 0xff) << 8)
#define NPI_GEMM_RESERVED_CUS_OF(flags) ((((flags) >> 8) & 0xff) * 8)
/* npi_linear_fwd_ex / npi_linear_bwd_data_ex, f32: the matrix-core kernel runs on TWO fp16 pieces per operand (11 + 11
 * significant bits) and THREE v_mfma_f32_32x32x16_f16 per product tile instead of three bf16 pieces and six products -- half the
 * matrix work for the same f32-rounding-level result (tools/micro/mfma_f16_split.hip: 3.8e-7 of a row's largest |C| against
 * 3.9e-7 for the six bf16 products and 5.5e-7 for an f32 FMA loop; EXPERIMENTS A33 / A34).  fp16 has five exponent bits, so every
 * row of A (dC) is scaled by a power of two that puts its largest magnitude into [2^14, 2^15) -- `a_scales`, [M], written by
 * npi_row_scales -- and every column of the weight operand likewise (inside the preparation); the store epilogue undoes both
 * exactly.  Elements within 2^-28 of their row's maximum keep 22 significant bits, smaller ones an absolute error of 2^-39 of
 * that maximum (the matrix pipe honours fp16 subnormals).  Non-finite operands behave as under NPI_GEMM_SPLIT_BF16.  A workspace
 * handed over with NPI_GEMM_WORKSPACE_PREPARED must have been prepared with `which | NPI_PREPARE_F16X2`.  Shapes that do not take
 * the matrix-core kernel ignore the flag. */
#define NPI_GEMM_SPLIT_F16X2 16
#define NPI_PREPARE_F16X2 4
int64_t npi_linear_workspace_bytes(int64_t K, int64_t N);
/* scales[m] = the power of two s with max_k |A[m, k]| s in [2^14, 2^15), clamped so that s and 1 / s are normal f32 (2^-126 ..
 * 2^126); NaN elements are skipped, and a row with no magnitude -- all zero (or NaN), or one that holds Inf -- gets the clamp
 * maximum 2^126, so that it never lowers the smallest scale of a matrix (npi_col_scales) -- the `a_scales` of the
 * NPI_GEMM_SPLIT_F16X2 calls.  Every launch that writes row scales (npi_segsum_ex, the GATConv fused passes) writes these values.
 * One pass over A. */
int npi_row_scales(const float* A, int64_t lda, int64_t M, int64_t K, float* scales, void* stream);
/* The re-laid copies of W [K, N] (the `weight` of PyG's `torch.matmul(aggr_out, self.weight)`, reference call sites
 * src/classes.py:62,66,70) for the matrix-core kernels, in ONE launch: which = 1: the copy npi_linear_fwd_ex uses, 2: the one
 * npi_linear_bwd_data_ex uses, 3: both, the second npi_linear_workspace_bytes(K, N) bytes behind the first; | NPI_PREPARE_F16X2:
 * the fp16 x 2 planes (and column scales) of NPI_GEMM_SPLIT_F16X2 calls instead of the three bf16 planes.  K and N
 * multiples of 16; workspace 16-byte aligned, npi_linear_workspace_bytes(K, N) bytes per copy. */
int npi_linear_prepare(const void* W, int64_t ldw, int64_t K, int64_t N, int which, int dtype, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* a_col_scales [K] / dc_col_scales [N] (16-byte aligned; NULL without the flag): NPI_GEMM_SPLIT_F16X2 for the weight gradient -- two fp16
 * pieces per operand, three matrix products per tile instead of six.  The contraction runs over the ROWS, so what factors out of
 * the sum is a power-of-two scale per COLUMN of A and of dC: npi_col_scales.  K, N multiples of 128, M >= 4096, f32. */
int npi_linear_bwd_weight_ex(const void* A, int64_t lda, const void* dC, int64_t lddc,
                             void* dW, int64_t lddw, void* db,
                             int64_t M, int64_t K, int64_t N,
                             float* workspace, int64_t workspace_elems, int dtype, int flags, int shared,
                             const float* a_col_scales, const float* dc_col_scales, void* stream);
/* scales[k] = the power of two that puts column k's largest magnitude into [2^14, 2^15) (npi_row_scales' rule: a column with no
 * magnitude gets 2^126).  A != NULL: from the column maxima of A [M, K] (one pass over it: for a matrix that does not change between
 * steps, once).  A == NULL: from `row_scales` [M] (npi_row_scales, or the launch that wrote the matrix): the SMALLEST row scale --
 * the scale of the matrix's largest finite magnitude; 2^126 when every row is zero, 1 when M == 0 -- for every column alike,
 * without a pass over the matrix; elements more than 2^-18 below that magnitude then keep an absolute 2^-39 of it rather than 22
 * relative bits.  workspace: npi_col_scales_workspace_elems(M, K) floats. */
int64_t npi_col_scales_workspace_elems(int64_t M, int64_t K);
int npi_col_scales(const float* A, int64_t lda, int64_t M, int64_t K, const float* row_scales, float* scales,
                   float* workspace, int64_t workspace_elems, void* stream);
/* a_scales / dc_scales: the row scales of the left operand for NPI_GEMM_SPLIT_F16X2 in `flags` (npi_row_scales, or the launch that
 * wrote the operand); NULL / ignored without the flag.  (ABI 4: the scale-taking twins of ABI 3, folded.) */
int npi_linear_fwd_ex(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias,
                       const float* rowscale, void* C, int64_t ldc,
                       int64_t M, int64_t K, int64_t N, int relu, int dtype, int flags,
                       void* workspace, int64_t workspace_bytes, const float* a_scales, void* stream);
int npi_linear_bwd_data_ex(const void* dC, int64_t lddc, const void* W, int64_t ldw,
                            const float* rowscale, void* dA, int64_t ldda,
                            int64_t M, int64_t K, int64_t N, int dtype, int flags,
                            void* workspace, int64_t workspace_bytes, const float* dc_scales, void* stream);

/* The same three GEMMs with A / W / C / bias / dW / db stored as `dtype` (NPI_F32 or NPI_BF16; bf16
 * storage, f32 MFMA accumulation, f32 rowscale and workspace) -- BASELINE.json configs[1]. */
/* C = A W (f32, no bias) and, from the accumulators on their way to C, the row dots sc0[m] = <C[m, :], att[:N]>,
 * sc1[m] = <C[m, :], att[N:]> (att: [2 N]; sc0 / sc1: [M]): GATConv's `x = torch.mm(x, self.weight)` together with the two
 * halves of `(torch.cat([x_i, x_j], dim=-1) * self.att).sum(dim=-1)` per NODE (PyG 1.4.2 gat_conv.py forward / message, one
 * head; not on the reference's own path: BASELINE configs[4]) -- the pass over h that npi_gat_scores makes is gone.  Only
 * shapes where one column tile of the matrix-core kernel covers N: npi_linear_fwd_scores_supported(M, K, N) (M >= 128,
 * K % 32 == 0, N = 128 or 256, default GEMM arithmetic); anything else returns NPI_ERR_ARG (the caller runs npi_linear_fwd_ex
 * + npi_gat_scores).  Operands 16-byte aligned, leading dimensions % 4 == 0; workspace as npi_linear_fwd_ex.  Fixed
 * summation order (bitwise reproducible). */
int npi_linear_fwd_scores_supported(int64_t M, int64_t K, int64_t N);
/* a_scales != NULL: the fp16 x 2 arithmetic (NPI_GEMM_SPLIT_F16X2) with the row scales of A -- npi_row_scales, ONCE for
 * a feature matrix that does not change between steps, or the launch that wrote A (npi_gat_aggregate_fused) */
int npi_linear_fwd_scores(const float* A, int64_t lda, const float* W, int64_t ldw, const float* att, float* C, int64_t ldc,
                              float* sc0, float* sc1, int64_t M, int64_t K, int64_t N, void* workspace, int64_t workspace_bytes,
                              const float* a_scales, void* stream);
/* dA = dC W^T + row0 (x) col0 + row1 (x) col1 (f32; row* are [M], col* [K] vectors): npi_linear_bwd_data_ex with a rank-2 term
 * added in the store epilogue of the matrix-core kernel -- no read-modify-write pass over dA or dC.  GATConv backward
 * (PyG 1.4.2 GATConv.message's `(x_i, x_j) * att` terms, reference call site src/classes.py:48-52 via BASELINE configs[4]): the
 * attention terms g_dst (x) W att_dst + g_src (x) W att_src of dX.  Only shapes the kernel covers completely:
 * npi_linear_bwd_data_rank2_supported(M, K, N) (M >= 128, K % 128 == 0, N % 32 == 0, default GEMM arithmetic); anything else
 * returns NPI_ERR_ARG (the caller adds the terms to dC with npi_gat_rank1_add instead).  Operands 16-byte aligned, leading
 * dimensions % 4 == 0; workspace as npi_linear_bwd_data_ex. */
int npi_linear_bwd_data_rank2_supported(int64_t M, int64_t K, int64_t N);
/* dc_scales != NULL: the fp16 x 2 arithmetic (NPI_GEMM_SPLIT_F16X2) with the row scales of dC, from npi_row_scales
 * or from the launch that wrote dC (npi_gat_backward_fused_heads) */
int npi_linear_bwd_data_rank2(const float* dC, int64_t lddc, const float* W, int64_t ldw, const float* row0,
                                  const float* row1, const float* col0, const float* col1, float* dA, int64_t ldda,
                                  int64_t M, int64_t K, int64_t N, void* workspace, int64_t workspace_bytes,
                                  const float* dc_scales, void* stream);

/* The two-row products around that epilogue, one head (att = [att_dst ; att_src], [2, C]; W [K, C]; P = x^T [g_dst g_src], [2, K] from
 * npi_gat_att_grad on x):  cols: U [2, K] = att W^T, the column vectors col0 / col1 above.  tail: dW [K, C] += P^T att (the
 * outer-product correction of the weight gradient; null: skipped) and datt [2, C] = P W (null: skipped).  Fixed summation
 * orders.  (GATConv.message's att terms, PyG 1.4.2 gat_conv.py; not on the reference's own path: BASELINE configs[4].) */
int npi_gat_rank2_cols(const float* W, int64_t ldw, const float* att, int64_t K, int64_t C, float* U, void* stream);
int npi_gat_rank2_tail(const float* P, const float* W, int64_t ldw, const float* att, int64_t K, int64_t C, float* dw, int64_t lddw,
                       float* datt, void* stream);

/* ------------------------------------------------------------------------------------------
 * One conv LAYER CALL as one entry point -- replaces `SAGEConv.forward` as the reference calls it (`self.convK(x, edge_index)`,
 * src/classes.py:62,66,70) and its autograd backward (src/train_with_twoDataset.PY:54); also GCNConv evaluated as (A_hat x) W + b.
 * They issue, in order on `stream`, exactly the launches of the per-op entry points above and add no kernel of their own; what
 * they save is the HOST's cost of eight separate calls per layer and direction, which bounds the step at the reference's real
 * sizes (batches of 200 enclosing subgraphs, the bundled full graphs).  Large graphs keep the per-op calls (their backward is
 * arranged on two streams by the caller).  Every buffer is the caller's, as everywhere.
 *
 *   npi_conv_fwd : agg[:, :F] = segsum(CSR by target, x)  (mean / per-entry weights w_entry as npi_segsum_ex; columns F .. of a
 *                  wider agg must be ZERO: NPI_GEMM_A_ZERO_PADDED in gemm_flags);  out = act(agg @ W[K, Nout] + bias).
 *                  prepare_which: 0 = the GEMM lays W out itself (ws: npi_linear_workspace_bytes(K rounded up to 128 if padded,
 *                  Nout)), 1 = npi_linear_prepare of the forward copy first, 3 = both copies (ws: two of them; the second one is
 *                  what npi_conv_bwd takes as ws_bwd with ws_prepared = 1).
 *   npi_conv_bwd : g = out_relu ? dout masked by out_relu > 0 (into dz; f32) : dout;
 *                  dW != NULL: dW[K, Nout] = agg^T g, db = colsum(g) (db may be NULL; dw_ws: npi_linear_bwd_weight_workspace_elems);
 *                  dx != NULL: dagg = rowscale * (g @ W^T), dx = segsum(transposed CSR t_*, dagg) (sum; weights t_w or NULL).
 * ------------------------------------------------------------------------------------------ */
int npi_conv_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* item_row, int64_t item_edges,
                 const float* w_entry, int64_t N, int64_t nnz_max, const void* x, int64_t ldx, int64_t F, int mean,
                 void* agg, int64_t ldagg, float* carry, const void* W, int64_t ldw, const void* bias, void* out,
                 int64_t ldo, int64_t K, int64_t Nout, int relu, int dtype, int gemm_flags, int prepare_which,
                 void* ws, int64_t ws_bytes, void* stream);
int npi_conv_bwd(const void* dout, int64_t lddo, const float* out_relu, int64_t ldor, float* dz, int64_t lddz, int64_t N,
                 int64_t K, int64_t Nout, int dtype, int gemm_flags, const void* agg, int64_t ldagg, void* dW, int64_t lddw,
                 void* db, float* dw_ws, int64_t dw_ws_elems, const void* W, int64_t ldw, const float* rowscale,
                 void* dagg, int64_t lddagg, void* ws_bwd, int64_t ws_bwd_bytes, int ws_prepared,
                 const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_item_row, int64_t t_item_edges,
                 const float* t_w, int64_t t_nnz_max, void* dx, int64_t lddx, float* t_carry, void* stream);

/* ------------------------------------------------------------------------------------------
 * GATConv (PyG 1.4.2; absent from the reference tree, BASELINE.json configs[4]).  H heads of C
 * channels, hfeat = x @ W is [N, H*C]; att is [H, 2C] (first C multiply the TARGET's features).
 * The attention coefficient alpha of an entry is recomputed from four per-node, per-head scalars
 * [N, H] -- a_dst, a_src (npi_gat_scores), m, s (npi_gat_softmax_stats_ex):
 *     alpha(i <- j) = exp(leaky_relu(a_dst[i] + a_src[j]) - m[i]) / (s[i] + 1e-16)
 * The backward may keep the alpha that npi_gat_edge_grad computes anyway (alpha_out [nnz_max, H], by-target
 * entry order) and hand it to the by-source npi_gat_aggregate (alpha + alpha_map = npi_entry_transpose_map;
 * one head): reading a weight back is cheaper there than the exp and the divide per entry.  Both NULL: recompute.
 *
 *   npi_gat_scores        `(cat[x_i, x_j] * att).sum(-1)` split into its two dot products
 *   npi_gat_softmax_stats_ex `utils.softmax`: scatter_max + scatter_add(exp) per target row
 *   npi_gat_aggregate     by_source == 0: out[i] = sum_p alpha_p hfeat[col p] (+ bias)          (forward)
 *                         by_source != 0: out[j] = sum_q alpha_q x[col q] + g_dst[j] att[:C] + g_src[j] att[C:]
 *                                         over the by-source CSR                                (backward, d hfeat)
 *   npi_gat_rowdot        D[i,h] = <a[i,h,:], b[i,h,:] - bias[h,:]>      (= sum_p alpha_p dalpha_p)
 *   npi_gat_edge_grad     dz[p,h] = alpha_p (<dout_i, hfeat_j> - D_i) * leaky_relu'(z_p), by-target entry order
 *   npi_seg_rowsum_ex     out[r,h] = sum_{p in row r} vals[map ? map[p] : p, h]
 *   npi_entry_transpose_map  map[q] = by-target position of by-source entry q
 *   npi_gat_att_grad      datt[h,:C] = sum_i g_dst[i,h] hfeat[i,h,:],  datt[h,C:] likewise with g_src
 * ------------------------------------------------------------------------------------------ */
int npi_gat_scores(const float* hfeat, int64_t ldh, const float* att, int64_t N, int64_t H, int64_t C,
                   float* a_dst, float* a_src, void* stream);
/* npi_gat_aggregate over a two-part table (x2 / split as in npi_segsum_ex). */
int npi_gat_aggregate_ex(const int32_t* rowptr, const int32_t* col, const int32_t* item_row, int64_t item_edges,
                         int64_t N, int64_t nnz_max, const float* x, int64_t ldx, const float* x2, int64_t split,
                         float* out, int64_t ldo,
                         int64_t H, int64_t C, const float* a_dst, const float* a_src, const float* m,
                         const float* s, float negative_slope, int by_source, const float* bias,
                         const float* g_dst, const float* g_src, const float* att,
                         const float* alpha, const int32_t* alpha_map,
                         float* carry, void* stream);
/* Fused backward pass over the by-SOURCE CSR, H in {1, 2, 4, 8} heads (H > 1: C in {32, 64, 128}), H C <= 256 -- in ONE pass over
 * the gathered dOut rows
 *     out[j, :]  = sum_q alpha_q dout[col q, :]                                   (the aggregation half of d hfeat)
 *     dz[q, h]   = alpha_q (<dout[col q], hfeat[j]> - D[col q]) leaky_relu'(a_dst[col q] + a_src[j])   (the SDDMM)
 * replaces npi_gat_edge_grad + the by-source npi_gat_aggregate: one gather pass over the entries instead of two.  The four
 * per-TARGET scalars the pass needs -- a_dst, m, 1 / (s + 1e-16), D -- are packed into one float4 per node and head
 * (npi_gat_pack_targets over the N H flattened scalars; tpack [n_cols, H, 4], 16 MB at N = 1M: cache resident): every entry
 * makes ONE 16-byte gather per head and alpha is recomputed by the lane that owns the entry (one exp per entry and head).
 * a_src [n_rows, H], dz [nnz_max, H]; every entry's H dots are reduced inside the C / 4 lanes of their head.  dout2 / split: the
 * gathered rows come from a two-part table as in npi_segsum_ex (tpack is ONE array indexed by the column id over both parts:
 * the sharded GATConv's received hub rows + the rank's own rows).  The attention terms g_dst att[:C] + g_src att[C:] of d hfeat
 * are added afterwards by npi_gat_rank1_add, or never formed (npi_linear_bwd_data_rank2); g_dst / g_src are row sums of dz
 * (npi_seg_rowsum_ex over both orientations). */
int npi_gat_pack_targets(const float* a_dst, const float* m, const float* s, const float* D, int64_t N, float* tpack,
                         void* stream);
/* row_scales_out != NULL ([N]; heads * out_channels == 256): the launch also writes the power-of-two scale of every finished row of `out`:
 * the dc_scales of the projection behind it (npi_linear_bwd_data_rank2 / npi_linear_bwd_data_ex) without a pass over `out`.
 * g_src_out != NULL ([N]; one head): the launch also leaves the row sums of dz -- what npi_seg_rowsum_ex(vals = dz) over this CSR would
 * return -- taken by the lanes that compute dz; workspace: npi_seg_scan_workspace_elems(nnz_max, 1) floats (rows cut by an item
 * boundary are added up by a small launch behind the pass).  NULL: workspace is not used. */
int npi_gat_backward_fused_heads(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx,
                                     const int32_t* item_row, int64_t item_edges, int64_t N, int64_t nnz_max,
                                     const float* dout, int64_t ldd, const float* dout2, int64_t split, const float* hfeat,
                                     int64_t ldh, float* out, int64_t ldo, int64_t H, int64_t C, const float* tpack,
                                     const float* a_src, float slope, float* dz, float* carry, float* row_scales_out,
                                     float* g_src_out, float* workspace, int64_t workspace_elems, void* stream);
int npi_gat_rank1_add(float* dh, int64_t ld, const float* g_dst, const float* g_src, const float* att,
                      int64_t N, int64_t H, int64_t C, void* stream);
int npi_gat_rowdot(const float* a, int64_t lda, const float* b, int64_t ldb, const float* bias,
                   int64_t N, int64_t H, int64_t C, float* D, void* stream);
/* npi_gat_edge_grad with a two-part gathered table (hfeat2 / split) and, swap != 0, the roles of rows and columns
 * exchanged -- the same dz seen from a by-SOURCE CSR: rows are source nodes (`dout` = their hfeat rows, a_src indexed
 * by row), columns are target nodes (`hfeat` = the gathered dOut rows; a_dst, m, s, D indexed by column).  The sharded
 * GAT backward uses it to sum dz by source without a transpose map between different ranks' entry sets. */
int npi_gat_edge_grad_ex(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx,
                         int64_t N, int64_t nnz_max, const float* hfeat, int64_t ldh,
                         const float* hfeat2, int64_t split,
                         const float* dout, int64_t ldd, int64_t H, int64_t C,
                         const float* a_dst, const float* a_src, const float* m, const float* s,
                         const float* D, float negative_slope, int swap, float* dz, float* alpha_out, void* stream);
/* Per-row reductions of per-ENTRY scalars (npi_gnn_amd/csrc/segscan.hip): the entries are streamed -- a wavefront per 64 / 256
 * consecutive entries, a segmented scan keyed by the CSR's rowidx, cut rows folded by a second launch in a fixed order
 * (deterministic, no atomics).  These calls keep no item state: they take no item_row and chunk the stream per call.
 *   npi_seg_rowsum_ex        out[r, h] = sum over the entries p of row r of vals[map ? map[p] : p, h]; rows without an entry: 0
 *   npi_gat_softmax_stats_ex (m, s)[r, h] = (max, sum exp(. - max)) of e_p = leaky_relu(a_row[r] + a_col[col p]) over row r (an empty
 *                              row: m = 0, s = 0); additionally writes e_p of every entry to scores [nnz_max, H] (may be NULL),
 *                              which npi_gat_aggregate_scores reads back
 *   npi_gat_aggregate_scores = npi_gat_aggregate_ex(by_source = 0), one head, with the per-entry scores of the statistics
 *                              pass instead of two gathered per-node scalars per entry;
 *                              relu != 0: max(., 0) in the row epilogue (the F.relu behind the layer)
 *   npi_gat_rowdot_colsum    = npi_gat_rowdot AND the column sums of `a` (GATConv's bias gradient; colsum may be NULL) in
 *                              one pass over a and b; needs 16-byte aligned rows, C % 4 == 0, H C <= 1024
 * workspace: npi_seg_scan_workspace_elems(nnz_max, H) / npi_gat_rowdot_colsum_workspace_elems(N, H, C) floats. */
int64_t npi_seg_scan_workspace_elems(int64_t nnz_max, int64_t H);
int npi_seg_rowsum_ex(const int32_t* rowptr, const int32_t* rowidx, const float* vals, const int32_t* map,
                      int64_t N, int64_t nnz_max, int64_t H, float* out, float* workspace, int64_t workspace_elems,
                      void* stream);
int npi_gat_softmax_stats_ex(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const float* a_row,
                             const float* a_col, int64_t N, int64_t nnz_max, int64_t H, float negative_slope, float* m,
                             float* s, float* scores, float* workspace, int64_t workspace_elems, void* stream);
int npi_gat_aggregate_scores(const int32_t* rowptr, const int32_t* col, const int32_t* item_row, int64_t item_edges,
                             int64_t N, int64_t nnz_max, const float* x, int64_t ldx, const float* x2, int64_t split,
                             float* out, int64_t ldo, int64_t C, const float* scores, const float* m, const float* s,
                             const float* bias, int relu, float* carry, void* stream);
/* The same forward aggregation WITHOUT the statistics pass in front of it (one head of at most 256 channels): an online softmax
 * inside the launch.  The score of an entry is e_p = leaky_relu(a_dst[row] + <x[col p], att[C:]>) -- the source's half recomputed
 * from the row that is gathered anyway (att: the layer's [2 C] attention vector, PyG layout: target half first), so no per-entry
 * score array and no 4-byte gather per entry exist; the open row keeps (max so far, sum of exp(e - max)) and rescales its
 * accumulators when the maximum moves; the parts of a row cut by an item boundary carry their (max, sum) and are merged with
 * exp(m_part - m_row) where cut rows are resolved, in a fixed order (bitwise reproducible).  Writes m[N], s[N] -- the row
 * maximum and the row sum of exp(e - m) that npi_gat_pack_targets / the backward need -- beside out.  (rowidx: unused, may be
 * NULL.)  The scores differ from npi_gat_scores' by the rounding of another summation order (1e-6 relative). */
/* row_scales_out != NULL ([N]; 256 channels): the launch also writes the power-of-two scale of every finished row of `out` -- bias and
 * ReLU applied, as stored --: the a_scales of the NEXT layer's projection (npi_linear_fwd_scores / npi_linear_fwd_ex) */
int npi_gat_aggregate_fused(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* item_row,
                                int64_t item_edges, int64_t N, int64_t nnz_max, const float* x, int64_t ldx, const float* x2,
                                int64_t split, float* out, int64_t ldo, int64_t C, const float* a_dst, const float* att,
                                float negative_slope, const float* bias, int relu, float* m, float* s, float* carry,
                                float* row_scales_out, void* stream);
/* The same launch for H = 2, 4 or 8 heads of C = 32, 64 or 128 channels with H C <= 256 (the shapes npi_gat_backward_fused_heads
 * serves): x / out rows are H C wide, a_dst, m, s are [N, H], att is the layer's [H, 2 C].  A head is a group of C / 4 lanes: the
 * score's dot is summed inside the group in one fixed order, every lane keeps the online softmax of its own head, and the parts of a
 * cut row carry (max, sum) per head.  x, x2, out and att must be 16-byte aligned (bias need not be), ldx and ldo multiples of 4.  H == 1 forwards
 * to npi_gat_aggregate_fused; row_scales_out must be NULL unless H == 1.  Any other shape returns NPI_ERR_ARG before a launch. */
int npi_gat_aggregate_fused_heads(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* item_row,
                                  int64_t item_edges, int64_t N, int64_t nnz_max, const float* x, int64_t ldx, const float* x2,
                                  int64_t split, float* out, int64_t ldo, int64_t H, int64_t C, const float* a_dst,
                                  const float* att, float negative_slope, const float* bias, int relu, float* m, float* s,
                                  float* carry, float* row_scales_out, void* stream);
int64_t npi_gat_rowdot_colsum_workspace_elems(int64_t N, int64_t H, int64_t C);
/* `F.relu(conv(x))` fused (npi_gat_aggregate_scores with relu != 0 applies the ReLU in the row epilogue): b is then the ReLU
 * OUTPUT, and this form first masks the incoming gradient, a' = a where b > 0 else 0 (threshold_backward), uses a' for D and
 * the column sums and writes it to a_masked [N, ldm] -- the gradient of the pre-activation the rest of the backward consumes.
 * D is unchanged by the fusion: where b > 0 the pre-activation equals b, elsewhere a' = 0. */
int npi_gat_rowdot_colsum_relu(const float* a, int64_t lda, const float* b, int64_t ldb, const float* bias,
                               int64_t N, int64_t H, int64_t C, float* D, float* colsum, float* a_masked, int64_t ldm,
                               float* workspace, int64_t workspace_elems, void* stream);
int npi_entry_transpose_map(const int32_t* src_eid, const int32_t* src_rowidx, const int32_t* src_rowptr,
                            const int32_t* dst_rowptr, const int32_t* pos_dst_of_edge, int64_t N,
                            int64_t nnz_max, int32_t* map, void* stream);
int64_t npi_gat_att_grad_workspace_elems(int64_t N, int64_t H, int64_t C);
int npi_gat_att_grad(const float* hfeat, int64_t ldh, const float* g_dst, const float* g_src,
                     int64_t N, int64_t H, int64_t C, float* datt, float* workspace,
                     int64_t workspace_elems, void* stream);

/* ------------------------------------------------------------------------------------------
 * GATConv with ATTENTION DROPOUT inside the fused launches (PyG 1.4.2 GATConv.message: alpha = F.dropout(softmax(alpha), p)).
 * The launches recompute alpha per entry in both orientations; they recompute the dropout decision the same way, as a pure
 * function of (key, edge, head) keyed on the entry's eid, which the by-target and the by-source CSR both carry -- no [nnz, H]
 * mask, no alpha array, and a step is reproducible from (seed, draw).
 *
 * Rule D (the mask; the counter-based generator of the other rules, npi_gnn_amd/csrc/draw.h; wrapping uint64 throughout):
 *     key    = epoch_seed(seed, draw)                       as every other rule (npi_sample_select's description)
 *     root   = mix64(mix64(key) + 6 G)                      draw_root(key, DRAW_RULE_D), G = 0x9E3779B97F4A7C15
 *     k      = eid                    an entry that is column eid of edge_index (0 <= eid < 2^31)
 *            = 2^32 + i               the self loop the CSR build appends at node i (eid < 0; rowidx == col == i on both sides)
 *     word_h = mix64(mix64(root ^ (k C)) + G (h + 1))       draw_word(draw_stream(root, k), h + 1), C = 0xD6E8FEB86659FD93, h = 0 .. H-1
 *     T      = floor(p 2^64)          p taken as the double it is; exact integers on the host: int(Fraction(p) * 2**64)
 *     dropped(k, h)  <=>  word_h < T ;   kappa(k, h) = 0 if dropped else float32(1 / (1 - p))
 * The calls take key (int64), T = `threshold` and kappa's kept value `scale` (float), never p: the host alone rounds.  T is an
 * unsigned 64-bit number; like `key` it travels as the int64_t with the same 64 bits (T - 2^64 from 2^63 on).
 * In numpy (uint64 arrays wrap):
 *     def mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *     root = mix64(mix64(uint64(key)) + 6 * G);  k = where(eid >= 0, eid, 2**32 + col).astype(uint64)
 *     keep[:, h] = where(mix64(mix64(root ^ (k * C)) + G * (h + 1)) < T, 0, float32(1 / (1 - p)))
 * Known answers (seed 0, draw 0): root = 0x6f163edb947c9e05, T(0.6) = 11068046444225730560; k = 0: words 0x16487dc5ae5a7950,
 * 0x36d77e7754a4d63d (heads 0, 1: both dropped at p = 0.6); k = 1: 0xedeff920902a8ec7, 0xb36d8fb43721e4f1 (both kept).
 *
 * The arithmetic of the layer changes in three places (m, s stay the statistics of the UNDROPPED scores, D_i = <dOut_i, out_i - b>
 * is the unchanged npi_gat_rowdot_colsum_relu):
 *     out_i = sum_p alpha_p kappa_p h_j + b;   dz_p = alpha_p (kappa_p <dOut_i, h_j> - D_i) leaky_relu'(z_p);
 *     dh_j  = sum_i alpha_ij kappa_ij dOut_i  (+ the rank-1 terms from dz)
 * Every call below is its sibling -- same arguments, same contract, the same NPI_ERR_ARG refusals before any launch -- followed by
 *     eid [nnz_max]: the eid array of the CSR side that is walked (NULL: NPI_ERR_ARG), key, threshold, scale.
 * Dropped entries are still gathered.  npi_gat_dropout_keep writes kappa itself, keep [nnz_max, H] f32 in the side's entry order
 * (0 behind the last entry): the same mask for a layer composed from the per-op calls, and for tests.
 * ------------------------------------------------------------------------------------------ */
int npi_gat_aggregate_fused_heads_dropout(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx, const int32_t* item_row,
                                          int64_t item_edges, int64_t N, int64_t nnz_max, const float* x, int64_t ldx, const float* x2,
                                          int64_t split, float* out, int64_t ldo, int64_t H, int64_t C, const float* a_dst,
                                          const float* att, float negative_slope, const float* bias, int relu, float* m, float* s,
                                          float* carry, float* row_scales_out, void* stream,
                                          const int32_t* eid, int64_t key, int64_t threshold, float scale);
int npi_gat_backward_fused_heads_dropout(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx,
                                         const int32_t* item_row, int64_t item_edges, int64_t N, int64_t nnz_max,
                                         const float* dout, int64_t ldd, const float* dout2, int64_t split, const float* hfeat,
                                         int64_t ldh, float* out, int64_t ldo, int64_t H, int64_t C, const float* tpack,
                                         const float* a_src, float slope, float* dz, float* carry, float* row_scales_out,
                                         float* g_src_out, float* workspace, int64_t workspace_elems, void* stream,
                                         const int32_t* eid, int64_t key, int64_t threshold, float scale);
int npi_gat_edge_grad_dropout(const int32_t* rowptr, const int32_t* col, const int32_t* rowidx,
                              int64_t N, int64_t nnz_max, const float* hfeat, int64_t ldh,
                              const float* hfeat2, int64_t split,
                              const float* dout, int64_t ldd, int64_t H, int64_t C,
                              const float* a_dst, const float* a_src, const float* m, const float* s,
                              const float* D, float negative_slope, int swap, float* dz, float* alpha_out, void* stream,
                              const int32_t* eid, int64_t key, int64_t threshold, float scale);
int npi_gat_dropout_keep(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t N, int64_t nnz_max, int64_t H,
                         int64_t key, int64_t threshold, float scale, float* keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * DropEdge (PyG 1.4.2 torch_geometric.utils.dropout_adj): seeded edge dropout as a SORT-FREE filter of both CSR sides.  A side is
 * ordered by (row, list order) and dropping entries keeps that order, so the dropped graph's sides are a stream compaction of the
 * parent's -- no radix sort, no renumbering of the columns, nothing read back, and a step is reproducible from (seed, draw, tick).
 *
 * Rule E (the generator of the other rules, npi_gnn_amd/csrc/draw.h; wrapping uint64 throughout):
 *     key    = epoch_seed(seed, draw)                       as every other rule
 *     root   = mix64(mix64(key) + 8 G)                      draw_root(key, DRAW_RULE_E)
 *     root_t = mix64(root + G (tick + 1))                   tick: an optional DEVICE int64 word, 0 when none is given (as Rule N)
 *     directed:    k = e, the column of edge_index (0 <= e < n_edges);     word = mix64(mix64(root_t ^ (k C)) + G)
 *     undirected:  k = 2^32 min(u, v) + max(u, v), (u, v) the column's ends; word = mix64(mix64(root_t ^ (k C)) + 2 G)
 *                  (min / max of the int64 ends, then wrapping uint64: (u, v), (v, u) and every parallel duplicate share a word)
 *     T      = floor(p 2^64)          exact integers on the host, as Rule D: int(Fraction(p) * 2**64); 0 <= p < 1
 *     column dropped  <=>  word < T
 * The calls take key and T = `threshold` (the int64_t with the same 64 bits), never p.  T = 0 drops nothing.
 * On a CSR side an entry is subject to the rule iff 0 <= eid < n_edges: directed, its slot is its eid; undirected, its slot comes
 * from (rowidx[p], col[p]), the same pair on both sides.  Every other entry is kept: the self loop the build appends (eid < 0) and
 * the root entries of a combined side (eid >= n_edges).  Kept entries keep their order AND the parent's column number in eid, so an
 * [E]-long edge_weight still lines up, npi_segmax's arg still names parent columns and Rule D's mask of an edge is unchanged.
 * In numpy (uint64 arrays wrap):
 *     root_t = mix64(mix64(mix64(uint64(key)) + 8 * G) + G * (tick + 1))
 *     k = arange(E) if directed else (minimum(u, v).astype(uint64) << 32) + maximum(u, v).astype(uint64)
 *     keep = mix64(mix64(root_t ^ (k * C)) + G * (1 if directed else 2)) >= T
 * Known answers (seed 0, draw 0): key = 0xe220a8397b1dcdaf, root = 0x3500c0e53fa8015b, root_t = 0x6ca685ee2acaed88 (tick 0),
 * 0x7eeb741d67e7ca58 (tick 1); tick 0, directed, slots 0, 1: 0x7f2790ca6cae07ac, 0x4836408e21e38141; undirected, slots 0, 1 (the
 * pairs (0, 0), (0, 1)): 0xa7db0d37986c2656, 0x37f4d516f27ca8a6.  T(0.5) = 2^63, T(0.3) = 5534023222112865280,
 * T(1 - 2^-53) = 18446744073709549568.
 *
 *   npi_csr_drop_side : the side (rowptr [N + 1], col / eid / rowidx [nnz_max], nnz = rowptr[N] read on the device; entries at or
 *       behind nnz are never touched or counted) with the dropped entries removed: rowptr_o [N + 1] (rowptr_o[N] = the number
 *       kept), col_o / eid_o / rowidx_o [nnz_max_out] compacted, item_row_o cut for capacity nnz_max_out and item_edges (64 or
 *       NPI_ITEM_EDGES).  nnz_max_out >= nnz_max is required and always enough, so nothing is read back.  Parallel over entries
 *       (one wavefront per 256): a hub row costs what its entries cost.  The outputs must not be the inputs.
 *   npi_drop_edge_list : the rule over the COLUMNS of an edge list (src, dst int64 [E]); every column takes part, (i, i) and
 *       (-1, -1) columns included.  The kept columns compacted in input order into out_src / out_dst [E]; newpos [E] (or NULL):
 *       the new position of column e, -1 if dropped; count: the number kept (int32 device word).  pad_tail != 0: the columns behind
 *       the kept ones are (-1, -1), the padding npi_filter_adj writes and npi_csr_build_ex drops.  Not in place.
 *   npi_drop_edge_keep : keep [E] uint8, 1 = kept: the decision itself, for tests and composed variants (src / dst may be NULL
 *       in directed mode).
 *   npi_drop_edges_workspace_elems(n) : int32 words of `workspace` for the two compactions over n entries / columns (-1: bad n).
 * flags: NPI_DROP_UNDIRECTED.  NPI_ERR_ARG before anything is launched: a null pointer, a bad size or item size, an unknown flag,
 * nnz_max_out < nnz_max, a workspace that is NULL, not aligned to 4 bytes or shorter than the query says.
 * ------------------------------------------------------------------------------------------ */
#define NPI_DROP_UNDIRECTED 1
int64_t npi_drop_edges_workspace_elems(int64_t n);
int npi_csr_drop_side(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t N,
                      int64_t nnz_max, int64_t n_edges, int64_t key, const int64_t* tick /* device word, or NULL */,
                      int64_t threshold, int flags, int64_t nnz_max_out, int64_t item_edges, int32_t* rowptr_o, int32_t* col_o,
                      int32_t* eid_o, int32_t* rowidx_o, int32_t* item_row_o, int32_t* workspace, int64_t workspace_elems,
                      void* stream);
int npi_drop_edge_list(const int64_t* src, const int64_t* dst, int64_t E, int64_t key, const int64_t* tick, int64_t threshold,
                       int flags, int64_t* out_src, int64_t* out_dst, int32_t* newpos, int32_t* count, int pad_tail,
                       int32_t* workspace, int64_t workspace_elems, void* stream);
int npi_drop_edge_keep(const int64_t* src, const int64_t* dst, int64_t E, int64_t key, const int64_t* tick, int64_t threshold,
                       int flags, uint8_t* keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * Between-layer steps of Net_1 (reference src/classes.py:63-64,67-68,71-72),
 * forward only: PyG 1.4.2 TopKPooling(ratio) and the [global_max_pool || global_mean_pool] readout.
 * `batch` is the PyG Batch vector (int64, non-decreasing); graph_ptr[B+1] its segment starts.
 *   npi_topk_score      score_i = tanh(<x_i, w> / ||w||)
 *   npi_graph_bounds    graph_ptr from batch
 *   npi_topk_select     per graph keep ceil(ratio n_g) best (score desc, index asc): out_ptr[B+1],
 *                       perm[out_ptr[B]], remap[N] (new id or -1); status bit 1 = a graph > 16384 nodes
 *   npi_topk_gather     x' = x[perm] * score[perm], batch' = batch[perm], score' = score[perm]
 *   npi_filter_adj      surviving edges, relabelled, original order; count[0] on device
 *   npi_readout_max_mean  out[g] = [max_i x_i || mean_i x_i]  ([B, 2F])
 * ------------------------------------------------------------------------------------------ */
int npi_topk_score(const float* x, int64_t ldx, const float* w, int64_t N, int64_t F, float* score, void* stream);
int npi_graph_bounds(const int64_t* batch, int64_t N, int64_t B, int32_t* graph_ptr, void* stream);
/* max_nodes: an upper bound of the largest graph of the batch, when the caller knows one (0 = unknown) */
int npi_topk_select(const float* score, const int32_t* graph_ptr, int64_t N, int64_t B, float ratio,
                    int32_t* out_ptr, int32_t* perm, int32_t* remap, int32_t* status, int64_t max_nodes, void* stream);
/* The same selection for graphs of ANY size (npi_topk_select sorts a graph's scores in LDS: at most 16,384 nodes per graph,
 * bit 1 of its status word otherwise): two stable radix sorts of the whole batch on the device -- by score, descending, ties
 * by the lower node index; then by graph id -- and one pass that keeps the first ceil(ratio n_g) nodes of every graph.
 * Same outputs (out_ptr [B+1], perm in graph-major, score-descending order, remap), no device read; `batch` is the PyG batch
 * vector (int64, non-decreasing).  workspace: npi_topk_sorted_workspace_bytes(N) bytes. */
int64_t npi_topk_sorted_workspace_bytes(int64_t N);
int npi_topk_select_sorted(const float* score, const int64_t* batch, const int32_t* graph_ptr, int64_t N, int64_t B,
                           float ratio, int32_t* out_ptr, int32_t* perm, int32_t* remap, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* perm64 (may be NULL) receives perm as int64 -- the LongTensor TopKPooling returns -- without a cast launch */
int npi_topk_gather(const float* x, int64_t ldx, const float* score, const int64_t* batch,
                    const int32_t* perm, const int32_t* out_ptr, int64_t B, int64_t F, int64_t n_out_max,
                    float* xo, int64_t ldo, int64_t* batch_o, float* score_o, int64_t* perm64, void* stream);
/* int32 workspace of npi_filter_adj: one count per tile of 2,048 edges, two spare words, then E words that receive the
 * new position of every input edge (-1: dropped) -- npi_filter_adj_newpos_offset(E) is where those start */
int64_t npi_filter_adj_workspace_elems(int64_t E);
/* pad_tail != 0: the output kept at the INPUT's length -- fills out_src / out_dst[count .. E) with -1.
 * A (-1, -1) column is padding everywhere downstream -- npi_csr_build_ex drops it without raising the out-of-range flag,
 * npi_filter_adj skips it -- so a caller that knows the node counts (TopKPooling keeps ceil(ratio n_g) per graph) never
 * has to read the surviving-edge count back and the whole Net_1 step runs without a host synchronisation (and captures
 * into a HIP graph).  Negative ids in src / dst are always treated as dropped.  Output arrays must not alias the input. */
int npi_filter_adj(const int64_t* src, const int64_t* dst, int64_t E, const int32_t* remap,
                      int64_t* out_src, int64_t* out_dst, int32_t* count, int32_t* workspace, int pad_tail, void* stream);
int64_t npi_filter_adj_newpos_offset(int64_t E);   /* npi_filter_adj: workspace[offset + e] = new position of input edge e, -1 if dropped */
/* The by-target CSR of the POOLED graph from the CSR of its parent, without a sort: row perm[r'] of the parent with the
 * entries whose source survived (remap[col] >= 0), in the parent's order, self loop last; eid through newpos
 * (npi_filter_adj's workspace tail).  Bit-identical to npi_csr_build_ex on the filtered edge list.  nnz_max_out = capacity
 * of col_o / eid_o / rowidx_o (>= the surviving entries; E_in + n_out is what a fresh build would use); item_edges: the item
 * size of the NEW CSR (independent of the parent's); workspace int32 [npi_csr_filter_workspace_elems(n_out)];
 * n_out <= npi_csr_filter_max_rows(). */
int64_t npi_csr_filter_max_rows(void);
int64_t npi_csr_filter_workspace_elems(int64_t n_out);
int npi_csr_filter(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* perm, const int32_t* remap,
                   const int32_t* newpos, int64_t n_out, int64_t nnz_max_out, int32_t* rowptr_o, int32_t* col_o,
                   int32_t* eid_o, int32_t* rowidx_o, int32_t* item_row_o, int64_t item_edges, int32_t* status_o, int32_t* workspace,
                   void* stream);
int npi_readout_max_mean(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t B, int64_t F,
                         float* out, void* stream);

/* Backward of the pooling layer (autograd of reference src/classes.py:63-72 in the train loop,
 * src/train_with_twoDataset.PY:52-54).  x is the layer INPUT, perm/score the forward's results.
 *   npi_topk_gather_bwd : per kept row i = perm[p]:  ds = <dxo[p], x[i]> (+ dscore_o[p], may be NULL),
 *                         dz = ds (1 - score_i^2),  dx[i] = dxo[p] score_i + dz w / ||w||;  dx must be
 *                         zero-filled by the caller (dropped rows get no gradient);  dzv[p] = dz,
 *                         dzz[p] = dz * (x_i . w / ||w||) feed the weight gradient.
 *   npi_topk_weight_grad: dw[f] = sum_p dzv[p] x[perm[p], f] / ||w|| - w[f] sum_p dzz[p] / ||w||^2
 *                         (deterministic two-level sum; workspace f32).
 *   npi_readout_max_mean_bwd: dx[i, c] = dout[g, F + c] / n_g + (i = first arg-max row of column c in graph g
 *                         ? dout[g, c] : 0); `out` is the forward's [B, 2F] result. */
int npi_topk_gather_bwd(const float* x, int64_t ldx, const float* score, const float* w, const int32_t* perm,
                        int64_t n_out, int64_t F, const float* dxo, int64_t lddxo, const float* dscore_o,
                        float* dx, int64_t lddx, float* dzv, float* dzz, void* stream);
/* The forms the training step uses: no fill launch in front of them.
 *   npi_topk_gather_bwd_ex     : one wave per INPUT row i of the N; remap[i] = its kept position p or -1 (npi_topk_select);
 *                                dropped rows are written as zeros, so dx may come in uninitialised.
 *   npi_readout_max_mean_bwd_ex: N = rows of x; rows outside [graph_ptr[0], graph_ptr[B]) are written as zeros. */
int npi_topk_gather_bwd_ex(const float* x, int64_t ldx, const float* score, const float* w, const int32_t* remap,
                           int64_t N, int64_t F, const float* dxo, int64_t lddxo, const float* dscore_o,
                           float* dx, int64_t lddx, float* dzv, float* dzz, void* stream);
int npi_readout_max_mean_bwd_ex(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t B, int64_t F,
                                const float* out, const float* dout, float* dx, int64_t lddx, int64_t N, void* stream);
int64_t npi_topk_weight_grad_workspace_elems(int64_t n_out, int64_t F);
int npi_topk_weight_grad(const float* x, int64_t ldx, const int32_t* perm, const float* dzv, const float* dzz,
                         int64_t n_out, int64_t F, const float* w, float* dw, float* workspace,
                         int64_t workspace_elems, void* stream);
int npi_readout_max_mean_bwd(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t B, int64_t F,
                             const float* out, const float* dout, float* dx, int64_t lddx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-hop enclosing-subgraph extraction + PyG Batch collate.  Replaces the
 * per-sample Python loops of local_subgraph_generation (reference src/classes.py:652-733) and the
 * DataLoader collate in front of Net_1.  Interaction graph = CSR over node serial numbers:
 * ptr[N+1], nbr[nnz] partners in interaction_list order (npi_csr_build_ex keeps it), ok[nnz] = pair usable
 * (not in set_allInteractionKey_cannotUse, src/generate_dataset.py:296-299).  keys[B][2] = (rna, protein)
 * targets.  Local node order of a sample: rna, protein, usable partners of the rna, then of the protein;
 * pairs: target first, then in that same order, each in both directions ((rna, protein) first).
 *   npi_subgraph_sizes   : node_off[B+1], pair_off[B+1] (exclusive prefix sums; directed edges = 2 pairs);
 *                          workspace int32[2B]; node_off[B] = pair_off[B] = -1 when the batch exceeds 2^31 - 1 rows
 *   npi_subgraph_fill    : node_id[n], batch[n] (int64), edge_src/edge_dst[2 * pairs] (int64, batch-global ids).  n_nodes /
 *                          n_pairs: the totals the CALLER sized those arrays with; when they are not node_off[B] / pair_off[B]
 *                          (totals computed for other keys) bit 2 (value 4) of status[0] is raised -- an error the host reads at its
 *                          next device read instead of an out-of-bounds write (status may be NULL) -- and the arrays are filled,
 *                          within the caller's sizes, with values every consumer is safe on until then: node 0 / graph 0 for
 *                          every row, the (-1, -1) padding column for every edge
 *   npi_subgraph_features: x[row] = [row is a target ? 0 : 1 | feat[node_id[row]][0..Ff)]; zero rows unless node_off[B] == n
 * ------------------------------------------------------------------------------------------ */
int npi_subgraph_sizes(const int32_t* ptr, const int32_t* nbr, const uint8_t* ok, const int32_t* keys, int64_t B,
                       int32_t* node_off, int32_t* pair_off, int32_t* workspace, void* stream);
int npi_subgraph_fill(const int32_t* ptr, const int32_t* nbr, const uint8_t* ok, const int32_t* keys, int64_t B,
                      const int32_t* node_off, const int32_t* pair_off, int32_t* node_id, int64_t* batch,
                      int64_t* edge_src, int64_t* edge_dst, int64_t n_nodes, int64_t n_pairs, int32_t* status, void* stream);
int npi_subgraph_features(const float* feat, int64_t ldf, int64_t Ff, const int32_t* node_id, const int64_t* batch,
                          const int32_t* node_off, int64_t B, int64_t n, float* x, int64_t ldx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Enclosing subgraphs: h-hop induced extraction with DRNL labels -- SEAL's data construction (Zhang & Chen, NeurIPS 2018; PyG's
 * `seal_link_pred` example) over any undirected graph in one id space, where the entry points above restate the reference's
 * one-hop star.  It follows the rule below, NOT the reference's own h-hop class, which is dead code.
 *
 * Rule H.  Inputs: edge_index [2, E] over N nodes holding every edge in both directions; an optional mask [E] (0: the column does
 * not exist), equal on the two directions of an edge; keys [B, 2], one (u, v) per sample, u != v and both in [0, N); h >= 1 hops.
 * Integer work throughout; the output is a pure function of these inputs.
 *   1. Walkable. Column e = (j -> i) is walkable for sample g iff j != i, the mask allows e, and {i, j} != {u_g, v_g}: the target
 *               link -- in either direction, every parallel copy -- is never walked and never emitted (no label leakage).
 *   2. Nodes.   S_g = { w : min(d(u, w), d(v, w)) <= h }, d the BFS distance over walkable entries.
 *   3. Order.   Local node 0 is u, local node 1 is v, the rest of S_g follows in ascending global id.
 *   4. Edges.   For local a = 0 .. n_g - 1 in order: the walkable entries whose target is node_id[a] and whose source lies in S_g,
 *               in ascending (source id, column number) order -- the order of a by-target CSR built with NPI_CSR_SORT_COLUMNS --,
 *               each as (local(source) + off_g, a + off_g) with e_id = its column number; parallel duplicates as often as they
 *               occur.  edge_dst comes out non-decreasing.  With NPI_ENCLOSE_ADD_TARGET_EDGE one (1 -> 0) column is put in front
 *               of row 0's entries and one (0 -> 1) column in front of row 1's, both with e_id = -1, whether or not the graph had
 *               the link (the reference's convention: positives and negatives both carry their target edge).
 *   5. Labels.  Inside the sample, over its emitted entries with e_id >= 0: dist[w, 0] = the BFS distance from local 0 with local 1
 *               removed (the source itself 0; node 1 and anything unreachable -1), dist[w, 1] = from local 1 with local 0 removed.
 *               z = 1 for the two targets, 0 where either distance is -1, otherwise with d = du + dv
 *                   z = 1 + min(du, dv) + (d / 2) * (d / 2 + d % 2 - 1)           (integer division; SEAL's DRNL), int64.
 * A bad key (u == v, or an id outside [0, N)) gives an EMPTY sample -- 0 nodes, 0 edges -- and raises NPI_STATUS_BAD_ENCLOSE_KEY.
 *
 * The parent graph is passed as its by-target CSR: rowptr [N + 1], col, eid of npi_csr_build_ex(dst, src, ...) WITHOUT self loops,
 * with NPI_CSR_DROP_EQUAL | NPI_CSR_SORT_COLUMNS ((i, i) columns dropped, a row's entries by source id); mask (uint8 [E], may be NULL) is looked up
 * through eid.  One workgroup per sample; no synchronisation between workgroups, no spin-waits; every loop is bounded by its input.
 *   workspace : npi_enclose_workspace_bytes(N, B) bytes (-1: bad size), 4-byte aligned, needs no clearing: per sample four bitmaps'
 *               worth of ceil(N / 32) words -- visited, current, next and the exclusive popcount prefix of visited, from which
 *               local(w) = 2 + rank(w) - [u < w] - [v < w].  npi_enclose_fill reads what npi_enclose_sizes left there: the two
 *               calls of a batch share keys, flags, mask and workspace.
 *   npi_enclose_sizes   : BFS marking, then counts[g] = n_g, counts[B + g] = e_g (the added target columns included) and their
 *                         exclusive prefix sums node_off[B + 1] / edge_off[B + 1]; both totals are -1 when one passes 2^31 - 2.
 *   npi_enclose_fill    : node_id [n] (int32), batch [n], edge_src / edge_dst / e_id [e] (int64, batch-global row ids), and the
 *                         by-target CSR of the emitted entries over the batch's rows: local_rowptr [n + 1], local_col [e] (int32) --
 *                         the entries are grouped by target already, so this is a counter, not a sort.  graph_ptr / edge_ptr
 *                         [B + 1] (int32): node_off / edge_off as the consumers of the batch get them.  n_nodes / n_edges: the
 *                         totals the CALLER sized the arrays with; when they are not node_off[B] / edge_off[B] nothing is
 *                         written through the offsets: node 0 / graph 0 for every row, (-1, -1) with e_id -1 for every column,
 *                         empty local rows, graph_ptr / edge_ptr = [0, n_nodes, n_nodes, ...] / [0, n_edges, ...] (one graph of the
 *                         caller's size, the rest empty), and NPI_STATUS_BAD_ENCLOSE_TOTALS.
 *   npi_drnl_label      : Rule H 5 over ANY batch of graphs given as a by-target CSR over the batch's n rows (nnz: the length of
 *                         col): graph g = rows [graph_ptr[g], graph_ptr[g + 1]), targets src[g] / dst[g] (int32 row ids; both NULL:
 *                         the graph's first two rows).  An entry whose source is its own row (a loop) or lies outside the graph is
 *                         skipped; every index is clamped to the arrays.  z [n] int64, dist [n, 2] int32; rows outside every graph
 *                         are not written.  A graph whose targets are equal or outside it gets z = 0, dist = -1.
 *   npi_enclose_features: x[row] = [label | feat[node_id[row]][0 .. Ff)], pad columns up to ldx zero; label = float(z[row])
 *                         (NPI_ENCLOSE_LABEL_DRNL), 0 for a sample's two targets and 1 elsewhere (NPI_ENCLOSE_LABEL_TARGETS, the
 *                         reference's), or no column (NPI_ENCLOSE_LABEL_NONE; then Ff > 0).  Zero rows unless node_off[B] == n and
 *                         edge_off[B] == e: the test of npi_enclose_fill.
 * status (int32 device word, may be NULL) is OR-ed into, never cleared.  Refused with NPI_ERR_ARG before any launch: N outside
 * [1, 2^31 - 1), B or a total outside its range, hops < 1, an unknown flag or label, a negative, short or misaligned workspace, a
 * pitch below its width, a null pointer for anything that would be read or written.
 * Out of scope: max_nodes_per_hop sampling, directed graphs, bf16 features.
 * ------------------------------------------------------------------------------------------ */
#define NPI_ENCLOSE_ADD_TARGET_EDGE 1
#define NPI_ENCLOSE_LABEL_NONE 0
#define NPI_ENCLOSE_LABEL_DRNL 1
#define NPI_ENCLOSE_LABEL_TARGETS 2
#define NPI_STATUS_BAD_ENCLOSE_KEY 4096
#define NPI_STATUS_BAD_ENCLOSE_TOTALS 8192
int64_t npi_enclose_workspace_bytes(int64_t N, int64_t B);
int npi_enclose_sizes(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const uint8_t* mask, int64_t N,
                      const int32_t* keys, int64_t B, int64_t hops, int flags, int32_t* counts /* [2 B] */, int32_t* node_off,
                      int32_t* edge_off, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);
int npi_enclose_fill(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const uint8_t* mask, int64_t N,
                     const int32_t* keys, int64_t B, int flags, const int32_t* node_off, const int32_t* edge_off,
                     void* workspace, int64_t workspace_bytes, int32_t* node_id, int64_t* batch, int64_t* edge_src,
                     int64_t* edge_dst, int64_t* e_id, int32_t* local_rowptr, int32_t* local_col, int32_t* graph_ptr,
                     int32_t* edge_ptr, int64_t n_nodes, int64_t n_edges, int32_t* status, void* stream);
int npi_drnl_label(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const int32_t* src, const int32_t* dst,
                   const int32_t* graph_ptr, int64_t B, int64_t* z /* [n] */, int32_t* dist /* [n, 2] */, void* stream);
int npi_enclose_features(const float* feat, int64_t ldf, int64_t Ff, const int32_t* node_id, const int64_t* z,
                         const int64_t* batch, const int32_t* node_off, const int32_t* edge_off, int64_t B, int64_t n,
                         int64_t e, int label, float* x, int64_t ldx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Neighbour sampling: the producer of the (x_src, None) / size= / res_n_id arguments of the bipartite layers.  Replaces, one hop
 * per sequence of calls, PyG 1.4.2 `torch_geometric.data.NeighborSampler.__produce_bipartite_data_flow__`:
 * `torch_cluster.neighbor_sampler(n_id, cumdeg, size)`, `torch.unique` over the sampled sources and the `tmp[n_id] = arange`
 * relabelling, all of which run on the CPU there.
 *
 * Input: the by-target CSR of the edge list AS IT IS (npi_csr_build_ex with key = edge_index[1], val = edge_index[0],
 * add_self_loops = 0, build_flags = 0): rowptr[N+1], col[nnz] = source, eid[nnz] = column of edge_index.  targets[n]: int64 global
 * ids of the hop's target list; an id outside [0, N) is never dereferenced: it gets no entry and raises NPI_STATUS_BAD_TARGET_ID.
 *
 * THE RULE.  Target v has d = rowptr[v+1] - rowptr[v] in-edges; its budget is k = min(d, budget) for an integer budget >= 1, or
 * k = min(d, ceil((double)frac * d)) for budget == 0 and a fraction 0 < frac <= 1 (the torch_cluster rule).  Position p of the row
 * (0 <= p < d) gets the 64-bit key (h32(seed, hop, v, p) << 32) | p, with all arithmetic in wrapping uint64:
 *     mix64(z) : z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *     base     = mix64( mix64(seed + 0x9E3779B97F4A7C15 * (hop + 1))  ^  (v * 0xD6E8FEB86659FD93) )
 *     h32      = mix64(base + 0x9E3779B97F4A7C15 * (p + 1)) >> 32
 * (splitmix64: one stream per (seed, hop, v), its p-th output, upper half).  The sample of v is the k positions with the SMALLEST
 * keys -- a uniform draw without replacement; p makes every key distinct -- emitted in ascending p; targets are emitted in list
 * order.  The result is a pure function of (seed, hop, v, the row): bitwise reproducible, independent of the other targets of the
 * call, of the launch geometry and of timing.  The random bits are not PyG's; the distribution and the structure are.
 *
 *   npi_sample_counts        : cnt[t] = k of targets[t] (int32); clears status[0] first (status may be NULL).  The caller turns cnt
 *                              into offsets[n+1] (int64 exclusive sums, offsets[0] = 0).
 *   npi_sample_select        : for every target its k entries at offsets[t] .. offsets[t+1]: out_src = col[pos] (global source
 *                              id), out_eid = eid[pos], out_tgt = t.  n_out: the length the caller gave the three arrays; offsets
 *                              that do not fit it or a row (offsets of another call) write nothing for that target and raise
 *                              NPI_STATUS_BAD_SAMPLE_SIZES.
 *   npi_sample_relabel_count : marks the sampled sources (the first min(offsets[n], n_out) entries of out_src) -- and, with
 *                              add_self_loops != 0, the targets -- in scratch[N] (int32, ALL ZERO on entry, 16-byte aligned), counts
 *                              them per chunk into workspace[npi_sample_workspace_elems(N)] and writes info[0] = number of distinct
 *                              ids U, info[1] = number of sampled entries E.  The caller reads info (the one host read of a hop:
 *                              U and E size the outputs below).
 *   npi_sample_relabel       : n_id[U] = the marked ids in ascending order (PyG's `unique(sorted=False)` leaves the order open);
 *                              edge_src[E] = index of out_src in n_id, edge_dst[E] = out_tgt, e_id[E] = out_eid (all int64, the
 *                              rows of Block.edge_index and Block.e_id); res_n_id[n] = index of targets[t] in n_id (NULL without
 *                              self loops; -1 for an id out of range).  U other than the count of the marks raises
 *                              NPI_STATUS_BAD_SAMPLE_SIZES and writes within U.  Leaves scratch ALL ZERO again.
 * ------------------------------------------------------------------------------------------ */
#define NPI_STATUS_BAD_TARGET_ID 16
#define NPI_STATUS_BAD_SAMPLE_SIZES 32
int npi_sample_counts(const int32_t* rowptr, int64_t N, const int64_t* targets, int64_t n, int64_t budget, float frac,
                      int32_t* cnt, int32_t* status, void* stream);
int npi_sample_select(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t N, const int64_t* targets, int64_t n,
                      const int64_t* offsets, int64_t seed, int64_t hop, int32_t* out_src, int32_t* out_eid, int32_t* out_tgt,
                      int64_t n_out, int32_t* status, void* stream);
int64_t npi_sample_workspace_elems(int64_t N);
int npi_sample_relabel_count(const int32_t* out_src, const int64_t* offsets, int64_t n, int64_t n_out, const int64_t* targets,
                             int add_self_loops, int32_t* scratch, int64_t N, int32_t* workspace, int32_t* info, void* stream);
int npi_sample_relabel(int32_t* scratch, int64_t N, const int32_t* workspace, const int32_t* out_src, const int32_t* out_eid,
                       const int32_t* out_tgt, int64_t E, const int64_t* targets, int64_t n, int64_t U, int64_t* n_id,
                       int64_t* edge_src, int64_t* edge_dst, int64_t* e_id, int64_t* res_n_id, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Neighbour sampling, the ONE-ID-SPACE data flow: the producer of the sampled subgraph that the square layers (SAGEConv, GCNConv,
 * GATConv over a CSRGraph, GraphBatch) run over.  Replaces PyG 1.4.2 `torch_geometric.data.NeighborSampler.__produce_subgraph__`
 * (`bipartite=False`), which walks the hops with `torch_cluster.neighbor_sampler`, concatenates their `n_id` / `e_id`, takes
 * `n_id.unique(sorted=False)`, relabels both edge ends through `tmp[n_id] = arange`, merges equal pairs with
 * `idx = src * num_nodes + dst; idx.unique()` and `scatter_`s one `e_id` per pair, all on the CPU.
 *
 * SEMANTICS.  For a batch b_id[n] (int64 global ids, repeats allowed), budgets size[0 .. L) and a key seed s:
 *   T_0 = b_id; hop l samples the in-edges of every node of T_l by THE RULE above with (seed, hop) = (s, l) and the budget size[l];
 *   T_{l+1} = the distinct sources sampled at hop l, ascending (targets are NOT carried over; add_self_loops plays no part).
 * These hops ARE the blocks of the bipartite data flow with add_self_loops = 0 for the same seed and batch: the caller runs
 * npi_sample_counts / npi_sample_select (/ npi_sample_relabel for T_{l+1}) per hop and hands the concatenation of the hops'
 * sampled entries -- src_g, dst_g (global ids of both ends), eid (column of the edge list), int32, E entries -- to the two calls
 * below.  Results:
 *   n_id        the distinct ids of b_id u T_1 u ... u T_L, ASCENDING (PyG's unique(sorted=False) leaves the order open); a batch
 *               node without in-edges is in it, isolated.  num_nodes = U = its length.
 *   sub_b_id[t] the position of b_id[t] in n_id (repeats repeat; -1 for an id outside [0, N), which is never dereferenced and raises
 *               NPI_STATUS_BAD_TARGET_ID).
 *   edge_index  the sampled edges of all hops with both ends relabelled into n_id positions, equal (src_local, dst_local) pairs
 *               merged into one column -- a pair repeats when its target is a target of two hops, for parallel edges of a multigraph
 *               and for a repeated batch id -- in ASCENDING (src_local, dst_local) order (the order of PyG's idx.unique() on the
 *               CPU).  (v, v) columns of the edge list are ordinary edges and stay.  Nothing sampled: no column.
 *   e_id        for each column the SMALLEST edge-list column among the merged ones (PyG's scatter_ leaves open which survives).
 * A pure function of (seed, batch, graph): bitwise reproducible, independent of launch geometry and timing (no float, no
 * order-dependent atomic: idempotent marks, stable sorts, a minimum).
 *
 *   npi_sample_union    : marks every src_g / dst_g / b_id in scratch[N] (int32, ALL ZERO on entry, 16-byte aligned; the sampler's),
 *                         counts the marks per chunk into workspace[npi_sample_workspace_elems(N)], writes info[0] = U and
 *                         info[1] = E, n_id[0 .. U) (n_id_cap: the length the caller gave n_id; U <= min(N, n + E) always holds for
 *                         hops as above, so that bound sizes it without a host read), src_l[E] / dst_l[E] = the positions of the
 *                         two ends in n_id (int32; -1 for an id outside [0, N)), sub_b_id[n].  More marks than n_id_cap: writes
 *                         within it and raises NPI_STATUS_BAD_SAMPLE_SIZES.  status[0] (may be NULL) is OR-ed into, never cleared.
 *                         Leaves scratch ALL ZERO again.
 *   npi_sample_coalesce : two stable radix sorts of the E entries on the bits that U - 1 needs (dst_l, then src_l, carrying the
 *                         entry index), run heads, their scan, and the compaction: edge_src / edge_dst / e_id[0 .. E_u) (int64; the
 *                         caller sizes them with the bound E) and info[0] = E_u.  workspace: npi_sample_coalesce_workspace_bytes(E)
 *                         bytes, 16-byte aligned.  Ids must lie in [0, U) (npi_sample_union's).
 * Both allocate nothing, keep no state and do nothing (return 0) for empty input (E == 0 and, for the union, n == 0).  The caller
 * reads (U, E_u) once, with the status word, and trims.
 * ------------------------------------------------------------------------------------------ */
int npi_sample_union(const int32_t* src_g, const int32_t* dst_g, int64_t E, const int64_t* b_id, int64_t n, int32_t* scratch,
                     int64_t N, int32_t* workspace, int64_t n_id_cap, int64_t* n_id, int32_t* src_l, int32_t* dst_l,
                     int64_t* sub_b_id, int32_t* info, int32_t* status, void* stream);
int64_t npi_sample_coalesce_workspace_bytes(int64_t E);
int npi_sample_coalesce(const int32_t* src_l, const int32_t* dst_l, const int32_t* eid, int64_t E, int64_t U, int64_t* edge_src,
                        int64_t* edge_dst, int64_t* e_id, int32_t* info, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Negative sampling: the pairs a link-prediction loss is taken against.  Replaces the reference's offline loop
 * `src/generate_edgelist.py:108-139` (draw a uniform ncRNA and a uniform protein; redraw if the pair is a positive or was already
 * drawn; stop at as many negatives as positives) and PyG 1.4.2 `torch_geometric.utils.negative_sampling` /
 * `structured_negative_sampling`, which run through Python `random.sample` and `isin` on the CPU.
 *
 * Input of both kernels: the by-target CSR WITH SORTED COLUMNS of the edge list as it is (npi_csr_build_ex with key = edge_index[1],
 * val = edge_index[0], add_self_loops = 0, build_flags = NPI_CSR_SORT_COLUMNS, NPI_CSR_DROP_EQUAL not set): rowptr[n_dst+1],
 * col[nnz] = source ids, ASCENDING within a row -- the rows MUST be sorted: membership is a binary search of row d for s.  "Edge"
 * means a column of the edge list as it is: no self loop is added or removed, parallel edges count once.
 *
 * THE TWO RULES.  All arithmetic in wrapping uint64; mix64 is the sampler's (above):
 *     mix64(z)    : z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *     G = 0x9E3779B97F4A7C15,  C = 0xD6E8FEB86659FD93
 *     mulhi(a, n) = (a * n) >> 64 of the 128-bit product: a 64-bit word to [0, n) with a bias below n / 2^64
 *     key         : a signed 64-bit integer (the Python side passes sampler.epoch_seed(seed, draw))
 *
 * RULE P -- distinct non-edge pairs (the reference's loop driven by a counter-based generator):
 *     base  = mix64(mix64(key) + G)
 *     src_i = mulhi(mix64(base + G * (2i + 1)), n_src)        i = 0, 1, 2, ...
 *     dst_i = mulhi(mix64(base + G * (2i + 2)), n_dst)
 * Candidate i is VALID if (src_i, dst_i) is not an edge and -- with no_loops -- src_i != dst_i.  The result is the first M valid
 * candidates that differ from every earlier valid candidate, in order of i: a uniform draw without replacement from the non-edges,
 * a pure function of (key, graph, M, no_loops) -- independent of launch geometry, of timing and of how many candidates the caller
 * looks at per round.
 *
 * RULE T -- corrupt the target of given sources (PyG's structured_negative_sampling; slots are independent, equal results in
 * different slots are allowed, as they are there):
 *     base_k = mix64( mix64(mix64(key) + 2 * G)  ^  (k * C) )            slot k = 0 .. K-1
 *     d_k,t  = mulhi(mix64(base_k + G * (t + 1)), n_dst)                  t = 0 .. tries-1
 * out[k] = the first d_k,t for which (src[k], d_k,t) is not an edge; none (the source is joined to every target, or tries ran out):
 * -1 and NPI_STATUS_NO_NEGATIVE.  A src[k] outside [0, n_src) is never dereferenced: -1 and NPI_STATUS_BAD_SOURCE_ID.
 *
 *   npi_negative_candidates : candidates first .. first + W - 1 of Rule P: cand_src[j], cand_dst[j] (int32) = candidate first + j,
 *                             or (-1, -1) when it is invalid.  flags bit 0: no_loops.
 *   npi_negative_targets    : Rule T: out_dst[K] (int64).  status (int32 device word, may be NULL) is cleared first, then OR-ed
 *                             into.  No host read and no allocation: it may run inside a stream capture.
 *   npi_negative_distinct   : the first M distinct valid pairs of a window of W candidates (npi_negative_candidates' output for
 *                             first = 0): two stable radix sorts on the bits the id bounds need (target, then source with one more
 *                             bit that sorts the invalid candidates last, carrying the position), run heads -- the earliest
 *                             occurrence of each pair -- set keep[position], an exclusive scan of keep in position order, and the
 *                             compaction: out_src / out_dst[0 .. min(M, info[0])) (int64) in position order.  info[0] = the number
 *                             of distinct valid pairs in the window; info[1] = the number of candidates consumed up to and including
 *                             the M-th kept one, 0 if the window holds fewer than M (the caller then runs a window twice as long,
 *                             from candidate 0).  workspace: npi_negative_distinct_workspace_bytes(W) bytes, 16-byte aligned.
 * All allocate nothing and keep no state.  Bad arguments -- a null pointer, a negative size, W / K or an id bound >= 2^31 - 1 (or an
 * id bound below 1), tries < 1, a misaligned or short workspace -- are refused with -1 before anything is launched; W == 0 / K == 0
 * returns 0 without a launch.
 * ------------------------------------------------------------------------------------------ */
#define NPI_STATUS_NO_NEGATIVE 64
#define NPI_STATUS_BAD_SOURCE_ID 128
int npi_negative_candidates(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t n_src, int64_t key, int64_t first,
                            int64_t W, int flags, int32_t* cand_src, int32_t* cand_dst, void* stream);
int npi_negative_targets(const int32_t* rowptr, const int32_t* col, int64_t n_dst, int64_t n_src, const int64_t* src, int64_t K,
                         int64_t key, int64_t tries, int64_t* out_dst, int32_t* status, void* stream);
int64_t npi_negative_distinct_workspace_bytes(int64_t W);
int npi_negative_distinct(const int32_t* cand_src, const int32_t* cand_dst, int64_t W, int64_t n_src, int64_t n_dst, int64_t M,
                          int64_t* out_src, int64_t* out_dst, int32_t* info, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Random walks and the skip-gram pair list: the node2vec columns of the feature vector, made where the graph already is.  Replaces
 * the reference's offline step `node2vec-master/src/main.py` (alias-sampled walks, 10 x 80 per node, then gensim) and PyG 1.4.2
 * `torch_geometric.nn.models.Node2Vec` over `torch_cluster.random_walk`.
 *
 * Input of npi_random_walk: the BY-SOURCE CSR WITH SORTED COLUMNS of the edge list as it is (npi_csr_build_ex with key =
 * edge_index[0], val = edge_index[1], add_self_loops = 0, build_flags = NPI_CSR_SORT_COLUMNS, NPI_CSR_DROP_EQUAL not set):
 * rowptr[N+1], col[nnz] = target ids, ASCENDING within a row -- the rows MUST be sorted: "is (u, x) an edge" is a binary search of
 * row u for x.  Parallel edges stay: they weigh in the uniform pick as in torch_cluster, and count once for membership.
 *
 * RULE W -- second-order walks by rejection.  mix64, G, C, mulhi and key as in the two rules above; all arithmetic wrapping uint64:
 *     root    = mix64(mix64(key) + 3 * G)
 *     base_w  = mix64(root ^ (w * C))                     walk (slot) w = 0 .. W-1: one stream per SLOT, so repeated starts differ
 *     word(i) = mix64(base_w + G * i)                     i = 1, 2, ...
 * Walk w starts at v_0 = start[w].  Step t = 1 .. L, from v = v_{t-1} with d = rowptr[v+1] - rowptr[v]:
 *   d == 0 : v_t = v (torch_cluster's rule: a walk stays at a dead end); no word is consumed.
 *   else   : attempts, numbered n = 0, 1, 2, ... over the WHOLE walk; attempt n draws pick = word(2n + 1), accept = word(2n + 2).
 *            The candidate x = col[rowptr[v] + mulhi(pick, d)] is accepted iff (accept >> 32) < thr, where
 *                thr = 2^32     when there is no previous node (t == 1),
 *                      thr_ret  when x == v_{t-2},
 *                      thr_nbr  when (v_{t-2}, x) is an edge (binary search of row v_{t-2}),
 *                      thr_far  otherwise.
 *            v_t = the first accepted candidate of at most `tries` attempts; none accepted: the LAST candidate is taken and
 *            NPI_STATUS_WALK_TRIES is raised.
 * The three thresholds are integers in [0, 2^32] (int64_t arguments, like every scalar of this header); there is no float in the kernel, so the rule is bitwise restatable.  (The Python
 * side computes them in double as min(2^32, floor(2^32 * a / mx)) for a in (1/p, 1, 1/q), mx = the largest of the three.)  With all
 * three 2^32 (p == q == 1) every first attempt is accepted and step t uses word(2t - 1); the kernel then skips the accept word and
 * the search, with the identical result.  A start[w] outside [0, N) is never dereferenced: the whole row is -1 and
 * NPI_STATUS_BAD_SOURCE_ID is raised.  Output: walks[W, L+1] int64, row-major (torch_cluster's layout).  A pure function of (key,
 * graph, start, L, thresholds, tries) -- independent of launch geometry and timing.
 *
 * npi_walk_pairs writes the pair list of PyG's `Node2Vec.loss` in the cat([pos, neg], 1) layout npi_pair_score takes.  With
 * J = L + 2 - c windows per walk and R = J * W window rows, row r = j * W + w (PyG's torch.cat(walks, dim=0) order) starts at
 * walks[w, j]:
 *     positives : m = r * (c-1) + (k-1),        k = 1 .. c-1 :  (walks[w, j], walks[w, j+k])
 *     negatives : m = R * (c-1) + r * S + s,    s = 0 .. S-1 :  (walks[w, j], mulhi(mix64(nbase + G * (r * S + s + 1)), N))
 *     nbase = mix64(mix64(key) + 4 * G)
 * A negative is a uniform node, as PyG's torch.randint: it may be the start or a true neighbour, as there.  -1 entries of a bad walk
 * are copied as they are (npi_pair_score scores such a pair 0 and reports it).  n_pos of npi_pair_score is R * (c-1);
 * M = R * (c - 1 + S) must stay below 2^31 - 1.
 *
 * Neither allocates or reads anything back: both may run inside a stream capture.  Refused with NPI_ERR_ARG before any launch: a
 * null pointer, a negative size, W, N or M >= 2^31 - 1, N < 1, tries < 1, a threshold outside [0, 2^32], c < 2 or c > L + 1.  W == 0
 * returns 0 without a launch.  status (int32 device word, may be NULL) is OR-ed into, never cleared here.
 * ------------------------------------------------------------------------------------------ */
#define NPI_STATUS_WALK_TRIES 512
int npi_random_walk(const int32_t* rowptr, const int32_t* col, int64_t N, const int64_t* start, int64_t W, int64_t L, int64_t key,
                    int64_t thr_ret, int64_t thr_nbr, int64_t thr_far, int64_t tries, int64_t* walks, int32_t* status,
                    void* stream);
int npi_walk_pairs(const int64_t* walks, int64_t W, int64_t L, int64_t c, int64_t S, int64_t N, int64_t key, int64_t* src,
                   int64_t* dst, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pair scores and the link-prediction loss: the third stage of a link-prediction step, after the samplers (the pairs) and the
 * layers (the embeddings).  Replaces PyG 1.4.2 `torch_geometric/nn/models/autoencoder.py`:
 *     InnerProductDecoder.forward : value = (z[edge_index[0]] * z[edge_index[1]]).sum(dim=1); torch.sigmoid(value) if sigmoid
 *     GAE.recon_loss              : pos_loss = -torch.log(self.decoder(z, pos_edge_index, sigmoid=True) + EPS).mean()
 *                                   neg_loss = -torch.log(1 - self.decoder(z, neg_edge_index, sigmoid=True) + EPS).mean()
 *                                   return pos_loss + neg_loss                                    (EPS = 1e-15)
 * and the composition `F.binary_cross_entropy_with_logits((z[i] * z[j]).sum(1), labels)`: two [M, F] gathers, their product and
 * its row sum, then sigmoid / log / mean, each a pass over memory -- here ONE launch over the pair list as it is (no CSR, no sort).
 *
 *   src, dst  : int64 [M] (PyG's edge_index rows / NegativeSampler.pairs as they are).  The first n_pos pairs are POSITIVES, the
 *               other M - n_pos negatives: the layout of `torch.cat([pos_edge_index, neg_edge_index], 1)`
 *   z_src     : f32 [n_src, F], leading dimension ld_src (elements);  z_dst : f32 [n_dst, F], ld_dst.  They may be the same pointer
 *               (one id space).  16-byte lanes when F % 4 == 0 and both bases and pitches are 16-byte aligned; else one float per lane
 *   mode      : NPI_PAIR_LOGITS, NPI_PAIR_LOSS_GAE or NPI_PAIR_LOSS_BCE
 *   logits [M]: <z_src[src_m], z_dst[dst_m]>, f32 accumulation in a fixed order                                     (may be NULL)
 *   coef [M]  : d loss / d logit_m                                                               (loss modes only; may be NULL)
 *   loss [1]  : the loss (loss modes only; may be NULL); needs `partials`: npi_pair_score_workspace_bytes(M) bytes, 16-byte aligned,
 *               caller-owned, fully overwritten (one fp64 partial per workgroup of 256 pairs)
 *   status    : int32 device word as npi_csr_build_ex's (may be NULL): OR-ed into, never cleared here
 * At least one of logits / coef / loss must be given.
 *
 * Per pair, with x = logit_m and s = sigmoid(x) = 1 / (1 + exp(-x)), all in f32:
 *   NPI_PAIR_LOSS_GAE : a positive contributes -log(s + EPS) / n_pos, a negative -log(q + EPS) / (M - n_pos) with q = 1 - s computed
 *                       ONCE; coef is what autograd gives for exactly these expressions: -s q / (s + EPS) / n_pos and
 *                       s q / (q + EPS) / (M - n_pos).  A part WITHOUT a pair (n_pos == 0 or n_pos == M) contributes 0 -- where
 *                       PyG's `.mean()` of an empty tensor gives NaN; a deliberate deviation
 *   NPI_PAIR_LOSS_BCE : binary_cross_entropy_with_logits(logits, y) with y = 1 for a positive, 0 for a negative, mean over all M:
 *                       (max(x, 0) - x y + log1p(exp(-|x|))) / M;  coef = (s - y) / M with s - 1 evaluated as -sigmoid(-x): finite
 *                       and accurate at any logit
 * The loss is a DETERMINISTIC sum: a wavefront adds its 64 terms (fp64) in a fixed tree, a workgroup its four wavefronts in order
 * into one partial, a second one-workgroup launch the partials in a fixed order.  No float atomics anywhere; bitwise reproducible.
 *
 * A pair with src_m outside [0, n_src) or dst_m outside [0, n_dst): logit 0, coef 0, loss term 0 (it still counts in n_pos / M);
 * no row is dereferenced for it and NPI_STATUS_BAD_PAIR_ID is raised (torch's indexing raises there).
 *
 * Nothing is allocated, nothing read back to the host.  Refused with NPI_ERR_ARG before any launch: an unknown mode; M, F, n_src or
 * n_dst negative or >= 2^31 - 1 (F < 1); n_pos outside [0, M]; a leading dimension below F; no output at all; coef or loss in
 * NPI_PAIR_LOGITS mode; loss without partials, or partials misaligned or shorter than npi_pair_score_workspace_bytes(M); a null
 * src / dst / z_src / z_dst when M > 0.  M == 0 returns NPI_OK WITHOUT a kernel launch; loss[0], if given, is then set to 0 by a
 * hipMemsetAsync on `stream`.  npi_pair_score_workspace_bytes returns -1 for an M outside [0, 2^31 - 1).
 *
 * The backward needs no kernel of its own: dZ_dst[j] = sum_{m: dst_m = j} g_m z_src[src_m] and dZ_src[i] = sum_{m: src_m = i} g_m
 * z_dst[dst_m] (g = coef times the upstream gradient) are npi_segsum_ex over the by-target / by-source CSR of the pair list with g
 * as per-entry weights (npi_entry_weights) -- one id space: ONE sum over the CSR of keys cat(src, dst), values cat(dst, src).
 * ------------------------------------------------------------------------------------------ */
#define NPI_PAIR_LOGITS 0
#define NPI_PAIR_LOSS_GAE 1
#define NPI_PAIR_LOSS_BCE 2
#define NPI_STATUS_BAD_PAIR_ID 256
int64_t npi_pair_score_workspace_bytes(int64_t M);
int npi_pair_score(const int64_t* src, const int64_t* dst, int64_t M, int64_t n_pos, const float* z_src, int64_t ld_src,
                   int64_t n_src, const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F, int mode, float* logits, float* coef,
                   float* loss, void* partials, int64_t partials_bytes, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ranking losses over corrupted targets: the listwise / pairwise sibling of npi_pair_score.  Where npi_pair_score pushes every pair
 * towards 0 or 1 on its own, these compare a positive with the corrupted targets of the SAME source -- what filtered MRR / Hits@K
 * (npi_link_ranks) and npi_topk_links measure.  The inputs are what NegativeSampler.corrupt (Rule T, npi_negative_targets),
 * structured_negative_sampling and npi_topk_links' ids already give; no expanded pair list is written.
 *
 * Rule G (the groups):
 *   src, dst  : int64 [P], the positives;  neg : int64 [P, K] with row pitch ld_neg >= K, 0 <= K <= 63 (may be NULL when K == 0)
 *   z_src     : f32 [n_src, F], leading dimension ld_src;  z_dst : f32 [n_dst, F], ld_dst; unit column stride, any pitch >= F; they
 *               may be the same pointer (one id space).  Lane widths as in npi_pair_score
 *   Group p has C = 1 + K slots: slot 0 is (src_p, dst_p), slot c >= 1 is (src_p, neg[p, c-1]).  The logit of a slot is
 *   x_{p,c} = <z_src[src_p], z_dst[target]>, in f32 exactly as npi_pair_score forms it: the value depends on the two rows only, not
 *   on where the group sits in the list or in a wavefront.
 *   Empty slots and bad ids:  neg[p, c-1] == -1 is an EMPTY slot (what corrupt and npi_topk_links write): no row is read, no status
 *   raised, logit -inf, coefficient and loss term 0.  Any other negative id outside [0, n_dst) behaves the same and raises
 *   NPI_STATUS_BAD_PAIR_ID.  A positive whose src or dst is out of range DROPS its whole group and raises the same status: all its
 *   logits, coefficients and terms are 0.
 *   With d_c = scale * (x_c - x_0) over the VALID negative slots V_p, terms and coefficients per slot in f32:
 *     NPI_GROUP_LOSS_BPR     : term softplus(d_c) = max(d, 0) + log1p(exp(-|d|));  loss = sum / (P K);
 *                              coef_c = scale sigmoid(d_c) / (P K)
 *     NPI_GROUP_LOSS_MARGIN  : term max(0, margin + d_c);  loss = sum / (P K);  coef_c = scale [margin + d_c > 0] / (P K) -- strictly
 *                              greater: 0 at the kink
 *     NPI_GROUP_LOSS_SOFTMAX : (sampled softmax / InfoNCE) per group m + log(exp(-m) + sum_V exp(d_c - m)), m = max(0, max_V d_c);
 *                              loss = sum_p / P;  coef_c = scale exp(d_c - m) / den / P
 *   In every form coef_0 = -(sum over c >= 1 of coef_c), added in ascending slot order (never softmax_0 - 1: nothing cancels).
 *   The divisors count SLOTS (P K, or P), not valid slots -- a deliberate deviation from masking followed by `.mean()`: it needs no
 *   host read of a device count, so the call may sit in a stream capture.  K == 0, or a group without a valid negative, contributes
 *   0; P == 0 gives loss 0.  The loss is a DETERMINISTIC sum, npi_pair_score's scheme: f32 terms, fp64 sums in a fixed order, one
 *   partial per workgroup (4 wavefronts of 64 / C whole groups each), then the one-workgroup sum.  No float atomics.
 * In numpy (fp64; the device computes logits, terms and coefficients in f32):
 *     tgt = concatenate([dst[:, None], neg], 1);  keep = (0 <= src) & (src < n_src) & (0 <= dst) & (dst < n_dst)
 *     valid = keep[:, None] & (0 <= tgt) & (tgt < n_dst);  V = valid.copy();  V[:, 0] = False
 *     x = where(valid, einsum("pf,pcf->pc", z_src[clip(src, 0, n_src-1)], z_dst[clip(tgt, 0, n_dst-1)]), where(keep[:, None], -inf, 0))
 *     d = where(V, scale * (x - x[:, :1]), -inf)
 *     bpr:     loss = where(V, logaddexp(0, d), 0).sum() / (P*K);      coef = where(V, scale / (1 + exp(-d)), 0) / (P*K)
 *     margin:  loss = where(V, maximum(0, margin + d), 0).sum() / (P*K);  coef = where(V & (margin + d > 0), scale, 0) / (P*K)
 *     softmax: m = maximum(0, d.max(1, initial=0));  den = exp(-m) + exp(d - m[:, None]).sum(1)
 *              loss = (m + log(den)).sum() / P;                        coef = scale * exp(d - m[:, None]) / den[:, None] / P
 *     coef[:, 0] = -coef[:, 1:].sum(1)
 *
 *   mode       : NPI_GROUP_LOGITS (logits only) or one of the three loss modes; margin is read by NPI_GROUP_LOSS_MARGIN only
 *   logits, coef : f32 [P, 1 + K] dense (either may be NULL);  coef = d loss / d logit       (coef: loss modes only)
 *   loss [1]   : loss modes only; may be NULL; needs `partials`: npi_group_score_workspace_bytes(P, K) bytes, 16-byte aligned,
 *                caller-owned, fully overwritten
 *   status     : as npi_pair_score's
 * Nothing is allocated, nothing read back.  Refused with NPI_ERR_ARG before any launch: an unknown mode; P, F, n_src or n_dst
 * negative or >= 2^31 - 1 (F < 1); K outside [0, 63]; P (1 + K) >= 2^31 - 1; ld_neg < K; a leading dimension below F; a margin or
 * scale that is not finite, scale <= 0; no output at all; coef or loss in NPI_GROUP_LOGITS mode; loss without partials, or partials
 * misaligned or short; a null src / dst / z_src / z_dst (neg when K > 0) when P > 0.  P == 0 returns NPI_OK WITHOUT a kernel
 * launch; loss[0], if given, is then set to 0 by a hipMemsetAsync on `stream`.  npi_group_score_workspace_bytes returns -1 on a bad
 * size, else a multiple of 16 that is at least 8.
 *
 * The backward is npi_pair_score's: npi_segsum_ex over the sides of the EXPANDED list (src repeated C times; dst and neg
 * interleaved, empty slots clamped to row 0) with g = coef times the upstream gradient as per-entry weights.  Empty, bad and
 * dropped slots carry weight exactly 0.  The expanded list exists in the backward only.
 *
 * Out of scope: K > 63, bf16 tables, per-slot weights, corrupting the source side (swap the tables), a loss over npi_topk_links'
 * scores without re-scoring.
 * ------------------------------------------------------------------------------------------ */
#define NPI_GROUP_LOGITS 0
#define NPI_GROUP_LOSS_BPR 1
#define NPI_GROUP_LOSS_MARGIN 2
#define NPI_GROUP_LOSS_SOFTMAX 3
int64_t npi_group_score_workspace_bytes(int64_t P, int64_t K);   /* -1 on a bad size; 16-byte multiple, >= 8 */
int npi_group_score(const int64_t* src, const int64_t* dst, int64_t P, const int64_t* neg, int64_t ld_neg, int64_t K,
                    const float* z_src, int64_t ld_src, int64_t n_src, const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                    int mode, float margin, float scale, float* logits /* [P, 1+K] dense */, float* coef /* [P, 1+K] dense */,
                    float* loss, void* partials, int64_t partials_bytes, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The variational half of PyG 1.4.2 `torch_geometric/nn/models/autoencoder.py` (VGAE / ARGVA):
 *     VGAE.reparametrize : mu + torch.randn_like(logvar) * torch.exp(0.5 * logvar)                     (training mode)
 *     VGAE.kl_loss       : -0.5 * torch.mean(torch.sum(1 + logvar - mu**2 - logvar.exp(), dim=1)),  logvar.clamp(max=MAX_LOGVAR)
 * some ten elementwise passes over [N, F] tables, a saved randn and a saved exp tensor, and torch's stateful generator -- here ONE
 * launch forward and ONE backward.  The noise is a pure function of (seed, draw, tick, table, row, column), recomputed in the
 * backward as Rule D's mask is: no eps and no sigma array exist, and a step is reproducible from (seed, draw, tick).
 *
 * Rule N (the seeded standard normal; the counter-based generator of the other rules, npi_gnn_amd/csrc/draw.h, then Box-Muller in
 * npi_gnn_amd/csrc/gauss.h; wrapping uint64 throughout, G = 0x9E3779B97F4A7C15, C = 0xD6E8FEB86659FD93):
 *     key    = epoch_seed(seed, draw)                          as every other rule (npi_sample_select's description)
 *     root   = mix64(mix64(key) + 7 G)                         draw_root(key, DRAW_RULE_N)
 *     root_t = mix64(root + G (tick + 1))                      draw_word(root, tick + 1); tick = 0 when no tick word is given
 *     slot   = table * 2^32 + row                              table: 0 (one id space, or z_src), 1 (z_dst); 0 <= row < 2^31 - 1
 *     w_p    = mix64(mix64(root_t ^ (slot C)) + G (p + 1))     draw_word(draw_stream(root_t, slot), p + 1); p = column >> 1
 *     u1     = float32((w_p >> 40) + 1) * 2^-24                in (0, 1]: exact
 *     u2     = float32((w_p >> 16) & 0xFFFFFF) * 2^-24         in [0, 1): exact
 *     theta  = float32(0x40C90FDB) * u2                        ONE f32 multiply by float32(2 pi)
 *     r      = sqrt(-2 ln u1)
 *     eps    = r cos(theta) for an even column, r sin(theta) for an odd one       (Box-Muller; one word serves two columns)
 * Everything up to theta is exact and bit-identical on the device; ln, cos and sin are defined by their mathematical values at the
 * f32 inputs u1 and theta, and the device evaluates them with the full-precision logf / sincosf / sqrtf (never the hardware
 * approximations): |eps_device - eps| <= 16 * 2^-24 * max(1, |eps|).  |eps| <= sqrt(48 ln 2) = 5.77.
 * `tick` is an optional DEVICE int64 word the kernel reads.  Every other rule bakes its key into the launch by value, so a captured
 * step replays the same draw; noise that must be fresh on every replay of a HIP graph counts the word up inside the graph
 * (`tick.add_(1)`), with nothing read back.  The forward and its backward must see the same value of the word.
 * In numpy (uint64 arrays wrap), eps in float64:
 *     def mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *     root_t = mix64(mix64(mix64(uint64(key)) + 7 * G) + G * (tick + 1));  stream = mix64(root_t ^ ((table * 2**32 + row) * C))
 *     w = mix64(stream[:, None] + G * (arange(ceil(F / 2)) + 1));  u1 = float32((w >> 40) + 1) * float32(2**-24)
 *     theta = float32(2 * pi) * (float32((w >> 16) & 0xFFFFFF) * float32(2**-24));  r = sqrt(-2 * log(float64(u1)))
 *     eps[:, 0::2], eps[:, 1::2] = r * cos(float64(theta)), r * sin(float64(theta))            (the last odd column cut off)
 * Known answers (seed 0, draw 0): key = 0xe220a8397b1dcdaf, root = 0x17b5b595bf33339a, root_t = 0xa7ef72c3db16c2d7 (tick 0),
 * 0xa8877caa7f09cab9 (tick 1); tick 0: table 0 row 0 words p = 0, 1: 0x889234032688d558, 0x069a7caf18ce8061; table 0 row 1:
 * 0x205b65805dff0d2e, 0x01ca425f2169d826; table 1 row 0 word 0: 0xe4e0adf25a413b08;
 * eps[0, 0:4] = 1.1176605005754783, 0.08659600134496356, -1.0901547752580947, -2.475222608957373.
 *
 *   mu, logvar : f32 [N, F] with leading dimensions ld_mu, ld_lv (elements, >= F): the two halves of ONE [N, 2 F] encoder output are
 *                passed as they are (ld = 2 F, the second base F floats on).  16-byte lanes when F % 4 == 0 and every base and
 *                pitch of the call is 16-byte aligned, else one float per access; a lane owns four columns (two words) either way
 *   n_total    : the node count the mean runs over: N, or n_src + n_dst when the call is one table of a pair
 *   key, tick, table : the rule's arguments; tick a device int64* or NULL
 *   flags      : NPI_GAUSS_SAMPLE (write z), NPI_GAUSS_KL (write kl), or both
 *   lv = min(logvar, max_logvar);   z = fmaf(eps, expf(0.5f * lv), mu)   [N, F], ld_z
 *   kl [1]     : -0.5 / n_total * sum over all elements of (1 + lv - mu^2 - exp(lv)).  A DETERMINISTIC sum (npi_pair_score's scheme):
 *                f32 terms, one fp64 partial per tile of NPI_GAUSS_TILE element slots -- the groups of four columns (the last of a
 *                row padded with zero terms) in row-major order, 1024 groups per tile: a function of N and F alone, not of the
 *                grid, the pitches or the lane width -- then a second one-workgroup launch that adds the partials in a fixed
 *                order.  No float atomics.  Needs `partials`: npi_gauss_workspace_bytes(N, F) bytes, 16-byte aligned, caller-owned
 *   npi_gauss_sample_kl_bwd : regenerates eps;  c = g_kl[0] / n_total (g_kl a DEVICE f32 word);
 *                d_mu = g_z + c mu;   d_logvar = [logvar <= max_logvar] (g_z * 0.5 * eps * sigma - 0.5 * c * (1 - exp(lv))).
 *                A part is present when its flag is set AND its pointer (g_z / g_kl) is not NULL; a missing part contributes 0.
 *                d_mu or d_logvar may be NULL (not wanted), not both
 *   npi_gauss_noise : eps [N, F] itself, for tests and for variants composed from other calls (as npi_gat_dropout_keep for Rule D)
 * f32 only.  Nothing is allocated, nothing read back: the calls may run inside a stream capture.  N == 0 returns NPI_OK without a
 * launch; kl[0], if asked for, is then set to 0 by a hipMemsetAsync on `stream`.  Refused with NPI_ERR_ARG before any launch: N or
 * n_total outside [0, 2^31 - 1), F outside [1, 2^31 - 1), more than 2^31 - 2 tiles, a leading dimension below F, n_total < N, or
 * n_total < 1 with N > 0; unknown or empty flags; table outside {0, 1}; NPI_GAUSS_KL without kl / partials, or partials misaligned
 * or shorter than npi_gauss_workspace_bytes(N, F); NPI_GAUSS_SAMPLE without z; a null table (or both of d_mu, d_logvar null) with
 * N > 0.  npi_gauss_workspace_bytes returns -1 for a bad size.
 *
 * Out of scope: bf16 tables, any distribution other than N(0, 1), antithetic or quasi-random draws, multi-GPU.
 * ------------------------------------------------------------------------------------------ */
#define NPI_GAUSS_SAMPLE 1
#define NPI_GAUSS_KL 2
#define NPI_GAUSS_TILE 4096
int64_t npi_gauss_workspace_bytes(int64_t N, int64_t F);   /* -1: bad size */
int npi_gauss_sample_kl(const float* mu, int64_t ld_mu, const float* logvar, int64_t ld_lv, int64_t N, int64_t F, int64_t n_total,
                        float max_logvar, int64_t key, const int64_t* tick /* device word, or NULL */, int table, int flags, float* z,
                        int64_t ld_z, float* kl /* [1] */, void* partials, int64_t partials_bytes, void* stream);
int npi_gauss_sample_kl_bwd(const float* mu, int64_t ld_mu, const float* logvar, int64_t ld_lv, int64_t N, int64_t F,
                            int64_t n_total, float max_logvar, int64_t key, const int64_t* tick, int table, int flags,
                            const float* g_z, int64_t ld_gz, const float* g_kl /* device f32[1], or NULL */, float* d_mu,
                            int64_t ld_dmu, float* d_logvar, int64_t ld_dlv, void* stream);
int npi_gauss_noise(int64_t N, int64_t F, int64_t key, const int64_t* tick, int table, float* eps, int64_t ld, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ranking metrics: the evaluation half of link prediction.  Replaces what PyG 1.4.2 `GAE.test` and the reference's ROC / PR
 * figures (src/compare_withKmer_noKmer.py:20-54) do on the host through sklearn: `roc_auc_score`, `average_precision_score`,
 * `roc_curve` and `precision_recall_curve` of M scores -- all four are functions of `_binary_clf_curve`, which this entry point
 * computes: one sort (the shared sorter, all 32 key bits), two passes over the sorted stream, one over the curve.
 *
 * RULE R -- the curve and the two areas of M float32 scores with binary labels.
 *   Input.  scores[M] f32 and a label per score, in one of two forms: y[M] int64 with values 0 / 1; or y = NULL and a count n_pos:
 *           score m is a positive exactly when m < n_pos -- the `cat([pos, neg])` layout npi_pair_score takes.
 *   1. Key.   s = score + 0.0f (so -0.0 ranks and reports as +0.0, as in sklearn's numeric comparison); with b = the bits of s,
 *             u = (b & 0x80000000) ? ~b : (b | 0x80000000) is ascending-orderable (npi_topk_select_sorted's transform) and the key
 *             is ~u: an ASCENDING key is a DESCENDING score.  The payload is the label.  +-inf are ordinary scores.  A NaN score
 *             raises NPI_STATUS_BAD_SCORE; a label other than 0 / 1 raises NPI_STATUS_BAD_LABEL and counts as 0.  Neither reads or
 *             writes out of bounds; what the metrics are worth then is undefined.
 *   2. Sort.  The pairs by all 32 key bits.
 *   3. Curve. Position i of the sorted stream ends a tie group iff i == M-1 or key[i] != key[i+1].  TP_i = the positives among
 *             positions 0..i, FP_i = i + 1 - TP_i.  The curve is the G triples (thr_g, TP_g, FP_g) at the group ends, in stream
 *             order, thr_g the score rebuilt from the key: sklearn's `_binary_clf_curve` (thresholds, tps, fps) -- all integers,
 *             thresholds bitwise.
 *   4. Metrics.  With TP_-1 = FP_-1 = 0, P = TP_{G-1}, N = FP_{G-1}:
 *             U2  = sum_g (FP_g - FP_{g-1}) * (TP_g + TP_{g-1})          int64, exact: U2 <= 2 P N < 2^62 for M < 2^31 - 1; it
 *                   equals 2 #{(p, n): s_p > s_n} + #{(p, n): s_p = s_n} over positives p and negatives n
 *             auc = U2 / (2.0 * P * N)                                    double;  P * N == 0: NaN
 *             ap  = sum_g ((TP_g - TP_{g-1}) / P) * (TP_g / (TP_g + FP_g))  every term in double;  P == 0: NaN
 *             The ap sum has a fixed order: a lane adds its (at most four) terms in order, a wavefront its lanes in a fixed tree,
 *             a workgroup of 1,024 curve entries its four wavefronts in order, one final workgroup the partials in a fixed order
 *             (npi_pair_score's scheme).  No float atomics anywhere.
 * The result is a pure function of the MULTISET of (score, label) pairs: the curve exists at group ends only, so the order of
 * labels inside a tie group cannot matter, and a permuted input gives bitwise the same auc, ap and curve.  It does not depend on
 * launch geometry either.
 *
 *   result [2]  : auc, ap (fp64)                         counts [4] : P, N, G, U2 (int64)                    -- both required
 *   thr / tps / fps : the curve, each of capacity M (G entries are written, G <= M; the rest is not touched) -- or all three NULL:
 *                 no curve is written
 *   status      : int32 device word as npi_csr_build_ex's (may be NULL): OR-ed into, never cleared here
 *   workspace   : npi_rank_workspace_bytes(M) bytes, 16-byte aligned, caller-owned (the sorter's buffers, then one int64 and two
 *                 8-byte partials per 1,024 scores)
 * Nothing is allocated, nothing read back: the call may run inside a stream capture.  Refused with NPI_ERR_ARG before any launch:
 * M outside [0, 2^31 - 1); n_pos outside [0, M] when y is NULL (it is ignored otherwise); a null result or counts; a curve given
 * in part; with M > 0 a null scores or workspace, or a workspace misaligned or shorter than npi_rank_workspace_bytes(M).  M == 0
 * launches no kernel: two hipMemsetAsync on `stream` write NaN, NaN (every bit set) and four zero counts.
 * npi_rank_workspace_bytes returns -1 for an M outside [0, 2^31 - 1).
 *
 * Out of scope: sample weights, multiclass / `average=`, `drop_intermediate=True`, `max_fpr`, bf16 / fp64 scores.
 * ------------------------------------------------------------------------------------------ */
#define NPI_STATUS_BAD_SCORE 1024
#define NPI_STATUS_BAD_LABEL 2048
int64_t npi_rank_workspace_bytes(int64_t M);
int npi_rank_metrics(const float* scores, const int64_t* y_or_null, int64_t M, int64_t n_pos, double* result /*[2]: auc, ap*/,
                     int64_t* counts /*[4]: P, N, G, U2*/, float* thr, int32_t* tps, int32_t* fps /*each capacity M, or all three NULL*/,
                     int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Edge splits: one edge list -> a training graph plus held-out positive and negative edges, the first step of a link-prediction
 * run.  Replaces PyG 1.4.2 `torch_geometric.utils.train_test_split_edges` (`row < col`, a host `torch.randperm`, a dense [N, N]
 * mask for the held-out negatives, `to_undirected` through `torch_sparse.coalesce`) and the reference's 5-fold key split
 * (`src/generate_edgelist.py:460-494`; the in-script k-fold of `src/train.py:108-184`).
 *
 * RULE S -- a random order of the kept columns; its contiguous ranges are the parts.  All arithmetic in wrapping uint64; mix64, G,
 * mulhi and key as in Rules P / T / W above.
 *   1. Keep.   Column e of the [2, E] list (src[e], dst[e]; int64) is KEPT when src[e] lies in [0, n_src) and dst[e] in [0, n_dst)
 *              and -- with NPI_SPLIT_UPPER (flag bit 0; one id space) -- src[e] < dst[e] (PyG's `row < col`).  An id out of range is
 *              never dereferenced: the column is dropped and NPI_STATUS_BAD_PAIR_ID is OR-ed into the status word.  K = the number
 *              of kept columns.  Parallel columns are kept as they are (as PyG keeps them).
 *   2. Order.  base = mix64(mix64(mix64(key) + 5 * G))           (5 G: the next free stream after the walks' 3 G / 4 G)
 *              r_e  = mix64(base + G * (e + 1))                  e = the column's index in the INPUT, not after the compaction
 *              The kept columns come out in ascending (r_e, e): out_src[K], out_dst[K], e_id[K] (int64; e_id = the input column,
 *              as the sampler's e_id), info[0] = K.  mix64 is a bijection, so for E < 2^31 no two r_e are equal; for a random key
 *              the order is a uniform random permutation.  A pure function of (key, edge list, flags), independent of launch
 *              geometry, of timing and of how the compaction is done.
 *   3. Parts.  Contiguous ranges of that order: slices, no kernel.  For train / val / test with n_v = floor(val_ratio * K) and
 *              n_t = floor(test_ratio * K): val = [0, n_v), test = [n_v, n_v + n_t), train = the rest (PyG's order).  For k folds,
 *              fold f tests on [floor(f K / k), floor((f + 1) K / k)) and trains on the complement.
 *   4. Held-out negatives, one id space.  Let U be the undirected form (5.) of the WHOLE edge list.  Take Rule P's candidates over U
 *              with no_loops, rewrite every valid candidate (s, d) as (min(s, d), max(s, d)) -- an invalid (-1, -1) stays -- and
 *              keep the first M distinct ones in candidate order (npi_negative_distinct).  U is symmetric, so (s, d) is valid exactly
 *              when (d, s) is, and every unordered non-edge {a, b} has the same probability: a uniform draw without replacement from
 *              the upper-triangle non-edges (PyG's `neg_adj_mask.triu(1)`), which are never materialised.  M is clamped to
 *              N (N - 1) / 2 - #{distinct (a, b) in U with a < b}.  As in Rule P the result does not depend on the window.
 *              Two id spaces: Rule P as it is, over the whole list.
 *   5. Undirected form.  Both orientations of the given columns, coalesced: sorted by (row, col), equal pairs once (PyG's
 *              `to_undirected`).  (v, v) columns stay, once.
 *
 *   npi_split_permute    : Rule S 1-2.  Keep flags, their exclusive scan, a stable partition that puts (low 32 bits of r_e, e) for
 *                          the kept columns in front of one padding pair per dropped column, two stable radix sorts of 32 bits (the
 *                          high half of r_e is recomputed from the carried e between them), one gather.  out_src / out_dst / e_id:
 *                          the caller sizes them with the bound E; K entries are written.  status (int32 device word, may be NULL)
 *                          is OR-ed into, never cleared here.  workspace: npi_split_workspace_bytes(E) bytes, 16-byte aligned.
 *   npi_split_canonical  : Rule S 4, in place over W candidates (npi_negative_candidates' output).
 *   npi_split_undirected : Rule S 5 over one id space [0, N).  out_src / out_dst / e_id: capacity 2 E (int64); info[0] = the number
 *                          of pairs written; e_id = the smallest input column that gives the pair in either orientation.  A column
 *                          with an id out of range is dropped and raises NPI_STATUS_BAD_PAIR_ID.  Both orientations are written as
 *                          int32 pairs and merged by npi_sample_coalesce.  workspace: npi_split_undirected_workspace_bytes(E) bytes,
 *                          16-byte aligned.
 * Nothing is allocated, nothing read back, no state is kept; there is no float anywhere.  Refused with -1 before any launch: a null
 * pointer, a negative size, E (2 E for the undirected form), W or an id bound >= 2^31 - 1 (or an id bound below 1; N >= 2^31 - 2 for
 * the undirected form), an unknown flag, a misaligned or short workspace.  E == 0 returns 0 without a launch and writes
 * info[0] = 0 (a hipMemsetAsync on `stream`); W == 0 returns 0.  The two workspace queries return -1 for a size out of range.
 *
 * Out of scope: stratified or grouped splits, weighted edges carried through the split, splits inside a stream capture (the caller
 * reads K), PyG's or the reference's random bits, `negative_sampling`'s `force_undirected`.
 * ------------------------------------------------------------------------------------------ */
#define NPI_SPLIT_UPPER 1
int64_t npi_split_workspace_bytes(int64_t E);
int npi_split_permute(const int64_t* src, const int64_t* dst, int64_t E, int64_t n_src, int64_t n_dst, int64_t key, int flags,
                      int64_t* out_src, int64_t* out_dst, int64_t* e_id, int32_t* info, int32_t* status, void* workspace,
                      int64_t workspace_bytes, void* stream);
int npi_split_canonical(int32_t* cand_src, int32_t* cand_dst, int64_t W, void* stream);
int64_t npi_split_undirected_workspace_bytes(int64_t E);
int npi_split_undirected(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int64_t* out_src, int64_t* out_dst,
                         int64_t* e_id, int32_t* info, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Top-k link prediction: the last stage of a link-prediction run -- for each query row the k target rows it most likely links to
 * and has no known edge to.  Replaces the dense route of PyG 1.4.2, `InnerProductDecoder.forward_all` (`torch.matmul(z, z.t())`, an
 * [N, N] matrix) followed by a mask and `torch.topk`, and the reference's per-case loops on the host (src/case_study*.py): the
 * scores are formed tile by tile on the matrix cores, masked and reduced to each row's best k on the chip; no score matrix is
 * written.
 *
 * RULE K -- the k best targets of each query, from two f32 tables, a list of query rows, a set of excluded pairs and k.
 *   1. Score.  score(i, j) = the f32 fmaf chain acc = fmaf(z_src[i][c], z_dst[j][c], acc) over c = 0 .. F-1 ascending, from acc =
 *              +0: what v_mfma_f32_32x32x2_f32 computes per output element.  It depends on the two rows alone: not on the tile,
 *              the split or the place in the query list the pair falls into.
 *   2. Candidates of query i: every j in [0, n_dst) except (i, j) in the exclusion set; j == i under NPI_TOPK_NO_LOOPS (one id
 *              space only); and j with a NaN score.  A NaN score of a pair that is not excluded otherwise raises
 *              NPI_STATUS_BAD_SCORE; it is never returned.
 *   3. Order.  Descending score with -0.0 equal to +0.0 -- ascending key of Rule R 1 --, ties by ascending j.  A total order:
 *              the answer is unique and independent of tiling, of the split count and of the order candidates are met in.
 *              +-inf are ordinary scores.
 *   4. Output. Row r of scores / ids holds the first min(k, #candidates) candidates of query rows[r] in that order, the score
 *              rebuilt from the key (-0.0 comes out as +0.0); the remaining slots hold id -1 and score -inf.
 *   5. Bad ids. A query id outside [0, n_src) is never dereferenced: its whole row is -1 / -inf and NPI_STATUS_BAD_SOURCE_ID is
 *              raised.
 *
 *   rows      : int64 [R] query ids into z_src, in any order, repeats allowed; NULL: the rows 0 .. R-1
 *   z_src     : f32 [n_src, F], leading dimension ld_src (elements);  z_dst : f32 [n_dst, F], ld_dst.  They may be the same pointer
 *               (one id space).  16-byte loads when F % 4 == 0 and both bases and pitches are 16-byte aligned, else guarded scalar
 *               loads: any F >= 1 and any pitch >= F
 *   k         : 1 <= k <= NPI_TOPK_MAX
 *   ex_rowptr : int32 [n_src + 1], ex_col : int32: the excluded pairs as a by-source CSR with every row's columns ASCENDING
 *               (npi_csr_build_ex with NPI_CSR_SORT_COLUMNS, no self loops; repeated columns allowed); both NULL: none
 *   flags     : NPI_TOPK_NO_LOOPS or 0
 *   splits    : the targets are cut into this many column ranges, each reduced on its own and merged afterwards, so that few
 *               queries still fill the chip; 0: chosen from R and n_dst alone (nothing is read from the device).  Every value
 *               gives bitwise the same output (more than there are tiles of 128 targets, or than 64, count as that many)
 *   scores    : f32 [R, k];  ids : int64 [R, k]
 *   status    : int32 device word as npi_csr_build_ex's (may be NULL): OR-ed into, never cleared here
 *   workspace : npi_topk_links_workspace_bytes(R, n_dst, k, splits) bytes, 16-byte aligned, caller-owned (k words of 8 bytes per
 *               query row and split)
 * Nothing is allocated, nothing read back: the call may run inside a stream capture.  No float atomics; the only atomic is the
 * status OR.  Refused with NPI_ERR_ARG before any launch: R, n_src or n_dst outside [0, 2^31 - 1), F outside [1, 2^31 - 1), a
 * leading dimension below F, k outside [1, NPI_TOPK_MAX], an unknown flag, NPI_TOPK_NO_LOOPS with n_src != n_dst, only one of
 * ex_rowptr / ex_col, negative splits; with R > 0 a null scores, ids or workspace, a null table that has rows, a workspace
 * misaligned or shorter than the query says.  R == 0 returns NPI_OK without a launch.  npi_topk_links_workspace_bytes returns -1
 * for R or n_dst outside [0, 2^31 - 1), k outside [1, NPI_TOPK_MAX] or negative splits.
 *
 * Out of scope: gradients through the selection, bf16 tables, k > NPI_TOPK_MAX, approximate search, per-pair weights, and a
 * by-target query direction (swap the tables and flip the edge list).
 * ------------------------------------------------------------------------------------------ */
#define NPI_TOPK_MAX 128
#define NPI_TOPK_NO_LOOPS 1
int64_t npi_topk_links_workspace_bytes(int64_t R, int64_t n_dst, int64_t k, int64_t splits);   /* -1: bad size */
int npi_topk_links(const int64_t* rows /* NULL: rows 0..R-1 */, int64_t R,
                   const float* z_src, int64_t ld_src, int64_t n_src,
                   const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F, int64_t k,
                   const int32_t* ex_rowptr, const int32_t* ex_col /* by-source CSR, columns ascending; both NULL: none */,
                   int flags /* NPI_TOPK_NO_LOOPS 1 */, int64_t splits,
                   float* scores, int64_t* ids, void* workspace, int64_t workspace_bytes,
                   int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Filtered link ranks: the ranking evaluation that goes with top-k prediction -- at which position does each held-out true link
 * (s, t) come out among all targets s has no known edge to?  What MRR, Hits@K and mean rank in the filtered setting are made of
 * (the protocol of the knowledge-graph literature and of the later PyG / OGB evaluators).  The dense route is the [N, N] product of
 * `InnerProductDecoder.forward_all`, a mask and a compare-and-sum against the gathered target score; here the scan is
 * npi_topk_links' -- tiles of 64 queries x 128 targets on the matrix cores, known edges masked on the chip -- and what is kept
 * per query is four integer counts.
 *
 * RULE F -- the filtered counts of each query pair, from two f32 tables, Q query pairs (s_q, t_q), a set of excluded pairs and a
 *           no-loops flag.
 *   1. Score and key.  Rule K 1 and Rule K 3: score(i, j) is the ascending f32 fmaf chain the MFMA computes per element, its key
 *              the ascending-orderable key of Rule R 1 (descending score, -0.0 equal to +0.0).  The target's own score
 *              score(s_q, t_q) is computed on the matrix cores by the same chain.
 *   2. Competitors of query q: every j in [0, n_dst) with j != t_q, (s_q, j) not in the exclusion set, j != s_q under
 *              NPI_LINK_RANK_NO_LOOPS, and a non-NaN score.  The target itself is never a competitor and is always ranked, also
 *              when (s_q, t_q) is in the exclusion set or is a loop: a known edge is ranked against the non-edges.
 *   3. Counts. counts[q] = { greater, equal, equal_before, candidates } (int64): the competitors with key < key(t_q); those with
 *              the same key; those of `equal` with j < t_q; all competitors.  scores[q] is the target's score rebuilt from its
 *              key (-0.0 comes out as +0.0).
 *   4. Consistency with Rule K.  greater + equal_before is the 0-based position t_q takes in npi_topk_links' list of s_q when the
 *              pair itself is not excluded.
 *   5. Bad input.  s_q outside [0, n_src) or t_q outside [0, n_dst): nothing is dereferenced, the row is -1, -1, -1, -1 with
 *              score -inf, and NPI_STATUS_BAD_PAIR_ID is raised.  A NaN target score: the same row, NPI_STATUS_BAD_SCORE.  A NaN
 *              competitor score raises NPI_STATUS_BAD_SCORE and is not counted (Rule K 2).
 *   6. The output is independent of `splits`, of the order and repetition of the queries, and of the call, bitwise.
 *
 *   src, dst  : int64 [Q] each: the query pairs, in any order, repeats allowed
 *   z_src, z_dst, ld_src, ld_dst, n_src, n_dst, F, ex_rowptr, ex_col, splits, status : as npi_topk_links takes them (16-byte loads
 *               when F % 4 == 0 and both bases and pitches are 16-byte aligned, else guarded scalar loads: any F >= 1 and any
 *               pitch >= F; the exclusion set a by-source CSR with columns ascending; splits 0: chosen as npi_topk_links chooses)
 *   flags     : NPI_LINK_RANK_NO_LOOPS or 0
 *   counts    : int64 [Q, 4];  scores : f32 [Q]
 *   workspace : npi_link_ranks_workspace_bytes(Q, n_dst, splits) bytes, 16-byte aligned, caller-owned (four int32 partial counts
 *               per query and split, one key per query)
 * Nothing is allocated, nothing read back: the call may run inside a stream capture.  Integer counts: no float atomics, the only
 * atomic is the status OR.  Refused with NPI_ERR_ARG before any launch: Q, n_src or n_dst outside [0, 2^31 - 1), F outside
 * [1, 2^31 - 1), a leading dimension below F, an unknown flag, NPI_LINK_RANK_NO_LOOPS with n_src != n_dst, only one of ex_rowptr /
 * ex_col, negative splits; with Q > 0 a null src, dst, counts, scores or workspace, a null table that has rows, a workspace
 * misaligned or shorter than the query says.  Q == 0 returns NPI_OK without a launch.  npi_link_ranks_workspace_bytes returns -1
 * for Q or n_dst outside [0, 2^31 - 1) or negative splits.
 *
 * Out of scope: the by-target direction (swap the tables and flip the lists), grouping queries by source to share rows, bf16
 * tables, gradients, and sampled-negative ranking (that is npi_rank_metrics / GAE.test).
 * ------------------------------------------------------------------------------------------ */
#define NPI_LINK_RANK_NO_LOOPS 1
int64_t npi_link_ranks_workspace_bytes(int64_t Q, int64_t n_dst, int64_t splits);   /* -1: bad size */
int npi_link_ranks(const int64_t* src, const int64_t* dst, int64_t Q,
                   const float* z_src, int64_t ld_src, int64_t n_src,
                   const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                   const int32_t* ex_rowptr, const int32_t* ex_col /* by-source CSR, columns ascending; both NULL: none */,
                   int flags /* NPI_LINK_RANK_NO_LOOPS 1 */, int64_t splits,
                   int64_t* counts /* [Q, 4] */, float* scores /* [Q] */, void* workspace, int64_t workspace_bytes,
                   int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Listwise link loss: the training objective whose optimum the filtered MRR of npi_link_ranks measures -- for every positive
 * (s, t) the negative log-probability of t under the softmax over EVERY candidate target of s (the "1-N" / full-softmax loss of
 * the knowledge-graph-embedding and recommender literature), where npi_group_score's softmax mode sees K <= 63 sampled
 * corruptions.  The three entry points replace `F.cross_entropy(scale * z_src[src] @ z_dst.t() + mask, t)` over
 * `InnerProductDecoder.forward_all` and its autograd backward: the dense [Q, n_dst] product, a dense additive mask, the
 * probability matrix kept for the backward, and `index_add_` on float atomics.  Here the scan is npi_topk_links' -- tiles of 64
 * queries x 128 targets on the matrix cores, known edges masked on the chip -- and nothing of size Q * n_dst is ever written,
 * forward or backward.
 *
 * RULE L -- lp_q, the loss and the gradients, from two f32 tables, Q query pairs (s_q, t_q), a set of excluded pairs, a no-loops
 *           flag and a finite scale > 0.
 *   1. Score.   x_qj = scale * score(s_q, j) with score the ascending f32 fmaf chain of Rule K 1 -- the bits npi_topk_links and
 *              npi_link_ranks produce for the pair -- and the product with scale ONE f32 multiply.
 *   2. Candidates of query q: j == t_q, OR ((s_q, j) not in the exclusion set AND (j != s_q unless NPI_SOFTMAX_LINK_NO_LOOPS is
 *              clear)).  The true target is always a candidate, also when (s_q, t_q) is itself a known edge (Rule F 2: in
 *              training the positives ARE the known edges); the other known partners of s_q are not in the denominator -- the
 *              filtered softmax, which removes the false negatives.
 *   3. Output.  lp_q = x_{q,t_q} - lse_q, lse_q = log(sum over the candidates j of exp(x_qj)) in the max-shifted form: finite
 *              for any finite scores, and exactly 0 (with exactly zero gradients) when the target is the only candidate.
 *   4. Bad pair. s_q outside [0, n_src) or t_q outside [0, n_dst): nothing is dereferenced, lp_q = 0 (lse_q = 0),
 *              NPI_STATUS_BAD_PAIR_ID is raised, and the pair contributes nothing to any sum or gradient.
 *   5. NaN.     A NaN score among the candidates makes lp_q NaN, as torch.logsumexp would, and raises NPI_STATUS_BAD_SCORE.
 *              The gradients of such a query are unspecified.
 *   6. Loss.    loss = -(sum over the good pairs of lp_q) / Q.  The divisor counts pairs, not good pairs (Rule G: nothing is read
 *              back); Q == 0 gives 0.  The sum is the fp64 scheme of npi_pair_score: one partial per workgroup, one workgroup adds
 *              them in a fixed order.
 *   7. Gradient. With u_q = d L / d lp_q and p_qj = exp(x_qj - lse_q) over the candidates, d L / d x_qj = u_q ([j == t_q] - p_qj):
 *                  dZ_src[i] = scale * sum over q with s_q == i and over the candidates j of u_q ([j == t_q] - p_qj) z_dst[j]
 *                  dZ_dst[j] = scale * sum over q that j is a candidate of, of u_q ([j == t_q] - p_qj) z_src[s_q]
 *              (one id space: both land in the one table).  The entry points compute the DENSE part, -u_q scale p_qj over the
 *              candidates j != t_q; the target's own term u_q scale (1 - exp(lp_q)) per pair is a weighted pair-list sum, which
 *              npi_segsum_ex over the pair list's sides already is (functional._pair_grads).
 *                  npi_softmax_link_bwd_src : dq[q, :] = sum_j w_qj z_dst[j, :], w_qj = -u_q scale p_qj, j ascending; dZ_src is
 *                                             then the segmented sum of dq's rows over the queries of each source
 *                  npi_softmax_link_bwd_dst : dz_dst[j, :] = sum_q w_qj z_src[s_q, :], q ascending
 *   8. Reproducibility, forward.  lp is a pure function of (tables, pair, exclusion set, flags, scale, splits): the same bits run
 *              to run and for any order or repetition of the queries (which lane adds which column depends on the column alone).
 *              Across different `splits` the float sum order changes: equal up to rounding, not bitwise.  Within one call all
 *              queries of one source with the same candidate set share lse bit for bit, so lp orders them as their scores do.
 *   9. Reproducibility, backward.  The same bits run to run for the same arguments: every element is one fmaf chain in ascending
 *              partner order per split, the splits added in ascending order.  No float atomics anywhere.
 *
 *   src, dst  : int64 [Q] each: the query pairs, in any order, repeats allowed
 *   z_src, z_dst, ld_src, ld_dst, n_src, n_dst, F, ex_rowptr, ex_col, status : as npi_link_ranks takes them
 *   flags     : NPI_SOFTMAX_LINK_NO_LOOPS or 0;  scale : finite, > 0
 *   splits    : 0 (chosen as npi_topk_links chooses) or the number of ranges scanned separately: column ranges of z_dst in
 *               npi_softmax_link_fwd / _bwd_src, ranges of the QUERY list in _bwd_dst
 *   lp, lse   : f32 [Q] each (fwd: written; bwd: lse read);  loss : f32 [1] or NULL;  u : f32 [Q], d L / d lp
 *   dq        : f32 [Q, F], contiguous;  dz_dst : f32 [n_dst, F], contiguous.  Both are written, not accumulated into
 *   workspace : npi_softmax_link_workspace_bytes(Q, n_src, n_dst, F, splits) bytes, 16-byte aligned, caller-owned; one size serves
 *               the three calls: (m, s) per query and split, a key per query and the loss partials forward, the F-wide partial rows
 *               of every split backward -- O(S (Q + n_dst) F), nowhere near a score matrix
 * Nothing is allocated, nothing read back: every call may run inside a stream capture.  The only atomic is the status OR.
 * Refused with NPI_ERR_ARG before any launch: Q, n_src or n_dst outside [0, 2^31 - 1), F outside [1, 2^31 - 1), a leading
 * dimension below F, an unknown flag, NPI_SOFTMAX_LINK_NO_LOOPS with n_src != n_dst, only one of ex_rowptr / ex_col, negative
 * splits, a scale that is not positive and finite; with Q > 0 a null list, table that has rows, lp / lse / u / dq / dz_dst or
 * workspace, and a workspace misaligned or shorter than the query says.  Q == 0: NPI_OK without a kernel (loss[0], if given, and
 * dz_dst are set to 0 by hipMemsetAsync).  npi_softmax_link_workspace_bytes returns -1 on a bad size, or when the byte count does not
 * fit an int64 (the calls then refuse too).
 *
 * Out of scope: bf16 tables, grouping the queries by source to share score rows (the obvious next optimisation: the queries of
 * one source share every x_qj), per-target weights or label smoothing, the by-target softmax (swap the tables and flip the
 * lists), decoders other than the inner product, a top-k truncated softmax, gradients through scale.
 * ------------------------------------------------------------------------------------------ */
#define NPI_SOFTMAX_LINK_NO_LOOPS 1
int64_t npi_softmax_link_workspace_bytes(int64_t Q, int64_t n_src, int64_t n_dst, int64_t F, int64_t splits);   /* -1: bad size */
int npi_softmax_link_fwd(const int64_t* src, const int64_t* dst, int64_t Q,
                         const float* z_src, int64_t ld_src, int64_t n_src,
                         const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                         const int32_t* ex_rowptr, const int32_t* ex_col /* by-source CSR, columns ascending; both NULL: none */,
                         int flags /* NPI_SOFTMAX_LINK_NO_LOOPS 1 */, float scale, int64_t splits,
                         float* lp /* [Q] */, float* lse /* [Q] */, float* loss /* [1], may be NULL */,
                         void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);
int npi_softmax_link_bwd_src(const int64_t* src, const int64_t* dst, int64_t Q,
                             const float* z_src, int64_t ld_src, int64_t n_src,
                             const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                             const int32_t* ex_rowptr, const int32_t* ex_col, int flags, float scale, int64_t splits,
                             const float* lse /* [Q] */, const float* u /* [Q] */, float* dq /* [Q, F] */,
                             void* workspace, int64_t workspace_bytes, void* stream);
int npi_softmax_link_bwd_dst(const int64_t* src, const int64_t* dst, int64_t Q,
                             const float* z_src, int64_t ld_src, int64_t n_src,
                             const float* z_dst, int64_t ld_dst, int64_t n_dst, int64_t F,
                             const int32_t* ex_rowptr, const int32_t* ex_col, int flags, float scale, int64_t splits,
                             const float* lse /* [Q] */, const float* u /* [Q] */, float* dz_dst /* [n_dst, F] */,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Max aggregation: the third aggregator of PyG's `MessagePassing` (`add`, `mean`, `max`) -- the pooling aggregator of GraphSAGE.
 * npi_segmax replaces `scatter_('max', x[col], row, dim_size=N)` inside `MessagePassing.propagate(aggr='max')`, npi_segmax_bwd the
 * backward of that composition (`index_add_` on float atomics).  Neither writes the [nnz, F] gather, neither uses a float atomic.
 *
 * RULE X -- out, arg of a CSR side (rowptr, col, eid, rowidx; items of 64 or 256 entries) and an f32 table x [n_cols, F].
 *   1. Value.   out[i, c] = the maximum of x[col[p], c] over the entries p of row i.  -0.0 equals +0.0 in this comparison and a
 *               zero maximum is written as +0.0 (the key of Rule R 1).  A NaN beats every number; what is written is the quiet NaN
 *               0x7fc00000.  +-inf are ordinary values.
 *   2. Winner.  arg[i, c] (int32) = eid of the winning entry: the column of edge_index it came from, or -1 for the self loop the
 *               CSR build appends (eid < 0).  Among equal values -- all NaNs count as equal -- the smallest uint32(eid) wins, so
 *               the appended loop loses every tie.
 *   3. Empty.   A row without entries: out = +0.0 (PyG's fill of scatter_('max')), arg = -2.
 *   4. Padding. Entries at positions >= rowptr[N] (up to nnz_max) are never read.
 * In numpy, per row i and column c (key() = the ascending-orderable uint32 of a float32 with NaN -> 0x7fc00000, -0.0 -> +0.0):
 *     p    = np.arange(rowptr[i], rowptr[i + 1]);  e = np.where(eid[p] < 0, -1, eid[p])
 *     word = (key(x[col[p], c]).astype(np.uint64) << 32) | (~e.astype(np.uint32)).astype(np.uint64)
 *     w    = word.argmax();  out[i, c] = value_of_key(word[w] >> 32);  arg[i, c] = e[w]          # len(p) == 0: +0.0, -2
 * Consequence: out and arg are a pure function of (x, the edge list, self_loops).  The maximum is exact and the tie rule does not
 * look at the entry order, so both are bitwise the same for either item size, for NPI_CSR_SORT_COLUMNS on or off and for any
 * order of merging partial rows.
 *
 * Backward (the by-SOURCE side of the same edge list; only eid links the two sides, no transpose map):
 *     dX[j, c] = sum of dOut[col[q], c] over the entries q of row j whose eid[q] (a loop entry: -1) equals arg[col[q], c]
 * a gather-form sum in a fixed order: ascending entry order inside an item; a row cut by item boundaries adds its parts as
 * tail[i] + head[i + 1] + ... ascending when it has at most 4 heads, and a longer chain (a hub row) as
 * tail[i] + s_0 + s_1 + ... + s_15 with s_w = head[i + 1 + w] + head[i + 1 + w + 16] + ... ascending.  Bitwise reproducible for a
 * given side; it gathers a dOut row AND an arg row per entry: the price of having no atomics.
 *
 *   rowptr .. rowidx : one side as npi_csr_build_ex wrote it, item_edges the item size it was built with (64 or 256)
 *   N, n_cols        : rows of the side (= rows of out / dX) and rows of the gathered table (x / dOut and arg)
 *   x, out, arg, dout, dx : unit column stride, leading dimensions (elements) >= F.  16-byte lanes when F > 64, F % 4 == 0 and every
 *                      base and pitch of the call is 16-byte aligned, one float per lane otherwise: any F >= 1, any pitch >= F
 *   workspace        : npi_segmax_workspace_bytes(nnz_max, item_edges, F) bytes, 16-byte aligned, caller-owned: the head / tail
 *                      partial rows of every item ((value, eid) pairs forward, sums backward) and the tails' rows.  Needs no clearing
 * Nothing is allocated, nothing read back: both calls may run inside a stream capture.  Refused with NPI_ERR_ARG before any
 * launch: N, n_cols or nnz_max outside [0, 2^31 - 1), F <= 0, a leading dimension below F, item_edges other than 64 / 256; with N > 0 a
 * null rowptr, col, eid, rowidx, table or output, and with nnz_max > 0 as well a workspace that is null, misaligned or shorter
 * than the query says.  N == 0 returns NPI_OK without a launch; nnz_max == 0 launches the empty-row fill alone.
 * npi_segmax_workspace_bytes returns -1 for a bad size or item size.
 *
 * Out of scope: bf16 storage, weighted messages, 'add' / 'min' (npi_segsum_ex is 'add'), two-part tables, hub streaming.
 * ------------------------------------------------------------------------------------------ */
int64_t npi_segmax_workspace_bytes(int64_t nnz_max, int64_t item_edges, int64_t F);   /* -1: bad size */
int npi_segmax(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t item_edges,
               int64_t N, int64_t n_cols, int64_t nnz_max, const float* x, int64_t ldx, int64_t F,
               float* out, int64_t ldo, int32_t* arg, int64_t lda, void* workspace, int64_t workspace_bytes, void* stream);
int npi_segmax_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* rowidx, int64_t item_edges,
                   int64_t N /* sources: rows of dx */, int64_t n_cols /* targets: rows of dout and arg */, int64_t nnz_max,
                   const float* dout, int64_t ldd, const int32_t* arg, int64_t lda, int64_t F,
                   float* dx, int64_t ldx, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-graph readouts: the rest of PyG 1.4.2's `nn.glob` next to npi_readout_max_mean -- `global_add_pool`, `global_sort_pool`
 * (DGCNN's SortPooling, the readout of SEAL) and the softmax + weighted sum of `GlobalAttention`, forward and backward.  None of them
 * builds a [B, n_max, F] dense batch or an [N] alpha array, none uses a float atomic.
 *
 * graph_ptr [B + 1] (int32, non-decreasing) are the segment starts: graph g owns rows [graph_ptr[g], graph_ptr[g + 1]), n_g of them.
 *
 * RULE O -- out of an f32 table x [N, F] and graph_ptr.
 *   O-add.   out[g, c] = sum of x[i, c] over the rows of g; an empty graph gives 0.
 *            Backward: dx[i] = dout[g(i)]; rows outside [graph_ptr[0], graph_ptr[B]) are written as zeros (no fill launch).
 *   O-sort.  key_i = x[i, F - 1], every NaN written as 0x7fc00000 (npi_sort_pool_keys).  The rows of a graph are ordered by key
 *            descending in the bit order of npi_topk_select: NaN above +inf, +0.0 above -0.0, equal bits by ascending row index --
 *            TopKPooling's order, taken with ratio = 1.0 (ceil(1.0f n) = n exactly below 2^24 rows per graph).
 *            out[g, r F : (r + 1) F] = x[row of rank r in g] for r < min(k, n_g), zeros for n_g <= r < k; out is [B, k F] and rows
 *            are copied bit for bit.  DEVIATION from PyG: PyG fills the dense batch with x.min() - 1 and afterwards zeroes EVERY
 *            cell that equals that value; here only the padding is zero.
 *            Backward: dx[i] = dout[g, r F : (r + 1) F] if row i has rank r < k, else zeros; every row of dx is written, each from
 *            at most one slot.  No gradient flows through the order.
 *   O-att.   gate [N] f32.  PyG's softmax(gate, batch): m_g = max gate_i, e_i = exp(gate_i - m_g), s_g = sum e_i,
 *            alpha_i = e_i / (s_g + 1e-16);  out[g] = sum alpha_i x_i; an empty graph gives zeros (m_g = s_g = 0).
 *            Backward, with c_g = <dout_g, out_g> from the SAVED out:  dx_i = alpha_i dout_g,  dgate_i = alpha_i (<dout_g, x_i> - c_g).
 *            The forward keeps m [B], s [B] and out [B, F] per graph; alpha is recomputed from them, never stored.
 *   Order.   The sums of O-add and O-att are taken in an order that is a function of n_g alone.  With C = NPI_READOUT_CHUNK, chunk q of
 *            a graph is its rows [q C, min(n_g, (q + 1) C)) (counted from the graph's first row); inside a chunk, lane l of 16 adds
 *            the rows l, l + 16, ... ascending from 0.0f; the chunk's partial is lane 0 + lane 1 + ... + lane 15 ascending; the
 *            graph's sum is partial 0 + partial 1 + ... ascending.  O-att computes a chunk relative to the chunk's own maximum m_q
 *            (terms fma(exp(gate_i - m_q), x[i, c], .), s_q the same sum of the exps) and merges with the online-softmax rescale:
 *            m = max m_q, s = sum s_q exp(m_q - m), acc = sum acc_q exp(m_q - m) ascending (fma), out = acc / (s + 1e-16); a graph
 *            of one chunk is acc_0 / (s_0 + 1e-16).
 * In numpy, per graph with rows r = x[b:e] (float32 arithmetic throughout; g8 = gate[b:e]):
 *     lanes = lambda v: reduce(add, [reduce(add, v[l::16], float32(0)) for l in range(16)])   # v: the chunk's terms, [n, F] or [n]
 *     add   = reduce(add, [lanes(r[q:q + C]) for q in range(0, e - b, C)])                     # e == b: zeros
 *     order = sorted(range(b, e), key=lambda i: (-bits(key_i), i))                             # bits(): ascending-orderable uint32
 *     m_q, e_q = g8[q:q + C].max(), exp(g8[q:q + C] - m_q);  s_q, acc_q = lanes(e_q), lanes(e_q[:, None] * r[q:q + C])
 *     m = max(m_q);  out = sum_q(acc_q * exp(m_q - m)) / (sum_q(s_q * exp(m_q - m)) + 1e-16)
 * Consequences: the bits of out[g] depend only on the rows of graph g -- not on B, on where the graph sits in the batch, on the
 * pitch or alignment of x (columns always travel in groups of 4 columns per thread; only the load width changes), or on the launch
 * geometry.  The backward of O-att sums its two dot products with lane l owning columns 4 l .. 4 l + 3 (+ 256 j) and the 64 lanes
 * added by an xor butterfly: a function of F alone.  No float atomics anywhere.
 *
 *   x, out, dout, dx : unit column stride, a pitch (elements) >= F each (out / dout of the sort pool: >= k F).  Rows are read and
 *                      written 16 / 8 / 4 bytes per lane: the widest that F, every pitch and every base pointer of the call allow
 *   workspace        : npi_readout_{add,attention}_workspace_bytes(N, B, F) bytes, 16-byte aligned, caller-owned; needs no clearing.
 *                      It holds the chunk scan and the partials of the N / C + B workgroups (a bound known on the host)
 *   order, remap     : perm and remap of npi_topk_select / npi_topk_select_sorted run on the keys with ratio 1.0 (out_ptr is then
 *                      graph_ptr, which must start at 0): order[graph_ptr[g] + r] = the row of rank r, remap[i] = graph_ptr[g] + rank
 * Nothing is allocated, nothing read back: every call may run inside a stream capture.  Refused with NPI_ERR_ARG before any launch,
 * the text of npi_last_error() starting with the entry point's name: N or B outside [0, 2^31 - 1), F <= 0, k <= 0, a pitch below
 * F (k F), a negative workspace length; with N > 0 and B > 0 also a null pointer and a workspace that is misaligned or shorter than
 * the query says.  N == 0 or B == 0 returns NPI_OK without a launch (the caller zero-fills what it wants to read).  The workspace
 * queries return -1 for a bad size.
 *
 * Out of scope: Set2Set, bf16 storage, SortPooling's 1-D conv head, `min_score` / SAGPooling, gradients through the sort.
 * ------------------------------------------------------------------------------------------ */
#define NPI_READOUT_CHUNK 1024
int64_t npi_readout_add_workspace_bytes(int64_t N, int64_t B, int64_t F);         /* -1: bad size */
int npi_readout_add(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t N, int64_t B, int64_t F,
                    float* out /* [B, F] */, int64_t ldo, void* workspace, int64_t workspace_bytes, void* stream);
int npi_readout_add_bwd(const float* dout, int64_t ldd, const int32_t* graph_ptr, int64_t N, int64_t B, int64_t F,
                        float* dx /* [N, F] */, int64_t lddx, void* stream);
int64_t npi_readout_attention_workspace_bytes(int64_t N, int64_t B, int64_t F);   /* -1: bad size */
int npi_readout_attention(const float* gate, const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t N, int64_t B, int64_t F,
                          float* out /* [B, F] */, int64_t ldo, float* m /* [B] */, float* s /* [B] */,
                          void* workspace, int64_t workspace_bytes, void* stream);
int npi_readout_attention_bwd(const float* gate, const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t N, int64_t B,
                              int64_t F, const float* out, int64_t ldo, const float* m, const float* s,
                              const float* dout, int64_t ldd, float* dx /* [N, F] */, int64_t lddx, float* dgate /* [N] */,
                              void* stream);
int npi_sort_pool_keys(const float* x, int64_t ldx, int64_t N, int64_t F, float* keys /* [N] */, void* stream);
int npi_sort_pool_gather(const float* x, int64_t ldx, const int32_t* order, const int32_t* graph_ptr, int64_t N, int64_t B,
                         int64_t F, int64_t k, float* out /* [B, k F] */, int64_t ldo, void* stream);
int npi_sort_pool_bwd(const float* dout, int64_t ldd, const int32_t* remap, const int32_t* graph_ptr, int64_t N, int64_t B,
                      int64_t F, int64_t k, float* dx /* [N, F] */, int64_t lddx, void* stream);

/* Evaluation loop(reference src/methods.py:87-105 compares one element per Python
 * iteration, one device sync each).  counts[4] += [TP, FN, TN, FP] for pred = first arg-max of scores[i, 0..C):
 * pred 1 & y 1 -> TP, pred 1 & y 0 -> FP, pred 0 & y 1 -> FN, anything else -> TN (the reference's else
 * branch).  counts is device memory, accumulated across calls; no synchronisation. */
int npi_confusion_update(const float* scores, int64_t lds, int64_t C, const int64_t* y, int64_t B, int64_t* counts,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * The readout sum and MLP head of Net_1 (reference src/classes.py:74-80):
 *     x = x1 + x2 + x3; relu(lin1) -> dropout -> relu(lin2) -> lin3 -> log_softmax
 * as one forward and two backward launches (a 200-row batch: every library GEMM / element-wise kernel of the head is
 * launch-latency bound).  Weights in torch.nn.Linear layout W [out, in], 16-byte aligned; D0 <= 1024, D1, D2 <= 256 (all
 * multiples of 4), D3 <= 32.  r2 / r3 may be NULL (fewer readouts).  mask [B, D1] holds 0 / 1 (NULL: evaluation), scale =
 * 1 / (1 - p).  Saved for the backward (may be NULL in evaluation): s = the summed input [B, D0], h1 = relu(lin1) before
 * dropout [B, D1], h2 [B, D2].  npi_mlp_head_bwd: ds (may be NULL) is the gradient of EACH readout; dW* / db* are written,
 * not accumulated; every sum over the batch runs in row order (deterministic).
 * activation: what follows lin3 -- NPI_HEAD_LOG_SOFTMAX (Net_1) or NPI_HEAD_SIGMOID (the one-output variant,
 * src/train_with_twoDataset_modelOnlyOneOutput.py:45-82: lin3 is 64 -> 1, `torch.sigmoid`, trained with binary cross entropy);
 * `logp` / `dlogp` are then the sigmoid's output and its gradient.
 * ------------------------------------------------------------------------------------------ */
#define NPI_HEAD_LOG_SOFTMAX 0
#define NPI_HEAD_SIGMOID 1
int npi_mlp_head_fwd(const float* r1, int64_t ld1, const float* r2, int64_t ld2, const float* r3, int64_t ld3,
                     int64_t B, int64_t D0, const float* W1, const float* b1, int64_t D1, const float* W2, const float* b2,
                     int64_t D2, const float* W3, const float* b3, int64_t D3, const float* mask, float scale, int activation,
                     float* s, float* h1, float* h2, float* logp, void* stream);
int64_t npi_mlp_head_workspace_elems(int64_t B, int64_t D1, int64_t D2, int64_t D3);
int npi_mlp_head_bwd(int64_t B, int64_t D0, int64_t D1, int64_t D2, int64_t D3, const float* W1, const float* W2,
                     const float* W3, const float* mask, float scale, int activation, const float* s, const float* h1, const float* h2,
                     const float* logp, const float* dlogp, float* ds, float* dW1, float* db1, float* dW2, float* db2,
                     float* dW3, float* db3, float* workspace, int64_t workspace_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NPI_GNN_H */
