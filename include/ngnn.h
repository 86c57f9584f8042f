/*
 * ngnn.h — C ABI of the MI355X-native GraphSAGE / GCN aggregation path.
 *
 * The reference (hhilsber/noise-GNN) is pure Python: its hot path is
 * SAGE.forward -> PyG SAGEConv.forward (src/models/layers/sage.py:30-40,
 * conv call at :34) and SimpleGCN.forward -> PyG GCNConv.forward
 * (src/models/layers/convolution.py:29-35, call at :31).  PyG 2.5.1 [ext]
 * implements each conv as index_select (gather) + scatter_add_/scatter_reduce_
 * (scatter) + Linear.  The reference has no FFI of its own; the entry points
 * below are what a ctypes binding of those PyG internals would bind, and are
 * what noise-gnn_amd/ngnn/_lib.py binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless stated; the caller owns every
 *     buffer (PyTorch caching-allocator tensors).  The library never
 *     allocates, frees or retains pointers beyond the call.
 *   - Every call is asynchronous and stream-ordered on `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream).
 *   - Return 0 on success, a negative NGNN_E_* for argument errors (nothing
 *     is launched), or a positive hipError_t from a failed launch.
 *   - Index arrays are int32 internally (N, E < 2^31), rows of feature
 *     matrices are addressed with an explicit leading dimension (elements).
 *   - No global mutable state: re-entrant, safe from any host thread.
 */
#ifndef NGNN_H
#define NGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGNN_ABI_VERSION 22

/* error codes (negative); positive values are hipError_t */
#define NGNN_OK 0
#define NGNN_E_ARG (-1)        /* null pointer / negative size / bad enum   */
#define NGNN_E_DTYPE (-2)      /* unsupported dtype                          */
#define NGNN_E_SHAPE (-3)      /* F / leading dimension / size out of range  */
#define NGNN_E_ALIGN (-4)      /* pointer alignment not supported            */
#define NGNN_E_RANGE (-5)      /* N or E does not fit int32                  */
#define NGNN_E_WORKSPACE (-6)  /* workspace too small                        */

/* reductions: PyG `aggr` names (utils/scatter.py [ext]) */
#define NGNN_REDUCE_SUM 0  /* GCNConv aggr='add'                             */
#define NGNN_REDUCE_MEAN 1 /* SAGEConv default aggr='mean' (sage.py:16-19)   */
#define NGNN_REDUCE_MAX 2  /* SAGEConv(aggr='max'): build extension          */
/* math-mode flag OR-ed into ngnn_sage_fwd_raw's `reduce`: the root term
 * x . W_r^T on exact fp32 MFMA (v_mfma_f32_16x16x4_f32, a fmaf chain) instead
 * of the default fp32-accurate 3 x bf16 split. */
#define NGNN_MATH_EXACT_F32 0x100
/* flag OR-ed into ngnn_sage_fwd_raw's `reduce` (MEAN / SUM, no ReLU, no
 * dropout, agg_out == NULL: an output layer): aggregate the neighbour term in
 * the F_out-wide space -- z = x W_l^T for every row in the same launch as the
 * root term (ws holds z: n_rows x ceil16(F_out) floats), then out[d] +=
 * mean/sum_{j -> d} z[j] for the rows below n_edge_rows.  Equal to
 * W_l . mean(x_j) up to fp32 rounding (the aggregation is linear); the
 * K-wide gather becomes an F_out-wide one.  Other cases run the fused path. */
#define NGNN_FWD_NARROW 0x200
/* flag OR-ed into ngnn_sage_fwd_raw's `reduce`: x (and x_dev's rows) are
 * bf16 [*, ldx] (ldx in elements, a multiple of 4; 16-B aligned base).  The
 * rows are read as bf16 -- half the bytes of the fp32 layout -- and widened
 * exactly: the split-bf16 root term needs one part (3 products), the gather
 * sums in fp32.  Outputs (unless NGNN_OUT_BF16), z and agg_out stay fp32.  Not
 * with NGNN_MATH_EXACT_F32 (NGNN_E_SHAPE: convert x and call again). */
#define NGNN_X_BF16 0x400
/* flag OR-ed into ngnn_sage_fwd_raw's `reduce`: the weights (W_r, and W_l of
 * NGNN_FWD_NARROW) hold bf16-exact values -- a bf16 model's parameters
 * (sage.py:40 under model.to(torch.bfloat16)) widened to fp32.  The split-bf16
 * root term then needs ONE weight part (its other two parts are zero): the
 * LDS image is a third of the size (wider column slices, fewer re-reads of x)
 * and each 32-deep chunk issues 3 MFMAs (1 with NGNN_X_BF16) instead of 6.
 * The result is bitwise the one without the flag on such weights (the
 * skipped products are exact zeros); weights that are not bf16-exact are
 * rounded to bf16.  MEAN / SUM only (NGNN_E_SHAPE otherwise: call without). */
#define NGNN_W_BF16 0x800
/* flag OR-ed into ngnn_sage_fwd_raw's `reduce`: `ws` already holds
 * ngnn_pack_weight(wl) (a producer packed this step's W_l: the graph slot's
 * load, ngnn_slot_load's pack job), so a layer whose W_l streams from L2
 * issues no pack launch of its own; ignored when W_l is staged in LDS. */
#define NGNN_WL_PREPACKED 0x1000
/* flag OR-ed into ngnn_sage_fwd_raw's `reduce`: `out` holds bf16 [n_rows,
 * ldo] (ldo in elements, a multiple of 4; 8-B aligned), each output rounded to
 * nearest even after bias, ReLU and dropout -- a bf16 model's hidden
 * activations, which the reference's bf16 layer stores in bf16 too.  Whole
 * 16-column output tiles only; not with NGNN_FWD_NARROW or the wide path
 * (NGNN_E_SHAPE: call without and convert). */
#define NGNN_OUT_BF16 0x2000

/* dtypes */
#define NGNN_F32 0
#define NGNN_BF16 1

int ngnn_abi_version(void);
const char *ngnn_strerror(int rc);

/* ------------------------------------------------------------------ edges
 * Validate a PyG edge_index [2,E] int64 (row 0 = source, row 1 = target,
 * flow source_to_target) before any kernel indexes with it.
 * status (device int32[4], caller zeroes it):
 *   [0] != 0  some source id outside [0, n_src)
 *   [1] != 0  some target id outside [0, n_dst)
 *   [2] != 0  targets are NOT non-decreasing (needs the sorting CSR path)
 *   [3] != 0  sources are NOT non-decreasing
 * Replaces PyG's implicit index checks in index_select / scatter [ext]
 * (reached from sage.py:34 / convolution.py:31). */
int ngnn_edge_probe(const int64_t *edge_index, int64_t E, int64_t n_src, int64_t n_dst,
                    int32_t *status, void *stream);

/* Workspace bytes ngnn_csr_build needs for the unsorted path. */
size_t ngnn_csr_workspace_bytes(int64_t E, int64_t n_rows);

/* Group the E edges by `keys` (int64, values in [0,n_rows)) into CSR:
 *   rowptr[n_rows+1] (int32), col[E] = vals in grouped order (int32),
 *   eid[E] = original edge position (int32, nullable).
 * Grouping is STABLE (edge order kept inside a row), so per-row reductions
 * run in the same order as PyG's CPU scatter_add_ / index_add_.
 * keys_sorted=1 claims keys are non-decreasing (fast path, no workspace);
 * keys_sorted=0 uses a stable radix sort in `ws`.
 * Forward CSR: keys = edge_index[1] (targets), vals = edge_index[0].
 * Transposed CSR for the backward gather: keys = edge_index[0], vals = edge_index[1]. */
int ngnn_csr_build(const int64_t *keys, const int64_t *vals, int64_t E, int64_t n_rows,
                   int keys_sorted, int32_t *rowptr, int32_t *col, int32_t *eid,
                   void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------ aggregation
 * out[i, :F] = reduce_{e in rowptr[i]..rowptr[i+1]} x[col[e], :F]
 * SUM : edge-order fp32 sum; MEAN: sum / max(deg,1) (IEEE division);
 * MAX : NaN-propagating max, empty rows -> 0 (scatter_reduce amax,
 *       include_self=False on a zero tensor).
 * Replaces PyG MessagePassing.propagate (gather x_j + utils.scatter) [ext].
 * dtype NGNN_BF16: x holds bf16 rows (F, ldx multiples of 4; 8-B aligned),
 * widened exactly; out stays fp32. */
int ngnn_seg_agg_fwd(const void *x, int64_t ldx, int64_t F, const int32_t *rowptr,
                     const int32_t *col, int64_t n_dst, int reduce, int dtype,
                     void *out, int64_t ldo, void *stream);

/* grad_x[j, :F] = sum over edges e with source j (transposed CSR, edge
 * order) of  SUM : g[dst_e]   MEAN: g[dst_e] / max(deg(dst_e),1)
 *            MAX : [x[j]==agg[dst_e]] * g[dst_e] / ties(dst_e)
 * where ties = #tied sources + [agg == 0] (torch scatter_reduce amax
 * backward, FunctionsManual.cpp [ext]).  grad_x is fully overwritten
 * (rows with no out-edges get 0).  For MAX, `ws` must hold n_dst*F floats
 * (ngnn_seg_agg_bwd_workspace_bytes) and x/agg/rowptr/col (forward CSR)
 * are required; for SUM/MEAN they may be NULL except rowptr (degrees). */
size_t ngnn_seg_agg_bwd_workspace_bytes(int64_t n_dst, int64_t F, int reduce);
int ngnn_seg_agg_bwd(const void *grad_out, int64_t ldg, int64_t F,
                     const int32_t *rowptr, const int32_t *col, int64_t n_dst,
                     const int32_t *rowptr_t, const int32_t *col_t, int64_t n_src,
                     int reduce, int dtype, const void *x, int64_t ldx,
                     const void *agg, int64_t lda, void *grad_x, int64_t ldgx,
                     void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------- sampling
 * One hop of uniform neighbour sampling without replacement (PyG
 * NeighborLoader / pyg-lib neighbor_sample semantics [ext], constructed at
 * pipeline.py:75-83): for frontier node v (global id) with in-degree d,
 * take min(d, fanout) distinct in-neighbours from graph CSR
 * (g_rowptr int64[N+1], g_col int32[nnz]) in Floyd order.
 *   out_nbr[i*fanout + k] = global neighbour id (or -1 past the count),
 *   out_cnt[i]            = number taken.
 * Deterministic in (seed, frontier position). */
int ngnn_sample_hop(const int64_t *g_rowptr, const int32_t *g_col, const int64_t *frontier,
                    int64_t n_frontier, int fanout, uint64_t seed, int64_t *out_nbr,
                    int32_t *out_cnt, void *stream);

/* ------------------------------------------------- whole-block sampling
 * The whole NeighborLoader mini-batch on the device: every hop of
 * ngnn_sample_hop's sampler (hop h uses seed*1000003 + h), the relabelling
 * of sampled global ids to block-local ids and the block's edge list --
 * what PyG's NeighborLoader (pipeline.py:75-83, pyg-lib neighbor_sample
 * [ext]) builds in its worker process plus the batch.to(device) of
 * pipeline.py:153.  Local ids: seeds first (seeds must be distinct), then
 * each hop's newly reached nodes in order of first appearance in the hop's
 * (frontier position, draw) sequence.  Edges: row 0 = local source (the
 * sampled neighbour), row 1 = local target, grouped by target in frontier
 * order (targets non-decreasing).
 *
 * Two calls.  ngnn_sample_block runs the hops and writes
 * counts (device int32[4]) = {n_nodes, n_edges, n_active, 0}, n_active =
 * rows that received in-edges (the frontiers of hops < last); the caller
 * reads them (one device->host copy), allocates the outputs and calls
 * ngnn_sample_block_finish with the same fanouts / seeds count / workspace,
 * which writes n_id int64[n_nodes], edge_index int64[2, n_edges]
 * (contiguous), optionally y = y_all[n_id] and x = x_all[n_id] (fp32 rows),
 * and restores node_map.
 *   node_map: int32[2 * n_graph], caller-owned, all -1 before the first call
 *             and again after every finish (one map per stream at a time).
 *   ws:       ngnn_sample_block_workspace_bytes(batch, fanouts, n_hops);
 *             holds the block between the two calls.
 *   fanouts:  HOST int32[n_hops], each 0..64.
 * ABI 18: n_active (counts[2]) and, nullable as a pair, csr_rowptr
 * int32[n_nodes + 1] / csr_col int32[n_edges]: the block's target-grouped
 * CSR (edge order kept inside a row; col = the local sources), taken from the
 * relabelling itself, so a consumer of the block builds none.  The hops run
 * as three launches each (one lane per draw: draws + claims; first-
 * appearance counts; the relabelling writes) and the outputs, x rows
 * included, as one.
 * ABI 19: counts_dev (nullable): the counts array ngnn_sample_block wrote,
 * read on the DEVICE -- no host read-back: n_nodes / n_edges / n_active are
 * then the capacities the outputs are sized for (the plan's n_cap / e_cap
 * at most) and bound the device counts; the first counts[0] rows / counts[1]
 * edges are written.  edge_index's row stride is n_edges in both modes (the
 * capacity here).  With ngnn_slot_load's counts_dev this is NeighborLoader's
 * sync-free pipeline (no host wait per batch). */
size_t ngnn_sample_block_workspace_bytes(int64_t batch, const int32_t *fanouts, int n_hops);
int ngnn_sample_block(const int64_t *g_rowptr, const int32_t *g_col, int64_t n_graph,
                      const int64_t *seeds, int64_t n_seeds, const int32_t *fanouts, int n_hops,
                      uint64_t seed, int32_t *node_map, void *ws, size_t ws_bytes,
                      int32_t *counts, void *stream);
int ngnn_sample_block_finish(const int32_t *fanouts, int n_hops, int64_t n_seeds,
                             int64_t n_nodes, int64_t n_edges, int32_t *node_map,
                             int64_t n_graph, const void *ws, size_t ws_bytes, int64_t *n_id,
                             int64_t *edge_index, const int64_t *y_all, int64_t *y,
                             const float *x_all, int64_t ldx, int64_t F, float *x, int64_t ldo,
                             int64_t n_active, int32_t *csr_rowptr, int32_t *csr_col,
                             const int32_t *counts_dev, void *stream);

/* ------------------------------------------- block-free layer-wise inference
 * ABI 22.  SAGE.inference / SimpleGCN.inference (sage.py:42-58,
 * convolution.py:37-53; called per epoch by test_ogb, pipeline.py:291) run
 * each layer over every node: per loader batch the conv on a whole multi-hop
 * block, of which only the seed rows are kept.  A seed row receives in-edges
 * from hop 0 alone (a later hop's frontier is the newly reached nodes), and
 * hop 0's draws depend only on (block seed, position in the batch, degree) --
 * so the kept rows need no block.  Both entries address a run of LOADER
 * POSITIONS p = r0 .. r0 + n_rows - 1 of a pass whose batches hold batch_size
 * seeds (r0 a multiple of batch_size: NGNN_E_ARG otherwise):
 *   batch b = p / batch_size, position i = p % batch_size,
 *   block seed S_b = seed0 + b * seed_stride (uint64 wrap-around), hop seed
 *   S_b * 1000003 + 0 (ngnn_sample_block's hop 0),
 *   node v = seeds ? seeds[p] : p   (seeds: int64, indexed by p; nullable),
 *   draws = ngnn_sample_hop's for (deg(v), fanout, hop seed, i): min(deg,
 *   fanout) distinct in-neighbours of the graph CSR (g_rowptr int64[N + 1],
 *   g_col int32) in Floyd order; deg <= fanout keeps every neighbour in CSR
 *   order, multi-edges included -- bitwise the in-edges NeighborLoader's block
 *   gives seed row i of batch b.
 * fanout > 64: NGNN_E_SHAPE; a negative size: NGNN_E_ARG; n_rows * fanout >=
 * 2^31: NGNN_E_RANGE -- nothing is launched.
 *
 * ngnn_infer_draw: the draws as a target-grouped CSR, rowptr int32[n_rows + 1]
 * and col int32[rowptr[n_rows]] (the caller sizes col for n_rows * fanout):
 * col holds GLOBAL node ids in draw order inside a row -- the col_x (with
 * xrow = the positions' nodes) of ngnn_sage_fwd_raw's fused gather, which then
 * reads the previous layer's table in place: no x[n_id] copy, no relabelling.
 * Three launches (counts + tile scan, tile offsets, one lane group per row
 * drawing).  ws: ngnn_infer_draw_workspace_bytes(n_rows), 4-B aligned.
 *
 * ngnn_infer_narrow: a narrowing layer's rows with the draws made in the
 * kernel (no CSR materialised), the neighbour term reduced F_out wide:
 *   out[r, c] = act(root[r, c] + red_j z[nbr_j(r), c] + bias[c]),  c < Fo,
 *   r < n_rows (row r = position r0 + r), red = MEAN (0 for an empty row) or
 *   SUM (NGNN_REDUCE_*; MAX is not linear: NGNN_E_ARG), act = ReLU if relu.
 * z [N, ldz] = x W_l^T for EVERY node (fp32, 16-B aligned, ldz a multiple of
 * 4 and >= ceil4(Fo)); root [n_rows, ld_root] (same layout rules; row r of the
 * chunk) = x W_r^T (+ b) of the positions' nodes, NULL for GCNConv (no root
 * term); bias nullable (NULL when root already carries it).  out [n_rows,
 * ldo]: the caller's row pointer and stride (the next table at the chunk's
 * row offset).  Equal to the K-wide aggregate followed by W_l up to fp32
 * rounding (NGNN_FWD_NARROW's identity).  Plain vector stores only.
 * Replaces, for whole-graph evaluation, NeighborLoader's block + x[n_id] +
 * PyG SAGEConv / GCNConv forward [ext] + the [:batch_size] slice. */
size_t ngnn_infer_draw_workspace_bytes(int64_t n_rows);
int ngnn_infer_draw(const int64_t *g_rowptr, const int32_t *g_col, const int64_t *seeds, int64_t r0,
                    int64_t n_rows, int64_t batch_size, int fanout, uint64_t seed0,
                    uint64_t seed_stride, int32_t *rowptr, int32_t *col, void *ws, size_t ws_bytes,
                    void *stream);
int ngnn_infer_narrow(const int64_t *g_rowptr, const int32_t *g_col, const int64_t *seeds, int64_t r0,
                      int64_t n_rows, int64_t batch_size, int fanout, uint64_t seed0,
                      uint64_t seed_stride, const float *z, int64_t ldz, const float *root,
                      int64_t ld_root, const float *bias, int64_t Fo, int reduce, int relu, float *out,
                      int64_t ldo, void *stream);

/* ------------------------------------------------------ co-teaching loss
 * CTLoss.forward (src/utils/losses.py:19-49) without its two host argsorts:
 * for models m = 1, 2 with logits y_m [B, C] (row stride ld_m) and noisy
 * labels y_noise int64[B]:
 *   l_m[r]       = cross_entropy(y_m[r], y_noise[r])  (0 if ignore_index)
 *   ind_m_sorted = argsort(l_m) ascending, ties by row index, NaN last
 *                  (np.argsort(loss_m) of losses.py:22,26)
 *   out[0] = mean_{r in ind_2_sorted[:R]} l_1[r]   (loss_1_update, :44)
 *   out[1] = mean_{r in ind_1_sorted[:R]} l_2[r]   (loss_2_update, :45)
 *   out[2] = sum noise_or_not[ind[ind_1_sorted[:R]]] / R  (pure_ratio_1, :33)
 *   out[3] = same for model 2 (NaN when noise_or_not is NULL)
 * with R = num_remember (losses.py:31), ind = the batch's n_id (NULL = row
 * ids), noise_or_not bool (uint8) [n_noise]; an index outside it sets *err
 * (device int, caller-zeroed) and contributes nothing.  B <= 8192.
 * ngnn_ct_loss_bwd: d y_m = grad_m / #valid (softmax - onehot) on the rows
 * the other model kept, 0 on every other row of [0, B) -- the autograd of
 * out[m-1]; model = 0 or 1.  ws: ngnn_ct_loss_workspace_bytes(B), kept
 * between the forward and both backwards. */
size_t ngnn_ct_loss_workspace_bytes(int64_t B);
int ngnn_ct_loss_fwd(const float *y1, int64_t ld1, const float *y2, int64_t ld2, int64_t B,
                     int64_t C, const int64_t *y_noise, int64_t ignore_index, int64_t num_remember,
                     const int64_t *ind, const uint8_t *noise_or_not, int64_t n_noise, float *out,
                     int64_t *ind1_sorted, int64_t *ind2_sorted, void *ws, size_t ws_bytes,
                     int *err, void *stream);
int ngnn_ct_loss_bwd(int model, const float *y, int64_t ld, int64_t B, int64_t C,
                     const int64_t *y_noise, int64_t ignore_index, const void *ws,
                     const float *grad, float *dy, int64_t ldd, void *stream);

/* ------------------------------------------------------- fused SAGE layer
 * One SAGEConv layer of SAGE.forward (sage.py:33-39) in one launch:
 *   out[r] = act( b + x[r] . W_r^T + [deg(r)>0] agg(r) . W_l^T ),   r < n_rows
 * agg(r) = reduce over the CSR row r of x (MEAN / SUM / MAX as in
 * ngnn_seg_agg_fwd, bit-identical); act = optional ReLU then optional
 * dropout with keep probability 1-p_drop and scale 1/(1-p_drop), drawn from a
 * counter-based hash of (seed, r, c) (no mask tensor; backward uses out > 0).
 * A dropped element is +0.0 whatever its pre-activation (NaN and inf too);
 * p_drop = 1 gives all +0.0.  Non-finite pre-activations otherwise: without
 * ReLU a kept NaN stays NaN; ReLU passes NaN like torch.relu (y < 0 ? 0 : y)
 * in every form but one -- the row-tile kernel's p_drop = 0.5 form
 * (ngnn_sage_fwd_raw; one keep bit per element) takes ReLU as an integer
 * max with 0 on the doubled value, so there a kept NaN with the sign bit set
 * becomes +0.0 and only a positive-signed NaN passes.
 * W_l / W_r are the PyG Linear weights [Fo, K] packed by ngnn_pack_weight;
 * wl_packed may be NULL (no neighbour term; rowptr/col may then be NULL).
 * bias may be NULL.  x, out fp32 (outputs wider than 512 columns run as
 * several launches of 512-column slices); exact fp32 MFMA
 * (v_mfma_f32_16x16x4_f32).  Optional modes:
 *   n_rows_dev  device int: rows = min(n_rows, *n_rows_dev) (rows past it are
 *               not written) -- bounds that only the device knows;
 *   agg_out     [n_rows, ld_agg]: workgroups whose 64 rows have in-edges also
 *               store those rows' aggregate (saved for the backward);
 *   xmask       stage x * (xmask > 0 ? xscale : 0) instead of x (ReLU/dropout
 *               backward fused into a dgrad GEMM's input);
 *   seed_dev    device uint64 XORed into `seed` when the kernel starts, so a
 *               captured HIP graph draws a fresh dropout mask per replay (the
 *               graph increments it); NULL = the host seed alone.
 * Replaces PyG SAGEConv.forward [ext] + relu + F.dropout. */
size_t ngnn_pack_weight_bytes(int64_t Fo, int64_t K);
int ngnn_pack_weight(const float *w, int64_t ldw, int64_t Fo, int64_t K, void *packed,
                     void *stream);
/* Pack M[Fo][K] = rows [0,rows0) from w0, rows [rows0,Fo) from w1 (either
 * read transposed: M[n][k] = src[k][n]).  The backward packs
 * [W_l^T ; W_r^T] for its dgrad GEMM. */
int ngnn_pack_weight_ex(const float *w0, const float *w1, int64_t ldw, int64_t rows0, int64_t Fo,
                        int64_t K, int transposed, void *packed, void *stream);
int ngnn_sage_fwd(const float *x, int64_t ldx, int64_t K, int64_t n_rows,
                  const int32_t *n_rows_dev, const int32_t *rowptr, const int32_t *col, int reduce,
                  const void *wl_packed, const void *wr_packed, const float *bias, int64_t Fo,
                  float *out, int64_t ldo, int relu, float p_drop, uint64_t seed,
                  const uint64_t *seed_dev, float *agg_out, int64_t ld_agg, const float *xmask,
                  int64_t ldm, float xscale, void *stream);

/* Same layer with the RAW PyG Linear weights (W_l, W_r: [Fo, K] row-major,
 * row stride ldw) through the row-tile kernel (ngnn_sage_rt.hip, the model's
 * path).  Root term x . W_r^T: by default fp32-accurate 3 x bf16 split MFMA
 * (each operand split v = v1 + v2 + v3 in bf16, the six products down to
 * 2^-18 of the leading one accumulated in fp32; error below the fp32
 * rounding of the reference GEMM); `reduce | NGNN_MATH_EXACT_F32` runs it on
 * exact fp32 MFMA.  The W_r image is built in LDS from these rows in the
 * kernel prologue (no pack launch); W_l (fp32, neighbour term of rows with
 * in-edges) shares the LDS when it fits, else it is packed into ws (one
 * launch) and streamed from L2.  Returns NGNN_E_SHAPE, launching nothing,
 * for shapes outside that kernel's envelope (K % 4 != 0, unaligned rows, W_r
 * slice too large for LDS, buffers >= 2 GiB): the caller then packs and calls
 * ngnn_sage_fwd.  x_dev (nullable): a device word holding x's address, read
 * at run time instead of x (a HIP-graph slot whose batch stays where the
 * loader put it; 16-B aligned, row stride ldx, rows < *n_rows_dev).
 * xrow / xrow_dev (nullable; the device word overrides): the fused
 * NeighborLoader feature gather -- logical row r of the layer input is row
 * xrow[r] (int64, the block's n_id) of x, the HBM-resident feature table of
 * x_rows rows (< 3.75 GiB), so x[n_id] is never materialised (pipeline.py:153
 * copies it per batch).  Root rows and gathered neighbour rows both go
 * through it; outputs and agg_out stay in block order.  col_x (nullable,
 * with xrow): col with every entry already mapped through xrow (the slot
 * load writes it), so the neighbour gather makes no dependent index load.
 * wr == NULL: no root term (GCNConv's form, see ngnn_gcn_agg_fwd; raw
 * weights only, not with NGNN_FWD_NARROW).
 * n_edge_rows / n_edge_rows_dev (device int, nullable, min'd with the
 * host value): rows at or past it have no in-edges (NGNN_FWD_NARROW's
 * gather stops there, and the row-tile kernel runs the tiles past it on its
 * root-term-only loop; NeighborLoader numbers the rows that receive edges
 * first).  Pass n_rows when unknown.
 * Wide layers (ngnn_sage_wide_preferred: K % 4 != 0, or F_out needing more
 * than four LDS column slices -- Amazon-Computers' 767 -> 512 layer) with
 * plain fp32 rows run as an aggregate launch over rows < n_edge_rows (into
 * agg_out, else ws) + a 2-D tiled exact-fp32 MFMA dual GEMM (ngnn_wide.hip).
 * ws: ngnn_sage_fwd_raw_workspace_bytes(K, Fo, n_rows) bytes (calls sharing
 * a ws must be stream-ordered); its last 160 KiB hold the launch's prebuilt
 * split-bf16 root image (k_x3_image) when the rest still fits the z rows /
 * packed W_l -- a smaller ws makes every workgroup build the image itself. */
size_t ngnn_sage_fwd_raw_workspace_bytes(int64_t K, int64_t Fo, int64_t n_rows);
/* 1 when ngnn_sage_fwd_raw runs a [K -> Fo] layer on the wide path (exact:
 * the NGNN_MATH_EXACT_F32 mode), else 0. */
int ngnn_sage_wide_preferred(int64_t K, int64_t Fo, int exact);
/* The output columns per launch ("column slice") of the row-tile kernel for a
 * [K -> Fo] ngnn_sage_fwd_raw call with a root term, or 0 when the call
 * leaves that kernel (the wide path is preferred, K % 4 != 0, no slice fits
 * the LDS, or the flags exclude it).  flags: the call's `reduce` argument --
 * NGNN_REDUCE_* with NGNN_MATH_EXACT_F32 / NGNN_W_BF16 / NGNN_X_BF16 /
 * NGNN_OUT_BF16 / NGNN_FWD_NARROW OR-ed in (NGNN_FWD_NARROW: the answer for a
 * call that meets narrow mode's other conditions, then Fo itself).  A layer
 * runs as ceil(Fo / slice) launches, slice s with its first column at
 * s * slice; a slice is a multiple of 16 columns, so (slice >> 4) odd means
 * every second launch starts mid-way through a 32-column dropout hash word.
 * A pure function of its arguments (no device call; the same envelope code
 * the forward runs).  A bad reduce or a non-positive size: NGNN_E_ARG; K or
 * Fo >= 2^31: NGNN_E_RANGE.  Added within ABI 22. */
int64_t ngnn_sage_fwd_slice_cols(int64_t K, int64_t Fo, int flags);
int ngnn_sage_fwd_raw(const float *x, const float *const *x_dev, const int64_t *xrow,
                      const int64_t *const *xrow_dev, int64_t x_rows, int64_t ldx, int64_t K,
                      int64_t n_rows, const int32_t *n_rows_dev, int64_t n_edge_rows,
                      const int32_t *n_edge_rows_dev, const int32_t *rowptr,
                      const int32_t *col, const int32_t *col_x,
                      int reduce, const float *wl, const float *wr, int64_t ldw, const float *bias,
                      int64_t Fo, float *out, int64_t ldo, int relu, float p_drop, uint64_t seed,
                      const uint64_t *seed_dev, float *agg_out, int64_t ld_agg, void *ws,
                      size_t ws_bytes, void *stream);

/* Two-layer SAGE forward of the headline shape in three launches
 * (ngnn_fwd2.hip): sage.py:33-39 for
 * SAGE(K0, 256, F1, num_layers=2) -- conv0 -> relu -> dropout -> conv1 --
 * replacing two ngnn_sage_fwd_raw calls (the second with NGNN_FWD_NARROW).
 * Shape envelope (ngnn_sage2_supported): 96 < K0 <= 128, K0 % 4 == 0, hidden
 * H == 256, 32 < F1 <= 48, reduce MEAN or SUM.  Weights are the raw PyG
 * Linear matrices (lin_l / lin_r of each conv, rows of ldw0 / ldw1 floats).
 *   h   [n_rows, ldh]  = dropout(relu(b0 + x W_r0^T + agg(x) W_l0^T)); only
 *        rows < min(h_rows, *h_rows_dev) are written (the rows a bounded
 *        backward reads: pass n_rows to write all);
 *   agg0 [n_rows, ld_agg] = the layer-0 neighbour aggregate of the rows of
 *        the 16-row tiles below n_edge_rows (the backward's saved aggregate;
 *        bit-identical to ngnn_seg_agg_fwd);
 *   out [n_rows, F1]   = b1 + h W_r1^T + agg(h) W_l1^T (logits, every row;
 *        rows packed: ldo == F1, out 16-B aligned -- a 16-row tile of out is
 *        one contiguous block, stored as 16-B pieces).
 * Rows at or past min(n_edge_rows, *n_edge_rows_dev) must have no in-edges
 * (NeighborLoader numbers the rows that receive edges first; pass n_rows
 * when unknown).  x_dev (nullable): device word holding x's address (graph
 * slot), x then unused.  xrow / xrow_dev / x_rows / col_x: the fused
 * x[n_id] gather, as ngnn_sage_fwd_raw's (x is the x_rows-row feature table,
 * col_x = n_id[col]).  wr0 (nullable, ABI 17): no layer-0 root term --
 * SimpleGCN's GCNConv(normalize=False), aggregate first: x is then read
 * only through the neighbour aggregate (not with xrow / xrow_dev); pass a
 * zero W_r1 for its output layer.  Arithmetic: H2 (two fp16 parts per operand after
 * power-of-two scaling, three MFMA products), inside the fp32 parity bars.
 * stages: NGNN_SAGE2_ALL, or a subset in order (per-launch timing; the
 * workspace carries nb and z between stages): EDGE the aggregate + nb of
 * the rows with in-edges, MAIN every row's layer 0 + layer-1 products,
 * NARROW the z aggregate into out; PREP is accepted and does nothing (the
 * kernels load their weight slices themselves).
 * head (nullable, ABI 15): the seed-row cross entropy of the training step
 * (pipeline.py:158, F.cross_entropy(out[:B], y[:B]) -- ngnn_seed_xent_fwd_grad's
 * contract) computed by the NARROW launch from the logits it finishes, plus
 * the first step of the backward (see ngnn_xent_head).
 * ws: ngnn_sage2_workspace_bytes(K0, F1, n_rows), 256-B aligned. */
/* The loss head of ngnn_sage2_fwd (ABI 15).  For the logit rows d < B:
 *   loss   = sum_{d < B, y[d] != ignore_index} (lse(out[d]) - out[d][y[d]]) / count
 *   count  = #{d < B : y[d] != ignore_index}   (an out-of-range label: NaN loss)
 *   dy[d]  = (softmax(out[d]) - onehot(y[d])) / count   (0 for an ignored row)
 *            -- d loss / d out at unit scale, rows >= B not written;
 *   g[s]  += dy[d] (/ deg(d) for MEAN) for every edge s -> d, d < B (float
 *            atomics; exact zeros skipped): the narrow scatter ngnn_sage2_bwd
 *            runs first, already done -- pass g as its g_pre.  g [n_rows rows,
 *            C4 = ceil4(F1) floats]: its rows < min(g_rows, *g_rows_dev) are
 *            zeroed by the EDGE launch of the same call (so a head whose
 *            backward never runs leaves nothing behind); nullable (no scatter).
 * ws: ngnn_xent_head_workspace_bytes(B) bytes, 16-B aligned, zero-filled
 * before its first use (it is zero again on return).  The loss sum is in a
 * fixed order (deterministic); needs the EDGE and NARROW stages in one call
 * or in order, F1 <= 64.
 * src_count (nullable, ABI 17): 2 g_rows + 1 int32, zero-filled before its
 * first use and then owned by the head: the EDGE launch counts every source's
 * edges into rows d < B (two count arrays alternating per call, the word past
 * them selects one), so a source with a single such edge takes ONE plain row
 * store of dy[d] (/ deg(d)) instead of F1 float atomics.  Counts left over
 * from a call whose NARROW stage did not finish only ever over-count (the
 * scatter then stays atomic): any call order is safe. */
typedef struct ngnn_xent_head {
    const int64_t *y;
    int64_t B;
    int64_t ignore_index;
    float *loss, *count;
    float *dy;
    int64_t ldd;
    float *g;
    int64_t g_rows;
    const int32_t *g_rows_dev;
    void *ws;
    size_t ws_bytes;
    int32_t *src_count;
} ngnn_xent_head;
size_t ngnn_xent_head_workspace_bytes(int64_t B);
#define NGNN_SAGE2_PREP 1
#define NGNN_SAGE2_EDGE 2
#define NGNN_SAGE2_MAIN 4
#define NGNN_SAGE2_NARROW 8
#define NGNN_SAGE2_ALL 15
int ngnn_sage2_supported(int64_t K0, int64_t H, int64_t F1, int reduce);
size_t ngnn_sage2_workspace_bytes(int64_t K0, int64_t F1, int64_t n_rows);
int ngnn_sage2_fwd(const float *x, const float *const *x_dev, const int64_t *xrow,
                   const int64_t *const *xrow_dev, int64_t x_rows, int64_t ldx, int64_t K0,
                   int64_t n_rows, const int32_t *n_rows_dev, int64_t n_edge_rows,
                   const int32_t *n_edge_rows_dev, const int32_t *rowptr, const int32_t *col,
                   const int32_t *col_x, int reduce, const float *wl0, const float *bl0, const float *wr0,
                   int64_t ldw0, int64_t H, const float *wl1, const float *bl1,
                   const float *wr1, int64_t ldw1, int64_t F1, float p_drop, uint64_t seed,
                   const uint64_t *seed_dev, float *h, int64_t ldh, int64_t h_rows,
                   const int32_t *h_rows_dev, float *agg0, int64_t ld_agg, float *out,
                   int64_t ldo, const ngnn_xent_head *head, int stages, void *ws, size_t ws_bytes,
                   void *stream);

/* Every weight gradient of the two-layer stack above in three launches
 * (ngnn_bwd2.hip): the backward of sage.py:33-39 under
 * loss.backward() when the loss reads logit rows < *r_ptr (the seed rows,
 * pipeline.py:155-160), replacing ngnn_seg_agg_fwd + two ngnn_sage_wgrad +
 * ngnn_sage_dgrad_lowdim.  With g[s] = sum over edges s -> d (d < R) of
 * dy[d] (/ deg(d) for MEAN), over rows < R' = max(R, *rnext_ptr):
 *   dW_l1 = g^T h, dW_r1 = dy^T h, db1 = sum dy            ([F1, 256], [F1])
 *   dz0 = (dy W_r1 + g W_l1) * [h > 0] * yscale            (on chip only)
 *   dW_l0 = dz0^T agg0, dW_r0 = dz0^T x, db0 = sum dz0     ([256, K0], [256])
 * dy [*, ldy] (rows < R read), h [*, ldh] / agg0 [*, ld_agg] the forward's
 * (rows < R' read; an edgeless row's aggregate counts as 0), x / x_dev /
 * xrow / xrow_dev / x_rows as ngnn_sage2_fwd's (row r of layer 0's input).
 * Arithmetic (round 5): H2 -- two fp16 parts per operand after a
 * power-of-two scaling per 32-row chunk, three MFMA products per product
 * (relative ~2^-22), fp32 accumulation -- inside the fp32 weight-gradient
 * bars (1e-5 of each tensor's max).  F1 <= 48, 0 < K0 <= 128, K0 % 4 == 0; weights [F1, 256] rows of
 * ldw1 floats.  ws: ngnn_sage2_bwd_workspace_bytes(n_rows, K0, F1), 256-B
 * aligned, ZERO-FILLED before its first use (g's part is zero again on
 * return; its offset depends on K0 and F1 only, so a zeroed workspace may be
 * grown for more rows).  Float atomics
 * build g: not bitwise reproducible run to run (as the reference's CUDA
 * index_add_).  g_pre (nullable, ABI 15): g already built (ngnn_sage2_fwd's
 * loss head, [n_rows, ceil4(F1)]): no scatter launch, g read from it.
 * adam (nullable, ABI 15): the optimizer step folded into the reduction --
 * every parameter updated from its gradient as ngnn_adam_step would (same
 * arithmetic, the same device step count advanced once); the gradients are
 * still written.  For a training step whose gradients need no exchange
 * (one rank) and whose optimizer holds exactly these six tensors. */
typedef struct ngnn_adam_fold {
    /* in the order dW_l1, db1, dW_r1, dW_l0, db0, dW_r0 (the gradient order) */
    float *param[6], *exp_avg[6], *exp_avg_sq[6];
    float *step; /* the device step count (advanced once, then read) */
    float lr, beta1, beta2, eps, weight_decay;
    /* ABI 20 (nullable): ngnn_slot_load's contract gate and the slot's r_next
     * word -- a step whose block broke the slot's contract updates no
     * parameter and leaves the step count (the gradients are still written) */
    const uint64_t *gate;
    const int64_t *gate_gen;
} ngnn_adam_fold;
size_t ngnn_sage2_bwd_workspace_bytes(int64_t n_rows, int64_t K0, int64_t F1);
int ngnn_sage2_bwd(const float *dy, int64_t ldy, int64_t F1, const float *wl1, const float *wr1,
                   int64_t ldw1, const float *h, int64_t ldh, float yscale, const float *x,
                   const float *const *x_dev, const int64_t *xrow, const int64_t *const *xrow_dev,
                   int64_t x_rows, int64_t ldx, int64_t K0, const float *agg0, int64_t ld_agg,
                   const int32_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *r_ptr,
                   const int32_t *rnext_ptr, int reduce, float *dwl1, float *dbl1, float *dwr1,
                   float *dwl0, float *dbl0, float *dwr0, const float *g_pre, const ngnn_adam_fold *adam,
                   void *ws, size_t ws_bytes, void *stream);

/* GCNConv(normalize=False) layer (convolution.py:19-35; PyG GCNConv [ext]):
 * out = act(A (x W^T) + b), A the target-grouped sum over in-edges.  The
 * fused path runs it as SAGE with W_r = 0 (linear aggregation: A x W^T ==
 * (A x) W^T up to fp32 rounding): aggregate-first through
 * ngnn_sage_fwd_raw(wr = NULL, wl = W, reduce = SUM) when F_in <= F_out,
 * else transform-first: z = x W^T through ngnn_sage_fwd_raw(wl = NULL, wr =
 * W, bias = NULL) into z [n_rows, ldz], then this launch:
 *   out[d] = act(sum_{e into d, edge order} z[col[e]] + b)   for every row
 *   d < min(n_rows, *n_rows_dev) (act = ReLU + quad-hash dropout as the
 *   row-tile epilogue; rows without in-edges get act(b)).
 * ldz >= ceil4(Fo), z 16-B aligned. */
int ngnn_gcn_agg_fwd(const float *z, int64_t ldz, int64_t Fo, const int32_t *rowptr,
                     const int32_t *col, int64_t n_rows, const int32_t *n_rows_dev,
                     const float *bias, int relu, float p_drop, uint64_t seed,
                     const uint64_t *seed_dev, float *out, int64_t ldo, void *stream);

/* ------------------------------------------ backward receptive-field bounds
 * ngnn_row_extent: out[0] = max(out[0], 1 + last row of g[n_rows, F] holding a
 * nonzero (or NaN)).  The reference's loss reads only the seed rows
 * (pipeline.py:155 slices [:batch_size]), so the output gradient is zero past
 * them and every backward product can stop at that row.
 * ngnn_block_prefix_stats: R = *r_ptr (device);  *r_next = max(*r_next, R,
 * 1 + max col[0..rowptr[R]))  = rows of the input gradient that can be
 * nonzero;  *nnz_out = rowptr[R] (nullable).  E bounds the sweep. */
int ngnn_row_extent(const float *g, int64_t ld, int64_t n_rows, int64_t F, int32_t *out,
                    void *stream);
int ngnn_block_prefix_stats(const int32_t *rowptr, const int32_t *col, const int32_t *r_ptr,
                            int32_t *nnz_out, int32_t *r_next, int64_t E, void *stream);

/* ------------------------------------------------- fused SAGE layer backward
 * Weight gradients over rows r < R = *r_ptr (device):
 *   dz = dy (* [y > 0] * yscale when y != NULL: ReLU+dropout backward)
 *   dW_r = dz^T h,  dW_l = dz^T agg (agg: the forward's saved aggregate; rows
 *   with no in-edges read as 0),  db = sum_r dz.
 * fp32 MFMA over 64-row chunks, per-slice partials in ws, fixed-order
 * reduction => deterministic.  Outputs are overwritten.
 * Replaces autograd of lin_l / lin_r (PyG Linear [ext]) in SAGEConv. */
size_t ngnn_sage_wgrad_workspace_bytes(int64_t Fo, int64_t K);
/* h_dev (nullable): device word holding h's address, read at run time (as
 * ngnn_sage_fwd_raw's x_dev). */
/* h_idx / h_idx_dev (nullable; the device word overrides): row r of h is
 * row h_idx[r] of h, a table of h_rows rows (< 2 GiB) -- layer 0 under the
 * fused x[n_id] gather (see ngnn_sage_fwd_raw's xrow).  bf16_flags: bit 0
 * (NGNN_WG_H_BF16) h holds bf16 (a bf16 model's layer input, as
 * ngnn_sage_fwd_raw's NGNN_X_BF16; K and ldh multiples of 4); bit 1
 * (NGNN_WG_Y_BF16) the mask rows y hold bf16 (a bf16 model's hidden
 * activations, NGNN_OUT_BF16); both widened exactly when staged. */
#define NGNN_WG_H_BF16 1
#define NGNN_WG_Y_BF16 2
int ngnn_sage_wgrad(const float *dy, int64_t ldy, const float *y, int64_t ldyy, float yscale,
                    const float *h, const float *const *h_dev, const int64_t *h_idx,
                    const int64_t *const *h_idx_dev, int64_t h_rows, int bf16_flags, int64_t ldh,
                    const float *agg, int64_t ld_agg, const int32_t *rowptr, int64_t n_rows,
                    const int32_t *r_ptr,
                    int64_t Fo, int64_t K, float *dwl, float *dbl, float *dwr, void *ws,
                    size_t ws_bytes, void *stream);
/* Input gradient of one layer, rows j < Rn = *rnext_ptr (R = *r_ptr):
 *   dh[j] = [j < R] droot[j] + sum over edges e with source j and target
 *           d = col_t[e] < R (transposed CSR, edge order) of
 *           MEAN: dagg[d] / deg(d)   SUM: dagg[d]
 *           MAX : [h[j] == agg[d]] * dagg[d] / ties(d)   (torch amax rule)
 * droot = dz W_r and dagg = dz W_l come from the dgrad GEMM (ngnn_sage_fwd
 * with packed [W_l^T ; W_r^T]).  Rows >= Rn are zeroed if zero_tail, else
 * left untouched.  MAX needs ws of n_rows*K floats
 * (ngnn_sage_dgrad_workspace_bytes).  Replaces autograd of index_select +
 * scatter (PyG propagate [ext]). */
size_t ngnn_sage_dgrad_workspace_bytes(int64_t n_rows, int64_t K, int reduce);
int ngnn_sage_dgrad_gather(const float *dagg, int64_t ld_dagg, const float *droot,
                           int64_t ld_droot, const int32_t *rowptr, const int32_t *col,
                           const int32_t *rowptr_t, const int32_t *col_t, int64_t n_rows,
                           const int32_t *r_ptr, const int32_t *rnext_ptr, int64_t K, int reduce,
                           const float *h, int64_t ldh, const float *agg, int64_t ld_agg,
                           float *dh, int64_t ldd, int zero_tail, void *ws, size_t ws_bytes,
                           void *stream);
/* Same result through float atomics instead of the source-grouped CSR (no
 * per-batch sort): dh[j] = [j < R] droot[j] for j < Rn, then every edge
 * (j -> d), d < R, adds its term into dh[j] (one 256-B atomic wave-instruction
 * per edge and 64 columns).  Summation order is not fixed (as with the
 * reference's CUDA index_add_); the gather variant is the deterministic one.
 * rowptr/col: target-grouped CSR. */
int ngnn_sage_dgrad_scatter(const float *dagg, int64_t ld_dagg, const float *droot,
                            int64_t ld_droot, const int32_t *rowptr, const int32_t *col,
                            int64_t n_rows, const int32_t *r_ptr, const int32_t *rnext_ptr,
                            int64_t K, int reduce, const float *h, int64_t ldh, const float *agg,
                            int64_t ld_agg, float *dh, int64_t ldd, int zero_tail, void *stream);
/* The whole atomic input-gradient path of one layer in two launches, no dgrad
 * GEMM: zero dh rows < Rn, then one wave per target row d < R computes
 * dz[d] = dy[d] (* [y>0] * yscale), dz[d] W_r (atomically into dh[d]) and
 * dz[d] W_l (scaled as in ngnn_sage_dgrad_gather, atomically into every
 * in-neighbour's row).  wl / wr: the raw PyG weights [Fo, K].  Fo <= 512. */
int ngnn_sage_dgrad_fused(const float *dy, int64_t ldy, const float *y, int64_t ldyy,
                          float yscale, const float *wl, const float *wr, int64_t Fo, int64_t K,
                          const int32_t *rowptr, const int32_t *col, int64_t n_rows,
                          const int32_t *r_ptr, const int32_t *rnext_ptr, int reduce,
                          const float *h, int64_t ldh, const float *agg, int64_t ld_agg,
                          float *dh, int64_t ldd, int zero_tail, void *stream);

/* Input gradient for MEAN / SUM when Fo < K, aggregating in the narrow
 * space (the aggregation is linear):
 *   g[j]  = sum over edges (j -> d), d < R, of dz[d] (MEAN: / deg(d))
 *           (Fo-wide float atomics; dz = dy (* [y > 0] * yscale))
 *   dh[j] = [j < R] dz[j] W_r + g[j] W_l   for j < Rn    (one MFMA pass)
 * = ngnn_sage_dgrad_fused's result up to fp32 summation order, with Fo/K of
 * its atomics and no zero-fill of dh.  wl / wr: raw PyG weights [Fo, K],
 * row stride ldw.  ws: ngnn_sage_dgrad_lowdim_workspace_bytes(n_rows, Fo, K)
 * bytes, 16-B aligned, ZERO-FILLED before its first use and dedicated to one
 * (Fo, K) pair: [packed W image | g], g = [n_rows][Fo rounded up to 4]
 * floats; every call leaves g zero again.  Rows >= Rn of dh are zeroed if zero_tail, else untouched.
 * NGNN_E_SHAPE when the weight image does not fit the LDS budget
 * (ngnn_sage_dgrad_route sends no such shape here).  Replaces autograd of lin_l + propagate
 * (sage.py:34, PyG SAGEConv [ext]). */
size_t ngnn_sage_dgrad_lowdim_workspace_bytes(int64_t n_rows, int64_t Fo, int64_t K);
int ngnn_sage_dgrad_lowdim(const float *dy, int64_t ldy, const float *y, int64_t ldyy,
                           float yscale, const float *wl, const float *wr, int64_t ldw, int64_t Fo,
                           int64_t K, const int32_t *rowptr, const int32_t *col, int64_t n_rows,
                           const int32_t *r_ptr, const int32_t *rnext_ptr, int reduce, float *dh,
                           int64_t ldd, int zero_tail, void *ws, size_t ws_bytes, void *stream);
/* Which of the input-gradient entries above a [Fo, K] layer's backward
 * takes (added within ABI 22) -- a pure function of its arguments, no
 * device call; the entries' own shape checks use the same predicates:
 *   deterministic != 0                          NGNN_DGRAD_GEMM_GATHER
 *   else Fo < K, SUM / MEAN, and a shape ngnn_sage_dgrad_lowdim does not
 *     answer NGNN_E_SHAPE to                    NGNN_DGRAD_LOWDIM
 *   else Fo <= 512 and both weights fit ngnn_sage_dgrad_fused's LDS
 *     (8 Fo K + 8 KiB <= 150 KiB)               NGNN_DGRAD_FUSED
 *   else                                        NGNN_DGRAD_GEMM_SCATTER
 * The two GEMM routes: the dgrad GEMM (ngnn_sage_fwd_raw with packed
 * [W_l^T ; W_r^T]), then ngnn_sage_dgrad_scatter / _gather.  Fo or K <= 0,
 * or a reduce outside NGNN_REDUCE_*: NGNN_E_ARG; K >= 2^31: NGNN_E_RANGE. */
#define NGNN_DGRAD_LOWDIM 0
#define NGNN_DGRAD_FUSED 1
#define NGNN_DGRAD_GEMM_SCATTER 2
#define NGNN_DGRAD_GEMM_GATHER 3
int ngnn_sage_dgrad_route(int64_t Fo, int64_t K, int reduce, int deterministic);

/* ------------------------------------------------------ seed-row loss
 * Mean cross entropy of the first B rows of logits [*, C] (row stride ld)
 * against labels y[0..B), rows whose label == ignore_index excluded (torch
 * reduction='mean' semantics):  loss = sum (lse(x_r) - x_r[y_r]) / count.
 * Writes *loss and *count (device floats).  Deterministic.  The backward
 * writes dlogits rows < B = g (softmax(x_r) - onehot(y_r)) / count with
 * g = *grad_scale (0 for ignored rows) and leaves rows >= B untouched.
 * Replaces F.cross_entropy(out[:batch_size], y[:batch_size]) in the
 * reference's training loop (pipeline.py:158) and its autograd. */
size_t ngnn_seed_xent_workspace_bytes(int64_t B);
/* ws: ngnn_seed_xent_workspace_bytes(B), 16-B aligned (row losses; calls
 * sharing a ws must be stream-ordered).  The backward takes the same ws
 * (reserved) and recomputes the row log-sum-exps. */
int ngnn_seed_xent_fwd(const float *logits, int64_t ld, int64_t B, int64_t C, const int64_t *y,
                       int64_t ignore_index, float *loss, float *count, void *ws,
                       size_t ws_bytes, void *stream);
/* Forward and the unit-scale input gradient in ONE launch (the captured
 * training step's loss.backward(1)): writes *loss, *count and dlogits rows
 * < B = (softmax(x_r) - onehot(y_r)) / count (zeros for ignored rows); rows >=
 * B untouched.  The loss sum is the last workgroup's fixed-order sum of the
 * workgroups' partial sums (device ticket in ws, zero on entry, reset on exit):
 * deterministic.  ws as ngnn_seed_xent_fwd (zero-filled once).  Replaces
 * F.cross_entropy(out[:bs], y[:bs]) + its backward (pipeline.py:158,167). */
int ngnn_seed_xent_fwd_grad(const float *logits, int64_t ld, int64_t B, int64_t C,
                            const int64_t *y, int64_t ignore_index, float *loss, float *count,
                            float *dlogits, int64_t ldd, void *ws, size_t ws_bytes, void *stream);
int ngnn_seed_xent_bwd(const float *logits, int64_t ld, int64_t B, int64_t C, const int64_t *y,
                       int64_t ignore_index, const void *ws, const float *grad_scale,
                       const float *count, float *dlogits, int64_t ldd, void *stream);

/* ------------------------------------------------------------- optimiser
 * Adam step over n_tensors parameter tensors (host arrays of device
 * pointers; grads, exp_avgs, exp_avg_sqs like params, numels their sizes),
 * torch.optim.Adam's rule (amsgrad/maximize off, optional L2 weight decay),
 * with the step count a device float that this call advances (so a captured
 * HIP graph replays correctly).  ticket (nullable): 1024 device uint32 (ABI
 * 21; 64 in ABI 17-20, one before), zero before the first call, that the
 * update's workgroups count themselves on in two levels (each group's word
 * on a 128-B line of its own); the last one advances *step and every
 * word is zero again on return (one launch per call instead of an update +
 * increment pair; up to 16 tensors).  dtypes (host, nullable
 * = all NGNN_F32): per tensor NGNN_F32 or NGNN_BF16 (params and grads in that
 * dtype; exp_avgs / exp_avg_sqs always fp32).  Replaces the reference's
 * torch.optim.Adam(...).step() (model.py:66-69). */
/* dst[i] = bf16(src[i]) (round to nearest even, NaN kept) for i < n: a bf16
 * model's fp32 logits handed back in bf16 (Tensor.to(torch.bfloat16), the
 * `SAGE.forward` return dtype of a bf16 model).  src 16-B, dst 8-B aligned. */
int ngnn_cast_f32_bf16(const float *src, void *dst, int64_t n, void *stream);
/* The same over rows < min(n_rows, *n_rows_dev) of row_elems contiguous
 * elements each (n_rows_dev nullable): a graph slot's logits, cast for the
 * block's real rows only (ABI 15). */
int ngnn_cast_f32_bf16_rows(const float *src, void *dst, int64_t n_rows, int64_t row_elems,
                            const int32_t *n_rows_dev, void *stream);
/* n <= 16 tensors cast in one launch: to_bf16 = 0: dst[k][i] = float(src[k]
 * [i]) (bf16 -> fp32, exact); 1: dst[k][i] = bf16(src[k][i]) (round to
 * nearest even, NaN kept), i < numels[k] -- a bf16 model's parameters widened
 * for the fused kernels and their fp32 gradients narrowed back (Tensor.float()
 * and its autograd backward, one ATen copy kernel per tensor). */
int ngnn_cast_tensors(int n, const void *const *src, void *const *dst, const int64_t *numels,
                      int to_bf16, void *stream);
/* ABI 18: n <= 16 tensors of mixed dtypes in one launch: dst[k][i] =
 * cast(src[k][i]) / divisor (src_dtypes / dst_dtypes: host arrays of NGNN_F32
 * or NGNN_BF16 per tensor; bf16 -> fp32 exact, fp32 -> bf16 round to nearest
 * even; divisor 1: no division, otherwise the IEEE quotient as Tensor.div_;
 * src[k] == dst[k] allowed when the dtypes agree: in place) -- the
 * data-parallel gradient bucket's pack (each parameter's gradient into the
 * flat fp32 bucket) and unpack (bucket / world back into bf16 gradients and
 * in place into the fp32 ones that are bucket views): the copies and the
 * div_ of DistributedDataParallel's bucket path (pipeline.py:167-169 under
 * seed-sharded DP) as one launch each way. */
int ngnn_cast_tensors_ex(int n, const void *const *src, void *const *dst, const int64_t *numels,
                         const int32_t *src_dtypes, const int32_t *dst_dtypes, float divisor,
                         void *stream);
/* dst[r, :F] = float(src[r, :F]) (bf16 -> fp32, exact) for rows r <
 * min(n_rows, *n_rows_dev) (n_rows_dev nullable): the rows of a bf16 model's
 * activations a backward kernel reads as an fp32 mask. */
int ngnn_widen_bf16_rows(const void *src, int64_t lds, int64_t F, int64_t n_rows,
                         const int32_t *n_rows_dev, float *dst, int64_t ldd, void *stream);
/* gate / gate_gen (ABI 20, nullable): as ngnn_adam_fold's -- the step of a
 * block that broke the graph slot's contract updates nothing.
 *
 * State after a reload.  The call takes addresses only: *step is ONE count
 * for all n_tensors (a parameter group), and exp_avgs[k] / exp_avg_sqs[k]
 * are numels[k] fp32 values whatever dtypes[k] is.  A host that restores
 * optimizer state must hand back that layout (torch's load_state_dict alone
 * casts a bf16 model's moments to bf16 and copies the count per parameter);
 * ngnn.optim.Adam.load_state_dict does, and Adam.step() checks it before a
 * launch.  Counts that differ within a group, and a first gradient that
 * arrives after the group's state was made, are errors there.  Against a
 * float64 restatement the error is at most 2.1 x max(torch's own, half an
 * fp32 ulp of the tensor's largest value) per tensor for p and both moments
 * (profiles/adam_errors.jsonl). */
int ngnn_adam_step(int n_tensors, float *const *params, const float *const *grads,
                   float *const *exp_avgs, float *const *exp_avg_sqs, const int64_t *numels,
                   const int32_t *dtypes, float *step, uint32_t *ticket, float lr, float beta1, float beta2, float eps,
                   float weight_decay, const uint64_t *gate, const int64_t *gate_gen, void *stream);

/* ------------------------------------------------------ HIP-graph slot
 * Fill the static slot a captured training step reads (ngnn/graphs.py) with
 * one NeighborLoader block, in one launch: x rows [0, N) (slot rows past N
 * untouched), edge_index [2, E] (row stride ld_ei) plus padding self-loops
 * on rows N + floor(j (n_cap - N) / (e_cap - E)) for slot edges E + j, the
 * first B labels, and *n_valid = N.  Padding needs N < n_cap when E < e_cap.
 * Optional (NULL to skip): slot_rowptr [n_cap + 1] / slot_col [e_cap] int32
 * = the target-grouped CSR of the padded edges (both or neither; targets
 * must be non-decreasing, NeighborLoader's order), and *seed_state advanced
 * by one splitmix64 step (the dropout seed of the captured step).  x_dev
 * (nullable): zero-copy -- store x's address there instead of copying the
 * rows (slot_x may then be NULL; x 16-B aligned with ldx == ld_slot).
 * r_next (nullable, 8-B aligned): its low 32 bits become max(B, 1 + max
 * source of the edges into rows < B) -- ngnn_block_prefix_stats for R = B,
 * the input-gradient row bound of the top layer's backward (computed here
 * so the captured step has no bound launch).  Kept by a 64-bit atomicMax of
 * (gen << 32 | value): gen must grow with every load (no reset launch).
 * n_edge_rows (nullable): 1 + the last target (0 without edges) = the split
 * of ngnn_sage_fwd_raw's n_edge_rows_dev.
 * slot_ei may be NULL when the CSR is written (a captured step that reads
 * only the CSR).
 * pack_dst (nullable): a pack job in the same launch -- pack_dst =
 * ngnn_pack_weight(pack_w [pack_fo, pack_k], row stride pack_ldw), the
 * current values of a weight the captured step's forward then reads with
 * NGNN_WL_PREPACKED (no pack launch inside the step; read at load time, so
 * parameters changed between steps are picked up).
 * err (nullable; may be host memory the device can write, e.g. pinned):
 * bits OR-ed in (never cleared here) when the block breaks the slot's
 * contract -- NGNN_SLOT_UNSORTED: a target smaller than the one before it;
 * NGNN_SLOT_RANGE: a source or target outside [0, N).  The CSR of such a
 * block is wrong, but no consumer of the slot reads or writes out of bounds:
 * a source outside [0, N) is stored as row 0 (slot_ei, slot_col, slot_colx
 * and the r_next bound; ABI 18), a target only selects which rowptr entries
 * (clamped to [0, n_cap]) its edge lands under.  E > 0 needs N >= 1.  The
 * caller checks the word without a device sync (ABI 16: replaces a host
 * read-back of the targets).
 * gate (ABI 20, nullable, 8-B aligned device word): (gen << 32 | bits) of the
 * newest load that broke the contract, by a 64-bit atomicMax -- the device
 * copy of err that ngnn_adam_fold / ngnn_adam_step read to skip that step's
 * update (no reset launch: the generation tells this load's bits from an
 * older load's).
 * counts_dev (ABI 19, nullable): device int32 {N', E', ...} -- the block's
 * row and edge counts are min(N', N) / min(E', E), read on the device (N / E
 * are then bounds: the capacity-sized buffers a sync-free sampler wrote;
 * ld_ei >= E still holds).
 * Replaces the host-side batch hand-over of pipeline.py:152-160 (batch.x,
 * batch.edge_index, batch.y[:batch_size]) for graph replay. */
#define NGNN_SLOT_UNSORTED 1
#define NGNN_SLOT_RANGE 2
int ngnn_slot_load(const float *x, int64_t ldx, int64_t N, int64_t F, const int64_t *edge_index,
                   int64_t ld_ei, int64_t E, const int64_t *y, int64_t B, float *slot_x,
                   int64_t ld_slot, int64_t n_cap, int64_t *slot_ei, int64_t e_cap,
                   int64_t *slot_y, int32_t *n_valid, int32_t *slot_rowptr, int32_t *slot_col,
                   uint64_t *seed_state, const float **x_dev, int64_t *r_next, uint32_t gen,
                   int32_t *n_edge_rows, const int64_t *xrow, const int64_t **xrow_dev,
                   int32_t *slot_colx, const float *pack_w, int64_t pack_ldw, int64_t pack_fo,
                   int64_t pack_k, float *pack_dst, int32_t *err, const int32_t *counts_dev,
                   uint64_t *gate, void *stream);

/* --------------------------------------------- SAGEPL's per-node input noise
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).  SAGEPL.adding_noise (src/models/layers/sagePL.py:
 * 41-49) in one launch, and its backward in one launch.  fp32 only, any
 * F >= 1.  For row i < n_rows, id = n_id ? n_id[i] : i (n_id int64, nullable;
 * NULL needs n_rows == n_nodes), v = noise[id, :F] of the table noise
 * [n_nodes, ldn], d = max(||v||_2, 1e-12) -- F.normalize(dim=1) as torch
 * defines it:
 *   fwd:  out[i, f] = x[i, f] + s * (v[f] / d) * rate
 *         s = 1, or sign(x[i, f]) with sign(0) = 0 under NGNN_NOISE_SIGN (the
 *         reference's n_id=None branch, sagePL.py:44)
 *   bwd:  gs = g[i, :] * rate * s,  u = v / d,
 *         dv = (gs - u <u, gs>) / d   if ||v|| >= 1e-12,  else  gs / 1e-12
 *         (clamp_min's backward: a zero row gets a large finite gradient, as
 *         in torch); the norm is recomputed from the table row, x is read
 *         only under NGNN_NOISE_SIGN (nullable otherwise)
 *         scatter = 1: dnoise[id, :] += dv by float atomics into the caller's
 *           zeroed [n_nodes, ldd] buffer (duplicate ids accumulate, as
 *           index_add_; the sum's last bits depend on arrival order)
 *         scatter = 0: dnoise[i, :] = dv, plain stores into [n_rows, ldd]
 *           (bitwise reproducible; the caller sums duplicates)
 * An id outside [0, n_nodes) neither reads nor writes the table: forward
 * copies x to out for that row, backward contributes nothing (scatter = 0
 * stores a zero row); each adds 1 to *bad (device int32, nullable).
 * 16-B accesses when the bases and leading dimensions allow, dword accesses
 * otherwise; a lane group per row, row sums by cross-lane shuffles; no
 * allocation, no host synchronisation (safe under stream capture).
 * n_rows == 0 or F == 0: success, no pointer is read.  Before any launch:
 * a negative size, an unknown flag, scatter not 0 / 1, n_id NULL with n_rows
 * != n_nodes, a NULL data pointer: NGNN_E_ARG; a leading dimension < F:
 * NGNN_E_SHAPE; n_rows or F >= 2^31: NGNN_E_RANGE.
 * Replaces x.clone(), noise[n_id], F.normalize, the scale and the add (and
 * their autograd backwards with index_add_) [ext: torch]. */
#define NGNN_NOISE_SIGN 1
int ngnn_node_noise_fwd(const float *x, int64_t ldx, const float *noise, int64_t ldn, int64_t n_nodes,
                        const int64_t *n_id, int64_t n_rows, int64_t F, float rate, int flags,
                        float *out, int64_t ldo, int32_t *bad, void *stream);
int ngnn_node_noise_bwd(const float *g, int64_t ldg, const float *x, int64_t ldx, const float *noise,
                        int64_t ldn, int64_t n_nodes, const int64_t *n_id, int scatter, int64_t n_rows,
                        int64_t F, float rate, int flags, float *dnoise, int64_t ldd, int32_t *bad,
                        void *stream);

/* ------------------------------------------- similarity top-k edge rewiring
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).  topk_rewire(h, edge_index, k_percent,
 * directed=False) of src/utils/augmentation.py:36-86 without any N x N
 * matrix.  h: fp32 [n, ldh], F columns used; src / dst: the two rows of
 * edge_index (int64 [e] each; duplicates collapse, self-loops count);
 * k2 = 2 * int(n * k_percent), computed by the caller.  With hn = h / max(
 * ||h||_2, 1e-12) per row (a zero row stays zero), S = hn hn^T clamped to
 * [-1, 1], A the edge set and D the diagonal, four selections of exactly k2
 * of the n * n entries each:
 *   1  k2 smallest of  S * (A and not D ? 1 : 1000)
 *   2  k2 largest  of  S - 100 [A and not selected by 1] - 100 [D]
 *   3  k2 largest  of  S * ([A] - 1000 [D])
 *   4  k2 smallest of  S * ((A ? 1000 : 1) + 1000 [D])
 * equal keys in ascending flat index i * n + j (-0 equals +0; selection 2
 * orders by penalty, then S: exactly, not through the rounding of S - 100);
 * pos = (A minus sel 1) or sel 2, neg = (A minus sel 3) or sel 4, each
 * written as int64 [2, cap] rows (row 0 at pos, row 1 at pos + pos_cap),
 * sorted by (row, column) without duplicates -- torch.nonzero's order.
 * counts (device int32 [3]): {entries of pos, entries of neg, overflow}; an
 * output longer than its capacity is cut at the capacity (its count is not),
 * e + k2 always suffices.  overflow = 1: a candidate list filled up (more
 * than 2^20 non-edges share, to within an fp32 step or two, the similarity
 * at a selection's threshold -- a mass tie): nothing was written out of
 * bounds, the outputs are not valid.
 * bad (device int32, nullable): incremented once per edge with an endpoint
 * outside [0, n); such an edge is otherwise ignored.
 * sel_out (nullable): int64 [4, k2], the four selections' flat indices in
 * selection order (best key first).
 * S is exact fp32 (v_mfma_f32_16x16x4_f32 over the non-edges, fp32 FMAs over
 * the edges and the diagonal); results are bitwise reproducible.
 * ws: ngnn_topk_rewire_workspace_bytes(n, F, e, k2) bytes, 256-B aligned:
 * O(n F + e + k2) plus the bounded candidate lists; 0 for n == 0 or sizes
 * the entry refuses.  Nothing is allocated and the host does not wait.
 * n == 0: success, nothing is read or written.  Before any launch: a
 * negative size or capacity, a NULL h / src / dst / pos / neg (where its
 * size is not 0) / counts / ws: NGNN_E_ARG; ldh < F: NGNN_E_SHAPE;
 * n > 65535 (a flat index fits 32 bits), k2 > n * n, e or k2 > 2^29,
 * F > 2^20, a capacity >= 2^31: NGNN_E_RANGE; a misaligned ws / pos / neg:
 * NGNN_E_ALIGN; ws_bytes too small: NGNN_E_WORKSPACE.
 * Replaces F.normalize, the dense similarity matrix, the dense masks, four
 * torch.topk over n * n keys and two torch.nonzero [ext: torch]. */
size_t ngnn_topk_rewire_workspace_bytes(int64_t n, int64_t F, int64_t e, int64_t k2);
int ngnn_topk_rewire(const float *h, int64_t ldh, int64_t n, int64_t F, const int64_t *src,
                     const int64_t *dst, int64_t e, int64_t k2, int64_t *pos, int64_t pos_cap,
                     int64_t *neg, int64_t neg_cap, int32_t *counts, int32_t *bad, int64_t *sel_out,
                     void *ws, size_t ws_bytes, void *stream);

/* ----------------------------------- backward-correction and CoDi losses
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * backward_correction(output, labels, C, nbr_class) of src/utils/losses.py:
 * 51-70, given the inverse Cinv float [C, C] (row stride ldc) of its
 * correction matrix.  With w_r = Cinv[labels[r]], p = softmax(logits[r]),
 * q = clamp(p, 1e-5, 1 - 1e-5):
 *   loss    = -(1 / (B C)) sum_{r < B} sum_k w_r[k] log q_rk
 *   d x_rj  = -(g / (B C)) (w_rj m_rj - p_rj sum_k w_rk m_rk),
 *             m_rk = [1e-5 <= p_rk <= 1 - 1e-5]  (clamp's gradient)
 * ngnn_bc_loss_fwd writes *loss and, when dlogits is not NULL, the gradient
 * rows [0, B) at unit scale (g = 1); ngnn_bc_loss_bwd writes them for the
 * device scalar *grad_scale.  Rows >= B are never read or written.  One wave
 * per row, the row partials added in a fixed order by a second launch:
 * deterministic.  No ignore_index (the reference's scatter_ would raise): a
 * label outside [0, C) reads no row of Cinv and makes the loss and its
 * gradient row NaN.  ws: ngnn_bc_loss_workspace_bytes(B), 16-B aligned.
 * Before any launch: a NULL logits / labels / Cinv / loss / ws (fwd) or
 * grad_scale / dlogits (bwd), B or C <= 0: NGNN_E_ARG; ld, ldc or ldd < C:
 * NGNN_E_SHAPE; B or C >= 2^31: NGNN_E_RANGE; ws too small or misaligned:
 * NGNN_E_WORKSPACE.
 * Replaces softmax, clamp, log, the one-hot scatter, the [B, C] x [C, C]
 * matmul, the mean and their autograd [ext: torch]. */
size_t ngnn_bc_loss_workspace_bytes(int64_t B);
int ngnn_bc_loss_fwd(const float *logits, int64_t ld, int64_t B, int64_t C, const int64_t *labels,
                     const float *Cinv, int64_t ldc, float *loss, float *dlogits, int64_t ldd,
                     void *ws, size_t ws_bytes, void *stream);
int ngnn_bc_loss_bwd(const float *logits, int64_t ld, int64_t B, int64_t C, const int64_t *labels,
                     const float *Cinv, int64_t ldc, const float *grad_scale, float *dlogits,
                     int64_t ldd, void *stream);

/* CoDiLoss.forward (src/utils/losses.py:106-137): ngnn_ct_loss_fwd's exchange
 * with the selection key
 *   key_m[r] = l_m[r] - co_lambda * js[r],
 *   js[r]    = sum_k mean_k (log mean_k - (lp_k + lq_k) / 2),
 *   lp = log_softmax(y_1[r]), lq = log_softmax(y_2[r]),
 *   mean = (softmax(y_1[r]) + softmax(y_2[r])) / 2
 * (js_loss_compute: kl_div with target `mean` against both log-softmaxes,
 * i.e. KL(mean || .), unbounded; a term with mean_k == 0 is 0, xlogy's rule).
 * ind_m_sorted = argsort(key_m) ascending, ties by row index, NaN last.
 * R = num_remember, and num_remember == 0 selects ALL B rows (R = B,
 * losses.py:125-128).  out[0] = mean of l_1 (the cross entropy, not the key)
 * over ind_2_sorted[:R], out[1] its mirror, out[2..3] the pure ratios over R
 * rows, as ngnn_ct_loss_fwd.  js_out: B floats, may be NULL.  The other
 * arguments, the B <= 8192 limit and the error codes are ngnn_ct_loss_fwd's.
 * js is detached in the reference, so the backward is ngnn_ct_loss_bwd's on
 * the rows the other model kept: ngnn_codi_loss_bwd, on this workspace
 * (ngnn_codi_loss_workspace_bytes(B), kept between the forward and both
 * backwards). */
size_t ngnn_codi_loss_workspace_bytes(int64_t B);
int ngnn_codi_loss_fwd(const float *y1, int64_t ld1, const float *y2, int64_t ld2, int64_t B,
                       int64_t C, const int64_t *y_noise, int64_t ignore_index, int64_t num_remember,
                       float co_lambda, const int64_t *ind, const uint8_t *noise_or_not,
                       int64_t n_noise, float *out, int64_t *ind1_sorted, int64_t *ind2_sorted,
                       float *js_out, void *ws, size_t ws_bytes, int *err, void *stream);
int ngnn_codi_loss_bwd(int model, const float *y, int64_t ld, int64_t B, int64_t C,
                       const int64_t *y_noise, int64_t ignore_index, const void *ws,
                       const float *grad, float *dy, int64_t ldd, void *stream);

/* ------------------------- shuffle_pos and the contrastive discriminator loss
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * ngnn_shuffle_rows: shuffle_pos(features, prob) of src/utils/augmentation.py:
 * 88-102 with m = int(F * prob) taken by the caller: per row, a uniform
 * random m-subset of the columns, the values at those columns permuted
 * uniformly at random.  The reference draws from torch's global CPU generator
 * (two randperm per row); this entry defines its own draw, a pure function
 * of (seed, row r, F, m), bitwise reproducible and independent of the launch
 * geometry.  With mix64 the sampler's mixer (splitmix64's finaliser on
 * z + 0x9E3779B97F4A7C15), all arithmetic modulo 2^64:
 *   b1 = mix64(seed ^ mix64(r + 0x632BE59BD9B4E019));  key1(c) = mix64(b1 + c)
 *   S_r = the m columns with the smallest (key1(c), c)        -- ties by column
 *   b2 = mix64(b1 ^ 0xD1B54A32D192ED03);               key2(c) = mix64(b2 + c)
 *   p_0 < ... < p_{m-1} the columns of S_r;
 *   rho(j) = rank of (key2(p_j), p_j) within S_r
 *   out[r, p_j] = x[r, p_rho(j)];  out[r, c] = x[r, c] for c not in S_r
 * m = 0 or 1 copies, m = F permutes whole rows.  Columns [F, ldo) of out are
 * never written, columns [F, ldx) of x never read.  out must not alias x
 * (rows are read after other columns of them were written).  n_rows == 0 or
 * F == 0: NGNN_OK, nothing read.  Before any launch: a negative size, m
 * outside [0, F], a NULL x or out (with rows to move): NGNN_E_ARG; ldx or
 * ldo < F: NGNN_E_SHAPE; n_rows >= 2^31 or F > 65535: NGNN_E_RANGE.
 * F <= 256 (the training shapes): one wave per row; wider rows: one
 * workgroup per row, O(F^2) key compares -- correct, not fast.  No
 * workspace, no allocation, no host wait: safe under stream capture (which
 * bakes `seed` in).
 * Replaces a Python loop of two torch.randperm and an indexed write per row
 * [ext: torch]. */
int ngnn_shuffle_rows(const float *x, int64_t ldx, int64_t n_rows, int64_t F, int64_t m,
                      uint64_t seed, float *out, int64_t ldo, void *stream);

/* Discriminator_innerprod + BCEExeprtLoss (src/utils/data_utils.py:34-64) on
 * the rows idx[0..M) of h, hp, hn (float [n_rows, F], row strides ldh, ldp,
 * ldn).  With a_i = <h[idx_i], hp[idx_i]>, b_i = <h[idx_i], hn[idx_i]>:
 *   loss = (1/M) sum_i softplus(-a_i) + (1/M) sum_i softplus(b_i)
 *          (BCEWithLogits against ones / zeros, each a mean;
 *           softplus(x) = max(x, 0) + log1p(exp(-|x|)))
 *   d h [idx_i] += (g/M) (-sigma(-a_i) hp[idx_i] + sigma(b_i) hn[idx_i])
 *   d hp[idx_i] += (g/M) (-sigma(-a_i)) h[idx_i]
 *   d hn[idx_i] += (g/M)   sigma(b_i)   h[idx_i]
 * ngnn_contrast_fwd writes out[0] = loss, out[1] / out[2] = its positive /
 * negative term and keeps a_i, b_i in ws (ngnn_contrast_workspace_bytes(M),
 * 16-B aligned, kept until the backward; the logits are accumulated and kept
 * in double: e^-a carries a's absolute error); one wave per selected row, the row
 * terms added in a fixed order by a second launch: deterministic.
 * ngnn_contrast_bwd ADDS the gradient rows, scaled by the device scalar
 * *grad_scale, with float atomics into the buffers the caller prepared (any
 * of dh, dhp, dhn may be NULL): duplicates in idx accumulate, as
 * index_put_(accumulate=True); distinct indices give a bitwise reproducible
 * result.  sigma(-a) is evaluated as 1 / (1 + e^a), so the positive term's
 * gradient survives large logits (torch's fp32 BCEWithLogits backward returns
 * 0 there from a ~ 17 on).  An idx entry outside [0, n_rows) reads and writes
 * nothing, makes the loss NaN and adds 1 to *bad (may be NULL); the
 * reference raises there.  Before any launch: a NULL h / hp / hn / idx / ws /
 * out (fwd) / grad_scale (bwd), n_rows, F or M <= 0: NGNN_E_ARG; a row
 * stride < F: NGNN_E_SHAPE; n_rows, F or M >= 2^31: NGNN_E_RANGE; ws too
 * small or misaligned (fwd): NGNN_E_WORKSPACE.
 * Replaces three index_select, two mul + sum, two BCEWithLogitsLoss and
 * three zero-filled [n_rows, F] index backward gradients [ext: torch]. */
size_t ngnn_contrast_workspace_bytes(int64_t M);
int ngnn_contrast_fwd(const float *h, int64_t ldh, const float *hp, int64_t ldp, const float *hn,
                      int64_t ldn, int64_t n_rows, int64_t F, const int64_t *idx, int64_t M,
                      float *out, int32_t *bad, void *ws, size_t ws_bytes, void *stream);
int ngnn_contrast_bwd(const float *h, int64_t ldh, const float *hp, int64_t ldp, const float *hn,
                      int64_t ldn, int64_t n_rows, int64_t F, const int64_t *idx, int64_t M,
                      const void *ws, const float *grad_scale, float *dh, int64_t lddh, float *dhp,
                      int64_t lddp, float *dhn, int64_t lddn, void *stream);

/* ------------------- neighbourhood uncertainty and the consistency loss
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * ngnn_nbr_uncertainty: get_uncertainty_batch(edge_index, y_pure,
 * nbr_classes, device, epsilon) of src/utils/losses.py:185-204 on the rows
 * [0, R) of a block, R <= n_rows.  logp: float [n_rows, C] log-probabilities
 * (row stride ld); rowptr int32 [n_rows + 1] / col int32 [E]: the edges
 * grouped by SOURCE, rowptr by edge_index[0] and col = edge_index[1] (the
 * reference's A = coo(row = edge_index[0], col = edge_index[1]), A @ p: the
 * transpose of what SAGEConv aggregates).  With p = exp(logp):
 *   s_i   = sum over list(i) of p[col[e]]       (duplicates and self-loops count)
 *   ptc_i = s_i / (deg_i + epsilon)             (deg_i = the list's length)
 *   h_i   = -sum_k ptc_ik log2(ptc_ik + 1e-5)
 *   w[i]  = exp(-h_i / log2(nbr_classes))       (an empty list: exactly 1)
 * One wave per row, lanes over the classes (a chunk loop for C > 64), the
 * list summed in list order in fp32 (groups of four, a Kahan compensation
 * across them: a hub's thousands of terms cost no accuracy), the entropy
 * reduced with wave shuffles:
 * no atomics, no workspace, no host wait, bitwise reproducible for a given
 * CSR; a wave runs as long as its list.  Nothing past w[R) is written,
 * columns [C, ld) are never read.  A col entry outside [0, n_rows) reads
 * nothing and makes its row's w NaN.  R == 0: NGNN_OK, nothing read.  Before
 * any launch: a negative size, R > n_rows, nbr_classes < 2 (the reference
 * divides by log2(1) = 0), a NULL logp / rowptr / w with rows to write (col
 * may be NULL for a CSR without edges): NGNN_E_ARG; ld < C: NGNN_E_SHAPE;
 * n_rows or R >= 2^31, C > 65535: NGNN_E_RANGE.
 * Replaces edge_index.cpu(), a scipy COO build, a sparse tensor upload,
 * torch.sparse.mm, a sparse row sum and about ten elementwise launches
 * [ext: torch, scipy]. */
int ngnn_nbr_uncertainty(const float *logp, int64_t ld, int64_t n_rows, int64_t C,
                         const int32_t *rowptr, const int32_t *col, int64_t R, int64_t nbr_classes,
                         float epsilon, float *w, void *stream);

/* fix_cr(y_pure, y_noisy, ind_noisy, batch_size, name, T, p_cutoff,
 * use_hard_labels, w) of src/utils/losses.py:206-246 on the rows [0, B) of
 * the log-probabilities lp_pure, lp_noisy (float, C columns, row strides ldp,
 * ldn).  Per row r: pp = exp(lp_pure[r]), pn = exp(lp_noisy[r]),
 * s = softmax(pn) (the reference feeds the probabilities pn to cross_entropy
 * as logits), m_r = [max_k pp_k >= p_cutoff], k* the FIRST index of that
 * maximum (torch.max's tie rule; a NaN is the maximum and masks the row),
 * w_r = w[r] (1 when w is NULL), c_r = g m_r w_r / B.
 *   mode 0 (name 'ce', hard labels): l_r = logsumexp(pn) - pn[k*]
 *     d lp_noisy[r,k] = c_r (s_k - [k == k*]) pn_k;  d lp_pure = 0
 *   mode 1 (name 'ce', soft labels): l_r = -sum_k pp_k log_softmax(pn)_k
 *     d lp_pure [r,k] = -c_r pp_k log_softmax(pn)_k   (pp is not detached)
 *     d lp_noisy[r,k] =  c_r (s_k sum_j pp_j - pp_k) pn_k
 *   modes 0, 1: loss = (1/B) sum_r w_r (m_r l_r) -- the mean over all B rows,
 *     the mask a factor: a NaN row term makes the loss NaN even at m_r = 0
 *   mode 2 (name 'l2'): loss = (1/(B C)) sum_rk (lp_noisy - lp_pure)^2,
 *     d lp_noisy = 2 g (lp_noisy - lp_pure) / (B C) = -d lp_pure;
 *     w and p_cutoff are not read
 * ngnn_fix_cr_fwd writes *loss and, for each of d_pure / d_noisy that is not
 * NULL, its gradient rows [0, B) at unit scale (g = 1); ngnn_fix_cr_bwd
 * recomputes from the inputs (no state between the calls) and writes them
 * for the device scalar *grad_scale (either may be NULL; in mode 0 a given
 * d_pure is written as zeros).  Rows >= B and columns >= C are never read or
 * written.  One wave per row, the row terms added in a fixed order by a
 * second launch: deterministic.  ws: ngnn_fix_cr_workspace_bytes(B), 16-B
 * aligned, free after the forward.  Before any launch: a NULL lp_pure /
 * lp_noisy / loss / ws (fwd) / grad_scale (bwd), B or C <= 0, a mode outside
 * {0, 1, 2}: NGNN_E_ARG; ldp, ldn or a given gradient's stride < C:
 * NGNN_E_SHAPE; B >= 2^31 or C > 65535: NGNN_E_RANGE; ws too small or
 * misaligned: NGNN_E_WORKSPACE.
 * Replaces two slices, two exp, max, ge, cross_entropy (or log_softmax, mul,
 * sum), two mul, mean and their autograd [ext: torch]. */
size_t ngnn_fix_cr_workspace_bytes(int64_t B);
int ngnn_fix_cr_fwd(const float *lp_pure, int64_t ldp, const float *lp_noisy, int64_t ldn, int64_t B,
                    int64_t C, int mode, float p_cutoff, const float *w, float *loss, float *d_pure,
                    int64_t lddp, float *d_noisy, int64_t lddn, void *ws, size_t ws_bytes, void *stream);
int ngnn_fix_cr_bwd(const float *lp_pure, int64_t ldp, const float *lp_noisy, int64_t ldn, int64_t B,
                    int64_t C, int mode, float p_cutoff, const float *w, const float *grad_scale,
                    float *d_pure, int64_t lddp, float *d_noisy, int64_t lddn, void *stream);

/* ------------------------------------------- flip_label: label-noise injection
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * ngnn_flip_labels: the per-node draw of flip_label(labels, nbr_classes,
 * noise_type, prob) of src/utils/noise.py:54-58: out[i] is drawn from row
 * y[i] of a row-stochastic [C, C] transition matrix M.  The reference draws
 * np.random.multinomial per node from numpy's global generator; this entry
 * defines its own draw, a pure function of (seed, i0 + i, y[i], M), bitwise
 * reproducible and independent of the launch geometry.
 *   Thresholds (taken by the caller, in float64): cs_k = cumsum(M[l])[k],
 *   jl = the largest k with M[l][k] > 0;
 *     T[l][k] = min(floor(cs_k * 2^32), 2^32 - 1)  for k <  jl
 *     T[l][k] = 2^32 (never reached)               for k >= jl
 *   passed as thr: uint32 [C, C] row-major (entries k >= jl are not read) and
 *   last: int32 [C] = jl (clamped to [0, C - 1]).  Rows of thr must be
 *   non-decreasing over k < jl, as a cumulative sum of non-negatives is.
 *   Draw, with mix64 the sampler's mixer (splitmix64's finaliser on
 *   z + 0x9E3779B97F4A7C15), all arithmetic modulo 2^64:
 *     r = mix64(seed ^ mix64((i0 + i) + 0xA0761D6478BD642F)) >> 32
 *     out[i] = the number of k with T[y[i]][k] <= r
 * Class j is drawn with a probability within 2^-32 of M[l][j]; a class of
 * probability zero is never drawn.  The salt is neither the sampler's
 * (0x632BE59BD9B4E019) nor the shuffle's second (0xD1B54A32D192ED03).
 * y: int64 [n]; out: int64 [n], must not alias y (the kernel takes both as
 * restrict, and an overlapping out is read after it was written); clean: uint8 [n] or NULL,
 * clean[i] = (out[i] == y[i]), the reference's noise_or_not; counts: int64
 * [C, C] zeroed by the caller, or NULL (then no histogram work is done):
 * counts[l][j] += the nodes with y = l and out = j; bad: int32 [1] or NULL: a
 * label outside [0, C) is copied unchanged (clean 1), added to *bad and left
 * out of counts (the reference raises IndexError there).  i0: the global
 * index of y[0] -- a shard [a, b) of the nodes flipped with i0 = a gets
 * exactly rows [a, b) of the whole vector's flip.
 * One launch, one lane per node: 1024-thread workgroups, grid =
 * min(ceil(n / 1024), compute units), a grid-stride loop of four nodes per
 * thread and trip (a trip of the whole grid covers 4 * 1024 * grid nodes);
 * thr, last and a [C, C] histogram live in dynamic LDS, 4 C (2 C + 1) bytes,
 * which limits C to ngnn_flip_labels_max_classes() (128: 128.5 KiB); counts
 * is gathered per workgroup in LDS and flushed once, non-zero cells only,
 * with 64-bit vector atomics (integer adds: the result does not depend on
 * their order).  No workspace, no allocation, no host wait: safe under
 * stream capture (which bakes seed and i0 in).  n == 0: NGNN_OK, nothing
 * read, no pointer needed.  Before any launch: a negative n or i0, C < 1, a
 * NULL y / out / thr / last with n > 0: NGNN_E_ARG; C above the limit:
 * NGNN_E_SHAPE; n >= 2^31: NGNN_E_RANGE.
 * Replaces a Python loop of .item(), np.random.multinomial and np.where per
 * node [ext: numpy]. */
int ngnn_flip_labels_max_classes(void);
int ngnn_flip_labels(const int64_t *y, int64_t n, int64_t C, const uint32_t *thr, const int32_t *last,
                     uint64_t seed, int64_t i0, int64_t *out, uint8_t *clean, int64_t *counts,
                     int32_t *bad, void *stream);

/* ------------------------------------- epoch metrics and per-split accuracy
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * The tail of every training loop body (pipeline.py:120-125, :164-165:
 * total_loss += float(loss); total_correct += int(out.argmax(dim=-1).eq(y)
 * .sum()); total_ratio += 100 * pure_ratio) and of every evaluation
 * (pipeline.py:182-195: out.argmax(dim=-1, keepdim=True), three index
 * gathers, three Evaluator.eval) without a host read.
 *
 * Argmax rule (both entries), torch.argmax's: the first index of the row's
 * maximum; +0.0 and -0.0 are equal; a NaN beats every number and the first
 * NaN wins; a row of -inf gives 0.  bf16 rows are widened exactly.  A row
 * starts at a multiple of ld elements and needs element alignment only (4 B
 * for fp32, 2 B for bf16): it is read with single-element loads, a group of
 * lanes per row (the power of two at or above C / 4, at most 64), which
 * consecutive lanes coalesce.
 *
 * ngnn_step_metrics: one launch, no workspace.  logits: [>= B, C], row
 * stride ld elements, dtype NGNN_F32 or NGNN_BF16; y: int64 [B]; s0..s3:
 * float [1] each or NULL (the step's loss, or loss_1, loss_2, pure_ratio_1,
 * pure_ratio_2); acc: eight 8-byte words owned (and zeroed) by the caller,
 * 8-byte aligned:
 *   word 0   int64   += 1 (steps)
 *   word 1   int64   += rows counted: rows < B whose label is in [0, C)
 *   word 2   int64   += rows counted whose argmax equals the label
 *   word 3   int64   += rows whose label is outside [0, C) and is not
 *                       ignore_index (never counted, never correct)
 *   word 4+k double  += (double)*s_k for each non-NULL s_k
 * A row that is not counted is not read.  Words 1..3 receive at most one
 * 64-bit integer vector atomic per workgroup, after a wave and an LDS
 * reduction; word 0 and the four sums are written by exactly one thread of
 * the launch, so a sum is the fp64 sum of the fp32 scalars in launch order
 * whatever the arrival order of the workgroups.  256-thread workgroups, grid
 * = min(max(ceil(B * lanes per row / 256), 1), 8 * compute units), a
 * grid-stride loop.  No allocation and every address an argument: safe under
 * stream capture.  B == 0 is valid (word 0 and the sums still advance;
 * logits and y may be NULL then).  Before any launch: B < 0, C < 1, a NULL
 * acc, a NULL logits or y with B > 0: NGNN_E_ARG; B or C >= 2^31:
 * NGNN_E_RANGE; ld < C: NGNN_E_SHAPE; an unknown dtype: NGNN_E_DTYPE; acc not
 * 8-byte aligned: NGNN_E_ALIGN.
 *
 * ngnn_split_accuracy: evaluation in one pass over a list of node ids.
 * logits: [N, C] as above; y: int64 [N]; rows: int64 [M] node ids or NULL (then
 * M must equal N and entry p is node p; an empty list, M = 0, needs no pointer); bounds: a HOST pointer -- the one
 * exception to "device pointers only" -- to S + 1 int64, 1 <= S <= 8,
 * non-decreasing, bounds[0] = 0, bounds[S] = M, read before the call returns
 * and passed to the kernel by value (so the call stays capturable).  Entries
 * [bounds[s], bounds[s + 1]) form segment s; ids may repeat and segments may
 * overlap in ids, and every entry counts (as y_pred[split_idx[k]] does).
 *   counts: int64 [S][4], overwritten:
 *     [s][0] evaluated entries: id in [0, N) and label in [0, C)
 *     [s][1] of those, entries whose argmax equals the label
 *     [s][2] bad entries: id outside [0, N), or label outside [0, C) and not
 *            ignore_index
 *     [s][3] ignored entries (label == ignore_index)
 *   pred: int64 [M] or NULL: pred[p] = the argmax of row rows[p], -1 for an
 *     id outside [0, N)
 *   confusion: int64 [C][C] or NULL, overwritten: confusion[t][q] = evaluated
 *     entries with label t and argmax q.  Needs C <=
 *     ngnn_confusion_max_classes() (128): the matrix is gathered per
 *     workgroup in a uint32 LDS histogram (4 C^2 bytes of dynamic LDS, 64 KiB
 *     at 128) and its non-zero cells flushed once with 64-bit vector atomics.
 * The row of an id outside [0, N) is never read (neither its label nor its
 * logits); the logits row of an ignored or badly labelled entry is read only
 * when pred is asked for.  Two memset nodes (counts, confusion) and one
 * launch: 1024-thread workgroups, grid = min(ceil(M * lanes per row / 1024),
 * 2 * compute units), a grid-stride loop; per-segment counts gathered in LDS
 * and flushed once per workgroup.  M == 0 or N == 0: NGNN_OK with counts (and
 * confusion) zeroed and, for N == 0, pred all -1; nothing else is read.
 * Before anything is enqueued: S outside [1, 8], negative N, M or C < 1, a
 * NULL bounds or counts, bounds not as stated, rows NULL with M neither N nor 0, a NULL
 * logits or y with M > 0 and N > 0: NGNN_E_ARG; N, M or C >= 2^31:
 * NGNN_E_RANGE; ld < C, or confusion with C above the limit: NGNN_E_SHAPE; an
 * unknown dtype: NGNN_E_DTYPE.
 * Replaces argmax, index_select, eq, sum and .item() per split, or a copy of
 * the logits to the host [ext: torch, ogb Evaluator, sklearn accuracy_score]. */
int ngnn_confusion_max_classes(void);
int ngnn_step_metrics(const void *logits, int64_t ld, int dtype, int64_t B, int64_t C, const int64_t *y,
                      int64_t ignore_index, const float *s0, const float *s1, const float *s2, const float *s3,
                      void *acc, void *stream);
int ngnn_split_accuracy(const void *logits, int64_t ld, int dtype, int64_t N, int64_t C, const int64_t *y,
                        int64_t ignore_index, const int64_t *rows, int64_t M, int S, const int64_t *bounds,
                        int64_t *counts, int64_t *pred, int64_t *confusion, void *stream);

/* ------------------------- symmetric-normalised GCN: the weighted aggregate
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * PyG 2.5.1 GCNConv(normalize=True) [ext] for a Tensor edge_index, flow
 * source -> target: out = D^-1/2 (A + I) D^-1/2 (x W^T) + b, with gcn_norm's
 * self-loop rewrite (add_remaining_self_loops) and optional edge weights.
 *
 * ngnn_gcn_norm: one pass over the rows of a target-grouped CSR (rowptr
 * int32 [n_rows + 1], col int32 [nnz]; w: fp32 [nnz] in CSR order or NULL =
 * all ones), one thread per row, no atomics: deterministic.
 *   add_self_loops != 0: every entry col == row leaves the degree; the row
 *     gets one loop of weight loop_w[row] = 1, or, weighted, the weight of the
 *     row's self-loop entry when it has one.  Several weighted self-loops on
 *     one node are unspecified in PyG (an index_put with duplicates); here the
 *     LAST in CSR (= edge) order wins.  deg = sum of the remaining entries'
 *     weights in CSR order, the loop's weight added last, accumulated in
 *     fp64 (a hub row's thousands of weights would cost dinv ulps in fp32).
 *   add_self_loops == 0: deg = sum of every entry's weight in CSR order;
 *     loop_w is not written (may be NULL).
 *   dinv[row] = 1 / sqrt(deg): IEEE fp64 sqrt and divide, rounded once to
 *     fp32 (no approximate reciprocal square root); deg == 0 gives 0 (PyG's
 *     masked_fill(inf, 0)), a negative degree NaN, as PyG.
 * Before any launch: n_rows < 0, a NULL rowptr or dinv, a NULL loop_w with
 * add_self_loops (n_rows > 0): NGNN_E_ARG; n_rows >= 2^31: NGNN_E_RANGE.
 * col (and w) may be NULL for a CSR without entries.
 *
 * ngnn_gcn_wagg: the weighted neighbour aggregate, for every row r < n_rows
 *   out[r, :F] = bias + dinv[r] * ( sum over the row's entries e, CSR order,
 *                  skipping col[e] == r when loop_w != NULL, of
 *                  (w[e] * dinv[col[e]]) * z[col[e], :F]
 *                  + (loop_w[r] * dinv[r]) * z[r, :F] )
 * w, dinv, loop_w, bias: each nullable.  NULL w: ones; NULL dinv: ones; NULL
 * loop_w: no loop term, and self-loop entries are ordinary entries; NULL
 * bias: zeros.  z: [n_src, ldz] fp32 with col < n_src; with loop_w the row
 * itself is read, so n_src >= n_rows.  fp32 accumulation in that fixed order,
 * the loop term last, every product entering by a fused multiply-add and the
 * additions compensated (Kahan: a row of a thousand equal terms would
 * otherwise miss the fp32 bar by itself): bitwise reproducible.  One group of 4..64 lanes
 * (the power of two at or above F / vector width) owns a row, a hub row
 * included (its order stays fixed; its time is its degree's); the lanes load
 * col, w and dinv[col] together and broadcast them; four gathered rows are in
 * flight per lane; 16-B loads when F, ldz, ldo and the bases allow, 8-B or
 * 4-B otherwise.  Plain vector stores, no atomics.  Row offsets are 64-bit.
 * The coefficient of an edge is symmetric in its ends, so the input gradient
 * is the same call on the source-grouped CSR with w permuted to that order
 * and no bias.
 * Before any launch: n_rows or F < 0, a NULL rowptr, a NULL z or out with
 * n_rows > 0 and F > 0: NGNN_E_ARG; ldz or ldo < F: NGNN_E_SHAPE; n_rows or
 * F >= 2^31: NGNN_E_RANGE. */
int ngnn_gcn_norm(const int32_t *rowptr, const int32_t *col, const float *w, int64_t n_rows,
                  int add_self_loops, float *dinv, float *loop_w, void *stream);
int ngnn_gcn_wagg(const float *z, int64_t ldz, int64_t F, const int32_t *rowptr, const int32_t *col,
                  const float *w, const float *dinv, const float *loop_w, const float *bias,
                  int64_t n_rows, float *out, int64_t ldo, void *stream);

/* ------------------------------------------ fused ReLU-BatchNorm-dropout
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * nn.BatchNorm1d over the n_rows nodes of x [n_rows, ldx] fp32 (columns: the
 * F features), with the ReLU in front of it and the hash dropout behind it
 * folded in: what SAGE / SAGEPL(use_bn=True) run per hidden layer
 * (DESIGN.md section 5o).  a = relu(x) when relu != 0, else x; torch's relu: a
 * NaN stays a NaN.
 *
 * ngnn_bn_fwd_train: out = drop(gamma * (a - mean) * invstd + beta), mean and
 *   var the per-column batch mean and BIASED variance of a, invstd =
 *   1 / sqrt(var + eps).  drop is ngnn_device.h::Dropout on
 *   (seed ^ *seed_dev, row, column) (seed_dev nullable): keep threshold
 *   ceil(p_drop * 256), survivors scaled by 256 / (256 - thresh), p_drop = 0.5
 *   in bit form; a dropped element is +0.0, p_drop = 0 is no dropout, 1 drops
 *   everything.  mean[F] and invstd[F] are saved for ngnn_bn_bwd, and with
 *   them mean_lo[F] = the fp64 mean minus its fp32 rounding: the kernels
 *   subtract the pair, (a - mean) - mean_lo, because fp32 alone holds a mean
 *   of 4096 to 2.4e-4, which would be the error of that column's every
 *   output (torch's CPU BatchNorm, the yardstick, normalises in fp64).  The running
 *   statistics move on the device as nn.BatchNorm1d's: running_mean =
 *   (1 - m) running_mean + m mean, running_var likewise with the UNBIASED
 *   var n / (n - 1), *num_batches_tracked += 1; m = momentum, or, momentum < 0
 *   (torch's None), 1 / num_batches_tracked after the increment.
 *   Statistics: never E[a^2] - E[a]^2.  Every thread takes eight rows' mean
 *   and squared deviations around it; chunks, lane groups, the slabs of
 *   ngnn_bn_slab_rows() rows (one (mean, M2) partial per slab and column in
 *   ws; counts follow from the indices) and the finalise kernel's slab lanes
 *   are merged by Chan's formula in one fixed order in fp64, then rounded once
 *   to fp32: no atomics, bitwise reproducible.  Three launches (partials,
 *   finalise, apply); ws holds ngnn_bn_workspace_bytes(n_rows, F) bytes,
 *   8-byte aligned.
 * ngnn_bn_fwd_eval: out = gamma * (a - running_mean) / sqrt(running_var + eps)
 *   + beta, one launch, nothing updated, no dropout.
 * ngnn_bn_bwd: with g = dout * keep * scale (the keep mask regenerated from
 *   the same seed pair) and xhat = (a - mean) * invstd:
 *     dbeta = sum_r g, dgamma = sum_r g * xhat (fp64 sums in the forward's
 *     fixed order, rounded once),
 *     dx = [relu: x > 0] gamma invstd (g - dbeta / n - xhat dgamma / n).
 *   dx == NULL skips the dx launch (an input that needs no gradient).  At
 *   most three launches; the same workspace size.
 * A NaN in a column makes that column's statistics, outputs, running
 * statistics and gradients NaN and leaves every other column alone.
 * 16-B accesses when F, every leading dimension and every base allow, 4-B
 * otherwise; consecutive lanes take consecutive columns.
 * Before any launch: n_rows < 2 (train, bwd: no batch statistics of one row),
 * n_rows < 0 (eval), F <= 0, a NULL required pointer, p_drop outside [0, 1],
 * eps < 0, momentum > 1: NGNN_E_ARG; a leading dimension < F: NGNN_E_SHAPE;
 * n_rows > 2^31 - 257 or F > 2^20: NGNN_E_RANGE; ws NULL, misaligned or too
 * small: NGNN_E_WORKSPACE.  ngnn_bn_fwd_eval with n_rows == 0: success. */
int ngnn_bn_slab_rows(void);
size_t ngnn_bn_workspace_bytes(int64_t n_rows, int64_t F);
int ngnn_bn_fwd_train(const float *x, int64_t ldx, int64_t n_rows, int64_t F, int relu, const float *gamma,
                      const float *beta, double eps, double momentum, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked, float p_drop, uint64_t seed, const uint64_t *seed_dev,
                      float *out, int64_t ldo, float *mean, float *mean_lo, float *invstd, void *ws,
                      size_t ws_bytes, void *stream);
int ngnn_bn_fwd_eval(const float *x, int64_t ldx, int64_t n_rows, int64_t F, int relu, const float *gamma,
                     const float *beta, double eps, const float *running_mean, const float *running_var,
                     float *out, int64_t ldo, void *stream);
int ngnn_bn_bwd(const float *dout, int64_t ldg, const float *x, int64_t ldx, int64_t n_rows, int64_t F, int relu,
                const float *gamma, const float *mean, const float *mean_lo, const float *invstd, float p_drop,
                uint64_t seed, const uint64_t *seed_dev, float *dgamma, float *dbeta, float *dx, int64_t ldd,
                void *ws, size_t ws_bytes, void *stream);

/* ----------------------------------- hidden-state tap of the fused SAGE stack
 * Added within ABI 22 (new entries only: nothing existing changed, so the
 * version did not move).
 *
 * A stack that hands out h = relu(conv_{L-2}(...)) BEFORE dropout next to its
 * logits (the reference's SAGEH and SAGEPL) runs that
 * layer through ngnn_sage_fwd_raw with relu = 1, p_drop = 0 and applies the
 * dropout with ngnn_dropout_rows; its backward folds the gradient that
 * arrives at h into the layer's dz with ngnn_tap_grad.
 *
 * ngnn_dropout_rows: for rows r < min(n_rows, *n_rows_dev) (n_rows_dev
 *   nullable) and columns c < F
 *     out[r, c] = keep(r, c) ? h[r, c] * scale : +0.0
 *   keep and scale are ngnn_device.h::Dropout's on (seed ^ *seed_dev, r, c)
 *   (seed_dev nullable), r and c counted from the tensor's first row and
 *   column: the mask and the one product of ngnn_sage_fwd_raw's epilogue, so
 *   with h what that call stores for (relu = 1, p_drop = 0), out is bit for
 *   bit what the same call stores for (relu = 1, p_drop, seed, seed_dev).
 *   (One exception, never met by a computed activation: the row-tile
 *   kernel's p_drop = 0.5 form takes ReLU as an integer max and so stores +0.0
 *   where h is -0.0 or a negative-signed NaN; here such an h keeps its sign.)
 *   p_drop = 0 copies, p_drop = 1 stores +0.0 everywhere.  out must not alias
 *   h.  Rows at or past the bound and columns F .. ldo - 1 are not written.
 * ngnn_tap_grad: for rows r < min(n_rows, *r_ptr) (r_ptr nullable)
 *     dz = dy * [xd > 0] * yscale + dh * [h > 0]
 *   The first term is ngnn_sage_wgrad's dz for y = xd (ReLU + dropout
 *   backward), the second the ReLU backward of the gradient dh that reached
 *   the tapped h.  xd == NULL (no dropout: xd would be h):
 *   dz = (dy + dh) * [h > 0], yscale unused.  dy == NULL (nothing read xd):
 *   dz = dh * [h > 0].  dz may alias dy.  Rows at or past the bound are left
 *   untouched.
 * One launch each, no allocation, no host synchronisation (capturable).  A
 * lane group per row (16, 32 or 64 lanes by width); 16-B accesses when every
 * base and leading dimension allows, 4-B otherwise.
 * Before any launch: n_rows or F negative, p_drop outside [0, 1]:
 * NGNN_E_ARG; a leading dimension (of a pointer that is read) < F:
 * NGNN_E_SHAPE; n_rows or F > 2^31 - 1: NGNN_E_RANGE; n_rows == 0 or F == 0:
 * success, no pointer read; then a NULL h / out (dh / h / dz), or out == h:
 * NGNN_E_ARG. */
int ngnn_dropout_rows(const float *h, int64_t ldh, int64_t n_rows, const int32_t *n_rows_dev, int64_t F,
                      float p_drop, uint64_t seed, const uint64_t *seed_dev, float *out, int64_t ldo,
                      void *stream);
int ngnn_tap_grad(const float *dy, int64_t ldy, const float *xd, int64_t ldx, float yscale, const float *dh,
                  int64_t ldg, const float *h, int64_t ldh, int64_t n_rows, const int32_t *r_ptr, int64_t F,
                  float *dz, int64_t ldz, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NGNN_H */
