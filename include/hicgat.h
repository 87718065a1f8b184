/*
 * hicgat.h -- C ABI of libhicgat.so, the MI355X (gfx950) kernels of the GAT-HiC per-epoch step.
 *
 * The reference (beyzoskaya/HiC-GNN, /root/reference) is pure Python: its "native boundary" is the
 * set of third-party torch custom ops that PyG 1.7.2's GATConv, torch.cdist and torch.optim.Adam
 * call.  Each entry point below replaces one group of those ops; the
 * comment on each names the reference call site it stands in for.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator); nothing
 *     is allocated inside; scratch ("workspace") is passed in and sized by the *_workspace_bytes()
 *     query;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the legacy default
 *     stream) and is stream-ordered; no call synchronises the host, so every call can be captured
 *     into a hipGraph;
 *   - return 0 on success or a negative HICGAT_E* code (hicgat_strerror() names it);
 *   - stateless and re-entrant; one process drives one GPU;
 *   - index arrays are int32 (nnz < 2^31), converted once from the reference's int64 when the
 *     adjacency is built; every matrix is row-major with the stated leading dimension.
 */
#ifndef HICGAT_H
#define HICGAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *hicgat_stream_t;

/* loss_kind of the fused distance / loss entry points */
enum { HICGAT_LOSS_MSE = 0, HICGAT_LOSS_COMBINED = 1, HICGAT_LOSS_CONTRASTIVE = 2 };

enum {
  HICGAT_OK = 0,
  HICGAT_EINVAL = -1,   /* bad size / null pointer / misaligned buffer */
  HICGAT_ELAUNCH = -2,  /* hipGetLastError() reported a launch failure */
  HICGAT_EUNSUPPORTED = -3
};

int hicgat_version(void);
const char *hicgat_strerror(int code);

/* ---- a13/a3: graph build -------------------------------------------------------------------
 * Reference: utils.load_input (utils.py:29-73; networkx edges + SparseTensor(...).to_symmetric())
 * followed by torch_sparse.set_diag inside PyG 1.7.2 GATConv.forward.  From a dense row-major
 * N x N contact matrix A (float64, leading dim lda), builds the symmetric CSR of
 * (A[i,j] != 0 || A[j,i] != 0) for i != j, with one self loop (i,i) inserted per row at its sorted
 * position.  Two calls: first with col == NULL to get rowptr (row_counts scratch of N+1 ints is
 * rowptr itself), then with col to fill the columns.  Bit-exact with the reference pattern. */
int hicgat_csr_from_dense(const double *A, int N, int64_t lda, int32_t *rowptr, int32_t *col,
                          void *workspace, size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_csr_workspace_bytes(int N);

/* ---- a12: utils.cont2dist (utils.py:75-80) on the device ------------------------------------
 * dist = (1/y)^factor, diagonal 0, +inf -> max finite, NaN -> 0, divided by the max; float64 in,
 * float32 (or float64) out with leading dimension ldo. workspace: hicgat_cont2dist_workspace_bytes */
int hicgat_cont2dist(const double *y, int N, int64_t ldy, double factor, float *out32, double *out64,
                     int64_t ldo, void *workspace, size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_cont2dist_workspace_bytes(int N);

/* ---- a2: GATConv lin_l + attention logits (PyG 1.7.2 GATConv.forward) ----------------------
 * h [N, H*C] = x [N, F] * W^T (W [H*C, F], lin_l.weight, no bias; lin_r is lin_l) and
 * a_src[n,h] = <h[n,h,:], att_l[h,:]>, a_dst[n,h] = <h[n,h,:], att_r[h,:]>.
 * hicgat_gat_linear_att computes both (fp32 MFMA GEMM with the logits fused in its epilogue);
 * hicgat_gat_att_logits computes only the logits from an existing h. */
int hicgat_gat_linear_att(const float *x, const float *W, const float *att_src, const float *att_dst,
                          int N, int F, int H, int C, float *h, float *a_src, float *a_dst,
                          hicgat_stream_t stream);
int hicgat_gat_att_logits(const float *h, const float *att_src, const float *att_dst, int N, int H,
                          int C, float *a_src, float *a_dst, hicgat_stream_t stream);

/* ---- a4+a5: edge softmax + neighbour aggregation (PyG 1.7.2 GATConv.propagate) --------------
 * CSR rows are destinations i, columns sources j, self loops already present (set_diag).
 *   e_ij = leaky_relu(a_src[j] + a_dst[i], neg_slope)
 *   alpha_ij = exp(e_ij - max_i) / (sum_i + 1e-16)        (torch_geometric.utils.softmax, ptr path)
 *   out[i] = sum_j alpha_ij * h[j] + bias                  (segment_csr sum; concat=True)
 * The operands that the forward and the source pass of the backward (hicgat_gat_agg_bwd_src) share
 * come in four structs; the last two select the form of the pass and are NULL for the plain gather.
 * hicgat_gat_graph: rowptr [N + 1] / col [nnz] and the destination rows [row_begin, row_end) of the
 *   pass (a rank's shard; 0..N on one GPU).  nnz = rowptr[N] (checked >= 0 only, by the forward only).
 * hicgat_gat_feats: h [N, H*C] (lin_l's output), a_src / a_dst [N, H], neg_slope.  Every per-row array
 *   of a pass is indexed by the GLOBAL row id (the neighbour rows of the shard must be present).
 * hicgat_attn_drop: PyG 1.7.2 GATConv(dropout=p), `alpha = F.dropout(alpha, p, training)` in message(),
 *   inside the two gathering passes.  Every alpha_ij of the forward is multiplied, per head, by m_ij in
 *   {0, scale}; the softmax itself (row_stats max / sum, hicgat_gat_alpha) is that of the undropped
 *   row, and self loops are dropped like any other edge.  The mask is a pure function of (seed, step,
 *   site, destination row i, source row j, head), with i and j GLOBAL node ids, so it depends neither
 *   on the launch geometry, nor on the row range, nor on the edge's position -- the source pass
 *   recomputes the bits of edge (i -> r) from (col[e], r) and no [nnz, H] tensor exists.
 *   Philox4x32-10 as under "feature dropout" below:
 *     counter = (i, j, step & 0xffffffff, site | HICGAT_ATTN_SITE_BIT);  key = (seed & 0xffffffff, seed >> 32);
 *     head hh uses output word r[hh] (H <= 4: one call per edge);  kept iff r[hh] >= T,
 *     T = min(floor(p * 2^32), 2^32 - 1);  m = kept ? scale : 0,  scale = (float)(1.0 / (1.0 - p)).
 *   HICGAT_ATTN_SITE_BIT keeps these sites apart from the feature-dropout sites that share a seed and a
 *   step count; the caller's site must be < 2^31.  step = *step_counter when the pointer is given (a
 *   device int64, 8-B aligned; NULL-able), else step_value.  p = 0 keeps everything (scale 1).  p
 *   outside [0, 1) or NaN, site >= 2^31, a misaligned step_counter: HICGAT_EINVAL, before the shape is
 *   looked at.  A gradient that arrives through alpha itself (hicgat_gat_alpha_bwd_*) sees no mask:
 *   PyG returns the pre-dropout alpha.  The dense-tile, aggregate-first (hicgat_xagg_*) and stand-alone
 *   destination (hicgat_gat_agg_bwd_dst) forms have no dropout: drop together with tiles is HICGAT_EINVAL.
 * hicgat_gat_tiles: the dense-tile form (gat_tiles.hip; formerly hicgat_gat_agg_fwd_tiled and its
 *   source-pass twin), the same results (fp32; the tiles' sums are added in another order) with the dense part of the graph on
 *   the matrix cores, H == 2 and C == 256 only (else HICGAT_EUNSUPPORTED).  The edge set is split in two:
 *     tiles: rows [row_begin, row_end) in blocks of 32 (block b = rows row_begin + 32b ..);
 *       tptr [nrb + 1] (nrb = ceil((row_end - row_begin) / 32)) indexes tcol [ntiles] (a 32-column
 *       block: columns 32*tcol[t] ..) and tmask [ntiles * 32] (bit c of word 32t + i: the edge
 *       (row_begin + 32b + i, 32*tcol[t] + c) exists); tiles of a block in any order, each edge in at
 *       most one tile;
 *     rowptr_s / col_s: the CSR (N + 1 row pointers, rows of the range) of every OTHER edge.
 *   The graph's rowptr / col (the whole rows) give the forward its softmax statistics; the source pass
 *   reads only rowptr_s / col_s, and the graph's two may be NULL there.  The tiles' products run as
 *   dense 32 x 32 x 32 x 512 blocks on v_mfma_f32_32x32x2_f32 (weights 0 off the edge set).  Built
 *   from the CSR by hicgat.graph.build_tiles (a 32x32 tile is dense when it holds >= min_edges edges).
 *   splits (1..64): the tiles of a row block are spread over `splits` workgroups (a graph with few row
 *   blocks, e.g. a dense 2000-node map: 63); splits > 1 needs a 16-B aligned workspace of
 *   hicgat_gat_tiled_workspace_bytes(row_end - row_begin, splits) bytes for the partial sums, which
 *   one more pass adds in split order. */
typedef struct {
  const int32_t *rowptr, *col;
  int N, nnz, row_begin, row_end;
} hicgat_gat_graph;
typedef struct {
  const float *h, *a_src, *a_dst;
  int H, C;
  float neg_slope;
} hicgat_gat_feats;
#define HICGAT_ATTN_SITE_BIT 0x80000000u
enum { HICGAT_ATTN_SITE_MAX = 0x7fffffff };   /* the largest site a caller may pass */
typedef struct {
  double p;
  uint64_t seed;
  const int64_t *step_counter;
  int64_t step_value;
  uint32_t site;
} hicgat_attn_drop;
typedef struct {
  const int32_t *rowptr_s, *col_s, *tptr, *tcol;
  const uint32_t *tmask;
  int ntiles, splits;
  void *workspace;
  size_t workspace_bytes;
} hicgat_gat_tiles;
size_t hicgat_gat_tiled_workspace_bytes(int rows, int splits);
/* The forward: out [N, H*C] (rows of the range written) and row_stats [N, 4H] = (max[H], sum[H],
 * delta[H], da_dst[H]) -- max/sum written here, delta/da_dst by the backward's destination pass.
 * Supported: C % 128 == 0, H*C a multiple of 256, H*C <= 1024, H <= 4
 * (every GATConv of models.py: (H, C) = (1, 256), (1, 512), (2, 128), (2, 256), (2, 512), (4, 256), ...);
 * other shapes return HICGAT_EUNSUPPORTED.  H == 2, C == 256 (the flagship's GATConv(512, 256,
 * heads=2), models.py:619) has entry kernels and launch parameters of its own around the per-row bodies
 * that every shape shares (gat_agg.hpp); one dispatcher (gat_launch.hpp) launches both kinds.
 * The same set holds for hicgat_gat_agg_bwd_dst, hicgat_gat_agg_bwd_rows and hicgat_gat_agg_bwd_src;
 * the aggregate-first (hicgat_xagg_*) forms stay H == 2, C == 256.
 * bias [H*C].  act = 1 writes out = relu(sum + bias) (the relu that follows the GATConv at
 * models.py:637), act = 0 the plain sum + bias (inference: act = 0, out2 = NULL); any other act:
 * HICGAT_EINVAL.  out2 != NULL (training) also writes, from the same gathered rows, out2 [N, H*C] =
 * sum_j alpha_ij lrelu'(e_ij) h_j and S3[i,h] = sum_j alpha_ij lrelu'(e_ij) into row_stats[i, 2H..3H)
 * -- the inputs that let hicgat_gat_agg_bwd_rows form the destination half of the backward without a
 * gather.  No pointer but out2, drop and tiles may be NULL (graph and feats neither: HICGAT_EINVAL); an
 * empty row range is a no-op that looks at no pointer inside or beside the structs.
 *   drop: out[i] = sum_j alpha_ij m_ij h[j] + bias (then relu, act = 1), out2[i] =
 *     sum_j alpha_ij lrelu'(e_ij) m_ij h[j] (masked) and S3[i] = sum_j alpha_ij lrelu'(e_ij) (NOT masked).
 *   tiles: the gather computes each row's statistics over ALL its edges and the sums of the remainder;
 *     the tile kernel adds the tiles' products and applies bias / relu.  S3 as without tiles. */
int hicgat_gat_agg_fwd(const hicgat_gat_graph *graph, const hicgat_gat_feats *feats, const float *bias, int act,
                       float *out, float *out2, float *row_stats, const hicgat_attn_drop *drop,
                       const hicgat_gat_tiles *tiles, hicgat_stream_t stream);

/* ---- a10 (part): backward of a4+a5 ----------------------------------------------------------
 * Pass 1 (destination side, rows of the range):  g_ij = <dout[i,h,:], h[j,h,:]>,
 *   delta[i,h] = sum_j alpha_ij g_ij,  da_dst[i,h] = sum_j alpha_ij lrelu'(e_ij) (g_ij - delta[i,h])
 *   -> row_stats[i, 2H..4H).
 * Pass 2 (source side, rows r of the range; the graph is symmetric so N(r) lists every i that
 *   has r as a neighbour; needs dout, row_stats of all those i):
 *   dh[r] = sum_i alpha_ir dout[i] + da_src[r] (x) att_l + da_dst[r] (x) att_r,
 *   da_src[r,h] = sum_i alpha_ir lrelu'(e_ir) (g_ir - delta[i,h]).
 * Requires a structurally symmetric CSR (utils.py:71 to_symmetric guarantees it).
 * Supported shapes: as hicgat_gat_agg_fwd (every pass; ld_stats >= 4H and a multiple of 4). */
int hicgat_gat_agg_bwd_dst(const int32_t *rowptr, const int32_t *col, int N, int H, int C,
                           int row_begin, int row_end, const float *h, const float *a_src,
                           const float *a_dst, const float *dout, float neg_slope,
                           float *row_stats, hicgat_stream_t stream);
/* Pass 1 without a gather, after hicgat_gat_agg_fwd with out2 (same row_stats):
 *   dout = g * [y > 0] (act = 1, written to dout with row stride ld_dout floats; torch's relu
 *   backward on the output y) or g
 *   (act = 0, dout unused); delta = <dout, y - bias>; da_dst = <dout, out2> - delta * S3,
 * per row of the range and head -> row_stats[i, 2H..4H) exactly as hicgat_gat_agg_bwd_dst. */
int hicgat_gat_agg_bwd_rows(int N, int H, int C, int row_begin, int row_end, int act, const float *g,
                            const float *y, const float *bias, const float *out2, float *dout,
                            int64_t ld_dout, float *row_stats, hicgat_stream_t stream);
/* Pass 2 (above): dh [N, H*C] and da_src [N, H], rows of the range written.  Row i of dout is at
 * dout + i*ld_dout and of row_stats at row_stats + i*ld_stats (floats; ld_dout >= H*C, ld_stats >= 4H,
 * both multiples of 4, else HICGAT_EINVAL): contiguous tensors pass H*C and 4H, hicgat.dist one
 * all-gathered [dout | row stats] buffer per row.  att_src / att_dst [H, C].  graph, feats, drop and
 * tiles as for the forward; no other pointer may be NULL.  flags: 0, or HICGAT_SRC_ROUND_ROBIN, which
 * spreads consecutive row blocks over the XCDs instead of giving each XCD a contiguous row range (the
 * multi-GPU "slab" pass, hicgat.dist, whose heavy rows are one contiguous block); any other bit, or the
 * flag together with tiles: HICGAT_EINVAL.
 *   drop: the forward's keep factors recomputed,
 *     dh[r] = sum_i alpha_ir m_ir dout[i] + da_src[r] (x) att_l + da_dst[r] (x) att_r,
 *     da_src[r] = <sum_i alpha_ir s_ir m_ir dout_i, h_r> - sum_i alpha_ir s_ir delta_i   (s = lrelu').
 *     hicgat_gat_agg_bwd_rows is unchanged: delta_i = <dout_i, out_i - bias> = sum_k alpha_ik m_ik g_ik
 *     and da_dst_i = <dout_i, out2_i> - delta_i S3_i are the dropped layer's.
 *   tiles: the gather writes the remainder's shares of dh and da_src; the tile kernel adds the tiles'
 *     products (the graph is symmetric, so a row block's tiles are also those of the transposed
 *     product) and finishes dh (logit terms) and da_src. */
enum { HICGAT_SRC_ROUND_ROBIN = 1 };
int hicgat_gat_agg_bwd_src(const hicgat_gat_graph *graph, const hicgat_gat_feats *feats, const float *row_stats,
                           int64_t ld_stats, const float *dout, int64_t ld_dout, const float *att_src,
                           const float *att_dst, float *dh, float *da_src, int flags,
                           const hicgat_attn_drop *drop, const hicgat_gat_tiles *tiles, hicgat_stream_t stream);
/* mask[e * H + hh] = kept ? 1 : 0 (uint8 [nnz, H], self-looped CSR order) from the device function the
 * two passes use (tests, tools).  N < 0, a NULL drop or one the passes refuse: HICGAT_EINVAL;
 * 1 <= H <= 4, else HICGAT_EUNSUPPORTED; N == 0 is a no-op. */
int hicgat_gat_attn_mask(const int32_t *rowptr, const int32_t *col, int N, int H, const hicgat_attn_drop *drop,
                         uint8_t *mask, hicgat_stream_t stream);

/* ---- the attention weights as an output, and their backward (gat_attn.hip) ---------------------
 * Reference: PyG 1.7.2 GATConv.forward(x, edge_index, return_attention_weights=True), which
 * models.py:1122 calls: alpha [nnz, H] in the order of the self-looped CSR, an autograd tensor there.
 * Same CSR, a_src / a_dst [N, H] and row_stats [N, 4H] as the aggregation above, same supported
 * (H, C) set (other shapes: HICGAT_EUNSUPPORTED).  One wave per row, no atomics, fixed summation order.
 *   hicgat_gat_transpose_map: tmap[e(r, i)] = e(i, r) over the CSR (a binary search per edge in row
 *     i's sorted columns); its own inverse, the identity on the self loops; -1 where (i, r) is
 *     missing (the CSR is not structurally symmetric).  Built once per graph.
 *   hicgat_gat_alpha: alpha[e, h] = exp(lrelu(a_src[j] + a_dst[i]) - max_i) / (sum_i + 1e-16) from
 *     row_stats[i, 0..2H) (after hicgat_gat_agg_fwd or its tiled form); gathers no h rows.
 * For G = dL/dalpha [nnz, H], with s = lrelu'(a_src[j] + a_dst[i]):
 *   hicgat_gat_alpha_bwd_dst, row i: c[i, h] = sum_j alpha_ij G_ij and
 *     da_dst_g[i, h] = sum_j alpha_ij s_ij (G_ij - c[i, h])            (both [N, H], written).
 *   hicgat_gat_alpha_bwd_src, row r: ds = sum_e alpha[t] s (G[t] - c[col[e]]), t = tmap[e], then IN
 *     PLACE dh[r] += ds (x) att_src + da_dst_g[r] (x) att_dst, da_src[r] += ds,
 *     row_stats[r, 3H..4H) += da_dst_g[r].  Runs after hicgat_gat_agg_bwd_src (or its tiled form) and
 *     before hicgat_gat_param_grad, which then sees the totals.
 * The two backward passes read alpha as hicgat_gat_alpha wrote it. */
int hicgat_gat_transpose_map(const int32_t *rowptr, const int32_t *col, int N, int32_t *tmap,
                             hicgat_stream_t stream);
int hicgat_gat_alpha(const int32_t *rowptr, const int32_t *col, int N, int H, int C, const float *a_src,
                     const float *a_dst, const float *row_stats, float neg_slope, float *alpha,
                     hicgat_stream_t stream);
int hicgat_gat_alpha_bwd_dst(const int32_t *rowptr, const int32_t *col, int N, int H, int C, const float *a_src,
                             const float *a_dst, const float *alpha, const float *G, float neg_slope, float *c,
                             float *da_dst_g, hicgat_stream_t stream);
int hicgat_gat_alpha_bwd_src(const int32_t *rowptr, const int32_t *col, const int32_t *tmap, int N, int H, int C,
                             const float *a_src, const float *a_dst, const float *alpha, const float *G,
                             const float *c, const float *da_dst_g, const float *att_src, const float *att_dst,
                             float neg_slope, float *dh, float *da_src, float *row_stats, hicgat_stream_t stream);

/* ---- GATConv in aggregate-first order (gat_xagg.hip; the multi-GPU "xagg" step of hicgat.dist) ----
 * Reference: the same PyG 1.7.2 GATConv (models.py:619) -- out_i^h = W_h (sum_j alpha_ij^h x_j) +
 * b^h and a_src_j^h = <W_h^T att_src^h, x_j> are the h-first expressions regrouped, so a rank that
 * owns destination rows needs no other rank's h and runs every GEMM on its own rows.  F = 512,
 * H = 2, C = 256 only.  Row ranges [row_begin, row_end) are the rank's rows of a CSR in global
 * numbering whose rowptr[row_begin] = 0 (hicgat.dist.ShardPlan.own_csr); per-row outputs marked
 * "local" are indexed i - row_begin, row_stats by the global row.
 *   hicgat_xagg_logits: vec [4][512] = W_h^T att_src^h (h = 0, 1), W_h^T att_dst^h; a_src / a_dst
 *     [N][2] = x . vec for all N rows (workspace vec: hicgat_xagg_vec_bytes()).  Its first launch
 *     can carry the step's other first-launch work, each part selected by a pointer (NULL: left out):
 *     zero_buf (16-B aligned; zero_n = 0 with NULL): zero_buf[0, zero_n) = 0, a step's flat gradient
 *     buffer (the optimizer's zero_grad, HiC-GNN_main.py:124);  step_counter: the optimizer's device
 *     step count += 1 (the step's Adam then calls hicgat_adam_step_table with counted = 1);  pack: the
 *     head-fused tail's packed weights of W1c, W2c and Wh = W (hicgat_tail_pack's layout and
 *     pack_bytes rule; W1c / W2c are read only with pack), so the sharded step's tail kernels need no
 *     pack launch of their own.  Logits alone: NULL, 0, NULL, NULL, NULL, NULL, 0.
 *   hicgat_xagg_fwd: softmax statistics (row_stats [N][8]: max, sum at [0:4], S3 at [4:6]) and
 *     X4 [2 heads][2 kinds][rows][512] (local): kind 0 xa = sum alpha x_j, kind 1 xa2 = sum alpha
 *     lrelu'(e) x_j.  The caller then forms [out; out2] per head = [xa; xa2] W_h^T (hicgat_gemm).
 *   hicgat_xagg_bias_relu: y0 += bias, o = relu(y0) over [rows][512].
 *   hicgat_xagg_rows_bwd: own rows (local row_stats view): dout = g [y0 > 0] (act 1) or g,
 *     delta^h = <dout^h, y0^h - bias^h> into row_stats[4:6]; the forward's S3 moves to [6:8].
 *   hicgat_xagg_edge: ds [nnz_own][2] (the rank's CSR order) = alpha lrelu'(e) (<dxa_i^h, x_j> -
 *     delta_i^h), dxa [rows][1024] (local; head h at columns 512h = dout_i^h W_h), delta from
 *     row_stats[i][4:6]; with xa2 (X4's kind-1 planes: X4 + rows*512) also da_dst^h =
 *     <dxa_i^h, xa2_i^h> - delta_i^h S3_i^h into row_stats[i][6:8] (S3 read from there).
 *   hicgat_xagg_slab_sum: da_src [N][2], da_src_j = sum over the slab entries k of row j
 *     (rowptr_s, N + 1) of ds[perm[k]] (perm: the rank's CSR index of the transposed edge), and
 *     g_src [2][512] = sum_j da_src_j^h x_j (x: all N rows), fixed-order partial sums
 *     (workspace hicgat_xagg_slab_workspace_bytes()).
 *   hicgat_xagg_param_finish: dW[256h + c][:] += att_src^h[c] g_src[h][:] + att_dst^h[c] g_dst[h][:],
 *     datt_src^h[c] += <W[256h + c][:], g_src[h][:]>, datt_dst likewise, where g [2][512] = sum_j
 *     da_j^h x_j is given in `segs` >= 1 segments (the segmented column sums of
 *     hicgat_param_grads_grouped): g_src = sum over s of g_src + s * seg_stride (floats; >= 1024 when
 *     segs > 1), g_dst likewise, added in segment order.  One flat g: segs = 1, seg_stride = 0. */
size_t hicgat_xagg_vec_bytes(void);
int hicgat_xagg_logits(const float *x, const float *W, const float *att_src, const float *att_dst, int N, int F,
                       int H, int C, float *vec, float *a_src, float *a_dst, float *zero_buf, int64_t zero_n,
                       int64_t *step_counter, const float *W1c, const float *W2c, void *pack, size_t pack_bytes,
                       hicgat_stream_t stream);
int hicgat_xagg_fwd(const int32_t *rowptr, const int32_t *col, int N, int F, int H, int C, int row_begin,
                    int row_end, const float *x, const float *a_src, const float *a_dst, float neg_slope, float *X4,
                    float *row_stats, hicgat_stream_t stream);
int hicgat_xagg_bias_relu(float *y0, const float *bias, float *o, int rows, int D, hicgat_stream_t stream);
int hicgat_xagg_rows_bwd(int rows, int D, int act, const float *g, const float *y0, const float *bias, float *dout,
                         float *row_stats, hicgat_stream_t stream);
int hicgat_xagg_edge(const int32_t *rowptr, const int32_t *col, int N, int F, int H, int C, int row_begin,
                     int row_end, const float *x, const float *a_src, const float *a_dst, float *row_stats,
                     const float *dxa, const float *xa2, float neg_slope, float *ds, hicgat_stream_t stream);
/* The edge pass with the source side folded in (replaces hicgat_xagg_edge + hicgat_xagg_slab_sum in
 * the sharded step): g_src^h = sum_j da_src_j^h x_j = sum over the own rows' edges (i, j) of
 * ds_ij^h x_j, formed in the pass that computes ds_ij; written as hicgat_xagg_edge_acc_blocks(rows)
 * partial rows gpart [blocks][1024] (head 0 | head 1) whose column sums are g_src (e.g. a
 * hicgat_param_grads_grouped column-sum job); with xa2, da_dst into row_stats[6:8] as hicgat_xagg_edge.
 * Deterministic (fixed row-to-block map and summation order). */
int hicgat_xagg_edge_acc(const int32_t *rowptr, const int32_t *col, int N, int F, int H, int C, int row_begin,
                         int row_end, const float *x, const float *a_src, const float *a_dst, float *row_stats,
                         const float *dxa, const float *xa2, float neg_slope, float *gpart, hicgat_stream_t stream);
int hicgat_xagg_edge_acc_blocks(int rows);
size_t hicgat_xagg_slab_workspace_bytes(void);
int hicgat_xagg_slab_sum(const int32_t *rowptr_s, const int32_t *perm, int N, const float *ds, const float *x,
                         float *da_src, float *g_src, void *workspace, size_t workspace_bytes,
                         hicgat_stream_t stream);
int hicgat_xagg_param_finish(const float *W, const float *att_src, const float *att_dst, const float *g_src,
                             const float *g_dst, int segs, int64_t seg_stride, int F, int H, int C, float *dW,
                             float *datt_src, float *datt_dst, hicgat_stream_t stream);

/* Column reductions for the GATConv parameter gradients over N rows (pass pointers offset to a
 * shard's first row for a partial sum; deterministic, two-stage):
 *   datt_src[h,c] = sum_n da_src[n,h] h[n,h,c];  datt_dst likewise with row_stats' da_dst;
 *   dbias[c] = sum_n dout[n,c].  workspace: hicgat_gat_param_grad_workspace_bytes(N, H*C).
 * Any of datt_src / datt_dst / dbias may be NULL (that part is skipped, and the inputs only it
 * reads may be NULL too): datt_dst and dbias need no source-pass output, so they can be summed
 * beside that pass; each part is bitwise the same whichever subset is asked for. */
int hicgat_gat_param_grad(const float *h, const float *dout, const float *da_src,
                          const float *row_stats, int N, int H, int C, float *datt_src,
                          float *datt_dst, float *dbias, int accumulate, void *workspace,
                          size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_gat_param_grad_workspace_bytes(int N, int D);

/* ---- a7: torch.cdist(c, c, p=2) (models.py:661) and its backward -----------------------------
 * D[i,j] = ||c_i - c_j||_2 (exact formula; the diagonal is exactly 0), ld = leading dim of D.
 * Backward: dc_i = sum_j (G_ij + G_ji) (c_i - c_j) / D_ij over D_ij != 0 (torch's
 * _euclidean_dist_backward masks res == 0).  workspace: hicgat_pairdist_workspace_bytes(N, HICGAT_PD_SQUARE). */
int hicgat_pairdist_fwd(const float *coords, int N, float *D, int64_t ldd, hicgat_stream_t stream);
int hicgat_pairdist_bwd(const float *coords, const float *G, int N, int64_t ldg, float *dcoords,
                        void *workspace, size_t workspace_bytes, hicgat_stream_t stream);

/* ---- a7+a8+a9 fused: distance + MSE + Pearson moments + d(MSE)/dcoords, D never stored ------
 * Reference: out = cdist(coords) (models.py:661); MSELoss()(out, truth) (HiC-GNN_main.py:127);
 * pearsonr / alpha / total (HiC_GAT_generalize_directly.py:210-225).  T is the SYMMETRIC truth or a
 * BAND of it (a rank's share, hicgat.dist): rows [t_row0, t_row0 + t_rows) and columns [t_col0,
 * t_col0 + ldt) of the N x N truth, element (i, j) at T[(i - t_row0) * ldt + (j - t_col0)]; the whole
 * truth is t_row0 = 0, t_rows = N, t_col0 = 0, ldt >= N.  Only upper-triangle tiles [tile_begin,
 * tile_end) of the 128x128 tiling are read (pass 0, -1 for all); the band must cover every pair of
 * the tile range: rows of its tile-rows I0..I1 and columns from I0*128 on, ldt >= N - t_col0 (else
 * HICGAT_EINVAL).  dcoords may be NULL (no gradient).  Outputs:
 *   stats[12] (float64): 0 sum_{i<j}(d-t)^2, 1 sum d, 2 sum d^2, 3 sum dt, 4 sum t, 5 sum t^2,
 *     6 sum_i T_ii^2 (moments 0..6 over the tile range; a multi-GPU caller all-reduces them and
 *     calls hicgat_pairdist_finalize), 7 mse = (2*[0] + [6])/N^2, 8 pearson r over i<j,
 *     9 alpha = min(1, 0.1 + 1/(mse + 1e-6)), 10 total = mse + alpha*(1 - r), 11 reserved;
 *   loss_kind 0 (the MSE of HiC-GNN_main.py) forms moments 0 and 6 only: 1..5 are 0, r (8) is NaN
 *     and 9..10 are not meaningful; loss_kind 1 (combined loss) forms all of them;
 *   loss_kind 2 (HICGAT_LOSS_CONTRASTIVE, train_and_test_same_res_GAT_node2vec.py:107-134:
 *     0.1 * mean_{i<j} |T_ij - D_ij|) forms moment 0 = sum_{i<j} |d - t| only (6 = 0: no diagonal
 *     term); finalized: 7 = mean |d - t| (fp64), 8 = NaN, 9 = 0.1, 10 = total = 0.1 * [7];
 *   loss[1] (float32): mse (loss_kind 0), total (loss_kind 1) or fp32(total) (loss_kind 2);
 *   dcoords [N,3] = d(loss)/dcoords restricted to the tile range (sum over ranks = full gradient):
 *     d(mse) (loss_kind 0, 1: the Pearson term carries no gradient in the reference) or
 *     float32(0.1 / M) * sum_j sign(d_ij - t_ij) (c_i - c_j) / d_ij, sign(0) = 0 (loss_kind 2).
 * workspace: hicgat_pairdist_workspace_bytes(N, HICGAT_PD_TRI). */
int hicgat_pairdist_mse_fused(const float *coords, const float *T, int N, int64_t ldt, int64_t t_row0,
                              int64_t t_rows, int64_t t_col0, int64_t tile_begin, int64_t tile_end,
                              int loss_kind, double *stats, float *loss, float *dcoords, void *workspace,
                              size_t workspace_bytes, hicgat_stream_t stream);
/* stats[7..11] and loss from the (all-reduced) moments stats[0..6], as above. */
int hicgat_pairdist_finalize(int N, int loss_kind, double *stats, float *loss, hicgat_stream_t stream);
/* hicgat_pairdist_finalize + dcoords[r][c] = (float)dc64[r][c] for rows [row_begin, row_end) of the
 * (all-reduced) fp64 coordinate gradient [N][3], in one launch (a rank's rows for its tail backward;
 * dc64 / dcoords may be NULL for an empty range).  With cbuf (NULL: none, then gidx and cglob are
 * unused; the padded all-gather coordinates [P*R][3]) also cglob[i] = cbuf[gidx[i]] (i < N: the
 * coordinates in global row order, hicgat.dist's step() output) in the same launch. */
int hicgat_pairdist_finalize_rows(int N, int loss_kind, double *stats, float *loss, const double *dc64,
                                  int row_begin, int row_end, float *dcoords, const float *cbuf,
                                  const int32_t *gidx, float *cglob, hicgat_stream_t stream);
/* Tile count and workspace of the two tilings, mode HICGAT_PD_TRI (the fused loss: upper-triangle
 * 128x128 tiles, nb(nb+1)/2) or HICGAT_PD_SQUARE (hicgat_pairdist_bwd: nb*nb), nb = ceil(N/128). */
enum { HICGAT_PD_SQUARE = 0, HICGAT_PD_TRI = 1 };
int64_t hicgat_pairdist_num_tiles(int N, int mode);
size_t hicgat_pairdist_workspace_bytes(int N, int mode);
/* The same fused loss (same reference call sites; stats / loss / dcoords as above) for a truth given
 * in BACKGROUND form: T[i][j] = background for i != j except at the support -- a symmetric CSR
 * (rowptr [N+1], sorted col, val = T there, no diagonal entries) -- and T[i][i] = diag[i].
 * cont2dist's target (utils.py:75-80) is of this form with background 1 (zero contacts: inf -> max
 * -> 1) and the support = the contacts, so the O(N^2) pass reads no truth at all: it takes every
 * pair at the background value and a pass over the support adds the difference (same sums up to
 * fp32 / fp64 reassociation).  Build the form with hicgat_truth_support.
 * The call covers a SHARE of the pairs: the bulk over the upper-triangle tiles [tile_begin,
 * tile_end) and the support rows [support_row_begin, support_row_end) (their entries j != i and
 * their diagonal); 0, -1, 0, N is the whole loss on one GPU.  For a rank of hicgat.dist, stats[0..6]
 * and dcoords [N,3] are its share's partial sums (the sum over shares that cover every tile and
 * every row once is the whole loss: the caller all-reduces stats[0..6] + dcoords and calls
 * hicgat_pairdist_finalize).
 * cmap (NULL: row g of coords is global row g): cmap [N] maps global row g to its row in coords (the
 * sharded step's padded [P*R, 3] all-gather buffer, so no reorder launch before the loss).
 * dcoords / dcoords64: either may be NULL.  dcoords64 (instead of dcoords): the same fp32 gradient
 * values widened to fp64, e.g. right behind stats[12] in one fp64 buffer that the caller all-reduces
 * as a whole; with dcoords64 and at most 4096 tiles + support blocks in the share, stats[7..11] and
 * loss are not written (the caller's finalize after the all-reduce sets them).
 * workspace: hicgat_pairdist_support_workspace_bytes(N). */
int hicgat_pairdist_mse_fused_support(const float *coords, const int32_t *cmap, int N, float background,
                                      const int32_t *rowptr, const int32_t *col, const float *val,
                                      const float *diag, int64_t tile_begin, int64_t tile_end,
                                      int support_row_begin, int support_row_end, int loss_kind,
                                      double *stats, float *loss, float *dcoords, double *dcoords64,
                                      void *workspace, size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_pairdist_support_workspace_bytes(int N);
/* ---- moment-dependent distance losses: the gradient weight of a pair depends on the global moments ----
 * mloss_kind (T symmetric, M = N(N-1)/2 pairs i < j, "all entries" = the N^2 entries with D_ii = 0):
 *   HICGAT_MLOSS_PEARSON: mse + alpha * (1 - r), mse the all-entries mean of (D - T)^2, r Pearson over
 *     the pairs, alpha the caller's fixed weight; the gradient goes through both terms.  A variance
 *     <= 0 (collapsed coordinates, constant truth): r taken as 0 in the value (combined_loss_training.py:
 *     136-138), no gradient from the term, stats[8] stays NaN;
 *   HICGAT_MLOSS_RMSE:    sqrt(mse + 1e-12) (HiC_GAT_generalize_directly.py:60-62);
 *   HICGAT_MLOSS_SI_MSE:  the all-entries mean of (e - ebar)^2, e = D - T, ebar its all-entries mean
 *     (scale_invariant_mse, HiC_GAT_generalize_directly.py:64-68).
 * Each derivative per pair is A d_ij + B t_ij + C with A, B, C functions of the moments, so ONE tile
 * pass accumulates R_i = sum_j (d_ij - t_ij) u_ij and W_i = sum_j u_ij, u_ij = (c_i - c_j)/d_ij (0 where
 * d_ij = 0), a second kernel reduces them per row, and a third finalizes the moments, forms A, B, C in
 * fp64 on the device and writes dcoords[i] = float(-B R_i + (A + B)(N c_i - sum_j c_j) + C W_i).  No
 * host read; the three launches (four in the background form) can be captured in a graph.  Whole
 * matrix only (no tile range, band or cmap).  alpha is read by HICGAT_MLOSS_PEARSON only.  Outputs:
 *   stats[12] (float64): 0..6 the moments as hicgat_pairdist_mse_fused (all seven, every kind), 7 mse,
 *     8 pearson r (NaN when a variance is <= 0), 9 alpha (PEARSON) / 0 (RMSE) / ebar (SI_MSE), 10 the
 *     loss value, 11 sum_i T_ii;
 *   loss[1] (float32, may be NULL): float(stats[10]);  dcoords [N,3] (may be NULL): d(loss)/dcoords.
 * T: the whole truth, element (i, j) at T[i * ldt + j], ldt >= N.  The _support form takes the truth
 * in background form, as hicgat_pairdist_mse_fused_support does (W comes from the bulk pass alone; R
 * and the t-moments take the support pass's correction).
 * workspace: hicgat_pairdist_moment_loss_workspace_bytes(N) / ..._support_workspace_bytes(N). */
enum { HICGAT_MLOSS_PEARSON = 0, HICGAT_MLOSS_RMSE = 1, HICGAT_MLOSS_SI_MSE = 2 };
int hicgat_pairdist_moment_loss(const float *coords, const float *T, int N, int64_t ldt, int mloss_kind,
                                double alpha, double *stats, float *loss, float *dcoords, void *workspace,
                                size_t workspace_bytes, hicgat_stream_t stream);
int hicgat_pairdist_moment_loss_support(const float *coords, int N, float background, const int32_t *rowptr,
                                        const int32_t *col, const float *val, const float *diag, int mloss_kind,
                                        double alpha, double *stats, float *loss, float *dcoords, void *workspace,
                                        size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_pairdist_moment_loss_workspace_bytes(int N);
size_t hicgat_pairdist_moment_loss_support_workspace_bytes(int N);
/* The background form of a symmetric N x N fp32 truth T (leading dim ldt): the sorted CSR of the
 * off-diagonal entries != background, their values, and the diagonal.  Two calls, as
 * hicgat_csr_from_dense: col == NULL fills rowptr (the counts, scanned); then col / val / diag. */
int hicgat_truth_support(const float *T, int N, int64_t ldt, float background, int32_t *rowptr, int32_t *col,
                         float *val, float *diag, hicgat_stream_t stream);

/* ---- a6 / a10: fp32 MFMA GEMM for torch.nn.Linear forward/backward (models.py:637-659) -------
 *   C[M,N] (+)= op(A) op(B) (+ bias[N]);  op(A) = A [M,K] (lda = row stride) or, with a_kmajor,
 *   A^T of A [K,M];  op(B) = B^T of B [N,K] or, with b_kmajor, B [K,N].
 *   Linear forward Y = X W^T + b (0,0); input grad dX = dY W (0,1); weight grad dW = dY^T X (1,1).
 * accumulate != 0 adds into C (a parameter's .grad).  splits > 1 splits K over workgroups into fp32
 * slabs (workspace: hicgat_gemm_workspace_bytes; NULL, 0 with splits = 1) added in split order:
 * deterministic.  bias may be NULL.  impl: there is one matrix-core arithmetic, v_mfma_f32_32x32x2_f32
 * (fp32 products, fp32 accumulate), and HICGAT_GEMM_AUTO (the default) and HICGAT_GEMM_F32 both run it
 * and give the same bits.  AUTO leaves the kernel to the dispatch: a K-split weight gradient (1,1)
 * of whole 128 x 128 tiles (M, N multiples of 128 up to 1024, lda and ldb multiples of 4, 16-byte
 * aligned operands) takes the LDS-DMA ring kernel (gemm_wgrad.hip).  F32 keeps the register-staged
 * gemm_kernel for that case too (A/B measurements, the bitwise test).
 * HICGAT_GEMM_X3 (a three-way bf16 operand split on the bf16 matrix cores, round 1-3) measured slower
 * per step and was removed: HICGAT_EUNSUPPORTED. */
enum { HICGAT_GEMM_AUTO = 0, HICGAT_GEMM_F32 = 1, HICGAT_GEMM_X3 = 2 };
int hicgat_gemm(int a_kmajor, int b_kmajor, int M, int N, int K, const float *A, int64_t lda,
                const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int accumulate,
                int splits, int impl, void *workspace, size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_gemm_workspace_bytes(int M, int N, int splits);
/* The `splits` a caller should hand hicgat_gemm for a node-row problem (a_kmajor = 0: Linear forward,
 * input gradient; M = rows): 1 when the problem fills the chip unsplit (the tall 160 x 128 kernel
 * takes it, or its 64-row tiles are >= 256 workgroups) and for M < 1024 or K < 256; else enough K
 * chunks, each >= 128 deep, for ~512 workgroups (a rank's shard of the multi-GPU step).  Derived from
 * the dispatch's own tile rule.  A pure function of its arguments: no stream, no HIP call, no GPU
 * needed (as hicgat_pairdist_num_tiles). */
int hicgat_gemm_row_splits(int M, int N, int K);
/* The form a hicgat_gemm or hicgat_gemm_wgrad call with these arguments launches, decided by the very
 * predicates the dispatch uses (tests assert through it that they reach the kernel they name).  A and
 * B are read for their alignment only and never dereferenced.  with_db = 0: a hicgat_gemm call.  A
 * hicgat_gemm_wgrad call is a_kmajor = b_kmajor = 1, impl = HICGAT_GEMM_F32 (it never takes the ring
 * kernel) and with_db = (db != NULL); with_db != 0 in any other layout is HICGAT_EINVAL.
 * Returns HICGAT_EINVAL / HICGAT_EUNSUPPORTED where the call would for these arguments (sizes, splits,
 * impl, NULL operands), HICGAT_GEMM_FORM_NONE (0) where it returns without a launch (M == 0 or N == 0),
 * else the bits
 *   HICGAT_GEMM_FORM_KERNEL (mask)  HICGAT_GEMM_FORM_GEMM_KERNEL (gemm.hip's register-staged
 *                                   gemm_kernel), _TALL (gemm_tall.hip, 160 x 128 LDS-DMA) or _RING
 *                                   (gemm_wgrad.hip, 128 x 128 LDS-DMA slabs)
 *   HICGAT_GEMM_FORM_TILE (mask)    HICGAT_GEMM_FORM_64x64, _64x128, _128x128 or _160x128
 *   HICGAT_GEMM_FORM_VEC            16-byte staging (float4 loads; always set for the LDS-DMA kernels),
 *                                   clear: scalar staging (a dimension or leading dimension that is no
 *                                   multiple of 4, or an operand that is not 16-byte aligned)
 *   HICGAT_GEMM_FORM_DB             gemm_kernel with double-buffered LDS
 *   HICGAT_GEMM_FORM_CS             gemm_kernel with the bias-gradient column sums
 * Pure host arithmetic: no stream, no HIP call, no GPU needed. */
enum {
  HICGAT_GEMM_FORM_NONE = 0,
  HICGAT_GEMM_FORM_GEMM_KERNEL = 1, HICGAT_GEMM_FORM_TALL = 2, HICGAT_GEMM_FORM_RING = 3, HICGAT_GEMM_FORM_KERNEL = 3,
  HICGAT_GEMM_FORM_64x64 = 0 << 2, HICGAT_GEMM_FORM_64x128 = 1 << 2, HICGAT_GEMM_FORM_128x128 = 2 << 2,
  HICGAT_GEMM_FORM_160x128 = 3 << 2, HICGAT_GEMM_FORM_TILE = 3 << 2,
  HICGAT_GEMM_FORM_VEC = 1 << 4, HICGAT_GEMM_FORM_DB = 1 << 5, HICGAT_GEMM_FORM_CS = 1 << 6
};
int hicgat_gemm_form(int a_kmajor, int b_kmajor, int M, int N, int K, const void *A, int64_t lda, const void *B,
                     int64_t ldb, int splits, int impl, int with_db);
/* Weight AND bias gradient of a Linear in one GEMM (replaces the dW GEMM + bias column sum of the
 * Linear backward, torch.nn.Linear via ATen addmm_backward / sum(0), models.py:637-659):
 *   dW[M,N] (+)= dY^T X  (dY [K,M] and X [K,N] row-major, K = node rows),
 *   db[M]   (+)= sum_k dY[k][m]  (db may be NULL)
 * the workgroups of the first column tile sum their staged dY tile over K; with splits > 1 the
 * per-split db partials sit in the slab beside the dW partials and ONE slab sum (split order,
 * deterministic) writes both.  fp32 MFMA (HICGAT_GEMM_F32 arithmetic).  Workspace:
 * hicgat_gemm_wgrad_workspace_bytes(M, N, splits). */
int hicgat_gemm_wgrad(int M, int N, int K, const float *dY, int64_t ldy, const float *X, int64_t ldx, float *dW,
                      int64_t lddw, float *db, int accumulate, int splits, void *workspace, size_t workspace_bytes,
                      hicgat_stream_t stream);
size_t hicgat_gemm_wgrad_workspace_bytes(int M, int N, int splits);
/* The `splits` a caller should hand hicgat_gemm_wgrad (or hicgat_gemm's (1,1) layout) for dW [M, N]
 * over K node rows: about target_wgs workgroups in all, every split at least 256 rows deep, at
 * least 1.  Pure host arithmetic: no stream, no HIP call, no GPU needed. */
int hicgat_gemm_wgrad_splits(int M, int N, int K, int target_wgs);
/* ---- grouped parameter gradients (one training step's dW / db / LayerNorm sums in two launches) ----
 * Replaces the per-Linear autograd weight-gradient calls (the ATen mm of dY^T X and the bias sum
 * behind every torch.nn.Linear.backward in models.py:637-659, and GATConv lin_l's) when a
 * step issues all of them at one point (the sharded step, hicgat.dist): the W weight-gradient
 * jobs dW (+)= dY^T X, db (+)= column sums of dY (db may be NULL; dY [K, M] ld ldy, X [K, N] ld
 * ldx, dW [M, N] ld lddw) run as ONE launch of 128 x 128 fp32-MFMA tiles over the union of their
 * tiles, K split into chunks of one common depth (about target_wgs workgroups in all), partials in
 * fp32 slabs; then ONE launch adds, in fixed order, every job's slabs into dW / db AND the C extra
 * column-sum jobs dst[c] (+)= sum_{r < rows} (wt ? wt[r * ldw] : 1) src[r * ld + c] (LayerNorm
 * dgamma/dbeta partial rows, bias sums, the rows of a few-row weight gradient).  Deterministic (no atomics); at most 16 weight-gradient and 32 column-sum jobs
 * (HICGAT_EUNSUPPORTED beyond).  Workspace: hicgat_param_grads_workspace_bytes(same jobs). */
typedef struct hicgat_wgrad_job {
  const float *dy;
  int64_t ldy;
  const float *x;
  int64_t ldx;
  float *dw;
  int64_t lddw;
  float *db;
  int M, N, K, accumulate;
} hicgat_wgrad_job;
typedef struct hicgat_colsum_job {
  const float *src;
  int64_t ld;
  int64_t rows;
  int64_t cols;
  float *dst;
  int accumulate;
  const float *wt;    /* NULL, or row weights: dst[c] (+)= sum_r wt[r * ldw] src[r * ld + c] (a dW row of a */
  int64_t ldw;        /* weight gradient with a handful of output rows, e.g. dense3's 3 x 64) */
  int segs;           /* <= 1: one sum into dst; else the rows in `segs` contiguous segments, segment s */
  int64_t ldd;        /* (rows [rows s / segs, rows (s + 1) / segs)) into dst + s * ldd: a tall job's sum
                       * spread over segs x more blocks, the segments added by the consumer */
} hicgat_colsum_job;
size_t hicgat_param_grads_workspace_bytes(const hicgat_wgrad_job *wjobs, int nw, int target_wgs);
int hicgat_param_grads_grouped(const hicgat_wgrad_job *wjobs, int nw, const hicgat_colsum_job *cjobs, int nc,
                               int target_wgs, void *workspace, size_t workspace_bytes, hicgat_stream_t stream);
/* Grouped node-row GEMMs of one layout: C_j = A_j op(B_j) (+ bias_j), A_j [M, K] row-major (ld lda),
 * op(B) = B^T (B [N, K], b_kmajor = 0: a Linear / head forward) or B (B [K, N], b_kmajor = 1: an
 * input gradient), c_relu (NULL or ld ldr): relu of the result too.  ONE launch of 64 x 128 fp32-MFMA
 * tiles over every job's tiles, K split in `splits` chunks into fp32 slabs; ONE launch adds the slabs
 * in split order (+ bias, relu copy).  splits = 1: the tiles write C (+ bias, relu copy) themselves,
 * no second launch, no workspace (NULL allowed).  Replaces the per-head GEMM calls (ATen mm of GATConv lin_l,
 * by linearity per head: hicgat.dist's aggregate-first form).  K, N, every ld a multiple of 4, every
 * pointer 16-B aligned (else HICGAT_EUNSUPPORTED); at most 8 jobs.
 * Workspace: hicgat_gemm_rows_grouped_workspace_bytes(same jobs, splits). */
typedef struct hicgat_gemm_job {
  const float *a;
  int64_t lda;
  const float *b;
  int64_t ldb;
  float *c;
  int64_t ldc;
  float *c_relu;
  int64_t ldr;
  const float *bias;
  int M, N, K;
} hicgat_gemm_job;
size_t hicgat_gemm_rows_grouped_workspace_bytes(const hicgat_gemm_job *jobs, int n, int splits);
/* The `splits` for these jobs (only M, N, K are read): enough K chunks, each >= 128 deep by the first
 * job's K, for about target_wgs 64 x 128 workgroups over all jobs; target_wgs = 0 (or no job): 1, the
 * unsplit form.  Pure host arithmetic: no stream, no HIP call, no GPU needed. */
int hicgat_gemm_rows_grouped_splits(const hicgat_gemm_job *jobs, int n, int target_wgs);
int hicgat_gemm_rows_grouped(const hicgat_gemm_job *jobs, int n, int b_kmajor, int splits, void *workspace,
                             size_t workspace_bytes, hicgat_stream_t stream);
/* out[n] = sum_k A[k][n] over K rows (a Linear bias gradient), deterministic two-stage. */
int hicgat_colsum(const float *A, int64_t lda, int K, int N, float *out, int accumulate, void *workspace,
                  size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_colsum_workspace_bytes(int K, int N);

/* ---- a6 and the zoo's other LayerNorm tails (ln_act.hip; the flagship's models.py:641-655, and :321-377,
 * :379-435, :437-526, :528-612, :693-773, :776-832): LayerNorm -> activation (+ residual) (-> a second
 * LayerNorm) as one row pass:
 *   u = act(LayerNorm(y; gamma, beta, eps)) + res            (res may be NULL)
 *   z = LayerNorm(u; gamma2, beta2, eps2)                    (gamma2 != NULL; else z = u)
 * torch.nn.LayerNorm semantics (biased variance about the mean, eps inside the square root).  act is a
 * HICGAT_ACT_* code: none, relu, leaky_relu (x > 0 ? x : x * slope) or gelu = 0.5 x (1 + erf(x / sqrt 2))
 * (F.gelu's default, not the tanh form).  W in {32, 64, 128, 256, 512}.  y / res / z rows are ldy / ldr /
 * ldz floats apart (column slices of one [M, 2W] buffer pass ld = 2W).  row_stats [M, 2] = (mean, rstd)
 * and, with the second norm, row_stats2 [M, 2] = (mean2, rstd2) are saved for the backward.  The
 * flagship's blocks are relu without a second norm at W = 256, 128 (res given) and 64 (res NULL).
 * Backward (recomputes pre = yhat gamma + beta, and u from y and res with the second norm: pass the
 * forward's res, gamma2 and row_stats2 then; res is not read otherwise):
 *   du = rstd2 (dz gamma2 - mean(.) - uhat mean(. uhat)), or dz without the second norm;
 *   dres = du, written to dres (ld lddres) when dres != NULL (without the second norm a NULL dres loses
 *   nothing: d(res) is the caller's dz) -- e.g. beside dy, dy = dY, dres = dY + W, lddy = lddres = 2W, so that
 *   one packed [dy | dres] row feeds the dual-Linear backward's single dx and dW GEMMs;
 *   g = du act'(pre): relu [pre > 0], leaky_relu (pre > 0 ? 1 : slope), gelu Phi(pre) + pre phi(pre);
 *   dy (ld lddy) = rstd (g gamma - mean(.) - yhat mean(. yhat));
 *   dgamma = sum g yhat, dbeta = sum g, dgamma2 = sum dz uhat, dbeta2 = sum dz over the rows: per-wave
 *   partials in the workspace, then fixed-order column sums (deterministic, no atomics); accumulate != 0
 *   adds into them.  dgamma = dbeta = dgamma2 = dbeta2 = NULL: the partials stay in the workspace and
 *   hicgat_ln_act_res_bwd_params (dgamma2 / dbeta2 given iff the backward had the second norm) reduces
 *   them, e.g. on another stream after an event -- the same bits as the one-call form.
 * Unknown W or act: HICGAT_EUNSUPPORTED.  A NULL pointer, M < 0, eps <= 0, an ld < W, leaky_relu with
 * slope <= 0, gamma2 without beta2 (or dgamma without dbeta, ...), a small workspace: HICGAT_EINVAL;
 * all of it is checked before any launch.  M == 0: the forward returns HICGAT_OK without a launch (the
 * backward still zeroes or keeps the parameter gradients).
 * workspace: hicgat_ln_act_res_workspace_bytes(W, second_norm) (0 for an unsupported W). */
int hicgat_ln_act_res_fwd(const float *y, int64_t ldy, int M, int W, const float *gamma, const float *beta, float eps,
                          int act, float slope, const float *res, int64_t ldr, const float *gamma2, const float *beta2,
                          float eps2, float *z, int64_t ldz, float *row_stats, float *row_stats2,
                          hicgat_stream_t stream);
int hicgat_ln_act_res_bwd(const float *dz, int64_t lddz, const float *y, int64_t ldy, int M, int W,
                          const float *row_stats, const float *gamma, const float *beta, int act, float slope,
                          const float *res, int64_t ldr, const float *gamma2, const float *row_stats2, float *dy,
                          int64_t lddy, float *dres, int64_t lddres, float *dgamma, float *dbeta, float *dgamma2,
                          float *dbeta2, int accumulate, void *workspace, size_t workspace_bytes,
                          hicgat_stream_t stream);
int hicgat_ln_act_res_bwd_params(int W, float *dgamma, float *dbeta, float *dgamma2, float *dbeta2, int accumulate,
                                 void *workspace, size_t workspace_bytes, hicgat_stream_t stream);
size_t hicgat_ln_act_res_workspace_bytes(int W, int second_norm);
/* Elementwise y = act(x) over a contiguous [M, W] tensor (the F.gelu / F.leaky_relu that follows the
 * GATConv at models.py:717 / :795), act = HICGAT_ACT_GELU or HICGAT_ACT_LEAKY_RELU (others, or W % 4 != 0:
 * HICGAT_EUNSUPPORTED), 16-B aligned (float4 loads); the backward dx = dy act'(x) reads the saved INPUT x. */
int hicgat_act_fwd(const float *x, int M, int W, int act, float slope, float *y, hicgat_stream_t stream);
int hicgat_act_bwd(const float *dy, const float *x, int M, int W, int act, float slope, float *dx,
                   hicgat_stream_t stream);

/* ---- The flagship's MLP tail in one launch per direction (tail_fused.hip; replaces the dual-Linear GEMMs,
 * LayerNorm row passes and Linear GEMMs of models.py:637-659 for GATNetSelectiveResidualsUpdated) ----
 * The operands travel as four structs, passed by pointer and read completely before the call returns
 * (the caller may free them right after it, also during a graph capture).  Each struct leads with the
 * pointers both directions require; a NULL struct or required pointer, M < 0: HICGAT_EINVAL; M == 0:
 * HICGAT_OK without a launch.
 * hicgat_tail_weights: W1c [512][512] = [W_densea; W_align_densea], b1c [512]; g1/be1 [256] = norm_a; W2c
 *   [256][256] = [W_dense1; W_align_dense1], b2c [256]; g2/be2 [128] = norm1; W3 [64][128] / b3 = dense2;
 *   g3/be3 [64] = norm2; W4 [3][64] / b4 = dense3; eps: the LayerNorms' (inside the square root).  The
 *   backward does not read b1c, b2c, b3, b4 and eps.  W1c, W2c, W3 and pack 16-B aligned (else
 *   HICGAT_EUNSUPPORTED).
 *   pack: NULL, or the packed weight copies hicgat_tail_pack made from THESE W1c / W2c (and, for HEADS,
 *   Wh): the kernels then read W1c, W2c and Wh from it (1 KB contiguous per wave load instead of
 *   16 rows x 64 B: the vector memory path serves the row-major rows at 16 B per clock per CU, a quarter
 *   of the contiguous rate, and that set the pace of the kernels' GEMM phases); results bitwise the
 *   row-major form.  W3 / W4 are always read row-major.  hicgat_tail_pack_bytes(): the buffer's size.
 *   Not a reference interface: the copies are a layout of the same parameters.  The library records,
 *   per pack buffer, whether its last hicgat_tail_pack included Wh: HEADS returns HICGAT_EINVAL for a
 *   pack made with Wh = NULL.
 * hicgat_tail_acts: what the forward writes for the backward: Y1 [M][512] (block-1 GEMM + bias), st1 [M][2]
 *   (mean, rstd), Y2 [M][256], st2, y3 [M][64], st3 -- the backward reads these six -- and z1 [M][256],
 *   z2 [M][128], z3 [M][64] (each block's output: the weight-gradient GEMMs' inputs). */
typedef struct {
  const float *W1c, *W2c, *W3, *W4, *g1, *be1, *g2, *be2, *g3, *be3;
  const float *b1c, *b2c, *b3, *b4;
  float eps;
  const void *pack;
} hicgat_tail_weights;
typedef struct {
  float *Y1, *st1, *Y2, *st2, *y3, *st3;
  float *z1, *z2, *z3;
} hicgat_tail_acts;
/* hicgat_tail_grads (the backward writes): dY1 [M][512] = [dy | dres] of block 1, dY2 [M][256] of block 2, dy3
 *   [M][64] (dense2's output gradient) -- the inputs of the weight-gradient GEMMs -- and each LayerNorm's
 *   dgamma/dbeta partials into ws[0] / ws[1] / ws[2] (W = 256 / 128 / 64): rows [0, ceil(M/16)) of a [.][2W]
 *   = [dgamma | dbeta] matrix, one per 16-row workgroup (its waves' partials added in wave order; the
 *   rows' column sums, e.g. hicgat_colsum, are dgamma / dbeta); ws_bytes[i] at least
 *   hicgat_tail_bwd_workspace_bytes(M, W) (else HICGAT_EINVAL).  dx [M][512], the gradient of the tail's
 *   input: required by the plain form, not read by the others. */
typedef struct {
  float *dY1, *dY2, *dy3;
  void *ws[3];
  float *dx;
  size_t ws_bytes[3];
} hicgat_tail_grads;
/* hicgat_tail_gat: the GATConv side of the fused forms (a NULL struct: HICGAT_TAIL_PLAIN, which reads no
 * other field; an unknown form: HICGAT_EINVAL).
 * HICGAT_TAIL_HEADS, for the sharded aggregate-first GATConv (hicgat.dist "xagg"; the GATConv of
 *   models.py:619 by linearity per head, then the tail): the forward forms the tail's input rows
 *   itself, Y0[:, 256h:256h+256] = xa^h W_h^T + b^h (xa^h = x + h * xa_head_stride, [M][ldx], a multiple
 *   of 4; W_h = rows 256h.. of lin_l's weight Wh [512][512]; bh [512]) and O = relu(Y0) (both [M][512],
 *   written), replacing the per-head GEMM launches and their slab sum.  The backward, instead of writing
 *   dx, runs the GATConv's rows backward and its input-gradient GEMM: dout = dx * (Y0 > 0) (act != 0;
 *   act = 0: dout = dx) into dout [M][512], delta^h = <dout^h, Y0^h - b^h> into row_stats[8r + 4 + h] (its
 *   [4:6] S3 values move to [6:8], as hicgat_xagg_rows_bwd does), dxa [M][1024] = [dout^0 W_0 | dout^1
 *   W_1].  Needs hicgat_tail_bwd_waves() >= 8 (else HICGAT_EUNSUPPORTED); out2 is not read.
 * HICGAT_TAIL_ROWS, a form of the backward only (hicgat_tail_fwd: HICGAT_EINVAL), for the single-GPU
 *   GATConv: its gather-free rows pass in the epilogue (hicgat_gat_agg_bwd_rows on the dx rows while they
 *   are in LDS, same arithmetic, bitwise): no dx is written; dout [M][512] = dx [Y0 > 0] (act != 0) or dx,
 *   and row_stats[8i + 4 .. 8i + 8) = (delta, da_dst) from the forward's S3 there, for Y0 = the GATConv's
 *   relu output (the tail's input rows), out2 and bh = bias of hicgat_gat_agg_fwd.  One row per wave:
 *   HICGAT_EUNSUPPORTED unless hicgat_tail_bwd_waves() == 16; Wh, O and dxa are not read.
 * Wh, Y0, O (forward) and Y0, bh, dout, row_stats, out2 (backward) 16-B aligned (else HICGAT_EUNSUPPORTED). */
#define HICGAT_TAIL_PLAIN 0
#define HICGAT_TAIL_HEADS 1
#define HICGAT_TAIL_ROWS 2
typedef struct {
  int form, act;
  int64_t xa_head_stride;
  const float *Wh, *bh;
  float *Y0, *O;
  const float *out2;
  float *dout, *row_stats, *dxa;
} hicgat_tail_gat;
/* Forward: x [M][512] (ld ldx >= 512, a multiple of 4, 16-B aligned rows) is the GATConv output after its
 * relu -- for HEADS the aggregates xa (ld ldx), see above; writes acts and coords [M][3].  16 rows per
 * workgroup, fp32 MFMA (16x16x4). */
int hicgat_tail_fwd(const hicgat_tail_weights *weights, const float *x, int64_t ldx, int M,
                    const hicgat_tail_acts *acts, float *coords, const hicgat_tail_gat *gat, hicgat_stream_t stream);
size_t hicgat_tail_pack_bytes(void);
int hicgat_tail_pack(const float *W1c, const float *W2c, const float *Wh, void *pack, size_t pack_bytes,
                     hicgat_stream_t stream);
/* Backward: the input-gradient chain from dcoords [M][3] and the forward's acts; writes grads (and, by
 * gat's form, dout / row_stats / dxa instead of dx).
 * hicgat_tail_bwd_waves(): the waves per workgroup of both tail kernels.
 * hicgat_tail_bwd_partial_rows(M): the rows of partials each workspace holds after the call, one per
 * workgroup (ceil(M / the kernel's row block); 0 for M <= 0) -- what the caller's column sums read.
 * Pure host arithmetic: no stream, no HIP call, no GPU needed. */
int hicgat_tail_bwd_waves(void);
int hicgat_tail_bwd_partial_rows(int M);
size_t hicgat_tail_bwd_workspace_bytes(int M, int W);
int hicgat_tail_bwd(const hicgat_tail_weights *weights, const hicgat_tail_acts *acts, const float *dcoords, int M,
                    const hicgat_tail_grads *grads, const hicgat_tail_gat *gat, hicgat_stream_t stream);

/* ---- f1: SAGEConv of the baseline model Net (layers.py:41-79, models.py:14-55) ----------------
 * hicgat_sage_weights: the float32 edge weight w of every entry of the (set_diag'd) device CSR --
 * the networkx weight utils.load_input assigns (utils.py:37-52): A[max(i,j), min(i,j)] when
 * non-zero, else A[min, max]; 0 on the self loops -- and inv_deg[i] = 1 / sum_j w_ij, the
 * SAGEConv.adjust_weights normaliser (layers.py:41-53; sum in ascending column order).
 * hicgat_sage_agg: z[i, 0:F] = sum_{j != i} (inv_deg[i] * w_ij) x[j]  (matmul(norm_mat, x), :74-77)
 * over rows [row_begin, row_end); transpose != 0 weights by inv_deg[j] instead (the adjoint,
 * d agg -> d x); write_trunc != 0 also writes z[i, F:2F] = trunc(x[i]) (x.long().float(), :64). */
int hicgat_sage_weights(const double *A, int N, int64_t lda, const int32_t *rowptr, const int32_t *col,
                        float *weights, float *inv_deg, hicgat_stream_t stream);
int hicgat_sage_agg(const int32_t *rowptr, const int32_t *col, const float *weights, const float *inv_deg,
                    int N, int F, int row_begin, int row_end, const float *x, int transpose, int write_trunc,
                    float *z, int64_t ldz, hicgat_stream_t stream);

/* ---- f2: Knight-Ruiz normalisation (r_utils.R:1-93 KRnorm, run by normalize.R from
 * HiC-GNN_main.py:85) -- the O(N^2) parts; the O(N) CG bookkeeping is the caller's (hicgat/kr.py).
 * A: float64 row-major n x n (leading dim lda), NaN entries count as 0.
 *   hicgat_kr_matvec: out_i = x_i * sum_j A_ij x_j p_j (+ v_i p_i if v != NULL)   (r_utils.R:24,42,64)
 *   hicgat_kr_scale:  out_ij = rint(((x_i A_ij) x_j) * 1e6) / 1e6, NaN kept        (r_utils.R:74-89) */
int hicgat_kr_matvec(const double *A, int64_t lda, int n, const double *x, const double *p, const double *v,
                     double *out, hicgat_stream_t stream);
int hicgat_kr_scale(const double *A, int64_t lda, int n, const double *x, double *out, int64_t ldo,
                    hicgat_stream_t stream);

/* ---- f4: node2vec embeddings (HiC_GAT_generalize_directly.py:150-155: node2vec 0.4 + gensim 4
 * Word2Vec, restated; see csrc/node2vec.hip).
 * hicgat_n2v_walks: nwalks biased walks of walk_length nodes from starts[w] over the weighted CSR
 *   (rows sorted, cum_weights[k] = inclusive per-row cumulative edge weight); second-order factors
 *   1/p (back to the previous node), 1 (a neighbour of it), 1/q (otherwise), by rejection sampling
 *   with a counter-based RNG (deterministic for a seed); a walk that reaches a node without
 *   neighbours ends and is padded with -1.  walks [nwalks, walk_length] int32.
 * hicgat_n2v_sgns_epoch: one skip-gram negative-sampling epoch over the walks (window, negative,
 *   learning rate decaying linearly from alpha0 to alpha1 over `epochs`), gensim's downsampling
 *   (keep_prob[v]) and unigram^0.75 negative table (cum_table[V], cumulative), syn0 / syn1 [V, D]
 *   fp32 (D a multiple of 64, <= 1024; negative <= 7), updated Hogwild-style by at most max_waves walks in flight
 *   (one wave per walk; a small vocabulary wants few, the reference trains with one worker):
 *   exactly min(nwalks, max_waves) waves take walks, wave g the walks g, g + that many, ..., so
 *   max_waves = 1 trains the walks one after the other, in order, and is deterministic.  Within one
 *   (centre, context) pair all target rows are read before any is written: a target drawn twice
 *   in the pair reads its row once, and the later write wins. */
int hicgat_n2v_walks(const int32_t *rowptr, const int32_t *col, const float *cum_weights, int N,
                     const int32_t *starts, int nwalks, int walk_length, float p, float q, uint64_t seed,
                     int32_t *walks, hicgat_stream_t stream);
int hicgat_n2v_sgns_epoch(const int32_t *walks, int nwalks, int walk_length, const float *keep_prob,
                          const uint32_t *cum_table, int V, int D, int window, int negative, float alpha0,
                          float alpha1, int epoch, int epochs, uint64_t seed, int max_waves, float *syn0,
                          float *syn1, hicgat_stream_t stream);

/* ---- LINE: second-order LINE embeddings, the feature generator of HiC-GNN_main.py:91-96
 * (`LINE(G, embedding_size=512, order='second')`, `line.train(batch_size, epochs)`: the `ge` package
 * over Keras, restated from its published source; see csrc/line.hip) ------------------------------
 * Host-supplied tables (device pointers): the E edges (head[i], tail[i]) with their alias table
 * (edge_accept float32, edge_alias int32) over p_edge = w / sum w; the N-entry node alias table
 * (node_accept, node_alias) over p_node ~ deg^0.75; perm [n_pass, E]: one permutation of 0..E-1 per
 * pass of the stream, for the passes pass_begin .. pass_begin + n_pass - 1.
 *
 * The sample stream.  R = 1 + negative batches per chunk, chunks = ceil(E / batch_size) chunks per
 * pass.  Step s (a batch, counted from 0 over the whole run) lies in pass s / (chunks R), at
 * r = s % (chunks R), chunk c = r / R, batch b = r % R; it has len = min(batch_size, E - c batch_size)
 * samples, slot j = 0 .. len-1.  The random words of (s, j) are Philox4x32-10 as under "feature
 * dropout" below:
 *   counter = (j, s & 0xffffffff, s >> 32, HICGAT_LINE_SITE);  key = (seed & 0xffffffff, seed >> 32);
 *   word -> uniform:  u(w) = (float)(w >> 8) * 2^-24        (24 bits, exact in float32, in [0, 1));
 *   word -> index:    idx(w, n) = (uint64(w) * n) >> 32      (in [0, n)).
 * The chunk's positives are drawn by the words of its batch 0, step s - b:
 *   i = perm[pass][c batch_size + j];  if u(w0) >= edge_accept[i]: i = edge_alias[i];  h = head[i];
 *   b == 0:  t = tail[i], y = +1;
 *   b  > 0:  with the words of (s, j):  n = idx(w0, N);  t = u(w1) < node_accept[n] ? n : node_alias[n];
 *            y = -1   (the same h as batch 0: a chunk's R batches share their heads).
 * So (h, t, y) is a pure function of (seed, s, j) and the tables: no state passes from step to step.
 *
 * hicgat_line_samples writes the (h, t, y) of steps [step_begin, step_end) into h / t / y
 * [step_end - step_begin, batch_size] int32; slots j >= len hold (-1, -1, 0).
 *
 * hicgat_line_train enqueues steps [step_begin, step_end), two launches each, on tables U (the
 * embeddings, `second_emb`) and C (`context_emb`), both [N, D] fp32, with the Adam moments mU, vU,
 * mC, vC (zero before step 0):
 *   s_k = <U[h_k], C[t_k]>;  loss = -mean_k log sigmoid(y_k s_k);  g_k = -(y_k / len) sigmoid(-y_k s_k);
 *   dU[h_k] += g_k C[t_k],  dC[t_k] += g_k U[h_k]   (both from the tables as they stand BEFORE the step;
 *   duplicates summed in ascending k);  then Keras' Adam, dense over both tables, t = s + 1:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)  (host, float64);  p -= lr_t m / (sqrt(v) + eps).
 * (Not torch's form: hicgat_adam_step divides sqrt(v) by sqrt(1-b2^t) before adding eps.)  No float
 * atomics and one summation order: the tables after a step range are bit-reproducible.
 * Checked before any launch: D % 64 == 0 and 64 <= D <= 1024 (else HICGAT_EUNSUPPORTED);
 * batch_size >= 1, 0 <= negative <= 64, a step range inside the passes that perm holds, non-NULL
 * 16-B aligned tables / moments / workspace, workspace_bytes >= hicgat_line_workspace_bytes(D,
 * batch_size), lr >= 0, 0 <= b1, b2 < 1, eps >= 0 (else HICGAT_EINVAL).  E == 0 or an empty step range
 * is a no-op. */
enum { HICGAT_LINE_SITE = 0x4C494E45 };   /* "LINE": the fourth counter word of the LINE sample stream */
size_t hicgat_line_workspace_bytes(int D, int batch_size);
int hicgat_line_samples(const int32_t *head, const int32_t *tail, const float *edge_accept,
                        const int32_t *edge_alias, int E, const float *node_accept, const int32_t *node_alias,
                        int N, const int32_t *perm, int64_t pass_begin, int64_t n_pass, int batch_size,
                        int negative, uint64_t seed, int64_t step_begin, int64_t step_end, int32_t *h,
                        int32_t *t, int32_t *y, hicgat_stream_t stream);
int hicgat_line_train(const int32_t *head, const int32_t *tail, const float *edge_accept,
                      const int32_t *edge_alias, int E, const float *node_accept, const int32_t *node_alias,
                      int N, const int32_t *perm, int64_t pass_begin, int64_t n_pass, int D, int batch_size,
                      int negative, uint64_t seed, int64_t step_begin, int64_t step_end, double lr,
                      double beta1, double beta2, double eps, float *U, float *C, float *mU, float *vU,
                      float *mC, float *vC, void *workspace, size_t workspace_bytes, hicgat_stream_t stream);

/* ---- a10 (part): torch.optim.Adam step (HiC-GNN_main.py:118,130) over one flat fp32 buffer ----
 * Same arithmetic as torch's single-tensor CPU Adam (lerp / addcmul / addcdiv, no weight decay):
 *   m = fma(1-b1, g-m, m); v = fma((1-b2)*g, g, b2*v);
 *   p += (-lr/(1-b1^t) * m) / (sqrt(v)/sqrt(1-b2^t) + eps). */
int hicgat_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                     double lr, double beta1, double beta2, double eps, int64_t step,
                     hicgat_stream_t stream);
/* Graph-replayable form: the step count lives on the device (*step_counter = steps done so far,
 * incremented by the call), the per-step constants come from table[step] = (-lr/(1-b1^t),
 * sqrt(1-b2^t)) for t = step+1, computed on the host exactly like hicgat_adam_step does.
 * counted = 0: the call reads row *step_counter and increments the count in a launch of its own.
 * counted = 1: this step's increment already happened in an earlier launch of the step
 * (hicgat_step_begin, hicgat_step_begin_pack or hicgat_xagg_logits with step_counter), so the table
 * row is *step_counter - 1 and no increment follows (one launch fewer).  No pointer may be NULL;
 * param / grad / exp_avg / exp_avg_sq 16-B, table 8-B aligned. */
int hicgat_adam_step_table(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                           int64_t n, double beta1, double beta2, double eps, const float *table,
                           int64_t table_len, int64_t *step_counter, int counted, hicgat_stream_t stream);
/* A step's first launch: grad[0, n) = 0 (zero_grad, HiC-GNN_main.py:124) and, with step_counter
 * (NULL: none), *step_counter += 1 (the step's Adam then uses counted = 1).  grad 16-B aligned. */
int hicgat_step_begin(float *grad, int64_t n, int64_t *step_counter, hicgat_stream_t stream);
/* hicgat_step_begin and hicgat_tail_pack(W1c, W2c, Wh, pack) in ONE launch (the step's first: the
 * weights change only at the previous step's Adam), so the one-kernel tail's packed copies cost no
 * launch of their own on the step's chain.  Same arguments and checks as the two. */
int hicgat_step_begin_pack(float *grad, int64_t n, int64_t *step_counter, const float *W1c, const float *W2c,
                           const float *Wh, void *pack, size_t pack_bytes, hicgat_stream_t stream);

/* ---- feature dropout: act -> torch.nn.Dropout of the zoo's forward() (models.py:74-75, :983-984,
 * :1379-1380, :1472-1473, ...) as one pass, with a counter-based mask ------------------------------
 * The keep mask is a pure function of (seed, step, site, global row, column), so it is generated
 * in the kernel, replays under a hipGraph (the step count is read from the device) and does not
 * depend on the launch geometry or on how the rows are sharded.  Philox4x32-10 (multipliers
 * 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85); for element (R, c) of a
 * width-W tensor, R = row_offset + local row:
 *   g = R * (W / 4) + c / 4 (uint64);  counter = (g & 0xffffffff, g >> 32, step & 0xffffffff, site);
 *   key = (seed & 0xffffffff, seed >> 32);  the element uses output word r[c % 4];
 *   kept iff r >= T,  T = min(floor(p * 2^32), 2^32 - 1);  kept values are multiplied by
 *   scale = (float)(1.0 / (1.0 - p)) (one rounding from double; torch's own constant may differ by
 *   an ulp, and its masks differ anyway).  0 <= p < 1 (else HICGAT_EINVAL); p = 0 keeps everything.
 * step = *step_counter when the pointer is given (a device int64, e.g. the one
 * hicgat_dropout_advance increments), else step_value.  W % 4 == 0 and every ld a multiple of 4
 * (else HICGAT_EUNSUPPORTED), x / y / dy / dx 16-B aligned, step_counter 8-B aligned, mask 4-B
 * aligned (else HICGAT_EINVAL); all of it checked before any launch.  M = 0 is a no-op. */
enum { HICGAT_ACT_NONE = 0, HICGAT_ACT_RELU = 1, HICGAT_ACT_LEAKY_RELU = 2,
       HICGAT_ACT_GELU = 3 /* hicgat_ln_act_res_* and hicgat_act_* only; HICGAT_EINVAL elsewhere */ };
/* y[r][c] = kept ? act(x[r][c]) * scale : 0;  relu(x) = x <= 0 ? 0 : x,  leaky_relu(x) = x > 0 ? x :
 * x * slope (fp32).  In place (y == x, ldy == ldx) is allowed. */
int hicgat_act_dropout_fwd(const float *x, int64_t ldx, int M, int W, int act, float slope, double p, uint64_t seed,
                           const int64_t *step_counter, int64_t step_value, uint32_t site, int64_t row_offset,
                           float *y, int64_t ldy, hicgat_stream_t stream);
/* dx from dy and the forward's OUTPUT y alone (no mask is stored or regenerated):
 *   relu:        dx = y > 0 ? dy * scale : 0
 *   leaky_relu:  dx = y > 0 ? dy * scale : y < 0 ? (dy * scale) * slope : 0      (slope > 0)
 * which is torch autograd of where(mask, act(x), 0) * scale bit for bit, with ONE deviation: a kept
 * element whose pre-activation is exactly 0.0 under leaky_relu gets 0 where torch gives
 * slope * scale * dy (y == 0 cannot tell it from a dropped one).  act = none is refused
 * (HICGAT_EUNSUPPORTED: y == 0 is ambiguous there and no model needs it), as is leaky_relu with
 * slope <= 0 (HICGAT_EINVAL).  dx may alias dy. */
int hicgat_act_dropout_bwd(const float *dy, int64_t lddy, const float *y, int64_t ldy, int M, int W, int act,
                           float slope, double p, float *dx, int64_t lddx, hicgat_stream_t stream);
/* mask[r * W + c] = kept ? 1 : 0 (uint8), from the same device function as the forward (tests, tools). */
int hicgat_dropout_mask(uint8_t *mask, int M, int W, double p, uint64_t seed, const int64_t *step_counter,
                        int64_t step_value, uint32_t site, int64_t row_offset, hicgat_stream_t stream);
/* *counter += 1 (one wave, lane 0, an ordinary store): a training forward's first launch, so that
 * every dropout site of the step, ordered after it, reads the same new count -- also in a replay. */
int hicgat_dropout_advance(int64_t *counter, hicgat_stream_t stream);

/* ---- BatchNorm1d over the node axis, fused with the activation and Dropout after it (models.py:
 * 288-298, :852-862: x = dropout(leaky_relu(bn(dense(x))))) ---------------------------------------
 *   z = dropout(act(gamma * yhat + beta)),  yhat = ((y - mean) - mean_lo) * rstd  per column
 * of y [M, W] (row stride ldy).  64 <= W <= 1024 and W % 64 == 0 (else HICGAT_EUNSUPPORTED); y / z /
 * dz / dy 16-B aligned with every ld >= W and a multiple of 4, eps > 0, 0 < momentum <= 1, M >= 2
 * with batch statistics and M >= 1 with running ones (else HICGAT_EINVAL); all of it checked before
 * any launch.  No float atomics: every sum runs in one fixed order, so two calls give the same bits.
 * act / slope / p / seed / step_counter / step_value / site / row_offset: as hicgat_act_dropout_fwd
 * (the same mask); p = 0 is act(BN(y)).
 * stats [4, W] = (mean, mean_lo, rstd, rstd_lo): mean + mean_lo is the batch mean and rstd + rstd_lo
 * is 1 / sqrt(biased variance + eps), each an fp64 value as two floats (the forward uses rstd alone,
 * the backward both).  The variance is a fixed-order Chan merge (fp64) of per-64-row-chunk (mean, sum
 * of squared deviations from it, fp64); E[y^2] - E[y]^2 is never formed. */
size_t hicgat_bn_workspace_bytes(int M, int W);
/* The statistics of a training forward and its side effects, all on the device (a captured step
 * replays them): stats as above;  running_mean = (1 - momentum) running_mean + momentum mean;
 * running_var likewise with the UNBIASED variance;  *num_batches_tracked += 1 (int64).  Each of the
 * three buffers may be NULL (not updated).  ws: 16-B aligned, hicgat_bn_workspace_bytes(M, W). */
int hicgat_bn_stats(const float *y, int64_t ldy, int M, int W, double eps, double momentum, float *stats,
                    float *running_mean, float *running_var, int64_t *num_batches_tracked, void *workspace,
                    size_t workspace_bytes, hicgat_stream_t stream);
/* One pass.  stats given: batch statistics (training).  stats NULL: eval mode, mean = running_mean,
 * rstd = 1 / sqrt(running_var + eps) computed per thread; nothing is updated. */
int hicgat_bn_act_dropout_fwd(const float *y, int64_t ldy, int M, int W, const float *gamma, const float *beta,
                              const float *stats, const float *running_mean, const float *running_var, double eps,
                              int act, float slope, double p, uint64_t seed, const int64_t *step_counter,
                              int64_t step_value, uint32_t site, int64_t row_offset, float *z, int64_t ldz,
                              hicgat_stream_t stream);
/* g = dz * dropout' * act' from the forward's OUTPUT z as in hicgat_act_dropout_bwd (act = none: g =
 * dz, z unused; act = none with p > 0 is HICGAT_EUNSUPPORTED);  dbeta = sum g,  dgamma = sum g yhat
 * (one pass + one launch of fixed-order column sums, fp64: with batch statistics the terms of dy
 * cancel, almost wholly when M = 2);  then one pass
 *   dy = gamma rstd (g - dbeta / M - yhat dgamma / M)     (stats given; fp64, rounded once)
 *   dy = g gamma rstd                                     (stats NULL: running statistics).
 * dgamma / dbeta (both or neither): written, or added to when accumulate != 0.  Either way the sums
 * [dgamma | dbeta] are left in the first 2 W floats of the workspace (e.g. to be added to a gradient
 * buffer by a later launch on another stream). */
int hicgat_bn_act_dropout_bwd(const float *dz, int64_t lddz, const float *z, int64_t ldz, const float *y, int64_t ldy,
                              int M, int W, const float *gamma, const float *stats, const float *running_mean,
                              const float *running_var, double eps, int act, float slope, double p, float *dy,
                              int64_t lddy, float *dgamma, float *dbeta, int accumulate, void *workspace,
                              size_t workspace_bytes, hicgat_stream_t stream);

/* ---- Spearman / per-step dSCC (a11: scipy.stats.spearmanr of HiC_GAT_generalize_directly.py:242
 * and combined_loss_training.py:135) ---------------------------------------------------------------
 * Exact Spearman correlation with scipy's tie rule (a tie group shares its average rank), by a
 * stable LSD radix sort (8-bit digits, four passes) of 32-bit keys with a 32-bit payload and one
 * tie-aware reduction; no host sync, no allocation, no N x N matrix.  The key is the
 * order-preserving image of the float's bits with -0 canonicalised to +0 (they tie); denormals stay
 * distinct.  A NaN on either side gives rho = NaN (nan_policy = 'propagate'), as do a constant side
 * and M < 2.  Ranks are DOUBLED average ranks (uint32, 2 <= rank2 <= 2 M), so every size needs
 * M < 2^31: larger M returns HICGAT_EUNSUPPORTED before anything else is looked at.
 * ws: 256-B aligned, the size the workspace query returns (0 for an unsupported M).  Two calls on the same inputs give the
 * same bits (integer atomics only; fp64 sums in a fixed order).
 *   side_stats [4] = (sum of a^2 with a = rank2 - (M + 1), number of tie groups, NaN flag, M)
 *   out        [4] = (rho, sum of b^2 of the scored side, its number of tie groups, NaN flag) */
/* keys per sort tile (tests place M around its multiples) */
int hicgat_rank_tile(void);
size_t hicgat_rank_workspace_bytes(int64_t M);
/* rank2[k] = 2 * (average rank of v[k] among v[0..M)), in the input's element order; prepares one
 * side (the truth) once. */
int hicgat_avg_rank2(const float *v, int64_t M, uint32_t *rank2, double *side_stats, void *ws, size_t ws_bytes,
                     hicgat_stream_t stream);
/* v[k] = T[i * ld + j] for the k-th pair i < j of torch.triu_indices(N, N, 1) (row-major upper
 * triangle); v holds N (N - 1) / 2 floats.  2 <= N <= 65536. */
int hicgat_triu_gather(const float *T, int N, int64_t ld, float *v, hicgat_stream_t stream);
/* Spearman of v against a side prepared by hicgat_avg_rank2 (same M, same element order). */
int hicgat_spearman_vs_rank2(const float *v, const uint32_t *rank2, const double *side_stats, int64_t M, double *out,
                             void *ws, size_t ws_bytes, hicgat_stream_t stream);
/* dSCC of coords [N, 3] against the prepared upper triangle of the truth: pair k's distance is
 * computed with the expression of hicgat_pairdist_fwd (the same bits) and goes straight into the
 * sort's key; the distance matrix is never stored.  M = N (N - 1) / 2, 2 <= N <= 65536. */
int hicgat_dscc_coords(const float *coords, int N, const uint32_t *rank2, const double *side_stats, double *out,
                       void *ws, size_t ws_bytes, hicgat_stream_t stream);

/* ---- measurement infrastructure (no reference counterpart) ----------------------------------
 * An emulated collective for the simulated P-rank step (bench.py --simulate-world,
 * hicgat.dist.SimComm): `workgroups` x `threads` threads resident on the device for `us`
 * microseconds of wall time, enqueued where the RCCL call would be, so the captured rank step
 * shows the modeled collective's duration, its overlap with the kernels on other streams and the
 * CU slots it holds.  Not used by the training path. */
int hicgat_sim_collective(float us, int workgroups, int threads, hicgat_stream_t stream);

/* ---- streams and stamps (host plumbing; no reference counterpart) ----------------------------
 * A non-blocking HIP stream at `priority` (hipStreamCreateWithPriority), made ONCE per device and
 * name by hicgat.streams and kept for the process: every side / comm / warm-up stream of the step
 * is one of these, never a stream from torch's round-robin pool (which aliases after 32 requests),
 * so two lanes of one step are always two streams.  *out receives the stream. */
int hicgat_stream_create(int priority, hicgat_stream_t *out);
/* out[slot] = the device's steady wall clock (100 MHz counter) when this one-wave launch runs on
 * `stream`: enqueued at fork / join points of a captured step it records, per replay, when each
 * branch started and ended (tests/test_gpu_overlap.py).  out 8-B aligned, slot >= 0. */
int hicgat_wall_stamp(unsigned long long *out, int slot, hicgat_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* HICGAT_H */
