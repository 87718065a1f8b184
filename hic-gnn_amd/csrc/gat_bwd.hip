// GATConv backward on gfx950 (autograd of a4+a5 in the reference: segment_csr/gather_csr/
// index_select/leaky_relu/exp backward of PyG 1.7.2), without float atomics.
//
// With out_i = sum_j alpha_ij h_j (+bias) and alpha the ptr-path softmax of
// e_ij = lrelu(a_src[j] + a_dst[i]):
//   g_ij   = <dout_i, h_j>                   (per head)
//   de_ij  = alpha_ij (g_ij - delta_i),      delta_i = sum_j alpha_ij g_ij
//   ds_ij  = de_ij * lrelu'(e_ij)
//   da_dst[i] = sum_j ds_ij,  da_src[j] = sum_i ds_ij,  dh_j = sum_i alpha_ij dout_i (+ logit terms)
// (the +1e-16 of the softmax denominator and the detached-max gradient change these by
// O(1e-16) relative; both are dropped.)
//
// Destination side, two forms with the same outputs (delta_i, da_dst_i into row_stats[i, 2H:4H]):
//  * agg_bwd_rows (the training path): no gather, from the forward's TRAIN outputs;
//  * agg_bwd_dst (stand-alone form, needs only h): gathers h_j and forms every g_ij.
// Source side (row r) gathers dout_i of the rows that have r as a neighbour.  The graph is
// structurally symmetric (to_symmetric, utils.py:71), so row r's own CSR list *is* that set: the
// transpose needs no permutation array and no atomics.
//
// The per-row bodies of the three passes are gat_agg.hpp's (agg_bwd_rows_row, agg_bwd_dst_row,
// agg_bwd_src_row).  Here: their entry kernels -- for (2, 256) under the names the profiles know, with
// measured launch parameters, and for every other supported shape -- one launch per pass (the
// dispatcher is gat_launch.hpp's), the parameter-gradient reductions, and the C ABI.
#include <algorithm>
#include <cstdlib>

#include "gat_agg.hpp"
#include "gat_launch.hpp"

namespace hicgat {

__global__ __launch_bounds__(256) void agg_bwd_dst_h2c256_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ dout, float ns, float *__restrict__ row_stats) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i < row_end) agg_bwd_dst_row<2, 256>(i, rowptr, col, h, a_src, a_dst, dout, ns, row_stats);
}

template <int H, int C>
__global__ __launch_bounds__(256) void agg_bwd_dst_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ dout, float ns, float *__restrict__ row_stats) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i >= row_end) return;
  agg_bwd_dst_row<H, C>(i, rowptr, col, h, a_src, a_dst, dout, ns, row_stats);
}

// One workgroup per 4 rows (a persistent grid of 2-3 workgroups per CU, leaving slots to the side
// stream's GEMMs, measured the same step or slower and was removed).
// REMAP: the XCD-aware block order (each XCD a contiguous row range: the rows of a banded Hi-C
// neighbourhood share that XCD's L2).  Off (plain round-robin over the XCDs) for the multi-GPU "slab"
// pass, whose heavy rows -- the rank's own diagonal block -- are contiguous: under the remap they
// would all land on one XCD.
// MK is empty or one AttnMaskArgs: attention dropout (DROP; gat_agg.hpp) is the same kernel with the
// mask arguments appended, as in the forward (gat_fwd.hip); no SPLIT form.
template <bool SPLIT = false, bool REMAP = true, class... MK>
__global__ __launch_bounds__(256) void agg_bwd_src_h2c256_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ row_stats, int64_t ldr, const float *__restrict__ dout, int64_t ldq,
    const float *__restrict__ att_s, const float *__restrict__ att_d, float ns,
    float *__restrict__ dh, float *__restrict__ da_src, MK... mk) {
  const int r = row_begin + (REMAP ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x) * 4 + wave_in_block();
  if (r < row_end)
    agg_bwd_src_row<2, 256, SPLIT, sizeof...(MK) != 0>(r, rowptr, col, h, a_src, a_dst, row_stats, ldr, dout, ldq,
                                                       att_s, att_d, ns, dh, da_src, mk...);
}

template <int H, int C, bool REMAP, class... MK>
__global__ __launch_bounds__(256) void agg_bwd_src_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ row_stats, int64_t ldr, const float *__restrict__ dout, int64_t ldq,
    const float *__restrict__ att_s, const float *__restrict__ att_d, float ns,
    float *__restrict__ dh, float *__restrict__ da_src, MK... mk) {
  const int r = row_begin + (REMAP ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x) * 4 + wave_in_block();
  if (r >= row_end) return;
  agg_bwd_src_row<H, C, false, sizeof...(MK) != 0>(r, rowptr, col, h, a_src, a_dst, row_stats, ldr, dout, ldq, att_s,
                                                   att_d, ns, dh, da_src, mk...);
}

template <int ACT>
__global__ __launch_bounds__(256) void agg_bwd_rows_kernel(int row_begin, int row_end,
                                                           const float *__restrict__ g,
                                                           const float *__restrict__ y,
                                                           const float *__restrict__ bias,
                                                           const float *__restrict__ out2,
                                                           float *__restrict__ dout, int64_t ldq,
                                                           float *__restrict__ row_stats) {
  const int i = row_begin + blockIdx.x * 4 + wave_in_block();
  if (i < row_end) agg_bwd_rows_row<2, 256, ACT>(i, g, y, bias, out2, dout, ldq, row_stats);
}

template <int H, int C, int ACT>
__global__ __launch_bounds__(256) void agg_bwd_rows_generic_kernel(int row_begin, int row_end,
                                                                   const float *__restrict__ g,
                                                                   const float *__restrict__ y,
                                                                   const float *__restrict__ bias,
                                                                   const float *__restrict__ out2,
                                                                   float *__restrict__ dout, int64_t ldq,
                                                                   float *__restrict__ row_stats) {
  const int i = row_begin + blockIdx.x * 4 + wave_in_block();
  if (i >= row_end) return;
  agg_bwd_rows_row<H, C, ACT>(i, g, y, bias, out2, dout, ldq, row_stats);
}

// ---- GATConv parameter gradients: deterministic two-stage column reductions over N rows. ------
// Three parts: datt_src (sum_n da_src[n,h] h[n,:]), datt_dst (sum_n da_dst[n,h] h[n,:]) and dbias
// (sum_n dout[n,:]); any subset may be asked for (PARTS bit 0 / 1 / 2), so datt_dst and dbias --
// known after the gather-free row pass -- can be summed beside the source-side gather and only
// datt_src is left behind it.  Each part's sum runs in the same order whatever subset is asked for
// (bitwise the all-parts call).
// stage 1: block b sums rows [b*R, (b+1)*R) into part[b][P][D] (the P asked-for parts in order);
// stage 2: one thread per output column sums the partials in block order.
// row blocks of stage 1 (128 left half the CUs idle; 1024 measured slower: stage 2 sums twice the partials)
constexpr int kParamBlocks = 512;

template <int PARTS>
__global__ __launch_bounds__(256) void param_grad_stage1(const float *__restrict__ h,
                                                         const float *__restrict__ dout,
                                                         const float *__restrict__ da_src,
                                                         const float *__restrict__ row_stats, int N,
                                                         int H, int C, int rows_per_block,
                                                         float *__restrict__ part) {
  constexpr bool kS = PARTS & 1, kT = PARTS & 2, kB = PARTS & 4;
  constexpr int P = (int)kS + (int)kT + (int)kB;
  const int D = H * C, Q = D / 4;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(N, r0 + rows_per_block);
  const float4 *h4 = reinterpret_cast<const float4 *>(h);
  const float4 *g4 = reinterpret_cast<const float4 *>(dout);
  float4 *p4 = reinterpret_cast<float4 *>(part + (size_t)blockIdx.x * P * D);
  for (int q = threadIdx.x; q < Q; q += blockDim.x) {
    const int hd = (4 * q) / C;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = s, b = s;
#pragma unroll 4   // several rows' loads in flight per thread (one wave per SIMD at this grid size)
    for (int n = r0; n < r1; ++n) {
      if (kS || kT) {
        const float4 hv = h4[(size_t)n * Q + q];
        if (kS) s = f4_fma(da_src[(size_t)n * H + hd], hv, s);
        if (kT) t = f4_fma(row_stats[(size_t)n * 4 * H + 3 * H + hd], hv, t);
      }
      if (kB) {
        const float4 gv = g4[(size_t)n * Q + q];
        b.x += gv.x; b.y += gv.y; b.z += gv.z; b.w += gv.w;
      }
    }
    int o = 0;
    if (kS) p4[(o++) * Q + q] = s;
    if (kT) p4[(o++) * Q + q] = t;
    if (kB) p4[o * Q + q] = b;
  }
}

// block = 16 output columns x 16 groups (256 threads); group g adds partials b = g, g+16, ...;
// the groups are combined in order through LDS (fixed order: bitwise reproducible).  The partial
// range is cut 16 ways to keep each thread's chain of dependent loads short (32 partials at
// nblk = 512); 256-thread blocks (P*D/16 of them) find room on CUs that the side stream's GEMMs
// occupy, where 1024-thread blocks waited (25-43 us in the step instead of a few).
constexpr int kPG2Groups = 16, kPG2Cols = 16;
struct PGOut {
  float *o[3];
};
__global__ __launch_bounds__(256) void param_grad_stage2(const float *__restrict__ part, int nblk, int P, int D,
                                                         PGOut out, int accumulate) {
  __shared__ float red[kPG2Groups][kPG2Cols];
  const int cl = threadIdx.x % kPG2Cols, grp = threadIdx.x / kPG2Cols;
  const int c = blockIdx.x * kPG2Cols + cl;
  float s = 0.f;
  if (c < P * D) {
    // all of this thread's partials (<= kParamBlocks / 16 = 32) in flight together, then added in order
    constexpr int kMax = (kParamBlocks + kPG2Groups - 1) / kPG2Groups;
    float v[kMax];
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
      const int b = grp + i * kPG2Groups;
      v[i] = b < nblk ? part[(size_t)b * P * D + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kMax; ++i) s += v[i];
  }
  red[grp][cl] = s;
  __syncthreads();
  if (grp == 0 && c < P * D) {
    float t = red[0][cl];
#pragma unroll
    for (int g = 1; g < kPG2Groups; ++g) t += red[g][cl];
    float *o = out.o[c / D] + c % D;
    *o = t + (accumulate ? *o : 0.f);
  }
}

// Unused dynamic LDS per workgroup of the whole-graph source pass at (2, 256): 5 workgroups per CU
// (the 160 KiB / 32 KiB) instead of the 7 its 68 VGPRs allow -- fewer rows in flight per CU (L2
// misses), and the side stream's dW kernels wait for the pass instead of sharing its CUs: single-GPU
// step -8 us alone, -20 us with the forward gather's cap (gat_fwd.hip; 3 per CU: even, 6 per CU:
// even), profiles/r05at_gather_occupancy_ab.txt.  It goes with the remapped pass of that kernel only:
// the round-robin order, the DROP form and the other shapes are unmeasured and launch without it.
constexpr size_t kSrcOccLds = 32768;

// The gather half of the source pass's tiled form (gat_tiles.hip): the sparse remainder's shares.
int agg_bwd_src_split_launch(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const hicgat_gat_tiles &t,
                             const SrcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((agg_bwd_src_h2c256_kernel<true>), dim3((g.row_end - g.row_begin + 3) / 4), dim3(256), 0, s,
                     t.rowptr_s, t.col_s, g.row_begin, g.row_end, f.h, f.a_src, f.a_dst, a.row_stats, a.ldr, a.dout,
                     a.ldq4, nullptr, nullptr, f.neg_slope, a.dh, a.da_src);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

// The source pass's one launch: REMAP = remap, DROP = a mask given.
template <class... MK>
int agg_bwd_src_launch(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const SrcArgs &a, bool remap,
                       hipStream_t s, MK... mk) {
  const dim3 grid((g.row_end - g.row_begin + 3) / 4), block(256);
  return for_gat_shape(f.H, f.C, [&](auto shape) {
    return with_flags(
        [&](auto rm) {
          using S = decltype(shape);
          constexpr bool REMAP = rm.value;
          if constexpr (S::h2c256)
            hipLaunchKernelGGL((agg_bwd_src_h2c256_kernel<false, REMAP, MK...>), grid, block,
                               REMAP && !sizeof...(MK) ? kSrcOccLds : 0, s, g.rowptr, g.col, g.row_begin, g.row_end,
                               f.h, f.a_src, f.a_dst, a.row_stats, a.ldr, a.dout, a.ldq4, a.att_s, a.att_d,
                               f.neg_slope, a.dh, a.da_src, mk...);
          else
            hipLaunchKernelGGL((agg_bwd_src_generic_kernel<S::H, S::C, REMAP, MK...>), grid, block, 0, s, g.rowptr,
                               g.col, g.row_begin, g.row_end, f.h, f.a_src, f.a_dst, a.row_stats, a.ldr, a.dout, a.ldq4,
                               a.att_s, a.att_d, f.neg_slope, a.dh, a.da_src, mk...);
          HICGAT_CHECK_LAUNCH();
          return HICGAT_OK;
        },
        remap);
  });
}

}  // namespace hicgat

using namespace hicgat;

extern "C" int hicgat_gat_agg_bwd_dst(const int32_t *rowptr, const int32_t *col, int N, int H,
                                      int C, int row_begin, int row_end, const float *h,
                                      const float *a_src, const float *a_dst, const float *dout,
                                      float neg_slope, float *row_stats, hicgat_stream_t stream) {
  if (N < 0 || row_begin < 0 || row_end > N || row_begin > row_end) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (row_end == row_begin) return HICGAT_OK;
  if (!rowptr || !col || !h || !a_src || !a_dst || !dout || !row_stats) return HICGAT_EINVAL;
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  return for_gat_shape(H, C, [&](auto shape) {
    using S = decltype(shape);
    if constexpr (S::h2c256)
      hipLaunchKernelGGL(agg_bwd_dst_h2c256_kernel, grid, block, 0, s, rowptr, col, row_begin, row_end, h, a_src, a_dst,
                         dout, neg_slope, row_stats);
    else
      hipLaunchKernelGGL((agg_bwd_dst_generic_kernel<S::H, S::C>), grid, block, 0, s, rowptr, col, row_begin, row_end,
                         h, a_src, a_dst, dout, neg_slope, row_stats);
    HICGAT_CHECK_LAUNCH();
    return HICGAT_OK;
  });
}

// The rules of every form, in the order of include/hicgat.h; the tiled form's own follow in agg_bwd_src_tiled,
// which reads the remainder's CSR in place of the graph's.  HICGAT_SRC_ROUND_ROBIN turns the XCD remap off.
extern "C" int hicgat_gat_agg_bwd_src(const hicgat_gat_graph *graph, const hicgat_gat_feats *feats,
                                      const float *row_stats, int64_t ld_stats, const float *dout, int64_t ld_dout,
                                      const float *att_src, const float *att_dst, float *dh, float *da_src, int flags,
                                      const hicgat_attn_drop *drop, const hicgat_gat_tiles *tiles,
                                      hicgat_stream_t stream) {
  if (!graph || !feats || (drop && tiles)) return HICGAT_EINVAL;
  if (drop && !attn_drop_ok(*drop)) return HICGAT_EINVAL;
  if ((flags & ~HICGAT_SRC_ROUND_ROBIN) || (flags && tiles)) return HICGAT_EINVAL;
  const hicgat_gat_graph &g = *graph;
  const hicgat_gat_feats &f = *feats;
  if (g.N < 0 || g.row_begin < 0 || g.row_end > g.N || g.row_begin > g.row_end || (tiles && tiles->ntiles < 0))
    return HICGAT_EINVAL;
  if (tiles ? f.H != 2 || f.C != 256 : !gat_shape_supported(f.H, f.C)) return HICGAT_EUNSUPPORTED;
  if (ld_stats < 4 * f.H || ld_stats % 4 || ld_dout < f.H * f.C || ld_dout % 4) return HICGAT_EINVAL;
  if (g.row_end == g.row_begin) return HICGAT_OK;
  if ((!tiles && (!g.rowptr || !g.col)) || !f.h || !f.a_src || !f.a_dst || !row_stats || !dout || !att_src ||
      !att_dst || !dh || !da_src)
    return HICGAT_EINVAL;
  const SrcArgs a{row_stats, ld_stats, dout, ld_dout / 4, att_src, att_dst, dh, da_src};
  const bool remap = !(flags & HICGAT_SRC_ROUND_ROBIN);
  hipStream_t s = (hipStream_t)stream;
  if (tiles) return agg_bwd_src_tiled(g, f, *tiles, a, s);
  if (drop) return agg_bwd_src_launch(g, f, a, remap, s, attn_mask_args(*drop));
  return agg_bwd_src_launch(g, f, a, remap, s);
}

extern "C" int hicgat_gat_agg_bwd_rows(int N, int H, int C, int row_begin, int row_end, int act,
                                       const float *g, const float *y, const float *bias,
                                       const float *out2, float *dout, int64_t ld_dout,
                                       float *row_stats, hicgat_stream_t stream) {
  if (N < 0 || row_begin < 0 || row_end > N || row_begin > row_end) return HICGAT_EINVAL;
  if (act && (ld_dout < (int64_t)H * C || ld_dout % 4)) return HICGAT_EINVAL;
  if (act != 0 && act != 1) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (row_end == row_begin) return HICGAT_OK;
  if (!g || !y || !bias || !out2 || !row_stats || (act && !dout)) return HICGAT_EINVAL;
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ldq4 = act ? ld_dout / 4 : 0;   // act = 0 writes no dout
  return for_gat_shape(H, C, [&](auto shape) {
    return with_flags(
        [&](auto relu) {
          using S = decltype(shape);
          constexpr int ACT = relu.value;
          if constexpr (S::h2c256)
            hipLaunchKernelGGL(agg_bwd_rows_kernel<ACT>, grid, block, 0, s, row_begin, row_end, g, y, bias, out2, dout,
                               ldq4, row_stats);
          else
            hipLaunchKernelGGL((agg_bwd_rows_generic_kernel<S::H, S::C, ACT>), grid, block, 0, s, row_begin, row_end, g,
                               y, bias, out2, dout, ldq4, row_stats);
          HICGAT_CHECK_LAUNCH();
          return HICGAT_OK;
        },
        act != 0);
  });
}

extern "C" size_t hicgat_gat_param_grad_workspace_bytes(int N, int D) {
  (void)N;
  return (size_t)kParamBlocks * 3 * (size_t)(D > 0 ? D : 0) * sizeof(float);
}

extern "C" int hicgat_gat_param_grad(const float *h, const float *dout, const float *da_src,
                                     const float *row_stats, int N, int H, int C, float *datt_src,
                                     float *datt_dst, float *dbias, int accumulate, void *workspace,
                                     size_t workspace_bytes, hicgat_stream_t stream) {
  if (N < 0 || H <= 0 || C <= 0 || (C % 4) != 0) return HICGAT_EINVAL;
  const int D = H * C;
  const int parts = (datt_src ? 1 : 0) | (datt_dst ? 2 : 0) | (dbias ? 4 : 0);
  if (!parts || !workspace) return HICGAT_EINVAL;
  if (((parts & 3) && !h) || ((parts & 1) && !da_src) || ((parts & 2) && !row_stats) || ((parts & 4) && !dout))
    return HICGAT_EINVAL;
  if (workspace_bytes < hicgat_gat_param_grad_workspace_bytes(N, D)) return HICGAT_EINVAL;
  const int rpb = N > 0 ? (N + kParamBlocks - 1) / kParamBlocks : 1;
  const int nblk = N > 0 ? (N + rpb - 1) / rpb : 0;
  float *part = static_cast<float *>(workspace);
  PGOut out{};
  int P = 0;
  if (datt_src) out.o[P++] = datt_src;
  if (datt_dst) out.o[P++] = datt_dst;
  if (dbias) out.o[P++] = dbias;
  hipStream_t s = (hipStream_t)stream;
  if (nblk > 0) {
    static constexpr decltype(&param_grad_stage1<1>) kStage1[8] = {   // by PARTS (1..7)
        nullptr,
        param_grad_stage1<1>, param_grad_stage1<2>, param_grad_stage1<3>, param_grad_stage1<4>,
        param_grad_stage1<5>, param_grad_stage1<6>, param_grad_stage1<7>};
    hipLaunchKernelGGL(kStage1[parts], dim3(nblk), dim3(128), 0, s, h, dout, da_src, row_stats, N, H, C, rpb, part);
    HICGAT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(param_grad_stage2, dim3((P * D + kPG2Cols - 1) / kPG2Cols), dim3(kPG2Cols * kPG2Groups), 0, s,
                     part, nblk, P, D, out, accumulate);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}
