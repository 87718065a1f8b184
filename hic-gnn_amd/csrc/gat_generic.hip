// The GATConv aggregation kernels for every supported (H, C) other than (2, 256): the shapes the
// reference's model zoo instantiates (models.py: GATConv(512, 128, heads=2), (512, 512, heads=2),
// (256, 256, heads=4), (512, 512, heads=1), ...).  The per-row bodies are gat_agg.hpp's, shared with
// the (2, 256) entry kernels of gat_fwd.hip / gat_bwd.hip; here are the __global__ wrappers that pick
// the row, and their launches.
//
// Launched without the dynamic-LDS occupancy caps of the (2, 256) launches (kAggFwdOccLds,
// kSrcOccLds): those were measured for (2, 256) at N = 20000 only, nobody has measured them for
// these shapes.
#include "gat_agg.hpp"

namespace hicgat {

template <int H, int C, bool TRAIN, int ACT>
__global__ __launch_bounds__(256) void agg_fwd_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ bias, float ns, float *__restrict__ out, float *__restrict__ out2,
    float *__restrict__ row_stats) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i >= row_end) return;
  agg_fwd_row<H, C, TRAIN, ACT, false>(i, rowptr, col, nullptr, nullptr, h, a_src, a_dst, bias, ns, out, out2,
                                       row_stats);
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

template <int H, int C>
__global__ __launch_bounds__(256) void agg_bwd_dst_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ dout, float ns, float *__restrict__ row_stats) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i >= row_end) return;
  agg_bwd_dst_row<H, C>(i, rowptr, col, h, a_src, a_dst, dout, ns, row_stats);
}

template <int H, int C, bool REMAP>
__global__ __launch_bounds__(256) void agg_bwd_src_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ row_stats, int64_t ldr, const float *__restrict__ dout, int64_t ldq,
    const float *__restrict__ att_s, const float *__restrict__ att_d, float ns,
    float *__restrict__ dh, float *__restrict__ da_src) {
  const int r = row_begin + (REMAP ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x) * 4 + wave_in_block();
  if (r >= row_end) return;
  agg_bwd_src_row<H, C, false>(r, rowptr, col, h, a_src, a_dst, row_stats, ldr, dout, ldq, att_s, att_d, ns, dh,
                               da_src);
}

// ---- attention dropout: the DROP forms of the forward and the source pass (gat_agg.hpp), kernels of
// their own so that the ones above keep their arguments and code.
template <int H, int C, bool TRAIN, int ACT>
__global__ __launch_bounds__(256) void agg_fwd_drop_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ bias, float ns, float *__restrict__ out, float *__restrict__ out2,
    float *__restrict__ row_stats, AttnMaskArgs mk) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i >= row_end) return;
  agg_fwd_row<H, C, TRAIN, ACT, false, true>(i, rowptr, col, nullptr, nullptr, h, a_src, a_dst, bias, ns, out, out2,
                                             row_stats, mk);
}

template <int H, int C, bool REMAP>
__global__ __launch_bounds__(256) void agg_bwd_src_drop_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ row_stats, int64_t ldr, const float *__restrict__ dout, int64_t ldq,
    const float *__restrict__ att_s, const float *__restrict__ att_d, float ns,
    float *__restrict__ dh, float *__restrict__ da_src, AttnMaskArgs mk) {
  const int r = row_begin + (REMAP ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x) * 4 + wave_in_block();
  if (r >= row_end) return;
  agg_bwd_src_row<H, C, false, true>(r, rowptr, col, h, a_src, a_dst, row_stats, ldr, dout, ldq, att_s, att_d, ns, dh,
                                     da_src, mk);
}

template <int H>
__global__ __launch_bounds__(256) void attn_mask_kernel(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        int N, AttnMaskArgs mk, uint8_t *__restrict__ mask) {
  const int i = blockIdx.x * 4 + wave_in_block();
  if (i >= N) return;
  attn_mask_row<H>(i, rowptr, col, mk, mask);
}

// every supported (H, C) but (2, 256)
#define HICGAT_GAT_SHAPES(X) X(1, 256) X(1, 512) X(1, 768) X(1, 1024) X(2, 128) X(2, 384) X(2, 512) X(3, 256) \
  X(4, 128) X(4, 256)

// The supported-shape rule (include/hicgat.h); (2, 256) is in it and has its own entry kernels.
bool gat_shape_supported(int H, int C) {
  return H >= 1 && H <= 4 && C > 0 && C % 128 == 0 && (H * C) % 256 == 0 && H * C <= 1024;
}

int agg_fwd_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                           const float *h, const float *a_src, const float *a_dst, const float *bias, float ns,
                           int act, float *out, float *out2, float *row_stats, hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_FWD_G(TR_, AC_, H_, C_)                                                                       \
  hipLaunchKernelGGL((agg_fwd_generic_kernel<H_, C_, TR_, AC_>), grid, block, 0, s, rowptr, col, row_begin, \
                     row_end, h, a_src, a_dst, bias, ns, out, out2, row_stats)
#define HICGAT_FWD_CASE(H_, C_)                 \
  if (H == H_ && C == C_) {                     \
    if (out2) {                                 \
      if (act) HICGAT_FWD_G(true, 1, H_, C_);   \
      else HICGAT_FWD_G(true, 0, H_, C_);       \
    } else {                                    \
      if (act) HICGAT_FWD_G(false, 1, H_, C_);  \
      else HICGAT_FWD_G(false, 0, H_, C_);      \
    }                                           \
    HICGAT_CHECK_LAUNCH();                      \
    return HICGAT_OK;                           \
  }
  HICGAT_GAT_SHAPES(HICGAT_FWD_CASE)
#undef HICGAT_FWD_CASE
#undef HICGAT_FWD_G
  return HICGAT_EUNSUPPORTED;
}

int agg_bwd_rows_generic_launch(int H, int C, int row_begin, int row_end, int act, const float *g, const float *y,
                                const float *bias, const float *out2, float *dout, int64_t ldq4,
                                float *row_stats, hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_ROWS_CASE(H_, C_)                                                                              \
  if (H == H_ && C == C_) {                                                                                   \
    if (act)                                                                                                  \
      hipLaunchKernelGGL((agg_bwd_rows_generic_kernel<H_, C_, 1>), grid, block, 0, s, row_begin, row_end, g, y, \
                         bias, out2, dout, ldq4, row_stats);                                                  \
    else                                                                                                      \
      hipLaunchKernelGGL((agg_bwd_rows_generic_kernel<H_, C_, 0>), grid, block, 0, s, row_begin, row_end, g, y, \
                         bias, out2, dout, (int64_t)0, row_stats);                                            \
    HICGAT_CHECK_LAUNCH();                                                                                    \
    return HICGAT_OK;                                                                                         \
  }
  HICGAT_GAT_SHAPES(HICGAT_ROWS_CASE)
#undef HICGAT_ROWS_CASE
  return HICGAT_EUNSUPPORTED;
}

int agg_bwd_dst_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                               const float *h, const float *a_src, const float *a_dst, const float *dout, float ns,
                               float *row_stats, hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_DST_CASE(H_, C_)                                                                                \
  if (H == H_ && C == C_) {                                                                                    \
    hipLaunchKernelGGL((agg_bwd_dst_generic_kernel<H_, C_>), grid, block, 0, s, rowptr, col, row_begin, row_end, \
                       h, a_src, a_dst, dout, ns, row_stats);                                                  \
    HICGAT_CHECK_LAUNCH();                                                                                     \
    return HICGAT_OK;                                                                                          \
  }
  HICGAT_GAT_SHAPES(HICGAT_DST_CASE)
#undef HICGAT_DST_CASE
  return HICGAT_EUNSUPPORTED;
}

int agg_bwd_src_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                               const float *h, const float *a_src, const float *a_dst, const float *row_stats,
                               int64_t ldr, const float *dout, int64_t ldq4, const float *att_s, const float *att_d,
                               float ns, float *dh, float *da_src, bool remap, hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_SRC_G(RM_, H_, C_)                                                                              \
  hipLaunchKernelGGL((agg_bwd_src_generic_kernel<H_, C_, RM_>), grid, block, 0, s, rowptr, col, row_begin,     \
                     row_end, h, a_src, a_dst, row_stats, ldr, dout, ldq4, att_s, att_d, ns, dh, da_src)
#define HICGAT_SRC_CASE(H_, C_)            \
  if (H == H_ && C == C_) {                \
    if (remap) HICGAT_SRC_G(true, H_, C_); \
    else HICGAT_SRC_G(false, H_, C_);      \
    HICGAT_CHECK_LAUNCH();                 \
    return HICGAT_OK;                      \
  }
  HICGAT_GAT_SHAPES(HICGAT_SRC_CASE)
#undef HICGAT_SRC_CASE
#undef HICGAT_SRC_G
  return HICGAT_EUNSUPPORTED;
}

int agg_fwd_drop_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                                const float *h, const float *a_src, const float *a_dst, const float *bias, float ns,
                                int act, float *out, float *out2, float *row_stats, const AttnMaskArgs &mk,
                                hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_FWD_G(TR_, AC_, H_, C_)                                                                            \
  hipLaunchKernelGGL((agg_fwd_drop_generic_kernel<H_, C_, TR_, AC_>), grid, block, 0, s, rowptr, col, row_begin, \
                     row_end, h, a_src, a_dst, bias, ns, out, out2, row_stats, mk)
#define HICGAT_FWD_CASE(H_, C_)                 \
  if (H == H_ && C == C_) {                     \
    if (out2) {                                 \
      if (act) HICGAT_FWD_G(true, 1, H_, C_);   \
      else HICGAT_FWD_G(true, 0, H_, C_);       \
    } else {                                    \
      if (act) HICGAT_FWD_G(false, 1, H_, C_);  \
      else HICGAT_FWD_G(false, 0, H_, C_);      \
    }                                           \
    HICGAT_CHECK_LAUNCH();                      \
    return HICGAT_OK;                           \
  }
  HICGAT_GAT_SHAPES(HICGAT_FWD_CASE)
#undef HICGAT_FWD_CASE
#undef HICGAT_FWD_G
  return HICGAT_EUNSUPPORTED;
}

int agg_bwd_src_drop_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                                    const float *h, const float *a_src, const float *a_dst, const float *row_stats,
                                    int64_t ldr, const float *dout, int64_t ldq4, const float *att_s,
                                    const float *att_d, float ns, float *dh, float *da_src, bool remap,
                                    const AttnMaskArgs &mk, hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_SRC_G(RM_, H_, C_)                                                                                \
  hipLaunchKernelGGL((agg_bwd_src_drop_generic_kernel<H_, C_, RM_>), grid, block, 0, s, rowptr, col, row_begin,  \
                     row_end, h, a_src, a_dst, row_stats, ldr, dout, ldq4, att_s, att_d, ns, dh, da_src, mk)
#define HICGAT_SRC_CASE(H_, C_)            \
  if (H == H_ && C == C_) {                \
    if (remap) HICGAT_SRC_G(true, H_, C_); \
    else HICGAT_SRC_G(false, H_, C_);      \
    HICGAT_CHECK_LAUNCH();                 \
    return HICGAT_OK;                      \
  }
  HICGAT_GAT_SHAPES(HICGAT_SRC_CASE)
#undef HICGAT_SRC_CASE
#undef HICGAT_SRC_G
  return HICGAT_EUNSUPPORTED;
}

int attn_mask_launch(const int *rowptr, const int *col, int N, int H, const AttnMaskArgs &mk, uint8_t *mask,
                     hipStream_t s) {
  const dim3 grid((N + 3) / 4), block(256);
  switch (H) {
    case 1: hipLaunchKernelGGL(attn_mask_kernel<1>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    case 2: hipLaunchKernelGGL(attn_mask_kernel<2>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    case 3: hipLaunchKernelGGL(attn_mask_kernel<3>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    case 4: hipLaunchKernelGGL(attn_mask_kernel<4>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    default: return HICGAT_EUNSUPPORTED;
  }
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

}  // namespace hicgat
