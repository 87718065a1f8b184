// GATConv forward on gfx950: attention logits (a2) and the entry points of the fused edge-softmax +
// aggregation (a4+a5), whose per-row body is agg_fwd_row (gat_agg.hpp: reference ops, layout, design).
// Here: the logits kernel, the (2, 256) entry kernel with its measured launch parameters, and the C
// ABI, which routes every other supported shape to gat_generic.hip.  A launch covers rows
// [row_begin, row_end) (a rank's destination shard).
#include "gat_agg.hpp"

namespace hicgat {

// ---- a2: a_src[n,h] = <h[n,h,:], att_src[h,:]>, a_dst likewise (one wave per row). -------------
__global__ __launch_bounds__(256) void att_logits_kernel(const float *__restrict__ h,
                                                         const float *__restrict__ att_s,
                                                         const float *__restrict__ att_d, int N,
                                                         int H, int C, float *__restrict__ a_src,
                                                         float *__restrict__ a_dst) {
  const int lane = lane_id();
  const int n = blockIdx.x * 4 + wave_in_block();
  if (n >= N) return;
  const int D = H * C;
  const float4 *h4 = reinterpret_cast<const float4 *>(h + (size_t)n * D);
  const float4 *s4 = reinterpret_cast<const float4 *>(att_s);
  const float4 *d4 = reinterpret_cast<const float4 *>(att_d);
  // C % 4 == 0: a float4 never straddles two heads.  Heads are visited one after the other.
  for (int hh = 0; hh < H; ++hh) {
    float ps = 0.f, pd = 0.f;
    for (int q = lane; q < C / 4; q += 64) {
      const int idx = hh * (C / 4) + q;
      const float4 v = h4[idx];
      ps += f4_dot(v, s4[idx]);
      pd += f4_dot(v, d4[idx]);
    }
    ps = wave_sum(ps);
    pd = wave_sum(pd);
    if (lane == 0) {
      a_src[(size_t)n * H + hh] = ps;
      a_dst[(size_t)n * H + hh] = pd;
    }
  }
}

// ---- a4+a5 at H = 2, C = 256 (D = 512, the GATConv(512, 256, heads=2) of models.py:619): agg_fwd_row
// at <2, 256> (lane l holds float4 #l of head 0 and float4 #l of head 1, 8 neighbours in flight)
// under the name the profiles and bench.py know, with its own launch bounds.  SPLIT is the gather
// half of the tiled form (gat_tiles.hip).
template <bool TRAIN, int ACT, bool SPLIT = false>
__global__ __launch_bounds__(256, 1) void agg_fwd_h2c256_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ bias, float ns, float *__restrict__ out, float *__restrict__ out2,
    float *__restrict__ row_stats, const int *__restrict__ rowptr_s = nullptr,
    const int *__restrict__ col_s = nullptr) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i < row_end)
    agg_fwd_row<2, 256, TRAIN, ACT, SPLIT>(i, rowptr, col, rowptr_s, col_s, h, a_src, a_dst, bias, ns, out, out2,
                                           row_stats);
}

// The gather half of hicgat_gat_agg_fwd_tiled (gat_tiles.hip): raw sums over the sparse remainder.
int agg_fwd_split_launch(const int *rowptr, const int *col, const int *rowptr_s, const int *col_s, int row_begin,
                         int row_end, const float *h, const float *a_src, const float *a_dst, float ns, float *out,
                         float *out2, float *row_stats, hipStream_t s) {
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
  if (out2)
    hipLaunchKernelGGL((agg_fwd_h2c256_kernel<true, 0, true>), grid, block, 0, s, rowptr, col, row_begin, row_end,
                       h, a_src, a_dst, nullptr, ns, out, out2, row_stats, rowptr_s, col_s);
  else
    hipLaunchKernelGGL((agg_fwd_h2c256_kernel<false, 0, true>), grid, block, 0, s, rowptr, col, row_begin, row_end,
                       h, a_src, a_dst, nullptr, ns, out, out2, row_stats, rowptr_s, col_s);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

// The same row body with attention dropout (DROP; gat_agg.hpp): a kernel of its own, so that the one
// above keeps its arguments and code.  No SPLIT form, and no occupancy cap: nobody has measured one.
template <bool TRAIN, int ACT>
__global__ __launch_bounds__(256, 1) void agg_fwd_drop_h2c256_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ bias, float ns, float *__restrict__ out, float *__restrict__ out2,
    float *__restrict__ row_stats, AttnMaskArgs mk) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i < row_end)
    agg_fwd_row<2, 256, TRAIN, ACT, false, true>(i, rowptr, col, nullptr, nullptr, h, a_src, a_dst, bias, ns, out,
                                                 out2, row_stats, mk);
}

// gat_generic.hip: the supported-shape rule and the kernels of every supported shape but (2, 256)
int agg_fwd_drop_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                                const float *h, const float *a_src, const float *a_dst, const float *bias, float ns,
                                int act, float *out, float *out2, float *row_stats, const AttnMaskArgs &mk,
                                hipStream_t s);
int attn_mask_launch(const int *rowptr, const int *col, int N, int H, const AttnMaskArgs &mk, uint8_t *mask,
                     hipStream_t s);
bool gat_shape_supported(int H, int C);
int agg_fwd_generic_launch(const int *rowptr, const int *col, int H, int C, int row_begin, int row_end,
                           const float *h, const float *a_src, const float *a_dst, const float *bias, float ns,
                           int act, float *out, float *out2, float *row_stats, hipStream_t s);

}  // namespace hicgat

using namespace hicgat;

extern "C" int hicgat_gat_att_logits(const float *h, const float *att_src, const float *att_dst,
                                     int N, int H, int C, float *a_src, float *a_dst,
                                     hicgat_stream_t stream) {
  if (N < 0 || H <= 0 || C <= 0 || (C % 4) != 0) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!h || !att_src || !att_dst || !a_src || !a_dst) return HICGAT_EINVAL;
  hipLaunchKernelGGL(att_logits_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, h,
                     att_src, att_dst, N, H, C, a_src, a_dst);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

// Unused dynamic LDS per workgroup of the gather launch below: 3 workgroups per CU (160 KiB / 52 KiB)
// instead of the 4 its 98 VGPRs allow -- fewer rows in flight per CU, fewer L2 misses: the
// single-GPU step 1.798-1.803 vs 1.820-1.821 ms together with the source pass's cap (gat_bwd.hip;
// 2 per CU: +30 us), profiles/r05at_gather_occupancy_ab.txt
constexpr size_t kAggFwdOccLds = 53248;

extern "C" int hicgat_gat_agg_fwd(const int32_t *rowptr, const int32_t *col, int N, int nnz,
                                  int H, int C, int row_begin, int row_end, const float *h,
                                  const float *a_src, const float *a_dst, const float *bias,
                                  float neg_slope, int act, float *out, float *out2,
                                  float *row_stats, hicgat_stream_t stream) {
  if (N < 0 || nnz < 0 || row_begin < 0 || row_end > N || row_begin > row_end) return HICGAT_EINVAL;
  if (act != 0 && act != 1) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (row_end == row_begin) return HICGAT_OK;
  if (!rowptr || !col || !h || !a_src || !a_dst || !bias || !out || !row_stats) return HICGAT_EINVAL;
  if (H != 2 || C != 256)   // the generic kernels, without the (2, 256) launch's occupancy cap (unmeasured there)
    return agg_fwd_generic_launch(rowptr, col, H, C, row_begin, row_end, h, a_src, a_dst, bias, neg_slope, act, out,
                                  out2, row_stats, (hipStream_t)stream);
  const int rows = row_end - row_begin;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define HICGAT_FWD_LAUNCH(TR, AC)                                                                  \
  hipLaunchKernelGGL((agg_fwd_h2c256_kernel<TR, AC>), grid, block, kAggFwdOccLds, s, rowptr, col, row_begin, \
                     row_end, h, a_src, a_dst, bias, neg_slope, out, out2, row_stats)
  if (out2) {
    if (act) HICGAT_FWD_LAUNCH(true, 1);
    else HICGAT_FWD_LAUNCH(true, 0);
  } else {
    if (act) HICGAT_FWD_LAUNCH(false, 1);
    else HICGAT_FWD_LAUNCH(false, 0);
  }
#undef HICGAT_FWD_LAUNCH
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

// ---- attention dropout: hicgat_gat_agg_fwd with each alpha_ij multiplied by its keep factor ------
extern "C" int hicgat_gat_agg_drop_fwd(const int32_t *rowptr, const int32_t *col, int N, int nnz, int H, int C,
                                       int row_begin, int row_end, const float *h, const float *a_src,
                                       const float *a_dst, const float *bias, float neg_slope, int act, float *out,
                                       float *out2, float *row_stats, double p, uint64_t seed,
                                       const int64_t *step_counter, int64_t step_value, uint32_t site,
                                       hicgat_stream_t stream) {
  if (N < 0 || nnz < 0 || row_begin < 0 || row_end > N || row_begin > row_end) return HICGAT_EINVAL;
  if (act != 0 && act != 1) return HICGAT_EINVAL;
  if (!p_ok(p) || !attn_site_ok(site) || misaligned(step_counter, 8)) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (row_end == row_begin) return HICGAT_OK;
  if (!rowptr || !col || !h || !a_src || !a_dst || !bias || !out || !row_stats) return HICGAT_EINVAL;
  const AttnMaskArgs mk = attn_mask_args(p, seed, step_counter, step_value, site);
  hipStream_t s = (hipStream_t)stream;
  if (H != 2 || C != 256)
    return agg_fwd_drop_generic_launch(rowptr, col, H, C, row_begin, row_end, h, a_src, a_dst, bias, neg_slope, act,
                                       out, out2, row_stats, mk, s);
  const dim3 grid((row_end - row_begin + 3) / 4), block(256);
#define HICGAT_FWD_LAUNCH(TR, AC)                                                                             \
  hipLaunchKernelGGL((agg_fwd_drop_h2c256_kernel<TR, AC>), grid, block, 0, s, rowptr, col, row_begin, row_end, \
                     h, a_src, a_dst, bias, neg_slope, out, out2, row_stats, mk)
  if (out2) {
    if (act) HICGAT_FWD_LAUNCH(true, 1);
    else HICGAT_FWD_LAUNCH(true, 0);
  } else {
    if (act) HICGAT_FWD_LAUNCH(false, 1);
    else HICGAT_FWD_LAUNCH(false, 0);
  }
#undef HICGAT_FWD_LAUNCH
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_gat_attn_mask(const int32_t *rowptr, const int32_t *col, int N, int H, double p, uint64_t seed,
                                    const int64_t *step_counter, int64_t step_value, uint32_t site, uint8_t *mask,
                                    hicgat_stream_t stream) {
  if (N < 0 || !p_ok(p) || !attn_site_ok(site) || misaligned(step_counter, 8)) return HICGAT_EINVAL;
  if (H < 1 || H > 4) return HICGAT_EUNSUPPORTED;
  if (N == 0) return HICGAT_OK;
  if (!rowptr || !col || !mask) return HICGAT_EINVAL;
  return attn_mask_launch(rowptr, col, N, H, attn_mask_args(p, seed, step_counter, step_value, site), mask,
                          (hipStream_t)stream);
}
