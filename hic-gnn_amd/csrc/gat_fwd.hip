// GATConv forward on gfx950: attention logits (a2) and the fused edge-softmax + aggregation (a4+a5),
// whose per-row body is agg_fwd_row (gat_agg.hpp: reference ops, layout, design).  Here: the logits
// kernel, the entry kernels of the aggregation -- one for (2, 256) with its measured launch
// parameters, one for every other supported shape -- their one launch (the dispatcher is
// gat_launch.hpp's), the attention-dropout mask kernel, and the C ABI.  A launch covers rows
// [row_begin, row_end) (a rank's destination shard).
#include "gat_agg.hpp"
#include "gat_launch.hpp"

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
// MK is empty or one AttnMaskArgs: attention dropout (DROP; gat_agg.hpp) is the same kernel with the
// mask arguments appended.  With the empty pack the arguments and the body are those of a kernel
// that knows no dropout, so those instances' code does not depend on DROP existing.
template <bool TRAIN, int ACT, bool SPLIT = false, class... MK>
__global__ __launch_bounds__(256, 1) void agg_fwd_h2c256_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ bias, float ns, float *__restrict__ out, float *__restrict__ out2,
    float *__restrict__ row_stats, const int *__restrict__ rowptr_s = nullptr,
    const int *__restrict__ col_s = nullptr, MK... mk) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i < row_end)
    agg_fwd_row<2, 256, TRAIN, ACT, SPLIT, sizeof...(MK) != 0>(i, rowptr, col, rowptr_s, col_s, h, a_src, a_dst, bias,
                                                               ns, out, out2, row_stats, mk...);
}

// Every other supported shape (the ones the reference's model zoo instantiates, models.py:
// GATConv(512, 128, heads=2), (512, 512, heads=2), (256, 256, heads=4), (512, 512, heads=1), ...).
template <int H, int C, bool TRAIN, int ACT, class... MK>
__global__ __launch_bounds__(256) void agg_fwd_generic_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, int row_begin, int row_end,
    const float *__restrict__ h, const float *__restrict__ a_src, const float *__restrict__ a_dst,
    const float *__restrict__ bias, float ns, float *__restrict__ out, float *__restrict__ out2,
    float *__restrict__ row_stats, MK... mk) {
  const int i = row_begin + xcd_remap(blockIdx.x, gridDim.x) * 4 + wave_in_block();
  if (i >= row_end) return;
  agg_fwd_row<H, C, TRAIN, ACT, false, sizeof...(MK) != 0>(i, rowptr, col, nullptr, nullptr, h, a_src, a_dst, bias,
                                                           ns, out, out2, row_stats, mk...);
}

template <int H>
__global__ __launch_bounds__(256) void attn_mask_kernel(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        int N, AttnMaskArgs mk, uint8_t *__restrict__ mask) {
  const int i = blockIdx.x * 4 + wave_in_block();
  if (i >= N) return;
  attn_mask_row<H>(i, rowptr, col, mk, mask);
}

// The gather half of the forward's tiled form (gat_tiles.hip): raw sums over the sparse remainder.
int agg_fwd_split_launch(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const hicgat_gat_tiles &t, float *out,
                         float *out2, float *row_stats, hipStream_t s) {
  const dim3 grid((g.row_end - g.row_begin + 3) / 4), block(256);
  return with_flags(
      [&](auto train) {
        hipLaunchKernelGGL((agg_fwd_h2c256_kernel<train.value, 0, true>), grid, block, 0, s, g.rowptr, g.col,
                           g.row_begin, g.row_end, f.h, f.a_src, f.a_dst, nullptr, f.neg_slope, out, out2, row_stats,
                           t.rowptr_s, t.col_s);
        HICGAT_CHECK_LAUNCH();
        return HICGAT_OK;
      },
      out2 != nullptr);
}

// Unused dynamic LDS per workgroup of the (2, 256) gather launch: 3 workgroups per CU (160 KiB / 52 KiB)
// instead of the 4 its 98 VGPRs allow -- fewer rows in flight per CU, fewer L2 misses: the
// single-GPU step 1.798-1.803 vs 1.820-1.821 ms together with the source pass's cap (gat_bwd.hip;
// 2 per CU: +30 us), profiles/r05at_gather_occupancy_ab.txt.  Measured for that kernel at N = 20000
// only: the DROP form and the other shapes launch without it.
constexpr size_t kAggFwdOccLds = 53248;

// The forward's one launch: TRAIN = out2 given, ACT = act, DROP = a mask given.
template <class... MK>
int agg_fwd_launch(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const float *bias, int act, float *out,
                   float *out2, float *row_stats, hipStream_t s, MK... mk) {
  const dim3 grid((g.row_end - g.row_begin + 3) / 4), block(256);
  return for_gat_shape(f.H, f.C, [&](auto shape) {
    return with_flags(
        [&](auto train, auto relu) {
          using S = decltype(shape);
          constexpr bool TRAIN = train.value;
          constexpr int ACT = relu.value;
          if constexpr (S::h2c256)
            hipLaunchKernelGGL((agg_fwd_h2c256_kernel<TRAIN, ACT, false, MK...>), grid, block,
                               sizeof...(MK) ? 0 : kAggFwdOccLds, s, g.rowptr, g.col, g.row_begin, g.row_end, f.h,
                               f.a_src, f.a_dst, bias, f.neg_slope, out, out2, row_stats, nullptr, nullptr, mk...);
          else
            hipLaunchKernelGGL((agg_fwd_generic_kernel<S::H, S::C, TRAIN, ACT, MK...>), grid, block, 0, s, g.rowptr,
                               g.col, g.row_begin, g.row_end, f.h, f.a_src, f.a_dst, bias, f.neg_slope, out, out2,
                               row_stats, mk...);
          HICGAT_CHECK_LAUNCH();
          return HICGAT_OK;
        },
        out2 != nullptr, act != 0);
  });
}

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

// The rules of every form, in the order of include/hicgat.h; the tiled form's own follow in agg_fwd_tiled.
extern "C" int hicgat_gat_agg_fwd(const hicgat_gat_graph *graph, const hicgat_gat_feats *feats, const float *bias,
                                  int act, float *out, float *out2, float *row_stats, const hicgat_attn_drop *drop,
                                  const hicgat_gat_tiles *tiles, hicgat_stream_t stream) {
  if (!graph || !feats || (drop && tiles)) return HICGAT_EINVAL;
  if (drop && !attn_drop_ok(*drop)) return HICGAT_EINVAL;
  const hicgat_gat_graph &g = *graph;
  const hicgat_gat_feats &f = *feats;
  if (g.N < 0 || g.nnz < 0 || g.row_begin < 0 || g.row_end > g.N || g.row_begin > g.row_end ||
      (tiles && tiles->ntiles < 0))
    return HICGAT_EINVAL;
  if (act != 0 && act != 1) return HICGAT_EINVAL;
  if (tiles ? f.H != 2 || f.C != 256 : !gat_shape_supported(f.H, f.C)) return HICGAT_EUNSUPPORTED;
  if (g.row_end == g.row_begin) return HICGAT_OK;
  if (!g.rowptr || !g.col || !f.h || !f.a_src || !f.a_dst || !bias || !out || !row_stats) return HICGAT_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (tiles) return agg_fwd_tiled(g, f, *tiles, bias, act, out, out2, row_stats, s);
  if (drop) return agg_fwd_launch(g, f, bias, act, out, out2, row_stats, s, attn_mask_args(*drop));
  return agg_fwd_launch(g, f, bias, act, out, out2, row_stats, s);
}

extern "C" int hicgat_gat_attn_mask(const int32_t *rowptr, const int32_t *col, int N, int H,
                                    const hicgat_attn_drop *drop, uint8_t *mask, hicgat_stream_t stream) {
  if (!drop || N < 0 || !attn_drop_ok(*drop)) return HICGAT_EINVAL;
  if (H < 1 || H > 4) return HICGAT_EUNSUPPORTED;
  if (N == 0) return HICGAT_OK;
  if (!rowptr || !col || !mask) return HICGAT_EINVAL;
  const AttnMaskArgs mk = attn_mask_args(*drop);
  const dim3 grid((N + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (H) {
    case 1: hipLaunchKernelGGL(attn_mask_kernel<1>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    case 2: hipLaunchKernelGGL(attn_mask_kernel<2>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    case 3: hipLaunchKernelGGL(attn_mask_kernel<3>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
    default: hipLaunchKernelGGL(attn_mask_kernel<4>, grid, block, 0, s, rowptr, col, N, mk, mask); break;
  }
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}
