// GATConv attention weights as an output (PyG 1.7.2 GATConv.forward(..., return_attention_weights=True))
// and the backward of a loss that depends on them.
//
//   alpha_ij = exp(lrelu(z_ij) - max_i) / (sum_i + 1e-16),  z_ij = a_src[j] + a_dst[i]   (gat_agg.hpp's expression)
// For an incoming G = dL/dalpha [nnz, H], with s_ij = lrelu'(z_ij):
//   c_i = sum_k alpha_ik G_ik,   dz_ij = alpha_ij s_ij (G_ij - c_i)
//   da_dst^G[i] = sum_j dz_ij = sum_j alpha_ij s_ij G_ij - c_i sum_j alpha_ij s_ij
//   da_src^G[r] = sum_i dz_ir  over the rows i that have r as a neighbour = row r's own list (symmetric CSR);
//                 the edge (i, r) sits at tmap[e] for row r's edge e = (r, i)
//   dh_r += da_src^G[r] att_l + da_dst^G[r] att_r,  da_src[r] += da_src^G[r],  row_stats[r, 3H..4H) += da_dst^G[r]
// The backward is linear in (dout, G): these passes add onto what the aggregation's own passes wrote.
//
// One wave per row, lanes over the row's edges in 64-edge chunks, a fixed-order wave reduction; no
// atomics.  The backward passes read alpha as the forward wrote it (no exp) and take the slope from
// the sign of the recomputed logit, so they move col / tmap, alpha and G once each plus row scalars.
#include "common.hpp"
#include "gat_launch.hpp"   // gat_shape_supported

namespace hicgat {

namespace {

// tmap[e(r, i)] = e(i, r): lower-bound search for r in row i's sorted columns; -1 where (i, r) is
// missing (a CSR that is not structurally symmetric).
__global__ __launch_bounds__(256) void transpose_map_kernel(const int *__restrict__ rowptr,
                                                            const int *__restrict__ col, int N,
                                                            int *__restrict__ tmap) {
  const int r = blockIdx.x * 4 + wave_in_block();
  if (r >= N) return;
  const int beg = rowptr[r], end = rowptr[r + 1];
  for (int e = beg + lane_id(); e < end; e += 64) {
    const int i = col[e];
    int lo = rowptr[i], hi = rowptr[i + 1];
    const int stop = hi;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (col[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    tmap[e] = (lo < stop && col[lo] == r) ? lo : -1;
  }
}

template <int H>
__global__ __launch_bounds__(256) void alpha_kernel(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                    int N, const float *__restrict__ a_src,
                                                    const float *__restrict__ a_dst,
                                                    const float *__restrict__ row_stats, float ns,
                                                    float *__restrict__ alpha) {
  const int i = blockIdx.x * 4 + wave_in_block();
  if (i >= N) return;
  const int beg = rowptr[i], end = rowptr[i + 1];
  const float *rs = row_stats + (size_t)i * 4 * H;
  float ad[H], mx[H], den[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    ad[hh] = a_dst[(size_t)i * H + hh];
    mx[hh] = rs[hh];
    den[hh] = rs[H + hh] + 1e-16f;
  }
  for (int e = beg + lane_id(); e < end; e += 64) {
    const float *as = a_src + (size_t)col[e] * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh)
      alpha[(size_t)e * H + hh] = expf(lrelu(as[hh] + ad[hh], ns) - mx[hh]) / den[hh];
  }
}

// row i: c_i and da_dst^G[i]
template <int H>
__global__ __launch_bounds__(256) void alpha_bwd_dst_kernel(const int *__restrict__ rowptr,
                                                            const int *__restrict__ col, int N,
                                                            const float *__restrict__ a_src,
                                                            const float *__restrict__ a_dst,
                                                            const float *__restrict__ alpha,
                                                            const float *__restrict__ G, float ns,
                                                            float *__restrict__ c, float *__restrict__ da_dst_g) {
  const int i = blockIdx.x * 4 + wave_in_block();
  if (i >= N) return;
  const int lane = lane_id();
  const int beg = rowptr[i], end = rowptr[i + 1];
  float ad[H], s1[H], s2[H], s3[H];   // sum alpha G, sum alpha s G, sum alpha s
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    ad[hh] = a_dst[(size_t)i * H + hh];
    s1[hh] = s2[hh] = s3[hh] = 0.f;
  }
  for (int e = beg + lane; e < end; e += 64) {
    const float *as = a_src + (size_t)col[e] * H;
    const float *al = alpha + (size_t)e * H;
    const float *g = G + (size_t)e * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      const float a = al[hh], gv = g[hh];
      const float A = a * (as[hh] + ad[hh] > 0.f ? 1.f : ns);
      s1[hh] = fmaf(a, gv, s1[hh]);
      s2[hh] = fmaf(A, gv, s2[hh]);
      s3[hh] += A;
    }
  }
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    s1[hh] = wave_sum(s1[hh]);
    s2[hh] = wave_sum(s2[hh]);
    s3[hh] = wave_sum(s3[hh]);
  }
  if (lane == 0) {
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      c[(size_t)i * H + hh] = s1[hh];
      da_dst_g[(size_t)i * H + hh] = fmaf(-s1[hh], s3[hh], s2[hh]);
    }
  }
}

// row r: da_src^G[r], then the three in-place updates (dh row r, da_src[r], row_stats[r, 3H..4H))
template <int H>
__global__ __launch_bounds__(256) void alpha_bwd_src_kernel(
    const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ tmap, int N, int C,
    const float *__restrict__ a_src, const float *__restrict__ a_dst, const float *__restrict__ alpha,
    const float *__restrict__ G, const float *__restrict__ c, const float *__restrict__ da_dst_g,
    const float *__restrict__ att_s, const float *__restrict__ att_d, float ns, float *__restrict__ dh,
    float *__restrict__ da_src, float *__restrict__ row_stats) {
  const int r = blockIdx.x * 4 + wave_in_block();
  if (r >= N) return;
  const int lane = lane_id();
  const int beg = rowptr[r], end = rowptr[r + 1];
  float asr[H], ds[H], dd[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    asr[hh] = a_src[(size_t)r * H + hh];
    ds[hh] = 0.f;
  }
  for (int e = beg + lane; e < end; e += 64) {
    const int i = col[e], t = tmap[e];
    if (t < 0) continue;   // no transposed edge (an asymmetric CSR): nothing flows back along it
    const float *ad = a_dst + (size_t)i * H;
    const float *ci = c + (size_t)i * H;
    const float *al = alpha + (size_t)t * H;
    const float *g = G + (size_t)t * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      const float A = al[hh] * (asr[hh] + ad[hh] > 0.f ? 1.f : ns);
      ds[hh] = fmaf(A, g[hh] - ci[hh], ds[hh]);
    }
  }
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    ds[hh] = wave_sum(ds[hh]);
    dd[hh] = da_dst_g[(size_t)r * H + hh];
  }
  // dh row r: float4 q covers columns 4q .. 4q + 3, all of head (4q) / C (C % 4 == 0)
  float4 *o4 = reinterpret_cast<float4 *>(dh) + (size_t)r * (H * C / 4);
  const float4 *s4 = reinterpret_cast<const float4 *>(att_s);
  const float4 *t4 = reinterpret_cast<const float4 *>(att_d);
  for (int q = lane; q < H * C / 4; q += 64) {
    const int head = (4 * q) / C;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      a = head == hh ? ds[hh] : a;
      b = head == hh ? dd[hh] : b;
    }
    o4[q] = f4_fma(b, t4[q], f4_fma(a, s4[q], o4[q]));
  }
  if (lane == 0) {
    float *rs = row_stats + (size_t)r * 4 * H + 3 * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      da_src[(size_t)r * H + hh] += ds[hh];
      rs[hh] += dd[hh];
    }
  }
}

}  // namespace

}  // namespace hicgat

using namespace hicgat;

#define HICGAT_ATTN_BY_H(LAUNCH) \
  switch (H) {                   \
    case 1: LAUNCH(1); break;    \
    case 2: LAUNCH(2); break;    \
    case 3: LAUNCH(3); break;    \
    default: LAUNCH(4); break;   \
  }

extern "C" int hicgat_gat_transpose_map(const int32_t *rowptr, const int32_t *col, int N, int32_t *tmap,
                                        hicgat_stream_t stream) {
  if (N < 0) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!rowptr || !col || !tmap) return HICGAT_EINVAL;
  hipLaunchKernelGGL(transpose_map_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, rowptr, col, N,
                     tmap);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_gat_alpha(const int32_t *rowptr, const int32_t *col, int N, int H, int C, const float *a_src,
                                const float *a_dst, const float *row_stats, float neg_slope, float *alpha,
                                hicgat_stream_t stream) {
  if (N < 0) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (N == 0) return HICGAT_OK;
  if (!rowptr || !col || !a_src || !a_dst || !row_stats || !alpha) return HICGAT_EINVAL;
  const dim3 grid((N + 3) / 4), block(256);
#define HICGAT_ALPHA(H_)                                                                                       \
  hipLaunchKernelGGL(alpha_kernel<H_>, grid, block, 0, (hipStream_t)stream, rowptr, col, N, a_src, a_dst, row_stats, \
                     neg_slope, alpha)
  HICGAT_ATTN_BY_H(HICGAT_ALPHA)
#undef HICGAT_ALPHA
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_gat_alpha_bwd_dst(const int32_t *rowptr, const int32_t *col, int N, int H, int C,
                                        const float *a_src, const float *a_dst, const float *alpha, const float *G,
                                        float neg_slope, float *c, float *da_dst_g, hicgat_stream_t stream) {
  if (N < 0) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (N == 0) return HICGAT_OK;
  if (!rowptr || !col || !a_src || !a_dst || !alpha || !G || !c || !da_dst_g) return HICGAT_EINVAL;
  const dim3 grid((N + 3) / 4), block(256);
#define HICGAT_ALPHA_DST(H_)                                                                                     \
  hipLaunchKernelGGL(alpha_bwd_dst_kernel<H_>, grid, block, 0, (hipStream_t)stream, rowptr, col, N, a_src, a_dst, \
                     alpha, G, neg_slope, c, da_dst_g)
  HICGAT_ATTN_BY_H(HICGAT_ALPHA_DST)
#undef HICGAT_ALPHA_DST
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_gat_alpha_bwd_src(const int32_t *rowptr, const int32_t *col, const int32_t *tmap, int N, int H,
                                        int C, const float *a_src, const float *a_dst, const float *alpha,
                                        const float *G, const float *c, const float *da_dst_g, const float *att_src,
                                        const float *att_dst, float neg_slope, float *dh, float *da_src,
                                        float *row_stats, hicgat_stream_t stream) {
  if (N < 0) return HICGAT_EINVAL;
  if (!gat_shape_supported(H, C)) return HICGAT_EUNSUPPORTED;
  if (N == 0) return HICGAT_OK;
  if (!rowptr || !col || !tmap || !a_src || !a_dst || !alpha || !G || !c || !da_dst_g || !att_src || !att_dst ||
      !dh || !da_src || !row_stats)
    return HICGAT_EINVAL;
  const dim3 grid((N + 3) / 4), block(256);
#define HICGAT_ALPHA_SRC(H_)                                                                                       \
  hipLaunchKernelGGL(alpha_bwd_src_kernel<H_>, grid, block, 0, (hipStream_t)stream, rowptr, col, tmap, N, C, a_src, \
                     a_dst, alpha, G, c, da_dst_g, att_src, att_dst, neg_slope, dh, da_src, row_stats)
  HICGAT_ATTN_BY_H(HICGAT_ALPHA_SRC)
#undef HICGAT_ALPHA_SRC
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}
