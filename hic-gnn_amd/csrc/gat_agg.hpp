// The GATConv aggregation passes, one __device__ body per pass for every supported (H, C):
//   agg_fwd_row       forward: softmax statistics, then the gather
//   agg_bwd_rows_row  destination side of the backward without a gather
//   agg_bwd_dst_row   destination side, stand-alone gathering form
//   agg_bwd_src_row   source side
//   attn_mask_row     the attention-dropout keep bits of a row's edges (tests, tools)
// The __global__ kernels around them only pick the row: per pass one (2, 256) entry kernel with its
// measured launch parameters and one for every other shape, the forward's in gat_fwd.hip, the
// backward's in gat_bwd.hip, launched through gat_launch.hpp's shape list.
// Supported set:  C % 128 == 0,  D = H*C a multiple of 256,  D <= 1024,  H <= 4.
//
// Design: one wave per destination row, four rows per 256-thread workgroup, no [nnz, H, C] tensor,
// no float atomics, fixed summation order; neighbour index and alphas broadcast with readlane from
// the lane that owns the edge; each gather one scalar base + per-lane dwordx4.
//
// Layout: h [N, D] fp32 row-major, a_src/a_dst [N, H], CSR int32 (rowptr [N+1], col [nnz]) with the
// self loops already inserted, row_stats [N, 4H] = (max[H], sum[H], delta[H], da_dst[H]) per row.
// Every per-row array is indexed by the global row id.
//
// Lane / head mapping.  A lane holds V = D/256 float4 slices of a row; slice v is float4
// #(64v + lane), columns 256v + 4*lane ...  A half wave's 128 columns of a slice lie inside one head
// (C % 128 == 0): lanes 0-31 of slice v belong to head (256v)/C, lanes 32-63 to head (256v + 128)/C.
// Where the two are the same head (every slice when C % 256 == 0, (2, 256) among them) the alpha of
// a neighbour is one scalar broadcast and pick / bcast_pick / scatter_add fold to a plain index;
// where they differ (every slice when C == 128, the middle slice of C == 384) the lane selects
// between two broadcast alphas by lane >> 5, and the per-head dot products of the backward are sums
// over a half wave (formed here as whole-wave sums of values that the other half contributes 0 to).
#pragma once
#include "common.hpp"
#include "philox.hpp"

namespace hicgat {

namespace {

template <int H, int C> struct Shape {
  static_assert(C % 128 == 0 && (H * C) % 256 == 0 && H * C <= 1024 && H >= 1 && H <= 4, "unsupported GAT shape");
  static constexpr int D = H * C, V = D / 256, Q = D / 4;
  static constexpr int HP = H <= 1 ? 1 : H <= 2 ? 2 : 4;        // heads padded to a power of two
  static constexpr int TR = 2 * HP;                             // transpose_reduce width for 2H values
  __host__ __device__ static constexpr int lo(int v) { return (256 * v) / C; }
  __host__ __device__ static constexpr int hi(int v) { return (256 * v + 128) / C; }
  // neighbours gathered per inner step: V float4 loads per lane each.  The forward keeps 16 (V <= 2)
  // or 12-16 (V >= 3) loads in flight, the source pass 4-8: at D = 1024 the TRAIN forward carries 32
  // accumulator floats, and U = 8 there (128 gathered floats) does not fit 128 VGPRs.
  static constexpr int UFwd = V <= 2 ? 8 : 4;
  static constexpr int USrc = V <= 2 ? 4 : 2;
  // agg_bwd_dst at (2, 256), N = 20000 on MI355X (tools/kbench.py): U = 8 -> 0.95 ms (118 VGPRs, 4
  // waves per SIMD); U = 4 -> 0.52; U = 2 -> 0.47.  With per-edge reductions in the loop the gather
  // wants waves, not ILP.
  static constexpr int UDst = 2;
};

// this lane's value among per-head values a[] for its slice v (upper: lane >> 5)
template <int H, int C> __device__ __forceinline__ float pick(const float (&a)[H], int v, bool upper) {
  using S = Shape<H, C>;
  return S::lo(v) == S::hi(v) ? a[S::lo(v)] : (upper ? a[S::hi(v)] : a[S::lo(v)]);
}
// the same of lane l's a[] (broadcast through SGPRs; one readlane where the slice lies in one head)
template <int H, int C> __device__ __forceinline__ float bcast_pick(const float (&a)[H], int l, int v, bool upper) {
  using S = Shape<H, C>;
  const float x = readlane_f(a[S::lo(v)], l);
  if (S::lo(v) == S::hi(v)) return x;
  const float y = readlane_f(a[S::hi(v)], l);
  return upper ? y : x;
}
// add x (a partial sum over this lane's slice v) to its head's entry of a[]
template <int H, int C, int NA> __device__ __forceinline__ void scatter_add(float (&a)[NA], int stride, int off,
                                                                         int v, bool upper, float x) {
  using S = Shape<H, C>;
  if (S::lo(v) == S::hi(v)) {
    a[S::lo(v) * stride + off] += x;
  } else {
    a[S::lo(v) * stride + off] += upper ? 0.f : x;
    a[S::hi(v) * stride + off] += upper ? x : 0.f;
  }
}

__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}

// ---- forward, row i (a4+a5 of the reference: PyG 1.7.2 GATConv.forward / propagate / message +
// torch_geometric.utils.softmax (ptr path) + torch_scatter segment_csr(sum), models.py:634-662).
// Pass 1/2 stream only col[] and a_src[] (row max, row sum); pass 3 gathers h[j] rows, UFwd
// neighbours in flight.
//
// TRAIN also accumulates, from the same gathered rows (FMAs only, no extra loads),
//   out2[i] = sum_j alpha_ij lrelu'(e_ij) h_j    and    S3[i] = sum_j alpha_ij lrelu'(e_ij)
// (S3 into the delta slot of row_stats).  With those the destination half of the backward needs no
// gather (agg_bwd_rows_row).  ACT = 1 applies the relu that follows the GATConv in
// GATNetSelectiveResidualsUpdated (models.py:637) in the epilogue: out = relu(acc + bias).
//
// SPLIT (the tiled form, gat_tiles.hip): the softmax statistics still come from the whole row
// (rowptr/col), but only the edges of the sparse remainder (rowptr_s/col_s) are gathered, and the
// raw sums (no bias, no activation) go to out/out2 with S3 of those edges; the matrix-core pass over
// the row's dense 32x32 tiles adds the rest and applies the epilogue.
//
// DROP (attention dropout, PyG's F.dropout(alpha, p) in message()): each alpha_ij is multiplied by
// m_ij in {0, 1/(1-p)} (philox.hpp attn_factor: one Philox call per edge, where the lane that owns the
// edge forms its weights -- once per 64-edge chunk, never inside the gather loop).  out and out2 take
// the masked weights, S3 the unmasked one; the softmax statistics are those of the undropped row.
// No SPLIT form.  With DROP = false `mk` is unused and the body is what it was without it.
template <int H, int C, bool TRAIN, int ACT, bool SPLIT, bool DROP = false>
__device__ __forceinline__ void agg_fwd_row(
    int i, const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ rowptr_s,
    const int *__restrict__ col_s, const float *__restrict__ h, const float *__restrict__ a_src,
    const float *__restrict__ a_dst, const float *__restrict__ bias, float ns, float *__restrict__ out,
    float *__restrict__ out2, float *__restrict__ row_stats, const AttnMaskArgs &mk = AttnMaskArgs{}) {
  static_assert(!(DROP && SPLIT), "the tiled form has no attention dropout");
  using S = Shape<H, C>;
  constexpr int U = S::UFwd, V = S::V, Q = S::Q;
  const int lane = lane_id();
  const bool upper = lane >= 32;
  const int beg = rowptr[i], end = rowptr[i + 1];
  float ad[H], m[H], s[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    ad[hh] = a_dst[(size_t)i * H + hh];
    m[hh] = -INFINITY;
    s[hh] = 0.f;
  }
  for (int e = beg + lane; e < end; e += 64) {
    const float *as = a_src + (size_t)col[e] * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) m[hh] = fmaxf(m[hh], lrelu(as[hh] + ad[hh], ns));
  }
#pragma unroll
  for (int hh = 0; hh < H; ++hh) m[hh] = wave_max(m[hh]);
  for (int e = beg + lane; e < end; e += 64) {
    const float *as = a_src + (size_t)col[e] * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) s[hh] += expf(lrelu(as[hh] + ad[hh], ns) - m[hh]);
  }
  float den[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    s[hh] = wave_sum(s[hh]);
    den[hh] = s[hh] + 1e-16f;
  }

  const float4 *h4 = reinterpret_cast<const float4 *>(h);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc[V], acs[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = acs[v] = z4;
  float t[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) t[hh] = 0.f;
  const int gbeg = SPLIT ? rowptr_s[i] : beg, gend = SPLIT ? rowptr_s[i + 1] : end;
  const int *__restrict__ gcol = SPLIT ? col_s : col;
  const uint32_t step = DROP ? mask_step(mk) : 0u;
  for (int base = gbeg; base < gend; base += 64) {
    const int e = base + lane;
    int j = i;  // padded slots gather the (valid) own row with weight 0
    float p[H], q[H];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) p[hh] = q[hh] = 0.f;
    if (e < gend) {
      j = gcol[e];
      const float *as = a_src + (size_t)j * H;
#pragma unroll
      for (int hh = 0; hh < H; ++hh) {
        const float ee = as[hh] + ad[hh];
        p[hh] = expf(lrelu(ee, ns) - m[hh]) / den[hh];
        if (TRAIN) {
          q[hh] = p[hh] * (ee > 0.f ? 1.f : ns);
          t[hh] += q[hh];
        }
      }
      if (DROP) {
        float f[H];
        attn_factor<H>(mk, step, i, j, f);
#pragma unroll
        for (int hh = 0; hh < H; ++hh) {
          p[hh] *= f[hh];
          q[hh] *= f[hh];
        }
      }
    }
    const int cnt = min(64, gend - base);
    for (int k = 0; k < cnt; k += U) {
      float4 g[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t jj = (size_t)readlane_i(j, k + u);
#pragma unroll
        for (int v = 0; v < V; ++v) g[u][v] = h4[jj * Q + 64 * v + lane];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          acc[v] = f4_fma(bcast_pick<H, C>(p, k + u, v, upper), g[u][v], acc[v]);
          if (TRAIN) acs[v] = f4_fma(bcast_pick<H, C>(q, k + u, v, upper), g[u][v], acs[v]);
        }
      }
    }
  }
  const float4 *b4 = reinterpret_cast<const float4 *>(bias);
  float4 *o4 = reinterpret_cast<float4 *>(out) + (size_t)i * Q + lane;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float4 r = f4_add(acc[v], SPLIT ? z4 : b4[64 * v + lane]);
    if (ACT == 1 && !SPLIT) r = f4_relu(r);
    o4[64 * v] = r;
  }
  float *rs = row_stats + (size_t)i * 4 * H;
  if (TRAIN) {
    float4 *q4 = reinterpret_cast<float4 *>(out2) + (size_t)i * Q + lane;
#pragma unroll
    for (int v = 0; v < V; ++v) q4[64 * v] = acs[v];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) t[hh] = wave_sum(t[hh]);
    if (lane == 0) {
#pragma unroll
      for (int hh = 0; hh < H; ++hh) {
        rs[2 * H + hh] = t[hh];   // S3, parked in the delta slot until the rows pass replaces it
        rs[3 * H + hh] = 0.f;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      rs[hh] = m[hh];
      rs[H + hh] = s[hh];
    }
  }
}

// ---- destination side without a gather, row i (the forward's TRAIN outputs):
//   dout_i = g_i * [y_i > 0] (ACT = 1: the relu after the GATConv, torch's threshold_backward on
//   its output) or g_i (ACT = 0);  delta_i = <dout_i, y_i - bias> (y = out where the mask is on);
//   da_dst_i = <dout_i, out2_i> - delta_i * S3_i.   One wave per row, 4 rows of D floats streamed.
template <int H, int C, int ACT>
__device__ __forceinline__ void agg_bwd_rows_row(int i, const float *__restrict__ g, const float *__restrict__ y,
                                                 const float *__restrict__ bias, const float *__restrict__ out2,
                                                 float *__restrict__ dout, int64_t ldq,
                                                 float *__restrict__ row_stats) {
  using S = Shape<H, C>;
  constexpr int V = S::V, Q = S::Q, TR = S::TR, HP = S::HP;
  const int lane = lane_id();
  const bool upper = lane >= 32;
  const float4 *g4 = reinterpret_cast<const float4 *>(g) + (size_t)i * Q + lane;
  const float4 *y4 = reinterpret_cast<const float4 *>(y) + (size_t)i * Q + lane;
  const float4 *q4 = reinterpret_cast<const float4 *>(out2) + (size_t)i * Q + lane;
  const float4 *b4 = reinterpret_cast<const float4 *>(bias) + lane;
  float val[TR];   // [hh]: <dout, y - bias> of head hh, [HP + hh]: <dout, out2>
#pragma unroll
  for (int k = 0; k < TR; ++k) val[k] = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float4 d = g4[64 * v];
    const float4 yv = y4[64 * v], qv = q4[64 * v], bv = b4[64 * v];
    if (ACT == 1) {
      d = make_float4(yv.x <= 0.f ? 0.f : d.x, yv.y <= 0.f ? 0.f : d.y, yv.z <= 0.f ? 0.f : d.z,
                      yv.w <= 0.f ? 0.f : d.w);
      reinterpret_cast<float4 *>(dout)[(size_t)i * ldq + 64 * v + lane] = d;   // ldq: row stride, float4
    }
    scatter_add<H, C>(val, 1, 0, v, upper, f4_dot(d, f4_sub(yv, bv)));
    scatter_add<H, C>(val, 1, HP, v, upper, f4_dot(d, qv));
  }
  transpose_reduce<TR>(val, lane);   // value k (summed over the wave) in lane k * 64 / TR
  float dl[H], pq[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    dl[hh] = readlane_f(val[0], hh * (64 / TR));
    pq[hh] = readlane_f(val[0], (HP + hh) * (64 / TR));
  }
  if (lane == 0) {
    float *rs = row_stats + (size_t)i * 4 * H;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      const float s3 = rs[2 * H + hh];   // from the forward
      rs[2 * H + hh] = dl[hh];
      rs[3 * H + hh] = fmaf(-dl[hh], s3, pq[hh]);
    }
  }
}

// ---- destination side, stand-alone gathering form, row i (needs only h): gathers h_j and forms
// every g_ij = <dout_i, h_j>; the per-edge dot products are reduced HP * UDst neighbour-heads at a
// time with one transpose reduce.
template <int H, int C>
__device__ __forceinline__ void agg_bwd_dst_row(int i, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                const float *__restrict__ h, const float *__restrict__ a_src,
                                                const float *__restrict__ a_dst, const float *__restrict__ dout,
                                                float ns, float *__restrict__ row_stats) {
  using S = Shape<H, C>;
  constexpr int U = S::UDst, V = S::V, Q = S::Q, HP = S::HP, NV = HP * U, G = 64 / NV;
  const int lane = lane_id();
  const bool upper = lane >= 32;
  const int beg = rowptr[i], end = rowptr[i + 1];
  const float4 *h4 = reinterpret_cast<const float4 *>(h);
  const float4 *g4 = reinterpret_cast<const float4 *>(dout) + (size_t)i * Q + lane;
  float4 d[V];
#pragma unroll
  for (int v = 0; v < V; ++v) d[v] = g4[64 * v];
  // after transpose_reduce<NV> over values [head * U + slot], the G lanes [idx * G, (idx + 1) * G) hold
  // the sum of value idx; the first of them is its owner
  const int idx = lane / G, myh = idx / U, kk = idx % U;
  const bool owner = (lane % G) == 0 && myh < H;
  float *rs = row_stats + (size_t)i * 4 * H;
  float ad[H], mx[H], den[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    ad[hh] = a_dst[(size_t)i * H + hh];
    mx[hh] = rs[hh];
    den[hh] = rs[H + hh] + 1e-16f;
  }
  float S1 = 0.f, S2 = 0.f, S3 = 0.f;
  for (int base = beg; base < end; base += 64) {
    const int e = base + lane;
    int j = i;
    // per-edge softmax weight and leaky-relu slope of this chunk, one edge per lane (the only
    // scattered loads of the row), later broadcast to the lane that owns each reduced dot product
    float al[H], alp[H];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) al[hh] = alp[hh] = 0.f;
    if (e < end) {
      j = col[e];
      const float *as = a_src + (size_t)j * H;
#pragma unroll
      for (int hh = 0; hh < H; ++hh) {
        const float ee = as[hh] + ad[hh];
        al[hh] = expf(lrelu(ee, ns) - mx[hh]) / den[hh];
        alp[hh] = al[hh] * (ee > 0.f ? 1.f : ns);
      }
    }
    const int cnt = min(64, end - base);
    for (int k = 0; k < cnt; k += U) {
      float4 gth[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t jj = (size_t)readlane_i(j, k + u);
#pragma unroll
        for (int v = 0; v < V; ++v) gth[u][v] = h4[jj * Q + 64 * v + lane];
      }
      float val[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) val[q] = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) scatter_add<H, C>(val, U, u, v, upper, f4_dot(d[v], gth[u][v]));
      transpose_reduce<NV>(val, lane);
      const int src = k + kk;
      float a = 0.f, ap = 0.f;
#pragma unroll
      for (int hh = 0; hh < H; ++hh) {
        const float x = __shfl(al[hh], src), xp = __shfl(alp[hh], src);
        a = myh == hh ? x : a;
        ap = myh == hh ? xp : ap;
      }
      if (owner && src < cnt) {
        S1 = fmaf(a, val[0], S1);
        S2 = fmaf(ap, val[0], S2);
        S3 += ap;
      }
    }
  }
  // the owners of head hh are among lanes [hh * 64 / HP, (hh + 1) * 64 / HP): sum within that group
#pragma unroll
  for (int o = 32 / HP; o > 0; o >>= 1) {
    S1 += __shfl_xor(S1, o);
    S2 += __shfl_xor(S2, o);
    S3 += __shfl_xor(S3, o);
  }
  const float dd = S2 - S1 * S3;
  float dl[H], da[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    dl[hh] = readlane_f(S1, hh * (64 / HP));
    da[hh] = readlane_f(dd, hh * (64 / HP));
  }
  if (lane == 0) {
#pragma unroll
    for (int hh = 0; hh < H; ++hh) {
      rs[2 * H + hh] = dl[hh];
      rs[3 * H + hh] = da[hh];
    }
  }
}

// ---- source side, row r: gathers dout_i of the rows that have r as a neighbour.  The graph is
// structurally symmetric, so row r's own CSR list *is* that set.  Algebraically regrouped so that no
// per-edge dot product (and no cross-lane reduction) sits inside the gather loop:
//   da_src[r] = sum_i alpha_ir s_ir (<dout_i, h_r> - delta_i)
//             = <sum_i alpha_ir s_ir dout_i, h_r> - sum_i alpha_ir s_ir delta_i      (s = lrelu')
// so the loop only accumulates two vectors (sum alpha dout_i, sum alpha s dout_i) and a scalar.
// ldq: dout row stride in float4, ldr: row_stats row stride in floats (both multiples of 4, so a
// multi-GPU caller can all-gather [dout | row stats] rows as one packed buffer).
// SPLIT (the tiled form, gat_tiles.hip): rowptr/col are the sparse remainder of the row's edges;
// dh gets the raw sum (no logit terms) and da_src the remainder's share of da_src; the matrix-core
// pass over the dense tiles adds the rest and finishes both.
// DROP: the two accumulated vectors take the masked weights alpha_ir m_ir, the scalar sum the unmasked
// one (delta_i already carries the mask); m_ir is the forward's bit of edge (i -> r), recomputed from
// (col[e], r).  No SPLIT form.
template <int H, int C, bool SPLIT, bool DROP = false>
__device__ __forceinline__ void agg_bwd_src_row(
    int r, const int *__restrict__ rowptr, const int *__restrict__ col, const float *__restrict__ h,
    const float *__restrict__ a_src, const float *__restrict__ a_dst, const float *__restrict__ row_stats,
    int64_t ldr, const float *__restrict__ dout, int64_t ldq, const float *__restrict__ att_s,
    const float *__restrict__ att_d, float ns, float *__restrict__ dh, float *__restrict__ da_src,
    const AttnMaskArgs &mk = AttnMaskArgs{}) {
  static_assert(!(DROP && SPLIT), "the tiled form has no attention dropout");
  using S = Shape<H, C>;
  constexpr int U = S::USrc, V = S::V, Q = S::Q, TR = S::TR, HP = S::HP;
  const int lane = lane_id();
  const bool upper = lane >= 32;
  const int beg = rowptr[r], end = rowptr[r + 1];
  const float4 *h4 = reinterpret_cast<const float4 *>(h);
  const float4 *g4 = reinterpret_cast<const float4 *>(dout);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float asr[H], sb[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh) {
    asr[hh] = a_src[(size_t)r * H + hh];
    sb[hh] = 0.f;
  }
  float4 acc[V], c[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = c[v] = z4;
  const uint32_t step = DROP ? mask_step(mk) : 0u;
  for (int base = beg; base < end; base += 64) {
    const int e = base + lane;
    int inb = r;
    float al[H], A[H];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) al[hh] = A[hh] = 0.f;
    if (e < end) {
      inb = col[e];
      const float *ad = a_dst + (size_t)inb * H;
      const float *rs = row_stats + ldr * inb;   // max[H] sum[H] delta[H] da_dst[H]
#pragma unroll
      for (int hh = 0; hh < H; ++hh) {
        const float ee = asr[hh] + ad[hh];
        al[hh] = expf(lrelu(ee, ns) - rs[hh]) / (rs[H + hh] + 1e-16f);
        A[hh] = al[hh] * (ee > 0.f ? 1.f : ns);
        sb[hh] = fmaf(A[hh], rs[2 * H + hh], sb[hh]);
      }
      if (DROP) {
        float f[H];
        attn_factor<H>(mk, step, inb, r, f);
#pragma unroll
        for (int hh = 0; hh < H; ++hh) {
          al[hh] *= f[hh];
          A[hh] *= f[hh];
        }
      }
    }
    const int cnt = min(64, end - base);
    for (int k = 0; k < cnt; k += U) {
      float4 gth[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t ii = (size_t)readlane_i(inb, k + u);
#pragma unroll
        for (int v = 0; v < V; ++v) gth[u][v] = g4[ii * ldq + 64 * v + lane];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          acc[v] = f4_fma(bcast_pick<H, C>(al, k + u, v, upper), gth[u][v], acc[v]);
          c[v] = f4_fma(bcast_pick<H, C>(A, k + u, v, upper), gth[u][v], c[v]);
        }
      }
    }
  }
  float val[TR];   // [hh]: <sum alpha s dout_i, h_r> of head hh, [HP + hh]: sum alpha s delta_i
#pragma unroll
  for (int k = 0; k < TR; ++k) val[k] = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v)
    scatter_add<H, C>(val, 1, 0, v, upper, f4_dot(c[v], h4[(size_t)r * Q + 64 * v + lane]));
#pragma unroll
  for (int hh = 0; hh < H; ++hh) val[HP + hh] = sb[hh];
  transpose_reduce<TR>(val, lane);
  float ds[H];
#pragma unroll
  for (int hh = 0; hh < H; ++hh)
    ds[hh] = readlane_f(val[0], hh * (64 / TR)) - readlane_f(val[0], (HP + hh) * (64 / TR));
  float4 *o4 = reinterpret_cast<float4 *>(dh) + (size_t)r * Q + lane;
  if (SPLIT) {
#pragma unroll
    for (int v = 0; v < V; ++v) o4[64 * v] = acc[v];
  } else {
    float dd[H];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) dd[hh] = row_stats[ldr * r + 3 * H + hh];
    const float4 *s4 = reinterpret_cast<const float4 *>(att_s);
    const float4 *t4 = reinterpret_cast<const float4 *>(att_d);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float4 a = f4_fma(pick<H, C>(ds, v, upper), s4[64 * v + lane], acc[v]);
      a = f4_fma(pick<H, C>(dd, v, upper), t4[64 * v + lane], a);
      o4[64 * v] = a;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int hh = 0; hh < H; ++hh) da_src[(size_t)r * H + hh] = ds[hh];
  }
}

// ---- the keep bits of row i's edges, [nnz, H] uint8 in self-looped CSR order, from the device
// function the DROP passes use (philox.hpp attn_keep).
template <int H>
__device__ __forceinline__ void attn_mask_row(int i, const int *__restrict__ rowptr, const int *__restrict__ col,
                                              const AttnMaskArgs &mk, uint8_t *__restrict__ mask) {
  const uint32_t step = mask_step(mk);
  const int beg = rowptr[i], end = rowptr[i + 1];
  for (int e = beg + lane_id(); e < end; e += 64) {
    bool keep[H];
    attn_keep<H>(mk, step, i, col[e], keep);
#pragma unroll
    for (int hh = 0; hh < H; ++hh) mask[(size_t)e * H + hh] = keep[hh] ? 1 : 0;
  }
}

}  // namespace

}  // namespace hicgat
