// General LayerNorm row pass of the zoo's LayerNorm tails, and the elementwise activation beside it.
//
// Reference: models.py:321-377 (`x = self.norm2(self.dense2(x)); x = x.relu()`, LayerNorm(32)),
// :437-526 (LayerNorm(512) on the GATConv output, relu, + align1(x)), :693-773 (`x = F.gelu(norm_a(
// densea(x))); x = x + x_initial; x = self.norm_residual_a(x)`), :776-832 (F.leaky_relu after the
// norm): up to five torch ops per block, here one wave pass over the row:
//   forward : u = act(LN(y; gamma, beta, eps)) + res                  (res optional)
//             z = LN(u; gamma2, beta2, eps2)                          (only with gamma2; else z = u)
//             LN: torch.nn.LayerNorm -- biased variance about the mean (second sweep over the
//             registers), rstd = 1 / sqrt(var + eps); saves (mean, rstd) and (mean2, rstd2) per row;
//   backward: recomputes yhat, pre = yhat * gamma + beta and (second norm) u, uhat;
//             dgamma2 += dz * uhat; dbeta2 += dz;  du = rstd2 (dz gamma2 - mean(.) - uhat mean(. uhat))
//             (no second norm: du = dz);  dres = du;  g = du * act'(pre);  dgamma += g * yhat;
//             dbeta += g;  dy = rstd (g gamma - mean(.) - yhat mean(. yhat)).
// act: none, relu, leaky_relu(slope), gelu = 0.5 x (1 + erf(x / sqrt 2)) (F.gelu's default, erff);
// gelu' = Phi(x) + x phi(x).
// Lane layout, W >= 64: one wave per row, column q * 64 + lane.  With relu and no second norm this is the
// flagship's row pass (models.py:641-655), whose bits tests/golden/ln_row_pass_bits.json pins.
// W = 32: two rows per wave -- lanes 0..31 hold row 2k, lanes 32..63 row 2k + 1, sums over the half
// wave -- so every wave load is a full 256 B and half as many waves run; the half wave whose row is
// past M loads and stores nothing (it feeds zeros to its own half's sums only).
// Parameter gradients: per-wave register partials over a grid-stride row loop, [waves, 2W] = [dgamma
// | dbeta] or [waves, 4W] = [dgamma | dbeta | dgamma2 | dbeta2], then the fixed-order column sums of
// reduce.hip (deterministic, no atomics).
#include "reduce.hpp"

namespace hicgat {

constexpr int kLnActWaves = 4096;   // waves of the backward grid (partials: kLnActWaves x 2 or 4 x W; 4 blocks per CU)

template <int W>
struct RowLanes {
  static constexpr int V = W >= 64 ? W / 64 : 1;   // values per lane
  static constexpr int R = W >= 64 ? 1 : 2;        // rows per wave
  static __device__ __forceinline__ int col(int q, int lane) { return W >= 64 ? q * 64 + lane : (lane & 31); }
  static __device__ __forceinline__ int sub(int lane) { return W >= 64 ? 0 : lane >> 5; }
  static __device__ __forceinline__ float sum(float v) { return W >= 64 ? wave_sum(v) : half_wave_sum(v); }
};

constexpr float kInvSqrt2 = 0.70710678118654752440f, kInvSqrt2Pi = 0.39894228040143267794f;

template <int ACT>
__device__ __forceinline__ float act_value(float x, float slope) {
  if (ACT == HICGAT_ACT_RELU) return fmaxf(x, 0.f);
  if (ACT == HICGAT_ACT_LEAKY_RELU) return lrelu(x, slope);
  if (ACT == HICGAT_ACT_GELU) return 0.5f * x * (1.f + erff(x * kInvSqrt2));
  return x;
}
// g * act'(x)
template <int ACT>
__device__ __forceinline__ float act_grad(float g, float x, float slope) {
  if (ACT == HICGAT_ACT_RELU) return x > 0.f ? g : 0.f;
  if (ACT == HICGAT_ACT_LEAKY_RELU) return x > 0.f ? g : g * slope;
  if (ACT == HICGAT_ACT_GELU) {
    const float cdf = 0.5f * (1.f + erff(x * kInvSqrt2));
    const float pdf = expf(-0.5f * x * x) * kInvSqrt2Pi;
    return g * fmaf(x, pdf, cdf);
  }
  return g;
}

template <int W, int ACT, bool N2>
__global__ __launch_bounds__(256) void ln_act_res_fwd_kernel(
    const float *__restrict__ y, int64_t ldy, int M, const float *__restrict__ gamma, const float *__restrict__ beta,
    float eps, float slope, const float *__restrict__ res, int64_t ldr, const float *__restrict__ gamma2,
    const float *__restrict__ beta2, float eps2, float *__restrict__ z, int64_t ldz, float2 *__restrict__ stats,
    float2 *__restrict__ stats2) {
  using L = RowLanes<W>;
  constexpr int V = L::V;
  const int lane = lane_id();
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave_in_block()) * L::R;
  if (row0 >= M) return;
  const int64_t row = row0 + L::sub(lane);
  const bool live = L::R == 1 || row < M;   // W = 32: the second row of the last wave may be past M
  float v[V];
#pragma unroll
  for (int q = 0; q < V; ++q) v[q] = live ? y[(size_t)row * ldy + L::col(q, lane)] : 0.f;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < V; ++q) s += v[q];
  const float mean = L::sum(s) / (float)W;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const float d = v[q] - mean;
    ss = fmaf(d, d, ss);
  }
  const float rstd = 1.0f / sqrt_rn_f32(L::sum(ss) / (float)W + eps);
  float u[V];
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const int c = L::col(q, lane);
    float o = act_value<ACT>(fmaf((v[q] - mean) * rstd, gamma[c], beta[c]), slope);
    if (res && live) o += res[(size_t)row * ldr + c];
    u[q] = o;
    if (!N2 && live) z[(size_t)row * ldz + c] = o;
  }
  const bool first = L::col(0, lane) == 0;
  if (first && live) stats[row] = make_float2(mean, rstd);
  if (N2) {
    float s2 = 0.f;
#pragma unroll
    for (int q = 0; q < V; ++q) s2 += u[q];
    const float mean2 = L::sum(s2) / (float)W;
    float ss2 = 0.f;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const float d = u[q] - mean2;
      ss2 = fmaf(d, d, ss2);
    }
    const float rstd2 = 1.0f / sqrt_rn_f32(L::sum(ss2) / (float)W + eps2);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const int c = L::col(q, lane);
      if (live) z[(size_t)row * ldz + c] = fmaf((u[q] - mean2) * rstd2, gamma2[c], beta2[c]);
    }
    if (first && live) stats2[row] = make_float2(mean2, rstd2);
  }
}

template <int W, int ACT, bool N2>
__global__ __launch_bounds__(256) void ln_act_res_bwd_kernel(
    const float *__restrict__ dz, int64_t lddz, const float *__restrict__ y, int64_t ldy, int M,
    const float2 *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta, float slope,
    const float *__restrict__ res, int64_t ldr, const float *__restrict__ gamma2, const float2 *__restrict__ stats2,
    float *__restrict__ dy, int64_t lddy, float *__restrict__ dres, int64_t lddres, float *__restrict__ part) {
  using L = RowLanes<W>;
  constexpr int V = L::V;
  constexpr int NP = N2 ? 4 : 2;   // partial rows of W per wave
  const int lane = lane_id();
  const int gw = blockIdx.x * 4 + wave_in_block();
  const int nw = gridDim.x * 4;
  float g_[V], b_[V], g2_[V], pg[V], pb[V], pg2[V], pb2[V];
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const int c = L::col(q, lane);
    g_[q] = gamma[c];
    b_[q] = beta[c];
    g2_[q] = N2 ? gamma2[c] : 0.f;
    pg[q] = pb[q] = pg2[q] = pb2[q] = 0.f;
  }
  for (int64_t row0 = (int64_t)gw * L::R; row0 < M; row0 += (int64_t)nw * L::R) {
    const int64_t row = row0 + L::sub(lane);
    const bool live = L::R == 1 || row < M;
    const float2 st = live ? stats[row] : make_float2(0.f, 0.f);
    float yh[V], dh[V], pre[V], du[V];
    if (N2) {
      const float2 st2 = live ? stats2[row] : make_float2(0.f, 0.f);
      float uh[V];
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const int c = L::col(q, lane);
        yh[q] = ((live ? y[(size_t)row * ldy + c] : 0.f) - st.x) * st.y;
        pre[q] = fmaf(yh[q], g_[q], b_[q]);
        float u = act_value<ACT>(pre[q], slope);
        if (res && live) u += res[(size_t)row * ldr + c];
        uh[q] = (u - st2.x) * st2.y;
        const float dzv = live ? dz[(size_t)row * lddz + c] : 0.f;
        pg2[q] = fmaf(dzv, uh[q], pg2[q]);
        pb2[q] += dzv;
        du[q] = dzv * g2_[q];
        t1 += du[q];
        t2 = fmaf(du[q], uh[q], t2);
      }
      const float n1 = L::sum(t1) / (float)W, n2 = L::sum(t2) / (float)W;
#pragma unroll
      for (int q = 0; q < V; ++q) du[q] = st2.y * (du[q] - n1 - uh[q] * n2);
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const int c = L::col(q, lane);
      if (!N2) {
        yh[q] = ((live ? y[(size_t)row * ldy + c] : 0.f) - st.x) * st.y;
        pre[q] = fmaf(yh[q], g_[q], b_[q]);
        du[q] = live ? dz[(size_t)row * lddz + c] : 0.f;
      }
      if (dres && live) dres[(size_t)row * lddres + c] = du[q];   // d(residual) = du, written beside dy
      const float g = act_grad<ACT>(du[q], pre[q], slope);
      pg[q] = fmaf(g, yh[q], pg[q]);
      pb[q] += g;
      dh[q] = g * g_[q];
      s1 += dh[q];
      s2 = fmaf(dh[q], yh[q], s2);
    }
    const float m1 = L::sum(s1) / (float)W, m2 = L::sum(s2) / (float)W;
#pragma unroll
    for (int q = 0; q < V; ++q)
      if (live) dy[(size_t)row * lddy + L::col(q, lane)] = st.y * (dh[q] - m1 - yh[q] * m2);
  }
  if (L::R == 2) {   // the wave's two rows' partials into one
#pragma unroll
    for (int q = 0; q < V; ++q) {
      pg[q] += __shfl_xor(pg[q], 32);
      pb[q] += __shfl_xor(pb[q], 32);
      if (N2) {
        pg2[q] += __shfl_xor(pg2[q], 32);
        pb2[q] += __shfl_xor(pb2[q], 32);
      }
    }
    if (lane >= 32) return;
  }
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const int c = L::col(q, lane);
    part[((size_t)gw * NP + 0) * W + c] = pg[q];
    part[((size_t)gw * NP + 1) * W + c] = pb[q];
    if (N2) {
      part[((size_t)gw * NP + 2) * W + c] = pg2[q];
      part[((size_t)gw * NP + 3) * W + c] = pb2[q];
    }
  }
}

// y = act(x) (BWD: dx = dy * act'(x) from the saved input x), four elements per thread.
template <int ACT, bool BWD>
__global__ __launch_bounds__(256) void act_kernel(const float4 *__restrict__ x, const float4 *__restrict__ dy,
                                                  float4 *__restrict__ out, int64_t n4, float slope) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 a = x[i];
    float4 o;
    if (BWD) {
      const float4 g = dy[i];
      o = make_float4(act_grad<ACT>(g.x, a.x, slope), act_grad<ACT>(g.y, a.y, slope), act_grad<ACT>(g.z, a.z, slope),
                      act_grad<ACT>(g.w, a.w, slope));
    } else {
      o = make_float4(act_value<ACT>(a.x, slope), act_value<ACT>(a.y, slope), act_value<ACT>(a.z, slope),
                      act_value<ACT>(a.w, slope));
    }
    out[i] = o;
  }
}

static bool ln_width_ok(int W) { return W == 32 || W == 64 || W == 128 || W == 256 || W == 512; }
static bool ln_act_ok(int act) { return act >= HICGAT_ACT_NONE && act <= HICGAT_ACT_GELU; }
static bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

struct LnFwdArgs {
  const float *y; int64_t ldy; int M; const float *gamma, *beta; float eps, slope; const float *res; int64_t ldr;
  const float *gamma2, *beta2; float eps2; float *z; int64_t ldz; float2 *stats, *stats2;
};
struct LnBwdArgs {
  const float *dz; int64_t lddz; const float *y; int64_t ldy; int M; const float2 *stats; const float *gamma, *beta;
  float slope; const float *res; int64_t ldr; const float *gamma2; const float2 *stats2; float *dy; int64_t lddy;
  float *dres; int64_t lddres; float *part;
};

template <int W, int ACT, bool N2>
static void ln_fwd_launch(const LnFwdArgs &a, hipStream_t s) {
  const int64_t waves = ((int64_t)a.M + RowLanes<W>::R - 1) / RowLanes<W>::R;
  hipLaunchKernelGGL((ln_act_res_fwd_kernel<W, ACT, N2>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a.y,
                     a.ldy, a.M, a.gamma, a.beta, a.eps, a.slope, a.res, a.ldr, a.gamma2, a.beta2, a.eps2, a.z, a.ldz,
                     a.stats, a.stats2);
}
template <int W, int ACT, bool N2>
static void ln_bwd_launch(const LnBwdArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((ln_act_res_bwd_kernel<W, ACT, N2>), dim3(kLnActWaves / 4), dim3(256), 0, s, a.dz, a.lddz, a.y,
                     a.ldy, a.M, a.stats, a.gamma, a.beta, a.slope, a.res, a.ldr, a.gamma2, a.stats2, a.dy, a.lddy,
                     a.dres, a.lddres, a.part);
}

#define LN_ACT_BY_N2(FN, W, ACT, n2, a, s) \
  do {                                     \
    if (n2) FN<W, ACT, true>(a, s);        \
    else FN<W, ACT, false>(a, s);          \
  } while (0)
#define LN_ACT_BY_ACT(FN, W, act, n2, a, s)                                                     \
  do {                                                                                          \
    if (act == HICGAT_ACT_RELU) LN_ACT_BY_N2(FN, W, HICGAT_ACT_RELU, n2, a, s);                 \
    else if (act == HICGAT_ACT_LEAKY_RELU) LN_ACT_BY_N2(FN, W, HICGAT_ACT_LEAKY_RELU, n2, a, s); \
    else if (act == HICGAT_ACT_GELU) LN_ACT_BY_N2(FN, W, HICGAT_ACT_GELU, n2, a, s);            \
    else LN_ACT_BY_N2(FN, W, HICGAT_ACT_NONE, n2, a, s);                                        \
  } while (0)
#define LN_ACT_DISPATCH(FN, W, act, n2, a, s)                  \
  do {                                                         \
    if (W == 32) LN_ACT_BY_ACT(FN, 32, act, n2, a, s);         \
    else if (W == 64) LN_ACT_BY_ACT(FN, 64, act, n2, a, s);    \
    else if (W == 128) LN_ACT_BY_ACT(FN, 128, act, n2, a, s);  \
    else if (W == 256) LN_ACT_BY_ACT(FN, 256, act, n2, a, s);  \
    else LN_ACT_BY_ACT(FN, 512, act, n2, a, s);                \
  } while (0)

}  // namespace hicgat

using namespace hicgat;

extern "C" size_t hicgat_ln_act_res_workspace_bytes(int W, int second_norm) {
  if (!ln_width_ok(W)) return 0;
  return (size_t)kLnActWaves * (second_norm ? 4 : 2) * W * sizeof(float) + colsum_workspace_bytes(kLnActWaves, 2 * W);
}

extern "C" int hicgat_ln_act_res_fwd(const float *y, int64_t ldy, int M, int W, const float *gamma, const float *beta,
                                     float eps, int act, float slope, const float *res, int64_t ldr,
                                     const float *gamma2, const float *beta2, float eps2, float *z, int64_t ldz,
                                     float *row_stats, float *row_stats2, hicgat_stream_t stream) {
  if (M < 0) return HICGAT_EINVAL;
  if (!ln_width_ok(W) || !ln_act_ok(act)) return HICGAT_EUNSUPPORTED;
  const bool n2 = gamma2 != nullptr;
  if (!(eps > 0.f) || (gamma2 == nullptr) != (beta2 == nullptr) || (n2 && !(eps2 > 0.f))) return HICGAT_EINVAL;
  if (act == HICGAT_ACT_LEAKY_RELU && !(slope > 0.f)) return HICGAT_EINVAL;
  if (ldy < W || ldz < W || (res && ldr < W)) return HICGAT_EINVAL;
  if (M == 0) return HICGAT_OK;
  if (!y || !gamma || !beta || !z || !row_stats || (n2 && !row_stats2)) return HICGAT_EINVAL;
  const LnFwdArgs a{y, ldy, M, gamma, beta, eps, slope, res, ldr, gamma2, beta2, eps2, z, ldz,
                    reinterpret_cast<float2 *>(row_stats), reinterpret_cast<float2 *>(row_stats2)};
  hipStream_t s = (hipStream_t)stream;
  LN_ACT_DISPATCH(ln_fwd_launch, W, act, n2, a, s);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_ln_act_res_bwd_params(int W, float *dgamma, float *dbeta, float *dgamma2, float *dbeta2,
                                            int accumulate, void *workspace, size_t workspace_bytes,
                                            hicgat_stream_t stream) {
  if (!ln_width_ok(W)) return HICGAT_EUNSUPPORTED;
  if (!dgamma || !dbeta || !workspace || (dgamma2 == nullptr) != (dbeta2 == nullptr)) return HICGAT_EINVAL;
  const bool n2 = dgamma2 != nullptr;
  if (workspace_bytes < hicgat_ln_act_res_workspace_bytes(W, n2)) return HICGAT_EINVAL;
  float *part = static_cast<float *>(workspace);
  const int64_t ld = (int64_t)(n2 ? 4 : 2) * W;
  float *ws = part + (size_t)kLnActWaves * ld;
  const ColOut o{dgamma, 0, W, dbeta, nullptr, accumulate};
  int rc = colsum_launch(part, ld, kLnActWaves, 2 * W, o, ws, (hipStream_t)stream);
  if (rc != HICGAT_OK || !n2) return rc;
  const ColOut o2{dgamma2, 0, W, dbeta2, nullptr, accumulate};   // the same scratch, after the first sum in stream order
  return colsum_launch(part + 2 * W, ld, kLnActWaves, 2 * W, o2, ws, (hipStream_t)stream);
}

extern "C" int hicgat_ln_act_res_bwd(const float *dz, int64_t lddz, const float *y, int64_t ldy, int M, int W,
                                     const float *row_stats, const float *gamma, const float *beta, int act,
                                     float slope, const float *res, int64_t ldr, const float *gamma2,
                                     const float *row_stats2, float *dy, int64_t lddy, float *dres, int64_t lddres,
                                     float *dgamma, float *dbeta, float *dgamma2, float *dbeta2, int accumulate,
                                     void *workspace, size_t workspace_bytes, hicgat_stream_t stream) {
  if (M < 0) return HICGAT_EINVAL;
  if (!ln_width_ok(W) || !ln_act_ok(act)) return HICGAT_EUNSUPPORTED;
  const bool n2 = gamma2 != nullptr;
  if (act == HICGAT_ACT_LEAKY_RELU && !(slope > 0.f)) return HICGAT_EINVAL;
  if (!gamma || !beta || !workspace || (n2 && !row_stats2)) return HICGAT_EINVAL;
  if ((dgamma == nullptr) != (dbeta == nullptr) || (dgamma2 == nullptr) != (dbeta2 == nullptr)) return HICGAT_EINVAL;
  if (dgamma && (dgamma2 != nullptr) != n2) return HICGAT_EINVAL;   // both norms' gradients, or none here
  if (!dgamma && dgamma2) return HICGAT_EINVAL;
  if (lddz < W || ldy < W || lddy < W || (res && ldr < W) || (dres && lddres < W)) return HICGAT_EINVAL;
  if (M > 0 && (!dz || !y || !row_stats || !dy)) return HICGAT_EINVAL;
  if (workspace_bytes < hicgat_ln_act_res_workspace_bytes(W, n2)) return HICGAT_EINVAL;
  const LnBwdArgs a{dz, lddz, y, ldy, M, reinterpret_cast<const float2 *>(row_stats), gamma, beta, slope, res, ldr,
                    gamma2, reinterpret_cast<const float2 *>(row_stats2), dy, lddy, dres, lddres,
                    static_cast<float *>(workspace)};
  hipStream_t s = (hipStream_t)stream;
  LN_ACT_DISPATCH(ln_bwd_launch, W, act, n2, a, s);   // M = 0 too: the partials must be zeros
  HICGAT_CHECK_LAUNCH();
  if (!dgamma) return HICGAT_OK;   // partials stay in the workspace for hicgat_ln_act_res_bwd_params
  return hicgat_ln_act_res_bwd_params(W, dgamma, dbeta, dgamma2, dbeta2, accumulate, workspace, workspace_bytes,
                                      stream);
}

static int act_launch(bool bwd, const float *x, const float *dy, float *out, int M, int W, int act, float slope,
                      hicgat_stream_t stream) {
  if (M < 0 || W <= 0) return HICGAT_EINVAL;
  if (act != HICGAT_ACT_LEAKY_RELU && act != HICGAT_ACT_GELU) return HICGAT_EUNSUPPORTED;
  if (W % 4) return HICGAT_EUNSUPPORTED;
  if (act == HICGAT_ACT_LEAKY_RELU && !(slope > 0.f)) return HICGAT_EINVAL;
  if (M == 0) return HICGAT_OK;
  if (!x || !out || (bwd && !dy) || misaligned16(x) || misaligned16(out) || misaligned16(dy)) return HICGAT_EINVAL;
  const int64_t n4 = (int64_t)M * W / 4;
  const dim3 grid((unsigned)std::min<int64_t>((n4 + 255) / 256, 16384));
  hipStream_t s = (hipStream_t)stream;
  const float4 *x4 = reinterpret_cast<const float4 *>(x), *d4 = reinterpret_cast<const float4 *>(dy);
  float4 *o4 = reinterpret_cast<float4 *>(out);
  if (act == HICGAT_ACT_GELU) {
    if (bwd) hipLaunchKernelGGL((act_kernel<HICGAT_ACT_GELU, true>), grid, dim3(256), 0, s, x4, d4, o4, n4, slope);
    else hipLaunchKernelGGL((act_kernel<HICGAT_ACT_GELU, false>), grid, dim3(256), 0, s, x4, d4, o4, n4, slope);
  } else {
    if (bwd) hipLaunchKernelGGL((act_kernel<HICGAT_ACT_LEAKY_RELU, true>), grid, dim3(256), 0, s, x4, d4, o4, n4, slope);
    else hipLaunchKernelGGL((act_kernel<HICGAT_ACT_LEAKY_RELU, false>), grid, dim3(256), 0, s, x4, d4, o4, n4, slope);
  }
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_act_fwd(const float *x, int M, int W, int act, float slope, float *y, hicgat_stream_t stream) {
  return act_launch(false, x, nullptr, y, M, W, act, slope, stream);
}

extern "C" int hicgat_act_bwd(const float *dy, const float *x, int M, int W, int act, float slope, float *dx,
                              hicgat_stream_t stream) {
  return act_launch(true, x, dy, dx, M, W, act, slope, stream);
}
