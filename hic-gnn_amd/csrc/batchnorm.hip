// torch.nn.BatchNorm1d over the node axis, fused with the activation and the Dropout that follow it
// in the zoo's MLP tails (models.py:288-298, :852-862):  z = dropout(act(gamma * yhat + beta)),
// yhat = (y - mean) * rstd per column of the [M, W] output y of the preceding Linear.
//
// Training forward, three launches and two passes over y:
//   stats    : grid (W / 64, ceil(M / 64)); a 256-thread block reduces 64 rows x 64 columns the way
//              colsum_tall_kernel does (4 row groups x 16 rows, all 16 loads of a thread issued before
//              the adds, groups combined in order through LDS) to the chunk's fp32 mean m_c (a pivot),
//              then, from the values still in registers and in fp64 (y - m_c is exact there), to
//              r_c = sum(y - m_c) and q_c = sum((y - m_c)^2).  E[y^2] - E[y]^2 is never formed.
//   finalize : per column the chunks are merged in index order, in fp64, with Chan's formula
//              (n = na + nb, d = mb - ma, mean = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n) after
//              each chunk's mean m_c + r_c / n_c and M2 q_c - r_c^2 / n_c are recovered; 16
//              contiguous groups of chunks per column, the groups merged in order through LDS.  It
//              writes (mean, mean_lo, rstd, rstd_lo) -- each pair is an fp64 value split in two floats
//              -- and the training forward's side effects: running_mean, running_var (unbiased),
//              num_batches_tracked.
//   apply    : one thread per 4 columns x a strided set of rows, its column constants in registers,
//              yhat = ((y - mean) - mean_lo) * rstd in fp32 (nothing is lost when |mean| >> std);
//              the keep mask is dropout.hip's (philox.hpp).  In eval mode it is the only launch:
//              mean = running_mean, rstd = 1 / sqrt(running_var + eps) per thread.
// Backward, two passes over (dz, z, y): g = dz * dropout' * act' from the saved OUTPUT z's sign
// (hicgat_act_dropout_bwd's convention);
//   reduce   : the stats geometry; per chunk (sum g yhat, sum g) -> partial rows;
//   sums     : the partial rows summed per column in index order (16 contiguous groups, combined in
//              order through LDS) -> (dgamma, dbeta);
//   dy       : the apply geometry; dy = gamma rstd (g - dbeta / M - yhat dgamma / M) (eval: g gamma
//              rstd); the blocks of the first row slab also write dgamma / dbeta to the caller.
// With batch statistics the three terms of dy cancel -- almost wholly on a two-row batch, where they
// leave eps / (d^2 + eps) of their size -- so yhat, rstd, the partial sums and that combination are
// fp64 in the backward (reduce.hip's fp32 column sums are not used for that reason); dy is rounded
// to fp32 once.  No float atomics; every sum runs in one fixed order.
#include "philox.hpp"

using namespace hicgat;

namespace {

constexpr int kRows = 16;            // rows per thread of a stats / reduce chunk
constexpr int kChunk = 4 * kRows;    // rows per chunk
constexpr int kGroups = 16;          // chunk groups per column in the finalize / sums
constexpr int kMaxBlocks = 2048;     // apply / dy: 8 blocks per CU, the rest of a tall tensor is strided

int chunks_of(int M) { return (M + kChunk - 1) / kChunk; }

// In-order sum over the 4 row groups of a chunk (each thread gives its group's value of column cl).
template <typename T>
__device__ __forceinline__ T chunk_sum(T (*red)[64], int g, int cl, T v) {
  __syncthreads();   // the previous use of red is over
  red[g][cl] = v;
  __syncthreads();
  return ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// part [chunks][3][W] doubles: (m_c, r_c, q_c)
__global__ __launch_bounds__(256) void bn_stats_kernel(const float *__restrict__ y, int64_t ldy, int M, int W,
                                                       double *__restrict__ part) {
  __shared__ float red[4][64];
  __shared__ double redd[4][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl;
  const int k0 = blockIdx.y * kChunk + g * kRows;
  const int nc = min(kChunk, M - (int)blockIdx.y * kChunk);   // rows of this chunk (>= 1)
  float v[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) v[r] = k0 + r < M ? y[(size_t)(k0 + r) * ldy + n] : 0.f;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < kRows; ++r) s += v[r];
  const float mean = chunk_sum(red, g, cl, s) / (float)nc;
  double rs = 0.0, qs = 0.0;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const double d = k0 + r < M ? (double)v[r] - (double)mean : 0.0;
    rs += d;
    qs = fma(d, d, qs);
  }
  const double rsum = chunk_sum(redd, g, cl, rs);
  const double qsum = chunk_sum(redd, g, cl, qs);
  if (g == 0) {
    double *p = part + (size_t)blockIdx.y * 3 * W + n;
    p[0] = (double)mean;
    p[W] = rsum;
    p[2 * W] = qsum;
  }
}

struct Moments {
  double n, mean, m2;
};

// Chan's pairwise update: a <- a merged with b (either may be empty).
__device__ __forceinline__ void chan_merge(Moments &a, const Moments &b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) {
    a = b;
    return;
  }
  const double n = a.n + b.n, d = b.mean - a.mean;
  a.mean += d * (b.n / n);
  a.m2 += b.m2 + d * d * (a.n * b.n / n);
  a.n = n;
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const double *__restrict__ part, int M, int W, int chunks,
                                                          double eps, double momentum, float *__restrict__ stats,
                                                          float *running_mean, float *running_var,
                                                          int64_t *num_batches_tracked) {
  __shared__ Moments sh[kGroups][16];
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + cl;
  const int per = (chunks + kGroups - 1) / kGroups;
  const int kb = g * per, ke = min(chunks, kb + per);
  Moments a{0.0, 0.0, 0.0};
  for (int k = kb; k < ke; ++k) {
    const double *p = part + (size_t)k * 3 * W + n;
    const double nc = (double)min(kChunk, M - k * kChunk);
    const double r = p[W];
    chan_merge(a, Moments{nc, p[0] + r / nc, fmax(p[2 * W] - r * r / nc, 0.0)});
  }
  sh[g][cl] = a;
  __syncthreads();
  if (g == 0) {
#pragma unroll 1
    for (int h = 1; h < kGroups; ++h) chan_merge(a, sh[h][cl]);
    const double var = a.m2 / a.n;   // biased
    const double rstd = 1.0 / sqrt_rn_f64(var + eps);
    const float mean = (float)a.mean, rstd_f = (float)rstd;
    stats[n] = mean;
    stats[W + n] = (float)(a.mean - (double)mean);
    stats[2 * W + n] = rstd_f;
    stats[3 * W + n] = (float)(rstd - (double)rstd_f);
    if (running_mean) running_mean[n] = (float)((1.0 - momentum) * (double)running_mean[n] + momentum * a.mean);
    if (running_var)
      running_var[n] = (float)((1.0 - momentum) * (double)running_var[n] + momentum * (var * (a.n / (a.n - 1.0))));
  }
  if (num_batches_tracked && blockIdx.x == 0) {   // lane 0 of the first wave writes (a per-lane vector store)
    const int64_t v = *num_batches_tracked + 1;
    if (threadIdx.x == 0) *num_batches_tracked = v;
  }
}

// The constants of one column: stats [4, W] (training) or the running buffers (eval: rstd =
// 1 / sqrt(running_var + eps), correctly rounded square root as in ln_act.hip).
struct Col {
  float mean, lo, rstd, rstd_lo;
};

__device__ __forceinline__ Col load_col(const float *stats, const float *rmean, const float *rvar, float eps, int W,
                                        int c) {
  if (stats) return Col{stats[c], stats[W + c], stats[2 * W + c], stats[3 * W + c]};
  return Col{rmean[c], 0.f, 1.0f / sqrt_rn_f32(rvar[c] + eps), 0.f};
}

__device__ __forceinline__ double yhat64(float y, const Col &c) {
  return ((double)y - ((double)c.mean + (double)c.lo)) * ((double)c.rstd + (double)c.rstd_lo);
}

__device__ __forceinline__ float f4_get(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ uint32_t u4_get(const uint4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// block: 16 column quads (64 columns, blockIdx.x) x 16 rows; the row slabs stride by gridDim.y * 16.
template <int ACT, bool DROP>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ y, int64_t ldy, int M, int W,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ stats,
                                                       const float *__restrict__ rmean, const float *__restrict__ rvar,
                                                       float eps, float slope, float scale, MaskArgs m,
                                                       float *__restrict__ z, int64_t ldz) {
  const int quad = blockIdx.x * 16 + (threadIdx.x & 15);
  const int c0 = 4 * quad;
  Col c[4];
  float ga[4], be[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = load_col(stats, rmean, rvar, eps, W, c0 + j);
    ga[j] = gamma[c0 + j];
    be[j] = beta[c0 + j];
  }
  const uint32_t step = DROP ? mask_step(m) : 0u;
  for (int64_t row = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4); row < M; row += (int64_t)gridDim.y * 16) {
    const float4 v = *reinterpret_cast<const float4 *>(y + row * ldy + c0);
    uint4 r = make_uint4(0, 0, 0, 0);
    if (DROP) r = quad_words(m, step, m.row_offset + row, W / 4, quad);
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float yh = ((f4_get(v, j) - c[j].mean) - c[j].lo) * c[j].rstd;
      const float a = act_apply<ACT>(fmaf(yh, ga[j], be[j]), slope);
      o[j] = DROP ? (u4_get(r, j) >= m.T ? a * scale : 0.f) : a;
    }
    *reinterpret_cast<float4 *>(z + row * ldz + c0) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// The gradient that reaches the BatchNorm's output, from dz and the saved output z.
template <int ACT>
__device__ __forceinline__ float bn_out_grad(float dz, float z, float slope, float scale) {
  if (ACT == HICGAT_ACT_NONE) return dz;
  return act_dropout_grad<ACT>(dz, z, slope, scale);
}

// part [chunks][2][W] doubles: (sum g yhat, sum g)
template <int ACT>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float *__restrict__ dz, int64_t lddz,
                                                            const float *__restrict__ z, int64_t ldz,
                                                            const float *__restrict__ y, int64_t ldy, int M, int W,
                                                            const float *__restrict__ stats,
                                                            const float *__restrict__ rmean,
                                                            const float *__restrict__ rvar, float eps, float slope,
                                                            float scale, double *__restrict__ part) {
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl;
  const int k0 = blockIdx.y * kChunk + g * kRows;
  const Col col = load_col(stats, rmean, rvar, eps, W, n);
  float a[kRows], b[kRows], c[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const bool in = k0 + r < M;
    a[r] = in ? dz[(size_t)(k0 + r) * lddz + n] : 0.f;
    b[r] = (in && ACT != HICGAT_ACT_NONE) ? z[(size_t)(k0 + r) * ldz + n] : 0.f;
    c[r] = in ? y[(size_t)(k0 + r) * ldy + n] : 0.f;
  }
  double sg = 0.0, sb = 0.0;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const double gr = (double)bn_out_grad<ACT>(a[r], b[r], slope, scale);   // 0 for a row past M (dz = 0)
    sg = fma(gr, yhat64(c[r], col), sg);
    sb += gr;
  }
  const double tg = chunk_sum(red, g, cl, sg);
  const double tb = chunk_sum(red, g, cl, sb);
  if (g == 0) {
    double *p = part + (size_t)blockIdx.y * 2 * W + n;
    p[0] = tg;
    p[W] = tb;
  }
}

// sums64 / sums32 [2 W] = the column sums of part [chunks][2 W], in index order.
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const double *__restrict__ part, int W2, int chunks,
                                                          double *__restrict__ sums64, float *__restrict__ sums32) {
  __shared__ double sh[kGroups][16];
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + cl;
  const int per = (chunks + kGroups - 1) / kGroups;
  const int kb = g * per, ke = min(chunks, kb + per);
  double s = 0.0;
  for (int k = kb; k < ke; ++k) s += part[(size_t)k * W2 + n];
  sh[g][cl] = s;
  __syncthreads();
  if (g == 0) {
#pragma unroll 1
    for (int h = 1; h < kGroups; ++h) s += sh[h][cl];
    sums64[n] = s;
    sums32[n] = (float)s;
  }
}

// sums64 = [dgamma | dbeta] (2 W doubles).  TRAIN: batch statistics (the two mean terms, fp64); else
// fixed ones.
template <int ACT, bool TRAIN>
__global__ __launch_bounds__(256) void bn_bwd_dy_kernel(const float *__restrict__ dz, int64_t lddz,
                                                        const float *__restrict__ z, int64_t ldz,
                                                        const float *__restrict__ y, int64_t ldy, int M, int W,
                                                        const float *__restrict__ gamma,
                                                        const float *__restrict__ stats,
                                                        const float *__restrict__ rmean,
                                                        const float *__restrict__ rvar, float eps, float slope,
                                                        float scale, const double *__restrict__ sums64,
                                                        float *__restrict__ dy, int64_t lddy, float *dgamma,
                                                        float *dbeta, int accumulate) {
  const int quad = blockIdx.x * 16 + (threadIdx.x & 15);
  const int c0 = 4 * quad;
  Col c[4];
  float gr32[4];               // eval: gamma * rstd
  double gr64[4], k1[4], k2[4];   // training: gamma * rstd, dbeta / M, dgamma / M
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = load_col(stats, rmean, rvar, eps, W, c0 + j);
    gr32[j] = gamma[c0 + j] * c[j].rstd;
    gr64[j] = (double)gamma[c0 + j] * ((double)c[j].rstd + (double)c[j].rstd_lo);
    k1[j] = TRAIN ? sums64[W + c0 + j] / (double)M : 0.0;
    k2[j] = TRAIN ? sums64[c0 + j] / (double)M : 0.0;
  }
  if (dgamma && blockIdx.y == 0 && threadIdx.x < 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dgamma[c0 + j] = (float)sums64[c0 + j] + (accumulate ? dgamma[c0 + j] : 0.f);
      dbeta[c0 + j] = (float)sums64[W + c0 + j] + (accumulate ? dbeta[c0 + j] : 0.f);
    }
  }
  for (int64_t row = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4); row < M; row += (int64_t)gridDim.y * 16) {
    const float4 d = *reinterpret_cast<const float4 *>(dz + row * lddz + c0);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ACT != HICGAT_ACT_NONE) o = *reinterpret_cast<const float4 *>(z + row * ldz + c0);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (TRAIN) v = *reinterpret_cast<const float4 *>(y + row * ldy + c0);
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float g = bn_out_grad<ACT>(f4_get(d, j), f4_get(o, j), slope, scale);
      if (TRAIN)
        out[j] = (float)(gr64[j] * (((double)g - k1[j]) - yhat64(f4_get(v, j), c[j]) * k2[j]));
      else
        out[j] = g * gr32[j];
    }
    *reinterpret_cast<float4 *>(dy + row * lddy + c0) = make_float4(out[0], out[1], out[2], out[3]);
  }
}

bool width_ok(int W) { return W >= 64 && W <= 1024 && W % 64 == 0; }
bool rows_ok(const float *p, int64_t ld, int W) { return p && ld >= W && ld % 4 == 0 && !misaligned(p, 16); }

dim3 apply_grid(int M, int W) {
  const int slabs = (M + 15) / 16, cap = kMaxBlocks / (W / 64);
  return dim3(W / 64, slabs < cap ? slabs : cap);
}

// workspace layouts, in bytes.  forward: part [chunks][3][W] doubles.  backward: sums32 [2 W] floats,
// sums64 [2 W] doubles, part [chunks][2][W] doubles.
size_t fwd_bytes(int M, int W) { return (size_t)chunks_of(M) * 3 * W * sizeof(double); }
size_t bwd_bytes(int M, int W) {
  return (size_t)2 * W * sizeof(float) + ((size_t)2 * W + (size_t)chunks_of(M) * 2 * W) * sizeof(double);
}

}  // namespace

extern "C" size_t hicgat_bn_workspace_bytes(int M, int W) {
  if (M < 1 || !width_ok(W)) return 0;
  const size_t f = fwd_bytes(M, W), b = bwd_bytes(M, W);
  return f > b ? f : b;
}

extern "C" int hicgat_bn_stats(const float *y, int64_t ldy, int M, int W, double eps, double momentum, float *stats,
                               float *running_mean, float *running_var, int64_t *num_batches_tracked,
                               void *workspace, size_t workspace_bytes, hicgat_stream_t stream) {
  if (W <= 0 || !stats || !workspace || !(eps > 0.0) || !(momentum > 0.0 && momentum <= 1.0) || M < 2)
    return HICGAT_EINVAL;
  if (!width_ok(W)) return HICGAT_EUNSUPPORTED;
  if (!rows_ok(y, ldy, W) || misaligned(num_batches_tracked, 8) || misaligned(workspace, 16) ||
      workspace_bytes < fwd_bytes(M, W))
    return HICGAT_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  double *part = static_cast<double *>(workspace);
  const int chunks = chunks_of(M);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(W / 64, chunks), dim3(256), 0, s, y, ldy, M, W, part);
  HICGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(W / 16), dim3(256), 0, s, part, M, W, chunks, eps, momentum, stats,
                     running_mean, running_var, num_batches_tracked);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

#define BN_BY_ACT(LAUNCH)                                   \
  do {                                                      \
    if (act == HICGAT_ACT_RELU) LAUNCH(HICGAT_ACT_RELU);    \
    else if (act == HICGAT_ACT_LEAKY_RELU) LAUNCH(HICGAT_ACT_LEAKY_RELU); \
    else LAUNCH(HICGAT_ACT_NONE);                           \
  } while (0)

extern "C" int hicgat_bn_act_dropout_fwd(const float *y, int64_t ldy, int M, int W, const float *gamma,
                                         const float *beta, const float *stats, const float *running_mean,
                                         const float *running_var, double eps, int act, float slope, double p,
                                         uint64_t seed, const int64_t *step_counter, int64_t step_value,
                                         uint32_t site, int64_t row_offset, float *z, int64_t ldz,
                                         hicgat_stream_t stream) {
  if (M < 1 || W <= 0 || !gamma || !beta || !(eps > 0.0) || !p_ok(p) || row_offset < 0 || act < HICGAT_ACT_NONE ||
      act > HICGAT_ACT_LEAKY_RELU || (!stats && (!running_mean || !running_var)))
    return HICGAT_EINVAL;
  if (!width_ok(W)) return HICGAT_EUNSUPPORTED;
  if (!rows_ok(y, ldy, W) || !rows_ok(z, ldz, W) || misaligned(step_counter, 8)) return HICGAT_EINVAL;
  const MaskArgs m{seed, step_counter, step_value, row_offset, site, keep_threshold(p)};
  const float scale = keep_scale(p), e = (float)eps;
  const dim3 grid = apply_grid(M, W);
  hipStream_t s = (hipStream_t)stream;
#define BN_FWD(A)                                                                                                  \
  do {                                                                                                             \
    if (p > 0.0)                                                                                                   \
      hipLaunchKernelGGL((bn_apply_kernel<A, true>), grid, dim3(256), 0, s, y, ldy, M, W, gamma, beta, stats,      \
                         running_mean, running_var, e, slope, scale, m, z, ldz);                                   \
    else                                                                                                           \
      hipLaunchKernelGGL((bn_apply_kernel<A, false>), grid, dim3(256), 0, s, y, ldy, M, W, gamma, beta, stats,     \
                         running_mean, running_var, e, slope, scale, m, z, ldz);                                   \
  } while (0)
  BN_BY_ACT(BN_FWD);
#undef BN_FWD
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_bn_act_dropout_bwd(const float *dz, int64_t lddz, const float *z, int64_t ldz, const float *y,
                                         int64_t ldy, int M, int W, const float *gamma, const float *stats,
                                         const float *running_mean, const float *running_var, double eps, int act,
                                         float slope, double p, float *dy, int64_t lddy, float *dgamma, float *dbeta,
                                         int accumulate, void *workspace, size_t workspace_bytes,
                                         hicgat_stream_t stream) {
  if (M < 1 || W <= 0 || !gamma || !workspace || !(eps > 0.0) || !p_ok(p) || act < HICGAT_ACT_NONE ||
      act > HICGAT_ACT_LEAKY_RELU || (!stats && (!running_mean || !running_var)) ||
      (dgamma == nullptr) != (dbeta == nullptr) || (stats && M < 2))
    return HICGAT_EINVAL;
  if (!width_ok(W)) return HICGAT_EUNSUPPORTED;
  if (act == HICGAT_ACT_NONE && p > 0.0) return HICGAT_EUNSUPPORTED;   // a zero output is ambiguous there
  if (act == HICGAT_ACT_LEAKY_RELU && !(slope > 0.f)) return HICGAT_EINVAL;
  if (!rows_ok(dz, lddz, W) || !rows_ok(y, ldy, W) || !rows_ok(dy, lddy, W) ||
      (act != HICGAT_ACT_NONE && !rows_ok(z, ldz, W)) || misaligned(workspace, 16) ||
      workspace_bytes < bwd_bytes(M, W))
    return HICGAT_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int chunks = chunks_of(M);
  float *sums32 = static_cast<float *>(workspace);
  double *sums64 = reinterpret_cast<double *>(sums32 + 2 * W), *part = sums64 + 2 * W;
  const float scale = keep_scale(p), e = (float)eps;
#define BN_RED(A)                                                                                                  \
  hipLaunchKernelGGL(bn_bwd_reduce_kernel<A>, dim3(W / 64, chunks), dim3(256), 0, s, dz, lddz, z, ldz, y, ldy, M,  \
                     W, stats, running_mean, running_var, e, slope, scale, part)
  BN_BY_ACT(BN_RED);
#undef BN_RED
  HICGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(2 * W / 16), dim3(256), 0, s, part, 2 * W, chunks, sums64, sums32);
  HICGAT_CHECK_LAUNCH();
  const dim3 grid = apply_grid(M, W);
#define BN_DY(A)                                                                                                   \
  do {                                                                                                             \
    if (stats)                                                                                                     \
      hipLaunchKernelGGL((bn_bwd_dy_kernel<A, true>), grid, dim3(256), 0, s, dz, lddz, z, ldz, y, ldy, M, W,       \
                         gamma, stats, running_mean, running_var, e, slope, scale, sums64, dy, lddy, dgamma,       \
                         dbeta, accumulate);                                                                       \
    else                                                                                                           \
      hipLaunchKernelGGL((bn_bwd_dy_kernel<A, false>), grid, dim3(256), 0, s, dz, lddz, z, ldz, y, ldy, M, W,      \
                         gamma, stats, running_mean, running_var, e, slope, scale, sums64, dy, lddy, dgamma,       \
                         dbeta, accumulate);                                                                       \
  } while (0)
  BN_BY_ACT(BN_DY);
#undef BN_DY
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}
