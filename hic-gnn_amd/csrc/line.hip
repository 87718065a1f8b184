// LINE second-order embeddings on gfx950: the feature generator of HiC-GNN_main.py:91-96,
// `LINE(G, embedding_size=512, order='second')` + `line.train(batch_size, epochs)` (the `ge` package
// over Keras; not installed, restated from its published source -- include/hicgat.h "LINE").
//
// One training step (one batch of the sample stream) is two launches:
//   line_grad_kernel    one wave per sample k: draw (h, t, y) from the counter-based stream, gather
//                       U[h] and C[t] (D/64 values per lane, float4 loads when D % 256 == 0), reduce
//                       the dot over the 64 lanes, write g_k and stage the two gathered rows;
//   line_update_kernel  one wave per table row (N rows of U, then N rows of C): sum the row's
//                       contributions g_k * staged row in ascending k (a ballot over the staged
//                       h / t list, 64 samples per scan step), then the Keras-form Adam on the row.
// The update reads only the staged rows, so dC sees the pre-update U and dU the pre-update C; there
// is no gradient buffer and no float atomic, and every sum has one fixed order: a run is
// bit-reproducible.  Every launch is bounded (no persistent grid, no waiting on other workgroups).
#include "common.hpp"
#include "philox.hpp"

namespace hicgat {

constexpr uint32_t kLineSite = HICGAT_LINE_SITE;

__device__ __forceinline__ float line_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }   // [0, 1)
__device__ __forceinline__ int line_index(uint32_t w, int n) { return (int)(((uint64_t)w * (uint64_t)n) >> 32); }
__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// What the sample stream is made of (by value).
struct LineStream {
  const int32_t *head, *tail, *edge_alias, *node_alias, *perm;
  const float *edge_accept, *node_accept;
  int E, N, B, R;            // R = 1 + negative_ratio batches per chunk
  int64_t chunks;            // chunks per pass = ceil(E / B)
  int64_t pass_begin;        // perm holds passes [pass_begin, pass_begin + n_pass)
  uint64_t seed;
};

__device__ __forceinline__ uint4 line_words(const LineStream &s, int64_t step, int slot) {
  return philox4x32_10(make_uint4((uint32_t)slot, (uint32_t)step, (uint32_t)((uint64_t)step >> 32), kLineSite),
                       (uint32_t)s.seed, (uint32_t)(s.seed >> 32));
}

// samples of step `step`: the chunk's start in its pass, and its length
__device__ __host__ __forceinline__ int line_batch_len(int E, int B, int R, int64_t chunks, int64_t step) {
  const int64_t c = (step % (chunks * R)) / R;
  const int64_t left = (int64_t)E - c * B;
  return (int)(left < B ? left : B);
}

// (h, t, y) of slot `slot` (< the batch's length) of step `step`
__device__ __forceinline__ void line_draw(const LineStream &s, int64_t step, int slot, int &h, int &t, int &y) {
  const int64_t per_pass = s.chunks * s.R;
  const int64_t pass = step / per_pass, r = step % per_pass;
  const int64_t c = r / s.R;
  const int b = (int)(r % s.R);
  // the chunk's positives: drawn by the words of its batch 0 (step - b)
  int i = s.perm[(pass - s.pass_begin) * (int64_t)s.E + c * s.B + slot];
  i = clampi(i, s.E);
  const uint4 w0 = line_words(s, step - b, slot);
  if (line_uniform(w0.x) >= s.edge_accept[i]) i = clampi(s.edge_alias[i], s.E);
  h = clampi(s.head[i], s.N);
  if (b == 0) {
    t = clampi(s.tail[i], s.N);
    y = 1;
  } else {
    const uint4 w = line_words(s, step, slot);
    const int n = line_index(w.x, s.N);
    t = line_uniform(w.y) < s.node_accept[n] ? n : clampi(s.node_alias[n], s.N);
    y = -1;
  }
}

__global__ __launch_bounds__(256) void line_samples_kernel(LineStream s, int64_t step_begin, int64_t nsteps,
                                                           int32_t *__restrict__ h, int32_t *__restrict__ t,
                                                           int32_t *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nsteps * s.B) return;
  const int64_t step = step_begin + idx / s.B;
  const int slot = (int)(idx % s.B);
  int hh = -1, tt = -1, yy = 0;
  if (slot < line_batch_len(s.E, s.B, s.R, s.chunks, step)) line_draw(s, step, slot, hh, tt, yy);
  h[idx] = hh;
  t[idx] = tt;
  y[idx] = yy;
}

// V = float4 (D % 256 == 0) or float (any D % 64 == 0); nq = D / (64 * width) chunks per lane
template <typename V>
__device__ __forceinline__ float vdot(V a, V b);
template <>
__device__ __forceinline__ float vdot<float>(float a, float b) { return a * b; }
template <>
__device__ __forceinline__ float vdot<float4>(float4 a, float4 b) { return f4_dot(a, b); }

template <typename V>
__global__ __launch_bounds__(256) void line_grad_kernel(LineStream s, int64_t step, int len, int nq,
                                                        const float *__restrict__ U, const float *__restrict__ C,
                                                        float *__restrict__ SU, float *__restrict__ SC,
                                                        float *__restrict__ g, int32_t *__restrict__ hs,
                                                        int32_t *__restrict__ ts) {
  const int lane = lane_id();
  const int k = blockIdx.x * 4 + wave_in_block();
  if (k >= len) return;
  int h, t, y;
  line_draw(s, step, k, h, t, y);
  const size_t rowv = (size_t)nq * 64;                     // V elements per row
  const V *u = reinterpret_cast<const V *>(U) + (size_t)h * rowv;
  const V *c = reinterpret_cast<const V *>(C) + (size_t)t * rowv;
  V *su = reinterpret_cast<V *>(SU) + (size_t)k * rowv;
  V *sc = reinterpret_cast<V *>(SC) + (size_t)k * rowv;
  float dot = 0.f;
  for (int q = 0; q < nq; ++q) {
    const V a = u[q * 64 + lane], b = c[q * 64 + lane];
    dot += vdot<V>(a, b);
    su[q * 64 + lane] = a;
    sc[q * 64 + lane] = b;
  }
  dot = wave_sum(dot);
  if (lane == 0) {
    const float yf = (float)y;
    const float sig = 1.f / (1.f + expf(yf * dot));        // sigmoid(-y s)
    g[k] = -(yf / (float)len) * sig;
    hs[k] = h;
    ts[k] = t;
  }
}

struct LineAdam {
  float b1, c1, b2, c2, eps, lr_t;
};

__device__ __forceinline__ void line_adam(float &p, float g, float &m, float &v, const LineAdam &k) {
  m = fmaf(k.b1, m, k.c1 * g);
  v = fmaf(k.b2, v, k.c2 * (g * g));
  p = p - __fdiv_rn(k.lr_t * m, sqrt_rn_f32(v) + k.eps);
}
__device__ __forceinline__ void line_adam(float4 &p, float4 g, float4 &m, float4 &v, const LineAdam &k) {
  line_adam(p.x, g.x, m.x, v.x, k);
  line_adam(p.y, g.y, m.y, v.y, k);
  line_adam(p.z, g.z, m.z, v.z, k);
  line_adam(p.w, g.w, m.w, v.w, k);
}
__device__ __forceinline__ float vfma(float a, float x, float acc) { return fmaf(a, x, acc); }
__device__ __forceinline__ float4 vfma(float a, float4 x, float4 acc) { return f4_fma(a, x, acc); }
template <typename V>
__device__ __forceinline__ V vzero();
template <>
__device__ __forceinline__ float vzero<float>() { return 0.f; }
template <>
__device__ __forceinline__ float4 vzero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// rows [0, N): U (its samples: h == row, contribution g * staged C row); rows [N, 2N): C (t == row,
// g * staged U row).  NQ: the most chunks a lane holds (16 scalars or 4 float4 at D = 1024).
template <typename V, int NQ>
__global__ __launch_bounds__(256) void line_update_kernel(int N, int len, int nq, const float *__restrict__ SU,
                                                          const float *__restrict__ SC, const float *__restrict__ g,
                                                          const int32_t *__restrict__ hs, const int32_t *__restrict__ ts,
                                                          float *__restrict__ U, float *__restrict__ C,
                                                          float *__restrict__ mU, float *__restrict__ vU,
                                                          float *__restrict__ mC, float *__restrict__ vC, LineAdam k) {
  const int lane = lane_id();
  const int row = blockIdx.x * 4 + wave_in_block();
  if (row >= 2 * N) return;
  const bool ctx = row >= N;
  const int n = ctx ? row - N : row;
  const int32_t *idx = ctx ? ts : hs;
  const size_t rowv = (size_t)nq * 64;
  const V *src = reinterpret_cast<const V *>(ctx ? SU : SC);
  V acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = vzero<V>();
  for (int base = 0; base < len; base += 64) {
    const int kk = base + lane;
    uint64_t m = __ballot(kk < len && idx[kk] == n);
    while (m) {                                            // ascending k
      const int j = base + __builtin_ctzll(m);
      m &= m - 1;
      const float gk = g[j];
      const V *r = src + (size_t)j * rowv;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (q < nq) acc[q] = vfma(gk, r[q * 64 + lane], acc[q]);
    }
  }
  V *p = reinterpret_cast<V *>(ctx ? C : U) + (size_t)n * rowv;
  V *pm = reinterpret_cast<V *>(ctx ? mC : mU) + (size_t)n * rowv;
  V *pv = reinterpret_cast<V *>(ctx ? vC : vU) + (size_t)n * rowv;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q < nq) {
      V pp = p[q * 64 + lane], mm = pm[q * 64 + lane], vv = pv[q * 64 + lane];
      line_adam(pp, acc[q], mm, vv, k);
      p[q * 64 + lane] = pp;
      pm[q * 64 + lane] = mm;
      pv[q * 64 + lane] = vv;
    }
  }
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// what both entry points check about the stream; fills s
inline int line_stream_args(const int32_t *head, const int32_t *tail, const float *edge_accept,
                            const int32_t *edge_alias, int E, const float *node_accept, const int32_t *node_alias,
                            int N, const int32_t *perm, int64_t pass_begin, int64_t n_pass, int batch_size,
                            int negative, uint64_t seed, int64_t step_begin, int64_t step_end, LineStream &s) {
  if (E < 0 || N < 0 || batch_size < 1 || negative < 0 || negative > 64 || pass_begin < 0 || n_pass < 0 ||
      step_begin < 0 || step_end < step_begin)
    return HICGAT_EINVAL;
  if (E == 0 || step_end == step_begin) return HICGAT_OK;
  if (N < 1 || !head || !tail || !edge_accept || !edge_alias || !node_accept || !node_alias || !perm)
    return HICGAT_EINVAL;
  s = LineStream{head, tail, edge_alias, node_alias, perm, edge_accept, node_accept, E, N, batch_size, 1 + negative,
                 ((int64_t)E + batch_size - 1) / batch_size, pass_begin, seed};
  const int64_t per_pass = s.chunks * s.R;
  if (step_begin / per_pass < pass_begin || (step_end - 1) / per_pass >= pass_begin + n_pass) return HICGAT_EINVAL;
  return HICGAT_OK;
}

}  // namespace hicgat

using namespace hicgat;

extern "C" size_t hicgat_line_workspace_bytes(int D, int batch_size) {
  if (D < 1 || batch_size < 1) return 0;
  return 2 * align16((size_t)batch_size * D * sizeof(float)) + 3 * align16((size_t)batch_size * 4);
}

extern "C" int hicgat_line_samples(const int32_t *head, const int32_t *tail, const float *edge_accept,
                                   const int32_t *edge_alias, int E, const float *node_accept,
                                   const int32_t *node_alias, int N, const int32_t *perm, int64_t pass_begin,
                                   int64_t n_pass, int batch_size, int negative, uint64_t seed, int64_t step_begin,
                                   int64_t step_end, int32_t *h, int32_t *t, int32_t *y, hicgat_stream_t stream) {
  LineStream s{};
  const int rc = line_stream_args(head, tail, edge_accept, edge_alias, E, node_accept, node_alias, N, perm,
                                  pass_begin, n_pass, batch_size, negative, seed, step_begin, step_end, s);
  if (rc != HICGAT_OK) return rc;
  if (E == 0 || step_end == step_begin) return HICGAT_OK;
  if (!h || !t || !y) return HICGAT_EINVAL;
  const int64_t nsteps = step_end - step_begin, total = nsteps * batch_size;
  if ((total + 255) / 256 > 0x7fffffffll) return HICGAT_EUNSUPPORTED;
  hipLaunchKernelGGL(line_samples_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s,
                     step_begin, nsteps, h, t, y);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_line_train(const int32_t *head, const int32_t *tail, const float *edge_accept,
                                 const int32_t *edge_alias, int E, const float *node_accept,
                                 const int32_t *node_alias, int N, const int32_t *perm, int64_t pass_begin,
                                 int64_t n_pass, int D, int batch_size, int negative, uint64_t seed,
                                 int64_t step_begin, int64_t step_end, double lr, double beta1, double beta2,
                                 double eps, float *U, float *C, float *mU, float *vU, float *mC, float *vC,
                                 void *workspace, size_t workspace_bytes, hicgat_stream_t stream) {
  if (D < 64 || D % 64 || D > 1024) return HICGAT_EUNSUPPORTED;
  if (batch_size < 1) return HICGAT_EINVAL;
  LineStream s{};
  const int rc = line_stream_args(head, tail, edge_accept, edge_alias, E, node_accept, node_alias, N, perm,
                                  pass_begin, n_pass, batch_size, negative, seed, step_begin, step_end, s);
  if (rc != HICGAT_OK) return rc;
  if (E == 0 || step_end == step_begin) return HICGAT_OK;
  if (!U || !C || !mU || !vU || !mC || !vC || !workspace) return HICGAT_EINVAL;
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
    return HICGAT_EINVAL;
  if (workspace_bytes < hicgat_line_workspace_bytes(D, batch_size)) return HICGAT_EINVAL;
  if (misaligned(U, 16) || misaligned(C, 16) || misaligned(mU, 16) || misaligned(vU, 16) || misaligned(mC, 16) ||
      misaligned(vC, 16) || misaligned(workspace, 16))
    return HICGAT_EINVAL;
  if (N > 0x3fffffff) return HICGAT_EUNSUPPORTED;

  char *ws = static_cast<char *>(workspace);
  const size_t rows = align16((size_t)batch_size * D * sizeof(float)), vec = align16((size_t)batch_size * 4);
  float *SU = reinterpret_cast<float *>(ws), *SC = reinterpret_cast<float *>(ws + rows);
  float *g = reinterpret_cast<float *>(ws + 2 * rows);
  int32_t *hs = reinterpret_cast<int32_t *>(ws + 2 * rows + vec), *ts = reinterpret_cast<int32_t *>(ws + 2 * rows + 2 * vec);

  const bool wide = D % 256 == 0;
  const int nq = wide ? D / 256 : D / 64;
  const dim3 block(256), ugrid((2u * (unsigned)N + 3u) / 4u);
  hipStream_t st = (hipStream_t)stream;
  LineAdam k{(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, 0.f};
  for (int64_t step = step_begin; step < step_end; ++step) {
    const int len = line_batch_len(E, batch_size, s.R, s.chunks, step);
    const double t = (double)(step + 1);                   // Keras' iterations + 1
    k.lr_t = (float)(lr * std::sqrt(1.0 - std::pow(beta2, t)) / (1.0 - std::pow(beta1, t)));
    const dim3 ggrid(((unsigned)len + 3u) / 4u);
    if (wide) {
      hipLaunchKernelGGL(line_grad_kernel<float4>, ggrid, block, 0, st, s, step, len, nq, U, C, SU, SC, g, hs, ts);
      HICGAT_CHECK_LAUNCH();
      hipLaunchKernelGGL((line_update_kernel<float4, 4>), ugrid, block, 0, st, N, len, nq, SU, SC, g, hs, ts, U, C, mU,
                         vU, mC, vC, k);
    } else {
      hipLaunchKernelGGL(line_grad_kernel<float>, ggrid, block, 0, st, s, step, len, nq, U, C, SU, SC, g, hs, ts);
      HICGAT_CHECK_LAUNCH();
      hipLaunchKernelGGL((line_update_kernel<float, 16>), ugrid, block, 0, st, N, len, nq, SU, SC, g, hs, ts, U, C, mU,
                         vU, mC, vC, k);
    }
    HICGAT_CHECK_LAUNCH();
  }
  return HICGAT_OK;
}
