// Feature dropout with a counter-based mask (include/hicgat.h "feature dropout"): the zoo's
// act -> torch.nn.Dropout pair as one streaming pass, its backward from the saved output, the mask
// alone (tests / tools) and the step count's advance.
//
// One thread per four columns of a row: one Philox4x32-10 call (its four words serve the four
// columns), one 16-byte load, one 16-byte store.  A quad's bits depend only on (seed, step, site,
// global row, column quad), never on which thread or block computes it, so the grid is free: at most
// kMaxBlocks blocks stride over the quads, each thread carrying (row, quad) forward by a stride the
// host split into whole rows and a remainder (no division in the loop).  No LDS, no scratch.
#include "philox.hpp"

using namespace hicgat;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;   // 8 blocks per CU; the rest of a tall tensor is strided

// The walk of one thread over the quads of an M x (4 W4) tensor: thread t starts at quad t of the
// row-major quad order and moves on by gridDim.x * kThreads quads = drow rows + dq quads.
struct QuadWalk {
  int64_t row;
  int q;
  __device__ __forceinline__ QuadWalk(int W4) {
    const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    row = t / (uint32_t)W4;
    q = (int)(t % (uint32_t)W4);
  }
  __device__ __forceinline__ void next(int W4, int drow, int dq) {
    row += drow;
    q += dq;
    if (q >= W4) {
      q -= W4;
      ++row;
    }
  }
};

template <int ACT>
__global__ __launch_bounds__(kThreads) void act_dropout_fwd_kernel(const float *x, int64_t ldx, int M, int W4,
                                                                   int drow, int dq, float slope, float scale,
                                                                   MaskArgs m, float *y, int64_t ldy) {
  const uint32_t step = mask_step(m);
  for (QuadWalk w(W4); w.row < M; w.next(W4, drow, dq)) {
    const uint4 r = quad_words(m, step, m.row_offset + w.row, W4, w.q);
    const float4 v = *reinterpret_cast<const float4 *>(x + w.row * ldx + 4 * w.q);
    float4 o;
    o.x = r.x >= m.T ? act_apply<ACT>(v.x, slope) * scale : 0.f;
    o.y = r.y >= m.T ? act_apply<ACT>(v.y, slope) * scale : 0.f;
    o.z = r.z >= m.T ? act_apply<ACT>(v.z, slope) * scale : 0.f;
    o.w = r.w >= m.T ? act_apply<ACT>(v.w, slope) * scale : 0.f;
    *reinterpret_cast<float4 *>(y + w.row * ldy + 4 * w.q) = o;
  }
}

__global__ __launch_bounds__(kThreads) void dropout_mask_kernel(uint8_t *mask, int M, int W4, int drow, int dq,
                                                                MaskArgs m) {
  const uint32_t step = mask_step(m);
  for (QuadWalk w(W4); w.row < M; w.next(W4, drow, dq)) {
    const uint4 r = quad_words(m, step, m.row_offset + w.row, W4, w.q);
    const uchar4 o = make_uchar4(r.x >= m.T, r.y >= m.T, r.z >= m.T, r.w >= m.T);
    *reinterpret_cast<uchar4 *>(mask + (w.row * W4 + w.q) * 4) = o;
  }
}

template <int ACT>
__global__ __launch_bounds__(kThreads) void act_dropout_bwd_kernel(const float *dy, int64_t lddy, const float *y,
                                                                   int64_t ldy, int M, int W4, int drow, int dq,
                                                                   float slope, float scale, float *dx,
                                                                   int64_t lddx) {
  for (QuadWalk w(W4); w.row < M; w.next(W4, drow, dq)) {
    const float4 g = *reinterpret_cast<const float4 *>(dy + w.row * lddy + 4 * w.q);
    const float4 v = *reinterpret_cast<const float4 *>(y + w.row * ldy + 4 * w.q);
    float4 o;
    o.x = act_dropout_grad<ACT>(g.x, v.x, slope, scale);
    o.y = act_dropout_grad<ACT>(g.y, v.y, slope, scale);
    o.z = act_dropout_grad<ACT>(g.z, v.z, slope, scale);
    o.w = act_dropout_grad<ACT>(g.w, v.w, slope, scale);
    *reinterpret_cast<float4 *>(dx + w.row * lddx + 4 * w.q) = o;
  }
}

// one wave; lane 0 writes (a per-lane vector store, like every other store of the library)
__global__ __launch_bounds__(64) void dropout_advance_kernel(int64_t *counter) {
  const int64_t v = *counter + 1;
  if (threadIdx.x == 0) *counter = v;
}

// ---- host side ------------------------------------------------------------------------------------
// Grid of the walk over M rows of W4 quads, and the stride of one step of it in rows + quads.
struct Walk {
  int blocks, drow, dq;
  Walk(int M, int W4) {
    const int64_t quads = (int64_t)M * W4;
    const int64_t need = (quads + kThreads - 1) / kThreads;
    blocks = (int)(need < kMaxBlocks ? need : kMaxBlocks);
    const int64_t stride = (int64_t)blocks * kThreads;
    drow = (int)(stride / W4);
    dq = (int)(stride % W4);
  }
};

}  // namespace

extern "C" int hicgat_act_dropout_fwd(const float *x, int64_t ldx, int M, int W, int act, float slope, double p,
                                      uint64_t seed, const int64_t *step_counter, int64_t step_value, uint32_t site,
                                      int64_t row_offset, float *y, int64_t ldy, hicgat_stream_t stream) {
  if (M < 0 || W <= 0 || !x || !y || !p_ok(p) || row_offset < 0 || act < HICGAT_ACT_NONE ||
      act > HICGAT_ACT_LEAKY_RELU || ldx < W || ldy < W)
    return HICGAT_EINVAL;
  if (W % 4 || ldx % 4 || ldy % 4) return HICGAT_EUNSUPPORTED;
  if (misaligned(x, 16) || misaligned(y, 16) || misaligned(step_counter, 8)) return HICGAT_EINVAL;
  if (M == 0) return HICGAT_OK;
  const int W4 = W / 4;
  const Walk wk(M, W4);
  const MaskArgs m{seed, step_counter, step_value, row_offset, site, keep_threshold(p)};
  const float scale = keep_scale(p);
  const dim3 grid(wk.blocks), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  if (act == HICGAT_ACT_RELU)
    hipLaunchKernelGGL(act_dropout_fwd_kernel<HICGAT_ACT_RELU>, grid, block, 0, s, x, ldx, M, W4, wk.drow, wk.dq,
                       slope, scale, m, y, ldy);
  else if (act == HICGAT_ACT_LEAKY_RELU)
    hipLaunchKernelGGL(act_dropout_fwd_kernel<HICGAT_ACT_LEAKY_RELU>, grid, block, 0, s, x, ldx, M, W4, wk.drow,
                       wk.dq, slope, scale, m, y, ldy);
  else
    hipLaunchKernelGGL(act_dropout_fwd_kernel<HICGAT_ACT_NONE>, grid, block, 0, s, x, ldx, M, W4, wk.drow, wk.dq,
                       slope, scale, m, y, ldy);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_act_dropout_bwd(const float *dy, int64_t lddy, const float *y, int64_t ldy, int M, int W,
                                      int act, float slope, double p, float *dx, int64_t lddx,
                                      hicgat_stream_t stream) {
  if (M < 0 || W <= 0 || !dy || !y || !dx || !p_ok(p) || act < HICGAT_ACT_NONE || act > HICGAT_ACT_LEAKY_RELU ||
      lddy < W || ldy < W || lddx < W)
    return HICGAT_EINVAL;
  if (act == HICGAT_ACT_NONE) return HICGAT_EUNSUPPORTED;
  if (act == HICGAT_ACT_LEAKY_RELU && !(slope > 0.f)) return HICGAT_EINVAL;
  if (W % 4 || lddy % 4 || ldy % 4 || lddx % 4) return HICGAT_EUNSUPPORTED;
  if (misaligned(dy, 16) || misaligned(y, 16) || misaligned(dx, 16)) return HICGAT_EINVAL;
  if (M == 0) return HICGAT_OK;
  const int W4 = W / 4;
  const Walk wk(M, W4);
  const float scale = keep_scale(p);
  const dim3 grid(wk.blocks), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  if (act == HICGAT_ACT_RELU)
    hipLaunchKernelGGL(act_dropout_bwd_kernel<HICGAT_ACT_RELU>, grid, block, 0, s, dy, lddy, y, ldy, M, W4, wk.drow,
                       wk.dq, slope, scale, dx, lddx);
  else
    hipLaunchKernelGGL(act_dropout_bwd_kernel<HICGAT_ACT_LEAKY_RELU>, grid, block, 0, s, dy, lddy, y, ldy, M, W4,
                       wk.drow, wk.dq, slope, scale, dx, lddx);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_dropout_mask(uint8_t *mask, int M, int W, double p, uint64_t seed, const int64_t *step_counter,
                                   int64_t step_value, uint32_t site, int64_t row_offset, hicgat_stream_t stream) {
  if (M < 0 || W <= 0 || !mask || !p_ok(p) || row_offset < 0) return HICGAT_EINVAL;
  if (W % 4) return HICGAT_EUNSUPPORTED;
  if (misaligned(mask, 4) || misaligned(step_counter, 8)) return HICGAT_EINVAL;
  if (M == 0) return HICGAT_OK;
  const int W4 = W / 4;
  const Walk wk(M, W4);
  const MaskArgs m{seed, step_counter, step_value, row_offset, site, keep_threshold(p)};
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(wk.blocks), dim3(kThreads), 0, (hipStream_t)stream, mask, M, W4,
                     wk.drow, wk.dq, m);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_dropout_advance(int64_t *counter, hicgat_stream_t stream) {
  if (!counter || misaligned(counter, 8)) return HICGAT_EINVAL;
  hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}
