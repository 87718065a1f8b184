// The counter-based keep mask of feature dropout (include/hicgat.h "feature dropout"), shared by
// dropout.hip and batchnorm.hip: Philox4x32-10 over (global row, column quad, step, site) keyed by
// the seed, and the host-side threshold / scale of a drop probability.  Also the per-(edge, head)
// mask of attention dropout (gat_agg.hpp's DROP forms): the same generator over (i, j, step, site).
#pragma once
#include "common.hpp"

namespace hicgat {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c.x), lo0 = kPhiloxM0 * c.x;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c.z), lo1 = kPhiloxM1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}

// What a launch needs to know about the mask (by value: 40 bytes of kernel arguments).
struct MaskArgs {
  uint64_t seed;
  const int64_t *step_counter;   // device; NULL: step_value
  int64_t step_value;
  int64_t row_offset;
  uint32_t site, T;
};

__device__ __forceinline__ uint32_t mask_step(const MaskArgs &m) {
  return (uint32_t)(m.step_counter ? *m.step_counter : m.step_value);
}

// The four random words of column quad `q` of global row `R` (W4 quads per row).
__device__ __forceinline__ uint4 quad_words(const MaskArgs &m, uint32_t step, int64_t R, int W4, int q) {
  const uint64_t g = (uint64_t)R * (uint64_t)W4 + (uint64_t)q;
  return philox4x32_10(make_uint4((uint32_t)g, (uint32_t)(g >> 32), step, m.site), (uint32_t)m.seed,
                       (uint32_t)(m.seed >> 32));
}

// ---- attention dropout (include/hicgat.h "attention dropout"): one keep bit per (edge, head), a
// pure function of (seed, step, site, destination row i, source row j, head).  One Philox call per
// edge, counter (i, j, step, site | kAttnSiteBit); head hh uses output word hh (H <= 4).  i and j are
// global node ids, so the source pass recomputes the bits of edge (i -> r) from (col[e], r).
constexpr uint32_t kAttnSiteBit = HICGAT_ATTN_SITE_BIT;  // keeps attention sites apart from feature-dropout sites

// What a DROP launch needs to know about the mask (by value: 40 bytes of kernel arguments).
struct AttnMaskArgs {
  uint64_t seed;
  const int64_t *step_counter;   // device; NULL: step_value
  int64_t step_value;
  uint32_t site, T;              // site with kAttnSiteBit already set
  float scale;
};

__device__ __forceinline__ uint32_t mask_step(const AttnMaskArgs &m) {
  return (uint32_t)(m.step_counter ? *m.step_counter : m.step_value);
}

// keep[hh] of edge (destination i, source j)
template <int H>
__device__ __forceinline__ void attn_keep(const AttnMaskArgs &m, uint32_t step, int i, int j, bool (&keep)[H]) {
  static_assert(H >= 1 && H <= 4, "one Philox call serves at most four heads");
  const uint4 r = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)j, step, m.site), (uint32_t)m.seed,
                                (uint32_t)(m.seed >> 32));
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int hh = 0; hh < H; ++hh) keep[hh] = w[hh] >= m.T;
}

// the factor m_ij in {0, scale} that multiplies alpha_ij, per head
template <int H>
__device__ __forceinline__ void attn_factor(const AttnMaskArgs &m, uint32_t step, int i, int j, float (&f)[H]) {
  bool keep[H];
  attn_keep<H>(m, step, i, j, keep);
#pragma unroll
  for (int hh = 0; hh < H; ++hh) f[hh] = keep[hh] ? m.scale : 0.f;
}

template <int ACT>
__device__ __forceinline__ float act_apply(float x, float slope) {
  if (ACT == HICGAT_ACT_RELU) return relu_t(x);
  if (ACT == HICGAT_ACT_LEAKY_RELU) return lrelu(x, slope);
  return x;
}

// g = dy * scale is the gradient that reaches the activation's output (rounded once, as torch's
// mul backward rounds it); the saved y's sign then selects the activation's branch.
template <int ACT>
__device__ __forceinline__ float act_dropout_grad(float dy, float y, float slope, float scale) {
  const float g = dy * scale;
  if (ACT == HICGAT_ACT_RELU) return y > 0.f ? g : 0.f;
  return y > 0.f ? g : (y < 0.f ? g * slope : 0.f);
}

// ---- host side ------------------------------------------------------------------------------------
inline bool p_ok(double p) { return p >= 0.0 && p < 1.0; }   // false for NaN

inline uint32_t keep_threshold(double p) {
  const double t = __builtin_floor(p * 4294967296.0);
  return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}

inline float keep_scale(double p) { return (float)(1.0 / (1.0 - p)); }

inline bool misaligned(const void *ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) != 0; }

// attention dropout: the caller's site must leave kAttnSiteBit free (site < 2^31)
inline bool attn_drop_ok(const hicgat_attn_drop &d) {
  return p_ok(d.p) && (d.site & kAttnSiteBit) == 0 && !misaligned(d.step_counter, 8);
}

inline AttnMaskArgs attn_mask_args(const hicgat_attn_drop &d) {
  return AttnMaskArgs{d.seed, d.step_counter, d.step_value, d.site | kAttnSiteBit, keep_threshold(d.p), keep_scale(d.p)};
}

}  // namespace hicgat
