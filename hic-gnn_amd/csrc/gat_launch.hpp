// The launch layer of the GATConv aggregation passes (gat_fwd.hip, gat_bwd.hip): the supported-shape
// rule, the one list of shapes that have kernels, the run-time-value-to-template-argument helpers
// their launches share, and the declarations of what crosses a translation unit.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace hicgat {

// The supported-shape rule (include/hicgat.h; hicgat.ops.gat_shape_supported is its Python copy).
constexpr bool gat_shape_supported(int H, int C) {
  return H >= 1 && H <= 4 && C > 0 && C % 128 == 0 && (H * C) % 256 == 0 && H * C <= 1024;
}

template <int H_, int C_> struct GatShape {
  static_assert(gat_shape_supported(H_, C_), "listed, but not in the rule");
  static constexpr int H = H_, C = C_;
  // the flagship's shape: entry kernels under the names the profiles know, with measured launch parameters
  static constexpr bool h2c256 = H_ == 2 && C_ == 256;
};

// f(GatShape<H, C>{}) for the run-time (H, C); HICGAT_EUNSUPPORTED where the list has no such shape.
template <class F> int for_gat_shape(int H, int C, F &&f) {
  int rc = HICGAT_EUNSUPPORTED;
  auto at = [&](auto shape) {
    if (H == shape.H && C == shape.C) rc = f(shape);
  };
  at(GatShape<1, 256>{}), at(GatShape<1, 512>{}), at(GatShape<1, 768>{}), at(GatShape<1, 1024>{});
  at(GatShape<2, 128>{}), at(GatShape<2, 256>{}), at(GatShape<2, 384>{}), at(GatShape<2, 512>{});
  at(GatShape<3, 256>{}), at(GatShape<4, 128>{}), at(GatShape<4, 256>{});
  return rc;
}

// ... and the list has every shape of the rule: 11 listed, 11 admitted
constexpr int gat_shapes_in_rule() {
  int n = 0;
  for (int H = 1; H <= 4; ++H)
    for (int C = 128; C <= 1024; C += 128) n += gat_shape_supported(H, C);
  return n;
}
static_assert(gat_shapes_in_rule() == 11, "for_gat_shape's list and gat_shape_supported disagree");

// f(std::bool_constant<b>{}...) for run-time bools (TRAIN, ACT, REMAP)
template <bool... B, class F> int with_flags(F &&f) { return f(std::bool_constant<B>{}...); }
template <bool... B, class F, class... R> int with_flags(F &&f, bool b, R... rest) {
  return b ? with_flags<B..., true>(f, rest...) : with_flags<B..., false>(f, rest...);
}

// The source pass's operands beside the graph and the features, as hicgat_gat_agg_bwd_src checked them.
struct SrcArgs {
  const float *row_stats;
  int64_t ldr;   // row_stats' row stride in floats
  const float *dout;
  int64_t ldq4;  // dout's row stride in float4s
  const float *att_s, *att_d;
  float *dh, *da_src;
};

// The tiled form of each pass (gat_tiles.hip), called by the entry point after the checks every form
// shares: refuses what only it reads (the tile arrays, splits and the workspace; HICGAT_EINVAL), then
// launches the gather half and the tile kernels.
int agg_fwd_tiled(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const hicgat_gat_tiles &t, const float *bias,
                  int act, float *out, float *out2, float *row_stats, hipStream_t s);
int agg_bwd_src_tiled(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const hicgat_gat_tiles &t,
                      const SrcArgs &a, hipStream_t s);
// Their gather halves, defined beside the SPLIT entry kernels:
// gat_fwd.hip: raw sums over the sparse remainder
int agg_fwd_split_launch(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const hicgat_gat_tiles &t, float *out,
                         float *out2, float *row_stats, hipStream_t s);
// gat_bwd.hip: the sparse remainder's shares
int agg_bwd_src_split_launch(const hicgat_gat_graph &g, const hicgat_gat_feats &f, const hicgat_gat_tiles &t,
                             const SrcArgs &a, hipStream_t s);

}  // namespace hicgat
