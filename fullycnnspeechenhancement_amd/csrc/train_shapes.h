// Which shapes the training step's MFMA kernels are built for, and which variants of them exist.  Host-pure (no HIP
// include): the two translation units that instantiate the kernels, the planner (train_plan.h) and its CPU test read
// the same lists.  A list names shapes only; each unit instantiates the lists it names in its own dispatchers.
#pragma once
#include "rced_spec.h"

// forward shapes (cin, taps, cout) of the 1xk layers and the shapes of their dgrad convolutions (cout, taps, cin):
// CR-CED V3, then R-CED V1 (train_api.hip) ...
#define RCED_TM_FWD(X)                        \
  X(8, 9, 18) X(18, 5, 30) X(30, 9, 8)        \
  X(12, 11, 16) X(16, 9, 20) X(20, 7, 24) X(24, 7, 32) X(32, 7, 24) X(24, 9, 20) X(20, 11, 16) X(16, 13, 12)
#define RCED_TM_BWD(X)                                   \
  X(18, 9, 8) X(30, 5, 18) X(8, 9, 30) X(1, 129, 8)      \
  X(16, 11, 12) X(20, 9, 16) X(24, 7, 20) X(32, 7, 24) X(24, 7, 32) X(20, 9, 24) X(16, 11, 20) X(12, 13, 16)
// ... and R-CED V2 in its even-padded internal layout (train_mfma_v2.hip)
#define RCED_TM_FWD_V2(X)                                                                                      \
  X(10, 7, 12) X(12, 5, 14) X(14, 5, 16) X(16, 5, 20) X(20, 5, 22) X(22, 7, 24) X(24, 11, 26) X(26, 7, 24)      \
  X(24, 5, 22) X(22, 5, 20) X(20, 5, 16) X(16, 5, 14) X(14, 7, 12) X(12, 11, 10)
#define RCED_TM_BWD_V2(X)                                                                                      \
  X(12, 7, 10) X(14, 5, 12) X(16, 5, 14) X(20, 5, 16) X(22, 5, 20) X(24, 7, 22) X(26, 11, 24) X(24, 7, 26)      \
  X(22, 5, 24) X(20, 5, 22) X(16, 5, 20) X(14, 5, 16) X(12, 7, 14) X(10, 11, 12)
// wgrad + dgrad of a layer in one kernel (tmm::bwd_fused_mfma): the CR-CED shapes whose input tensor has one consumer
#define RCED_TM_FUSED(X) X(18, 5, 30) X(30, 9, 8)
// forward shapes built in the three-part bf16 form (tmm::conv_x6_fwd): CR-CED's 18 -> 30 layers (no remainder pass; the
// 30 -> 8 layers' three planes + packet do not leave room for two workgroups per CU: tmm::GeoX6::kFits; the 8 -> 18 layers
// wait for their tiles, not for the fp32 matrix pipe: DESIGN 3.5, "tried and retired")
#define RCED_TM_X6_FWD(X) X(18, 5, 30)
#define RCED_FIRST(X) X(9, 18) X(13, 12) X(11, 10)   // first layer (8 x kw on the 1-channel input): (kw, cout)
#define RCED_FIN_CH(X) X(8) X(10) X(12)              // output layer (1x129, CH -> 1): CH

namespace rced {
namespace tms {

#define RCED_SHAPE_IS(CI, TP, CO) if (cin == CI && taps == TP && cout == CO) return true;
constexpr bool tm_has_main(bool fwd, int cin, int taps, int cout) {
  if (fwd) { RCED_TM_FWD(RCED_SHAPE_IS) } else { RCED_TM_BWD(RCED_SHAPE_IS) }
  return false;
}
constexpr bool tm_has_v2(bool fwd, int cin, int taps, int cout) {
  if (fwd) { RCED_TM_FWD_V2(RCED_SHAPE_IS) } else { RCED_TM_BWD_V2(RCED_SHAPE_IS) }
  return false;
}
// a 1xk convolution kernel (fwd: also the wgrad kernel of that forward shape) exists in one of the two units
constexpr bool tm_has(bool fwd, int cin, int taps, int cout) { return tm_has_main(fwd, cin, taps, cout) || tm_has_v2(fwd, cin, taps, cout); }
constexpr bool tm_fused_has(int cin, int taps, int cout) { RCED_TM_FUSED(RCED_SHAPE_IS) return false; }
constexpr bool tm_x6_has(int cin, int taps, int cout) { RCED_TM_X6_FWD(RCED_SHAPE_IS) return false; }
#undef RCED_SHAPE_IS
constexpr bool first_has(const LayerSpec& s, int cin) {
#define X(KW, CO) if (s.kh == 8 && cin == 1 && s.src == 0 && s.kw == KW && s.cout == CO) return true;
  RCED_FIRST(X)
#undef X
  return false;
}
constexpr bool fin_has(int ch) {
#define X(CH) if (ch == CH) return true;
  RCED_FIN_CH(X)
#undef X
  return false;
}
constexpr bool is_output_layer(const LayerSpec& s, int cin) {
  return s.kh == 1 && s.kw == kFeatureDim && s.cout == 1 && !s.use_norm && !s.use_act && s.skip_pre < 0 && s.skip_post < 0 && fin_has(cin);
}

// Which variants of tmm::conv1xk_mfma<CIN, TAPS, COUT> a built shape has: what tmd::tm_conv_launch instantiates and
// what it answers 0 to.  cin / cout are the kernel's own (a dgrad shape has the layer's cout as its cin).
//   accum: out += conv (or acc_from + conv)     stats: (sum z, sum z^2) records        xa: input rebuilt from the producer's z
//   ba: input dz rebuilt from (d_u, z)          sa: the producer's BatchNorm-backward records come out as well
constexpr bool tm_variant_has(bool fwd, int cin, int cout, bool accum, bool stats, bool xa, bool ba, bool sa) {
  if (sa) {
    if (fwd || cin % 2 != 0 || cout % 2 != 0 || stats || xa) return false;
    if (accum) return cout == 8 && ba;   // the accumulating form: the 8-channel tensors (CR-CED's skip sources) with the rebuilt dz only
    return ba || cout != 8;
  }
  if (fwd) return !accum && !ba && (!xa || cin % 2 == 0);
  return !stats && !xa && (!ba || cin % 2 == 0);
}

}  // namespace tms
}  // namespace rced
