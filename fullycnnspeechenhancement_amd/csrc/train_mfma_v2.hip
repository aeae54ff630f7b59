// R-CED V2's shapes on the MFMA training kernels.  V2's channel counts (10 12 14 15 19 21 23 25 ...) are trained in the
// even-padded internal layout of train_api.hip (10 12 14 16 20 22 24 26 24 22 20 16 14 12 10), so every shape here
// (RCED_TM_FWD_V2 / RCED_TM_BWD_V2, train_shapes.h) is even.  A translation unit of its own: these 28 shapes are half
// of the training kernels' compile time.
#include <hip/hip_runtime.h>

#include "train_mfma_dispatch.h"

using namespace rced;

namespace {
RCED_TM_DEFINE_DISPATCH(_v2, RCED_TM_FWD_V2, RCED_TM_BWD_V2)
}  // namespace

int rced_tm_conv_v2(bool fwd, int cin, int taps, int cout, bool accum, bool stats, const float* in, const float* packet,
                    float* out, int frames, const rced::tmd::Cus& cus, double* part, const tmm::XformArgs* xa, const tmm::BnBwdArgs* ba,
                    hipStream_t st, const tmm::SumArgs* sa, const float* acc_from) {
  return tm_conv_v2(fwd, cin, taps, cout, accum, stats, in, packet, out, frames, cus, part, xa, ba, st, sa, acc_from);
}
int rced_tm_wgrad_v2(const tmd::WgDet& wd, int cin, int taps, int cout, const float* x, const float* dz, float* dW, float* dbias,
                     int frames, const rced::tmd::Cus& cus, const tmm::XformArgs* xa, const tmm::BnBwdArgs* ba, hipStream_t st) {
  return tm_wgrad_v2(wd, cin, taps, cout, x, dz, dW, dbias, frames, cus, xa, ba, st);
}
