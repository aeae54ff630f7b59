// Launchers of the training step's first layer, output layer and fused backward kernels, and the forwarders that pick a
// 1xk layer's MFMA kernel from this translation unit's shapes or from train_mfma_v2.hip's.  Included by train_api.hip ONLY:
// the dispatch bodies below are not templates, and a second includer would instantiate every kernel they name again.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels_final_x6.h"
#include "kernels_train_mfma.h"
#include "rced_spec.h"
#include "train_mfma_dispatch.h"

// train_mfma_v2.hip
int rced_tm_conv_v2(bool fwd, int cin, int taps, int cout, bool accum, bool stats, const float* in, const float* packet,
                    float* out, int frames, const rced::tmd::Cus& cus, double* part, const rced::tmm::XformArgs* xa,
                    const rced::tmm::BnBwdArgs* ba, hipStream_t st, const rced::tmm::SumArgs* sa, const float* acc_from);
int rced_tm_wgrad_v2(const rced::tmd::WgDet& wd, int cin, int taps, int cout, const float* x, const float* dz, float* dW, float* dbias, int frames, const rced::tmd::Cus& cus,
                     const rced::tmm::XformArgs* xa, const rced::tmm::BnBwdArgs* ba, hipStream_t st);

namespace rced {
namespace {
using tmd::allow_lds;
using tmd::Cus;
using tmd::kPairGrid;
using tmd::WgDet;

// ---- MFMA paths for the 1xk layers (kernels_train_mfma.h, launchers in train_mfma_dispatch.h) ----
// the shapes of CR-CED V3 and R-CED V1 (RCED_TM_FWD / RCED_TM_BWD, train_shapes.h); R-CED V2 lives in train_mfma_v2.hip
RCED_TM_DEFINE_DISPATCH(_main, RCED_TM_FWD, RCED_TM_BWD)

// Returns the grid size (= number of partial-sum records when stats), 0 if no kernel was built for the request.
int tm_conv(bool fwd, int cin, int taps, int cout, bool accum, bool stats, const float* in, const float* packet, float* out,
            int frames, const Cus& cus, double* part, const tmm::XformArgs* xa, const tmm::BnBwdArgs* ba, hipStream_t st,
            const tmm::SumArgs* sa = nullptr, const float* acc_from = nullptr) {
  if (rced::tms::tm_has_main(fwd, cin, taps, cout))
    return tm_conv_main(fwd, cin, taps, cout, accum, stats, in, packet, out, frames, cus, part, xa, ba, st, sa, acc_from);
  return rced_tm_conv_v2(fwd, cin, taps, cout, accum, stats, in, packet, out, frames, cus, part, xa, ba, st, sa, acc_from);
}
int tm_wgrad(const WgDet& wd, int cin, int taps, int cout, const float* x, const float* dz, float* dW, float* dbias, int frames, const Cus& cus,
             const tmm::XformArgs* xa, const tmm::BnBwdArgs* ba, hipStream_t st) {
  if (rced::tms::tm_has_main(true, cin, taps, cout)) return tm_wgrad_main(wd, cin, taps, cout, x, dz, dW, dbias, frames, cus, xa, ba, st);
  return rced_tm_wgrad_v2(wd, cin, taps, cout, x, dz, dW, dbias, frames, cus, xa, ba, st);
}

// ---- wgrad + dgrad of a layer in one kernel (tmm::bwd_fused_mfma): RCED_TM_FUSED ----
// (x virtual, sums) must be (1, 1) or (0, 0).  Returns the grid size, 0 if no kernel was built for the request.
int tm_bwd_fused(const WgDet& wd, int cin, int taps, int cout, bool xf_sums, const float* x, const float* du, const float* packet, float* dx,
                 float* dW, float* dbias, int frames, const Cus& cus, double* part, const tmm::XformArgs* xa, const tmm::BnBwdArgs* ba,
                 hipStream_t st) {
  const tmm::XformArgs nx{nullptr, nullptr, nullptr, nullptr};
  if (!ba || (xf_sums && !xa)) return 0;
#define X(CI, TP, CO)                                                                                                          \
  if (cin == CI && taps == TP && cout == CO)                                                                                   \
    return xf_sums ? rced::tmd::tm_bwd_fused_launch<CI, TP, CO, true, true>(wd, x, du, packet, dx, dW, dbias, frames, cus, part, *xa, *ba, st) \
                   : rced::tmd::tm_bwd_fused_launch<CI, TP, CO, false, false>(wd, x, du, packet, dx, dW, dbias, frames, cus, part, nx, *ba, st);
  RCED_TM_FUSED(X)
#undef X
  return 0;
}

// ---- first layer (8 x kw on the 1-channel input, RCED_FIRST): MFMA forward and wgrad (kernels_train_mfma.h) ----
template <int KW, int COUT>
int first_wgrad_launch(const WgDet& wd, const float* x, const float* dz, float* dW, float* dbias, int frames, int T, const Cus& cus,
                       const tmm::BnBwdArgs* ba, hipStream_t st) {
  constexpr int RS = 129 + KW - 1;
  const size_t lds = (((size_t)(tmm::kTF * 8 * RS + 32 + 3) / 4) * 4 + (size_t)(tmm::kTF * tmm::first_wgrad_fs(KW, COUT) + 4) * 32 + 4 * COUT) * sizeof(float);
  const int ntiles = (frames + tmm::kTF - 1) / tmm::kTF;
  const tmm::BnBwdArgs nb{nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, nullptr};
  static unsigned long long attr_t = 0, attr_f = 0;
  static int occ_t = 0, occ_f = 0;
  allow_lds(reinterpret_cast<const void*>(tmm::first_wgrad<KW, COUT, true>), lds, attr_t);
  allow_lds(reinterpret_cast<const void*>(tmm::first_wgrad<KW, COUT, false>), lds, attr_f);
  // persistent grid = what is resident (it was cus * 3 with two workgroups per CU resident: half of the second round idle)
  const dim3 grid(cus.grid(ntiles, ba ? rced::tmd::resident_grid(reinterpret_cast<const void*>(tmm::first_wgrad<KW, COUT, true>), lds, cus, occ_t)
                                      : rced::tmd::resident_grid(reinterpret_cast<const void*>(tmm::first_wgrad<KW, COUT, false>), lds, cus, occ_f)));
  rced::tmd::wg_launch(wd, [&](float* dw, float* db, unsigned ps) {
    if (ba) hipLaunchKernelGGL((tmm::first_wgrad<KW, COUT, true>), grid, dim3(tmm::kThreads), lds, st, x, dz, dw, db, frames, T, *ba, ps);
    else hipLaunchKernelGGL((tmm::first_wgrad<KW, COUT, false>), grid, dim3(tmm::kThreads), lds, st, x, dz, dw, db, frames, T, nb, ps);
  }, (int)grid.x * tmm::kWaves, 8 * KW * COUT, COUT, dW, dbias, st);
  return 1;
}
int first_wgrad(const WgDet& wd, const LayerSpec& s, const float* x, const float* dz, float* dW, float* dbias, int frames, int T, const Cus& cus,
                const tmm::BnBwdArgs* ba, hipStream_t st) {
#define X(KW, CO) if (s.kw == KW && s.cout == CO) return first_wgrad_launch<KW, CO>(wd, x, dz, dW, dbias, frames, T, cus, ba, st);
  RCED_FIRST(X)
#undef X
  return 0;
}

template <int KW, int COUT>
int first_fwd_launch(const float* x, const float* w, const float* bias, float* packet, float* z, int frames, int T, const Cus& cus,
                     bool stats, double* part, hipStream_t st) {
  constexpr int MT = tmm::tm_rem(COUT) ? 1 : (COUT + 15) / 16, data = 2 * KW * MT * 64 + (tmm::tm_rem(COUT) ? 32 * 64 : 0), RS = 129 + KW - 1;
  hipLaunchKernelGGL(tmm::pack_first, dim3((data + 32 + 255) / 256), dim3(256), 0, st, w, bias, KW, COUT, packet);
  const size_t lds = (((size_t)(tmm::kTF * 8 * RS + 32 + 3) / 4) * 4 + data + 32) * sizeof(float);
  const int ntiles = (frames + tmm::kTF - 1) / tmm::kTF;
  static int occ_s = 0, occ_n = 0;
  const int res = stats ? rced::tmd::resident_grid(reinterpret_cast<const void*>(tmm::first_fwd<KW, COUT, true>), lds, cus, occ_s)
                        : rced::tmd::resident_grid(reinterpret_cast<const void*>(tmm::first_fwd<KW, COUT, false>), lds, cus, occ_n);
  const int grid = cus.grid(ntiles, std::min(res, kPairGrid));
  if (stats) hipLaunchKernelGGL((tmm::first_fwd<KW, COUT, true>), dim3(grid), dim3(tmm::kThreads), lds, st, x, (const float*)packet, z, frames, T, part);
  else hipLaunchKernelGGL((tmm::first_fwd<KW, COUT, false>), dim3(grid), dim3(tmm::kThreads), lds, st, x, (const float*)packet, z, frames, T, part);
  return grid;
}
// returns the grid size (= partial-sum records when stats)
int first_fwd(const LayerSpec& s, const float* x, const float* w, const float* bias, float* packet, float* z, int frames, int T,
              const Cus& cus, bool stats, double* part, hipStream_t st) {
#define X(KW, CO) if (s.kw == KW && s.cout == CO) return first_fwd_launch<KW, CO>(x, w, bias, packet, z, frames, T, cus, stats, part, st);
  RCED_FIRST(X)
#undef X
  return 0;
}
size_t first_packet_floats(const LayerSpec& s) {   // pack_first: main section, the 18-channel form's remainder section, 32 shifts
  return (size_t)2 * s.kw * (tmm::tm_rem(s.cout) ? 1 : (s.cout + 15) / 16) * 64 + (tmm::tm_rem(s.cout) ? 32 * 64 : 0) + 32;
}

// ---- output layer (1x129, CH -> 1, RCED_FIN_CH): Toeplitz forward + MFMA wgrad (kernels_train_mfma.h) ----
size_t fin_pack_floats(int ch) {
#define X(CH) if (ch == CH) return tmm::FinGeo<CH>::kPack;
  RCED_FIN_CH(X)
#undef X
  return 0;
}
// floats of the buffer that holds the output layer's packed A: the fp32 form, or the three-part bf16 form (kernels_final_x6.h)
size_t fin_pack_alloc_floats(int ch) {
  const size_t x6 = ((size_t)((129 * ch + 31) / 32) * 9 * 3 * 64 * 8 * sizeof(unsigned short) + 3) / 4;
  return std::max(fin_pack_floats(ch), x6);
}
int fin_forward(int ch, const float* h, const float* w, const float* bias, float* pack, float* y, int frames, hipStream_t st,
                bool use_x6) {
  if (use_x6) {
    // fp32 quality on the bf16 matrix pipe: every operand as three bf16 parts, six MFMAs of K = 32 per product
    const int total6 = ((129 * ch + 31) / 32) * 9 * 64 * 8;
    hipLaunchKernelGGL(x6::pack_final_x6_dev, dim3((total6 + 255) / 256), dim3(256), 0, st, w, ch, reinterpret_cast<unsigned short*>(pack));
    const dim3 grid6((frames + chain::kFinFrames - 1) / chain::kFinFrames);
#define X(CH)                                                                                                                      \
  if (ch == CH)                                                                                                                    \
    hipLaunchKernelGGL((x6::final_gemm_x6_kernel<CH>), grid6, dim3(chain::kFinThreads), 0, st, h,                                  \
                       (const unsigned short*)reinterpret_cast<unsigned short*>(pack), 0.f, y, frames, bias);
    RCED_FIN_CH(X)
#undef X
    return 1;
  }
  const int total = (int)fin_pack_floats(ch);
  hipLaunchKernelGGL(tmm::pack_final_fwd, dim3((total + 255) / 256), dim3(256), 0, st, w, ch, pack);
  const dim3 grid((frames + tmm::kFinFrames - 1) / tmm::kFinFrames);
  // the inference path's output-layer GEMM with its B operand staged through LDS (kernels_fused_chain.h: 0.54 -> 0.41 ms at
  // config 5's size against tmm::final_fwd's strided global reads); same packed A fragments, the bias read on the device
#define X(CH)                                                                                                               \
  if (ch == CH) {                                                                                                           \
    static_assert(tmm::FinGeo<CH>::kPack == chain::FinalGeo<CH>::kPack && tmm::kFinFrames == chain::kFinFrames, "one pack");   \
    hipLaunchKernelGGL((chain::final_gemm_lds_kernel<CH>), grid, dim3(chain::kFinThreads), 0, st, h, (const float*)pack, 0.f,  \
                       y, frames, bias);                                                                                    \
  }
  RCED_FIN_CH(X)
#undef X
  return 1;
}
size_t fin_dgrad_pack_floats(int ch) {   // the fp32 pack, or the three-part bf16 pack of x6::final_dgrad_x6_kernel
  const size_t mt = (size_t)((129 * ch + 15) / 16);
  return std::max(mt * tmm::kDgSteps * 64, (mt * x6::kDgX6Steps * 3 * 64 * 8 * sizeof(unsigned short) + 3) / 4);
}
int fin_dgrad(int ch, const float* dz, const float* w, float* pack, float* dx, int frames, hipStream_t st, bool use_x6) {
  if (use_x6) {
    const int total6 = ((129 * ch + 15) / 16) * x6::kDgX6Steps * 64 * 8;
    hipLaunchKernelGGL(x6::pack_dgrad_x6_dev, dim3((total6 + 255) / 256), dim3(256), 0, st, w, ch, reinterpret_cast<unsigned short*>(pack));
    const dim3 grid6((frames + x6::kDgX6Frames - 1) / x6::kDgX6Frames);
#define X(CH) \
  if (ch == CH) hipLaunchKernelGGL((x6::final_dgrad_x6_kernel<CH>), grid6, dim3(x6::kDgX6Threads), 0, st, dz, (const unsigned short*)reinterpret_cast<unsigned short*>(pack), dx, frames);
    RCED_FIN_CH(X)
#undef X
    return 1;
  }
  const int total = (int)(((129 * ch + 15) / 16) * tmm::kDgSteps * 64);
  hipLaunchKernelGGL(tmm::pack_final_dgrad, dim3((total + 255) / 256), dim3(256), 0, st, w, ch, pack);
  const dim3 grid((frames + tmm::kDgFrames - 1) / tmm::kDgFrames);
#define X(CH) \
  if (ch == CH) hipLaunchKernelGGL((tmm::final_dgrad<CH>), grid, dim3(tmm::kThreads), 0, st, dz, (const float*)pack, dx, frames);
  RCED_FIN_CH(X)
#undef X
  return 1;
}
int fin_wgrad(const WgDet& wd, int ch, const float* x, const float* dz, float* dW, float* dbias, int frames, const Cus& cus, hipStream_t st) {
  const dim3 grid(cus.grid((frames + tmm::kWaves - 1) / tmm::kWaves, cus.n * 2));   // (units: rounds of kWaves frames, one per wave)
#define X(CH)                                                                                                              \
  if (ch == CH)                                                                                                            \
    rced::tmd::wg_launch(wd, [&](float* dw, float* db, unsigned ps) {                                                      \
      hipLaunchKernelGGL((tmm::final_wgrad<CH>), grid, dim3(tmm::kThreads), 0, st, x, dz, dw, db, frames, ps);             \
    }, (int)grid.x, 129 * CH, 1, dW, dbias, st);
  RCED_FIN_CH(X)
#undef X
  return 1;
}
}  // namespace
}  // namespace rced
