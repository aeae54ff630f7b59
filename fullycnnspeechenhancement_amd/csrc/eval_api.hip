// C ABI of the evaluation loop's device pieces (include/rced.h, "evaluation" section): host side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/rced.h"
#include "kernels_eval.h"
#include "kernels_stoi.h"
#include "rced_internal.h"

using namespace rced;

namespace {

// Slice partials [N, slices, 2] double, one buffer per (device, stream): launches on one stream are ordered, so the buffer
// of a stream is never shared by two calls in flight.  It only grows; a call whose shape fits allocates nothing, so the
// entries can be stream-captured after one warm-up call of the shape.
struct Workspace {
  double* p = nullptr;
  size_t bytes = 0;
};
// STOI, SI-SDR and the segmental SNR keep buffers of their own: none ever moves the one another entry's captured graph reads
enum { kWsSlices = 0, kWsStoi = 1, kWsSiSdr = 2, kWsSegSnr = 3, kWsKinds = 4 };
std::map<void*, Workspace> g_ws[kWsKinds][kMaxDevices];
std::mutex g_mu;

int workspace(int device, void* stream, size_t bytes, double** out, int which = kWsSlices) {
  std::lock_guard<std::mutex> lk(g_mu);
  Workspace& w = g_ws[which][device][stream];
  if (w.bytes < bytes) {
    if (w.p) {
      HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));   // an earlier call may still read it
      (void)hipFree(w.p);
      w = Workspace();
    }
    HIP_TRY(hipMalloc(&w.p, bytes));
    w.bytes = bytes;
  }
  *out = w.p;
  return RCED_OK;
}

// ---- STOI tables: built on the host once per process, uploaded once per device ---------------------------------------------------
struct StoiTables {
  double* tab = nullptr;             // resampler taps [0, 365), first window [368, 624)
  unsigned short* apack = nullptr;   // the windowed DFT matrix, three bf16 parts, MFMA fragment order
};
StoiTables g_stoi[kMaxDevices];
std::mutex g_stoi_mu;

double bessel_i0(double x) {         // power series: converges to the last bit in < 30 terms for x <= 6
  double s = 1.0, t = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 60; ++k) {
    t *= q / ((double)k * k);
    s += t;
    if (t < 1e-18 * s) break;
  }
  return s;
}

// np.hanning(258)[1:-1]
double stoi_window(int k) { return 0.5 - 0.5 * std::cos(2.0 * M_PI * (k + 1) / (stoi::kFrame + 1)); }

// 5 * h / sum(h), h = kaiser(365, 0.1102 (60 - 8.7)) * 2 p fc sinc(2 fc t), p = 5, fc = 1 / 10, t = -182 .. 182
std::vector<double> stoi_taps() {
  const int L = stoi::kTapHalf;
  const double beta = 0.1102 * (60.0 - 8.7), fc = 1.0 / 10.0;
  std::vector<double> h(stoi::kTaps);
  double sum = 0.0;
  for (int i = 0; i < stoi::kTaps; ++i) {
    const double t = i - L, a = t / L;
    const double kaiser = bessel_i0(beta * std::sqrt(1.0 - a * a)) / bessel_i0(beta);
    const double px = M_PI * 2.0 * fc * t;
    const double sinc = t == 0.0 ? 1.0 : std::sin(px) / px;
    h[i] = kaiser * (2.0 * 5.0 * fc * sinc);
    sum += h[i];
  }
  for (double& v : h) v = v / sum * 5.0;
  return h;
}

// row 4 q + {0, 1, 2, 3} = re, im of the first bin of pair slot q, re, im of its second (kernels_stoi.h); k = sample 0 .. 255
double stoi_coef(int row, int k) {
  const int q = row >> 2, second = (row >> 1) & 1, im = row & 1;
  if (q >= stoi::kSlots) return 0.0;
  int band = 0;
  while (stoi::band_slot(band + 1) <= q) ++band;
  const int bin = stoi::band_lo(band) + 2 * (q - stoi::band_slot(band)) + second;
  if (bin >= stoi::band_lo(band + 1)) return 0.0;
  const double th = 2.0 * M_PI * ((bin * k) % 512) / 512.0;
  return stoi_window(k) * (im ? -std::sin(th) : std::cos(th));
}

int stoi_tables(int device, StoiTables** out) {
  std::lock_guard<std::mutex> lk(g_stoi_mu);
  StoiTables& t = g_stoi[device];
  if (!t.tab) {
    std::vector<double> tab(stoi::kTabLen, 0.0);
    const std::vector<double> taps = stoi_taps();
    std::copy(taps.begin(), taps.end(), tab.begin());
    for (int k = 0; k < stoi::kFrame; ++k) tab[stoi::kTabWin + k] = stoi_window(k);
    const std::vector<unsigned short> pack = x6dft::pack_x6(stoi::kMTiles, stoi_coef);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(stoi::band_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                stoi::kBandLdsBytes));
    double* dt = nullptr;
    unsigned short* dp = nullptr;
    if (int rc = upload(&dt, tab, "STOI tables")) return rc;
    if (int rc = upload(&dp, pack, "STOI tables")) {
      (void)hipFree(dt);
      return rc;
    }
    t.apack = dp;
    t.tab = dt;
  }
  *out = &t;
  return RCED_OK;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int rced_stoi_ex(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int fs_sig,
                 int which, double* stoi_dev, double* estoi_dev, int* detail_dev, int device, void* stream) {
  if (N < 0 || ref_stride < 0 || est_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (which <= 0 || (which & ~(RCED_STOI_CLASSIC | RCED_STOI_EXTENDED)))
    return rced_fail(RCED_ERR_ARG, "which must be RCED_STOI_CLASSIC, RCED_STOI_EXTENDED or both, got %d", which);
  const bool classic = which & RCED_STOI_CLASSIC, extended = which & RCED_STOI_EXTENDED;
  if (!ref_dev || !est_dev || (classic && !stoi_dev) || (extended && !estoi_dev)) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (fs_sig != 8000 && fs_sig != stoi::kFs) return rced_fail(RCED_ERR_ARG, "fs_sig must be 8000 or 10000, got %d", fs_sig);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  const int cap = ref_stride < est_stride ? ref_stride : est_stride;
  if (cap > stoi::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^28 samples");
  if (N == 0) return RCED_OK;
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  StoiTables* t = nullptr;
  if (int rc = stoi_tables(device, &t)) return rc;
  // workspace: r [N][2][rstride] f64 | e [N][fcap] f64 | tob [N][2][fcap][16] f64 | dseg [2][N][mcap] f64 (classic, extended) |
  // kept [N][fcap] i32 | cnt [N][4] i32 -- one layout whatever `which` asks for: a shape's size never depends on it
  const int l10 = stoi::len10k(cap, fs_sig);
  const int fcap = stoi::num_frames(l10) > 0 ? stoi::num_frames(l10) : 1;
  const int mcap = fcap > stoi::kSeg ? fcap - stoi::kSeg : 1;
  const int rstride = (l10 + 1) & ~1;
  const size_t o_r = 0, o_e = o_r + align256((size_t)N * 2 * rstride * 8), o_tob = o_e + align256((size_t)N * fcap * 8),
               o_d = o_tob + align256((size_t)N * 2 * fcap * 16 * 8), o_kept = o_d + 2 * align256((size_t)N * mcap * 8),
               o_cnt = o_kept + align256((size_t)N * fcap * 4), total = o_cnt + align256((size_t)N * 4 * 4);
  double* ws = nullptr;
  if (int rc = workspace(device, stream, total, &ws, kWsStoi)) return rc;
  char* base = reinterpret_cast<char*>(ws);
  double* r = reinterpret_cast<double*>(base + o_r);
  double* e = reinterpret_cast<double*>(base + o_e);
  double* tob = reinterpret_cast<double*>(base + o_tob);
  double* dseg = reinterpret_cast<double*>(base + o_d);
  double* dseg_ext = reinterpret_cast<double*>(base + o_d + align256((size_t)N * mcap * 8));
  int* kept = reinterpret_cast<int*>(base + o_kept);
  int* cnt = reinterpret_cast<int*>(base + o_cnt);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (l10 > 0) {
    hipLaunchKernelGGL(stoi::resample_kernel, dim3((l10 + 255) / 256, 2, N), dim3(256), 0, st, ref_dev, ref_stride, est_dev,
                       est_stride, lengths_dev, cap, fs_sig, (const double*)t->tab, r, rstride);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(stoi::energy_kernel, dim3((fcap + 3) / 4, N), dim3(256), 0, st, (const double*)r, rstride, lengths_dev, cap,
                     fs_sig, (const double*)t->tab, e, fcap);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(stoi::mask_kernel, dim3(N), dim3(64), 0, st, (const double*)e, lengths_dev, cap, fs_sig, fcap, kept, cnt);
  HIP_TRY(hipGetLastError());
  if (fcap - 1 >= stoi::kSeg) {
    hipLaunchKernelGGL(stoi::band_kernel, dim3((fcap - 1 + stoi::kBlockFrames - 1) / stoi::kBlockFrames, 2, N), dim3(stoi::kThreads),
                       stoi::kBandLdsBytes, st, (const double*)r, rstride, (const int*)kept, (const int*)cnt, fcap,
                       (const unsigned short*)t->apack, (const double*)t->tab, tob);
    HIP_TRY(hipGetLastError());
    if (classic) {
      hipLaunchKernelGGL(stoi::segment_kernel, dim3((mcap + 15) / 16, N), dim3(256), 0, st, (const double*)tob, (const int*)cnt, fcap,
                         mcap, 1.0 + std::pow(10.0, 15.0 / 20.0), dseg);
      HIP_TRY(hipGetLastError());
    }
    if (extended) {
      hipLaunchKernelGGL(stoi::segment_ext_kernel, dim3((mcap + 15) / 16, N), dim3(256), 0, st, (const double*)tob, (const int*)cnt,
                         fcap, mcap, dseg_ext);
      HIP_TRY(hipGetLastError());
    }
  }
  if (classic) {
    hipLaunchKernelGGL(stoi::final_kernel, dim3(N), dim3(256), 0, st, (const double*)dseg, (const int*)cnt, mcap, (double)stoi::kBands,
                       stoi_dev, detail_dev);
    HIP_TRY(hipGetLastError());
  }
  if (extended) {
    hipLaunchKernelGGL(stoi::final_kernel, dim3(N), dim3(256), 0, st, (const double*)dseg_ext, (const int*)cnt, mcap, (double)stoi::kSeg,
                       estoi_dev, classic ? nullptr : detail_dev);
    HIP_TRY(hipGetLastError());
  }
  return RCED_OK;
}

int rced_stoi(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int fs_sig,
              double* stoi_dev, int* detail_dev, int device, void* stream) {
  return rced_stoi_ex(ref_dev, ref_stride, est_dev, est_stride, lengths_dev, N, fs_sig, RCED_STOI_CLASSIC, stoi_dev, nullptr, detail_dev,
                      device, stream);
}

int rced_si_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
                double* out_dev, double* parts_dev, int device, void* stream) {
  if (N < 0 || ref_stride < 0 || est_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!ref_dev || !est_dev || !out_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  const int cap = ref_stride < est_stride ? ref_stride : est_stride;
  if (cap > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0) return RCED_OK;
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const int slices = eval::num_slices(cap) > 0 ? eval::num_slices(cap) : 1;
  const size_t pass = (size_t)N * slices * 2;            // doubles per pass: [N, slices, 2]
  double* ws1 = nullptr;
  if (int rc = workspace(device, stream, 2 * pass * sizeof(double), &ws1, kWsSiSdr)) return rc;
  double* ws2 = ws1 + pass;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eval::si_sdr_dot_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride,
                     lengths_dev, cap, ws1, slices);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(eval::si_sdr_energy_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev,
                     est_stride, lengths_dev, cap, (const double*)ws1, ws2, slices);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(eval::si_sdr_final_kernel, dim3(N), dim3(eval::kThreads), 0, st, (const double*)ws1, (const double*)ws2,
                     lengths_dev, cap, slices, out_dev, parts_dev);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

int rced_seg_snr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int fs,
                 double* out_dev, int* frames_dev, int device, void* stream) {
  if (N < 0 || ref_stride < 0 || est_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!ref_dev || !est_dev || !out_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  const int W = fs > 0 ? eval::seg_window(fs) : 0;
  if (W < eval::kSegMinW || W > eval::kSegMaxW)
    return rced_fail(RCED_ERR_ARG, "fs = %d gives frames of %d samples: outside [%d, %d]", fs, W, eval::kSegMinW, eval::kSegMaxW);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  const int cap = ref_stride < est_stride ? ref_stride : est_stride;
  if (cap > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0) return RCED_OK;
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const int nfcap = eval::seg_frames(cap, W) > 0 ? eval::seg_frames(cap, W) : 1;
  const int blocks = (nfcap + eval::kSegFramesPerBlock - 1) / eval::kSegFramesPerBlock;
  double* snr = nullptr;
  if (int rc = workspace(device, stream, (size_t)N * nfcap * sizeof(double), &snr, kWsSegSnr)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eval::seg_snr_frame_kernel, dim3(blocks, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev,
                     est_stride, lengths_dev, cap, W, snr, nfcap);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(eval::seg_snr_mean_kernel, dim3(N), dim3(eval::kThreads), 0, st, (const double*)snr, lengths_dev, cap, W, nfcap,
                     out_dev, frames_dev);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

int rced_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
             double* sdr_dev, double* energies_dev, int device, void* stream) {
  if (N < 0 || ref_stride < 0 || est_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!ref_dev || !est_dev || !sdr_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  const int cap = ref_stride < est_stride ? ref_stride : est_stride;
  if (cap > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0) return RCED_OK;
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const int slices = eval::num_slices(cap) > 0 ? eval::num_slices(cap) : 1;
  double* ws = nullptr;
  if (int rc = workspace(device, stream, (size_t)N * slices * 2 * sizeof(double), &ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eval::sdr_partial_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev,
                     est_stride, lengths_dev, cap, ws, slices);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(eval::sdr_final_kernel, dim3(N), dim3(64), 0, st, (const double*)ws, lengths_dev, cap, slices, sdr_dev,
                     energies_dev);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

int rced_mix_snr(const float* speech_dev, const int* speech_len_dev, int N, int Ls, const float* noise_dev,
                 const int* noise_len_dev, int Ln, const int* start_dev, const double* gains_dev, int n_gains, double snr_db,
                 float* mix_dev, int device, void* stream) {
  if (N < 0 || Ls < 0 || Ln < 0 || n_gains < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!speech_dev || !noise_dev || !mix_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (n_gains > 0 && !gains_dev) return rced_fail(RCED_ERR_ARG, "n_gains = %d without gains", n_gains);
  if (n_gains > 31) return rced_fail(RCED_ERR_ARG, "n_gains > 31: a tile index has at most 31 bits");
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (Ls > eval::kMaxLen || Ln > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0 || Ls == 0) return RCED_OK;
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const int slices = eval::num_slices(Ls);
  double* ws = nullptr;
  if (int rc = workspace(device, stream, (size_t)N * slices * 2 * sizeof(double), &ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eval::mix_partial_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, speech_dev, speech_len_dev, Ls,
                     noise_dev, noise_len_dev, Ln, start_dev, gains_dev, n_gains, ws, slices);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(eval::mix_apply_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, speech_dev, speech_len_dev, Ls,
                     noise_dev, noise_len_dev, Ln, start_dev, gains_dev, n_gains, (const double*)ws, slices,
                     std::pow(10.0, snr_db / 10.0), mix_dev);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

int rced_gather_pcm(const void* arena_dev, int arena_dtype, long long arena_samples, const long long* begin_dev, const int* count_dev,
                    int N, int L, float* rows_dev, int row_stride, int device, void* stream) {
  if (N < 0 || L < 0 || arena_samples < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (arena_dtype != RCED_PCM_S16 && arena_dtype != RCED_PCM_F32)
    return rced_fail(RCED_ERR_ARG, "arena_dtype must be RCED_PCM_S16 or RCED_PCM_F32, got %d", arena_dtype);
  if (row_stride < L) return rced_fail(RCED_ERR_ARG, "row_stride %d < L %d", row_stride, L);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (L > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0 || L == 0) return RCED_OK;
  if (!begin_dev || !count_dev || !rows_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (!arena_dev && arena_samples > 0) return rced_fail(RCED_ERR_ARG, "null arena of %lld samples", arena_samples);
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(eval::num_slices(L), N), block(eval::kThreads);
  static_assert(eval::kSlice == eval::kThreads * eval::kGatherPerLane, "a column block of the gather is one slice");
  if (arena_dtype == RCED_PCM_F32)
    hipLaunchKernelGGL(eval::gather_pcm_kernel<true>, grid, block, 0, st, arena_dev, arena_samples, begin_dev, count_dev, L, rows_dev,
                       row_stride);
  else
    hipLaunchKernelGGL(eval::gather_pcm_kernel<false>, grid, block, 0, st, arena_dev, arena_samples, begin_dev, count_dev, L, rows_dev,
                       row_stride);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

}  // extern "C"
