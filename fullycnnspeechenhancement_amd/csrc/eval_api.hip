// C ABI of the evaluation loop's device pieces (include/rced.h, "evaluation" section): host side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>

#include "../../include/rced.h"
#include "kernels_eval.h"
#include "rced_internal.h"

using namespace rced;

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return rced_fail(e_ == hipErrorOutOfMemory ? RCED_ERR_ALLOC : RCED_ERR_HIP, "%s: %s", #expr, \
                       hipGetErrorString(e_));                                                 \
  } while (0)

namespace {

constexpr int kMaxDevices = 16;
// Slice partials [N, slices, 2] double, one buffer per (device, stream): launches on one stream are ordered, so the buffer
// of a stream is never shared by two calls in flight.  It only grows; a call whose shape fits allocates nothing, so the
// entries can be stream-captured after one warm-up call of the shape.
struct Workspace {
  double* p = nullptr;
  size_t bytes = 0;
};
std::map<void*, Workspace> g_ws[kMaxDevices];
std::mutex g_mu;

int check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return rced_fail(RCED_ERR_HIP, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= n || device >= kMaxDevices) return rced_fail(RCED_ERR_ARG, "device %d out of range", device);
  return RCED_OK;
}

int workspace(int device, void* stream, size_t bytes, double** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  Workspace& w = g_ws[device][stream];
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

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; return; }
    ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

extern "C" {

int rced_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
             double* sdr_dev, double* energies_dev, int device, void* stream) {
  if (N < 0 || ref_stride < 0 || est_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!ref_dev || !est_dev || !sdr_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  const int cap = ref_stride < est_stride ? ref_stride : est_stride;
  if (cap > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0) return RCED_OK;
  if (int rc = check_device(device)) return rc;
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
  if (int rc = check_device(device)) return rc;
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

}  // extern "C"
