// C ABI of the resampler lanes (include/rced.h, "streaming resampler" section): host side.  One launch per push on the
// caller's stream (kernels_rstream.h), no allocation, no synchronisation; the arithmetic of a lane stream is rstream_plan.h's.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/rced.h"
#include "kernels_rstream.h"
#include "rced_internal.h"

using namespace rced;

struct rced_rstream {
  rstream::Plan plan;
  int sr_in = 0, sr_out = 0, channels = 1, src_dtype = 0, out_dtype = 0, lanes = 0, device = 0;
  const double* table = nullptr;   // the ratio's, on the device: resample_api.hip owns it
  long long* state = nullptr;      // [lanes][plan.words]
  hipStream_t last = nullptr;      // the stream of the latest push / finish: rced_rstream_reset is ordered on it
};

namespace {

int launch(rced_rstream* h, const void* in, int in_frames, const int* flags, int finish, int K, void* out, int out_cols, int* out_counts,
           hipStream_t st) {
  const rstream::Plan& L = h->plan;
  rstream::Params P;
  P.in = in;
  P.in_frames = in_frames;
  P.channels = h->channels;
  P.flags = flags;
  P.finish = finish;
  P.K = K;
  P.state = h->state;
  P.words = L.words;
  P.hist = L.hist;
  P.table = h->table;
  P.p = L.p;
  P.q = L.q;
  P.left = L.left;
  P.width = L.width;
  P.ratio = (double)h->sr_out / (double)h->sr_in;
  P.unit_in = L.unit_in;
  P.unit_out = L.unit_out;
  P.delay = L.delay;
  P.tile = L.tile;
  P.out = out;
  P.out_cols = out_cols;
  P.out_counts = out_counts;
  const dim3 grid(h->lanes), block(rstream::kThreads);
  const bool sf = h->src_dtype == RCED_PCM_F32, of = h->out_dtype == RCED_PCM_F32;
  if (sf && of)
    hipLaunchKernelGGL((rstream::rstream_kernel<true, true>), grid, block, 0, st, P);
  else if (sf)
    hipLaunchKernelGGL((rstream::rstream_kernel<true, false>), grid, block, 0, st, P);
  else if (of)
    hipLaunchKernelGGL((rstream::rstream_kernel<false, true>), grid, block, 0, st, P);
  else
    hipLaunchKernelGGL((rstream::rstream_kernel<false, false>), grid, block, 0, st, P);
  HIP_TRY(hipGetLastError());
  h->last = st;
  return RCED_OK;
}

}  // namespace

extern "C" {

int rced_rstream_create(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int unit_in, int unit_out, int lanes, int max_units,
                        int device, rced_rstream** out) {
  return rced_rstream_create_ex(sr_in, sr_out, channels, src_dtype, out_dtype, unit_in, unit_out, lanes, max_units, -1, device, out);
}

int rced_rstream_create_ex(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int unit_in, int unit_out, int lanes, int max_units,
                           int delay, int device, rced_rstream** out) {
  if (!out) return rced_fail(RCED_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (sr_in <= 0 || sr_out <= 0) return rced_fail(RCED_ERR_ARG, "sample rates must be positive, got %d -> %d", sr_in, sr_out);
  if (channels < 1) return rced_fail(RCED_ERR_ARG, "channels must be >= 1, got %d", channels);
  if (src_dtype != RCED_PCM_S16 && src_dtype != RCED_PCM_F32)
    return rced_fail(RCED_ERR_ARG, "src_dtype must be RCED_PCM_S16 or RCED_PCM_F32, got %d", src_dtype);
  if (out_dtype != RCED_PCM_S16 && out_dtype != RCED_PCM_F32)
    return rced_fail(RCED_ERR_ARG, "out_dtype must be RCED_PCM_S16 or RCED_PCM_F32, got %d", out_dtype);
  // the ratio and the plan need no device: a refusal comes before one is looked for
  int p, q, left, width;
  if (int rc = rced_resample_table(sr_in, sr_out, &p, &q, &left, &width, 0, nullptr)) return rc;
  rstream::Plan plan;
  char err[256] = "";
  if (rstream::plan(p, q, left, width, unit_in, unit_out, max_units, lanes, delay, &plan, err, sizeof err) != rstream::kPlanOk)
    return rced_fail(RCED_ERR_ARG, "resampler lanes %d Hz -> %d Hz: %s", sr_in, sr_out, err);
  if (int rc = check_device(device, kMaxDevices)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  rced_rstream* h = new (std::nothrow) rced_rstream();
  if (!h) return rced_fail(RCED_ERR_ALLOC, "host allocation failed");
  h->plan = plan;
  h->sr_in = sr_in;
  h->sr_out = sr_out;
  h->channels = channels;
  h->src_dtype = src_dtype;
  h->out_dtype = out_dtype;
  h->lanes = lanes;
  h->device = device;
  int rc = rced_resample_table(sr_in, sr_out, &p, &q, &left, &width, device, &h->table);
  const size_t bytes = (size_t)lanes * plan.words * sizeof(long long);
  if (!rc) {
    const hipError_t e = hipMalloc(&h->state, bytes);
    if (e != hipSuccess) rc = rced_fail(e == hipErrorOutOfMemory ? RCED_ERR_ALLOC : RCED_ERR_HIP, "hipMalloc(resampler lanes): %s", hipGetErrorString(e));
  }
  if (!rc && hipMemset(h->state, 0, bytes) != hipSuccess) rc = rced_fail(RCED_ERR_HIP, "hipMemset(resampler lane state)");
  if (rc) {
    (void)hipFree(h->state);
    delete h;
    return rc;
  }
  *out = h;
  return RCED_OK;
}

void rced_rstream_destroy(rced_rstream* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipDeviceSynchronize();   // launches that still use the state
  (void)hipFree(h->state);
  delete h;
}

int rced_rstream_delay(const rced_rstream* h) { return h ? h->plan.delay : -1; }

int rced_rstream_push(rced_rstream* h, const void* pcm_dev, const int* active_dev, int K, void* out_dev, void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (K < 1 || K > h->plan.max_units) return rced_fail(RCED_ERR_ARG, "K must be 1..max_units = %d, got %d", h->plan.max_units, K);
  if (!pcm_dev || !out_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  DeviceGuard g(h->device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", h->device);
  return launch(h, pcm_dev, K * h->plan.unit_in, active_dev, 0, K, out_dev, K * h->plan.unit_out, nullptr, static_cast<hipStream_t>(stream));
}

int rced_rstream_finish(rced_rstream* h, const void* tail_dev, const int* tail_counts_dev, void* out_dev, int* out_counts_dev, void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (!tail_dev || !tail_counts_dev || !out_dev || !out_counts_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  DeviceGuard g(h->device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", h->device);
  return launch(h, tail_dev, h->plan.unit_in, tail_counts_dev, 1, 0, out_dev, h->plan.finish_max, out_counts_dev, static_cast<hipStream_t>(stream));
}

int rced_rstream_started(rced_rstream* h, const int* active_dev, int* started_dev, void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (!started_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  DeviceGuard g(h->device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rstream::started_kernel, dim3((h->lanes + 255) / 256), dim3(256), 0, st, (const long long*)h->state, h->plan.words, active_dev,
                     h->lanes, started_dev);
  HIP_TRY(hipGetLastError());
  h->last = st;
  return RCED_OK;
}

int rced_rstream_reset(rced_rstream* h, int lane) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (lane < -1 || lane >= h->lanes) return rced_fail(RCED_ERR_ARG, "lane must be -1 (all) or 0..%d, got %d", h->lanes - 1, lane);
  DeviceGuard g(h->device);
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", h->device);
  const size_t one = (size_t)h->plan.words * sizeof(long long);
  if (lane < 0) HIP_TRY(hipMemsetAsync(h->state, 0, one * h->lanes, h->last));
  else HIP_TRY(hipMemsetAsync(h->state + (size_t)lane * h->plan.words, 0, one, h->last));
  return RCED_OK;
}

}  // extern "C"
