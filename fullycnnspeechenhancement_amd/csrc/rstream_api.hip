// C ABI of the resampler lanes (include/rced.h, "streaming resampler" section): host side.  One launch per push on the
// caller's stream (kernels_rstream.h), no allocation, no synchronisation; the arithmetic of a lane stream is rstream_plan.h's.
// Below them the free-running lanes ("free-running resampler" section): kernels_rfree.h and rfree_plan.h.  Both
// handles are an rced_lanes (format, device, table, state) with the family's plan; open, destroy and reset are written once, for that base.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/rced.h"
#include "kernels_rfree.h"
#include "kernels_rstream.h"
#include "rced_internal.h"

using namespace rced;

struct rced_lanes {
  int sr_in = 0, sr_out = 0, channels = 1, src_dtype = 0, out_dtype = 0, lanes = 0, device = 0;
  int words = 0;                   // 8-byte words of state per lane: the plan's
  const double* table = nullptr;   // the ratio's, on the device: resample_api.hip owns it
  long long* state = nullptr;      // [lanes][words]
  hipStream_t last = nullptr;      // the stream of the latest push / finish: a reset is ordered on it
};

struct rced_rstream : rced_lanes {
  rstream::Plan plan;
};
struct rced_rfree : rced_lanes {
  rfree::Plan plan;
};

namespace {

// the refusals of a format that need no device, and the ratio's table geometry
int check_format(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int* p, int* q, int* left, int* width) {
  if (int rc = check_rates(sr_in, sr_out)) return rc;
  if (int rc = check_channels(channels)) return rc;
  if (int rc = check_pcm_dtypes(src_dtype, out_dtype)) return rc;
  return rced_resample_table(sr_in, sr_out, p, q, left, width, 0, nullptr);
}

// A handle of family H (`what` lanes) with a plan made: the device, the table on it, the state allocated and zeroed; nothing is left
// behind on a failure.
template <class H, class Plan>
int open_lanes(const rced_lanes& format, const Plan& plan, const char* what, H** out) {
  OnDevice on(format.device, kMaxDevices);
  if (on.rc) return on.rc;
  H* h = new (std::nothrow) H();
  if (!h) return rced_fail(RCED_ERR_ALLOC, "host allocation failed");
  static_cast<rced_lanes&>(*h) = format;
  h->plan = plan;
  h->words = plan.words;
  int p, q, left, width;
  int rc = rced_resample_table(h->sr_in, h->sr_out, &p, &q, &left, &width, h->device, &h->table);
  const size_t bytes = (size_t)h->lanes * h->words * sizeof(long long);
  if (!rc) {
    const hipError_t e = hipMalloc(&h->state, bytes);
    if (e != hipSuccess) rc = rced_fail(e == hipErrorOutOfMemory ? RCED_ERR_ALLOC : RCED_ERR_HIP, "hipMalloc(%s lanes): %s", what, hipGetErrorString(e));
  }
  if (!rc && hipMemset(h->state, 0, bytes) != hipSuccess) rc = rced_fail(RCED_ERR_HIP, "hipMemset(%s lane state)", what);
  if (rc) {
    (void)hipFree(h->state);
    delete h;
    return rc;
  }
  *out = h;
  return RCED_OK;
}

template <class H>
void destroy(H* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipDeviceSynchronize();   // launches that still use the state
  (void)hipFree(h->state);
  delete h;
}

rced_lanes format_of(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int lanes, int device) {
  rced_lanes f;
  f.sr_in = sr_in;
  f.sr_out = sr_out;
  f.channels = channels;
  f.src_dtype = src_dtype;
  f.out_dtype = out_dtype;
  f.lanes = lanes;
  f.device = device;
  return f;
}

// one workgroup a lane: kernel(sf, of) launches the family's kernel for the handle's two PCM types on `st` and returns the launch's code
template <class Kernel>
int launch_lanes(rced_lanes* h, hipStream_t st, Kernel kernel) {
  if (int rc = with_pcm_types(h->src_dtype, h->out_dtype, kernel)) return rc;
  h->last = st;
  return RCED_OK;
}

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
  return launch_lanes(h, st, [&](auto sf, auto of) -> int {
    LAUNCH((rstream::rstream_kernel<decltype(sf)::value, decltype(of)::value>), dim3(h->lanes), dim3(rstream::kThreads), 0, st, P);
    return RCED_OK;
  });
}

// the checks and the plan of free-running lanes that need no device
int plan_for(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int lanes, int max_frames, int max_take, int prefill,
             rfree::Plan* plan) {
  int p, q, left, width;
  if (int rc = check_format(sr_in, sr_out, channels, src_dtype, out_dtype, &p, &q, &left, &width)) return rc;
  char err[256] = "";
  if (rfree::plan(p, q, left, width, max_frames, max_take, prefill, out_dtype == RCED_PCM_F32 ? 4 : 2, lanes, plan, err, sizeof err) !=
      rfree::kPlanOk)
    return rced_fail(RCED_ERR_ARG, "free-running lanes %d Hz -> %d Hz: %s", sr_in, sr_out, err);
  return RCED_OK;
}

int launch(rced_rfree* h, const void* in, int in_cols, const int* counts, const int* take, int finish, void* out, int out_cols, int* out_counts,
           hipStream_t st) {
  const rfree::Plan& L = h->plan;
  rfree::Params P;
  P.in = in;
  P.in_cols = in_cols;
  P.channels = h->channels;
  P.counts = counts;
  P.take = take;
  P.finish = finish;
  P.state = h->state;
  P.words = L.words;
  P.hist = L.hist;
  P.cap = L.cap;
  P.prefill = L.prefill;
  P.table = h->table;
  P.p = L.p;
  P.q = L.q;
  P.left = L.left;
  P.width = L.width;
  P.right = L.right;
  P.ratio = (double)h->sr_out / (double)h->sr_in;
  P.tile = L.tile;
  P.out = out;
  P.out_cols = out_cols;
  P.out_counts = out_counts;
  return launch_lanes(h, st, [&](auto sf, auto of) -> int {
    LAUNCH((rfree::rfree_kernel<decltype(sf)::value, decltype(of)::value>), dim3(h->lanes), dim3(rfree::kThreads), 0, st, P);
    return RCED_OK;
  });
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
  // the ratio and the plan need no device: a refusal comes before one is looked for
  int p, q, left, width;
  if (int rc = check_format(sr_in, sr_out, channels, src_dtype, out_dtype, &p, &q, &left, &width)) return rc;
  rstream::Plan plan;
  char err[256] = "";
  if (rstream::plan(p, q, left, width, unit_in, unit_out, max_units, lanes, delay, &plan, err, sizeof err) != rstream::kPlanOk)
    return rced_fail(RCED_ERR_ARG, "resampler lanes %d Hz -> %d Hz: %s", sr_in, sr_out, err);
  return open_lanes(format_of(sr_in, sr_out, channels, src_dtype, out_dtype, lanes, device), plan, "resampler", out);
}

void rced_rstream_destroy(rced_rstream* h) { destroy(h); }

int rced_rstream_delay(const rced_rstream* h) { return h ? h->plan.delay : -1; }

int rced_rstream_push(rced_rstream* h, const void* pcm_dev, const int* active_dev, int K, void* out_dev, void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (K < 1 || K > h->plan.max_units) return rced_fail(RCED_ERR_ARG, "K must be 1..max_units = %d, got %d", h->plan.max_units, K);
  if (!pcm_dev || !out_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  ON_DEVICE(h->device);
  return launch(h, pcm_dev, K * h->plan.unit_in, active_dev, 0, K, out_dev, K * h->plan.unit_out, nullptr, static_cast<hipStream_t>(stream));
}

int rced_rstream_finish(rced_rstream* h, const void* tail_dev, const int* tail_counts_dev, void* out_dev, int* out_counts_dev, void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (!tail_dev || !tail_counts_dev || !out_dev || !out_counts_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  ON_DEVICE(h->device);
  return launch(h, tail_dev, h->plan.unit_in, tail_counts_dev, 1, 0, out_dev, h->plan.finish_max, out_counts_dev, static_cast<hipStream_t>(stream));
}

int rced_rstream_started(rced_rstream* h, const int* active_dev, int* started_dev, void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (!started_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  ON_DEVICE(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(rstream::started_kernel, dim3((h->lanes + 255) / 256), dim3(256), 0, st, (const long long*)h->state, h->words, active_dev, h->lanes, started_dev);
  h->last = st;
  return RCED_OK;
}

int rced_rstream_reset(rced_rstream* h, int lane) {
  if (!h) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  return reset_lanes(h->state, h->words, h->lanes, lane, h->device, h->last);
}

// ---- free-running lanes ----

long long rced_rfree_available(int sr_in, int sr_out, long long frames) {
  if (sr_in <= 0 || sr_out <= 0 || frames < 0) {
    rced_fail(RCED_ERR_ARG, "rates must be positive and frames >= 0, got %d -> %d, %lld frames", sr_in, sr_out, frames);
    return -1;
  }
  int p, q, left, width;
  if (rced_resample_table(sr_in, sr_out, &p, &q, &left, &width, 0, nullptr)) return -1;
  if (frames > ((long long)1 << 62) / p) {
    rced_fail(RCED_ERR_ARG, "%lld frames at %d / %d: the count does not fit 64 bits", frames, p, q);
    return -1;
  }
  return rfree::emitted(frames, p, q, width - 1 - left);
}

int rced_rfree_plan(int sr_in, int sr_out, int out_dtype, int lanes, int max_frames, int max_take, int prefill, int* history, int* tile,
                    int* capacity, int* finish_max) {
  rfree::Plan plan;
  if (int rc = plan_for(sr_in, sr_out, 1, RCED_PCM_F32, out_dtype, lanes, max_frames, max_take, prefill, &plan)) return rc;
  if (history) *history = plan.hist;
  if (tile) *tile = plan.tile;
  if (capacity) *capacity = plan.cap;
  if (finish_max) *finish_max = plan.finish_max;
  return RCED_OK;
}

int rced_rfree_create(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int lanes, int max_frames, int max_take, int prefill,
                      int device, rced_rfree** out) {
  if (!out) return rced_fail(RCED_ERR_ARG, "out is NULL");
  *out = nullptr;
  // the ratio and the plan need no device: a refusal comes before one is looked for
  rfree::Plan plan;
  if (int rc = plan_for(sr_in, sr_out, channels, src_dtype, out_dtype, lanes, max_frames, max_take, prefill, &plan)) return rc;
  return open_lanes(format_of(sr_in, sr_out, channels, src_dtype, out_dtype, lanes, device), plan, "free-running", out);
}

void rced_rfree_destroy(rced_rfree* h) { destroy(h); }

int rced_rfree_push(rced_rfree* h, const void* pcm_dev, int in_cols, const int* counts_dev, void* out_dev, int out_cols, const int* take_dev,
                    void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "lanes are NULL");
  if (in_cols < 0 || in_cols > h->plan.max_in) return rced_fail(RCED_ERR_ARG, "in_cols must be 0..max_frames = %d, got %d", h->plan.max_in, in_cols);
  if (out_cols < 0 || out_cols > h->plan.max_take)
    return rced_fail(RCED_ERR_ARG, "out_cols must be 0..max_take = %d, got %d", h->plan.max_take, out_cols);
  if ((in_cols && !pcm_dev) || (out_cols && !out_dev)) return rced_fail(RCED_ERR_ARG, "null pointer");
  ON_DEVICE(h->device);
  return launch(h, pcm_dev, in_cols, counts_dev, take_dev, 0, out_dev, out_cols, nullptr, static_cast<hipStream_t>(stream));
}

int rced_rfree_finish(rced_rfree* h, const void* tail_dev, int in_cols, const int* tail_counts_dev, void* out_dev, int* out_counts_dev,
                      void* stream) {
  if (!h) return rced_fail(RCED_ERR_ARG, "lanes are NULL");
  if (in_cols < 0 || in_cols > h->plan.max_in) return rced_fail(RCED_ERR_ARG, "in_cols must be 0..max_frames = %d, got %d", h->plan.max_in, in_cols);
  if ((in_cols && !tail_dev) || !tail_counts_dev || !out_dev || !out_counts_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  ON_DEVICE(h->device);
  return launch(h, tail_dev, in_cols, tail_counts_dev, nullptr, 1, out_dev, h->plan.finish_max, out_counts_dev, static_cast<hipStream_t>(stream));
}

int rced_rfree_reset(rced_rfree* h, int lane) {
  if (!h) return rced_fail(RCED_ERR_ARG, "lanes are NULL");
  return reset_lanes(h->state, h->words, h->lanes, lane, h->device, h->last);
}

}  // extern "C"
