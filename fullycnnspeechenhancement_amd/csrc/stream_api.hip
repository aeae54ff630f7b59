// C ABI of the streaming denoiser (include/rced.h, "streaming" section): host side.  Three launches per push on the caller's stream --
// the stateful STFT, rced_forward on the lanes' windows, the stateful ISTFT (kernels_stream.h; for a stream created with
// RCED_STREAM_REBUILD_OLA the overlap-add one, kernels_stream_ola.h) --, no allocation, no synchronisation.  A stream created at a framing
// (rced_stream_create_fr) runs the general kernels instead, four launches per push (kernels_stream_fr.h, planned by stream_fr_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/rced.h"
#include "rced_internal.h"
#include "stream_fr_plan.h"

namespace sfp = ::rced::stream_fr;   // (named before the unnamed namespace below gets an rced of its own)

// kernels_audio.h / kernels_audio_x6.h define their kernels with external linkage and audio_api.hip is their translation unit: this
// one takes the headers into an unnamed namespace, so that its copies (it launches only its own three kernels) are local to it.
// (x6_dft.h comes in with them; what it includes -- <vector>, host_util.h through rced_internal.h -- is already in, at file scope.)
namespace {
#include "kernels_stream.h"
#include "kernels_stream_ola.h"
#include "kernels_stream_fr.h"
namespace audio = rced::audio;
namespace as = rced::audio::stream;
namespace af = rced::audio::stream::fr;
}  // namespace

struct rced_stream {
  rced_model* model = nullptr;   // null once the model was destroyed under the stream
  int device = 0, lanes = 0, max_hops = 0, nfft = 0, rebuild = RCED_STREAM_REBUILD_REFERENCE;
  float* state = nullptr;        // [S, kStFloats]
  float* win = nullptr;          // [S, 7 + K, 129] magnitudes: the CNN's input
  float* phw = nullptr;          // [S, 7 + K, 129, 2]
  float* masks = nullptr;        // [S, 7 + K, 129]: the CNN's output
  hipStream_t last = nullptr;    // the stream of the latest push / finish: rced_stream_reset is ordered on it
  rced_audio_x6_tables tab;
  // a stream at a framing (rced_stream_create_fr): the general kernels, their state layout, their packs (pinned in audio_api.hip's cache)
  bool fr = false, pinned = false;
  int window = 0, stride = 0, window_name = 0;
  float* frames = nullptr;       // [S, window_hops, 256]: the frames between the two steps of the rebuild
  rced_fr_tables ft;
  int state_floats = 0;          // per lane
};

namespace {

std::mutex g_mu;
std::vector<rced_stream*> g_streams;   // the live ones: rced_destroy of a model detaches its streams

int finish_slots(const rced_stream* s) { return s->fr ? sfp::finish_slots(s->window, s->stride) : as::kFinishSlots; }
int window_hops(const rced_stream* s) { return std::max(s->max_hops, finish_slots(s)); }

void release(rced_stream* s) {
  for (void* p : {(void*)s->state, (void*)s->win, (void*)s->phw, (void*)s->masks, (void*)s->frames}) (void)hipFree(p);
  if (s->pinned) rced_fr_tables_unpin(s->device, s->window, s->window_name, s->rebuild == RCED_STREAM_REBUILD_OLA, s->nfft);
  delete s;
}

// the four launches of a stream at a framing; K slots per lane (push: K hops, finish: R + 4)
int run_fr(rced_stream* s, const float* in, const int* flags, int finish, int K, float* out, int* out_counts, hipStream_t st) {
  const int S = s->lanes, W = s->window, hop = s->stride;
  const dim3 grid((S * K + audio::kFramesPerWg - 1) / audio::kFramesPerWg, 2), block(audio::x6::kThreadsX);
  LAUNCH(af::stream_fr_stft_kernel, grid, block, af::kStftLds, st, in, flags, finish, s->ft.stft, (const float*)s->state, S, K, W, hop, s->win, s->phw);
  if (int rc = rced_forward(s->model, s->win, s->masks, S, as::kKeep + K, st)) return rc;
  LAUNCH(af::stream_fr_frames_kernel, grid, block, af::kFramesLds, st, (const float*)s->masks, (const float*)s->phw, flags, finish, s->ft.rebuild,
         s->ft.cim, (const float*)s->state, S, K, window_hops(s), W, hop, s->frames);
  if (s->rebuild == RCED_STREAM_REBUILD_OLA)
    LAUNCH(af::stream_fr_rebuild_kernel<true>, dim3(S), block, 0, st, (const float*)s->frames, s->ft.w2, in, flags, finish, (const float*)s->win,
           (const float*)s->phw, s->state, K, window_hops(s), W, hop, out, out_counts);
  else
    LAUNCH(af::stream_fr_rebuild_kernel<false>, dim3(S), block, 0, st, (const float*)s->frames, s->ft.w2, in, flags, finish, (const float*)s->win,
           (const float*)s->phw, s->state, K, window_hops(s), W, hop, out, out_counts);
  s->last = st;
  return RCED_OK;
}

// the three launches; K slots per lane (push: K hops, finish: kFinishSlots)
int run(rced_stream* s, const float* in, const int* flags, int finish, int K, float* out, int* out_counts, hipStream_t st) {
  if (s->fr) return run_fr(s, in, flags, finish, K, out, out_counts, st);
  const int S = s->lanes;
  LAUNCH(as::stream_stft_kernel, dim3((S * K + audio::kFramesPerWg - 1) / audio::kFramesPerWg, 2), dim3(audio::x6::kThreadsX), as::kStreamStftLds, st,
         in, flags, finish, s->tab.stft, (const float*)s->state, S, K, s->win, s->phw);
  if (int rc = rced_forward(s->model, s->win, s->masks, S, as::kKeep + K, st)) return rc;
  const int lpw = audio::kFramesPerWg / K;
  if (s->rebuild == RCED_STREAM_REBUILD_OLA)
    LAUNCH(as::stream_istft_ola_kernel, dim3((S + lpw - 1) / lpw), dim3(audio::x6::kThreadsX), as::kStreamOlaLds, st, (const float*)s->masks,
           (const float*)s->win, (const float*)s->phw, in, flags, finish, s->tab.ola, s->tab.ola_fix, s->state, S, K, out, out_counts);
  else
    LAUNCH(as::stream_istft_kernel, dim3((S + lpw - 1) / lpw), dim3(audio::x6::kThreadsX), as::kStreamIstftLds, st, (const float*)s->masks,
           (const float*)s->win, (const float*)s->phw, in, flags, finish, s->tab.istft, s->tab.cim, s->tab.chead, s->state, S, K, out, out_counts);
  s->last = st;
  return RCED_OK;
}

int usable(rced_stream* s) {
  if (!s) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  std::lock_guard<std::mutex> lk(g_mu);
  if (!s->model) return rced_fail(RCED_ERR_STATE, "the stream's model has been destroyed");
  return RCED_OK;
}

// what every create entry ends in; fr: at a framing (checked by the caller), the general kernels
int create(rced_model* m, int lanes, int max_hops, int nfft, int rebuild, bool fr, int window, int stride, int window_name, rced_stream** out) {
  static_assert(RCED_STREAM_DELAY == as::kDelayHops * audio::kStep && RCED_STREAM_FINISH_MAX == as::kFinishOut, "rced.h and kernels_stream.h");
  if (!out) return rced_fail(RCED_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (lanes < 1 || lanes > 65536) return rced_fail(RCED_ERR_ARG, "lanes must be 1..65536, got %d", lanes);
  if (max_hops < 1 || max_hops > as::kMaxHops) return rced_fail(RCED_ERR_ARG, "max_hops must be 1..%d, got %d", as::kMaxHops, max_hops);
  if (nfft != 512 && nfft != 256) return rced_fail(RCED_ERR_ARG, "nfft must be 512 (reference default) or 256");
  if (rebuild != RCED_STREAM_REBUILD_REFERENCE && rebuild != RCED_STREAM_REBUILD_OLA)
    return rced_fail(RCED_ERR_ARG, "rebuild must be RCED_STREAM_REBUILD_REFERENCE (0) or RCED_STREAM_REBUILD_OLA (1), got %d", rebuild);
  if (!m) return rced_fail(RCED_ERR_ARG, "model is NULL");
  ON_DEVICE(m->device);
  rced_stream* s = new (std::nothrow) rced_stream();
  if (!s) return rced_fail(RCED_ERR_ALLOC, "host allocation failed");
  s->model = m;
  s->device = m->device;
  s->lanes = lanes;
  s->max_hops = max_hops;
  s->nfft = nfft;
  s->rebuild = rebuild;
  s->fr = fr;
  s->window = window;
  s->stride = stride;
  s->window_name = window_name;
  s->state_floats = fr ? sfp::kStFloats : as::kStFloats;
  int rc = fr ? rced_fr_tables_pin(m->device, window, window_name, rebuild == RCED_STREAM_REBUILD_OLA, nfft, &s->ft)
              : rced_audio_x6_tables_get(m->device, nfft, &s->tab);
  s->pinned = fr && !rc;
  const size_t rows = (size_t)lanes * (as::kKeep + window_hops(s)) * audio::kBins;
  auto alloc = [&](float** p, size_t floats) {
    if (rc) return;
    const hipError_t e = hipMalloc(p, floats * sizeof(float));
    if (e != hipSuccess) rc = rced_fail(e == hipErrorOutOfMemory ? RCED_ERR_ALLOC : RCED_ERR_HIP, "hipMalloc(stream): %s", hipGetErrorString(e));
  };
  alloc(&s->state, (size_t)lanes * s->state_floats);
  alloc(&s->win, rows);
  alloc(&s->phw, 2 * rows);
  alloc(&s->masks, rows);
  if (fr) alloc(&s->frames, (size_t)lanes * window_hops(s) * audio::kFrame);
  if (!rc && hipMemset(s->state, 0, (size_t)lanes * s->state_floats * sizeof(float)) != hipSuccess) rc = rced_fail(RCED_ERR_HIP, "hipMemset(stream state)");
  if (!rc && fr)
    rc = set_dynamic_lds({{kernel_ptr(af::stream_fr_stft_kernel), af::kStftLds}, {kernel_ptr(af::stream_fr_frames_kernel), af::kFramesLds}}, "stream LDS");
  else if (!rc)
    rc = set_dynamic_lds({{kernel_ptr(as::stream_stft_kernel), as::kStreamStftLds}, {kernel_ptr(as::stream_istft_kernel), as::kStreamIstftLds},
                          {kernel_ptr(as::stream_istft_ola_kernel), as::kStreamOlaLds}}, "stream LDS");
  if (!rc) rc = rced_reserve(m, lanes, as::kKeep + window_hops(s));   // the forward of a push allocates nothing
  if (rc) {
    release(s);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_streams.push_back(s);
  }
  *out = s;
  return RCED_OK;
}

}  // namespace

void rced_streams_detach(rced_model* m) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (rced_stream* s : g_streams)
    if (s->model == m) s->model = nullptr;
}

extern "C" {

int rced_stream_delay(void) { return RCED_STREAM_DELAY; }

int rced_stream_create(rced_model* m, int lanes, int max_hops, int nfft, rced_stream** out) {
  return rced_stream_create_ex(m, lanes, max_hops, nfft, RCED_STREAM_REBUILD_REFERENCE, out);
}

int rced_stream_create_ex(rced_model* m, int lanes, int max_hops, int nfft, int rebuild, rced_stream** out) {
  return create(m, lanes, max_hops, nfft, rebuild, false, 0, 0, 0, out);
}

int rced_stream_fr_check(int window, int stride, int window_name, int rebuild) {
  char err[512];
  if (sfp::check(window, stride, window_name, rebuild, err, sizeof err)) return rced_fail(RCED_ERR_ARG, "%s", err);
  return RCED_OK;
}

int rced_stream_delay_fr(int window, int stride) {
  char err[512];
  if (sfp::check(window, stride, RCED_WINDOW_HAMMING, RCED_STREAM_REBUILD_OLA, err, sizeof err)) return -1;
  return sfp::delay(window, stride);
}

int rced_stream_finish_max_fr(int window, int stride) {
  char err[512];
  if (sfp::check(window, stride, RCED_WINDOW_HAMMING, RCED_STREAM_REBUILD_OLA, err, sizeof err)) return -1;
  return sfp::finish_max(window, stride);
}

int rced_stream_create_fr(rced_model* m, int lanes, int max_hops, int nfft, int rebuild, int window, int stride, int window_name,
                          rced_stream** out) {
  if (!out) return rced_fail(RCED_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (int rc = rced_stream_fr_check(window, stride, window_name, rebuild)) return rc;
  return create(m, lanes, max_hops, nfft, rebuild, true, window, stride, window_name, out);
}

void rced_stream_destroy(rced_stream* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_streams.erase(std::remove(g_streams.begin(), g_streams.end(), s), g_streams.end());
  }
  DeviceGuard g(s->device);
  (void)hipDeviceSynchronize();   // launches that still read the buffers
  release(s);
}

int rced_stream_push(rced_stream* s, const float* pcm_dev, const int* active_dev, int K, float* out_dev, void* stream) {
  if (!s) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (K < 1 || K > s->max_hops) return rced_fail(RCED_ERR_ARG, "K must be 1..max_hops = %d, got %d", s->max_hops, K);
  if (!pcm_dev || !out_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (int rc = usable(s)) return rc;
  ON_DEVICE(s->device);
  return run(s, pcm_dev, active_dev, 0, K, out_dev, nullptr, static_cast<hipStream_t>(stream));
}

int rced_stream_finish(rced_stream* s, const float* tail_dev, const int* tail_counts_dev, float* out_dev, int* out_counts_dev, void* stream) {
  if (!s) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  if (!tail_dev || !tail_counts_dev || !out_dev || !out_counts_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (int rc = usable(s)) return rc;
  ON_DEVICE(s->device);
  return run(s, tail_dev, tail_counts_dev, 1, finish_slots(s), out_dev, out_counts_dev, static_cast<hipStream_t>(stream));
}

int rced_stream_reset(rced_stream* s, int lane) {
  if (!s) return rced_fail(RCED_ERR_ARG, "stream is NULL");
  return reset_lanes(s->state, (size_t)s->state_floats, s->lanes, lane, s->device, s->last);
}

}  // extern "C"
