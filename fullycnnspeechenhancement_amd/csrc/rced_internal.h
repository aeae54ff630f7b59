// Internal model object shared by the C ABI (rced_api.hip) and the fused-kernel runtime.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "host_util.h"
#include "rced_spec.h"

// kernel kinds for the built-in HIP-event profiler ("profile" option)
enum {
  RCED_K_GENERIC = 0,   // conv_layer_generic (layerwise path)
  RCED_K_FUSED = 1,     // fused multi-layer MFMA kernel (the dominant kernel)
  RCED_K_FINAL = 2,     // final 1x129 layer as a Toeplitz GEMM
  RCED_K_COUNT = 3
};

struct rced_layer_dev {
  int cin = 0, cout4 = 0;
  float* w = nullptr;      // [kh,kw,cin,cout4] BN-folded, device
  float* shift = nullptr;  // [cout4] device
  std::vector<float> host_w, host_shift;  // the same, host copies (fused packers read these)
};

struct rced_fused;  // opaque: kernels_fused.hip

struct rced_model {
  int variant = 0, device = 0, num_cus = 0;
  const rced::NetSpec* net = nullptr;
  std::vector<float> host_blob;
  std::vector<rced_layer_dev> layers;
  // layerwise path
  std::vector<int> slot_of_tensor, slot_ch_offset;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  // rced_forward_host staging
  void *stage_x = nullptr, *stage_y = nullptr;
  size_t stage_bytes = 0;
  hipStream_t host_streams[3] = {nullptr, nullptr, nullptr};   // rced_forward_host: upload, compute, download
  std::vector<hipEvent_t> host_events;                         // its per-chunk events (upload done / compute done), reused
  int host_chunks = 0;                                         // option "host_chunks" (0 = default 8)
  // options
  int path = 0;
  bool profile = false;
  rced_fused* fused = nullptr;
  // profiler
  struct ProfEvent { int kind; hipEvent_t start, stop; };
  std::vector<ProfEvent> prof_events;
  void prof_begin(int kind, hipStream_t st);
  void prof_end(int kind, hipStream_t st);
  void prof_reset();
  float prof_dominant_ms(int* kind_out, int* launches_out);
  ~rced_model();
};

// fused-kernel runtime (kernels_fused.hip).  fused_create leaves m->fused null when the
// variant has no fused implementation; all return RCED_* codes and set the thread error.
int fused_create(rced_model* m);
void fused_destroy(rced_model* m);
int fused_reserve(rced_model* m, int N, int T);
int fused_forward(rced_model* m, const float* x, float* y, int N, int T, hipStream_t st);
int fused_check(rced_model* m);   // RCED_ERR_STATE if an earlier launch recorded a hand-off time-out
#define RCED_OPT_UNKNOWN (-1)   // fused_set_option: "not a key of mine" (internal; never crosses the C ABI)
int fused_set_option(rced_model* m, const char* key, int value);
int fused_get_option(rced_model* m, const char* key, int* value);

// the device's three-part bf16 STFT / ISTFT tables (audio_api.hip builds them once per device), for the streaming kernels
struct rced_audio_x6_tables {
  const unsigned short* stft = nullptr;    // audio::x6::kStftPackX
  const unsigned short* istft = nullptr;   // audio::x6::kIstftPackX, of the nfft asked for
  const float* cim = nullptr;              // [128]
  const float* chead = nullptr;            // [258][128]
  const unsigned short* ola = nullptr;     // audio::x6::kOlaPackX: the overlap-add rebuild's 16 M-tiles (no nfft)
  const float* ola_fix = nullptr;          // [2][128]: its single-frame factors
};
int rced_audio_x6_tables_get(int device, int nfft, rced_audio_x6_tables* out);

// the packs of a framing (audio_api.hip's per-device cache, kernels_framing.h), for the streaming kernels at a framing: the STFT pack,
// the rebuild's (overlap-add, or the reference rebuild at nfft 256 / 512) and its two fp32 tables.  Pinned: they stay until
// rced_fr_tables_unpin with the same arguments, whatever else the cache drops.
struct rced_fr_tables {
  const unsigned short* stft = nullptr;      // audio::fr::kFrPack
  const unsigned short* rebuild = nullptr;   // audio::fr::kFrPack
  const float* cim = nullptr;                // [256]: the coefficients of im(bin 128), row scale folded in (zeros unless nfft = 512)
  const float* w2 = nullptr;                 // [256]: w^2, zero past the window
};
int rced_fr_tables_pin(int device, int window, int window_name, int ola, int nfft, rced_fr_tables* out);
void rced_fr_tables_unpin(int device, int window, int window_name, int ola, int nfft);

// audio_api.hip: rced_wave_loss (rced.h) with one more argument, for the training pass -- accumulate != 0: the gradient is added to
// grad_dev (which then holds the spectral term's, written by an earlier launch on the stream) instead of written
int rced_wave_loss_run(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                       const int* lengths_dev, int N, int T, double w_sse, double w_si_sdr, int skip_edges, double inv_batch,
                       double* terms_dev, float* grad_dev, int accumulate, int device, void* stream);
// ... and rced_wave_loss_fr likewise: the same pass at a framing (W, S, window name), always through the general kernels
int rced_wave_loss_fr_run(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                          const int* lengths_dev, int N, int T, int W, int S, int name, double w_sse, double w_si_sdr, int skip_edges,
                          double inv_batch, double* terms_dev, float* grad_dev, int accumulate, int device, void* stream);
// ... and rced_wave_loss_mr: the same with the multi-resolution STFT term on the rebuilt signal; terms_dev [N, 5]
struct rced_mr_args;
int rced_wave_loss_mr_run(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                          const int* lengths_dev, int N, int T, int W, int S, int name, double w_sse, double w_si_sdr, int skip_edges,
                          double inv_batch, const rced_mr_args* mr, double* terms_dev, float* grad_dev, int accumulate, int device,
                          void* stream);

// stream_api.hip: streams created on `m` answer RCED_ERR_STATE from now on (rced_destroy calls this before the model goes)
void rced_streams_detach(rced_model* m);

// resample_api.hip: the phase table of sr_new / sr_orig (found or built, as rced_resample_taps refuses) and, with table_dev, its
// copy on `device` (uploaded once; the caller has checked the device and made it current), for the resampler lanes
int rced_resample_table(int sr_orig, int sr_new, int* p, int* q, int* left, int* width, int device, const double** table_dev);
