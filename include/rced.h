/*
 * rced.h -- C ABI of the MI355X-native R-CED / CR-CED forward pass (librced_hip.so).
 *
 * This is the drop-in boundary for the one hot path of phecda-xu/FullyCNNSpeechEnhancement:
 * what the reference runs as `sess.run(self.pred, {self.input_x: x})`
 *   (model_utils/tester.py:85-90, infer.py:62-65, model_utils/trainer.py:245-250)
 * over the graph built by `self.pred = self.model(self.input_x)`
 *   (model_utils/tester.py:69-83; model_utils/model.py:6-96; model_utils/module.py:11-34).
 *
 * Plain C types only; integer status codes; caller-owned buffers; no exceptions cross the
 * boundary.  A model handle is NOT thread-safe (one stream per call, like the reference's
 * single tf.Session).  There is no CPU fallback: every entry point that computes needs a
 * gfx950 device and fails with RCED_ERR_HIP otherwise.
 *
 * Tensor layout (module.py:15, data_loader.py:206-208): NHWC float32,
 *   x, y : [N, T, 129, 1]   N utterances, T time frames, 129 frequency bins.
 *
 * Weight blob (float32), per layer in graph order -- exactly the TF variables of
 * module.py:27,29, raw (BatchNorm is folded inside rced_create, not by the caller):
 *   "{scope}/kernel"                      [kh, kw, cin, cout]  (HWIO)
 *   "{scope}/bias"                        [cout]
 *   "{scope}/batch_norm/gamma"            [cout]   } only for layers with use_norm
 *   "{scope}/batch_norm/beta"             [cout]   }
 *   "{scope}/batch_norm/moving_mean"      [cout]   }
 *   "{scope}/batch_norm/moving_variance"  [cout]   }
 */
#ifndef RCED_H_
#define RCED_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCED_FEATURE_DIM 129 /* cfg [data] feature_dim (Work/.../fully_cnn_*.cfg) */

/* net_work selection of infer.py:45-51 / tester.py:76-82 */
#define RCED_V1 1 /* FullyCNNSEModel    R-CED 10 layers  model.py:6-29  */
#define RCED_V2 2 /* FullyCNNSEModelV2  R-CED 16 layers  model.py:32-61 */
#define RCED_V3 3 /* FullyCNNSEModelV3  CR-CED 16 layers model.py:64-96 */

/* status codes */
#define RCED_OK 0
#define RCED_ERR_ARG 1    /* bad argument (shape, null pointer, unknown variant)  */
#define RCED_ERR_HIP 2    /* HIP runtime error or no gfx950 device                */
#define RCED_ERR_ALLOC 3  /* device or host allocation failed                     */
#define RCED_ERR_STATE 4  /* handle used after destroy / wrong device             */

/* execution paths (rced_set_option "path") */
#define RCED_PATH_AUTO 0      /* fused kernels where available, else layerwise      */
#define RCED_PATH_LAYERWISE 1 /* one generic direct-conv launch per layer           */
#define RCED_PATH_FUSED 2     /* fused multi-layer MFMA kernels; error if unavailable */

typedef struct rced_model rced_model;

/* Topology queries (host only; no device needed).  Replace reading model.py by hand. */
int rced_num_layers(int variant);                 /* 10 / 16 / 16, or -1 */
size_t rced_num_weights(int variant);             /* blob length in floats, or 0 */
size_t rced_num_trainable(int variant);           /* 32765 / 32192 / 32653 (readme.md:65-67) */
/* Layer i of `variant`: out[0..8] = cout,kh,kw,use_norm,use_act,src,skip_pre,skip_post,cin.
 * src/skip ids: 0 = network input, k+1 = output of layer k, -1 = none. */
int rced_layer_desc(int variant, int layer, int out[9]);
const char* rced_layer_scope(int variant, int layer); /* TF variable scope, e.g. "CE1_encode_1" */

/* Model(is_training=False) + Saver.restore: tester.py:69-83, 36-39.
 * blob: host pointer, n_floats == rced_num_weights(variant).  device: HIP ordinal. */
int rced_create(int variant, const float* blob, size_t n_floats, int device, rced_model** out);
void rced_destroy(rced_model* m);

/* y = model(x).  x_dev / y_dev: DEVICE pointers to [N,T,129,1] float32, resident on the
 * model's device.  stream: a hipStream_t (NULL = default stream).  Asynchronous: returns
 * after enqueueing.  Replaces sess.run(self.pred, ...) with device-resident tensors. */
int rced_forward(rced_model* m, const float* x_dev, float* y_dev, int N, int T, void* stream);

/* State of the model AFTER work the caller has synchronised itself.  rced_forward only enqueues; the fused CR-CED kernel
 * records a wave-to-wave hand-off that timed out in a sticky word in pinned host memory, which the library looks at before
 * the NEXT launch and in its synchronising entry points (rced_forward_host, rced_profile_query) -- a caller that enqueues
 * one forward, synchronises its own stream and reads y calls this to learn that y is valid: RCED_OK, or RCED_ERR_STATE
 * (the masks of that launch are wrong; destroy and recreate the model).  No device call, no synchronisation. */
int rced_check(rced_model* m);

/* Same with HOST pointers (the reference boundary hands numpy arrays: tester.py:85-90).
 * Copies H2D, runs, copies D2H, synchronises.  Batches >= 8 MB are split into "host_chunks" utterance chunks and
 * the three legs are overlapped on internal streams (a helper thread issues the downloads). */
int rced_forward_host(rced_model* m, const float* x_host, float* y_host, int N, int T);

/* Pre-size the internal workspace for shapes up to [N,T,...] so that rced_forward performs
 * no allocation (needed before stream capture into a hipGraph). */
int rced_reserve(rced_model* m, int N, int T);

/* Options (set/get unless noted).  Returns RCED_ERR_ARG for unknown keys/values.
 *   "path"        RCED_PATH_*
 *   "profile"     1: HIP events around every kernel launch (read with rced_profile_query); set re-arms
 *   "host_chunks" pipeline depth of rced_forward_host (0 = default 8, 1 = no overlap, <= 64)
 *   "fused_grid"  workgroups of the persistent fused kernel (0 = one per CU)
 *   "bf16"        R-CED V1 / V2 only: 1 = bf16 activations + inner-layer weights, fp32 accumulation (BASELINE config 2;
 *                 ~6e-3 of the largest output away from the fp32 result -- opt-in)
 *   "v3_bf16"     CR-CED only: 1 = the whole forward in bf16 (activations, weights; fp32 accumulation), ONE launch of the wave-per-frame
 *                 kernel "bf16" runs for R-CED -- ~6e-3 of the largest output away from the fp32 result, opt-in, no
 *                 environment default; 0 (default) = the "v3_l2x6" form selected.  Built on first use.  "bf16" itself stays refused for
 *                 CR-CED ("v3_l2x6", "fused_final" and rced_check are unaffected: the kernel has no wave-to-wave hand-off).
 *   "bf16_frames" "bf16" / "v3_bf16" mode: frames (= waves) per workgroup of the kernel, 0 (default) = chosen per call -- eight once
 *                 the call has 16 frames per CU, four below that --, 4 or 8 = always that form.  Results are bit-identical either way.
 *   "v3_l2x6"     CR-CED only: which form of the fused kernel runs.  3 (default) = EVERY layer at fp32 quality on the bf16 matrix pipe
 *                 (three-part operands, six products): the first layer from an im2col-along-time of the input rows, the 18 -> 30 and
 *                 30 -> 8 layers as one stream in which the 30-channel tensor never leaves the registers, decode_final as a GEMM over a
 *                 tap table resident in LDS; 0 = every layer on the fp32 MFMA (bit-for-bit an fp32 fmaf chain; the in-build comparator:
 *                 the two agree to ~1e-6 of the largest output).  The intermediate forms of rounds 3 - 4 (1, 2) are in the library only
 *                 when it is compiled with -DRCED_V3_LEGACY_FORMS=1; otherwise they are refused ("v3_l2x6 takes 3 ... or 0").  A form's
 *                 weight stream is built when it is first selected.
 *   "final_x6", "final_lds"   R-CED V1 / V2 only, fp32 mode: the 1x129 output layer's kernel -- three-part bf16 products (1,
 *                 default) or the fp32 MFMA (0), the latter with (1) / without (0) LDS staging of its B operand.  (In "bf16" mode the
 *                 output layer runs inside the one fused kernel.)
 *   "latency_form"  R-CED V1 / V2 only (fp32 kernel): 1 (default) = a call with fewer 3-frame tiles than the part has CUs (BASELINE
 *                 config 1: one utterance of 256 frames) runs on ONE-frame tiles -- three times the workgroups, a third of the work
 *                 each, bit-identical results; 0 = always 3-frame tiles
 *   "inject_handoff_error"  set only, CR-CED: writes the value into the sticky hand-off error word as the kernel would on a
 *                 time-out (0 clears it) -- a test hook for rced_check / RCED_ERR_STATE handling
 *   "has_fused", "num_cus", "fused_final"  get only ("fused_final": the 1x129 output layer runs inside the fused kernel)
 * Options are PER HANDLE.  Environment variables only supply DEFAULTS, read once when a handle is created (rced_create /
 * rced_train_create) and never afterwards: RCED_V3_L2X6, RCED_FINAL_X6, RCED_FINAL_LDS (the options of the
 * same meaning above); for rced_train_create RCED_TRAIN_MFMA=0 (direct-conv kernels only), RCED_TRAIN_FUSE_ACT=0,
 * RCED_TRAIN_FUSE_DZ=0 (materialise activations / dz), RCED_TRAIN_FUSE_SUMS, RCED_TRAIN_FUSE_BWD, RCED_TRAIN_DET, RCED_TRAIN_X6,
 * and the test knob RCED_TRAIN_MAX_GRID=n (n >= 1: no tile-walking training kernel is launched with more than n workgroups, so a
 * batch of a few frames walks several tiles per workgroup; unset or 0: no cap; see rced_train_grid_stats). */
int rced_set_option(rced_model* m, const char* key, int value);
int rced_get_option(rced_model* m, const char* key, int* value);

/* The single op, module.py:11-34 conv_bn_relu with is_training=False, on DEVICE pointers:
 *   x [N,T,F,cin] -> y [N,T,F,cout];  kernel [kh,kw,cin,cout], bias [cout] (device);
 *   bn = gamma,beta,moving_mean,moving_variance (4*cout floats, device) or NULL (use_norm=False);
 *   skip_input [N,T,F,cout] or NULL; use_act 0/1.  padding SAME, stride 1. */
int rced_conv_bn_relu(const float* x, float* y, const float* kernel, const float* bias,
                      const float* bn, const float* skip_input, int use_act, int N, int T, int F,
                      int cin, int cout, int kh, int kw, int device, void* stream);

/* ---- audio front-end / back-end around the CNN, fixed to the reference's
 * configuration: 8 kHz, 256-sample hamming window, 128-sample stride, rfft(256) -> 129 bins. ---- */

/* Frames the reference produces for a signal of `length` samples: ceil(|L-256|/128 + 1)
 * (data_utils/audio_feature.py:70). */
int rced_stft_num_frames(int length);

/* AudioFeature.compute_spectrogram + power_spectrum + divide_phase (audio_feature.py:22-44,102-115) for a
 * batch, laid out as DataLoader.padding_batch does (data_loader.py:198-209):
 *   pcm_dev [N, L] float32; lengths_dev [N] int32 (device) or NULL (= L each);
 *   mag_dev [N, T, 129] float32 (= the CNN's [N, T, 129, 1] input);
 *   phase_dev [N, T, 129, 2] float32 (re, im of exp(j*angle)) or NULL.
 * Frames past an utterance's own rced_stft_num_frames(length) are zero magnitude, phase 1+0j. */
int rced_stft(const float* pcm_dev, const int* lengths_dev, int N, int L, int T, float* mag_dev,
              float* phase_dev, int device, void* stream);

/* AudioReBuild.rebuild_audio (model_utils/utils.py:171-183): merge mag*phase, irfft(n=nfft)[:256],
 * divide by the hamming window, keep the first half of frame 0 and the second half of every frame,
 * de-emphasis.  audio_dev [N, (T+1)*128] float32; the caller trims row n to its signal length.
 * nfft = 512 reproduces the reference as shipped (AudioReBuild() default although the STFT used 256);
 * nfft = 256 is the matching inverse. */
int rced_istft(const float* mag_dev, const float* phase_dev, int N, int T, int nfft, float* audio_dev,
               int device, void* stream);

/* The same two entries with the kernel family as an ARGUMENT (there is no process-wide state): RCED_AUDIO_X6 = the three-part bf16
 * kernels (fp32 quality on the bf16 matrix pipe, kernels_audio_x6.h: what rced_stft / rced_istft launch), RCED_AUDIO_F32 = the
 * fp32-MFMA kernels (the in-build comparator; both pass the same reference-pinned tests).  Any other value: RCED_ERR_ARG. */
#define RCED_AUDIO_F32 0
#define RCED_AUDIO_X6 1
int rced_stft_ex(const float* pcm_dev, const int* lengths_dev, int N, int L, int T, float* mag_dev,
                 float* phase_dev, int device, void* stream, int kernels);
int rced_istft_ex(const float* mag_dev, const float* phase_dev, int N, int T, int nfft, float* audio_dev,
                  int device, void* stream, int kernels);

/* The opt-in rebuild: least-squares weighted overlap-add (Griffin-Lim synthesis) in place of AudioReBuild's divide-by-window-and-
 * keep-half.  For utterance n with F = frames_dev[n] frames, w = hamming(256):
 *   x_t  = irfft(mag[n,t] * phase[n,t], 256), t < F (the imaginary parts of bins 0 and 128 are ignored, as irfft ignores them);
 *   e[i] = sum_{t<F} w[i - 128t] x_t[i - 128t] / sum_{t<F} w[i - 128t]^2,  i < 128 (F + 1), the sums over the frames that cover i
 *          (hops 0 and F are covered by one frame: their denominator is that frame's w^2 alone);
 *   y[0] = e[0], y[i] = e[i] + 0.97 y[i-1] (the reference's de-emphasis); columns 128 (F + 1) .. (T + 1) * 128 are written as 0.
 * frames_dev [N] int32 (device) or NULL (= T each); a value outside [0, T] is clamped into it.  Frames t >= F are never read (after
 * the net a padded frame is not zero and would bleed into hop F), so utterance n's result does not depend on T, N, its row or its
 * neighbours, and is bit-identical run to run (no atomics).  audio_dev [N, (T+1)*128] float32, every column written; there is no
 * nfft (the nfft = 512 quirk has no overlap-add counterpart) and no RCED_AUDIO_F32 form.  One launch; after the first call's table
 * upload it is asynchronous and allocates nothing. */
int rced_istft_ola(const float* mag_dev, const float* phase_dev, const int* frames_dev, int N, int T, float* audio_dev,
                   int device, void* stream);

/* Waveform terms of a training objective on the overlap-add rebuild, and their gradient with respect to the magnitudes.  Default
 * framing only (256 / 128 / hamming, 8 kHz).  Per utterance n: M = mag[n] [T,129], P = phase[n] [T,129,2] (unit phase of the
 * mixture), F frames, c = the clean row of l = lengths_dev[n] samples (clamped into [0, clean_stride]).
 *   The rebuild.  y = rced_istft_ola(M, P, F), exactly as defined above: x_t = irfft(M_t P_t, 256); e = sum_t w x_t / sum_t w^2 over
 *     the frames that cover a sample; y[i] = e[i] + 0.97 y[i-1].
 *   The range R = [lo, hi).  skip_edges = 1: lo = 128, hi = min(l, 128 F) -- only the hops two frames cover are scored; hops 0 and
 *     F divide by one frame's w^2, down to 0.0064, and would weight sample 0 about 156 times over the middle of the signal.
 *     skip_edges = 0: lo = 0, hi = min(l, 128 (F + 1)), the range rced_si_sdr scores.  An empty range contributes nothing to any term
 *     and has zero gradient.
 *   The terms.  wave_sse = sum_R (y - c)^2;  si_sdr = 10 log10((|alpha c|^2 + eps) / (|y - alpha c|^2 + eps)), alpha = <y,c> / <c,c>,
 *     every sum over R, in two passes (alpha first), fp64 from the fp32 signals; eps = 1e-8 is this project's choice.  If <c,c> = 0
 *     or R is empty the SI-SDR term is INVALID: it counts 0, its gradient is 0, and the validity column says so.
 *   terms_dev [N,3] double = (wave_sse, si_sdr, valid 1.0 / 0.0), unweighted.
 *   The gradient of  w_sse * inv_batch * sum_n wave_sse_n  -  w_si_sdr * inv_batch * sum_valid si_sdr_n  (inv_batch = 1 / B, B the
 *     trainer's batch size).  With k = 10 / ln 10, r = y - alpha c:
 *       g_y = w_sse inv_batch 2 (y - c) - w_si_sdr inv_batch k (2 alpha c / (|alpha c|^2 + eps) - 2 r / (|r|^2 + eps)) on R, 0 outside;
 *       g_e[i] = g_y[i] + 0.97 g_e[i+1] (the de-emphasis transposed);  u = g_e / sum w^2;  G_t = rfft(w u[128t : 128t + 256]);
 *       dM_t[b] = (kappa_b / 256)(P_re G_re + P_im G_im), kappa = 1 at bins 0 and 128 and 2 elsewhere.
 *     grad_dev: NULL (terms only) or [N,T,129] float32, every element written; frames t >= F as zeros.
 * frames_dev [N] int32 or NULL (= rced_stft_num_frames(length)); either is clamped into [0, T].  Frames t >= F of mag and phase and
 * samples >= l of the clean rows are never read.  No atomics: bit-identical run to run, and a row's bits do not depend on N, T, its
 * row index or its neighbours.  The weights must be finite and >= 0, inv_batch finite and > 0, skip_edges 0 or 1: anything else is
 * RCED_ERR_ARG before any device work.  Seven launches with a gradient, five without; a workspace of its own per (device, stream),
 * growing only: after the first call at a shape nothing is allocated.  Asynchronous. */
int rced_wave_loss(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                   const int* lengths_dev, int N, int T, double w_sse, double w_si_sdr, int skip_edges, double inv_batch,
                   double* terms_dev, float* grad_dev, int device, void* stream);

/* ---- any framing: the same three transforms with the window length W, the stride S and the window's name as arguments.
 * 2 <= W <= 256 (rfft(256) would crop a longer frame), 1 <= S <= W; the window is numpy's hamming / hanning / blackman / bartlett at
 * length W, evaluated in double on the host.  These entries always run the general kernels (kernels_framing.h), at 256 / 128 / hamming
 * too, where the entries above run the specialised ones.  Coefficient packs are cached per device and (W, name); the rebuilds keep a
 * frame buffer [N, T, 256] per (device, stream) that only grows: after one call of a shape they allocate nothing. ---- */
#define RCED_WINDOW_HAMMING 0
#define RCED_WINDOW_HANNING 1
#define RCED_WINDOW_BLACKMAN 2
#define RCED_WINDOW_BARTLETT 3

/* RCED_OK or RCED_ERR_ARG (the reason in rced_last_error); touches no device. */
int rced_framing_check(int window, int stride, int window_name);

/* ceil(|L - W| / S + 1) (audio_feature.py:70); 0 for length <= 0, -1 for a framing rced_framing_check refuses.  Host only. */
int rced_stft_num_frames_fr(int length, int window, int stride);

/* rced_stft at a framing: frame t holds the pre-emphasised samples t S .. t S + W - 1 (zero fill after pre-emphasis), times the window,
 * rfft(256).  Shapes, lengths_dev, phase_dev = NULL and the padding frames (zero magnitude, phase 1+0j) as rced_stft. */
int rced_stft_fr(const float* pcm_dev, const int* lengths_dev, int N, int L, int T, int window, int stride, int window_name,
                 float* mag_dev, float* phase_dev, int device, void* stream);

/* rced_istft at a framing, hamming window: irfft(n = nfft)[:W] / w, the first W - S samples of frame 0 and the last S samples of
 * every frame, de-emphasis.  audio_dev [N, (W - S) + T * S].  There is no window name: the other three windows end in zero, so the
 * reference's own division is not finite there (hanning, bartlett) or off by 1e17 (blackman); rced_istft_fr_check says so by name. */
int rced_istft_fr(const float* mag_dev, const float* phase_dev, int N, int T, int nfft, int window, int stride, float* audio_dev,
                  int device, void* stream);

/* Whether the reference rebuild exists for a framing: RCED_OK for hamming, RCED_ERR_ARG with the reason for the other names (decided
 * by the name, not by testing a window value against zero) and for a framing rced_framing_check refuses.  Touches no device. */
int rced_istft_fr_check(int window, int stride, int window_name);

/* rced_istft_ola at a framing.  x_t = irfft(mag_t * phase_t, 256)[:W];
 *   e[i] = sum_t w[i - tS] x_t[i - tS] / sum_t w[i - tS]^2 over the frames t < F that cover i, and 0 where the denominator is at most
 *   1e-10 (scipy.signal.istft's rule; never for hamming); y[i] = e[i] + 0.97 y[i-1]; columns from (F - 1) S + W on are 0.
 * audio_dev [N, (W - S) + T * S], every column written; frames_dev and everything about frame counts as rced_istft_ola.  The addends
 * of a sample are summed in ascending frame order: bit-identical run to run and whatever N, T or the utterance's row. */
int rced_istft_ola_fr(const float* mag_dev, const float* phase_dev, const int* frames_dev, int N, int T, int window, int stride,
                      int window_name, float* audio_dev, int device, void* stream);

/* rced_wave_loss at a framing: the same terms, validity, eps, objective and g_y, with W = window, S = stride and w = numpy's window of
 * that name at length W in place of 256, 128 and hamming.  Per utterance: M [T,129] the prediction, P the mixture's unit phase, F its
 * frame count, c the clean row of l samples.
 *   The rebuild.  y = rced_istft_ola_fr(M, P, F), exactly as defined above: x_t = irfft(M_t P_t, 256)[:W];
 *     D[i] = sum_t w[i - tS]^2 and e[i] = sum_t w[i - tS] x_t[i - tS] / D[i] over the frames t < F that cover i; e[i] = 0 where
 *     D[i] <= 1e-10; y[i] = e[i] + 0.97 y[i-1]; n_out = (F - 1) S + W.
 *   The range R = [lo, hi).  skip_edges = 1: lo = W - S, hi = min(l, F S) -- exactly the samples whose covering frames are limited
 *     neither by t >= 0 nor by t <= F - 1; in there D is periodic in S.  At 256 / 128 this is rced_wave_loss's [128, 128 F).
 *     skip_edges = 0: lo = 0, hi = min(l, n_out).  F <= 0 or hi <= lo gives an empty range: no contribution, zero gradient, the SI-SDR
 *     term invalid.
 *   The gradient.  g_e[i] = g_y[i] + 0.97 g_e[i+1] for i < n_out; u[i] = g_e[i] / D[i], and u[i] = 0 where D[i] <= 1e-10 -- decided
 *     with the expression the rebuild uses (an fp32 sum of w[r]^2 in ascending frame order), so the forward's zero set and the
 *     gradient's are the same set; G_t = rfft_256(w u[tS : tS + W]), zero-padded to 256;
 *     dM_t[b] = (kappa_b / 256)(P_re G_re + P_im G_im) for t < F, exact zeros for t >= F.
 * frames_dev [N] int32 or NULL (= rced_stft_num_frames_fr(length, W, S)); either is clamped into [0, T].  Like the other _fr entries
 * this one always runs the general kernels, at 256 / 128 / hamming too.  A framing rced_framing_check refuses is RCED_ERR_ARG before
 * any device work; everything else about arguments, reads, determinism and the workspace (one of its own per (device, stream),
 * growing only: the second call at a shape allocates nothing and can be captured) as rced_wave_loss.  Eight launches with a
 * gradient, six without. */
int rced_wave_loss_fr(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                      const int* lengths_dev, int N, int T, int window, int stride, int window_name, double w_sse, double w_si_sdr,
                      int skip_edges, double inv_batch, double* terms_dev, float* grad_dev, int device, void* stream);

/* ---- the multi-resolution STFT term: a spectral-convergence part and a log-magnitude part per resolution (Yamamoto et al. 2020,
 * Defossez et al. 2020), between a signal y and a clean signal c.  All sums are fp64, taken from the fp32 signals.  For one utterance,
 * [lo, hi) the scored range and K resolutions (W_r, S_r, name_r), 1 <= K <= 4, each one rced_framing_check accepts:
 *   J_r = floor((hi - lo - W_r) / S_r) + 1 if hi - lo >= W_r, else 0: only whole frames inside the range, no padding, nothing outside
 *     [lo, hi) is read, and the samples behind the last whole frame play no part at that resolution.
 *   X_j = rfft_256(w_r x[lo + j S_r : lo + j S_r + W_r]), zero-padded to 256, no pre-emphasis; w_r = numpy's window of that name at
 *     length W_r, in double, on the host.
 *   |X|_eps = sqrt(re^2 + im^2 + eps), eps = 1e-8 (this project's choice, as for SI-SDR).
 *   A_r = sum (|C|_eps - |Y|_eps)^2, B_r = sum |C|_eps^2 over j < J_r and 129 bins;  sc_r = sqrt(A_r / B_r);
 *   lsd_r = sum (ln|C|_eps - ln|Y|_eps)^2 / (129 J_r): the mean SQUARED log-magnitude difference, not the published L1 -- an L1
 *     term's gradient jumps where two magnitudes tie, and an fp32 device cannot be held to a derived bar across a sign flip.
 *   term = sum_{r: J_r > 0} (sc_r + lsd_r) / K;  mr_valid = 1 if any J_r > 0, else 0: an invalid term counts 0 and has zero gradient.
 *   The gradient with respect to y.  Per bin, d = ln|C|_eps - ln|Y|_eps:
 *     g = -(|C|_eps - |Y|_eps) / (sqrt(A_r) sqrt(B_r)) - 2 d / (129 J_r |Y|_eps), the first part exactly 0 where A_r = 0;
 *     G = g Y / |Y|_eps;  d/dy[lo + j S_r + k] += w_r[k] sum_b (G_re cos(2 pi b k / 256) - G_im sin(2 pi b k / 256));
 *     divided by K, times w_mr inv_batch; summed over frames in ascending j, then over resolutions in ascending r.  No kappa factor:
 *     the loss sums 129 bins, not 256.
 * No model has been trained to convergence with this term. */
typedef struct rced_mr_args {
  double w_mr;        /* the term's weight, finite and >= 0 */
  int n_res;          /* K, 1 .. 4 */
  int window[4];      /* W_r, S_r, RCED_WINDOW_* of resolution r < K */
  int stride[4];
  int window_name[4];
} rced_mr_args;

/* RCED_OK or RCED_ERR_ARG (the reason in rced_last_error): NULL, a weight that is negative or not finite, n_res outside [1, 4], a
 * resolution rced_framing_check refuses.  Touches no device. */
int rced_mr_stft_check(const rced_mr_args* mr);

/* The term between two ragged row sets over [0, l_n), l_n = lengths_dev[n] clamped into [0, min(est_stride, ref_stride)].
 * est_dev, ref_dev: N rows of est_stride / ref_stride floats, any alignment.  terms_dev [N, 2 + 3 K] double = (term, valid, then
 * sc_r, lsd_r, J_r per resolution), unweighted.  grad_dev: NULL, or [N, est_stride] float32 = d(w_mr inv_batch sum_n term_n) / d est,
 * every column written, zeros from l_n on.  What rced_mr_stft_check refuses, a negative shape, inv_batch not finite or <= 0,
 * N > 65535 and a missing pointer are RCED_ERR_ARG before any device work.  No atomics: bit-identical run to run, and a row's bits do
 * not depend on N, its row index or its neighbours.  A workspace per (device, stream), growing only (Y, |Y|, |C| of the resolution
 * with the most frames, and with a gradient a frame scratch [N, J_r, W_r] per resolution): the second call at a shape allocates
 * nothing and can be captured.  2 K + 2 launches, 3 K + 3 with a gradient.  Asynchronous. */
int rced_mr_stft(const float* est_dev, int est_stride, const float* ref_dev, int ref_stride, const int* lengths_dev, int N,
                 const rced_mr_args* mr, double inv_batch, double* terms_dev, float* grad_dev, int device, void* stream);

/* rced_wave_loss_fr plus the term on its rebuilt y against the clean rows, over its R (the same skip_edges rule).
 * terms_dev [N, 5] double = (wave_sse, si_sdr, valid, mr_stft, mr_valid), unweighted.  grad_dev: NULL or [N, T, 129] float32, the
 * gradient of  w_sse inv_batch sum wave_sse - w_si_sdr inv_batch sum_valid si_sdr + w_mr inv_batch sum_valid mr_stft  with respect to
 * mag: the term's gradient with respect to y is added to g_y in fp64, before the de-emphasis' transposed scan; everything behind
 * that place is rced_wave_loss_fr's.  The same kernels as rced_mr_stft, with R as the per-utterance range.  It always runs the
 * general kernels, at 256 / 128 / hamming too.  Arguments, reads, determinism and workspaces as rced_wave_loss_fr and rced_mr_stft.
 * 8 + 2 K launches, 11 + 3 K with a gradient. */
int rced_wave_loss_mr(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                      const int* lengths_dev, int N, int T, int window, int stride, int window_name, double w_sse, double w_si_sdr,
                      int skip_edges, double inv_batch, const rced_mr_args* mr, double* terms_dev, float* grad_dev, int device,
                      void* stream);

/* ---- evaluation loop (tester.py:92-167, trainer.py:252-338): the two numpy pieces around the rebuilt audio, for a
 * ragged batch.  Streaming reductions without atomics: results are bit-identical run to run, and utterance n's result
 * does not depend on N, on its neighbours, on its row index or on the row strides (kernels_eval.h).  Both keep a slice
 * workspace per (device, stream) that only grows: after one call of a shape they allocate nothing and can be
 * stream-captured. ---- */

/* SDR.sdr (model_utils/utils.py:68-86) per utterance over its own length:
 *   10 * log10( sum(y^2) / ( sum((y_pred - y)^2) + eps ) ),  eps = np.finfo(np.float32).eps = 2^-23.
 * ref_dev [N, ref_stride] (y), est_dev [N, est_stride] (y_pred) float32, row n holds utterance n from column 0 -- two
 * strides because the estimate is rced_istft's [N, (T+1)*128] buffer and the clean signals are [N, Lmax]: trimming is
 * done by the length, never by a copy.  lengths_dev [N] int32 (device) or NULL (= min(ref_stride, est_stride) each); a
 * length outside [0, min(ref_stride, est_stride)] is clamped into it.  sdr_dev [N] double (dB).  energies_dev: NULL or
 * [N, 2] double receiving sum(y^2), sum((y_pred - y)^2).  Differences and sums in fp64.  y = 0 gives -inf, y_pred == y
 * gives 10*log10(sum(y^2) / 2^-23), a length of 0 gives -inf, as numpy does.  Asynchronous. */
int rced_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride,
             const int* lengths_dev, int N, double* sdr_dev, double* energies_dev, int device, void* stream);

/* AudioParser.add_noise (data_utils/data_loader.py:35-52) for a batch, in closed form (no doubling buffer):
 *   speech_dev [N, Ls] + speech_len_dev [N] int32 (or NULL = Ls each); noise_dev [N, Ln] + noise_len_dev [N] (or NULL);
 *   start_dev [N] int32: the crop offset np.random.randint(0, ln - ls) drew, read only where noise_len > speech_len
 *     (NULL = 0; clamped into [0, ln - ls]);
 *   gains_dev [N, n_gains] double: the np.random.uniform(0, 2) draws u_0.., read only where speech_len >= noise_len.
 * The noise under sample p of an utterance with ls >= ln is noise[p % ln] * prod(u_k for every bit k set in p / ln)
 * (only the first bit_length((ls-1)/ln) gains can matter; bits at or above n_gains count as gain 1), with ls < ln it is
 * noise[start + p].  Then p_sig = sum(speech^2), p_back = sum(noise^2) over [0, ls) and
 *   mix = speech + sqrt(p_sig / 10^(snr_db/10) / p_back) * noise,
 * sums, gain products and the scale in fp64, one rounding at the fp32 store.  p_back = 0 follows IEEE (inf / nan) as
 * numpy does.  mix_dev [N, Ls] float32, columns past speech_len written as 0.  Asynchronous. */
int rced_mix_snr(const float* speech_dev, const int* speech_len_dev, int N, int Ls,
                 const float* noise_dev, const int* noise_len_dev, int Ln,
                 const int* start_dev, const double* gains_dev, int n_gains,
                 double snr_db, float* mix_dev, int device, void* stream);

#define RCED_PCM_S16 0
#define RCED_PCM_F32 1
/* Rows of a zero-padded batch, cut out of a device-resident corpus (the training loader):
 *   rows_dev[n, 0 .. count[n])  = arena[begin[n] .. begin[n] + count[n])  as float32
 *                                 (int16: value / 32768, exact -- what librosa / soundfile give for PCM16; float32: copied)
 *   rows_dev[n, count[n] .. L)  = 0;   columns L .. row_stride are not touched.
 * arena_dev: int16 or float32 [arena_samples]; begin_dev [N] int64 (absolute sample index); count_dev [N] int32.
 * A row whose range leaves [0, arena_samples) or whose count leaves [0, L] is clamped into them (begin into
 * [0, arena_samples], count into [0, min(L, arena_samples - begin)]: never read outside the arena), as the other entries
 * clamp lengths; the Python side validates and raises.  The same item may fill several rows.  One launch, grid over
 * (column blocks, N); asynchronous, allocates nothing, stream-capturable, bit-reproducible. */
int rced_gather_pcm(const void* arena_dev, int arena_dtype, long long arena_samples,
                    const long long* begin_dev, const int* count_dev, int N, int L,
                    float* rows_dev, int row_stride, int device, void* stream);

#define RCED_CONV_MAX_TAPS 8192
/* Room impulse responses for the training loader (DESIGN.md 3.4e "Reverberation"): a ragged batched FIR.  Per row n a
 * signal x_n of len_n samples, a filter h_n of K_n taps and a shift d_n, 0 <= d_n < max(K_n, 1):
 *   y_n[p] = sum_{k < K_n} h_n[k] x_n[p + d_n - k]   for 0 <= p < len_n,   x_n = 0 outside [0, len_n)
 *   y_n[p] = 0                                        for len_n <= p < L;   columns L .. y_stride are not touched
 * -- np.convolve(x, h)[d : d + len]: the output keeps the signal's length, tap d (the direct path) has zero delay, the
 * tail past the end is dropped; K_n = 0 gives zeros.
 * x_dev [N, x_stride], h_dev [N, h_stride], y_dev [N, y_stride] float32; x_len_dev, h_len_dev, shift_dev [N] int32 on
 * the device, or NULL: L each, h_stride each, 0.  A length is clamped into its row (len into [0, L], K into
 * [0, min(h_stride, RCED_CONV_MAX_TAPS)]) and the shift into [0, max(K - 1, 0)], as the other entries clamp lengths:
 * nothing is ever read outside a row; the Python side validates and raises.  y must not overlap x or h.
 * Products and sums in fp64 from the stored fp32 values on the f64 matrix pipe, one rounding at the fp32 store; a
 * row's summation order depends on positions inside the row and on K_n, d_n, len_n only, so a row's bits do not depend
 * on N, its row index, the strides or its neighbours, and are the same run to run.  A sample of -0.0 comes back +0.0; a
 * non-finite sample also reaches, as NaN, the outputs of its own and the neighbouring 16-sample block.  No atomics;
 * samples past len_n and taps past K_n are never read.  One launch, grid over (output slices, N); asynchronous,
 * allocates nothing, stream-capturable.
 * RCED_ERR_ARG before any device work: a null x_dev, h_dev or y_dev, a negative stride or L, L > x_stride, L > y_stride,
 * h_stride > RCED_CONV_MAX_TAPS with h_len_dev NULL, N outside [0, 65535], L > 2^30.  N = 0 is RCED_OK. */
int rced_convolve(const float* x_dev, int x_stride, const int* x_len_dev,
                  const float* h_dev, int h_stride, const int* h_len_dev, const int* shift_dev,
                  int N, int L, float* y_dev, int y_stride, int device, void* stream);

/* ---- resample: audio at any rate ---------------------------------------------------------------------
 * A band-limited (Kaiser-windowed sinc) interpolator with the parameters of resampy's kaiser_best, evaluated exactly:
 *   ratio = (double)sr_new / sr_orig, s = min(1, ratio), p / q = sr_new / sr_orig in lowest terms,
 *   y[m] = sum_j x[j] s h(s ((j - n0) - r / p)),  (n0, r) = divmod(m q, p),  m < (long long)(n * ratio),  x = 0 outside the row,
 *   h(t) = rho sinc(rho t) I0(beta sqrt(1 - (t / 64)^2)) / I0(beta) for |t| < 64, else 0,
 * everything in float64 from the stored samples.  sr_orig == sr_new is the (downmixing) copy. */

/* Output samples of n input frames: (long long)((double)n * ((double)sr_new / sr_orig)); -1 on bad arguments (n < 0, a rate <= 0). */
long long rced_resample_length(long long n, int sr_orig, int sr_new);

/* The phase table of a ratio, host only (works without a GPU): table[r][c] = s h(s ((c - left) - r / p)), r < p, c < width: the
 * `width` columns any phase reaches, `left` of them before n0.  Writes p, q, left, width (each may be NULL) and, when
 * table_host is not NULL, the p * width doubles (n_doubles: the buffer's size; too small is RCED_ERR_ARG).  Built once per
 * ratio and process.  A ratio whose table would exceed 1 MiB (8001 -> 8000, say), or one output of which reaches more frames
 * than a workgroup stages (rates more than 47 : 1 apart going down), is refused: RCED_ERR_ARG, the message names the ratio. */
int rced_resample_taps(int sr_orig, int sr_new, int* p, int* q, int* left, int* width,
                       double* table_host, size_t n_doubles);

/* Row n = frames [begin[n], begin[n] + count[n]) of src_dev, resampled.  src_dev: int16 or float32 (RCED_PCM_*),
 * [src_frames][channels] interleaved; a sample is value / 32768 (int16) or the value, the channels are averaged in float64.
 * begin_dev [N] int64 and count_dev [N] int32 are in frames and clamped into the source as rced_gather_pcm clamps (never
 * read outside it; the Python side validates and raises).  Row n has rced_resample_length(count[n]) outputs, at most L.
 *   out_begin_dev == NULL: they go to out + n * row_stride, zeros from there up to column L; columns L .. row_stride are not touched.
 *   out_begin_dev [N] int64: they go to out + out_begin[n], packed, nothing else is written (a corpus arena, say); L bounds them.
 * out_dtype RCED_PCM_F32: the float64 sum rounded once; RCED_PCM_S16: clip(rint(y * 32768), -32768, 32767), ties to even.
 * One launch, grid over (output tiles, N).  The first call of a ratio on a device uploads its table (allocates, synchronises);
 * every later one allocates nothing, is asynchronous and stream-capturable.  Finite inputs give bit-identical results from
 * run to run, independent of N, the row, begin's alignment, the output mode and the neighbouring rows. */
int rced_resample(const void* src_dev, int src_dtype, int channels, long long src_frames,
                  const long long* begin_dev, const int* count_dev, int N,
                  int sr_orig, int sr_new,
                  void* out_dev, int out_dtype, const long long* out_begin_dev,
                  int row_stride, int L, int device, void* stream);

/* STOI (Taal, Hendriks, Heusdens, Jensen 2011; the reference takes it from pystoi, tester.py:92-167) per utterance over
 * its own length: stoi(x = ref row, y = est row, fs_sig), exactly as DESIGN.md "STOI" specifies it -- polyphase resampling
 * to 10 kHz (fs_sig = 8000; fs_sig = 10000 skips it; any other rate is RCED_ERR_ARG), removal of the frames more than
 * 40 dB under the loudest clean frame, 512-point spectra in 15 one-third-octave bands, 30-frame segments.  Pointers,
 * strides, lengths_dev and their clamping as in rced_sdr.  stoi_dev [N] double; detail_dev: NULL or [N, 3] int32
 * receiving F (frames at 10 kHz), K (frames kept), M (segments).  Fewer than 30 spectral frames (K - 1 < 30, a length of
 * 0 included) give 1e-5; an all-zero clean signal gives 0.  Everything is fp64 from the fp32 inputs except the products
 * of the DFT, which run as three-part bf16 on the matrix pipe (fp32 quality).  No atomics, fixed summation order: the
 * invariants stated above hold; the workspace (per device and stream, growing only) is separate from rced_sdr's.
 * Asynchronous. */
int rced_stoi(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride,
              const int* lengths_dev, int N, int fs_sig, double* stoi_dev, int* detail_dev, int device, void* stream);

/* STOI and / or ESTOI (Jensen, Taal 2016: the `extended` mode of the package the reference takes STOI from) in one call.
 * which: RCED_STOI_CLASSIC, RCED_STOI_EXTENDED or both; with both, the resampling, the silent-frame removal and the band
 * spectra run once.  stoi_dev [N] double is written with CLASSIC, estoi_dev [N] double with EXTENDED; an output that is asked
 * for and NULL, or any other `which`, is RCED_ERR_ARG; one that is not asked for is not touched and may be NULL.  detail_dev
 * and everything else as in rced_stoi, whose results are the bits of which = RCED_STOI_CLASSIC and of the classic half of both.
 * ESTOI as DESIGN.md "ESTOI" specifies it: the same M = K - 30 segments of 30 frames x 15 bands, of x and of y, no clipping
 * and no scaling; each segment's band rows lose their mean over the 30 frames and are divided by (their 2-norm + eps), then
 * its frame columns lose their mean over the 15 bands and are divided by (their 2-norm + eps); sum(xn yn) / (30 M).  M = 0
 * gives 1e-5, an all-zero row gives 0.  fp64; the same invariants; the workspace is rced_stoi's. */
#define RCED_STOI_CLASSIC 1
#define RCED_STOI_EXTENDED 2
int rced_stoi_ex(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride,
                 const int* lengths_dev, int N, int fs_sig, int which, double* stoi_dev, double* estoi_dev,
                 int* detail_dev, int device, void* stream);

/* SI-SDR per utterance over its own length, x = ref row, y = est row, no mean removal:
 *   alpha = sum(y x) / sum(x x);   10 * log10( sum((alpha x)^2) / sum((y - alpha x)^2) ),
 * in two passes (alpha first, then the two energies with alpha in hand: the one-pass closed form cancels for good
 * estimates), fp64 from the fp32 inputs.  Pointers, strides, lengths_dev and their clamping as in rced_sdr.  out_dev [N]
 * double (dB); parts_dev: NULL or [N, 3] double receiving alpha, sum((alpha x)^2), sum((y - alpha x)^2).  IEEE results stand
 * as numpy gives them: y = 2^k x gives +inf (both sums of the first pass run in one order: alpha is exact, the residual
 * zero), x = 0, y = 0 or a length of 0 give nan.  Three launches; a workspace of its own per (device, stream), growing
 * only.  The invariants stated above hold.  Asynchronous. */
int rced_si_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride,
                const int* lengths_dev, int N, double* out_dev, double* parts_dev, int device, void* stream);

/* Segmental SNR per utterance over its own length L: frames of W = (3 fs + 50) / 100 samples (240 at 8 kHz) at hop
 * H = W / 4 (integer divisions), frame i starting at i H, nf = (L - W) / H + 1 frames for L >= W, else 0; window
 * w[j] = 0.5 (1 - cos(2 pi (j + 1) / (W + 1))), j = 0 .. W - 1; per frame
 *   s = 10 * log10( sum((w x)^2) / (sum((w (x - y))^2) + eps) + eps ),  eps = np.finfo(float).eps,
 * clamped to [-10, 35]; the score is the mean over the frames, nan for nf = 0.  fs with W outside [4, 1440] is
 * RCED_ERR_ARG.  Pointers, strides, lengths_dev and their clamping as in rced_sdr; samples past a length are never read.
 * out_dev [N] double (dB); frames_dev: NULL or [N] int32 receiving nf.  fp64 from the fp32 inputs.  Two launches; a
 * workspace of its own per (device, stream), growing only.  The invariants stated above hold.  Asynchronous. */
int rced_seg_snr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride,
                 const int* lengths_dev, int N, int fs, double* out_dev, int* frames_dev, int device, void* stream);

/* LLR and WSS per utterance over its own length L: the log-likelihood ratio of the two signals' LPC models and the
 * weighted spectral slope distance, the two spectral terms of the composite measures CSIG / CBAK / COVL (Hu, Loizou 2008;
 * the other two are the segmental SNR above and PESQ, which this library does not compute).  Both are built as DESIGN.md
 * 3.4c writes them; parity with pysepm or the MATLAB originals is unpinned.
 *   Framing: rced_seg_snr's (W = (3 fs + 50) / 100, hop W / 4, the same window), sample_rate 8000 or 16000 only -- any
 * other rate is RCED_ERR_ARG.  Aggregation, both scores: the mean of the k = (95 nf + 50) / 100 smallest frame values
 * (ties by frame index, summed in one order fixed by the ranks), nan for nf = 0.
 *   LLR: order P = 10 below 10 kHz, else 16; frames of x + eps and y + eps under the window; autocorrelation lags 0 .. P;
 * Levinson-Durbin; d = ln((A_y T A_y') / (A_x T A_x')), T the Toeplitz matrix of the clean frame's lags; with a finite
 * `limit` each d enters the aggregation as min(d, limit) (the usual limit is 2; +inf leaves d alone: the form the
 * composite formulas take; nan is RCED_ERR_ARG).  IEEE results stand.
 *   WSS: |DFT_nfft(w frame)|^2 (nfft = 512 at 8 kHz, 1024 at 16 kHz) in fp64 on the matrix pipe, 25 critical-band
 * energies in dB, 24 slopes, nearest-peak weights, d = sum(W (s_x - s_y)^2) / sum(W).
 *   Pointers, strides, lengths_dev and their clamping as in rced_sdr; samples past a length are never read.  out_dev [N]
 * double.  frames_out: NULL or [N][frames_stride] double receiving every frame's value in frame order (LLR: before the
 * limit); entries at and past an utterance's nf are left untouched.  The lengths live on the device, so frames_stride is
 * held against the most frames a row can carry: frames_stride < frames(min(ref_stride, est_stride)) is RCED_ERR_ARG.
 * nf_out: NULL or [N] int32 receiving nf.  Four launches each; a workspace of its own per (device, stream), growing only;
 * the WSS tables are built once per process and rate and uploaded once per device.  The ranking compares every pair of an
 * utterance's frames: its cost grows with nf^2.  The invariants stated above hold.  Asynchronous. */
int rced_llr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
             int sample_rate, double limit, double* out_dev, double* frames_out, int frames_stride, int* nf_out,
             int device, void* stream);
int rced_wss(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
             int sample_rate, double* out_dev, double* frames_out, int frames_stride, int* nf_out, int device, void* stream);

/* The frequency-weighted segmental SNR (fwSNRseg) and the cepstral distance (CD) per utterance over its own length L: the two
 * objective measures of Hu and Loizou (2008) left beside rced_seg_snr, rced_llr and rced_wss (PESQ is not computed).  Both are
 * built as DESIGN.md 3.4c writes them; parity with pysepm or the MATLAB originals is unpinned.  Framing, window, rates,
 * pointers, strides, lengths_dev, frames_out, frames_stride, nf_out and their checks as in rced_llr / rced_wss; frames_out
 * receives every frame's value after its limits.
 *   fwSNRseg: |DFT_nfft(w frame)| on all nb = nfft / 2 bins in fp64 on the matrix pipe (WSS's coefficient stream; at 16 kHz
 * a second pass over bins 256 .. 511), each signal's magnitudes divided by their sum over the nb bins (added in bin order),
 * the 25 critical-band filters of WSS on those, Wt = E_x^0.2, snr = 10 log10(E_x^2 / max((E_x - E_y)^2, eps)) limited to
 * [-10, 35], frame value sum(Wt snr) / sum(Wt) in band order; the score is the plain mean over the frames in one fixed order,
 * nan for nf = 0.  A frame whose magnitudes sum to zero is 0 / 0 = nan, and so is its utterance.  Three launches.
 *   CD: rced_llr's lags and Levinson-Durbin at order `order`, 1 .. 16 (anything else is RCED_ERR_ARG; LLR's own order is 10
 * below 10 kHz, else 16); cepstra c[1] = -A[1], c[k] = -(A[k] + (sum_{i < k} i c[i] A[k - i]) / k); frame value
 * (10 / ln 10) sqrt(2 sum_k (cx[k] - cy[k])^2) limited to [0, 10]; the score is rced_llr's aggregation, the mean of the
 * k = (95 nf + 50) / 100 smallest frame values.  Four launches.
 *   A workspace of its own each per (device, stream), growing only; the tables are rced_wss's, plus the second pass's
 * coefficients, uploaded once per device.  The invariants stated above hold.  Asynchronous. */
int rced_fwseg(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
               int sample_rate, double* out_dev, double* frames_out, int frames_stride, int* nf_out, int device, void* stream);
int rced_cepd(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
              int sample_rate, int order, double* out_dev, double* frames_out, int frames_stride, int* nf_out,
              int device, void* stream);

/* The signal-to-distortion ratio of BSS Eval (Vincent, Gribonval, Fevotte 2006) for a single source, per utterance over
 * its own length L: the estimate is first projected onto the span of the clean signal delayed by 0 .. F - 1 samples,
 * F = filter_length, 1 <= F <= 512 (anything else is RCED_ERR_ARG), so a fixed linear filtering or a delay of the estimate
 * is forgiven.  x = ref row, y = est row, float32 samples [0, L) read as float64; samples at or past L count as 0 and are
 * never read:
 *   r[t] = sum_n x[n] x[n + t],  d[t] = sum_n x[n] y[n + t],  t = 0 .. F - 1;
 *   G = toeplitz(r), G c = d: the least-squares causal FIR of F taps from x to y;
 *   s = x * c over L + F - 1 samples,  e = [y, 0 .. 0] - s over the same;   score = 10 * log10(sum s^2 / sum e^2) dB.
 * This is bss_eval_sources for one source (its SDR equals its SAR, its SIR is infinite); parity with mir_eval or museval
 * is unpinned: the pin is the float64 restatement in tests/bsseval_np.py.  With F = 1 the score is rced_si_sdr's.
 * L = 0, x = 0 and y = 0 give nan; non-finite samples propagate.  Nothing is regularised and there is no least-squares
 * fallback: a singular or numerically singular G (a reference with an empty band) gives whatever the recursion gives.
 * Pointers, strides, lengths_dev (NULL: every row is read to the shorter stride) and their clamping as in rced_sdr.
 * sdr_dev [N] double; filter_dev: NULL or [N, filter_length] double receiving c; energies_dev: NULL or [N, 2] double
 * receiving sum s^2, sum e^2.  fp64 throughout: both correlations and the projection are block-Toeplitz products on the
 * fp64 matrix pipe over slices of 4096 samples, summed in slice order; the solve is Levinson's recursion with a general
 * right-hand side, one wave per utterance.  Four launches; a workspace of its own per (device, stream), growing only: after
 * one call of a shape nothing is allocated and the call can be stream-captured.  The invariants stated above hold.
 * Asynchronous. */
int rced_bss_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
                 int filter_length, double* sdr_dev, double* filter_dev, double* energies_dev, int device, void* stream);

/* ---- streaming denoiser: PCM in, PCM out, 128 samples (one hop, 16 ms) at a time, for many independent streams ("lanes") at once,
 * at a fixed delay.  Only the first layer of the three networks looks across time (3 past, 4 future frames) and the rebuild uses no
 * overlap-add, so the chunked run reproduces the whole-utterance chain rced_stft -> rced_forward -> rced_istft.
 * For one lane let s[0..L) be everything pushed before rced_stream_finish (the tail included), H the hops pushed and `off` the
 * whole-utterance result of length L.  The lane's output stream is `off` delayed by RCED_STREAM_DELAY samples: a push of K hops
 * returns K*128 samples per lane, zeros until 640 samples have left, then off[i - 640].  Frames are the reference's own set
 * (rced_stft_num_frames(L), zero padding applied after pre-emphasis): pushing zeros is not finishing.  All state lives on the device;
 * after rced_stream_create a push is three launches on the caller's stream, allocates nothing and does not synchronise.  The input
 * buffers must stay valid until that work has run (the last launch reads them again).  A stream object is not thread-safe.
 *
 * A stream created with RCED_STREAM_REBUILD_OLA (rced_stream_create_ex) rebuilds by weighted overlap-add instead: `off` is the chain
 * rced_stft -> rced_forward -> rced_istft_ola over the utterance's T = rced_stft_num_frames(L) frames, and everything else above holds
 * as it stands -- the delay too: a push that brings a lane to H' hops has the masks of frames <= H' - 6 and emits hops <= H' - 6, and
 * hop h needs frames h and h - 1.  With w = hamming(256), D[s] = w[s]^2 + w[s+128]^2 and x_t = irfft(mask_t * phase_t, 256), output
 * position p of a push to a lane at H hops is hop t = H - 5 + p:
 *   t < 0: exactly zero;   t = 0: e = w[s] x_0[s] / w[s]^2;   t >= 1: e = (w[s] x_t[s] + w[s+128] x_{t-1}[s+128]) / D[s];
 * a hop a push emits is never the utterance's last.  y = e + 0.97 * (the sample before), through the hops in time order, y[0] = e[0].
 * rced_stream_finish (L = 128*H + r): frames at or past T are not rebuilt, hop T has frame T - 1 alone (denominator w[s+128]^2), hops
 * past T are not owed; a frame t < T counts in numerator and denominator even where the signal gave it only zeros (L < 256).
 * A lane keeps the second half of its newest rebuilt frame and the last sample handed out; the state's size does not change. ---- */
#define RCED_STREAM_DELAY 640       /* samples: 5 hops */
#define RCED_STREAM_FINISH_MAX 768  /* floats per lane of rced_stream_finish's out_dev (at most 767 are owed) */
typedef struct rced_stream rced_stream;
int rced_stream_delay(void);

/* lanes >= 1 streams, pushes of at most max_hops (1..64) hops, nfft 512 (the reference as shipped) or 256 for the rebuild; anything
 * else is RCED_ERR_ARG.  Runs the forward form the model handle has selected at each push, on the model's device.  The model must
 * outlive the stream: after rced_destroy(m) the stream's entry points return RCED_ERR_STATE (rced_stream_destroy stays valid). */
int rced_stream_create(rced_model* m, int lanes, int max_hops, int nfft, rced_stream** out);
/* The same with the rebuild named: RCED_STREAM_REBUILD_REFERENCE (what rced_stream_create makes, bit for bit) or
 * RCED_STREAM_REBUILD_OLA (weighted overlap-add, above); any other value is RCED_ERR_ARG.  With overlap-add nfft is checked as above
 * and plays no part, as in rced_istft_ola.  Push, finish, reset and destroy do not differ. */
#define RCED_STREAM_REBUILD_REFERENCE 0
#define RCED_STREAM_REBUILD_OLA 1
int rced_stream_create_ex(rced_model* m, int lanes, int max_hops, int nfft, int rebuild, rced_stream** out);
void rced_stream_destroy(rced_stream* s);

/* pcm_dev [lanes, K*128] float32: the next K hops of every lane; out_dev [lanes, K*128].  active_dev: NULL (every lane) or [lanes]
 * int32 flags; a lane flagged 0 is idle: its state does not change, its input row is not read and zeros are written to its output
 * row.  K < 1 or K > max_hops: RCED_ERR_ARG.  Asynchronous. */
int rced_stream_push(rced_stream* s, const float* pcm_dev, const int* active_dev, int K, float* out_dev, void* stream);

/* Ends the utterance of every lane whose tail_counts_dev entry is 0..127: tail_dev [lanes, 128] holds that many last samples (fewer
 * than a hop).  out_dev [lanes, RCED_STREAM_FINISH_MAX] receives from column 0 the L - max(0, 128*H - 640) samples still owed --
 * off[max(0, 128*H - 640) .. L); for H < 5 that is the whole of `off`, the zeros pushes have returned so far being all there are --,
 * zeros behind them; out_counts_dev [lanes] int32 that count.  The lane is then reset for a new utterance.  Entry -1: the lane is
 * left alone (count 0).  Asynchronous. */
int rced_stream_finish(rced_stream* s, const float* tail_dev, const int* tail_counts_dev, float* out_dev, int* out_counts_dev,
                       void* stream);

/* Back to the start of an utterance without output: lane, or -1 for every lane.  Ordered on the stream of the latest push / finish. */
int rced_stream_reset(rced_stream* s, int lane);

/* ---- streaming at a framing: a stream created for a window W, a stride S and a window name (the "any framing"
 * section above).  The hop is S samples, R = ceil(W / S), and `off` is the offline chain at that framing cut to L samples:
 * rced_stft_fr -> rced_forward -> rced_istft_ola_fr (RCED_STREAM_REBUILD_OLA) or rced_istft_fr (RCED_STREAM_REBUILD_REFERENCE) over
 * the utterance's T = rced_stft_num_frames_fr(L, W, S) frames.  The lane's output is `off` delayed by D = (R + 3) * S samples: frame t
 * covers samples tS .. tS + W - 1 and is complete with hop t + R - 1, its mask needs 4 future frames, and hop h is rebuilt from frames
 * h - R + 1 .. h.  Everything the section above says about frame sets holds with W, S and T: the tail is zero-filled after
 * pre-emphasis, a frame at or past T is neither input nor rebuilt, a frame below T counts in numerator and denominator, denominators
 * count the frames that exist, a sample whose sum of w^2 is at most 1e-10 is 0, de-emphasis is carried across pushes.
 * rced_stream_push, _finish, _reset and _destroy serve such a stream with their signatures unchanged: K*S floats per lane in and out,
 * tail counts 0 .. S - 1 with tail_dev [lanes, S], out_dev of a finish [lanes, rced_stream_finish_max_fr(W, S)], of which the first
 * L - max(0, S*H - D) are owed.  A push is four launches (the rebuild is two), allocates nothing and does not synchronise.  Such a
 * stream always runs the general kernels, at 256 / 128 / hamming too (delay 640, as RCED_STREAM_DELAY). ---- */

/* RCED_OK, or RCED_ERR_ARG with the reason: what rced_framing_check refuses; rebuild other than the two above; the reference rebuild
 * with a window rced_istft_fr_check refuses; ceil(W / S) > 8 (state and delay grow with the overlap).  Touches no device. */
int rced_stream_fr_check(int window, int stride, int window_name, int rebuild);
/* D = (ceil(W / S) + 3) * S samples; -1 for a framing rced_stream_fr_check refuses.  Host only. */
int rced_stream_delay_fr(int window, int stride);
/* Floats per lane of rced_stream_finish's out_dev on such a stream: (ceil(W / S) + 4) * S = D + S; -1 as above.  Host only. */
int rced_stream_finish_max_fr(int window, int stride);
/* rced_stream_create_ex at a framing.  lanes, max_hops (1..64) and nfft are checked as there (nfft plays no part in overlap-add);
 * what rced_stream_fr_check refuses is RCED_ERR_ARG. */
int rced_stream_create_fr(rced_model* m, int lanes, int max_hops, int nfft, int rebuild, int window, int stride, int window_name,
                          rced_stream** out);

/* ---- streaming resampler: the conversion of the "resample" section for audio that arrives piece by piece, for many independent
 * streams ("lanes") at once, at a fixed delay.  A lane stream is created for a unit pair: every push of K units
 * hands each active lane K * unit_in source frames and returns K * unit_out samples; unit_in * p must equal unit_out * q (p / q =
 * sr_out / sr_in in lowest terms).  For one lane let x[0..L) be everything pushed before rced_rstream_finish (the tail included),
 * H the units pushed and y = rced_resample(x), M = rced_resample_length(L) samples, x = 0 outside [0, L).  The lane's output stream
 * is y delayed by D = rced_rstream_delay() samples -- zeros first, then y[i - D] --, bit for bit: every sample is the chain of
 * fused multiply-adds rced_resample runs.  D is the smallest delay at which a push reaches only frames already pushed:
 * floor(right * p / q) with right = width - 1 - left of rced_resample_taps (63 for 16 k -> 8 k and 48 k -> 8 k, 128 for 8 k -> 16 k,
 * 384 for 8 k -> 48 k).  Source and output formats, downmix and scaling as in rced_resample.  All state lives on the device (per
 * lane the units pushed and the last ceil(D q / p) + left frames in float64); after rced_rstream_create a push is one launch on the
 * caller's stream, allocates nothing, does not synchronise and can be captured.  A stream object is not thread-safe. ---- */
typedef struct rced_rstream rced_rstream;

/* lanes 1..65536, pushes of at most max_units units.  RCED_ERR_ARG, before a device is looked for: units that do not stand in the
 * ratio, and what rced_resample_taps refuses (the message names the ratio).  The first stream of a ratio on a device uploads its table. */
int rced_rstream_create(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int unit_in, int unit_out,
                        int lanes, int max_units, int device, rced_rstream** out);
/* The same with a delay of the caller's, D <= delay (less is RCED_ERR_ARG); delay < 0: D.  The history grows with it.  The streaming
 * denoiser's down lanes run at 128, a whole hop, so that every hop they hand on is a whole hop of the 8 kHz signal. */
int rced_rstream_create_ex(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int unit_in, int unit_out,
                           int lanes, int max_units, int delay, int device, rced_rstream** out);
void rced_rstream_destroy(rced_rstream* h);
/* D, in output samples; -1 for NULL. */
int rced_rstream_delay(const rced_rstream* h);

/* pcm_dev [lanes, K * unit_in, channels] of src_dtype: the next K units of every lane; out_dev [lanes, K * unit_out] of out_dtype.
 * active_dev: NULL (every lane) or [lanes] int32 flags; a lane flagged 0 is idle: its state does not change, its input row is not
 * read and zeros are written to its output row.  K < 1 or K > max_units: RCED_ERR_ARG.  Asynchronous. */
int rced_rstream_push(rced_rstream* h, const void* pcm_dev, const int* active_dev, int K, void* out_dev, void* stream);

/* Ends the utterance of every lane whose tail_counts_dev entry is 0 .. unit_in - 1: tail_dev [lanes, unit_in, channels] holds that
 * many last frames.  out_dev [lanes, unit_out + D] receives from column 0 the M - max(0, H * unit_out - D) samples still owed,
 * computed with zeros past L, zeros behind them; out_counts_dev [lanes] int32 that count.  The lane is then reset for a new
 * utterance.  Entry -1 (or any other value): the lane is left alone (count 0).  Asynchronous. */
int rced_rstream_finish(rced_rstream* h, const void* tail_dev, const int* tail_counts_dev, void* out_dev, int* out_counts_dev,
                        void* stream);

/* started_dev [lanes] int32 = 1 where the lane is active (active_dev as in rced_rstream_push) and has taken at least one unit since
 * the start of its utterance, else 0: what the next push's first unit_out samples of a lane at a delay >= unit_out are -- signal, or
 * the zeros of the delay.  One small launch, asynchronous. */
int rced_rstream_started(rced_rstream* h, const int* active_dev, int* started_dev, void* stream);

/* Back to the start of an utterance without output: lane, or -1 for every lane.  Ordered on the stream of the latest push / finish. */
int rced_rstream_reset(rced_rstream* h, int lane);

/* ---- free-running resampler: the same conversion for audio that arrives in pieces of any size, without a delay.  A
 * lane counts in frames.  With right = width - 1 - left of rced_resample_taps, output m of y = rced_resample(x) reads frames up to
 * floor(m q / p) + right, so after F frames exactly A(F) = ceil((F - right) p / q) outputs (0 for F <= right) are final; a push
 * computes the new ones, [A(F), A(F + count)), each by the chain of fused multiply-adds rced_resample runs, into a ring on the device
 * and hands out of the ring as many samples as the caller takes.  The ring starts an utterance holding `prefill` zeros.  What a lane
 * hands out, from the start of an utterance to the end of its rced_rfree_finish, is `prefill` zeros and then y, M =
 * rced_resample_length(L) samples, bit for bit.  The ring holds prefill + A(F) - (samples taken) samples, a function of numbers the
 * caller knows: the caller keeps count, takes no more than is there and leaves no more than the capacity (rced_rfree_plan) less what
 * the next push adds -- at most ceil(max_frames p / q).  A take beyond what is there hands out zeros for the rest and does not move
 * past the ring's end; no call reads or writes outside the ring.  sr_in == sr_out passes samples through exactly (a re-blocker).
 * Source and output formats, downmix and scaling as in rced_resample.  All state lives on the device (per lane the frames taken, the
 * samples handed out, the last width - 1 frames in float64 and the ring); after rced_rfree_create a push is one launch on the
 * caller's stream, allocates nothing, does not synchronise and can be captured.  An object is not thread-safe. ---- */
typedef struct rced_rfree rced_rfree;

/* A(frames) for the ratio: host arithmetic, no device.  -1 (and rced_last_error) for what rced_resample_taps refuses or frames < 0. */
long long rced_rfree_available(int sr_in, int sr_out, long long frames);

/* The sizes rced_rfree_create would give lanes of these arguments, without a device; any pointer may be NULL.  history: frames a lane
 * keeps (width - 1); tile: outputs per staging pass; capacity: the ring's, prefill + ceil(max_frames p / q) + max_take samples;
 * finish_max: samples per lane of rced_rfree_finish's out_dev.  Refuses what rced_rfree_create refuses. */
int rced_rfree_plan(int sr_in, int sr_out, int out_dtype, int lanes, int max_frames, int max_take, int prefill, int* history, int* tile,
                    int* capacity, int* finish_max);

/* lanes 1..65536; a push brings at most max_frames >= 1 frames and takes at most max_take >= 1 samples per lane; prefill >= 0.
 * RCED_ERR_ARG, before a device is looked for: bad formats and sizes, and what rced_resample_taps refuses (the message names the
 * ratio).  The first object of a ratio on a device uploads its table. */
int rced_rfree_create(int sr_in, int sr_out, int channels, int src_dtype, int out_dtype, int lanes, int max_frames, int max_take,
                      int prefill, int device, rced_rfree** out);
void rced_rfree_destroy(rced_rfree* h);

/* pcm_dev [lanes, in_cols, channels] of src_dtype, 0 <= in_cols <= max_frames; counts_dev: NULL (in_cols frames each) or [lanes] int32,
 * the frames lane s brings, 0 .. in_cols (more counts as in_cols); a negative count is an idle lane: its state does not change, its
 * input row is not read and zeros are written to its output row.  out_dev [lanes, out_cols] of out_dtype, 0 <= out_cols <= max_take;
 * take_dev: NULL (out_cols each) or [lanes] int32, the samples lane s hands out into out_dev[s, :take], zeros behind them.  A pointer
 * may be NULL where its column count is 0.  Asynchronous. */
int rced_rfree_push(rced_rfree* h, const void* pcm_dev, int in_cols, const int* counts_dev, void* out_dev, int out_cols,
                    const int* take_dev, void* stream);

/* Ends the utterance of every lane whose tail_counts_dev entry is 0 .. in_cols: tail_dev [lanes, in_cols, channels] holds that many
 * last frames (in_cols <= max_frames).  out_dev [lanes, finish_max] receives from column 0 what is in the ring and behind it the
 * outputs up to M, computed with zeros past L, zeros behind them; out_counts_dev [lanes] int32 that count, prefill + M - (samples
 * taken).  The lane is then at the start of an utterance.  Any other entry: the lane is left alone (count 0).  Asynchronous. */
int rced_rfree_finish(rced_rfree* h, const void* tail_dev, int in_cols, const int* tail_counts_dev, void* out_dev, int* out_counts_dev,
                      void* stream);

/* Back to the start of an utterance without output: lane, or -1 for every lane.  Ordered on the stream of the latest push / finish. */
int rced_rfree_reset(rced_rfree* h, int lane);

/* ---- training step: FullyCNNTrainer.creat_graph + train_step,
 * model_utils/trainer.py:156-192, over Model(is_training=True).  Layer-by-layer, correctness first. ---- */
typedef struct rced_trainer rced_trainer;

/* blob: the same TF-variable blob rced_create takes (initial values, incl. BN moving statistics);
 * batch_size: the CONFIGURED batch size the loss divides by (trainer.py:146-147), not the dynamic N.
 * Which kernel every layer gets under the RCED_TRAIN_* switches is planned here, once; a combination of net, switches and
 * built kernels that cannot be planned is refused with RCED_ERR_STATE (RCED_ERR_ARG: a layer too large for the direct
 * kernels) instead of failing inside a step.  The three nets plan under every switch combination.  A device allocation
 * that fails here returns RCED_ERR_ALLOC, as everywhere else in the library. */
int rced_train_create(int variant, const float* blob, size_t n_floats, int batch_size, int device,
                      rced_trainer** out);
void rced_train_destroy(rced_trainer* t);

/* sess.run([loss, global_step, train_op]) (trainer.py:181-192) with the UPDATE_OPS: forward with batch
 * statistics, loss = sum((y - pred)^2) / batch_size, backward, tf.train.AdamOptimizer(lr) step in TF's
 * form (beta1 0.9, beta2 0.999, eps 1e-8), moving mean / variance update (momentum 0.99; behind Adam: a
 * step that returns an error has changed neither).
 * x_dev, y_dev: DEVICE [N, T, 129, 1] float32.  lr: the value fed to the learning-rate placeholder.
 * *loss_out (host) receives the batch loss.  Synchronises the stream. */
int rced_train_step(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr,
                    double* loss_out, void* stream);

/* FullyCNNTrainer.valid_step (trainer.py:245-250): sess.run(self.pred) on the TRAINING graph, i.e. the model
 * built with is_training=True -- BatchNorm normalises with the statistics of the batch it is given, and because
 * only pred is fetched nothing is updated (no UPDATE_OPS, no optimizer step).  x_dev, pred_dev: DEVICE
 * [N, T, 129, 1] float32.  Synchronises the stream. */
int rced_train_forward(rced_trainer* t, const float* x_dev, float* pred_dev, int N, int T, void* stream);

/* ---- the step in shards (gradient accumulation on one device, data-parallel ranks): one optimizer step over a batch
 * that arrives as shards s = 0 .. S-1 of [N_s, T_s, 129, 1].  Per shard: the forward with BatchNorm normalising by THAT
 * shard's statistics, loss_s = sum((y_s - pred_s)^2) / batch_size, and its gradient g_s by the step's own kernels.  The
 * step's gradient is G = ((g_0 + g_1) + g_2) + ... in fp32 in shard order; every BatchNorm channel's fp64 sums (sum z,
 * sum z^2) and the pixel count are added over the shards in fp64 in shard order, and the moving statistics are updated
 * once from the totals (they follow the union batch); Adam runs once from G.  With one shard all of it is rced_train_step,
 * bit for bit.
 *
 * The two caller-owned exchange buffers: n_floats float32 (the gradient, in blob order) and n_doubles float64 (per
 * BatchNorm layer in layer order: (sum z, sum z^2) per channel, interleaved, then the pixel count).  The layout depends
 * on the variant alone; adding two buffers elementwise is the sum of the shards. */
int rced_train_exchange_size(rced_trainer* t, size_t* n_floats, size_t* n_doubles);

/* One shard: forward, loss and backward of (x_dev, y_dev), DEVICE [N, T, 129, 1] float32.  accumulate == 0: g_dev / s_dev
 * (device) are overwritten with this shard's gradient and sums; otherwise the shard is added to them (g += g_s, s += s_s,
 * one element per thread).  *loss_out (host) receives loss_s.  Nothing else changes: variables, Adam slots, moving
 * statistics and global_step stay as they are.  RCED_ERR_ARG for a NULL handle or buffer, N <= 0 or T <= 0.
 * Synchronises the stream. */
int rced_train_grad(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                    int accumulate, double* loss_out, void* stream);

/* rced_train_step / rced_train_grad with the objective
 *   loss = w_spectral * sum((target - M)^2) / B + w_sse * sum_n wave_sse_n / B - w_si_sdr * sum_valid si_sdr_n / B,
 * M the net's prediction, B the trainer's batch_size, wave_sse_n and si_sdr_n rced_wave_loss's terms of utterance n on the rebuilt
 * prediction (default framing only; the definition is there).  The weights are finite, >= 0 and not all zero; (1, 0, 0) is
 * rced_train_step's loss.  Pure SI-SDR leaves the output's scale free while inference uses the mask as a magnitude: that is why
 * the terms mix.  phase_dev [N,T,129,2] float32: the mixture's unit phase; clean_dev: N rows of clean_stride floats; lengths_dev
 * [N] int32: samples per utterance; frames_dev [N] int32 or NULL (= rced_stft_num_frames(length)); all DEVICE memory, read by this
 * call only, and needed only where w_sse or w_si_sdr has a weight.  y_dev may be NULL when w_spectral = 0.  Anything else is
 * RCED_ERR_ARG before any device work.  The pass is rced_train_step's up to the loss: there the spectral term's
 * kernel runs at w_spectral / B (if it has a weight), then rced_wave_loss's launches on the prediction, their gradient added to the
 * spectral term's; everything behind is unchanged.  *loss_out (host): the objective; parts_out: NULL or 3 doubles (host) receiving
 * the unweighted sums sum((target - M)^2), sum_n wave_sse_n, sum_valid si_sdr_n of this call's rows.  Deterministic as the step
 * is.  The synchronised pass (rced_train_sync_*) has no such form. */
typedef struct rced_wave_args {
  double w_spectral, w_sse, w_si_sdr;
  int skip_edges; /* 1: score only the hops two frames cover; 0: the whole rebuilt signal */
  const float* phase_dev;
  const float* clean_dev;
  int clean_stride;
  const int* lengths_dev;
  const int* frames_dev;
} rced_wave_args;
int rced_train_step_wave(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr,
                         const rced_wave_args* wave, double* loss_out, double* parts_out, void* stream);
int rced_train_grad_wave(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                         int accumulate, const rced_wave_args* wave, double* loss_out, double* parts_out, void* stream);

/* ... at a framing: the wave terms are rced_wave_loss_fr's at (window, stride, window_name), frames_dev = NULL meaning
 * rced_stft_num_frames_fr(length, window, stride); the pass differs at the same one place.  They always run the general kernels, at
 * 256 / 128 / hamming too.  A framing rced_framing_check refuses is RCED_ERR_ARG before anything else is looked at. */
int rced_train_step_wave_fr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr,
                            const rced_wave_args* wave, int window, int stride, int window_name, double* loss_out,
                            double* parts_out, void* stream);
int rced_train_grad_wave_fr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                            int accumulate, const rced_wave_args* wave, int window, int stride, int window_name, double* loss_out,
                            double* parts_out, void* stream);

/* ... with the multi-resolution STFT term (rced_wave_loss_mr) on the rebuilt prediction:
 *   loss = w_spectral sum((target - M)^2) / B + w_sse sum_n wave_sse_n / B - w_si_sdr sum_valid si_sdr_n / B + w_mr sum_valid mr_stft_n / B.
 * The _fr entries with the resolutions and 4 doubles in parts_out (the fourth: sum_valid mr_stft_n).  The four weights must not all
 * be zero; phase_dev, clean_dev and lengths_dev are needed where w_sse, w_si_sdr or w_mr has a weight; y_dev may be NULL when
 * w_spectral = 0.  What rced_framing_check or rced_mr_stft_check refuses is RCED_ERR_ARG before anything else is looked at. */
int rced_train_step_wave_mr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr,
                            const rced_wave_args* wave, int window, int stride, int window_name, const rced_mr_args* mr,
                            double* loss_out, double* parts_out, void* stream);
int rced_train_grad_wave_mr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                            int accumulate, const rced_wave_args* wave, int window, int stride, int window_name,
                            const rced_mr_args* mr, double* loss_out, double* parts_out, void* stream);

/* The moving-statistics update from s_dev (momentum 0.99, unbiased variance, by the step's expressions), then the Adam
 * step from g_dev with the fed learning rate; global_step += 1.  Afterwards rced_train_get_gradients returns g_dev's
 * content.  Buffers no rced_train_grad has filled are the caller's error and are not detected.  Synchronises the stream. */
int rced_train_apply(rced_trainer* t, const float* g_dev, const double* s_dev, float lr, void* stream);

/* ---- the synchronised step: rced_train_grad with every BatchNorm layer normalising by, and differentiating through, the
 * statistics of the UNION of the shards, so that the step over the shards is the unsharded step over the whole batch up to
 * the rounding of a few fp64 additions.  The pass of one shard stops at every exchange point -- each BatchNorm layer once
 * in the forward, with the raw (sum z, sum z^2) per channel, and once in the backward, with the raw (sum d_u, sum d_u z) or
 * (sum d_u, sum d_u x) -- and leaves those sums in the caller's device buffer xs_dev (interleaved per channel of the
 * even-padded internal layout, n_doubles doubles, the tail unused).  The caller replaces xs_dev by the sum over all shards,
 * on the pass's stream, and resumes; the layer is then finished with pixels_total, the pixel count of all shards
 * (sum of N_s * T_s * 129), in place of the shard's own.  Every shard of a step stops at the same points in the same order
 * (which kernels run is a matter of the variant and the variables alone).  With one shard, pixels_total its own count and
 * xs_dev left as it is, the pass is rced_train_grad bit for bit.
 *
 *   rced_train_sync_points   the exchange points of a pass (2 per BatchNorm layer) and the size of xs_dev in doubles
 *   rced_train_sync_begin    packs the weights and runs to the first exchange point.  Asynchronous.  RCED_ERR_STATE where the
 *                            handle's plan has a layer whose sums are not formed from records (RCED_TRAIN_MFMA=0)
 *   rced_train_sync_next     xs_dev holds the shards' sum: finishes that point and runs to the next.  *more = 0 once the
 *                            backward is through.  Asynchronous.  An error ends the pass
 *   rced_train_sync_end      what the end of rced_train_grad does: the shard's own gradient -- d gamma and d beta are the
 *                            shard's own sums, so the sum over shards makes them the batch's -- and its own (sum z, sum z^2,
 *                            pixels) into g_dev / s_dev (accumulate as there), *loss_out = loss_s.  Synchronises the stream.
 *                            RCED_ERR_STATE while exchange points are left
 *   rced_train_sync_abort    leaves a pass that was begun, at any point; synchronises its stream.  Without one: RCED_OK
 *
 * While a pass is open, every other entry point that takes the handle and touches its state (step, forward, grad, apply,
 * get_* / set_state, copy_variables, a second begin) returns RCED_ERR_STATE and says that a pass is pending. */
int rced_train_sync_points(rced_trainer* t, int* n_points, size_t* n_doubles);
int rced_train_sync_begin(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, double pixels_total,
                          double* xs_dev, void* stream);
int rced_train_sync_next(rced_trainer* t, int* more);
int rced_train_sync_end(rced_trainer* t, float* g_dev, double* s_dev, double* loss_out, int accumulate);
int rced_train_sync_abort(rced_trainer* t);
/* xs_dev[i] = ((g[0][i] + g[1][i]) + g[2][i]) + ... for i < n_doubles, the shards' rows `stride` doubles apart in
 * gathered_dev (stride >= n_doubles): the ordered sum of an exchange point in one launch.  Asynchronous. */
int rced_train_sync_reduce(rced_trainer* t, const double* gathered_dev, int shards, size_t stride, double* xs_dev, void* stream);
/* dst's variables (moving statistics included) := src's; two trainers of one variant on one device.  Adam slots and
 * global_step stay dst's own.  Asynchronous. */
int rced_train_copy_variables(rced_trainer* dst, rced_trainer* src, void* stream);

long long rced_train_global_step(rced_trainer* t);
/* Read-only, no device work: over the tile-walking launchers of the last pass on the handle (step, grad, forward; the
 * persistent MFMA kernels that walk two-frame tiles, and the output layer's wgrad, whose waves stride over frames),
 * *max_grid = the largest workgroup count one of them was launched with and *max_tiles_per_workgroup = the largest
 * ceil(tiles / workgroups), i.e. the longest walk.  Both 0 before the first pass and where no such launcher ran
 * (RCED_TRAIN_MFMA=0).  What RCED_TRAIN_MAX_GRID made of a step: the tests of the tile walks assert both. */
int rced_train_grid_stats(rced_trainer* t, int* max_grid, int* max_tiles_per_workgroup);
/* Current variables / last gradients, in blob order (gradients of moving statistics are 0). */
int rced_train_get_variables(rced_trainer* t, float* blob_host, size_t n_floats);
int rced_train_get_gradients(rced_trainer* t, float* blob_host, size_t n_floats);
/* Optimizer state, to save / resume a run as the reference does (trainer.py:50-65: tf.train.Saver(tf.global_variables())
 * stores the Adam slots "<var>/Adam", "<var>/Adam_1" and global_step next to the model variables).  m / v: first and
 * second moments in variable-blob order (entries of non-trainable variables are unused). */
int rced_train_get_state(rced_trainer* t, float* m_blob_host, float* v_blob_host, size_t n_floats, long long* global_step);
int rced_train_set_state(rced_trainer* t, const float* m_blob_host, const float* v_blob_host, size_t n_floats,
                         long long global_step);

/* The single op with is_training=True (module.py:29 `training=is_training`): BatchNorm normalises with the mean and the
 * BIASED variance of this batch over N*T*F (eps 1e-3), then + skip_input, then ReLU.  gamma_beta: gamma[cout], beta[cout]
 * (device).  batch_mean_var_out: NULL, or device [2*cout] receiving (mean, biased variance) -- what TF's UPDATE_OPS fold
 * into moving_mean / moving_variance (momentum 0.99; the variance Bessel-corrected by the fused kernel); the op itself
 * updates nothing, as the TF op does not unless the UPDATE_OPS are run.  use_norm=False has no training form: use
 * rced_conv_bn_relu with bn = NULL.  Direct-convolution kernels; synchronises the stream. */
int rced_conv_bn_relu_train(const float* x, float* y, const float* kernel, const float* bias, const float* gamma_beta,
                            const float* skip_input, int use_act, int N, int T, int F, int cin, int cout, int kh, int kw,
                            float* batch_mean_var_out, int device, void* stream);

/* Average device time (ms) of the dominant kernel of the last rced_forward, measured with HIP
 * events on the launch stream when profiling is on ("profile" option = 1).  <0 if none. */
float rced_last_kernel_ms(rced_model* m);

/* HIP-event profiler ("profile" option = 1 arms it and clears old samples): total device time
 * and launch count of kernel kind 0 = generic layer, 1 = fused multi-layer kernel, 2 = final
 * 1x129 Toeplitz GEMM, over every rced_forward since it was armed.  Synchronises. */
int rced_profile_query(rced_model* m, int kind, float* total_ms, int* launches);

/* Thread-local description of the last error on this thread ("" if none). */
const char* rced_last_error(void);

/* Library / build identification, e.g. "rced-hip 0.1 gfx950". */
const char* rced_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RCED_H_ */
