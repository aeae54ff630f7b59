// Streaming denoiser: the stateful STFT front end and ISTFT back end around the unchanged CNN forward.
// A lane is one audio stream; audio arrives in hops of 128 samples and leaves 5 hops (640 samples) later.  Same reference rows as
// kernels_audio_x6.h.  Both GEMMs are x6_dft.h's (three-part bf16 operands, six products per term), and everything around them that
// the offline kernels do as well is the device function they call: stft_store, slot_pair, rank1_add, head_spectrum / head_sample /
// head_deemph, deemph_scan (kernels_audio_x6.h).  So a frame's spectrum comes out of the same code as in stft_x6_kernel, whatever was
// pushed with it.  What is stateful is here: frame_sample, the lanes' bookkeeping, sample_at, the state update.
//
// One push of K hops to a lane that has seen H hops (frame t = hops t, t + 1; hop g completes frame g - 1):
//   stream_stft_kernel   frames H - 1 .. H + K - 2 -> rows 7 .. 6 + K of the lane's window [7 + K, 129]; rows 0 .. 6 = the 7 kept frames,
//                        so row r holds frame H - 8 + r.  Frames with a negative index are zero rows: the time padding of the first layer.
//   rced_forward         on [S, 7 + K, 129]: rows 3 .. K + 2 (frames H - 5 .. H + K - 6) have seen their 3 past and 4 future frames.
//   stream_istft_kernel  slot p = window row p + 3 = frame H - 5 + p -> samples 128 .. 255 of its irfft = hop H - 4 + p of the result;
//                        frame 0 also gives hop 0 (its samples 0 .. 127, "the head").  Output position p of the push is hop H - 5 + p:
//                        position 0 is the hop the previous push left pending, position p >= 1 is slot p - 1, slot K - 1 becomes the
//                        pending hop.  De-emphasis runs through the slots in time order from the pending hop's last sample.
// Nothing but the last kernel writes the lane's state, and every lane's state is written by the one workgroup that owns the lane.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_audio_x6.h"

namespace rced {
namespace audio {
namespace stream {

using namespace x6;

constexpr int kKeep = 7;          // frames kept in front of the new ones: 3 past + 4 future of the first layer
constexpr int kDelayHops = 5;     // RCED_STREAM_DELAY / 128
constexpr int kFinishSlots = 6;   // finish: frames H - 5 .. H
constexpr int kMaxHops = kFramesPerWg;   // a lane's slots of one push sit in one workgroup
constexpr int kFinishOut = 6 * kStep;    // floats per lane of rced_stream_finish's output (owed <= 767)

// per-lane state, floats; all zero = the start of an utterance
constexpr int kStHops = 0;                                  // int: hops pushed
constexpr int kStSample = 1;                                // the last input sample (pre-emphasis carry)
constexpr int kStCarry = 2;                                 // overlap-add streams only: the de-emphasis carry (word 3 is unused)
constexpr int kStPrevE = 4;                                 // the previous hop, pre-emphasised
constexpr int kStPend = kStPrevE + kStep;                   // the pending output hop, de-emphasised; its last sample is the carry
                                                            // (overlap-add streams: the newest frame's second-half addend, kernels_stream_ola.h)
constexpr int kStPhase = kStPend + kStep;                   // phase of the 7 kept frames [7, 129, 2]
constexpr int kStMag = kStPhase + kKeep * kBins * 2;        // magnitude of the 7 kept frames [7, 129]
constexpr int kStFloats = (kStMag + kKeep * kBins + 3) & ~3;
static_assert(kStPhase % 2 == 0 && kStFloats % 2 == 0, "phase pairs stay 8-byte aligned");

constexpr int kStreamStftLds = 3 * kXPartB;
constexpr int kHRow = kStep + 1;                            // a head per lane of the workgroup, one bank apart
constexpr int kStreamIstftLds = 3 * kXPartB + (kFramesPerWg + 2 * kBins + 2 + kFramesPerWg * kHRow) * 4;
static_assert(kStreamIstftLds <= 160 * 1024, "LDS of one CU");

// e[i] of a hop: ONE float32 multiply and ONE float32 subtract, as stft_x6_kernel does it; only a lane's very first sample is e = s
__device__ __forceinline__ float pre_emph(const float* __restrict__ hop0, int i, float before, bool first) {
  const float s = hop0[i];
  if (first && i == 0) return s;
  return __fsub_rn(s, __fmul_rn(kPre, i > 0 ? hop0[i - 1] : before));
}

// Sample k (0 .. 255) of the frame in slot h of a lane, pre-emphasised.  Push: first half = hop h - 1 of this push (h = 0: the state's
// previous hop), second half = hop h.  Finish (r tail samples, zero-filled AFTER pre-emphasis): slot 0 = (previous hop, tail), slot 1 =
// (tail, zeros).
__device__ __forceinline__ float frame_sample(const float* __restrict__ in, const float* __restrict__ st, bool finish, int r, int H, int h,
                                              int k) {
  const float before = st[kStSample];
  if (finish) {
    const int i = h == 0 ? k - kStep : k;
    if (h == 0 && k < kStep) return st[kStPrevE + k];
    if (h > 1 || i < 0 || i >= r) return 0.f;
    return pre_emph(in, i, before, H == 0);
  }
  if (k < kStep) {
    if (h == 0) return st[kStPrevE + k];
    return pre_emph(in, (h - 1) * kStep + k, before, H == 0);
  }
  return pre_emph(in, h * kStep + k - kStep, before, H == 0);
}

// A lane's state after a push of K hops, but for what the rebuild keeps (the pending hop, a carry): the 7 newest frames of its window
// (o0 = the index of bin 0 of window row K), the last hop pre-emphasised, the last sample, the hop count.  By the whole workgroup.
__device__ __forceinline__ void advance_lane(float* __restrict__ st, const float* __restrict__ src, const float* __restrict__ win,
                                             const float* __restrict__ phw, size_t o0, int K, int H, float sample, int tid) {
  for (int i = tid; i < kKeep * kBins; i += kThreadsX) {
    st[kStMag + i] = win[o0 + i];
    *reinterpret_cast<f32x2*>(st + kStPhase + 2 * i) = *reinterpret_cast<const f32x2*>(phw + 2 * (o0 + i));
  }
  if (tid < kStep) st[kStPrevE + tid] = pre_emph(src, (K - 1) * kStep + tid, sample, H == 0);
  if (tid == 0) {
    reinterpret_cast<int*>(st)[kStHops] = H + K;
    st[kStSample] = src[K * kStep - 1];
  }
}

// in: pcm [S, K * 128] (push) or the tails [S, 128] (finish, K = 6 slots); flags: push: active [S] or null, finish: tail counts [S]
// (-1 = not finishing).  win [S, 7 + K, 129], phw [S, 7 + K, 129, 2].  grid (ceil(S K / 64), 2 M-groups), dynamic LDS kStreamStftLds.
// phw nonnull (stream_api.hip allocates it with win): stft_store serves "magnitude only" too, and without the attribute the compiler
// unswitches on the pointer and keeps both forms of the epilogue here, 1,915 instructions against 1,506 (1,512 before it was shared).
__global__ __launch_bounds__(kThreadsX) void stream_stft_kernel(const float* __restrict__ in, const int* __restrict__ flags, int finish,
                                                                 const unsigned short* __restrict__ apack, const float* __restrict__ state,
                                                                 int S, int K, float* __restrict__ win,
                                                                 float* __restrict__ phw __attribute__((nonnull))) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int mt = blockIdx.y * kWaves + wave;
  const int j0 = blockIdx.x * kFramesPerWg, total = S * K, rows = kKeep + K;
  const int in_stride = finish ? kStep : K * kStep;
  AFrag A;
  load_a(A, apack, mt, lane);
  // the kept frames -> rows 0 .. 6 of every lane's window
  if (blockIdx.y == 0) {
    const int step = gridDim.x * kThreadsX;
    for (int i = blockIdx.x * kThreadsX + tid; i < S * kKeep * kBins; i += step) {
      const int s = i / (kKeep * kBins), e = i - s * (kKeep * kBins);
      const float* st = state + (size_t)s * kStFloats;
      const size_t o = (size_t)s * rows * kBins + e;
      win[o] = st[kStMag + e];
      *reinterpret_cast<f32x2*>(phw + 2 * o) = *reinterpret_cast<const f32x2*>(st + kStPhase + 2 * e);
    }
  }
  // stage the 64 frames of this block, 256 samples each, as three bf16 parts, two samples per store; zeros where there is no frame
  for (int i = tid; i < kFramesPerWg * kStep; i += kThreadsX) {
    const int fr = i >> 7, k = 2 * (i & 127), j = j0 + fr;
    float e0 = 0.f, e1 = 0.f;
    if (j < total) {
      const int s = j / K, h = j - s * K;
      const float* st = state + (size_t)s * kStFloats;
      const int H = reinterpret_cast<const int*>(st)[kStHops];
      const int flag = flags ? flags[s] : 1;
      bool live;
      int r = 0;
      if (finish) {   // contract point 2: frame H - 1 from the tail exists if the tail is not empty (or it is frame 0), frame H only as frame 0 or 1
        r = min(flag, kStep - 1);
        live = flag >= 0 && ((h == 0 && H >= 1 && (r > 0 || H == 1)) || (h == 1 && H <= 1 && r > 0));
      } else {
        live = flag != 0 && H + h >= 1;
      }
      if (live) {
        const float* src = in + (size_t)s * in_stride;
        e0 = frame_sample(src, st, finish, r, H, h, k);
        e1 = frame_sample(src, st, finish, r, H, h, k + 1);
      }
    }
    put_pair(xs, kXPartB, fr * kXRowB + (i & 127) * 4, e0, e1);
  }
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
  // the offline epilogue, every frame live (one staged as zeros leaves as zero magnitude, phase 1 + 0j), but for the two roundings
  // this kernel has always had in re^2 + im^2
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + n;
    if (j >= total) continue;
    const int s = j / K, h = j - s * K;
    stft_store(acc[t], true, false, mt, kq, ((size_t)s * rows + kKeep + h) * kBins, win, phw);
  }
}

// y: the masks [S, 7 + K, 129]; win / phw: the windows stream_stft_kernel wrote; in / flags / finish as there.  Push: out [S, K * 128].
// Finish (K = 6): out [S, 768] + out_counts [S], and the finishing lanes' state returns to zero.  Workgroup w owns lanes
// [w LPW, (w + 1) LPW), LPW = 64 / K; grid ceil(S / LPW); dynamic LDS kStreamIstftLds.
__global__ __launch_bounds__(kThreadsX) void stream_istft_kernel(const float* __restrict__ y, const float* __restrict__ win,
                                                                  const float* __restrict__ phw, const float* __restrict__ in,
                                                                  const int* __restrict__ flags, int finish,
                                                                  const unsigned short* __restrict__ cpack, const float* __restrict__ cim,
                                                                  const float* __restrict__ chead, float* __restrict__ state, int S, int K,
                                                                  float* __restrict__ out, int* __restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  __shared__ int sH[kFramesPerWg], sFlag[kFramesPerWg], sP0[kFramesPerWg];
  __shared__ float sCarry[kFramesPerWg], sSample[kFramesPerWg], sHeadLast[kFramesPerWg];
  float* xim = reinterpret_cast<float*>(xs + 3 * kXPartB);
  float* xk = xim + kFramesPerWg;                 // one frame 0's spectrum (fp32, k = 2b + c)
  float* hbuf = xk + 2 * kBins + 2;               // [lane of the workgroup][kHRow]: samples 0 .. 127 of frame 0
  float* obuf = reinterpret_cast<float*>(xs);     // [slot][kORow]: aliases the images once the GEMM has read them
  float* sa = obuf + kFramesPerWg * kORow;
  float* sb = sa + kThreadsX;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int lpw = kFramesPerWg / K, s0w = blockIdx.x * lpw, rows = kKeep + K;
  const int in_stride = finish ? kStep : K * kStep;
  AFrag A;
  load_a(A, cpack, wave, lane);
  const f32x4 ci = *reinterpret_cast<const f32x4*>(cim + 16 * wave + 4 * kq);

  // the lanes of this workgroup: hops so far, flag (0 = leave the lane alone), the slot that holds frame 0 (or -1), the two carries
  if (tid < kFramesPerWg) {
    const int s = s0w + tid;
    int H = 0, flag = 0, p0 = -1;
    float carry = 0.f, sample = 0.f;
    if (tid < lpw && s < S) {
      const float* st = state + (size_t)s * kStFloats;
      H = reinterpret_cast<const int*>(st)[kStHops];
      flag = flags ? flags[s] : 1;
      if (finish) flag = flag < 0 ? 0 : 1 + min(flag, kStep - 1);   // 1 + tail count
      if (flag && kDelayHops - H >= 0 && kDelayHops - H < K) p0 = kDelayHops - H;
      carry = st[kStPend + kStep - 1];
      sample = st[kStSample];
    }
    sH[tid] = H;
    sFlag[tid] = flag;
    sP0[tid] = p0;
    sCarry[tid] = carry;
    sSample[tid] = sample;
    sHeadLast[tid] = 0.f;
  }
  __syncthreads();

  // heads: samples 0 .. 127 of frame 0 (the only frame whose first half survives de_frame), K = 258 on the VALU, once per utterance
  for (int q = 0; q < lpw; ++q) {
    const int p0 = sP0[q];
    if (p0 < 0) continue;   // (uniform over the workgroup)
    head_spectrum(xk, y, phw, ((size_t)(s0w + q) * rows + p0 + 3) * kBins, tid, kThreadsX);
    __syncthreads();
    if (tid < kStep) hbuf[q * kHRow + tid] = head_sample(chead, xk, tid);
    __syncthreads();
  }
  // their de-emphasis: serial, the lanes side by side
  if (tid < lpw && sP0[tid] >= 0) sHeadLast[tid] = head_deemph(hbuf + tid * kHRow);

  // stage X[slot][2b + c] of the masked spectrum as three bf16 parts, im of bin 128 to xim; zeros where the slot has no frame (no lane,
  // an idle lane, a frame index below 0)
  for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
    const int fr = i >> 7, b = i & 127;
    const int q = fr / K, p = fr - q * K;
    float v0 = 0.f, v1 = 0.f, vi = 0.f;
    if (sFlag[q] && sH[q] - kDelayHops + p >= 0) slot_pair(y, phw, ((size_t)(s0w + q) * rows + p + 3) * kBins + b, b, v0, v1, vi);
    if (b == 0) xim[fr] = vi;
    put_pair(xs, kXPartB, fr * kXRowB + b * 4, v0, v1);
  }
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
  rank1_add(acc, ci, xim, n);
  __syncthreads();   // every wave has read its last fragment: the images are dead
#pragma unroll
  for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(obuf + (16 * t + n) * kORow + 16 * wave + 4 * kq) = acc[t];
  __syncthreads();

  // de-emphasis: a blocked affine scan over the 8,192 samples in slot order (thread i: samples 16 (i & 7) .. of slot i >> 3), cut into one
  // segment per lane; a lane whose frame 0 is in this push starts at that slot from its head's last sample (the slots before it are zeros)
  {
    const int fl = tid >> 3;
    const int q = fl / K, p = fl - q * K;
    const bool after_head = sP0[q] >= 0 && p >= sP0[q];
    const int seg0 = (q * K + (after_head ? sP0[q] : 0)) * 8;
    f32x4 yv[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, true, seg0, after_head ? sHeadLast[q] : sCarry[q], yv);
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) *reinterpret_cast<f32x4*>(obuf + fl * kORow + kDeBlock * (tid & 7) + 4 * j4) = yv[j4];
  }
  __syncthreads();

  // the lane's hops in time: position 0 = the pending hop, position p >= 1 = slot p - 1; the head replaces the (zero) position of hop 0
  auto sample_at = [&](int q, int s, int pos, int i) -> float {
    if (pos == sP0[q]) return hbuf[q * kHRow + i];
    if (pos == 0) return state[(size_t)s * kStFloats + kStPend + i];
    return obuf[(q * K + pos - 1) * kORow + i];
  };
  if (!finish) {
    for (int i = tid; i < lpw * K * kStep; i += kThreadsX) {
      const int q = i / (K * kStep), rem = i - q * (K * kStep), s = s0w + q;
      if (s >= S) break;
      out[(size_t)s * K * kStep + rem] = sFlag[q] ? sample_at(q, s, rem >> 7, rem & 127) : 0.f;
    }
  } else {   // the L - max(0, 128 H - 640) samples still owed, from hop max(0, H - 5) on
    for (int i = tid; i < lpw * kFinishOut; i += kThreadsX) {
      const int q = i / kFinishOut, rem = i - q * kFinishOut, s = s0w + q;
      if (s >= S) break;
      const int H = sH[q];
      const int count = sFlag[q] ? kStep * H + sFlag[q] - 1 - max(0, kStep * (H - kDelayHops)) : 0;
      const int t = rem + kStep * max(0, kDelayHops - H);
      out[(size_t)s * kFinishOut + rem] = rem < count ? sample_at(q, s, t >> 7, t & 127) : 0.f;
      if (rem == 0) out_counts[s] = count;
    }
  }
  __syncthreads();   // the old pending hops have been read

  // the lanes' new state
  for (int q = 0; q < lpw; ++q) {
    const int s = s0w + q;
    if (s >= S) break;
    if (!sFlag[q]) continue;   // an idle lane keeps its state
    float* st = state + (size_t)s * kStFloats;
    if (finish) {   // reset for a new utterance
      for (int i = tid; i < kStFloats; i += kThreadsX) st[i] = 0.f;
      continue;
    }
    if (tid < kStep) st[kStPend + tid] = obuf[(q * K + K - 1) * kORow + tid];
    advance_lane(st, in + (size_t)s * in_stride, win, phw, ((size_t)s * rows + K) * kBins, K, sH[q], sSample[q], tid);
  }
}

}  // namespace stream
}  // namespace audio
}  // namespace rced
