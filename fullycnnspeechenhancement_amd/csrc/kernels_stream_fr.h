// Streaming denoiser at any framing (W, S, window name), 2 <= W <= 256, 1 <= S <= W, R = ceil(W / S) <= 8: the general stateful front
// and back end beside the ones specialised for 256 / 128 / hamming (kernels_stream.h, kernels_stream_ola.h), which stay what
// rced_stream_create / _ex run.  DESIGN.md 3.4j; the arithmetic (delay, state layout, finish rows, owed samples) is stream_fr_plan.h.
//
// A lane is one audio stream; audio arrives in hops of S samples and leaves R + 3 hops later.  One push of K hops to a lane that has
// seen H hops (frame t = samples tS .. tS + W - 1; hop g completes frame g - R + 1) is FOUR launches, always:
//   stream_fr_stft_kernel     frames H - R + 1 .. H + K - R -> rows 7 .. 6 + K of the lane's window [7 + K, 129]; rows 0 .. 6 = the 7 kept
//                             frames, so row r holds frame H - R - 6 + r.  A frame is staged one aligned row (kernels_framing.h), from
//                             the lane's kept tail (the last (R - 1) S pre-emphasised samples) and the new hops; slots at and past W,
//                             samples past the utterance's end and frames with a negative index or at and past the utterance's count
//                             are zeros.  The three-part DFT GEMM and stft_store, with the framing's window pack.
//   rced_forward              on [lanes, 7 + K, 129]: rows 3 .. K + 2 (frames H - R - 3 .. H + K - R - 4) have seen 3 past, 4 future frames.
//   stream_fr_frames_kernel   slot p = window row p + 3 = frame H - R - 3 + p -> Y[lane][p][r] = sum_k C[r][k] X[k], r < W, the row scale (w
//                             for overlap-add, 1 / w for the reference rebuild, 1 / 256 and irfft's 2) in the pack, the rank-1 term of
//                             im(bin 128) at nfft = 512: frames_fr_kernel's GEMM over the lanes' slots, into the stream's scratch
//                             (allocated at create).  A slot without a frame to rebuild (an idle lane, a frame index below 0 or at and
//                             past the utterance's count T) is staged as zeros, never loaded, and not stored.
//   stream_fr_rebuild_kernel  one workgroup per lane.  Output sample j of the push is sample (H - R - 3) S + j of the utterance; it gathers
//                             its addends in ASCENDING FRAME ORDER: first the lane's pending sum (frames of earlier pushes, themselves
//                             summed in ascending order), then this push's frames that cover it -- so the sum is the offline kernel's,
//                             term for term, however the hops were cut into pushes.  Overlap-add divides by the sum of w^2 over the
//                             frames 0 <= t < T that cover the sample (0 where that is at most 1e-10); the reference rebuild has one
//                             addend per sample (the frame de_frame keeps).  Then deemph_scan from the lane's carry, 8,192 samples a
//                             step, and the lane's new state.
// A finish is a push of R + 4 hops made of the tail and zeros (T = the utterance's frame count), and returns the state to zero.
// No atomics, one summation order; a lane's bits depend on its own state and input only.  Nothing but the last kernel writes the
// lane's state, and every lane's state is written by the one workgroup that owns the lane.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_audio_x6.h"
#include "kernels_stream.h"
#include "lds_dma.h"
#include "stream_fr_plan.h"

namespace rced {
namespace audio {
namespace stream {
namespace fr {

// the plan's state layout and index functions (declared here, so that they hide kernels_stream.h's layout of the same names)
namespace plan = ::rced::stream_fr;
using plan::kStHops; using plan::kStSample; using plan::kStCarry; using plan::kStTail; using plan::kStPend; using plan::kStPhase;
using plan::kStMag; using plan::kStFloats; using plan::kMaxWindow; using plan::kMaxFinishSlots; using plan::overlap;
using plan::delay_hops; using plan::tail_len; using plan::pend_len; using plan::finish_max; using plan::num_frames; using plan::owed;
using plan::finish_skip;

constexpr int kNoEnd = 0x7fffffff;                               // T of a push
constexpr int kStftLds = 3 * kXPartB;                            // the three images
constexpr int kFramesLds = 3 * kXPartB + kFramesPerWg * 4;       // + im of bin 128 per slot
constexpr int kChunk = kThreadsX * kDeBlock;                     // samples per step of the rebuild's walk: 8,192
static_assert(kChunk == kFramesPerWg * kStep, "deemph_scan's staging holds one chunk");
static_assert(kMaxFinishSlots * kMaxWindow <= kChunk, "a finish is one step of the rebuild");
static_assert(plan::kKeep == kKeep && plan::kMaxHops == kMaxHops && plan::kBins == kBins && kMaxWindow == kFrame,
              "stream_fr_plan.h and kernels_stream.h");

// what a lane's flag means: push: active (null: every lane); finish: the tail's count, -1 = not finishing
struct LaneIn {
  bool on;
  int fresh;   // new samples at `in`: K S of a push, the tail's r of a finish
  int T;       // the utterance's frame count (finish), kNoEnd (push)
};
__device__ __forceinline__ LaneIn lane_in(const int* __restrict__ flags, int s, int finish, int H, int K, int W, int S) {
  const int flag = flags ? flags[s] : 1;
  LaneIn l;
  if (finish) {
    l.on = flag >= 0;
    l.fresh = l.on ? min(flag, S - 1) : 0;
    l.T = num_frames((long long)H * S + l.fresh, W, S);
  } else {
    l.on = flag != 0;
    l.fresh = K * S;
    l.T = kNoEnd;
  }
  return l;
}

// in: pcm [lanes, K S] (push) or the tails [lanes, S] (finish, K = R + 4 slots); flags as lane_in.  win [lanes, 7 + K, 129], phw
// [lanes, 7 + K, 129, 2].  grid (ceil(lanes K / 64), 2 M-groups), dynamic LDS kStftLds.  apack: the framing's STFT pack (16 M-tiles,
// w folded in, columns past W zero).
__global__ __launch_bounds__(kThreadsX) void stream_fr_stft_kernel(const float* __restrict__ in, const int* __restrict__ flags, int finish,
                                                                    const unsigned short* __restrict__ apack,
                                                                    const float* __restrict__ state, int lanes, int K, int W, int S,
                                                                    float* __restrict__ win, float* __restrict__ phw __attribute__((nonnull))) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int mt = blockIdx.y * kWaves + wave;
  const int j0 = blockIdx.x * kFramesPerWg, total = lanes * K, rows = kKeep + K;
  const int R = overlap(W, S), tl = tail_len(W, S);
  const int in_stride = finish ? S : K * S;
  AFrag A;
  load_a(A, apack, mt, lane);
  // the kept frames -> rows 0 .. 6 of every lane's window
  if (blockIdx.y == 0) {
    const int step = gridDim.x * kThreadsX;
    for (int i = blockIdx.x * kThreadsX + tid; i < lanes * kKeep * kBins; i += step) {
      const int s = i / (kKeep * kBins), e = i - s * (kKeep * kBins);
      const float* st = state + (size_t)s * kStFloats;
      const size_t o = (size_t)s * rows * kBins + e;
      win[o] = st[kStMag + e];
      *reinterpret_cast<f32x2*>(phw + 2 * o) = *reinterpret_cast<const f32x2*>(st + kStPhase + 2 * e);
    }
  }
  // stage the 64 frames of this block one row each, as three bf16 parts, two samples per store; zeros where there is no frame, at and
  // past W, and past the utterance's end (zero fill AFTER pre-emphasis)
  for (int i = tid; i < kFramesPerWg * (kFrame / 2); i += kThreadsX) {
    const int fr = i >> 7, k = 2 * (i & 127), j = j0 + fr;
    float e0 = 0.f, e1 = 0.f;
    if (j < total && k < W) {
      const int s = j / K, h = j - s * K;
      const float* st = state + (size_t)s * kStFloats;
      const int H = reinterpret_cast<const int*>(st)[kStHops];
      const LaneIn l = lane_in(flags, s, finish, H, K, W, S);
      const int t = H - R + 1 + h;
      if (l.on && t >= 0 && t < l.T) {
        const float* src = in + (size_t)s * in_stride;
        const float before = st[kStSample];
        const int g = (h - R + 1) * S + k;   // relative to the first new sample
        auto at = [&](int gg) -> float {
          if (gg < 0) return st[kStTail + tl + gg];
          return gg < l.fresh ? pre_emph(src, gg, before, H == 0) : 0.f;
        };
        e0 = at(g);
        if (k + 1 < W) e1 = at(g + 1);
      }
    }
    put_pair(xs, kXPartB, fr * kXRowB + (i & 127) * 4, e0, e1);
  }
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
  // the offline epilogue (stft_fr_kernel's: one rounding in re^2 + im^2), every frame live: one staged as zeros leaves as zero
  // magnitude, phase 1 + 0j
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + n;
    if (j >= total) continue;
    const int s = j / K, h = j - s * K;
    stft_store(acc[t], true, true, mt, kq, ((size_t)s * rows + kKeep + h) * kBins, win, phw);
  }
}

// y: the masks [lanes, 7 + K, 129]; phw: the phases stream_fr_stft_kernel wrote; flags / finish as there -> Y [lanes, Kmax, 256]: samples
// r < W of the frame in slot p (window row p + 3), times the pack's row scale.  grid (ceil(lanes K / 64), 2 M-groups), dynamic LDS
// kFramesLds.  cpack: the framing's rebuild pack (16 M-tiles, K slot 2b + c, slot 1 = re of bin 128); cim: 256 floats, the
// coefficients of im(bin 128) (zeros unless nfft = 512).
__global__ __launch_bounds__(kThreadsX) void stream_fr_frames_kernel(const float* __restrict__ y, const float* __restrict__ phw,
                                                                      const int* __restrict__ flags, int finish,
                                                                      const unsigned short* __restrict__ cpack, const float* __restrict__ cim,
                                                                      const float* __restrict__ state, int lanes, int K, int Kmax, int W,
                                                                      int S, float* __restrict__ Y) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  __shared__ int sLive[kFramesPerWg];
  float* xim = reinterpret_cast<float*>(xs + 3 * kXPartB);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int mt = blockIdx.y * kWaves + wave;
  const int j0 = blockIdx.x * kFramesPerWg, total = lanes * K, rows = kKeep + K;
  if (16 * kWaves * (int)blockIdx.y >= W) return;   // (the whole workgroup: before any barrier)
  if (tid < kFramesPerWg) {
    const int j = j0 + tid;
    int live = 0;
    if (j < total) {
      const int s = j / K, p = j - s * K;
      const int H = reinterpret_cast<const int*>(state + (size_t)s * kStFloats)[kStHops];
      const LaneIn l = lane_in(flags, s, finish, H, K, W, S);
      const int t = H - delay_hops(W, S) + p;
      live = l.on && t >= 0 && t < l.T;
    }
    sLive[tid] = live;
  }
  __syncthreads();
  for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
    const int fr = i >> 7, b = i & 127;
    float v0 = 0.f, v1 = 0.f, vi = 0.f;
    if (sLive[fr]) {
      const int j = j0 + fr, s = j / K, p = j - s * K;
      slot_pair(y, phw, ((size_t)s * rows + p + 3) * kBins + b, b, v0, v1, vi);
    }
    if (b == 0) xim[fr] = vi;
    put_pair(xs, kXPartB, fr * kXRowB + b * 4, v0, v1);
  }
  __syncthreads();
  if (16 * mt >= W) return;   // a wave whose rows are all past W (no barrier follows)
  AFrag A;
  load_a(A, cpack, mt, lane);
  const f32x4 ci = *reinterpret_cast<const f32x4*>(cim + 16 * mt + 4 * kq);
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
  rank1_add(acc, ci, xim, n);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int fr = 16 * t + n;
    if (!sLive[fr]) continue;
    const int j = j0 + fr, s = j / K, p = j - s * K;
    *reinterpret_cast<f32x4*>(Y + ((size_t)s * Kmax + p) * kFrame + 16 * mt + 4 * kq) = acc[t];
  }
}

// Y [lanes, Kmax, 256] (stream_fr_frames_kernel), w2: 256 floats, w^2; in / flags / finish / win / phw as stream_fr_stft_kernel.  Push: out
// [lanes, K S].  Finish (K = R + 4): out [lanes, finish_max(W, S)] + out_counts [lanes], and the finishing lanes' state returns to
// zero.  grid (lanes).
// With q = j / S, rem = j - q S the frames that cover output sample j are slots q - m, m = 0 .. (W - 1 - rem) / S, at their sample
// rem + m S; a negative slot is a frame of an earlier push (its addend is in the pending sum), one at or past K a frame still to come.
// OLA: all of them below T add up, over the sum of w^2 of the same frames.  !OLA: de_frame (utils.py:139-147) keeps the last S samples
// of every frame, m = the largest, and of frame 0 the first W - S as well.
template <bool OLA>
__global__ __launch_bounds__(kThreadsX) void stream_fr_rebuild_kernel(const float* __restrict__ Y, const float* __restrict__ w2,
                                                                       const float* __restrict__ in, const int* __restrict__ flags,
                                                                       int finish, const float* __restrict__ win,
                                                                       const float* __restrict__ phw, float* __restrict__ state, int K,
                                                                       int Kmax, int W, int S, float* __restrict__ out,
                                                                       int* __restrict__ out_counts) {
  __shared__ __attribute__((aligned(16))) float obuf[kFramesPerWg * kORow];   // a chunk in time order, rows of 128 (deemph_scan's layout)
  __shared__ float sa[kThreadsX], sb[kThreadsX];
  __shared__ float sPend[kMaxWindow], sTail[kMaxWindow], sW2[kMaxWindow];
  const int tid = threadIdx.x, s = blockIdx.x;
  float* st = state + (size_t)s * kStFloats;
  const int H = reinterpret_cast<const int*>(st)[kStHops];
  const LaneIn l = lane_in(flags, s, finish, H, K, W, S);
  const int n_out = K * S, fmax = finish_max(W, S);
  if (!l.on) {   // an idle lane keeps its state and gets zeros (uniform over the workgroup: before any barrier)
    float* o = out + (size_t)s * (finish ? fmax : n_out);
    const int n = finish ? fmax : n_out;
    for (int i0 = 0; i0 < n; i0 += kThreadsX)   // (uniform trip counts here and below: the lane's own bound guards the store, not the loop)
      if (i0 + tid < n) {
        o[i0 + tid] = 0.f;
        store_wait_state();
      }
    if (finish && tid == 0) out_counts[s] = 0;
    return;
  }
  const int hb = H - delay_hops(W, S);   // the frame in slot 0 = the hop at output position 0
  const int T = l.T, pl = pend_len(W, S), tl = tail_len(W, S), rows = kKeep + K;
  const float sample = st[kStSample];
  float carry = st[kStCarry];
  if (tid < kMaxWindow) {
    sPend[tid] = tid < pl ? st[kStPend + tid] : 0.f;
    sTail[tid] = tid < tl ? st[kStTail + tid] : 0.f;
    sW2[tid] = w2[tid];
  }
  __syncthreads();
  const float* Yl = Y + (size_t)s * Kmax * kFrame;
  // the numerator of sample j (j < K S + W - S): the pending sum, then this push's frames in ascending order
  auto numer = [&](int j) -> float {
    const int q = j / S, rem = j - q * S, mmax = (W - 1 - rem) / S;
    float num = j < pl ? sPend[j] : 0.f;
    if (OLA) {
      for (int m = mmax; m >= 0; --m) {
        const int p = q - m, t = hb + p;
        if (p >= 0 && p < K && t >= 0 && t < T) num += Yl[p * kFrame + rem + m * S];
      }
    } else if (hb + q >= 0) {
      const int m = hb + q - mmax < 0 ? hb + q : mmax;   // frame 0's head, or the frame whose last S samples hold j
      const int p = q - m;
      if (p >= 0 && p < K && hb + p < T) num += Yl[p * kFrame + rem + m * S];
    }
    return num;
  };
  auto value = [&](int j) -> float {
    const float num = numer(j);
    if (!OLA) return num;
    const int q = j / S, rem = j - q * S, mmax = (W - 1 - rem) / S;
    float den = 0.f;
    for (int m = mmax; m >= 0; --m) {
      const int t = hb + q - m;
      if (t >= 0 && t < T) den += sW2[rem + m * S];
    }
    return den > 1e-10f ? num / den : 0.f;
  };
  for (int base = 0; base < n_out; base += kChunk) {
    __syncthreads();   // the previous chunk's reads of obuf, sa, sb are done
#pragma unroll 4
    for (int jj = 0; jj < kDeBlock; ++jj) {
      const int p = jj * kThreadsX + tid;
      obuf[(p >> 7) * kORow + (p & 127)] = base + p < n_out ? value(base + p) : 0.f;
    }
    __syncthreads();
    f32x4 yv[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, true, 0, carry, yv);
    float* own = obuf + (tid >> 3) * kORow + kDeBlock * (tid & 7);
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) *reinterpret_cast<f32x4*>(own + 4 * j4) = yv[j4];
    __syncthreads();
    const int cnt = min(kChunk, n_out - base);
    carry = obuf[((cnt - 1) >> 7) * kORow + ((cnt - 1) & 127)];   // y at the chunk's last sample (what follows it in obuf is fill)
    if (!finish) {
      float* o = out + (size_t)s * n_out + base;
      for (int p0 = 0; p0 < cnt; p0 += kThreadsX) {
        const int p = p0 + tid;
        if (p < cnt) {
          o[p] = obuf[(p >> 7) * kORow + (p & 127)];
          store_wait_state();
        }
      }
    } else {   // one chunk: the L - max(0, S H - D) samples still owed, from hop max(0, H - R - 3) on
      const int count = (int)owed(H, l.fresh, W, S), skip = finish_skip(H, W, S);
      float* o = out + (size_t)s * fmax;
      for (int i0 = 0; i0 < fmax; i0 += kThreadsX) {
        const int i = i0 + tid, p = i + skip;
        if (i < fmax) {
          o[i] = i < count ? obuf[(p >> 7) * kORow + (p & 127)] : 0.f;
          store_wait_state();
        }
      }
      if (tid == 0) out_counts[s] = count;
    }
  }
  // the lane's new state (every read of the old one is behind the first barrier, but for the hop count and the two carries in registers)
  if (finish) {   // reset for a new utterance
    for (int i0 = 0; i0 < kStFloats; i0 += kThreadsX)
      if (i0 + tid < kStFloats) {
        st[i0 + tid] = 0.f;
        store_wait_state();
      }
    return;
  }
  const float* src = in + (size_t)s * n_out;
  // (each guarded store carries its wait state: the next guard's compare may be scheduled in front of it, lds_dma.h)
  if (tid < pl) {
    st[kStPend + tid] = numer(n_out + tid);
    store_wait_state();
  }
  if (tid < tl) {
    const int g = n_out - tl + tid;
    st[kStTail + tid] = g >= 0 ? pre_emph(src, g, sample, H == 0) : sTail[tid + n_out];
    store_wait_state();
  }
  const size_t o0 = ((size_t)s * rows + K) * kBins;   // the 7 newest frames of the window
  for (int i0 = 0; i0 < kKeep * kBins; i0 += kThreadsX) {
    const int i = i0 + tid;
    if (i < kKeep * kBins) {
      st[kStMag + i] = win[o0 + i];
      *reinterpret_cast<f32x2*>(st + kStPhase + 2 * i) = *reinterpret_cast<const f32x2*>(phw + 2 * (o0 + i));
      store_wait_state();
    }
  }
  if (tid == 0) {
    reinterpret_cast<int*>(st)[kStHops] = H + K;
    st[kStSample] = src[n_out - 1];
    st[kStCarry] = carry;
  }
}

}  // namespace fr
}  // namespace stream
}  // namespace audio
}  // namespace rced
