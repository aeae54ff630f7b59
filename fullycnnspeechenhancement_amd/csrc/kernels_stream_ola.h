// Streaming denoiser, overlap-add rebuild: the stateful back end beside stream_istft_kernel (kernels_stream.h), for streams created with
// RCED_STREAM_REBUILD_OLA.  The front end and the forward are the reference stream's; so are the slots: slot p of a
// push to a lane at H hops = window row p + 3 = frame t = H - 5 + p.  What differs is which hop a slot gives.  With w = hamming(256),
// D[s] = w[s]^2 + w[s + 128]^2, x_t = irfft(mask_t * phase_t, 256):
//   hop t = (w[s] x_t[s] + w[s + 128] x_{t-1}[s + 128]) / D[s]: the first half of frame t and the second half of frame t - 1.
// Frame t is slot p, so OUTPUT POSITION p OF THE PUSH IS SLOT p (the reference rebuild's is slot p - 1: it needs frame t - 1 alone and
// holds a finished hop back); frame t - 1 is slot p - 1 or, for p = 0, the lane's state.  Both are there after the forward, so the
// delay is the reference stream's: 640 samples.  Hop 0 has frame 0 alone, and in a finish hop T (T = the utterance's frame count) has
// frame T - 1 alone: x fix[0], x fix[1] per sample, as offline.  A hop a push emits is never the utterance's last.
// The pieces are the offline kernel's (kernels_ola_x6.h): the 16 M-tile coefficient pack with 1 / 256, irfft's factor 2, w and 1 / D
// folded in, `fix`, two GEMM passes by wave v over the same staged images (M-tiles v, v + 8: samples 16v .. 16v + 15 of both halves),
// frame_below's shuffle, the output staging behind the images.  There is no head path and no rank-1 term.
//   State: the 128 floats at kStPend hold the second-half addend of the newest frame rebuilt, NOT de-emphasised; the de-emphasis carry
//     is kStCarry.  All zero is still the start of an utterance: hops t < 0 come out as exact zeros from zero slots, a zero addend, a
//     zero carry.
//   Where streaming differs from offline: the slot below slot 0 of a lane is the NEIGHBOURING lane's last slot (one lane, or one
//     N-tile, down in the 64-slot block).  frame_below's value is dropped there; the lane's addend comes from its state instead, put
//     into the output staging before the GEMMs, when the images are staged.  So a hop is (state or 0) + first half + (slot below or
//     nothing), each lane of the wave adding to its own four words: no atomics, one order, the same bits in every slot layout.
//   Frames at or past T are staged as zeros, never loaded: after the net a zero row is not zero, and it would bleed into hop T.
// Only this kernel writes state, and each lane's state is written by the workgroup that owns it.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_ola_x6.h"
#include "kernels_stream.h"

namespace rced {
namespace audio {
namespace stream {

constexpr int kStreamOlaLds = kOlaLdsBytes;   // the three images, the output staging behind them, the scan's arrays
constexpr int kNoLastFrame = 0x7fffffff;      // T of a push

// y, win, phw, in, flags, finish, state, S, K, out, out_counts: as stream_istft_kernel.  cpack: kOlaPackX bf16; fix: [2][128] fp32.
// Workgroup w owns lanes [w LPW, (w + 1) LPW), LPW = 64 / K, slot q K + p = slot p of its lane q; grid ceil(S / LPW); dynamic LDS
// kStreamOlaLds.
__global__ __launch_bounds__(kThreadsX) void stream_istft_ola_kernel(const float* __restrict__ y, const float* __restrict__ win,
                                                                      const float* __restrict__ phw, const float* __restrict__ in,
                                                                      const int* __restrict__ flags, int finish,
                                                                      const unsigned short* __restrict__ cpack, const float* __restrict__ fix,
                                                                      float* __restrict__ state, int S, int K, float* __restrict__ out,
                                                                      int* __restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  __shared__ int sH[kFramesPerWg], sFlag[kFramesPerWg], sT[kFramesPerWg];
  __shared__ float sCarry[kFramesPerWg], sSample[kFramesPerWg];
  float* obuf = reinterpret_cast<float*>(xs + 3 * kXPartB);   // [slot][kORow], behind the images: it fills while they are still read
  float* sa = obuf + kFramesPerWg * kORow;
  float* sb = sa + kThreadsX;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int lpw = kFramesPerWg / K, s0w = blockIdx.x * lpw, rows = kKeep + K;
  const int in_stride = finish ? kStep : K * kStep;
  const int s0 = 16 * wave + 4 * kq;   // this lane's four samples of a hop
  AFrag A;
  load_a(A, cpack, wave, lane);

  // the lanes of this workgroup: hops so far, flag (0 = leave the lane alone), the utterance's frame count (finish), the two carries
  if (tid < kFramesPerWg) {
    const int s = s0w + tid;
    int H = 0, flag = 0, T = kNoLastFrame;
    float carry = 0.f, sample = 0.f;
    if (tid < lpw && s < S) {
      const float* st = state + (size_t)s * kStFloats;
      H = reinterpret_cast<const int*>(st)[kStHops];
      flag = flags ? flags[s] : 1;
      if (finish) {
        flag = flag < 0 ? 0 : 1 + min(flag, kStep - 1);   // 1 + tail count
        T = num_frames(kStep * H + flag - 1);
      }
      carry = st[kStCarry];
      sample = st[kStSample];
    }
    sH[tid] = H;
    sFlag[tid] = flag;
    sT[tid] = T;
    sCarry[tid] = carry;
    sSample[tid] = sample;
  }
  __syncthreads();

  // stage X[slot][2b + c] of the masked spectrum as three bf16 parts; zeros where the slot has no frame to rebuild (no lane, an idle
  // lane, a frame index below 0, one at or past T)
  for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
    const int fr = i >> 7, b = i & 127;
    const int q = fr / K, p = fr - q * K;
    const int t = sH[q] - kDelayHops + p;
    float v0 = 0.f, v1 = 0.f, vi = 0.f;
    if (sFlag[q] && t >= 0 && t < sT[q]) slot_pair(y, phw, ((size_t)(s0w + q) * rows + p + 3) * kBins + b, b, v0, v1, vi);
    put_pair(xs, kXPartB, fr * kXRowB + b * 4, v0, v1);
  }
  // ... and the output staging: the state's addend under slot 0 of every lane, zeros under the others
  for (int i = tid; i < kFramesPerWg * (kStep / 4); i += kThreadsX) {
    const int fr = i >> 5, c = 4 * (i & 31);
    const int q = fr / K;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (fr == q * K && sFlag[q]) v = *reinterpret_cast<const f32x4*>(state + (size_t)(s0w + q) * kStFloats + kStPend + c);
    *reinterpret_cast<f32x4*>(obuf + fr * kORow + c) = v;
  }
  __syncthreads();

  float* mine = obuf + n * kORow + s0;   // + 16 t rows: this lane's words of slot 16 t + n
  const int lane_off = n * kXRowB + 16 * kq;
  auto chunk = [](int c) { return 64 * c; };
  f32x4 acc[4];
  // M-tile wave: first halves, frame = hop
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_block(A, xs, kXPartB, lane_off, 16 * kXRowB, chunk, acc);
  load_a(A, cpack, wave + kWaves, lane);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x4* at = reinterpret_cast<f32x4*>(mine + 16 * t * kORow);
    const f32x4 o = *at;
    *at = f32x4{o.x + acc[t].x, o.y + acc[t].y, o.z + acc[t].z, o.w + acc[t].w};
  }
  // M-tile wave + 8: second halves, frame = hop - 1: the slot below, but never across a lane's slot 0; then the two single-frame hops
  // are put right, and the last slot's second half is the lane's new addend (the old one was read before the barrier above)
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_block(A, xs, kXPartB, lane_off, 16 * kXRowB, chunk, acc);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f32x4 v = frame_below(acc[t], t ? acc[t - 1] : f32x4{0.f, 0.f, 0.f, 0.f}, lane);
    const int fr = 16 * t + n;
    const int q = fr / K, p = fr - q * K;
    const int hop = sH[q] - kDelayHops + p;
    f32x4* at = reinterpret_cast<f32x4*>(mine + 16 * t * kORow);
    f32x4 u = *at;
    if (p) u = f32x4{u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w};
    if (hop == 0 || hop == sT[q]) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(fix + (hop == 0 ? 0 : kStep) + s0);
      u = f32x4{u.x * g.x, u.y * g.y, u.z * g.z, u.w * g.w};
    }
    *at = u;
    if (!finish && p == K - 1 && sFlag[q]) *reinterpret_cast<f32x4*>(state + (size_t)(s0w + q) * kStFloats + kStPend + s0) = acc[t];
  }
  __syncthreads();

  // de-emphasis: the blocked affine scan over the 8,192 samples in slot order, one segment per lane, from the lane's carry
  {
    const int fl = tid >> 3;
    const int q = fl / K, p = fl - q * K;
    f32x4 yv[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, true, q * K * 8, sCarry[q], yv);
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) *reinterpret_cast<f32x4*>(obuf + fl * kORow + kDeBlock * (tid & 7) + 4 * j4) = yv[j4];
    if (!finish && p == K - 1 && (tid & 7) == 7 && sFlag[q]) state[(size_t)(s0w + q) * kStFloats + kStCarry] = yv[kDeBlock / 4 - 1].w;
  }
  __syncthreads();

  // the lane's hops in time: position p = slot p
  if (!finish) {
    for (int i = tid; i < lpw * K * kStep; i += kThreadsX) {
      const int q = i / (K * kStep), rem = i - q * (K * kStep), s = s0w + q;
      if (s >= S) break;
      out[(size_t)s * K * kStep + rem] = sFlag[q] ? obuf[(q * K + (rem >> 7)) * kORow + (rem & 127)] : 0.f;
    }
  } else {   // the L - max(0, 128 H - 640) samples still owed, from hop max(0, H - 5) on
    for (int i = tid; i < lpw * kFinishOut; i += kThreadsX) {
      const int q = i / kFinishOut, rem = i - q * kFinishOut, s = s0w + q;
      if (s >= S) break;
      const int H = sH[q];
      const int count = sFlag[q] ? kStep * H + sFlag[q] - 1 - max(0, kStep * (H - kDelayHops)) : 0;
      const int t = rem + kStep * max(0, kDelayHops - H);
      out[(size_t)s * kFinishOut + rem] = rem < count ? obuf[(q * K + (t >> 7)) * kORow + (t & 127)] : 0.f;
      if (rem == 0) out_counts[s] = count;
    }
  }

  // the rest of the lanes' new state
  for (int q = 0; q < lpw; ++q) {
    const int s = s0w + q;
    if (s >= S) break;
    if (!sFlag[q]) continue;   // an idle lane keeps its state
    float* st = state + (size_t)s * kStFloats;
    if (finish) {   // reset for a new utterance
      for (int i = tid; i < kStFloats; i += kThreadsX) st[i] = 0.f;
      continue;
    }
    advance_lane(st, in + (size_t)s * in_stride, win, phw, ((size_t)s * rows + K) * kBins, K, sH[q], sSample[q], tid);
  }
}

}  // namespace stream
}  // namespace audio
}  // namespace rced
