// STFT and the two rebuilds at any framing (W, S, window name), 2 <= W <= 256, 1 <= S <= W, under rfft(256): the general entries next
// to the ones specialised for 256 / 128 / hamming (kernels_audio_x6.h, kernels_ola_x6.h), which stay what the default path runs.
// Reference rows: data_utils/audio_feature.py:22-115 (STFT), model_utils/utils.py:171-183 (rebuild); DESIGN.md 3.4i.
//
// Both transforms stay x6_dft.h's K = 256 GEMM, one M-tile per wave with its A fragments in registers.  The window (and 1 / 256, irfft's
// factor 2, for the reference rebuild 1 / w) is in the coefficient pack, whose columns (STFT) or rows (rebuilds) past W are zero
// (audio_api.hip builds them in double, per device and framing).  What is new is the staging:
//   STFT     The B operand of frame f starts at sample f S.  The block's frames are staged ONE ROW EACH (256 slots + 16 bytes of pad,
//            the ISTFT's image layout), not as one contiguous span of (64 - 1) S + 256 samples: a lane's 16-byte fragment read of a
//            span would start at byte 2 (f S + 32 c + 8 kq), which is 16-byte aligned only when S is a multiple of 8, and an unaligned
//            ds_read_b128 is replayed at 64 cycles.  A sample is split up to ceil(W / S) times instead of once; slots at and past W, at
//            and past the utterance's length, and of frames at and past its count are zeros (never garbage: 0 x NaN is NaN).
//   Rebuilds Two steps.  frames_fr_kernel: Y[utt][t][r] = sum_k C[r][k] X_t[k], r < W, all W samples of every frame, to a scratch
//            buffer (row scale folded in: w[r] for overlap-add, 1 / w[r] for the reference rebuild; the rank-1 term of im(bin 128) at
//            nfft = 512).  rebuild_fr_kernel: one workgroup per utterance walks its samples 8,192 at a time; a sample gathers its
//            addends from the frames that cover it in ascending frame order (overlap-add: up to ceil(W / S), divided by the sum of
//            w^2 over the same frames, 0 where that is at most 1e-10; reference: the one frame de_frame keeps), then deemph_scan,
//            the carry across chunks in a register.  No atomics, one summation order; utterance n's result depends on its own
//            frames and count only.  Frames at or past an utterance's count are neither read nor written.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_audio_x6.h"

namespace rced {
namespace audio {
namespace fr {

using namespace x6;   // kThreadsX, kWaves, kXRowB, kXPartB, kORow, AFrag, load_a, gemm_block, put_pair, slot_pair, rank1_add, stft_store, deemph_scan

constexpr int kMaxWindow = kFrame;                 // rfft(256) would crop a longer frame
constexpr int kFrMT = 16;                          // M-tiles of every pack: 256 rows
constexpr int kFrPack = kFrMT * kPackPerMT;        // bf16
constexpr int kStftFrLdsBytes = 3 * kXPartB;                           // the three images: 101,376
constexpr int kFramesFrLdsBytes = 3 * kXPartB + kFramesPerWg * 4;      // + im of bin 128 per frame
constexpr int kChunk = kThreadsX * kDeBlock;       // samples per step of the rebuild's walk: 8,192
static_assert(kChunk == kFramesPerWg * kStep, "deemph_scan's staging holds one chunk");
static_assert(kFramesFrLdsBytes <= 160 * 1024, "one workgroup's LDS");

// ceil(|L - W| / S + 1)   (audio_feature.py:70)
__host__ __device__ inline int num_frames(int len, int W, int S) {
  const int d = len >= W ? len - W : W - len;
  return (d + S - 1) / S + 1;
}

// pcm [N, L]; lengths [N] or null (= L); mag [N, T, 129]; phase [N, T, 129, 2] or null.  grid (N, 2 M-groups, frame ranges);
// apack: kFrPack bf16, rows as stft_x6_kernel's (0 = re(0), 1 = re(128), 2b / 2b + 1 = re / im of bin b), w[k] folded in, 0 for k >= W.
__global__ __launch_bounds__(kThreadsX) void stft_fr_kernel(const float* __restrict__ pcm, const int* __restrict__ lengths,
                                                             const unsigned short* __restrict__ apack, int L, int T, int W, int S,
                                                             float* __restrict__ mag, float* __restrict__ phase) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x, mt = blockIdx.y * kWaves + wave;
  const int len = lengths ? min(lengths[utt], L) : L;
  const int nf = len > 0 ? num_frames(len, W, S) : 0;
  const float* s = pcm + (size_t)utt * L;
  AFrag A;
  load_a(A, apack, mt, lane);
  const int nblk = (T + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    __syncthreads();   // the previous block's reads of the images are done
    // frame f0 + fr, slots k, k + 1: e[g] = s[g] - 0.97 s[g-1] at g = (f0 + fr) S + k as ONE float32 multiply and ONE float32 subtract
    // (audio_feature.py:54 works in float32), e[0] = s[0]; zero fill AFTER pre-emphasis, so e[len] = 0, not -0.97 s[len-1]
    for (int i = tid; i < kFramesPerWg * (kFrame / 2); i += kThreadsX) {
      const int fr = i >> 7, k = 2 * (i & 127);
      float e0 = 0.f, e1 = 0.f;
      if (f0 + fr < nf && k < W) {
        const long long g = (long long)(f0 + fr) * S + k;
        if (g < len) {
          const float z = s[g];
          e0 = g == 0 ? z : __fsub_rn(z, __fmul_rn(kPre, s[g - 1]));
          if (k + 1 < W && g + 1 < len) e1 = __fsub_rn(s[g + 1], __fmul_rn(kPre, z));
        }
      }
      put_pair(xs, kXPartB, fr * kXRowB + (i & 127) * 4, e0, e1);
    }
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int fr = f0 + 16 * t + n;
      if (fr < T) stft_store(acc[t], fr < nf, true, mt, kq, ((size_t)utt * T + fr) * kBins, mag, phase);
    }
  }
}

// mag [N, T, 129], phase [N, T, 129, 2], frames [N] or null (= T each; clamped into [0, T]) -> Y [N, T, 256] fp32: samples r < W of
// every frame below the utterance's count, times the pack's row scale.  grid (N, 2 M-groups, 64-frame blocks).  cpack: kFrPack bf16,
// K slot 2b + c (slot 1 = re of bin 128); cim: 256 floats, the coefficients of im(bin 128) (zeros at nfft = 256).
__global__ __launch_bounds__(kThreadsX) void frames_fr_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                               const int* __restrict__ frames, const unsigned short* __restrict__ cpack,
                                                               const float* __restrict__ cim, int T, int W, float* __restrict__ Y) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  float* xim = reinterpret_cast<float*>(xs + 3 * kXPartB);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x, mt = blockIdx.y * kWaves + wave;
  const int F = frames ? min(max(frames[utt], 0), T) : T;
  const int f0 = blockIdx.z * kFramesPerWg;
  if (f0 >= F || 16 * kWaves * (int)blockIdx.y >= W) return;   // (the whole workgroup: before any barrier)
  for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
    const int fr = i >> 7, b = i & 127;
    float v0 = 0.f, v1 = 0.f, vi = 0.f;
    if (f0 + fr < F) slot_pair(mag, phase, ((size_t)utt * T + f0 + fr) * kBins + b, b, v0, v1, vi);
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
    const int fr = f0 + 16 * t + n;
    if (fr < F) *reinterpret_cast<f32x4*>(Y + ((size_t)utt * T + fr) * kFrame + 16 * mt + 4 * kq) = acc[t];
  }
}

// Y [N, T, 256] (frames_fr_kernel) -> y [N, (W - S) + T S], every column written; rows `ystride` floats apart (>= that width: the
// wave objective's rows are padded to whole 16-byte groups, kernels_wave_loss_fr.h).  grid (N).
// OLA:  e[i] = sum_t Y[t][i - tS] / sum_t w2[i - tS] over the frames t < F that cover i (0 where the denominator is at most 1e-10,
//       scipy.signal.istft's rule), i < (F - 1) S + W; zeros from there on.  w2: 256 floats, w^2.  frames as above.
// !OLA: de_frame (utils.py:139-147): the first W - S samples of frame 0, then the last S samples of every frame (F = T).
// Then y[i] = e[i] + 0.97 y[i-1], y[0] = e[0].
template <bool OLA>
__global__ __launch_bounds__(kThreadsX) void rebuild_fr_kernel(const float* __restrict__ Y, const int* __restrict__ frames,
                                                                const float* __restrict__ w2, int T, int W, int S, long long ystride,
                                                                float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float obuf[kFramesPerWg * kORow];   // a chunk in time order, rows of 128 (deemph_scan's layout)
  __shared__ float sa[kThreadsX], sb[kThreadsX];
  const int tid = threadIdx.x, utt = blockIdx.x;
  const int F = OLA && frames ? min(max(frames[utt], 0), T) : T;
  const long long width = (long long)(W - S) + (long long)T * S;
  const long long n_out = F > 0 ? (long long)(F - 1) * S + W : 0;
  const float* Yu = Y + (size_t)utt * T * kFrame;
  float* yo = y + (size_t)utt * ystride;
  float carry = 0.f;   // y just before the chunk
  for (long long base = 0; base < n_out; base += kChunk) {
    __syncthreads();   // the previous chunk's reads of obuf, sa, sb are done
#pragma unroll 4
    for (int j = 0; j < kDeBlock; ++j) {
      const int p = j * kThreadsX + tid;
      const long long i = base + p;
      float v = 0.f;
      if (i < n_out) {
        if (OLA) {
          const long long t0 = i < W ? 0 : (i - W) / S + 1, t1 = min(i / S, (long long)F - 1);
          float num = 0.f, den = 0.f;
          for (long long t = t0; t <= t1; ++t) {
            const int r = (int)(i - t * S);
            num += Yu[t * kFrame + r];
            den += w2[r];
          }
          v = den > 1e-10f ? num / den : 0.f;
        } else if (i < W - S) {
          v = Yu[i];
        } else {
          const long long q = i - (W - S), t = q / S;
          v = Yu[t * kFrame + (W - S) + (int)(q - t * S)];
        }
      }
      obuf[(p >> 7) * kORow + (p & 127)] = v;
    }
    __syncthreads();
    f32x4 yv[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, true, 0, carry, yv);
    // back through obuf (the scan has read it; every thread owns its sixteen words) and out in time order: a row of y starts
    // wherever the width puts it, so the stores are single words, a wave's 64 of them contiguous
    float* own = obuf + (tid >> 3) * kORow + kDeBlock * (tid & 7);
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) *reinterpret_cast<f32x4*>(own + 4 * j4) = yv[j4];
    carry = fmaf(sa[kThreadsX - 1], carry, sb[kThreadsX - 1]);
    __syncthreads();
    const int cnt = (int)min((long long)kChunk, n_out - base);
    for (int p0 = 0; p0 < cnt; p0 += kThreadsX) {   // (a uniform trip count: the lane's own bound guards the store, not the loop)
      const int p = p0 + tid;
      if (p < cnt) yo[base + p] = obuf[(p >> 7) * kORow + (p & 127)];
    }
  }
  for (long long z = n_out; z < width; z += kThreadsX)
    if (z + tid < width) yo[z + tid] = 0.f;
}

}  // namespace fr
}  // namespace audio
}  // namespace rced
