// The waveform and SI-SDR terms at any framing (W, S, window name): rced_wave_loss_fr (include/rced.h).  The definition
// is kernels_wave_loss.h's with W, S and w in place of 256, 128 and hamming, over y = rced_istft_ola_fr(M, P, F), n_out = (F - 1) S + W.
//   forward  frames_fr_kernel + rebuild_fr_kernel<true> (kernels_framing.h) into the call's workspace, rows padded to whole 16-byte
//            groups; sums_kernel / terms_kernel (kernels_wave_loss.h) over R = [W - S, min(l, F S)) with skip_edges, else
//            [0, min(l, n_out));
//   reverse  g_y on R, g_e[i] = g_y[i] + 0.97 g_e[i+1] (deemph_scan over 8,192-sample chunks mirrored in time, last chunk first),
//            u[i] = g_e[i] / D[i], D[i] = sum_t w2[i - tS] over the frames t < F that cover i: rebuild_fr_kernel's loop, bounds, order and
//            fp32 sum, so D[i] <= 1e-10 holds for the samples the rebuild left at zero and for no others; u = 0 there;
//   adjoint  G_t = rfft_256(w u[tS : tS + W]), dM_t[b] = (kappa_b / 256)(P_re G_re + P_im G_im): stft_fr_kernel's decomposition and
//            staging (one aligned row of 256 slots per frame: S is no multiple of 8 in general, kernels_framing.h) with the pack
//            w[k] (kappa_b / 256)(cos, -sin), zero for k >= W, no pre-emphasis, and wloss::project_store as the epilogue.
// No atomics, one summation order, fp32 stores; utterance n's results depend on its own F, l and data only.  Included from one
// translation unit (audio_api.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_framing.h"
#include "kernels_wave_loss.h"

namespace rced {
namespace wloss {
namespace fr {

using audio::fr::kChunk;
using audio::fr::kStftFrLdsBytes;

// floats between rows of y and u: the rebuild's width (W - S) + T S, up to whole 16-byte groups
__host__ __device__ inline long long row_stride(int T, int W, int S) { return (((long long)(W - S) + (long long)T * S) + 3) & ~3ll; }

// grid (ceil(N / 256)): frames_kernel at a framing.  given: [N] or null (= fr::num_frames(length, W, S)); clamped into [0, T]
__global__ __launch_bounds__(256) void counts_kernel(const int* __restrict__ given, const int* __restrict__ lengths, int N, int T, int W,
                                                      int S, int* __restrict__ frames) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int len = lengths[n];
  const int f = given ? given[n] : (len > 0 ? audio::fr::num_frames(len, W, S) : 0);
  frames[n] = min(max(f, 0), T);
}

// 1 / D[i], D[i] = sum of w2[i - tS] over the frames t < F that cover i, in ascending frame order (rebuild_fr_kernel's expression);
// 0 where D[i] <= 1e-10 and for i at or past n_out (no frame covers it)
__device__ __forceinline__ float inv_den(const float* w2, int i, int W, int S, int F) {
  const int t0 = i < W ? 0 : (i - W) / S + 1, t1 = min(i / S, F - 1);
  float den = 0.f;
  for (int t = t0; t <= t1; ++t) den += w2[i - t * S];
  return den > 1e-10f ? 1.f / den : 0.f;
}

constexpr int kRevLdsFloats = kFramesPerWg * kORow + 2 * kThreadsX + audio::kFrame;   // the mirror, the scan's maps, w^2: 38,912 bytes

// grid (N), one workgroup per utterance, its n_out samples in chunks of 8,192 from the last to the first.  Thread i owns samples
// 8192 c + 8176 - 16 i .. + 15 of chunk c; position p = 8191 - q of the mirrored chunk is deemph_scan's time order, the carry (g_e of
// the later chunk's first sample) in a register: wloss::reverse_kernel's walk.  g_y as there, in fp64, rounded once.
// y, u [N, ystride], ystride a multiple of four floats; w2: 256 floats, w^2 (zero past W).  Every column of u is written: g_e / D below
// n_out, zeros from there on.  ADD: gadd [N, ystride] (the multi-resolution STFT term's gradient with respect to y, kernels_mr_stft.h) is
// added to g_y on R in fp64, before the rounding and the scan; without it the instantiation is the kernel as it has always been.
template <bool ADD>
__global__ __launch_bounds__(kThreadsX) void reverse_kernel(const float* __restrict__ y, long long ystride, const float* __restrict__ clean,
                                                             int clean_stride, const int* __restrict__ lengths,
                                                             const int* __restrict__ frames, int skip_edges, int W, int S,
                                                             const double* __restrict__ scal, double a2, double wsi,
                                                             const float* __restrict__ w2, const float* __restrict__ gadd,
                                                             float* __restrict__ u) {
  __shared__ __attribute__((aligned(16))) float lds[kRevLdsFloats];
  float* obuf = lds;
  float* sa = obuf + kFramesPerWg * kORow;
  float* sb = sa + kThreadsX;
  float* sw2 = sb + kThreadsX;
  const int tid = threadIdx.x, n = blockIdx.x;
  const int F = frames[n];
  const Range R = range_of(lengths, frames, n, clean_stride, skip_edges, W, S);
  const double alpha = scal[(size_t)n * 4], q1 = wsi * scal[(size_t)n * 4 + 1], q2 = wsi * scal[(size_t)n * 4 + 2];
  const float* yr = y + (size_t)n * ystride;
  const float* cr = clean + (size_t)n * clean_stride;
  float* ur = u + (size_t)n * ystride;
  if (tid < audio::kFrame) sw2[tid] = w2[tid];   // (the first barrier of the walk orders it)
  const int n_out = F > 0 ? (F - 1) * S + W : 0;   // <= ystride
  const int q0 = kChunk - kDeBlock * (tid + 1);    // this thread's first sample inside a chunk, time order
  const int p0 = kDeBlock * tid;                   // = 8191 - (q0 + 15): where its mirror starts
  float* mine = obuf + (p0 >> 7) * kORow + (p0 & 127);
  float carry = 0.f;
  const int nchunk = (n_out + kChunk - 1) / kChunk;
  for (int c = nchunk - 1; c >= 0; --c) {
    const int g0 = c * kChunk + q0;
    __syncthreads();                               // the previous chunk's reads of sa, sb are done
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) {    // mirror group j4 = samples g0 + 12 - 4 j4 .. + 3, last first
      const int g = g0 + kDeBlock - 4 - 4 * j4;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (g < R.hi && g + 4 > R.lo) {              // R.hi <= n_out <= ystride, a multiple of four: the group is inside the row
        const f32x4 v = *reinterpret_cast<const f32x4*>(yr + g);
        const float yv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (g + k >= R.lo && g + k < R.hi) {
            const double yy = yv[k], cc = cr[g + k];
            const double gy = a2 * (yy - cc) + (q2 * (yy - alpha * cc) - q1 * cc);
            o[k] = ADD ? (float)(gy + (double)gadd[(size_t)n * ystride + g + k]) : (float)gy;
          }
      }
      *reinterpret_cast<f32x4*>(mine + 4 * j4) = f32x4{o[3], o[2], o[1], o[0]};
    }
    f32x4 ge[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, true, 0, carry, ge);   // reads the thread's own sixteen words only, then sa / sb behind barriers
    carry = fmaf(sa[kThreadsX - 1], carry, sb[kThreadsX - 1]);
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) {
      const int g = g0 + kDeBlock - 4 - 4 * j4;
      if (g < ystride) {                           // whole groups: ystride is a multiple of four
        const f32x4 r = f32x4{ge[j4].w * inv_den(sw2, g, W, S, F), ge[j4].z * inv_den(sw2, g + 1, W, S, F),
                              ge[j4].y * inv_den(sw2, g + 2, W, S, F), ge[j4].x * inv_den(sw2, g + 3, W, S, F)};
        *reinterpret_cast<f32x4*>(ur + g) = r;     // at and past n_out: g_e = 0 (nothing scored there) times 0
      }
    }
  }
  for (long long base = (long long)nchunk * kChunk; base < ystride; base += 4 * kThreadsX)
    if (base + 4 * tid < ystride) *reinterpret_cast<f32x4*>(ur + base + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// grid (N, 2 M-groups, frame ranges); apack: kFrPack bf16, rows as the STFT's, coefficient w[k] (kappa_b / 256)(cos, -sin), 0 for k >= W.
// u [N, ystride] -> grad [N, T, 129], every element written, frames at or past F as zeros; ACC: added to grad instead (a frame at or
// past F is then left as it is).  Slot k of frame f is u[f S + k] for k < W, f < F and f S + k < n_out, else zero.
template <bool ACC>
__global__ __launch_bounds__(kThreadsX) void adjoint_kernel(const float* __restrict__ u, long long ystride, const int* __restrict__ frames,
                                                             const unsigned short* __restrict__ apack, const float* __restrict__ phase,
                                                             int T, int W, int S, float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x, mt = blockIdx.y * kWaves + wave;
  const int F = frames[utt];
  const int n_out = F > 0 ? (F - 1) * S + W : 0;   // <= ystride
  const float* s = u + (size_t)utt * ystride;
  AFrag A;
  load_a(A, apack, mt, lane);
  const int nblk = (T + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (f0 < F) {   // (uniform over the workgroup; a block past F is zeros and runs no GEMM)
      __syncthreads();   // the previous block's reads of the images are done
      for (int i = tid; i < kFramesPerWg * (audio::kFrame / 2); i += kThreadsX) {
        const int fr = i >> 7, k = 2 * (i & 127);
        float e0 = 0.f, e1 = 0.f;
        if (f0 + fr < F && k < W) {
          const int g = (f0 + fr) * S + k;
          if (g < n_out) {
            e0 = s[g];
            if (k + 1 < W && g + 1 < n_out) e1 = s[g + 1];
          }
        }
        put_pair(xs, kXPartB, fr * kXRowB + (i & 127) * 4, e0, e1);
      }
      __syncthreads();
      gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int fr = f0 + 16 * t + n;
      if (fr < T) project_store<ACC>(acc[t], fr < F, mt, kq, ((size_t)utt * T + fr) * kBins, phase, grad);
    }
  }
}

}  // namespace fr
}  // namespace wloss
}  // namespace rced
