// Waveform and SI-SDR terms on the overlap-add rebuild, and their gradient with respect to the magnitudes (include/rced.h,
// rced_wave_loss).  Default framing: 256 / 128 / hamming (any other: kernels_wave_loss_fr.h, which reuses the sums, the
// terms and project_store from here with the scored range as a function of (W, S)).  Per utterance, with y = rced_istft_ola(M, P, F)
// (istft_ola_x6_kernel, unchanged, into a workspace), c the clean row of l samples and R = [lo, hi) the scored range:
//   sums     <y,c>, <c,c>, then with alpha = <y,c> / <c,c>:  |y - alpha c|^2, |y - c|^2, all over R, fp64, in slices (the mapping of
//            kernels_eval.h: a sum's order depends on the sample's index inside its utterance only), no atomics;
//   reverse  g_y on R from the stored scalars, g_e[i] = g_y[i] + 0.97 g_e[i+1] (the de-emphasis transposed: deemph_scan over the
//            block mirrored in time), u = g_e / sum w^2;
//   adjoint  G_t = rfft(w u[128t : 128t + 256]), dM_t[b] = (kappa_b / 256)(P_re G_re + P_im G_im): stft_x6_kernel's decomposition
//            with another coefficient pack (window and kappa_b / 256 folded in), no pre-emphasis, and a projection onto the phase
//            where the STFT takes the magnitude.
// Frames at or past F and clean samples at or past l are never read; every result of utterance n depends on its own F, l and data
// only.  Kernels are defined here and the header is included from one translation unit (audio_api.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_ola_x6.h"

namespace rced {
namespace wloss {

using audio::f32x2;
using audio::f32x4;
using audio::kBins;
using audio::kDeBlock;
using audio::kFramesPerWg;
using audio::kPre;
using audio::kStep;
using namespace audio::x6;   // the DFT GEMM, the segment geometry of the STFT, deemph_scan

constexpr int kSumThreads = 256, kSumWaves = kSumThreads / 64;
constexpr int kSlice = kSumThreads * 8;             // samples per workgroup of the two partial passes: two 16-byte groups per lane
constexpr double kEps = 1e-8;                       // this project's choice (rced.h)
constexpr double kDb = 4.342944819032518;           // 10 / ln 10
constexpr int kBlockSamples = kFramesPerWg * kStep; // a block of the reverse pass: 64 hops

__host__ __device__ inline int num_slices(int hi) { return (hi + kSlice - 1) / kSlice; }

// The scored range of utterance n, [lo, hi): hi = 0 for an empty one
struct Range {
  int lo, hi;
};
// at a framing (W, S): with skip_edges the samples whose covering frames are limited neither by t >= 0 nor by t <= F - 1
__device__ __forceinline__ Range range_of(const int* __restrict__ lengths, const int* __restrict__ frames, int n, int clean_stride,
                                          int skip_edges, int W, int S) {
  const int len = min(max(lengths[n], 0), clean_stride), F = frames[n];
  Range r;
  r.lo = skip_edges ? W - S : 0;
  r.hi = min(len, skip_edges ? F * S : (F - 1) * S + W);
  if (F <= 0 || r.hi <= r.lo) r.hi = 0;
  return r;
}
__device__ __forceinline__ Range range_of(const int* __restrict__ lengths, const int* __restrict__ frames, int n, int clean_stride,
                                          int skip_edges) {
  return range_of(lengths, frames, n, clean_stride, skip_edges, audio::kFrame, kStep);
}

// grid (ceil(N / 256)): the frame counts every later launch reads.  given: [N] or null (= num_frames(length)); clamped into [0, T]
__global__ __launch_bounds__(256) void frames_kernel(const int* __restrict__ given, const int* __restrict__ lengths, int N, int T,
                                                      int* __restrict__ frames) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int len = lengths[n];
  const int f = given ? given[n] : (len > 0 ? audio::num_frames(len) : 0);
  frames[n] = min(max(f, 0), T);
}

__device__ __forceinline__ double wave_sum(double v) {   // every lane ends with the same bits
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// (a, b) summed over a workgroup of kSumThreads, waves in wave order, the result in every thread; safe to call again on `sh`
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*sh)[2]) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = a;
    sh[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  a = sh[0][0];
  b = sh[0][1];
#pragma unroll
  for (int w = 1; w < kSumWaves; ++w) {
    a += sh[w][0];
    b += sh[w][1];
  }
}
// the partials of utterance n in slice order
__device__ __forceinline__ void sum_partials(const double* __restrict__ ws, int n, int slices, int nsl, double& a, double& b,
                                             double (*sh)[2]) {
  a = 0.0;
  b = 0.0;
  for (int j = threadIdx.x; j < nsl; j += kSumThreads) {
    const double2 v = *reinterpret_cast<const double2*>(ws + ((size_t)n * slices + j) * 2);
    a += v.x;
    b += v.y;
  }
  block_sum2(a, b, sh);
}

// grid (slices, N); (W, S): the framing of the scored range.  PASS 0: ws1[n][s] = (<y,c>, <c,c>) over R in slice s; PASS 1: ws2[n][s] = (|y - alpha c|^2, |y - c|^2), every
// workgroup summing pass 0's partials itself, in slice order (one alpha everywhere).  y: the rebuild, rows of `ystride` (a multiple of
// four floats on a 16-byte base); c: rows of `clean_stride`, any alignment, read one float at a time below hi only.
template <int PASS>
__global__ __launch_bounds__(kSumThreads) void sums_kernel(const float* __restrict__ y, int ystride, const float* __restrict__ clean,
                                                            int clean_stride, const int* __restrict__ lengths,
                                                            const int* __restrict__ frames, int skip_edges, int W, int S,
                                                            const double* __restrict__ ws1, double* __restrict__ out, int slices) {
  __shared__ double red[kSumWaves][2];
  const int n = blockIdx.y, s = blockIdx.x;
  const Range R = range_of(lengths, frames, n, clean_stride, skip_edges, W, S);
  const int base = s * kSlice;
  if (base >= R.hi) return;
  double alpha = 0.0;
  if (PASS == 1) {
    double yc, cc;
    sum_partials(ws1, n, slices, num_slices(R.hi), yc, cc, red);
    alpha = cc > 0.0 ? yc / cc : 0.0;
  }
  const float* yr = y + (size_t)n * ystride;
  const float* cr = clean + (size_t)n * clean_stride;
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = base + (j * kSumThreads + threadIdx.x) * 4;
    if (p < R.hi && p + 4 > R.lo) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(yr + p);   // p + 3 < ystride: the row holds whole groups
      const float yv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k >= R.lo && p + k < R.hi) {
          const double yy = yv[k], c = cr[p + k];
          if (PASS == 0) {
            a += yy * c;
            b += c * c;
          } else {
            const double r = yy - __dmul_rn(alpha, c), d = yy - c;
            a += r * r;
            b += d * d;
          }
        }
    }
  }
  block_sum2(a, b, red);
  if (threadIdx.x == 0) *reinterpret_cast<double2*>(out + ((size_t)n * slices + s) * 2) = make_double2(a, b);
}

// grid (N): terms[n] = (wave_sse, si_sdr, valid), rows tstride doubles apart; scal[n] = (alpha, 2 k alpha / (|alpha c|^2 + eps), 2 k / (|r|^2 + eps), 0), the
// last two zero for an invalid row: what the reverse pass forms g_y from
__global__ __launch_bounds__(kSumThreads) void terms_kernel(const double* __restrict__ ws1, const double* __restrict__ ws2,
                                                             const int* __restrict__ lengths, const int* __restrict__ frames,
                                                             int clean_stride, int skip_edges, int W, int S, int slices,
                                                             double* __restrict__ terms, int tstride, double* __restrict__ scal) {
  __shared__ double red[kSumWaves][2];
  const int n = blockIdx.x;
  const int nsl = num_slices(range_of(lengths, frames, n, clean_stride, skip_edges, W, S).hi);
  double yc, cc, rr, sse;
  sum_partials(ws1, n, slices, nsl, yc, cc, red);
  sum_partials(ws2, n, slices, nsl, rr, sse, red);
  if (threadIdx.x == 0) {
    const bool valid = nsl > 0 && cc > 0.0;
    const double alpha = valid ? yc / cc : 0.0;
    const double target = alpha * alpha * cc;
    terms[(size_t)n * tstride] = sse;
    terms[(size_t)n * tstride + 1] = valid ? 10.0 * log10((target + kEps) / (rr + kEps)) : 0.0;
    terms[(size_t)n * tstride + 2] = valid ? 1.0 : 0.0;
    scal[(size_t)n * 4] = alpha;
    scal[(size_t)n * 4 + 1] = valid ? 2.0 * kDb * alpha / (target + kEps) : 0.0;
    scal[(size_t)n * 4 + 2] = valid ? 2.0 * kDb / (rr + kEps) : 0.0;
    scal[(size_t)n * 4 + 3] = 0.0;
  }
}

// ---- the reverse pass ---------------------------------------------------------------------------------------------------------------
constexpr int kRevLdsFloats = kFramesPerWg * kORow + 2 * kThreadsX;   // the block mirrored in time + the scan's maps: 37,888 bytes

// grid (N), one workgroup per utterance, its 64-hop blocks from the last to the first.  Thread i owns samples
// 128 f0 + 8176 - 16 i .. + 15 of a block: position p = 8191 - q of the mirrored block is deemph_scan's time order, so the forward scan
// over the mirror is g_e[q] = g_y[q] + 0.97 g_e[q+1], the carry (g_e of the later block's first sample) in a register.
//   g_y = 2 a (y - c) - q1 c + q2 (y - alpha c) on R, 0 elsewhere, formed in fp64 (y - alpha c cancels for a good estimate) and
//   rounded once; a = w_sse / B, q1, q2 = w_si_sdr / B times scal's.
//   u = g_e * inv: inv [3][128] = 1 / (w[s]^2 + w[s+128]^2), 1 / w[s]^2 (hop 0), 1 / w[s+128]^2 (hop F).
// u [N, ystride]: hops 0 .. F written here, everything from 128 (F + 1) -- from 0 for F = 0 -- as zeros.
__global__ __launch_bounds__(kThreadsX) void reverse_kernel(const float* __restrict__ y, int ystride, const float* __restrict__ clean,
                                                             int clean_stride, const int* __restrict__ lengths,
                                                             const int* __restrict__ frames, int skip_edges,
                                                             const double* __restrict__ scal, double a2, double wsi,
                                                             const float* __restrict__ inv, float* __restrict__ u) {
  __shared__ __attribute__((aligned(16))) float lds[kRevLdsFloats];
  float* obuf = lds;
  float* sa = obuf + kFramesPerWg * kORow;
  float* sb = sa + kThreadsX;
  const int tid = threadIdx.x, n = blockIdx.x;
  const int F = frames[n];
  const Range R = range_of(lengths, frames, n, clean_stride, skip_edges);
  const double alpha = scal[(size_t)n * 4], q1 = wsi * scal[(size_t)n * 4 + 1], q2 = wsi * scal[(size_t)n * 4 + 2];
  const float* yr = y + (size_t)n * ystride;
  const float* cr = clean + (size_t)n * clean_stride;
  float* ur = u + (size_t)n * ystride;
  const int q0 = kBlockSamples - kDeBlock * (tid + 1);   // this thread's first sample inside a block, time order
  const int p0 = kDeBlock * tid;                         // = 8191 - (q0 + 15): where its mirror starts
  float* mine = obuf + (p0 >> 7) * kORow + (p0 & 127);
  float carry = 0.f;
  const int nblk = F > 0 ? F / kFramesPerWg + 1 : 0;
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const int g0 = blk * kBlockSamples + q0;             // < ystride for every hop <= F; hops past F are not touched
    __syncthreads();                                     // the previous block's reads of sa, sb are done
#pragma unroll
    for (int j4 = 0; j4 < kDeBlock / 4; ++j4) {          // mirror group j4 = samples g0 + 12 - 4 j4 .. + 3, last first
      const int g = g0 + kDeBlock - 4 - 4 * j4;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (g < R.hi && g + 4 > R.lo) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(yr + g);
        const float yv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (g + k >= R.lo && g + k < R.hi) {
            const double yy = yv[k], c = cr[g + k];
            o[k] = (float)(a2 * (yy - c) + (q2 * (yy - alpha * c) - q1 * c));
          }
      }
      *reinterpret_cast<f32x4*>(mine + 4 * j4) = f32x4{o[3], o[2], o[1], o[0]};
    }
    f32x4 ge[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, true, 0, carry, ge);  // reads the thread's own sixteen words only, then sa / sb behind barriers
    carry = fmaf(sa[kThreadsX - 1], carry, sb[kThreadsX - 1]);
    const int hop = blk * kFramesPerWg + (q0 >> 7);
    if (hop <= F) {
      const float* iv = inv + (hop == 0 ? kStep : hop == F ? 2 * kStep : 0) + (q0 & 127);
#pragma unroll
      for (int j4 = 0; j4 < kDeBlock / 4; ++j4) {
        const int k = kDeBlock - 4 - 4 * j4;
        const f32x4 w = *reinterpret_cast<const f32x4*>(iv + k);
        *reinterpret_cast<f32x4*>(ur + g0 + k) = f32x4{ge[j4].w * w.x, ge[j4].z * w.y, ge[j4].y * w.z, ge[j4].x * w.w};
      }
    }
  }
  const int z0 = F > 0 ? (F + 1) * kStep : 0;
  for (int base = z0; base < ystride; base += 4 * kThreadsX)
    if (base + 4 * tid < ystride) *reinterpret_cast<f32x4*>(ur + base + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- the adjoint GEMM ---------------------------------------------------------------------------------------------------------------
// The sample pairs a thread stages for one block, fetched a block ahead (stft_x6_kernel's SegRaw without the pre-emphasis' neighbours)
struct SegPairs {
  f32x2 v[kSegIter];
};
__device__ __forceinline__ void pairs_fetch(SegPairs& R, const float* __restrict__ s, int len, int f0, int tid) {
#pragma unroll
  for (int it = 0; it < kSegIter; ++it) {
    const int g = f0 * kStep + 2 * (tid + it * kThreadsX);   // even, len is even: a pair is inside or outside
    R.v[it] = tid + it * kThreadsX < kSegPairs && g < len ? *reinterpret_cast<const f32x2*>(s + g) : f32x2{0.f, 0.f};
  }
}
// One frame's accumulators of M-tile mt projected onto the phase at `row` (= the frame's index * 129): stft_store's rows -- 4kq + {0,1} /
// {2,3} = (re, im) of bins 8 mt + 2kq + {0, 1}; M-tile 0, kq 0: rows 0, 1 = re of bin 0, re of bin 128, whose imaginary parts the
// rebuild ignores.  !live: zeros, and the phase is not read.  ACC: added to what grad holds (the spectral term's gradient, written by an
// earlier launch on the stream); a frame that is not live is then left as it is.
template <bool ACC>
__device__ __forceinline__ void project_store(const f32x4 v, bool live, int mt, int kq, size_t row, const float* __restrict__ phase,
                                              float* __restrict__ grad) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float re = h ? v.z : v.x, im = h ? v.w : v.y;
    const int b = 8 * mt + 2 * kq + h;
    float g = 0.f;
    if (b == 0) {
      float g128 = 0.f;
      if (live) {
        g = phase[2 * row] * re;
        g128 = phase[2 * (row + kBins - 1)] * im;
      }
      if (!ACC) grad[row + kBins - 1] = g128;
      else if (live) grad[row + kBins - 1] += g128;
    } else if (live) {
      const f32x2 p = *reinterpret_cast<const f32x2*>(phase + 2 * (row + b));
      g = fmaf(p.x, re, p.y * im);
    }
    if (!ACC) grad[row + b] = g;
    else if (live) grad[row + b] += g;
  }
}

// grid (N, 2 M-groups, S frame ranges); pack: kStftPackX bf16, rows as the STFT's, coefficient w[k] (kappa_b / 256)(cos, -sin).
// u [N, ystride] -> grad [N, T, 129], every element written, frames at or past F as zeros; ACC: added to grad instead.
template <bool ACC>
__global__ __launch_bounds__(kThreadsX) void adjoint_kernel(const float* __restrict__ u, int ystride, const int* __restrict__ frames,
                                                             const unsigned short* __restrict__ apack, const float* __restrict__ phase,
                                                             int T, float* __restrict__ grad) {
  __shared__ __attribute__((aligned(16))) char seg[3 * kSegPartB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x, mt = blockIdx.y * kWaves + wave;
  const int F = frames[utt];
  const int len = F > 0 ? (F + 1) * kStep : 0;   // <= ystride
  const float* s = u + (size_t)utt * ystride;
  AFrag A;
  load_a(A, apack, mt, lane);
  const int nblk = (T + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  SegPairs R;
  if (blk0 < blk1 && blk0 * kFramesPerWg < F) pairs_fetch(R, s, len, blk0 * kFramesPerWg, tid);
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (f0 < F) {   // (uniform over the workgroup; a block past F is zeros and runs no GEMM)
      __syncthreads();   // the previous block's reads of seg are done
#pragma unroll
      for (int it = 0; it < kSegIter; ++it) {
        const int p = tid + it * kThreadsX;
        if (p < kSegPairs) put_pair(seg, kSegPartB, (p >> 6) * kSegRowB + (p & 63) * 4, R.v[it].x, R.v[it].y);
      }
      __syncthreads();
      if (blk + 1 < blk1 && f0 + kFramesPerWg < F) pairs_fetch(R, s, len, f0 + kFramesPerWg, tid);   // in flight during the MFMAs
      gemm_block(A, seg, kSegPartB, n * kSegRowB + 16 * kq, 16 * kSegRowB, [](int c) { return (c >> 2) * kSegRowB + 64 * (c & 3); }, acc);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int fr = f0 + 16 * t + n;
      if (fr < T) project_store<ACC>(acc[t], fr < F, mt, kq, ((size_t)utt * T + fr) * kBins, phase, grad);
    }
  }
}

}  // namespace wloss
}  // namespace rced
