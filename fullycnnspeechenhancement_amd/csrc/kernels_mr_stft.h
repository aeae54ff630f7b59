// The multi-resolution STFT term between two ragged row sets, and its gradient with respect to the estimate: rced_mr_stft and the
// term of rced_wave_loss_mr (include/rced.h).  Per utterance a scored range [lo, hi) and K <= 4 resolutions (W, S, w):
//   analysis  stft_fr_kernel's decomposition and staging (one aligned row of 256 slots per frame, kernels_framing.h) over the frames
//             lo + j S, j < J = floor((hi - lo - W) / S) + 1, the STFT's pack (w[k](cos, -sin), zero for k >= W) and no pre-emphasis; the
//             estimate's rows and the reference's in one launch; the epilogue forms |X|_eps = sqrt(re^2 + im^2 + 1e-8) in fp64, rounded
//             once, and keeps Y (re, im), |Y|_eps and |C|_eps in the workspace for the second pass;
//   sums      A = sum (|C| - |Y|)^2, B = sum |C|^2, L = sum (ln|C| - ln|Y|)^2 per (utterance, resolution) in fp64: 64-frame slices, a
//             thread's elements in ascending order, the lanes by xor shuffles, the waves and then the slices in ascending order;
//   terms     sc = sqrt(A / B), lsd = L / (129 J), term = sum_{J > 0} (sc + lsd) / K;
//   synth     (before the next resolution's analysis reuses the spectra) per bin G = g Y / |Y|, g = -(|C| - |Y|) c1 - c2 (ln|C| - ln|Y|) / |Y|
//             formed in fp64 and rounded once, c1 and c2 from the slice sums in the terms' order, then the GEMM 129 complex bins -> W
//             reals (slot 2b + c, slot 1 = re of bin 128: the imaginary parts of bins 0 and 128 are zero and so are their sines),
//             w[k] in the pack, into a frame scratch [N, Jmax, Wp];
//   gather    sample i adds its addends in ascending frame order, then ascending resolution, in one fp32 chain; zeros outside [lo, hi).
// No atomics, one summation order; nothing outside [lo, hi) is read; utterance n's results depend on its own range and data only.
// Included from one translation unit (audio_api.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_framing.h"
#include "kernels_wave_loss.h"

namespace rced {
namespace mrstft {

using namespace audio::x6;   // kThreadsX, kWaves, kXRowB, kXPartB, AFrag, load_a, gemm_block, put_pair
using audio::f32x2;
using audio::f32x4;
using audio::kBins;
using audio::kFramesPerWg;

constexpr int kMaxRes = 4;
constexpr double kEps = 1e-8;      // this project's choice (rced.h)
constexpr int kSumThreads = 256, kSumWaves = kSumThreads / 64;

struct Res {
  int W, S, Wp, Jmax;   // Wp: floats per frame of the scratch, W up to a whole M-tile; Jmax: the most frames a row of the call can hold
  long long off;        // floats from the scratch's base to this resolution's [N, Jmax, Wp]
};
struct Params {
  int K;
  Res r[kMaxRes];
};

// whole frames inside [lo, hi)
__host__ __device__ inline int frames_in(int lo, int hi, int W, int S) { return hi - lo >= W ? (hi - lo - W) / S + 1 : 0; }

// grid (ceil(N / 256)): [0, l_n) with the length clamped into [0, width]
__global__ __launch_bounds__(256) void ranges_kernel(const int* __restrict__ lengths, int N, int width, int2* __restrict__ rng) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < N) rng[n] = make_int2(0, min(max(lengths[n], 0), width));
}
// ... the wave objective's R at its framing (wloss::range_of), from the frame counts counts_kernel left
__global__ __launch_bounds__(256) void wave_ranges_kernel(const int* __restrict__ lengths, const int* __restrict__ frames, int N,
                                                           int clean_stride, int skip_edges, int W, int S, int2* __restrict__ rng) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const wloss::Range R = wloss::range_of(lengths, frames, n, clean_stride, skip_edges, W, S);
  rng[n] = make_int2(R.hi > R.lo ? R.lo : 0, R.hi > R.lo ? R.hi : 0);
}

__device__ __forceinline__ float mag_eps(float re, float im) {
  const double r = re, i = im;
  return (float)sqrt(r * r + i * i + kEps);
}

// One frame's accumulators of M-tile mt at `row` (= (utterance * Jmax + frame) * 129): stft_store's rows.  The estimate keeps (re, im)
// and the magnitude, the reference the magnitude alone.
__device__ __forceinline__ void spectrum_store(const f32x4 v, bool is_ref, int mt, int kq, size_t row, float* __restrict__ ysp,
                                               float* __restrict__ ym, float* __restrict__ cm) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float re = h ? v.z : v.x, im = h ? v.w : v.y;
    const int b = 8 * mt + 2 * kq + h;
    if (b == 0) {   // (re(0), re(128)): two bins with zero imaginary part
      const float m128 = mag_eps(im, 0.f);
      if (is_ref) {
        cm[row + kBins - 1] = m128;
      } else {
        ym[row + kBins - 1] = m128;
        *reinterpret_cast<f32x2*>(ysp + 2 * (row + kBins - 1)) = f32x2{im, 0.f};
      }
      im = 0.f;
    }
    const float m = mag_eps(re, im);
    if (is_ref) {
      cm[row + b] = m;
    } else {
      ym[row + b] = m;
      *reinterpret_cast<f32x2*>(ysp + 2 * (row + b)) = f32x2{re, im};
    }
  }
}

// grid (2 N, 2 M-groups, frame ranges): workgroups x < N take the estimate's row x, the others the reference's row x - N.
// apack: the STFT's pack of (W, name).  ysp [N, Jmax, 129, 2], ym, cm [N, Jmax, 129]: frames below the utterance's J are written.
__global__ __launch_bounds__(kThreadsX) void analysis_kernel(const float* __restrict__ est, long long est_stride, const float* __restrict__ ref,
                                                              long long ref_stride, const int2* __restrict__ rng,
                                                              const unsigned short* __restrict__ apack, int N, int W, int S, int Jmax,
                                                              float* __restrict__ ysp, float* __restrict__ ym, float* __restrict__ cm) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const bool is_ref = (int)blockIdx.x >= N;
  const int utt = is_ref ? blockIdx.x - N : blockIdx.x, mt = blockIdx.y * kWaves + wave;
  const int2 R = rng[utt];
  const int J = min(frames_in(R.x, R.y, W, S), Jmax);
  const float* s = (is_ref ? ref + (size_t)utt * ref_stride : est + (size_t)utt * est_stride) + R.x;
  AFrag A;
  load_a(A, apack, mt, lane);
  const int nblk = (Jmax + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    if (f0 >= J) break;   // (uniform over the workgroup)
    __syncthreads();      // the previous block's reads of the images are done
    for (int i = tid; i < kFramesPerWg * (audio::kFrame / 2); i += kThreadsX) {
      const int fr = i >> 7, k = 2 * (i & 127);
      float e0 = 0.f, e1 = 0.f;
      if (f0 + fr < J && k < W) {   // frame j < J lies inside [lo, hi): lo + j S + W <= hi
        const long long g = (long long)(f0 + fr) * S + k;
        e0 = s[g];
        if (k + 1 < W) e1 = s[g + 1];
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
      if (fr < J) spectrum_store(acc[t], is_ref, mt, kq, ((size_t)utt * Jmax + fr) * kBins, ysp, ym, cm);
    }
  }
}

__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double (*sh)[3]) {
  a = wloss::wave_sum(a);
  b = wloss::wave_sum(b);
  c = wloss::wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = a;
    sh[threadIdx.x >> 6][1] = b;
    sh[threadIdx.x >> 6][2] = c;
  }
  __syncthreads();
  a = sh[0][0];
  b = sh[0][1];
  c = sh[0][2];
#pragma unroll
  for (int w = 1; w < kSumWaves; ++w) {
    a += sh[w][0];
    b += sh[w][1];
    c += sh[w][2];
  }
}

// grid (ceil(Jmax / 64), N): part[n * pstride + 3 s] = (A, B, L) over frames [64 s, 64 s + 64) below J; slices at or past J are not written
__global__ __launch_bounds__(kSumThreads) void sums_kernel(const int2* __restrict__ rng, int W, int S, int Jmax, const float* __restrict__ ym,
                                                            const float* __restrict__ cm, double* __restrict__ part, size_t pstride) {
  __shared__ double red[kSumWaves][3];
  const int n = blockIdx.y, f0 = blockIdx.x * kFramesPerWg;
  const int2 R = rng[n];
  const int J = min(frames_in(R.x, R.y, W, S), Jmax);
  if (f0 >= J) return;
  const int cnt = min(kFramesPerWg, J - f0) * kBins;
  const size_t base = ((size_t)n * Jmax + f0) * kBins;
  double a = 0.0, b = 0.0, l = 0.0;
  for (int i = threadIdx.x; i < cnt; i += kSumThreads) {
    const double c = cm[base + i], y = ym[base + i];
    const double d = c - y, dl = log(c) - log(y);
    a += d * d;
    b += c * c;
    l += dl * dl;
  }
  block_sum3(a, b, l, red);
  if (threadIdx.x == 0) {
    double* p = part + (size_t)n * pstride + (size_t)blockIdx.x * 3;
    p[0] = a;
    p[1] = b;
    p[2] = l;
  }
}

// (A, B, L) of one (utterance, resolution): its slices in ascending order.  p: the row of partials; the one order for every reader
struct Sums {
  double a, b, l;
};
__device__ __forceinline__ Sums sum_slices(const double* __restrict__ p, int J) {
  const int nsl = (J + kFramesPerWg - 1) / kFramesPerWg;
  Sums s{0.0, 0.0, 0.0};
  for (int i = 0; i < nsl; ++i) {
    s.a += p[3 * i];
    s.b += p[3 * i + 1];
    s.l += p[3 * i + 2];
  }
  return s;
}

// grid (N), 64 threads.  part [N, K, nslmax, 3]; out[n * out_stride] = (term, valid) and, with detail, (sc_r, lsd_r, J_r) per resolution
__global__ __launch_bounds__(64) void terms_kernel(const int2* __restrict__ rng, Params P, const double* __restrict__ part, int nslmax,
                                                    double* __restrict__ out, int out_stride, int detail) {
  __shared__ double sh[kMaxRes][3];
  const int n = blockIdx.x, r = threadIdx.x;
  if (r < P.K) {
    const int2 R = rng[n];
    const int J = min(frames_in(R.x, R.y, P.r[r].W, P.r[r].S), P.r[r].Jmax);
    const Sums s = sum_slices(part + ((size_t)n * P.K + r) * nslmax * 3, J);
    sh[r][0] = J > 0 ? sqrt(s.a / s.b) : 0.0;
    sh[r][1] = J > 0 ? s.l / (129.0 * J) : 0.0;
    sh[r][2] = J;
  }
  __syncthreads();
  if (r == 0) {
    double term = 0.0, valid = 0.0;
    for (int q = 0; q < P.K; ++q)
      if (sh[q][2] > 0.0) {
        term += sh[q][0] + sh[q][1];
        valid = 1.0;
      }
    double* o = out + (size_t)n * out_stride;
    o[0] = term / P.K;
    o[1] = valid;
    if (detail)
      for (int q = 0; q < P.K; ++q) {
        o[2 + 3 * q] = sh[q][0];
        o[3 + 3 * q] = sh[q][1];
        o[4 + 3 * q] = sh[q][2];
      }
  }
}

// G of one bin (scaled): g Y / |Y|_eps
__device__ __forceinline__ f32x2 grad_bin(const f32x2 ysp, float ymag, float cmag, double c1, double c2) {
  const double y = ymag, c = cmag;
  const double g = -(c - y) * c1 - c2 * (log(c) - log(y)) / y;
  const double q = g / y;
  return f32x2{(float)(q * ysp.x), (float)(q * ysp.y)};
}

// grid (N, 2 M-groups, frame ranges).  spack: rows = samples k of a frame, K slot 2b + c (slot 1 = re of bin 128), coefficient
// w[k](cos, -sin)(2 pi b k / 256), zero rows for k >= W.  part: this resolution's partials of utterance 0, rows pstride doubles apart;
// c1 = scale / (sqrt(A) sqrt(B)), exactly 0 where A = 0, c2 = 2 scale / (129 J); scale = w_mr inv_batch / K.
// fr [N, Jmax, Wp]: frames below J written, all Wp columns of the M-tiles that hold a sample below W.
__global__ __launch_bounds__(kThreadsX) void synth_kernel(const int2* __restrict__ rng, const unsigned short* __restrict__ spack,
                                                           const float* __restrict__ ysp, const float* __restrict__ ym,
                                                           const float* __restrict__ cm, const double* __restrict__ part, size_t pstride,
                                                           double scale, int W, int S, int Wp, int Jmax, float* __restrict__ fr) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x, mt = blockIdx.y * kWaves + wave;
  if (16 * kWaves * (int)blockIdx.y >= W) return;   // (the whole workgroup: before any barrier)
  const int2 R = rng[utt];
  const int J = min(frames_in(R.x, R.y, W, S), Jmax);
  if (J == 0) return;
  const Sums sm = sum_slices(part + (size_t)utt * pstride, J);   // (every thread, the same loads in the same order)
  const double c1 = sm.a > 0.0 ? scale / (sqrt(sm.a) * sqrt(sm.b)) : 0.0, c2 = scale * 2.0 / (129.0 * J);
  AFrag A;
  load_a(A, spack, mt, lane);
  const int nblk = (Jmax + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    if (f0 >= J) break;   // (uniform over the workgroup)
    __syncthreads();      // the previous block's reads of the images are done
    for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
      const int f = i >> 7, b = i & 127;
      float v0 = 0.f, v1 = 0.f;
      if (f0 + f < J) {
        const size_t row = ((size_t)utt * Jmax + f0 + f) * kBins;
        const f32x2 g = grad_bin(*reinterpret_cast<const f32x2*>(ysp + 2 * (row + b)), ym[row + b], cm[row + b], c1, c2);
        v0 = g.x;
        v1 = g.y;
        if (b == 0) v1 = grad_bin(*reinterpret_cast<const f32x2*>(ysp + 2 * (row + kBins - 1)), ym[row + kBins - 1], cm[row + kBins - 1], c1, c2).x;
      }
      put_pair(xs, kXPartB, f * kXRowB + b * 4, v0, v1);
    }
    __syncthreads();
    if (16 * mt < W) {   // (a wave whose rows are all past W runs no GEMM; it still meets the barriers)
      f32x4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int f = f0 + 16 * t + n;
        if (f < J) *reinterpret_cast<f32x4*>(fr + ((size_t)utt * Jmax + f) * Wp + 16 * mt + 4 * kq) = acc[t];   // 16 mt + 4 kq + 3 < Wp
      }
    }
  }
}

// grid (ceil(width / 256), N).  scratch: the frame scratch's base.  g [N, gstride]: columns below `width` written, zeros outside
// [lo, hi).  Sample i = lo + p takes frame j's addend at k = p - j S, over j0 = max(0, floor((p - W) / S) + 1) .. min(floor(p / S), J - 1).
__global__ __launch_bounds__(256) void gather_kernel(const int2* __restrict__ rng, Params P, const float* __restrict__ scratch, long long width,
                                                      long long gstride, float* __restrict__ g) {
  const int n = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= width) return;
  const int2 R = rng[n];
  float v = 0.f;
  if (i >= R.x && i < R.y) {
    const int p = (int)(i - R.x);
    for (int r = 0; r < P.K; ++r) {
      const int W = P.r[r].W, S = P.r[r].S, Wp = P.r[r].Wp;
      const int J = min(frames_in(R.x, R.y, W, S), P.r[r].Jmax);
      const float* f = scratch + P.r[r].off + (size_t)n * P.r[r].Jmax * Wp;
      const int j0 = p < W ? 0 : (p - W) / S + 1, j1 = min(p / S, J - 1);
      for (int j = j0; j <= j1; ++j) v += f[(size_t)j * Wp + (p - j * S)];
    }
  }
  g[(size_t)n * gstride + i] = v;
}

}  // namespace mrstft
}  // namespace rced
