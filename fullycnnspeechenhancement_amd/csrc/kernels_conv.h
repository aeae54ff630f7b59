// A ragged batched FIR (include/rced.h, "room impulse responses"; DESIGN.md 3.4e "Reverberation"): per row n a signal x of
// len samples, a filter h of K <= kMaxTaps taps and a shift d < max(K, 1),
//   y[p] = sum_{k < K} h[k] x[p + d - k]  for p < len,  x = 0 outside [0, len);   y[p] = 0 for len <= p < L
// -- np.convolve(x, h)[d : d + len]: the output keeps the signal's length, tap d has zero delay, the tail is dropped.
//
// The mapping is project_kernel's (kernels_bsseval.h) with the taps taken in pieces:
//   convolve_kernel   one workgroup per (kOutSlice outputs, row).  With u[q] = x[q + d], p = 16 m' + b and q = 16 (m' - dl) + a
//                     the tap is k = 16 dl + b - a: for every block lag dl = 0 .. (K + 14) / 16 the 16 x 16 Toeplitz tile
//                     C_dl[a][b] = h[16 dl + b - a] (zero where the tap leaves [0, K)) meets 16 rows m' of the signal in four
//                     v_mfma_f64_16x16x4_f64 (four a each).  Every (output, tap) pair occurs in exactly one (dl, a).  A wave
//                     takes kTilesPerWave tiles of 256 outputs.  8192 taps are 513 block lags: they are walked in chunks of
//                     kLagChunk, and a chunk stages what it alone reads -- kWindow samples of the signal's history (19.6 KB
//                     as padded float32) and kTapSlots taps (4.2 KB as float64) --, so the LDS does not grow with K.
//
// The data-path family's invariants (kernels_eval.h, kernels_sepm.h) hold: no atomics; samples past len and taps past K are
// never read (they are staged as zeros); products and sums in fp64 from the stored fp32 values, one rounding at the store; an
// output's summation order -- dl ascending, a ascending -- depends on p, K, d and len only, never on N, the row index, the
// strides or other rows.  A chunk whose samples all lie outside the signal, and a wave whose outputs all lie past len, are left
// out: they would add zeros, +0.0 + (+-0.0) = +0.0, so the bits are those of the full walk.  A sample of -0.0 comes back as
// +0.0.  A tile multiplies samples by the zeros around the filter, so a non-finite sample reaches the outputs of its own
// and the neighbouring 16-sample block as NaN, not only those its taps reach.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_eval.h"
#include "kernels_sepm.h"

namespace rced {
namespace conv {

using eval::kThreads;
using eval::kWaves;
using sepm::d4;

constexpr int kMaxTaps = 8192;
constexpr int kMaxBlockLags = (kMaxTaps + 14) / 16 + 1;      // dl = 0 .. 512
constexpr int kLagChunk = 32;                                // block lags staged together: 512 taps
constexpr int kTilesPerWave = 4;
constexpr int kOutSlice = kWaves * kTilesPerWave * 256;      // 4096 outputs per workgroup
constexpr int kBack = 16 * kLagChunk;                        // samples staged before the slice's first, chunk 0
constexpr int kWindow = kOutSlice + kBack;                   // samples of the signal a chunk stages
constexpr int kTapSlots = 16 * kLagChunk + 16;               // ts[15 + j] = h[16 dl0 + j], j = -15 .. 16 kLagChunk - 1, zeros around the filter

__host__ __device__ inline int block_lags(int K) { return K > 0 ? (K + 14) / 16 + 1 : 0; }
__host__ __device__ inline int out_slices(int L) { return (L + kOutSlice - 1) / kOutSlice; }
// one pad float every 16: the 16 rows of an A operand, 16 samples apart, fall into different banks
__host__ __device__ inline int padded(int i) { return i + (i >> 4); }

__device__ inline int clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (out_slices(L), N)
__global__ __launch_bounds__(kThreads) void convolve_kernel(const float* __restrict__ xin, int x_stride, const int* __restrict__ x_len,
                                                            const float* __restrict__ hin, int h_stride, const int* __restrict__ h_len,
                                                            const int* __restrict__ shift, int L, float* __restrict__ yout,
                                                            int y_stride) {
  __shared__ float xs[kWindow + kWindow / 16 + 1];
  __shared__ double ts[kTapSlots];
  const int n = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = eval::clamp_len(x_len, n, L);
  const int kcap = h_stride < kMaxTaps ? h_stride : kMaxTaps;
  const int K = h_len ? clamp(h_len[n], 0, kcap) : kcap;
  const int d = shift ? clamp(shift[n], 0, K > 0 ? K - 1 : 0) : 0;
  const float* x = xin + (size_t)n * x_stride;
  const float* h = hin + (size_t)n * h_stride;
  float* y = yout + (size_t)n * y_stride;
  const int base = sl * kOutSlice;                       // < L
  const int left = len - base;                           // outputs of this slice that are sums; <= 0: only zeros to write
  const int nd = left > 0 ? block_lags(K) : 0;
  const int row = lane & 15, kk = lane >> 4;             // A: row m', k; B: k, column b = row
  const int tile0 = wave * kTilesPerWave;
  // whether a tile of this wave holds an output below len; the same in every lane, and kept in a scalar register so that
  // the matrix instructions sit behind a scalar branch, every lane enabled
  const bool active = __builtin_amdgcn_readfirstlane(left - 256 * tile0) > 0;
  d4 acc[kTilesPerWave];
#pragma unroll
  for (int t = 0; t < kTilesPerWave; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  for (int dl0 = 0; dl0 < nd; dl0 += kLagChunk) {
    // xs[i] = x[org + i]: the chunk reads i = kBack + 256 tile + 16 (row - dl') + a, dl' < kLagChunk
    const int org = base - 16 * dl0 - kBack + d;
    if (org + kWindow <= 0 || org >= len) continue;      // uniform over the workgroup: nothing of the signal in the window
    __syncthreads();                                     // the chunk before has been read
    for (int i = threadIdx.x; i < kWindow; i += kThreads) {
      const int p = org + i;
      xs[padded(i)] = (p >= 0 && p < len) ? x[p] : 0.f;
    }
    for (int i = threadIdx.x; i < kTapSlots; i += kThreads) {
      const int k = 16 * dl0 + i - 15;
      ts[i] = (k >= 0 && k < K) ? (double)h[k] : 0.0;
    }
    __syncthreads();
    const int ndc = active ? (nd - dl0 < kLagChunk ? nd - dl0 : kLagChunk) : 0;
    for (int dl = 0; dl < ndc; ++dl) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int a = 4 * q + kk;
        const double b = ts[15 + 16 * dl + row - a];     // >= 0, <= 15 + 16 (kLagChunk - 1) + 15 < kTapSlots
#pragma unroll
        for (int t = 0; t < kTilesPerWave; ++t) {
          // output block m' = 16 (tile0 + t) + row of the slice, input block m' - (dl0 + dl), sample a of it
          const int i = kBack + 256 * (tile0 + t) + 16 * (row - dl) + a;      // >= kBack - 16 (kLagChunk - 1), < kWindow
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xs[padded(i)], b, acc[t], 0, 0, 0);
        }
      }
    }
  }
  const int end = L - base < kOutSlice ? L - base : kOutSlice;
#pragma unroll
  for (int t = 0; t < kTilesPerWave; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 256 * (tile0 + t) + 16 * (kk + 4 * r) + row;              // D: row kk + 4 r, column lane & 15
      if (o < end) y[base + o] = o < left ? (float)acc[t][r] : 0.f;
    }
}

}  // namespace conv
}  // namespace rced
