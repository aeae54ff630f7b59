// BSS Eval SDR of one source per utterance (include/rced.h, "evaluation" section; DESIGN.md 3.4c "BSS Eval SDR"): the
// estimate y is projected onto the span of the clean signal x delayed by 0 .. F - 1 samples (F = filter_length <= 512),
//   r[t] = sum_n x[n] x[n + t],  d[t] = sum_n x[n] y[n + t],  toeplitz(r) c = d,  s = x * c,  e = [y, 0 ..] - s,
//   10 log10(sum s^2 / sum e^2) over the L + F - 1 samples of s.
//
// The mapping (the one the issue proposed; nothing else was tried):
//   correlate_kernel  one workgroup per (4096-sample slice, r or d, utterance).  With n = 16 m + a and n + t = 16 m' + b the
//                     lag is t = 16 (m' - m) + b - a: for every block lag dl = m' - m = 0 .. (F + 14) / 16 the 16 x 16 tile
//                     P_dl[a][b] = sum_m x[16 m + a] y[16 (m + dl) + b] is one chain of v_mfma_f64_16x16x4_f64 over the slice
//                     (four m per instruction, A = x[64 s + lane], B = y[64 s + 16 dl + lane]).  Wave w owns dl = w, w + 4, ...
//                     The tiles' diagonals are folded in row order, a lag's (at most two) block lags in dl order.
//   solve_kernel      one wave per utterance: the slices' partial lags summed in slice order, then Levinson's recursion
//                     with a general right-hand side, r, d, the predictor and c in LDS (O(F)), F - 1 steps of two reductions.
//   project_kernel    one workgroup per (4096 outputs, utterance): s[16 m' + b] = sum_dl sum_a x[16 (m' - dl) + a] C_dl[a][b],
//                     C_dl[a][b] = c[16 dl + b - a]: rows m', columns b, K = (dl, a), four a per instruction.  A wave takes four
//                     tiles of 256 outputs; sum s^2 and sum e^2 of the slice follow.
//   final_kernel      the slices' energies in slice order, the score.
//
// The family's invariants (kernels_sepm.h) hold: no atomics; an utterance's slices depend on its own length and on F only;
// every sum runs in an order fixed by positions inside the utterance; samples past a length are never read (they are
// staged as zeros); fp64 throughout.  Nothing is regularised: a singular toeplitz(r) gives what the recursion gives.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_eval.h"
#include "kernels_sepm.h"

namespace rced {
namespace bss {

using eval::kThreads;
using eval::kWaves;
using sepm::d4;

constexpr int kMaxTaps = 512;
constexpr int kMaxBlockLags = (kMaxTaps + 14) / 16 + 1;      // dl = 0 .. 32
constexpr int kLagsPerWave = (kMaxBlockLags + kWaves - 1) / kWaves;
constexpr int kSlice = 4096;                                 // samples of x a correlation workgroup takes
constexpr int kReach = 16 * (kMaxBlockLags - 1);             // 512: how far past (before) its slice a workgroup reads y (x)
constexpr int kTilePitch = 17;
constexpr int kTilesPerWave = 4;
constexpr int kOutSlice = kWaves * kTilesPerWave * 256;      // outputs of s a projection workgroup takes
constexpr int kBack = kReach + 16;                           // samples staged before a projection slice

__host__ __device__ inline int block_lags(int F) { return (F + 14) / 16 + 1; }
__host__ __device__ inline int corr_slices(int len) { return (len + kSlice - 1) / kSlice; }
__host__ __device__ inline int out_len(int len, int F) { return len > 0 ? len + F - 1 : 0; }
__host__ __device__ inline int out_slices(int len, int F) { return (out_len(len, F) + kOutSlice - 1) / kOutSlice; }
// one pad float every 16: the 16 rows of an A operand, 16 samples apart, fall into different banks
__host__ __device__ inline int padded(int i) { return i + (i >> 4); }

// grid (corr_slices(cap), 2, N): part[n][which][slice][t], t < F, = sum over n' in the slice of x[n'] z[n' + t], z = x (which 0) or y
__global__ __launch_bounds__(kThreads) void correlate_kernel(const float* __restrict__ ref, int ref_stride,
                                                             const float* __restrict__ est, int est_stride,
                                                             const int* __restrict__ lengths, int cap, int F,
                                                             double* __restrict__ part, int slices) {
  __shared__ float xs[kSlice];
  __shared__ float zs[kSlice + kReach];
  __shared__ double tile[kWaves][16 * kTilePitch];
  __shared__ double diag[kMaxBlockLags][32];
  const int n = blockIdx.z, which = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = eval::clamp_len(lengths, n, cap);
  const int base = sl * kSlice;
  if (base >= len) return;                               // uniform over the workgroup
  const float* x = ref + (size_t)n * ref_stride;
  const float* z = which ? est + (size_t)n * est_stride : x;
  const int left = len - base;                           // > 0
  for (int i = threadIdx.x; i < kSlice; i += kThreads) xs[i] = i < left ? x[base + i] : 0.f;
  for (int i = threadIdx.x; i < kSlice + kReach; i += kThreads) zs[i] = i < left ? z[base + i] : 0.f;
  __syncthreads();
  const int nd = block_lags(F);
  const int steps = ((left < kSlice ? left : kSlice) + 63) / 64;
  d4 acc[kLagsPerWave];
#pragma unroll
  for (int i = 0; i < kLagsPerWave; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < steps; ++s) {
    const double a = (double)xs[64 * s + lane];
#pragma unroll
    for (int i = 0; i < kLagsPerWave; ++i) {
      const int dl = wave + kWaves * i;
      if (dl < nd) {                                     // uniform over the wave
        const double b = (double)zs[64 * s + 16 * dl + lane];     // <= kSlice - 64 + kReach + 63
        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
      }
    }
  }
  // diag[dl][15 + k] = sum_a P_dl[a][a + k], a in order; every wave runs every round: the barriers are uniform
  const int row = lane >> 4, col = lane & 15;
#pragma unroll
  for (int i = 0; i < kLagsPerWave; ++i) {
    const int dl = wave + kWaves * i;
    if (dl < nd) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[wave][(row + 4 * r) * kTilePitch + col] = acc[i][r];
    }
    __syncthreads();
    if (dl < nd && lane < 31) {
      const int k = lane - 15;
      const int a0 = k < 0 ? -k : 0, a1 = k < 0 ? 15 : 15 - k;
      double sum = 0.0;
      for (int a = a0; a <= a1; ++a) sum += tile[wave][a * kTilePitch + a + k];
      diag[dl][lane] = sum;
    }
    __syncthreads();
  }
  double* out = part + ((size_t)(n * 2 + which) * slices + sl) * F;
  for (int t = threadIdx.x; t < F; t += kThreads) {
    const int dl = t >> 4, k = t & 15;                   // t = 16 dl + k = 16 (dl + 1) + (k - 16); dl + 1 < nd when k > 0
    double v = diag[dl][15 + k];
    if (k) v += diag[dl + 1][k - 1];
    out[t] = v;
  }
}

// grid (N), one wave.  cws: [N][F], the filter for project_kernel; filter: NULL or [N][F]
__global__ __launch_bounds__(64) void solve_kernel(const double* __restrict__ part, const int* __restrict__ lengths, int cap,
                                                   int F, int slices, double* __restrict__ cws, double* __restrict__ filter) {
  __shared__ double r[kMaxTaps], d[kMaxTaps], c[kMaxTaps], pa[2][kMaxTaps];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int nsl = corr_slices(eval::clamp_len(lengths, n, cap));
  const double* pr = part + (size_t)(n * 2) * slices * F;
  const double* pd = pr + (size_t)slices * F;
  for (int t = lane; t < F; t += 64) {
    double sr = 0.0, sd = 0.0;
    for (int j = 0; j < nsl; ++j) {                      // slice order
      sr += pr[(size_t)j * F + t];
      sd += pd[(size_t)j * F + t];
    }
    r[t] = sr;
    d[t] = sd;
    c[t] = 0.0;
    pa[0][t] = 0.0;
    pa[1][t] = 0.0;
  }
  __syncthreads();
  // order k - 1 -> k: toeplitz(r[0 .. k)) a = (E, 0 ..), a[0] = 1; toeplitz(r[0 .. k)) c = d[0 .. k)
  double E = r[0];
  if (lane == 0) {
    pa[0][0] = 1.0;
    c[0] = d[0] / r[0];
  }
  __syncthreads();
  int cur = 0;
  for (int k = 1; k < F; ++k) {
    const double* a = pa[cur];
    double* an = pa[cur ^ 1];
    double sa = 0.0, sc = 0.0;
    for (int j = lane; j < k; j += 64) {
      const double rr = r[k - j];
      sa += a[j] * rr;
      sc += c[j] * rr;
    }
    sa = eval::wave_sum(sa);
    sc = eval::wave_sum(sc);
    const double lambda = -sa / E;
    for (int j = lane; j <= k; j += 64) an[j] = a[j] + lambda * a[k - j];      // a[k] = 0
    E = E * (1.0 - lambda * lambda);
    const double mu = (d[k] - sc) / E;
    __syncthreads();
    for (int j = lane; j <= k; j += 64) c[j] = c[j] + mu * an[k - j];          // c[k] = 0
    __syncthreads();
    cur ^= 1;
  }
  for (int t = lane; t < F; t += 64) {
    cws[(size_t)n * F + t] = c[t];
    if (filter) filter[(size_t)n * F + t] = c[t];
  }
}

// grid (out_slices(cap, F), N): pws[n][slice] = (sum s^2, sum e^2) over outputs [slice kOutSlice, + kOutSlice) below L + F - 1
__global__ __launch_bounds__(kThreads) void project_kernel(const float* __restrict__ ref, int ref_stride,
                                                           const float* __restrict__ est, int est_stride,
                                                           const int* __restrict__ lengths, int cap, int F,
                                                           const double* __restrict__ cws, double* __restrict__ pws, int pslices) {
  __shared__ float xs[kOutSlice + kBack + (kOutSlice + kBack) / 16 + 1];
  __shared__ double cs[16 * kMaxBlockLags + 32];         // cs[15 + i] = c[i], zeros around: i = -15 .. 16 nd + 14
  __shared__ double red[kWaves][2];
  const int n = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = eval::clamp_len(lengths, n, cap);
  const int total = out_len(len, F);
  const int base = sl * kOutSlice;
  if (base >= total) return;                             // uniform over the workgroup
  const float* x = ref + (size_t)n * ref_stride;
  const float* y = est + (size_t)n * est_stride;
  for (int i = threadIdx.x; i < kOutSlice + kBack; i += kThreads) {
    const int p = base - kBack + i;
    xs[padded(i)] = (p >= 0 && p < len) ? x[p] : 0.f;
  }
  const double* c = cws + (size_t)n * F;
  for (int i = threadIdx.x; i < 16 * kMaxBlockLags + 32; i += kThreads) cs[i] = (i >= 15 && i - 15 < F) ? c[i - 15] : 0.0;
  __syncthreads();
  const int nd = block_lags(F);
  const int row = lane & 15, kk = lane >> 4;             // A: row m', k; B: k, column b = row
  d4 acc[kTilesPerWave];
#pragma unroll
  for (int t = 0; t < kTilesPerWave; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  const int tile0 = wave * kTilesPerWave;
  for (int dl = 0; dl < nd; ++dl) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = 4 * q + kk;
      const double b = cs[15 + 16 * dl + row - a];       // >= 0, <= 15 + 16 (nd - 1) + 15
#pragma unroll
      for (int t = 0; t < kTilesPerWave; ++t) {
        // output block m' = 16 (tile0 + t) + row of the slice, input block m' - dl, sample a of it
        const int i = kBack + 256 * (tile0 + t) + 16 * (row - dl) + a;        // >= kBack - kReach
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xs[padded(i)], b, acc[t], 0, 0, 0);
      }
    }
  }
  double ss = 0.0, se = 0.0;
#pragma unroll
  for (int t = 0; t < kTilesPerWave; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = base + 256 * (tile0 + t) + 16 * (kk + 4 * r) + row;       // D: row kk + 4 r, column lane & 15
      if (p < total) {
        const double s = acc[t][r], e = (p < len ? (double)y[p] : 0.0) - s;
        ss += s * s;
        se += e * e;
      }
    }
  eval::block_sum2<kWaves>(ss, se, red);
  if (threadIdx.x == 0) *reinterpret_cast<double2*>(pws + ((size_t)n * pslices + sl) * 2) = make_double2(ss, se);
}

// grid (N), one wave.  L = 0, x = 0 and y = 0 give nan (0 / 0); energies: NULL or [N][2]
__global__ __launch_bounds__(64) void final_kernel(const double* __restrict__ pws, const int* __restrict__ lengths, int cap, int F,
                                                   int pslices, double* __restrict__ out, double* __restrict__ energies) {
  const int n = blockIdx.x;
  double ss, se;
  eval::sum_partials<1>(pws, n, pslices, out_slices(eval::clamp_len(lengths, n, cap), F), ss, se, nullptr);
  if (threadIdx.x == 0) {
    out[n] = 10.0 * log10(ss / se);
    if (energies) *reinterpret_cast<double2*>(energies + (size_t)n * 2) = make_double2(ss, se);
  }
}

}  // namespace bss
}  // namespace rced
