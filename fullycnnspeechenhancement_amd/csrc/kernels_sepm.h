// LLR and WSS per utterance (include/rced.h, "evaluation" section): the two spectral terms of the composite
// measures of Hu and Loizou (2008).  Both frame the signals as the segmental SNR does (kernels_eval.h) and end in the same
// order statistic, the mean of the lowest 95 % of the frame values.  The cepstral distance (CD) sits on LLR's lags and models
// and ends in the same order statistic; the frequency-weighted segmental SNR (fwSNRseg) sits on WSS's staging, coefficient
// stream, GEMM and filters and ends in the plain mean over the frames (eval::seg_snr_mean_kernel).
//
// The family's invariants hold: no atomics; every sum runs in one order fixed by positions inside the utterance (which lane,
// which register and which workgroup an element lands in depends on its frame and sample index only); samples past a length
// are never read; fp64 throughout, the DFT of WSS included (v_mfma_f64_16x16x4_f64): a slope's sign is a decision.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_eval.h"

namespace rced {
namespace sepm {

using eval::kThreads;
using eval::kWaves;

constexpr int kMaxW = 480;                 // 30 ms at 16 kHz; 240 at 8 kHz
constexpr int kMaxLags = 17;               // P + 1 at 16 kHz
constexpr int kLlrFramesPerBlock = 16;     // four per wave
constexpr int kBands = 25;
constexpr int kBins = 256;                 // DFT bins the GEMM takes: the filters of both rates end below bin kPowLd
constexpr int kPowLd = 249;                // row pitch of the power tile in LDS (odd: frames fall into different banks)
constexpr int kBinTilesPerWave = kBins / 16 / kWaves;

__host__ __device__ inline int lpc_order(int fs) { return fs < 10000 ? 10 : 16; }
__host__ __device__ inline long long lowest_count(int nf) { return (95ll * nf + 50) / 100; }
__device__ inline double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double hann(int j, int W) { return 0.5 * (1.0 - cos(2.0 * M_PI * (double)(j + 1) / (double)(W + 1))); }

// ---- LLR ---------------------------------------------------------------------------------------------------------

// grid (ceil(nfcap / 16), N), 4 waves: wave w takes frames 16 bx + w, + 4, + 8, + 12.  The wave's two windowed frames
// (w (x + eps), w (y + eps)) stand in LDS; lag m of a signal is summed by lane l over n = l, l + 64, ... < W - m in index
// order, then the xor butterfly.  R: [N][nfcap][2][kMaxLags], lags 0 .. P written
__global__ __launch_bounds__(kThreads) void llr_frame_kernel(const float* __restrict__ ref, int ref_stride,
                                                             const float* __restrict__ est, int est_stride,
                                                             const int* __restrict__ lengths, int cap, int W, int P,
                                                             double* __restrict__ R, int nfcap) {
  __shared__ double win[kMaxW];
  __shared__ double sig[kWaves][2][kMaxW];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = W / 4;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  const int f0 = blockIdx.x * kLlrFramesPerBlock;
  if (f0 >= nf) return;                                  // uniform over the workgroup
  for (int j = threadIdx.x; j < W; j += kThreads) win[j] = hann(j, W);
  const float* r = ref + (size_t)n * ref_stride;
  const float* e = est + (size_t)n * est_stride;
  for (int it = 0; it < kLlrFramesPerBlock / kWaves; ++it) {   // every wave runs every round: the barriers are uniform
    const int f = f0 + it * kWaves + wave;
    const bool live = f < nf;                            // uniform over the wave
    __syncthreads();                                     // win is written; the last round's reads are done
    if (live) {
      const float* x = r + (size_t)f * H;                // f H + W <= (nf - 1) H + W <= len
      const float* y = e + (size_t)f * H;
      for (int j = lane; j < W; j += 64) {
        sig[wave][0][j] = ((double)x[j] + eval::kEps64) * win[j];
        sig[wave][1][j] = ((double)y[j] + eval::kEps64) * win[j];
      }
    }
    __syncthreads();
    if (live) {
      double* out = R + ((size_t)n * nfcap + f) * 2 * kMaxLags;
      for (int s = 0; s < 2; ++s) {
        const double* v = sig[wave][s];
        for (int m = 0; m <= P; ++m) {
          double acc = 0.0;
          for (int j = lane; j < W - m; j += 64) acc += v[j] * v[j + m];
          acc = eval::wave_sum(acc);
          if (lane == 0) out[s * kMaxLags + m] = acc;
        }
      }
    }
  }
}

// Levinson-Durbin as DESIGN.md writes it, every index a constant after unrolling: the model stays in registers.
// No contraction here: the recursion rounds as the restatement's does.
template <int P>
__device__ inline void lpc_model(const double* __restrict__ R, double (&A)[P + 1]) {
#pragma clang fp contract(off)
  double a[P], ap[P];
#pragma unroll
  for (int j = 0; j < P; ++j) a[j] = 0.0;
  double E = R[0];
#pragma unroll
  for (int i = 0; i < P; ++i) {
#pragma unroll
    for (int j = 0; j < P; ++j) ap[j] = a[j];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j) s += ap[j] * R[i - j];
    const double rc = (R[i + 1] - s) / E;
    a[i] = rc;
#pragma unroll
    for (int j = 0; j < i; ++j) a[j] = ap[j] - rc * ap[i - 1 - j];
    E = (1.0 - rc * rc) * E;
  }
  A[0] = 1.0;
#pragma unroll
  for (int j = 0; j < P; ++j) A[j + 1] = -a[j];
}

// A T A^T, T the Toeplitz matrix of R: rows in order, each row's sum in column order
template <int P>
__device__ inline double toeplitz_form(const double (&A)[P + 1], const double* __restrict__ R) {
#pragma clang fp contract(off)
  double q = 0.0;
#pragma unroll
  for (int i = 0; i <= P; ++i) {
    double row = 0.0;
#pragma unroll
    for (int j = 0; j <= P; ++j) row += R[i > j ? i - j : j - i] * A[j];
    q += A[i] * row;
  }
  return q;
}

// grid (ceil(nfcap / kThreads), N): one thread per frame.  d: [N][nfcap], limited; frames_out: NULL or [N][frames_stride], unlimited
template <int P>
__global__ __launch_bounds__(kThreads) void llr_recursion_kernel(const double* __restrict__ R, const int* __restrict__ lengths,
                                                                 int cap, int W, int nfcap, double limit, double* __restrict__ d,
                                                                 double* __restrict__ frames_out, int frames_stride) {
  const int n = blockIdx.y, f = blockIdx.x * kThreads + threadIdx.x;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  if (f >= nf) return;
  const double* src = R + ((size_t)n * nfcap + f) * 2 * kMaxLags;
  double Rx[P + 1], Ry[P + 1], Ax[P + 1], Ay[P + 1];
#pragma unroll
  for (int m = 0; m <= P; ++m) {
    Rx[m] = src[m];
    Ry[m] = src[kMaxLags + m];
  }
  lpc_model<P>(Rx, Ax);
  lpc_model<P>(Ry, Ay);
  const double v = log(toeplitz_form<P>(Ay, Rx) / toeplitz_form<P>(Ax, Rx));
  if (frames_out) frames_out[(size_t)n * frames_stride + f] = v;
  d[(size_t)n * nfcap + f] = v > limit ? limit : v;      // a nan stays a nan, as np.minimum leaves it
}

// ---- CD: the cepstral distance of the same two LPC models ---------------------------------------------------------------

constexpr int kMaxOrder = kMaxLags - 1;    // the orders rced_cepd takes: 1 .. 16
constexpr double kCdScale = 4.3429448190325175;   // 10 / ln 10
constexpr double kCdMax = 10.0;

// c[1 .. P] of 1 / A(z): c[1] = -A[1], c[k] = -(A[k] + (sum_{i < k} i c[i] A[k - i]) / k), the sum in ascending i
template <int P>
__device__ inline void lpc_cepstrum(const double (&A)[P + 1], double (&c)[P + 1]) {
#pragma clang fp contract(off)
  c[0] = 0.0;
#pragma unroll
  for (int k = 1; k <= P; ++k) {
    double s = 0.0;
#pragma unroll
    for (int i = 1; i < k; ++i) s += ((double)i * c[i]) * A[k - i];
    c[k] = -(A[k] + s / (double)k);
  }
}

// grid (ceil(nfcap / kThreads), N): one thread per frame, on llr_frame_kernel's lags.  (10 / ln 10) sqrt(2 sum (cx - cy)^2)
// limited to [0, 10] (a nan stays a nan): d [N][nfcap] and frames_out, NULL or [N][frames_stride], take the same value
template <int P>
__global__ __launch_bounds__(kThreads) void cepd_recursion_kernel(const double* __restrict__ R, const int* __restrict__ lengths,
                                                                  int cap, int W, int nfcap, double* __restrict__ d,
                                                                  double* __restrict__ frames_out, int frames_stride) {
#pragma clang fp contract(off)
  const int n = blockIdx.y, f = blockIdx.x * kThreads + threadIdx.x;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  if (f >= nf) return;
  const double* src = R + ((size_t)n * nfcap + f) * 2 * kMaxLags;
  double lags[P + 1], A[P + 1], cx[P + 1], cy[P + 1];
#pragma unroll
  for (int m = 0; m <= P; ++m) lags[m] = src[m];
  lpc_model<P>(lags, A);
  lpc_cepstrum<P>(A, cx);
#pragma unroll
  for (int m = 0; m <= P; ++m) lags[m] = src[kMaxLags + m];
  lpc_model<P>(lags, A);
  lpc_cepstrum<P>(A, cy);
  double s = 0.0;
#pragma unroll
  for (int k = 1; k <= P; ++k) {
    const double diff = cx[k] - cy[k];
    s += diff * diff;
  }
  double v = kCdScale * sqrt(2.0 * s);
  v = v < 0.0 ? 0.0 : (v > kCdMax ? kCdMax : v);
  if (frames_out) frames_out[(size_t)n * frames_stride + f] = v;
  d[(size_t)n * nfcap + f] = v;
}

// ---- the mean of the k smallest of nf values -----------------------------------------------------------------------

// a before b in np.sort's order: nan last
__device__ inline bool sorts_before(double a, double b) { return a < b || (b != b && a == a); }
__device__ inline bool sorts_equal(double a, double b) { return a == b || (a != a && b != b); }

// grid (ceil(nfcap / kThreads), N): thread i counts the values that sort before its own, ties by frame index, and
// puts its value at that rank.  The ranks of an utterance are a permutation of 0 .. nf - 1: plain stores, no two alike
__global__ __launch_bounds__(kThreads) void rank_kernel(const double* __restrict__ d, const int* __restrict__ lengths, int cap,
                                                        int W, int nfcap, double* __restrict__ sorted) {
  __shared__ double tile[kThreads];
  const int n = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  if ((int)(blockIdx.x * kThreads) >= nf) return;        // uniform over the workgroup
  const double* v = d + (size_t)n * nfcap;
  const double mine = i < nf ? v[i] : 0.0;
  int rank = 0;
  for (int j0 = 0; j0 < nf; j0 += kThreads) {
    __syncthreads();
    if (j0 + (int)threadIdx.x < nf) tile[threadIdx.x] = v[j0 + threadIdx.x];
    __syncthreads();
    const int cnt = nf - j0 < kThreads ? nf - j0 : kThreads;
    for (int t = 0; t < cnt; ++t) {
      const double o = tile[t];
      rank += (sorts_before(o, mine) || (sorts_equal(o, mine) && j0 + t < i)) ? 1 : 0;
    }
  }
  if (i < nf) sorted[(size_t)n * nfcap + rank] = mine;
}

// grid (N), kThreads: lane t takes ranks t, t + kThreads, ... < k, then block_sum2: one order, fixed by the ranks
__global__ __launch_bounds__(kThreads) void lowest_mean_kernel(const double* __restrict__ sorted, const int* __restrict__ lengths,
                                                               int cap, int W, int nfcap, double* __restrict__ out,
                                                               int* __restrict__ frames) {
  __shared__ double red[kWaves][2];
  const int n = blockIdx.x;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  const int k = (int)lowest_count(nf);
  double s = 0.0, z = 0.0;
  for (int t = threadIdx.x; t < k; t += kThreads) s += sorted[(size_t)n * nfcap + t];
  eval::block_sum2<kWaves>(s, z, red);
  if (threadIdx.x == 0) {
    out[n] = nf > 0 ? s / (double)k : quiet_nan();
    if (frames) frames[n] = nf;
  }
}

// ---- WSS -----------------------------------------------------------------------------------------------------------

typedef double d4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int wss_frame_ld(int MT) { return 16 * MT + 1; }
__host__ __device__ inline size_t wss_lds_bytes(int W, int MT) {
  const size_t a = (size_t)W * wss_frame_ld(MT), b = (size_t)16 * MT * kPowLd;
  return (a > b ? a : b) * sizeof(double);
}
// doubles of the coefficient stream at a window of W samples
__host__ __device__ inline size_t wss_coef_len(int W) { return (size_t)kWaves * (W / 4) * kBinTilesPerWave * 2 * 64; }

// The windowed frames f0 .. f0 + 16 MT - 1 of one row into LDS as [sample][frame], pitch 16 MT + 1; frames at or past nf are
// zero rows: nothing past a length is read
template <int MT>
__device__ __forceinline__ void dft_stage(double* __restrict__ sh, const float* __restrict__ row, int f0, int nf, int W) {
  constexpr int FR = 16 * MT, LD = FR + 1;
  const int H = W / 4;
  for (int k = threadIdx.x; k < W; k += kThreads) {
    const double w = hann(k, W);
    for (int i = 0; i < FR; ++i)
      sh[k * LD + i] = f0 + i < nf ? w * (double)row[(size_t)(f0 + i) * H + k] : 0.0;   // (f0 + i) H + k < len
  }
}

// D[frame][bin] = sum_k A[frame][k] B[k][bin] over the staged frames, K = W in steps of 4, once with the cos and once with the
// -sin columns of `coef` (a stream of wss_coef_len(W) doubles in fragment order): wave w takes the stream's bin tiles
// 4 w .. 4 w + 3, and a lane ends with re and im of the same (frame, bin)
template <int MT>
__device__ __forceinline__ void dft_gemm(const double* __restrict__ sh, const double* __restrict__ coef, int W,
                                         d4 (&acc)[kBinTilesPerWave][MT][2]) {
  constexpr int LD = 16 * MT + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = W / 4;
#pragma unroll
  for (int q = 0; q < kBinTilesPerWave; ++q)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      acc[q][m][0] = d4{0.0, 0.0, 0.0, 0.0};
      acc[q][m][1] = d4{0.0, 0.0, 0.0, 0.0};
    }
  const double* b = coef + (size_t)wave * S * kBinTilesPerWave * 2 * 64 + lane;
  const int arow = lane >> 4, acol = lane & 15;
  // the coefficients of step s + 1 are loaded before the matrix instructions of step s: one wave per SIMD hides no latency
  double bc[kBinTilesPerWave][2], bn[kBinTilesPerWave][2];
#pragma unroll
  for (int q = 0; q < kBinTilesPerWave; ++q) {
    bc[q][0] = b[(size_t)q * 128];
    bc[q][1] = b[(size_t)q * 128 + 64];
  }
  for (int s = 0; s < S; ++s) {
    const int sn = s + 1 < S ? s + 1 : s;                // the last step loads its own again: in bounds, unused
#pragma unroll
    for (int q = 0; q < kBinTilesPerWave; ++q) {
      bn[q][0] = b[((size_t)sn * kBinTilesPerWave + q) * 128];
      bn[q][1] = b[((size_t)sn * kBinTilesPerWave + q) * 128 + 64];
    }
    double a[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) a[m] = sh[(4 * s + arow) * LD + 16 * m + acol];
#pragma unroll
    for (int q = 0; q < kBinTilesPerWave; ++q) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        acc[q][m][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bc[q][0], acc[q][m][0], 0, 0, 0);
        acc[q][m][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bc[q][1], acc[q][m][1], 0, 0, 0);
      }
      bc[q][0] = bn[q][0];
      bc[q][1] = bn[q][1];
    }
  }
}

// grid (ceil(nfcap / (16 MT)), 2, N), 4 waves: a tile of 16 MT frames of one signal (y = 0 clean, 1 estimate).
// The windowed frames stand in LDS (dft_stage); wave w takes bin tiles 4 w .. 4 w + 3 (16 bins each) of the DFT (dft_gemm).
// The powers replace the frames in LDS; then 25 sums per frame over each filter's nonzero bins in bin order.  energy: [N][2][nfcap][25] dB.
// Frames at or past nf are zero rows: nothing past a length is read.  Two workgroups share a CU (at most 256 registers a
// lane, 2 x 64 KB of LDS): one stages or sums its filters while the other holds the matrix pipe.
template <int MT>
__global__ __launch_bounds__(kThreads, 2) void wss_spectrum_kernel(const float* __restrict__ ref, int ref_stride,
                                                                const float* __restrict__ est, int est_stride,
                                                                const int* __restrict__ lengths, int cap, int W,
                                                                const double* __restrict__ coef, const double* __restrict__ filt,
                                                                const int* __restrict__ range, double* __restrict__ energy,
                                                                int nfcap) {
  extern __shared__ double sh[];
  constexpr int FR = 16 * MT;
  const int n = blockIdx.z, which = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int arow = lane >> 4, acol = lane & 15;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  const int f0 = blockIdx.x * FR;
  if (f0 >= nf) return;                                  // uniform over the workgroup
  const float* row = which ? est + (size_t)n * est_stride : ref + (size_t)n * ref_stride;
  dft_stage<MT>(sh, row, f0, nf, W);
  __syncthreads();
  d4 acc[kBinTilesPerWave][MT][2];
  dft_gemm<MT>(sh, coef, W, acc);
  __syncthreads();                                       // every wave is done with the frames
#pragma unroll
  for (int q = 0; q < kBinTilesPerWave; ++q) {
    const int bin = (wave * kBinTilesPerWave + q) * 16 + acol;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double re = acc[q][m][0][r], im = acc[q][m][1][r];
        if (bin < kPowLd) sh[(16 * m + arow + 4 * r) * kPowLd + bin] = re * re + im * im;
      }
  }
  __syncthreads();
  double* out = energy + ((size_t)(n * 2 + which) * nfcap + f0) * kBands;
  for (int t = threadIdx.x; t < FR * kBands; t += kThreads) {
    const int i = t % FR, band = t / FR;
    if (f0 + i >= nf) continue;
    const int lo = range[2 * band], hi = range[2 * band + 1];          // 0 <= lo <= hi <= kPowLd: checked where the table is built
    double sum = 0.0;
    for (int j = lo; j < hi; j += 4) {                   // four loads in flight, the additions still in bin order
      double f[4], p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jj = j + u < hi ? j + u : hi - 1;
        f[u] = filt[band * kBins + jj];
        p[u] = sh[i * kPowLd + jj];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j + u < hi) sum += f[u] * p[u];
    }
    out[(size_t)i * kBands + band] = 10.0 * log10((sum > 1e-10 || sum != sum) ? sum : 1e-10);
  }
}

// slopes and weights of one signal's 25 band energies; the peak searches as recurrences over constant indices:
// down[i] = the walk "n = i; while n >= 0 and s[n] <= 0: n -= 1" ends at e[n + 1]; up[i] = the walk "n = i; while n < 24 and
// s[n] > 0: n += 1" ends at e[n - 1]
__device__ inline void wss_weights(const double (&e)[kBands], double (&s)[kBands - 1], double (&wt)[kBands - 1]) {
#pragma clang fp contract(off)
  constexpr int NS = kBands - 1;
  double emax = e[0];
#pragma unroll
  for (int i = 1; i < kBands; ++i) emax = (e[i] > emax || e[i] != e[i]) ? e[i] : emax;
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = e[i + 1] - e[i];
  double up[NS], down[NS];
#pragma unroll
  for (int i = NS - 1; i >= 0; --i) up[i] = s[i] > 0.0 ? (i == NS - 1 ? e[NS - 1] : up[i + 1]) : e[i > 0 ? i - 1 : 0];
#pragma unroll
  for (int i = 0; i < NS; ++i) down[i] = s[i] <= 0.0 ? (i == 0 ? e[0] : down[i - 1]) : e[i + 1];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const double p = s[i] > 0.0 ? up[i] : down[i];
    wt[i] = 20.0 / (20.0 + emax - e[i]) * (1.0 / (1.0 + p - e[i]));
  }
}

// grid (ceil(nfcap / kThreads), N): one thread per frame.  d: [N][nfcap]; frames_out: NULL or [N][frames_stride]
__global__ __launch_bounds__(kThreads) void wss_slope_kernel(const double* __restrict__ energy, const int* __restrict__ lengths,
                                                             int cap, int W, int nfcap, double* __restrict__ d,
                                                             double* __restrict__ frames_out, int frames_stride) {
#pragma clang fp contract(off)
  const int n = blockIdx.y, f = blockIdx.x * kThreads + threadIdx.x;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  if (f >= nf) return;
  const double* px = energy + ((size_t)(n * 2) * nfcap + f) * kBands;
  const double* py = energy + ((size_t)(n * 2 + 1) * nfcap + f) * kBands;
  double ex[kBands], ey[kBands], sx[kBands - 1], sy[kBands - 1], wx[kBands - 1], wy[kBands - 1];
#pragma unroll
  for (int i = 0; i < kBands; ++i) {
    ex[i] = px[i];
    ey[i] = py[i];
  }
  wss_weights(ex, sx, wx);
  wss_weights(ey, sy, wy);
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int i = 0; i < kBands - 1; ++i) {
    const double w = (wx[i] + wy[i]) / 2.0, diff = sx[i] - sy[i];
    num += w * (diff * diff);
    den += w;
  }
  const double v = num / den;
  if (frames_out) frames_out[(size_t)n * frames_stride + f] = v;
  d[(size_t)n * nfcap + f] = v;
}

// ---- fwSNRseg: the frequency-weighted segmental SNR -----------------------------------------------------------------------

// LDS of fwseg_spectrum_kernel: the staged frames, then in their place the magnitudes [16 MT][nb + 1] and 16 MT sums
__host__ __device__ inline size_t fwseg_lds_bytes(int W, int MT, int nb) {
  const size_t a = (size_t)W * wss_frame_ld(MT), b = (size_t)16 * MT * (nb + 2);
  return (a > b ? a : b) * sizeof(double);
}

// grid, staging, coefficient stream and GEMM of wss_spectrum_kernel; nb = kBins PASSES bins (256 at 8 kHz, 512 at 16 kHz).
// The normalising sum takes every bin, so with PASSES = 2 the GEMM runs twice over the same staged frames: first coef (bins
// 0 .. 255, WSS's stream), whose magnitudes wait in registers, then coef_hi (bins 256 .. 511): the accumulators of one pass at
// a time keep two workgroups on a CU.  The magnitudes sqrt(re^2 + im^2) replace the frames in LDS; thread i < 16 MT adds
// frame i's bins 0 .. nb - 1 in bin order; then 25 sums per frame over each filter's nonzero bins in bin order of
// magnitude / sum.  bands: [N][2][nfcap][25], linear.  A frame of zeros gives 0 / 0 = nan in every band.
template <int MT, int PASSES>
__global__ __launch_bounds__(kThreads, 2) void fwseg_spectrum_kernel(const float* __restrict__ ref, int ref_stride,
                                                                  const float* __restrict__ est, int est_stride,
                                                                  const int* __restrict__ lengths, int cap, int W,
                                                                  const double* __restrict__ coef, const double* __restrict__ coef_hi,
                                                                  const double* __restrict__ filt, const int* __restrict__ range,
                                                                  double* __restrict__ bands, int nfcap) {
#pragma clang fp contract(off)
  extern __shared__ double sh[];
  constexpr int FR = 16 * MT, NB = kBins * PASSES, MLD = NB + 1;
  const int n = blockIdx.z, which = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int arow = lane >> 4, acol = lane & 15;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  const int f0 = blockIdx.x * FR;
  if (f0 >= nf) return;                                  // uniform over the workgroup
  const float* row = which ? est + (size_t)n * est_stride : ref + (size_t)n * ref_stride;
  dft_stage<MT>(sh, row, f0, nf, W);
  __syncthreads();
  d4 acc[kBinTilesPerWave][MT][2];
  double low[PASSES > 1 ? kBinTilesPerWave : 1][MT][4];
  dft_gemm<MT>(sh, coef, W, acc);
  if constexpr (PASSES > 1) {
#pragma unroll
    for (int q = 0; q < kBinTilesPerWave; ++q)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double re = acc[q][m][0][r], im = acc[q][m][1][r];
          low[q][m][r] = sqrt(re * re + im * im);
        }
    dft_gemm<MT>(sh, coef_hi, W, acc);
  }
  __syncthreads();                                       // every wave is done with the frames
#pragma unroll
  for (int q = 0; q < kBinTilesPerWave; ++q) {
    const int bin = (wave * kBinTilesPerWave + q) * 16 + acol;          // < kBins
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double re = acc[q][m][0][r], im = acc[q][m][1][r];
        double* at = sh + (16 * m + arow + 4 * r) * MLD + bin;          // row < FR, bin + kBins (PASSES - 1) < NB
        if constexpr (PASSES > 1) at[0] = low[q][m][r];
        at[kBins * (PASSES - 1)] = sqrt(re * re + im * im);
      }
  }
  __syncthreads();
  double* total = sh + FR * MLD;                         // FR more doubles: fwseg_lds_bytes
  if (threadIdx.x < FR) {
    const double* v = sh + threadIdx.x * MLD;
    double sum = 0.0;
    for (int j = 0; j < NB; j += 4) {                    // four loads in flight, the additions in bin order
      double p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u] = v[j + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) sum += p[u];
    }
    total[threadIdx.x] = sum;
  }
  __syncthreads();
  double* out = bands + ((size_t)(n * 2 + which) * nfcap + f0) * kBands;
  for (int t = threadIdx.x; t < FR * kBands; t += kThreads) {
    const int i = t % FR, band = t / FR;
    if (f0 + i >= nf) continue;
    const int lo = range[2 * band], hi = range[2 * band + 1];          // 0 <= lo <= hi <= kPowLd < NB: checked where the table is built
    const double all = total[i];
    double sum = 0.0;
    for (int j = lo; j < hi; j += 4) {
      double f[4], p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jj = j + u < hi ? j + u : hi - 1;
        f[u] = filt[band * kBins + jj];
        p[u] = sh[i * MLD + jj];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j + u < hi) sum += (p[u] / all) * f[u];
    }
    out[(size_t)i * kBands + band] = sum;
  }
}

// grid (ceil(nfcap / kThreads), N): one thread per frame.  sum(Wt snr) / sum(Wt) in band order, Wt = E_x^0.2,
// snr = 10 log10(E_x^2 / max((E_x - E_y)^2, eps)) limited to [-10, 35]; a nan stays a nan, as np.maximum / np.minimum leave it.
// d: [N][nfcap]; frames_out: NULL or [N][frames_stride]
__global__ __launch_bounds__(kThreads) void fwseg_band_kernel(const double* __restrict__ bands, const int* __restrict__ lengths,
                                                              int cap, int W, int nfcap, double* __restrict__ d,
                                                              double* __restrict__ frames_out, int frames_stride) {
#pragma clang fp contract(off)
  const int n = blockIdx.y, f = blockIdx.x * kThreads + threadIdx.x;
  const int nf = eval::seg_frames(eval::clamp_len(lengths, n, cap), W);
  if (f >= nf) return;
  const double* px = bands + ((size_t)(n * 2) * nfcap + f) * kBands;
  const double* py = bands + ((size_t)(n * 2 + 1) * nfcap + f) * kBands;
  double num = 0.0, den = 0.0;
  for (int i = 0; i < kBands; ++i) {
    const double ex = px[i], diff = ex - py[i], wt = pow(ex, 0.2);
    double dd = diff * diff;
    dd = (dd > eval::kEps64 || dd != dd) ? dd : eval::kEps64;
    double s = 10.0 * log10(ex * ex / dd);
    s = s < -10.0 ? -10.0 : (s > 35.0 ? 35.0 : s);
    num += wt * s;
    den += wt;
  }
  const double v = num / den;
  if (frames_out) frames_out[(size_t)n * frames_stride + f] = v;
  d[(size_t)n * nfcap + f] = v;
}

}  // namespace sepm
}  // namespace rced
