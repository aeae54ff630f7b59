// Evaluation-loop kernels (include/rced.h, "evaluation" section): AudioParser.add_noise for a ragged batch in closed form,
// and the per-utterance SDR, SI-SDR and segmental SNR.  All are streaming reductions over ragged rows.
//
// One mapping for every kernel here: an utterance is cut into slices of kSlice samples; inside a slice, lane t of the
// workgroup owns the 16-byte groups t and t + kThreads (samples 4g .. 4g+3 of the slice).  Which lane and slice an element
// lands in therefore depends on its index inside its utterance only -- not on the batch, the row, the stride or the
// alignment -- and every sum is taken in one fixed order: per lane over its elements in index order, across the wave by
// an xor butterfly, across the four waves through LDS in wave order, across slices (second pass) in the same shape.
// Row alignment picks the load WIDTH (dwordx4 when the row base is 16-byte aligned, dword otherwise), never the order.
// No atomics: slice partials go to a workspace [N, slices, 2] with plain vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rced {
namespace eval {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroupsPerLane = 2;
constexpr int kSlice = kThreads * 4 * kGroupsPerLane;   // 2048 samples per workgroup
constexpr int kQTable = 160;                            // gain products kept in LDS: a slice spans <= kSlice / ln + 2 tiles
constexpr int kMaxLen = 1 << 30;                        // index math is 32-bit

__host__ __device__ inline int num_slices(int len) { return (len + kSlice - 1) / kSlice; }

__device__ inline double wave_sum(double v) {   // every lane ends with the same bits: a + b and b + a are the same sum
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// (a, b) summed over the workgroup, the result in every thread.  Safe to call again on the same scratch.
template <int NW>
__device__ inline void block_sum2(double& a, double& b, double (*sh)[2]) {
  a = wave_sum(a);
  b = wave_sum(b);
  if (NW > 1) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      sh[threadIdx.x >> 6][0] = a;
      sh[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = sh[0][0];
    b = sh[0][1];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      a += sh[w][0];
      b += sh[w][1];
    }
  }
}

__device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// row[p .. p+3] with everything at or past `limit` read as 0; p is a multiple of 4 whenever vec is set
__device__ inline void load4(const float* row, int p, int limit, bool vec, float v[4]) {
  if (vec && p + 4 <= limit) {
    const float4 t = *reinterpret_cast<const float4*>(row + p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p + k < limit ? row[p + k] : 0.f;
  }
}

__device__ inline int clamp_len(const int* lens, int n, int cap) {
  const int v = lens ? lens[n] : cap;
  return v < 0 ? 0 : (v > cap ? cap : v);
}

// ---- SDR ---------------------------------------------------------------------------------------------------------

// grid (slices, N): ws[n][s] = (sum y^2, sum (y_pred - y)^2) over slice s of utterance n
__global__ __launch_bounds__(kThreads) void sdr_partial_kernel(const float* __restrict__ ref, int ref_stride,
                                                               const float* __restrict__ est, int est_stride,
                                                               const int* __restrict__ lengths, int cap,
                                                               double* __restrict__ ws, int slices) {
  __shared__ double red[kWaves][2];
  const int n = blockIdx.y, s = blockIdx.x;
  const int len = clamp_len(lengths, n, cap);
  const int base = s * kSlice;
  if (base >= len) return;
  const float* r = ref + (size_t)n * ref_stride;
  const float* e = est + (size_t)n * est_stride;
  const bool rvec = aligned16(r), evec = aligned16(e);
  double sy = 0.0, se = 0.0;
#pragma unroll
  for (int j = 0; j < kGroupsPerLane; ++j) {
    const int p = base + (j * kThreads + threadIdx.x) * 4;
    if (p < len) {
      float a[4], b[4];
      load4(r, p, len, rvec, a);
      load4(e, p, len, evec, b);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < len) {
          const double y = a[k], d = (double)b[k] - y;
          sy += y * y;
          se += d * d;
        }
    }
  }
  block_sum2<kWaves>(sy, se, red);
  if (threadIdx.x == 0) *reinterpret_cast<double2*>(ws + ((size_t)n * slices + s) * 2) = make_double2(sy, se);
}

// partials of utterance n summed in slice order: lane t takes slices t, t + blockDim, ..., then block_sum2
template <int NW>
__device__ inline void sum_partials(const double* __restrict__ ws, int n, int slices, int nsl, double& a, double& b,
                                    double (*sh)[2]) {
  a = 0.0;
  b = 0.0;
  for (int j = threadIdx.x; j < nsl; j += NW * 64) {
    const double2 v = *reinterpret_cast<const double2*>(ws + ((size_t)n * slices + j) * 2);
    a += v.x;
    b += v.y;
  }
  block_sum2<NW>(a, b, sh);
}

// grid (N), one wave: SDR.sdr's last line.  y_en = 0 gives -inf, as numpy's log10(0) does.
__global__ __launch_bounds__(64) void sdr_final_kernel(const double* __restrict__ ws, const int* __restrict__ lengths,
                                                       int cap, int slices, double* __restrict__ sdr,
                                                       double* __restrict__ energies) {
  const int n = blockIdx.x;
  const int len = clamp_len(lengths, n, cap);
  double sy, se;
  sum_partials<1>(ws, n, slices, num_slices(len), sy, se, nullptr);
  if (threadIdx.x == 0) {
    sdr[n] = 10.0 * log10(sy / (se + 1.1920928955078125e-07));   // np.finfo(np.float32).eps = 2^-23
    if (energies) *reinterpret_cast<double2*>(energies + (size_t)n * 2) = make_double2(sy, se);
  }
}

// ---- SI-SDR ------------------------------------------------------------------------------------------------------
// alpha = sum(y x) / sum(x x), then 10 log10(sum((alpha x)^2) / sum((y - alpha x)^2)), x = ref, y = est: two partial passes
// over the SDR's slices and a final.  The one-pass form (Sxy^2 / Sxx against Syy - Sxy^2 / Sxx) cancels for good estimates
// and is not used.  Both sums of pass 1 run in one order, so y = 2^k x gives alpha = 2^k and a residual of exactly zero.

// grid (slices, N): ws1[n][s] = (sum y x, sum x x) over slice s of utterance n
__global__ __launch_bounds__(kThreads) void si_sdr_dot_kernel(const float* __restrict__ ref, int ref_stride,
                                                              const float* __restrict__ est, int est_stride,
                                                              const int* __restrict__ lengths, int cap,
                                                              double* __restrict__ ws1, int slices) {
  __shared__ double red[kWaves][2];
  const int n = blockIdx.y, s = blockIdx.x;
  const int len = clamp_len(lengths, n, cap);
  const int base = s * kSlice;
  if (base >= len) return;
  const float* r = ref + (size_t)n * ref_stride;
  const float* e = est + (size_t)n * est_stride;
  const bool rvec = aligned16(r), evec = aligned16(e);
  double sxy = 0.0, sxx = 0.0;
#pragma unroll
  for (int j = 0; j < kGroupsPerLane; ++j) {
    const int p = base + (j * kThreads + threadIdx.x) * 4;
    if (p < len) {
      float a[4], b[4];
      load4(r, p, len, rvec, a);
      load4(e, p, len, evec, b);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < len) {
          const double x = a[k], y = b[k];
          sxy += y * x;
          sxx += x * x;
        }
    }
  }
  block_sum2<kWaves>(sxy, sxx, red);
  if (threadIdx.x == 0) *reinterpret_cast<double2*>(ws1 + ((size_t)n * slices + s) * 2) = make_double2(sxy, sxx);
}

// grid (slices, N): every workgroup sums its utterance's pass-1 partials itself (in slice order: the same alpha in every
// workgroup and in the final), then ws2[n][s] = (sum (alpha x)^2, sum (y - alpha x)^2) over its slice.  alpha x is rounded
// before the subtraction, as numpy rounds it (no fused multiply-subtract).
__global__ __launch_bounds__(kThreads) void si_sdr_energy_kernel(const float* __restrict__ ref, int ref_stride,
                                                                 const float* __restrict__ est, int est_stride,
                                                                 const int* __restrict__ lengths, int cap,
                                                                 const double* __restrict__ ws1, double* __restrict__ ws2,
                                                                 int slices) {
  __shared__ double red[kWaves][2];
  const int n = blockIdx.y, s = blockIdx.x;
  const int len = clamp_len(lengths, n, cap);
  const int base = s * kSlice;
  if (base >= len) return;
  double sxy, sxx;
  sum_partials<kWaves>(ws1, n, slices, num_slices(len), sxy, sxx, red);
  const double alpha = sxy / sxx;
  const float* r = ref + (size_t)n * ref_stride;
  const float* e = est + (size_t)n * est_stride;
  const bool rvec = aligned16(r), evec = aligned16(e);
  double st = 0.0, sn = 0.0;
#pragma unroll
  for (int j = 0; j < kGroupsPerLane; ++j) {
    const int p = base + (j * kThreads + threadIdx.x) * 4;
    if (p < len) {
      float a[4], b[4];
      load4(r, p, len, rvec, a);
      load4(e, p, len, evec, b);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < len) {
          const double t = __dmul_rn(alpha, (double)a[k]), d = (double)b[k] - t;
          st += t * t;
          sn += d * d;
        }
    }
  }
  block_sum2<kWaves>(st, sn, red);
  if (threadIdx.x == 0) *reinterpret_cast<double2*>(ws2 + ((size_t)n * slices + s) * 2) = make_double2(st, sn);
}

// grid (N), kThreads: both sets of partials in the order the energy pass summed the first.  x = 0, y = 0 or a length of 0
// give nan (0 / 0), a zero residual gives +inf, as numpy does.  parts: NULL or [N][3] = alpha, sum (alpha x)^2, sum (y - alpha x)^2
__global__ __launch_bounds__(kThreads) void si_sdr_final_kernel(const double* __restrict__ ws1, const double* __restrict__ ws2,
                                                                const int* __restrict__ lengths, int cap, int slices,
                                                                double* __restrict__ out, double* __restrict__ parts) {
  __shared__ double red[kWaves][2];
  const int n = blockIdx.x;
  const int nsl = num_slices(clamp_len(lengths, n, cap));
  double sxy, sxx, st, sn;
  sum_partials<kWaves>(ws1, n, slices, nsl, sxy, sxx, red);
  sum_partials<kWaves>(ws2, n, slices, nsl, st, sn, red);
  if (threadIdx.x == 0) {
    out[n] = 10.0 * log10(st / sn);
    if (parts) {
      parts[(size_t)n * 3] = sxy / sxx;
      parts[(size_t)n * 3 + 1] = st;
      parts[(size_t)n * 3 + 2] = sn;
    }
  }
}

// ---- segmental SNR -----------------------------------------------------------------------------------------------
// Frames of W = (3 fs + 50) / 100 samples at hop W / 4 under w[j] = 0.5 (1 - cos(2 pi (j + 1) / (W + 1))); per frame
// 10 log10(sum (w x)^2 / (sum (w (x - y))^2 + eps) + eps) clamped to [-10, 35]; the mean over the frames.

constexpr int kSegMinW = 4, kSegMaxW = 1440;
constexpr int kSegFramesPerBlock = 16;                  // four per wave
constexpr double kEps64 = 2.220446049250313e-16;        // np.finfo(float).eps

__host__ __device__ inline int seg_window(int fs) { return (int)((3ll * fs + 50) / 100); }
__host__ __device__ inline int seg_frames(int len, int W) { return len >= W ? (len - W) / (W / 4) + 1 : 0; }

// grid (ceil(nfcap / 16), N), 4 waves: wave w takes frames 16 bx + w, + 4, + 8, + 12.  Lane l of the wave owns samples l, l + 64, ...
// of the frame, summed in index order, then the xor butterfly.  Every load is a scalar load.  snr: [N][nfcap], clamped
__global__ __launch_bounds__(kThreads) void seg_snr_frame_kernel(const float* __restrict__ ref, int ref_stride,
                                                                 const float* __restrict__ est, int est_stride,
                                                                 const int* __restrict__ lengths, int cap, int W,
                                                                 double* __restrict__ snr, int nfcap) {
  __shared__ double win[kSegMaxW];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = W / 4;
  const int nf = seg_frames(clamp_len(lengths, n, cap), W);
  const int f0 = blockIdx.x * kSegFramesPerBlock;
  if (f0 >= nf) return;                                  // uniform over the workgroup
  for (int j = threadIdx.x; j < W; j += kThreads) win[j] = 0.5 * (1.0 - cos(2.0 * M_PI * (double)(j + 1) / (double)(W + 1)));
  __syncthreads();
  const float* r = ref + (size_t)n * ref_stride;
  const float* e = est + (size_t)n * est_stride;
  for (int f = f0 + wave; f < f0 + kSegFramesPerBlock && f < nf; f += kWaves) {   // uniform over the wave
    const float* x = r + (size_t)f * H;                  // f H + W <= (nf - 1) H + W <= len
    const float* y = e + (size_t)f * H;
    double ss = 0.0, sn = 0.0;
    for (int j = lane; j < W; j += 64) {
      const double a = x[j], wx = win[j] * a, wd = win[j] * (a - (double)y[j]);
      ss += wx * wx;
      sn += wd * wd;
    }
    ss = wave_sum(ss);
    sn = wave_sum(sn);
    if (lane == 0) {
      const double s = 10.0 * log10(ss / (sn + kEps64) + kEps64);
      snr[(size_t)n * nfcap + f] = s < -10.0 ? -10.0 : (s > 35.0 ? 35.0 : s);
    }
  }
}

// grid (N), kThreads: lane t takes frames t, t + kThreads, ..., then block_sum2; no frame gives nan.  frames: NULL or [N] = nf
__global__ __launch_bounds__(kThreads) void seg_snr_mean_kernel(const double* __restrict__ snr, const int* __restrict__ lengths,
                                                                int cap, int W, int nfcap, double* __restrict__ out,
                                                                int* __restrict__ frames) {
  __shared__ double red[kWaves][2];
  const int n = blockIdx.x;
  const int nf = seg_frames(clamp_len(lengths, n, cap), W);
  double s = 0.0, z = 0.0;
  for (int f = threadIdx.x; f < nf; f += kThreads) s += snr[(size_t)n * nfcap + f];
  block_sum2<kWaves>(s, z, red);
  if (threadIdx.x == 0) {
    out[n] = nf > 0 ? s / (double)nf : __longlong_as_double(0x7ff8000000000000ll);
    if (frames) frames[n] = nf;
  }
}

// ---- add_noise ---------------------------------------------------------------------------------------------------

// The noise the reference lays under sample p of an utterance (speech length ls, noise length ln):
//   ls >= ln: the buffer that doubles ceil((ls-ln)/ln) times, noise = (noise, noise * u_i): position p = q * ln + r holds
//             noise[r] * prod(u_k for every bit k set in q);
//   ls <  ln: noise[start + p].
struct NoiseTile {
  const float* row;
  const double* gains;
  const double* qtab;
  int ls, ln, start, n_gains, q_lo;
  bool tile, vec, table;

  __device__ double gain_prod(int q) const {
    double g = 1.0;
    for (int k = 0; k < n_gains && (q >> k); ++k)
      if ((q >> k) & 1) g *= gains[k];
    return g;
  }
  __device__ double gain(int q) const { return table ? qtab[q - q_lo] : gain_prod(q); }

  // Called by every thread of the workgroup (it holds a barrier); base = first sample of the slice, base < ls.
  __device__ void init(const float* noise_row, int ls_, int ln_, int start_, const double* gains_row, int n_gains_,
                       int base, double* qtab_lds) {
    row = noise_row; ls = ls_; ln = ln_; gains = gains_row; n_gains = gains_row ? n_gains_ : 0; qtab = qtab_lds;
    tile = ls >= ln;
    vec = aligned16(noise_row);
    start = 0; q_lo = 0; table = false;
    if (!tile) {
      const int room = ln - ls;
      start = start_ < 0 ? 0 : (start_ > room ? room : start_);
    } else if (ln > 0) {
      const int end = base + kSlice < ls ? base + kSlice : ls;
      q_lo = base / ln;
      const int nq = (end - 1) / ln - q_lo + 1;
      table = nq <= kQTable;     // otherwise ln is tiny: multiply out from the bits per element
      if (table)
        for (int j = threadIdx.x; j < nq; j += kThreads) qtab_lds[j] = gain_prod(q_lo + j);
    }
    __syncthreads();
  }

  // w[k] = the noise under sample p + k (fp64, exact products of an fp32 and the fp64 gain product); 0 past ls
  __device__ void get4(int p, double w[4]) const {
    if (!tile) {
      float v[4];
      const int i = start + p;
      load4(row, i, start + ls, vec && (i & 3) == 0, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = v[k];
    } else if (ln <= 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = 0.0;
    } else {
      int q = p / ln, r = p - q * ln;      // the one division of this 16-byte group
      if (vec && (r & 3) == 0 && r + 4 <= ln) {
        const float4 t = *reinterpret_cast<const float4*>(row + r);
        const double g = gain(q);
        w[0] = t.x * g; w[1] = t.y * g; w[2] = t.z * g; w[3] = t.w * g;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          w[k] = p + k < ls ? (double)row[r] * gain(q) : 0.0;
          if (++r == ln) { r = 0; ++q; }
        }
      }
    }
  }
};

// grid (slices of Ls, N): ws[n][s] = (sum speech^2, sum tiled_noise^2) over slice s of [0, ls)
__global__ __launch_bounds__(kThreads) void mix_partial_kernel(const float* __restrict__ speech, const int* __restrict__ speech_len,
                                                               int Ls, const float* __restrict__ noise,
                                                               const int* __restrict__ noise_len, int Ln,
                                                               const int* __restrict__ start, const double* __restrict__ gains,
                                                               int n_gains, double* __restrict__ ws, int slices) {
  __shared__ double red[kWaves][2];
  __shared__ double qtab[kQTable];
  const int n = blockIdx.y, s = blockIdx.x;
  const int ls = clamp_len(speech_len, n, Ls), ln = clamp_len(noise_len, n, Ln);
  const int base = s * kSlice;
  if (base >= ls) return;
  const float* srow = speech + (size_t)n * Ls;
  const bool svec = aligned16(srow);
  NoiseTile nt;
  nt.init(noise + (size_t)n * Ln, ls, ln, start && ls < ln ? start[n] : 0, gains ? gains + (size_t)n * n_gains : nullptr,
          n_gains, base, qtab);
  double ps = 0.0, pb = 0.0;
#pragma unroll
  for (int j = 0; j < kGroupsPerLane; ++j) {
    const int p = base + (j * kThreads + threadIdx.x) * 4;
    if (p < ls) {
      float a[4];
      double w[4];
      load4(srow, p, ls, svec, a);
      nt.get4(p, w);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < ls) {
          const double y = a[k];
          ps += y * y;
          pb += w[k] * w[k];
        }
    }
  }
  block_sum2<kWaves>(ps, pb, red);
  if (threadIdx.x == 0) *reinterpret_cast<double2*>(ws + ((size_t)n * slices + s) * 2) = make_double2(ps, pb);
}

// grid (slices of Ls, N): every workgroup sums its utterance's partials itself (in slice order), then
// mix = speech + sqrt(p_sig / 10^(snr/10) / p_back) * tiled_noise in fp64, rounded once at the fp32 store; 0 past ls.
__global__ __launch_bounds__(kThreads) void mix_apply_kernel(const float* __restrict__ speech, const int* __restrict__ speech_len,
                                                             int Ls, const float* __restrict__ noise,
                                                             const int* __restrict__ noise_len, int Ln,
                                                             const int* __restrict__ start, const double* __restrict__ gains,
                                                             int n_gains, const double* __restrict__ ws, int slices,
                                                             double snr_lin, float* __restrict__ mix) {
  __shared__ double red[kWaves][2];
  __shared__ double qtab[kQTable];
  const int n = blockIdx.y, s = blockIdx.x;
  const int ls = clamp_len(speech_len, n, Ls), ln = clamp_len(noise_len, n, Ln);
  const int base = s * kSlice;
  const float* srow = speech + (size_t)n * Ls;
  float* orow = mix + (size_t)n * Ls;
  const bool svec = aligned16(srow), ovec = aligned16(orow);
  const bool live = base < ls;                      // uniform over the workgroup
  double scale = 0.0;
  NoiseTile nt;
  if (live) {
    double ps, pb;
    sum_partials<kWaves>(ws, n, slices, num_slices(ls), ps, pb, red);
    scale = sqrt(ps / snr_lin / pb);                // IEEE like numpy: p_back = 0 gives inf or nan
    nt.init(noise + (size_t)n * Ln, ls, ln, start && ls < ln ? start[n] : 0, gains ? gains + (size_t)n * n_gains : nullptr,
            n_gains, base, qtab);
  }
#pragma unroll
  for (int j = 0; j < kGroupsPerLane; ++j) {
    const int p = base + (j * kThreads + threadIdx.x) * 4;
    if (p >= Ls) continue;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (live && p < ls) {
      float a[4];
      double w[4];
      load4(srow, p, ls, svec, a);
      nt.get4(p, w);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < ls) o[k] = (float)((double)a[k] + scale * w[k]);
    }
    if (ovec && p + 4 <= Ls) {
      *reinterpret_cast<float4*>(orow + p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < Ls) orow[p + k] = o[k];
    }
  }
}

// ---- ragged crop-gather from a PCM arena (the loader's other half) -------------------------------------------------------------
//
// grid (column blocks of kSlice, N): lane t of block x owns the 8 output columns 8 (x kThreads + t) .. + 7 of row n, two
// 16-byte stores.  A row's source starts at any sample of the arena, so its 16-byte phase (begin mod 8 for int16, mod 4 for
// float32) is whatever the corpus index says -- but it is ONE phase for the whole row, uniform over the workgroup: the lanes
// load the aligned 16-byte groups that cover their columns and pick their samples out of them at compile-time positions
// (a switch over the phase, no indexed registers).  Only the last lanes of a row, and a row whose covering groups would
// leave the arena, read sample by sample.  A copy with an exact conversion: nothing is summed, every output element has one
// source element, so the result cannot depend on the batch around it.

constexpr int kGatherPerLane = 8;

// v[k] = sample P + k of the 16 int16 held in lo | hi, as float: value / 32768 (a power of two: exact)
template <int P>
__device__ inline void unpack_s16(const uint4& lo, const uint4& hi, float v[kGatherPerLane]) {
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int k = 0; k < kGatherPerLane; ++k) {
    const unsigned d = w[(P + k) >> 1];
    const short s = (short)(((P + k) & 1) ? (d >> 16) : (d & 0xffffu));
    v[k] = (float)s * (1.f / 32768.f);
  }
}

// v[k] = sample P + k of the 12 floats held in a | b | c
template <int P>
__device__ inline void pick_f32(const float4& a, const float4& b, const float4& c, float v[kGatherPerLane]) {
  const float w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k = 0; k < kGatherPerLane; ++k) v[k] = w[P + k];
}

template <bool F32>
__global__ __launch_bounds__(kThreads) void gather_pcm_kernel(const void* __restrict__ arena, long long arena_samples,
                                                              const long long* __restrict__ begin, const int* __restrict__ count,
                                                              int L, float* __restrict__ rows, int row_stride) {
  const int n = blockIdx.y;
  const int j = (blockIdx.x * kThreads + threadIdx.x) * kGatherPerLane;
  if (j >= L) return;
  // the row's range, clamped into the arena: nothing below reads outside [b, b + c)
  long long b = begin[n];
  b = b < 0 ? 0 : (b > arena_samples ? arena_samples : b);
  int c = count[n];
  c = c < 0 ? 0 : (c > L ? L : c);
  if ((long long)c > arena_samples - b) c = (int)(arena_samples - b);
  float v[kGatherPerLane] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (j < c) {
    const long long s = b + j;                     // first source sample of this lane
    const bool full = j + kGatherPerLane <= c;     // all 8 columns inside the row's count
    const bool avec = aligned16(arena);
    if (!F32) {
      const short* src = static_cast<const short*>(arena);
      const int p = (int)(s & 7);                  // = b & 7: j is a multiple of 8
      const long long a = s - p;                   // a >= 0, and a + 8 <= s + 8 <= b + c <= arena_samples when full
      if (avec && full && (p == 0 || a + 16 <= arena_samples)) {
        const uint4 lo = *reinterpret_cast<const uint4*>(src + a);
        const uint4 hi = p ? *reinterpret_cast<const uint4*>(src + a + 8) : lo;
        switch (p) {
          case 0: unpack_s16<0>(lo, hi, v); break;
          case 1: unpack_s16<1>(lo, hi, v); break;
          case 2: unpack_s16<2>(lo, hi, v); break;
          case 3: unpack_s16<3>(lo, hi, v); break;
          case 4: unpack_s16<4>(lo, hi, v); break;
          case 5: unpack_s16<5>(lo, hi, v); break;
          case 6: unpack_s16<6>(lo, hi, v); break;
          default: unpack_s16<7>(lo, hi, v); break;
        }
      } else {
#pragma unroll
        for (int k = 0; k < kGatherPerLane; ++k)
          if (j + k < c) v[k] = (float)src[s + k] * (1.f / 32768.f);
      }
    } else {
      const float* src = static_cast<const float*>(arena);
      const int p = (int)(s & 3);
      const long long a = s - p;                   // a + 8 <= arena_samples when full, as above
      if (avec && full && (p == 0 || a + 12 <= arena_samples)) {
        const float4 f0 = *reinterpret_cast<const float4*>(src + a);
        const float4 f1 = *reinterpret_cast<const float4*>(src + a + 4);
        const float4 f2 = p ? *reinterpret_cast<const float4*>(src + a + 8) : f1;
        switch (p) {
          case 0: pick_f32<0>(f0, f1, f2, v); break;
          case 1: pick_f32<1>(f0, f1, f2, v); break;
          case 2: pick_f32<2>(f0, f1, f2, v); break;
          default: pick_f32<3>(f0, f1, f2, v); break;
        }
      } else {
#pragma unroll
        for (int k = 0; k < kGatherPerLane; ++k)
          if (j + k < c) v[k] = src[s + k];
      }
    }
  }
  // columns [c, L) are zeros; columns [L, row_stride) belong to the caller
  float* orow = rows + (size_t)n * row_stride;
  if (aligned16(orow) && j + kGatherPerLane <= L) {
    *reinterpret_cast<float4*>(orow + j) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(orow + j + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
#pragma unroll
    for (int k = 0; k < kGatherPerLane; ++k)
      if (j + k < L) orow[j + k] = v[k];
  }
}

}  // namespace eval
}  // namespace rced
