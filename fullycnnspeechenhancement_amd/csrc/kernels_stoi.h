// STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016) per utterance for a ragged batch, on the device
// (include/rced.h, "evaluation" section; the specification, stage by stage, is in DESIGN.md).  Six launches on one stream for either
// score, eight for both (stages 1-4 run once):
//   1. resample_kernel  8 kHz -> 10 kHz polyphase (5/4, 365 fp64 taps from the host), both signals, fp64 out        [or a widening copy]
//   2. energy_kernel    20 log10(|| hann * frame || + eps) of every clean frame (256 samples, hop 128), one wave per frame
//   3. mask_kernel      per utterance: max energy, the 40 dB mask, its exclusive scan -> the list of kept frames; (F, K, M)
//   4. band_kernel      the 512-point DFT of the re-windowed overlap-added kept frames, bins 7..218 only, as a GEMM with K = 256 (the
//                       second window is folded into the matrix, the zero-padded half drops out): three-part bf16 operands, six products,
//                       fp32 accumulators -- x6_dft.h, the GEMM of kernels_audio_x6.h.  The epilogue squares the accumulators in fp64 and sums them
//                       per one-third-octave band: spectra never reach memory, only sqrt(band power) [frame][15] does.
//   5. segment_kernel   one thread per (segment of 30 frames, band): normalise, clip, centre, correlate -- fp64
//      segment_ext_kernel  the extended form on the same thread map: rows normalised in registers, columns across 16 lanes -- fp64
//   6. final_kernel     the mean over segments and bands (or frames); 1e-5 where fewer than 30 spectral frames exist
// Everything but the DFT products is fp64 from the fp32 inputs.  The invariants of kernels_eval.h hold: no atomics; every sum in one
// fixed order that depends on positions inside the utterance only (never on N, the row, the neighbours or the strides: every load of
// the inputs is a scalar load); samples past a length are never read; all scratch lives in a caller-provided workspace.
//
// Row order of the DFT matrix.  Band b covers bins [lo_b, hi_b); its bins are taken two at a time ("pair slots": rows 4q .. 4q + 3 =
// re, im of bin A, re, im of bin B; an odd band's last slot has a zero second bin), so that the four accumulator registers of a lane
// always belong to ONE band.  110 pair slots -> 28 M-tiles of 16 rows (the last two slots are zero).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_eval.h"
#include "x6_dft.h"

namespace rced {
namespace stoi {

constexpr int kFs = 10000, kFrame = 256, kHop = 128, kBands = 15, kSeg = 30;
constexpr int kTapHalf = 182, kTaps = 2 * kTapHalf + 1;          // 8 kHz -> 10 kHz: up 5, down 4
constexpr int kTabWin = 368;                                     // table: taps [0, 365), pad, window [368, 624)
constexpr int kTabLen = kTabWin + kFrame;
constexpr int kMaxLen = 1 << 28;                                 // 5 * len stays a 32-bit int
constexpr double kEps = 2.220446049250313e-16;                   // np.finfo(float).eps

// bins [kBandLo[b], kBandLo[b + 1]) of rfft(512) at 10 kHz: the nearest bins to 150 * 2^((2b -+ 1) / 6)
__host__ __device__ constexpr int band_lo(int b) {
  constexpr int lo[kBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
  return lo[b];
}
// first pair slot of band b (slots of a band are contiguous)
__host__ __device__ constexpr int band_slot(int b) {
  int s = 0;
  for (int i = 0; i < b; ++i) s += (band_lo(i + 1) - band_lo(i) + 1) / 2;
  return s;
}
constexpr int kSlots = band_slot(kBands);                        // 110
struct SlotTab {
  int s[kBands + 1];
};
__host__ __device__ constexpr SlotTab slot_tab() {
  SlotTab t{};
  for (int b = 0; b <= kBands; ++b) t.s[b] = band_slot(b);
  return t;
}
constexpr int kMTiles = (kSlots + 3) / 4;                        // 28
static_assert(kSlots == 110 && kMTiles == 28, "one-third-octave table");

__host__ __device__ inline int len10k(int len, int fs) { return fs == kFs ? len : (5 * len + 3) / 4; }
__host__ __device__ inline int num_frames(int l10) { return l10 > kFrame ? (l10 - kFrame + kHop - 1) / kHop : 0; }

// ---- 1. resample ----------------------------------------------------------------------------------------------------------------
// scipy.signal.resample_poly(x, 5, 4, window = h / sum(h)): out[i] = sum_j c[182 + 4 i - 5 j] x[j], c = 5 h / sum(h), x zero outside
// [0, len); ceil(5 len / 4) outputs.  grid (blocks of 256 outputs, 2 signals, N); r: [N][2][rstride] fp64.
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ ref, int ref_stride, const float* __restrict__ est,
                                                       int est_stride, const int* __restrict__ lengths, int cap, int fs,
                                                       const double* __restrict__ tab, double* __restrict__ r, int rstride) {
  __shared__ double taps[kTaps];
  const int n = blockIdx.z, sig = blockIdx.y;
  const int len = eval::clamp_len(lengths, n, cap), l10 = len10k(len, fs);
  const int i0 = blockIdx.x * 256;
  if (i0 >= l10) return;
  const float* x = sig ? est + (size_t)n * est_stride : ref + (size_t)n * ref_stride;
  double* out = r + ((size_t)n * 2 + sig) * rstride;
  const int i = i0 + threadIdx.x;
  if (fs == kFs) {
    if (i < l10) out[i] = (double)x[i];
    return;
  }
  for (int t = threadIdx.x; t < kTaps; t += 256) taps[t] = tab[t];
  __syncthreads();
  if (i >= l10) return;
  const int c = kTapHalf + 4 * i;                     // tap index = c - 5 j in [0, 364]
  int j_lo = c - (kTaps - 1);
  j_lo = j_lo <= 0 ? 0 : (j_lo + 4) / 5;
  int j_hi = c / 5;
  if (j_hi > len - 1) j_hi = len - 1;
  double s = 0.0;
  for (int j = j_lo; j <= j_hi; ++j) s += taps[c - 5 * j] * (double)x[j];
  out[i] = s;
}

// ---- 2. frame energies ----------------------------------------------------------------------------------------------------------
// grid (ceil(fcap / 4), N), 4 waves: wave w takes frame 4 bx + w of the clean signal.  e: [N][fcap]
__global__ __launch_bounds__(256) void energy_kernel(const double* __restrict__ r, int rstride, const int* __restrict__ lengths, int cap,
                                                     int fs, const double* __restrict__ tab, double* __restrict__ e, int fcap) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nf = num_frames(len10k(eval::clamp_len(lengths, n, cap), fs));
  if (f >= nf) return;
  const double* x = r + (size_t)n * 2 * rstride + (size_t)f * kHop;
  const double* w = tab + kTabWin;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = w[4 * lane + k] * x[4 * lane + k];
    s += v * v;
  }
  s = eval::wave_sum(s);
  if (lane == 0) e[(size_t)n * fcap + f] = 20.0 * log10(sqrt(s) + kEps);
}

// ---- 3. mask + scan -------------------------------------------------------------------------------------------------------------
// grid (N), one wave.  kept: [N][fcap] frame indices in order; cnt: [N][4] = F, K, M, 0
__global__ __launch_bounds__(64) void mask_kernel(const double* __restrict__ e, const int* __restrict__ lengths, int cap, int fs, int fcap,
                                                  int* __restrict__ kept, int* __restrict__ cnt) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int nf = num_frames(len10k(eval::clamp_len(lengths, n, cap), fs));
  const double* en = e + (size_t)n * fcap;
  double mx = -INFINITY;
  for (int f = lane; f < nf; f += 64) mx = fmax(mx, en[f]);
#pragma unroll
  for (int o = 32; o; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  int k = 0;
  for (int f0 = 0; f0 < nf; f0 += 64) {
    const int f = f0 + lane;
    const bool keep = f < nf && (mx - 40.0 - en[f]) < 0.0;
    const unsigned long long m = __ballot(keep);
    if (keep) kept[(size_t)n * fcap + k + __popcll(m & ((1ull << lane) - 1ull))] = f;
    k += __popcll(m);
  }
  if (lane == 0) {
    int* c = cnt + (size_t)n * 4;
    c[0] = nf;
    c[1] = k;
    c[2] = k - 1 >= kSeg ? k - kSeg : 0;
    c[3] = 0;
  }
}

// ---- 4. DFT + one-third-octave bands ---------------------------------------------------------------------------------------------
using namespace x6dft;   // the GEMM: put_pair, AFrag, load_a, gemm_block (x6_dft.h); STOI's frame is its depth
static_assert(kFrame == kK, "a frame is the GEMM's depth");

constexpr int kWaves = 8, kThreads = kWaves * 64;
constexpr int kBlockFrames = 64;                              // spectral frames per workgroup
constexpr int kRowB = 2 * kHop + 16;                          // bytes per 128 samples of one part (+ pad): 272
constexpr int kPartB = (kBlockFrames + 1) * kRowB;            // 65 rows: 17,680
constexpr int kPairs = (kBlockFrames + 1) * (kHop / 2);       // 4,160 sample pairs
constexpr int kPowB = kMTiles * 4 * kBlockFrames * 8;         // [slot][frame] fp64: 57,344
constexpr int kBandLdsBytes = 3 * kPartB + kPowB + kFrame * 8 + (kBlockFrames + 2) * 4 + 8;
static_assert((3 * kPartB) % 16 == 0 && kBandLdsBytes <= 160 * 1024, "LDS layout");

// grid (ceil((fcap - 1) / 64), 2 signals, N), 8 waves; wave w takes M-tiles w, w + 8, ...  apack: kMTiles * kPackPerMT bf16.
// tob: [N][2][fcap][16] fp64, sqrt(band power) of spectral frame m in [.. m][band]
__global__ __launch_bounds__(kThreads) void band_kernel(const double* __restrict__ r, int rstride, const int* __restrict__ kept,
                                                        const int* __restrict__ cnt, int fcap, const unsigned short* __restrict__ apack,
                                                        const double* __restrict__ tab, double* __restrict__ tob) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* img = lds;
  double* pw = reinterpret_cast<double*>(lds + 3 * kPartB);                    // [slot][frame]
  double* win = pw + kMTiles * 4 * kBlockFrames;
  int* kp = reinterpret_cast<int*>(win + kFrame);                               // kept[f0 - 1 .. f0 + 64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fn = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.z, sig = blockIdx.y, f0 = blockIdx.x * kBlockFrames;
  const int K = cnt[(size_t)utt * 4 + 1], nsp = K - 1;
  if (nsp < kSeg || f0 >= nsp) return;                                          // uniform over the workgroup
  const double* x = r + ((size_t)utt * 2 + sig) * rstride;
  const int* kn = kept + (size_t)utt * fcap;
  if (tid < kBlockFrames + 2) {
    const int c = f0 - 1 + tid;
    kp[tid] = c >= 0 && c < K ? kn[c] : -1;
  }
  if (tid < kFrame) win[tid] = tab[kTabWin + tid];
  __syncthreads();
  // The overlap-added signal, chunk c = f0 + row (128 samples): the second half of kept frame c - 1 plus the first half of kept frame c,
  // each under the first window; rounded to fp32 once, split into three bf16 parts, two samples per store.
  for (int p = tid; p < kPairs; p += kThreads) {
    const int row = p >> 6, j = 2 * (p & 63);
    const int fa = kp[row], fb = kp[row + 1];
    double v0 = 0.0, v1 = 0.0;
    if (fa >= 0) {
      const double* s = x + (size_t)fa * kHop + kHop + j;
      v0 = win[kHop + j] * s[0];
      v1 = win[kHop + j + 1] * s[1];
    }
    if (fb >= 0) {
      const double* s = x + (size_t)fb * kHop + j;
      v0 += win[j] * s[0];
      v1 += win[j + 1] * s[1];
    }
    put_pair(img, kPartB, row * kRowB + (p & 63) * 4, (float)v0, (float)v1);
  }
  __syncthreads();
  for (int mt = wave; mt < kMTiles; mt += kWaves) {
    AFrag A;
    load_a(A, apack, mt, lane);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // sample k = 32 c + 8 kq + e of frame 16 t + fn: row (16 t + fn) + (c >> 2), byte 64 (c & 3) + 16 kq (the rows of stft_x6_kernel)
    gemm_block(A, img, kPartB, fn * kRowB + 16 * kq, 16 * kRowB, [](int c) { return (c >> 2) * kRowB + 64 * (c & 3); }, acc);
    // rows 4 kq .. 4 kq + 3 of the tile = pair slot 4 mt + kq: |A|^2 + |B|^2 in fp64, fixed order
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double a = acc[t].x, b = acc[t].y, c = acc[t].z, d = acc[t].w;
      pw[(4 * mt + kq) * kBlockFrames + 16 * t + fn] = (a * a + b * b) + (c * c + d * d);
    }
  }
  __syncthreads();
  double* out = tob + ((size_t)utt * 2 + sig) * fcap * 16;
  for (int i = tid; i < kBands * kBlockFrames; i += kThreads) {
    const int band = i >> 6, fr = i & 63;
    if (f0 + fr >= nsp) continue;
    constexpr SlotTab st = slot_tab();
    const int s0 = st.s[band], s1 = st.s[band + 1];
    double s = 0.0;
    for (int q = s0; q < s1; ++q) s += pw[q * kBlockFrames + fr];
    out[(size_t)(f0 + fr) * 16 + band] = sqrt(s);
  }
}

// ---- 5. segments ----------------------------------------------------------------------------------------------------------------
// grid (ceil(mcap / 16), N), 256 threads: thread (segment = tid >> 4, band = tid & 15).  dseg: [N][mcap], the sum over the 15 bands.
__global__ __launch_bounds__(256) void segment_kernel(const double* __restrict__ tob, const int* __restrict__ cnt, int fcap, int mcap,
                                                      double clip1, double* __restrict__ dseg) {
  __shared__ double sh[16][16];
  const int n = blockIdx.y, band = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int seg = blockIdx.x * 16 + sl;
  const int M = cnt[(size_t)n * 4 + 2];
  if (blockIdx.x * 16 >= M) return;                                             // uniform
  double d = 0.0;
  if (seg < M && band < kBands) {
    const double* px = tob + ((size_t)n * 2) * fcap * 16 + (size_t)seg * 16 + band;
    const double* py = px + (size_t)fcap * 16;
    double xs[kSeg], ys[kSeg];
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int t = 0; t < kSeg; ++t) {
      xs[t] = px[t * 16];
      ys[t] = py[t * 16];
      sx += xs[t] * xs[t];
      sy += ys[t] * ys[t];
    }
    const double c = sqrt(sx) / (sqrt(sy) + kEps);
    double my = 0.0, mx = 0.0;
#pragma unroll
    for (int t = 0; t < kSeg; ++t) {
      ys[t] = fmin(ys[t] * c, xs[t] * clip1);
      my += ys[t];
      mx += xs[t];
    }
    my /= kSeg;
    mx /= kSeg;
    double ny = 0.0, nx = 0.0;
#pragma unroll
    for (int t = 0; t < kSeg; ++t) {
      ys[t] -= my;
      xs[t] -= mx;
      ny += ys[t] * ys[t];
      nx += xs[t] * xs[t];
    }
    ny = sqrt(ny) + kEps;
    nx = sqrt(nx) + kEps;
#pragma unroll
    for (int t = 0; t < kSeg; ++t) d += (ys[t] / ny) * (xs[t] / nx);
  }
  sh[sl][band] = d;
  __syncthreads();
  if (band == 0 && seg < M) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < kBands; ++b) s += sh[sl][b];
    dseg[(size_t)n * mcap + seg] = s;
  }
}

// ---- 5x. segments, extended (ESTOI: Jensen & Taal 2016) ---------------------------------------------------------------------------
// The same grid and thread map as segment_kernel: thread (segment = tid >> 4, band = tid & 15), the 16 band-threads of a segment in
// 16 consecutive lanes; lane 15 (no band) and the lanes of segments past M hold zeros and take part in every shuffle.  No clipping,
// no scaling.  Summation order, all fp64:
//   rows     (band over the 30 frames): mean and squared norm in the thread's registers, frames 0 .. 29 in order;
//   columns  (frame over the 15 bands): a butterfly over the 16 lanes of the segment, one DPP row, in four steps -- lane ^ 1, lane ^ 2
//            (quad permutes), then the mirror of its 8 lanes, then the mirror of the 16: pairs, quads, halves, the row (each fp64
//            travels as its two 32-bit halves; a + b and b + a are the same sum, so all 16 lanes end with the same bits), lane 15
//            adding zero;
//   segment  sum of xn * yn: per thread over frames 0 .. 29 in order, then the same butterfly over the bands.
// dseg: [N][mcap], the sum over the 30 frames and 15 bands.
template <int kCtrl>
__device__ inline double dpp_add(double v) {   // v + the v of the lane kCtrl names; every lane of the row is active
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xf, 0xf, true);
  return v + __hiloint2double(hi, lo);
}
__device__ inline double band_sum16(double v) {
  v = dpp_add<0xB1>(v);      // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);      // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);     // row_half_mirror
  return dpp_add<0x140>(v);  // row_mirror
}

__global__ __launch_bounds__(256) void segment_ext_kernel(const double* __restrict__ tob, const int* __restrict__ cnt, int fcap, int mcap,
                                                          double* __restrict__ dseg) {
  const int n = blockIdx.y, band = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int seg = blockIdx.x * 16 + sl;
  const int M = cnt[(size_t)n * 4 + 2];
  if (blockIdx.x * 16 >= M) return;                                             // uniform
  const bool live = seg < M && band < kBands;
  const double* px = tob + ((size_t)n * 2) * fcap * 16 + (size_t)(live ? seg : 0) * 16 + (live ? band : 0);
  const double* py = px + (size_t)fcap * 16;
  double xs[kSeg], ys[kSeg];
  double mx = 0.0, my = 0.0;
#pragma unroll
  for (int t = 0; t < kSeg; ++t) {
    xs[t] = live ? px[t * 16] : 0.0;
    ys[t] = live ? py[t * 16] : 0.0;
    mx += xs[t];
    my += ys[t];
  }
  mx /= kSeg;
  my /= kSeg;
  double nx = 0.0, ny = 0.0;
#pragma unroll
  for (int t = 0; t < kSeg; ++t) {
    xs[t] -= mx;
    ys[t] -= my;
    nx += xs[t] * xs[t];
    ny += ys[t] * ys[t];
  }
  nx = sqrt(nx) + kEps;
  ny = sqrt(ny) + kEps;
  double d = 0.0;
#pragma unroll
  for (int t = 0; t < kSeg; ++t) {
    double x = xs[t] / nx, y = ys[t] / ny;                                      // 0 in the lanes that are not live
    const double cx = band_sum16(x) / kBands, cy = band_sum16(y) / kBands;
    x = live ? x - cx : 0.0;
    y = live ? y - cy : 0.0;
    const double qx = sqrt(band_sum16(x * x)) + kEps, qy = sqrt(band_sum16(y * y)) + kEps;
    d += (x / qx) * (y / qy);
  }
  d = band_sum16(d);
  if (band == 0 && seg < M) dseg[(size_t)n * mcap + seg] = d;
}

// ---- 6. the mean ----------------------------------------------------------------------------------------------------------------
// grid (N), 256 threads: lane t takes segments t, t + 256, ..., then the block sum of kernels_eval.h.  per: what one segment's sum is
// a sum of per unit of score -- the 15 bands (classic) or the 30 frames (extended).
__global__ __launch_bounds__(256) void final_kernel(const double* __restrict__ dseg, const int* __restrict__ cnt, int mcap, double per,
                                                    double* __restrict__ out, int* __restrict__ detail) {
  __shared__ double red[4][2];
  const int n = blockIdx.x;
  const int M = cnt[(size_t)n * 4 + 2];
  double s = 0.0, z = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) s += dseg[(size_t)n * mcap + m];
  eval::block_sum2<4>(s, z, red);
  if (threadIdx.x == 0) {
    out[n] = M > 0 ? s / (per * (double)M) : 1e-5;
    if (detail) {
      detail[(size_t)n * 3] = cnt[(size_t)n * 4];
      detail[(size_t)n * 3 + 1] = cnt[(size_t)n * 4 + 1];
      detail[(size_t)n * 3 + 2] = M;
    }
  }
}

}  // namespace stoi
}  // namespace rced
