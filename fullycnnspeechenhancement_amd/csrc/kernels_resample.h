// Sample-rate conversion (include/rced.h, "resample" section): a ragged p-phase polyphase FIR in fp64.
//
//   y[m] = sum_i x[n0 + i - left] * table[r][i],  i = 0 .. width - 1,   (n0, r) = divmod(m q, p)
//
// One workgroup takes `tile` consecutive outputs of one row.  It stages the source frames those outputs can reach -- a span of
// at most kSpanMax frames -- in LDS once, as fp64: int16 / 32768 or float32, the channels averaged ((c0 + c1 + ..) / C in
// channel order), zero outside the row's own range [0, count).  Nothing outside [begin, begin + count) is read.
//
// Outputs of one phase lie p apart (r depends on m mod p only), their first inputs q apart.  A wave takes up to 64 * kK of
// them at a time: lane l owns outputs v = l, l + 64, .. of the run, so a phase's tap is one wave-uniform read (the compiler
// turns it into a scalar load: the table stays in the scalar cache / L2, whatever its size) that feeds kK FMAs per lane,
// and every LDS read carries an immediate offset off one per-output base address.  Every output is the same chain of
// `width` fp64 FMAs, i ascending -- ascending position inside the utterance --, whatever tile, lane, row or batch it falls
// in: results are bit-identical from run to run and independent of N, the row, begin's alignment and the neighbours.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resample_plan.h"

namespace rced {
namespace resample {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLen = 1 << 30;   // outputs per row

struct Params {
  const void* src;           // interleaved frames
  long long src_frames;
  int channels;
  const long long* begin;    // [N] first frame
  const int* count;          // [N] frames
  const double* table;       // [p][width]
  int p, q, left, width;
  double ratio;              // (double)sr_new / sr_orig
  int tile;                  // outputs per workgroup: span(tile) <= kSpanMax (resample_plan.h: tile_for)
  void* out;
  const long long* out_begin;   // nullptr: row n at out + n * row_stride, zeros from its length to L
  int row_stride, L;
};

// the frame whose first value is element `at` of interleaved PCM, as every kernel here stages it: fp64, the channels averaged
template <bool SRC_F32>
__device__ inline double frame(const void* in, long long at, int C) {
  double v;
  const double inv = 1.0 / 32768.0;
  if (SRC_F32) {
    const float* s = static_cast<const float*>(in) + at;
    v = (double)s[0];
    for (int ch = 1; ch < C; ++ch) v += (double)s[ch];
  } else {
    const short* s = static_cast<const short*>(in) + at;
    v = (double)s[0] * inv;
    for (int ch = 1; ch < C; ++ch) v += (double)s[ch] * inv;
  }
  if (C > 1) v /= (double)C;
  return v;
}

// what the Tn outputs from m0 on reach: frames j0 .. j0 + span of the utterance, LDS slot 0 holding frame j0 = n0_first - left
struct Reach {
  long long n0_first, j0;
  int span;
};
__device__ inline Reach reach_of(long long m0, int Tn, int p, int q, int left, int width) {
  Reach R;
  R.n0_first = (m0 * q) / p;
  const long long n0_last = ((m0 + Tn - 1) * q) / p;
  R.j0 = R.n0_first - left;
  R.span = (int)(n0_last - R.n0_first) + width;
  if (R.span > kSpanMax) R.span = kSpanMax;   // never: the host sizes the tile (span_bound)
  return R;
}

template <int KK>
__device__ inline void fir(const double* __restrict__ lds, const double* __restrict__ taps, int width, const int (&xo)[kK],
                           double (&acc)[kK]) {
  const double* x[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) x[k] = lds + xo[k];
#pragma unroll 8
  for (int i = 0; i < width; ++i) {
    const double t = taps[i];   // wave-uniform
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[k] = fma(x[k][i], t, acc[k]);
  }
}

template <bool OUT_F32>
__device__ inline void put(void* out, long long at, double y) {
  if (OUT_F32) {
    static_cast<float*>(out)[at] = (float)y;
  } else {   // clip(rint(y * 32768)), ties to even
    double v = rint(y * 32768.0);
    v = v < -32768.0 ? -32768.0 : (v > 32767.0 ? 32767.0 : v);
    static_cast<short*>(out)[at] = (short)(int)v;
  }
}

// The Tn outputs from m0 on, out of the staged frames: runs of same-phase outputs, class u = outputs m0 + u + v p, run g = its outputs
// v in [256 g, 256 g + 256).  store(t, y): output m0 + t of the utterance.  The trip counts are the wave's; the bound is a mask at the
// store.  t and not m: the caller adds m0 to its own row base, one scalar sum a tile.
// rstream_kernel (kernels_rstream.h) carries a copy of this loop, of stage_lane<> and of shift_history<>: an edit here goes there too.
template <class Store>
__device__ __forceinline__ void fir_tile(const double* __restrict__ lds, const double* __restrict__ table, int p, int q, int width, long long m0,
                                         int Tn, long long n0_first, int tid, Store store) {
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int V = (Tn + p - 1) / p;
  const int G = (V + kRun - 1) / kRun;
  const int classes = Tn < p ? Tn : p;
  for (int w = wave; w < classes * G; w += kWaves) {
    const int u = w / G, g = w - u * G;
    const int Vu = (Tn - u + p - 1) / p;   // outputs of class u in this tile, >= 1
    const int v0 = g * kRun;
    if (v0 >= Vu) continue;
    const int left_v = Vu - v0;
    const int nk = left_v >= kRun ? kK : (left_v + 63) / 64;
    const long long a = (m0 + u) * q;
    const long long n0u = a / p;
    const int r = (int)(a - n0u * p);
    const double* taps = table + (size_t)r * width;
    int xo[kK];
    double acc[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      int v = v0 + 64 * k + lane;
      if (v > Vu - 1) v = Vu - 1;   // idle lanes recompute the class's last output: every read stays inside the span
      xo[k] = (int)(n0u - n0_first) + v * q;
      acc[k] = 0.0;
    }
    switch (nk) {
      case 1: fir<1>(lds, taps, width, xo, acc); break;
      case 2: fir<2>(lds, taps, width, xo, acc); break;
      case 3: fir<3>(lds, taps, width, xo, acc); break;
      default: fir<4>(lds, taps, width, xo, acc); break;
    }
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      const int v = v0 + 64 * k + lane;
      if (k < nk && v < Vu) store(u + (long long)v * p, acc[k]);
    }
  }
}

// A lane's tile staged: the lane's history (its last `nh` frames) below frame F0, the call's `avail` frames from there -- row `irow`
// of `in` --, zero behind them.
template <bool SRC_F32>
__device__ __forceinline__ void stage_lane(double* __restrict__ lds, const Reach R, long long F0, const double* hist, int nh, const void* in,
                                           long long irow, long long avail, int C, int tid) {
  for (int e = tid; e < R.span; e += kThreads) {
    const long long j = R.j0 + e;
    double v = 0.0;
    if (j < F0) {
      const long long at = j - (F0 - nh);
      if (at >= 0) v = hist[at];          // always: the plan's history covers how far back a push reaches
    } else if (j - F0 < avail) {
      v = frame<SRC_F32>(in, (irow + (j - F0)) * C, C);
    }
    lds[e] = v;
  }
}

// A lane's history moves on by the call's frames: the last `nh` of (history, input).  A pass reads its 256 values, then writes them
// `avail` frames further down; what a later pass reads lies above everything written so far.
template <bool SRC_F32>
__device__ __forceinline__ void shift_history(double* hist, int nh, const void* in, long long irow, long long avail, int C, int tid) {
  for (int e0 = 0; e0 < nh; e0 += kThreads) {
    const int e = e0 + tid;
    double v = 0.0;
    if (e < nh) {
      const long long g = (long long)e + avail;
      v = g < nh ? hist[g] : frame<SRC_F32>(in, (irow + (g - nh)) * C, C);
    }
    __syncthreads();
    if (e < nh) hist[e] = v;
  }
}

template <bool SRC_F32, bool OUT_F32>
__global__ __launch_bounds__(kThreads) void resample_kernel(const Params P) {
  __shared__ double lds[kSpanMax];
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * P.tile;
  // the row's range, clamped into the source: nothing below reads outside [b, b + c)
  long long b = P.begin[n];
  b = b < 0 ? 0 : (b > P.src_frames ? P.src_frames : b);
  long long c = P.count[n];
  c = c < 0 ? 0 : c;
  if (c > P.src_frames - b) c = P.src_frames - b;
  long long M = (long long)((double)c * P.ratio);   // the row's output length
  if (M > P.L) M = P.L;
  const long long obase = P.out_begin ? P.out_begin[n] : (long long)n * P.row_stride;

  if (!P.out_begin) {   // the padding of this tile's columns
    for (int t = tid; t < P.tile; t += kThreads) {
      const long long m = m0 + t;
      if (m >= M && m < P.L) put<OUT_F32>(P.out, obase + m, 0.0);
    }
  }
  if (m0 >= M) return;
  const int Tn = (int)(M - m0 < P.tile ? M - m0 : P.tile);   // outputs of this tile

  // stage the frames of the row the tile reaches, zero outside [0, c)
  const Reach reach = reach_of(m0, Tn, P.p, P.q, P.left, P.width);
  const int C = P.channels;
  for (int e = tid; e < reach.span; e += kThreads) {
    const long long j = reach.j0 + e;
    lds[e] = j >= 0 && j < c ? frame<SRC_F32>(P.src, (b + j) * C, C) : 0.0;
  }
  __syncthreads();
  fir_tile(lds, P.table, P.p, P.q, P.width, m0, Tn, reach.n0_first, tid, [&](long long t, double y) { put<OUT_F32>(P.out, obase + m0 + t, y); });
}

}  // namespace resample
}  // namespace rced
