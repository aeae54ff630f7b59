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

namespace rced {
namespace resample {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kK = 4;              // same-phase outputs per lane and run
constexpr int kSpanMax = 6144;     // staged frames per workgroup: 48 KB of fp64
constexpr int kTileMax = 4096;     // outputs per workgroup, at most
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
  int tile;                  // outputs per workgroup: span(tile) <= kSpanMax (host: tile_for)
  void* out;
  const long long* out_begin;   // nullptr: row n at out + n * row_stride, zeros from its length to L
  int row_stride, L;
};

// the span of `tile` consecutive outputs is at most ((tile - 1) q) / p + 1 + width frames
__host__ __device__ inline long long span_bound(int tile, int p, int q, int width) {
  return ((long long)(tile - 1) * q) / p + 1 + width;
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

  // stage frames j0 .. j0 + span of the row
  const long long n0_first = (m0 * P.q) / P.p;
  const long long n0_last = ((m0 + Tn - 1) * P.q) / P.p;
  const long long j0 = n0_first - P.left;
  int span = (int)(n0_last - n0_first) + P.width;
  if (span > kSpanMax) span = kSpanMax;   // never: the host sizes the tile (span_bound)
  const int C = P.channels;
  const double inv = 1.0 / 32768.0;
  for (int e = tid; e < span; e += kThreads) {
    const long long j = j0 + e;
    double v = 0.0;
    if (j >= 0 && j < c) {
      const long long at = (b + j) * C;
      if (SRC_F32) {
        const float* s = static_cast<const float*>(P.src) + at;
        v = (double)s[0];
        for (int ch = 1; ch < C; ++ch) v += (double)s[ch];
      } else {
        const short* s = static_cast<const short*>(P.src) + at;
        v = (double)s[0] * inv;
        for (int ch = 1; ch < C; ++ch) v += (double)s[ch] * inv;
      }
      if (C > 1) v /= (double)C;
    }
    lds[e] = v;
  }
  __syncthreads();

  // runs of same-phase outputs: class u = outputs m0 + u + v p; run g = its outputs v in [256 g, 256 g + 256)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int V = (Tn + P.p - 1) / P.p;
  const int G = (V + 64 * kK - 1) / (64 * kK);
  const int classes = Tn < P.p ? Tn : P.p;
  for (int w = wave; w < classes * G; w += kWaves) {
    const int u = w / G, g = w - u * G;
    const int Vu = (Tn - u + P.p - 1) / P.p;   // outputs of class u in this tile, >= 1
    const int v0 = g * 64 * kK;
    if (v0 >= Vu) continue;
    const int left_v = Vu - v0;
    const int nk = left_v >= 64 * kK ? kK : (left_v + 63) / 64;
    const long long a = (m0 + u) * P.q;
    const long long n0u = a / P.p;
    const int r = (int)(a - n0u * P.p);
    const double* taps = P.table + (size_t)r * P.width;
    int xo[kK];
    double acc[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      int v = v0 + 64 * k + lane;
      if (v > Vu - 1) v = Vu - 1;   // idle lanes recompute the class's last output: every read stays inside the span
      xo[k] = (int)(n0u - n0_first) + v * P.q;
      acc[k] = 0.0;
    }
    switch (nk) {
      case 1: fir<1>(lds, taps, P.width, xo, acc); break;
      case 2: fir<2>(lds, taps, P.width, xo, acc); break;
      case 3: fir<3>(lds, taps, P.width, xo, acc); break;
      default: fir<4>(lds, taps, P.width, xo, acc); break;
    }
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      const int v = v0 + 64 * k + lane;
      if (k < nk && v < Vu) put<OUT_F32>(P.out, obase + m0 + u + (long long)v * P.p, acc[k]);
    }
  }
}

}  // namespace resample
}  // namespace rced
