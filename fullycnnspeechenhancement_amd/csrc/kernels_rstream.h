// Resampler lanes (include/rced.h, "streaming resampler" section): the polyphase FIR of kernels_resample.h for
// audio that arrives unit by unit.  A lane's output stream is the offline result of everything pushed, delayed by D samples.
//
// One workgroup per lane and launch.  Of a lane the device keeps 1 + hist 8-byte words: the units pushed so far, and the last
// `hist` source frames as the fp64 values resample_kernel stages (int16 / 32768 or float32, the channels averaged); all zero
// is the start of an utterance.  The workgroup walks the outputs of the call in tiles of at most `tile`; for each it stages
// the frames the tile reaches in LDS -- out of the history, out of the call's own input, zero past a finished utterance's end
// -- and runs resample_kernel's loop over them: resample::fir<> and put<>, the same chain of `width` FMAs in ascending tap
// order for every output, so that the stream equals the offline result bit for bit.  Only then, behind the barrier that ends
// the last tile, does the workgroup write the lane's state: nothing is read and written by different workgroups.
// The staging, the run loop and the history shift stand here in full, the text of kernels_resample.h's stage_lane<>, fir_tile and
// shift_history<>: compiled over those, this kernel alone ran measurably slower ("One tile loop").
// The loops that store to global memory run a trip count the whole workgroup shares, with the bound as a mask inside: a trip
// count per lane compiles to "v_cmp vcc / global_store / s_or .., vcc", the sequence tools/isa_lint.py keeps out of the library.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_resample.h"
#include "rstream_plan.h"

namespace rced {
namespace rstream {

using resample::kK;
using resample::kThreads;
using resample::kWaves;

struct Params {
  const void* in;           // [S][in_frames][channels]: a push's K unit_in frames of every lane, a finish's tail (unit_in)
  int in_frames, channels;
  const int* flags;         // push: [S] active flags or nullptr (all); finish: [S] tail counts, -1 = the lane is left alone
  int finish, K;
  long long* state;         // [S][words]
  int words, hist;
  const double* table;      // [p][width]
  int p, q, left, width;
  double ratio;             // (double)sr_out / sr_in
  int unit_in, unit_out, delay, tile;
  void* out;                // [S][out_cols]: K unit_out (push), unit_out + delay (finish)
  int out_cols;
  int* out_counts;          // finish: [S] outputs owed
};

template <bool SRC_F32, bool OUT_F32>
__global__ __launch_bounds__(kThreads) void rstream_kernel(const Params P) {
  __shared__ double lds[kSpanMax];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int flag = P.flags ? P.flags[s] : 1;
  const long long orow = (long long)s * P.out_cols;
  const bool live = P.finish ? (flag >= 0 && flag < P.unit_in) : flag != 0;
  if (!live) {   // idle: the state is not touched, the input row not read
    for (int t0 = 0; t0 < P.out_cols; t0 += kThreads)
      if (t0 + tid < P.out_cols) resample::put<OUT_F32>(P.out, orow + t0 + tid, 0.0);
    if (P.finish && tid == 0) P.out_counts[s] = 0;
    return;
  }
  long long* st = P.state + (size_t)s * P.words;
  double* hist = reinterpret_cast<double*>(st + 1);
  const long long H = st[0];
  __syncthreads();   // every thread holds H before thread 0 replaces it
  const int avail = P.finish ? flag : P.K * P.unit_in;            // frames this call brings
  const long long F0 = H * P.unit_in;                             // frames before it
  const long long irow = (long long)s * P.in_frames;
  // outputs [m_lo, m_hi) of the offline result; column 0 of the lane's row holds output `first` (a push: negative at the start)
  long long m_lo = H * P.unit_out - P.delay;
  const long long first = P.finish ? (m_lo < 0 ? 0 : m_lo) : m_lo;
  if (m_lo < 0) m_lo = 0;
  long long m_hi = P.finish ? (long long)((double)(F0 + avail) * P.ratio) : (H + P.K) * P.unit_out - P.delay;
  if (m_hi > first + P.out_cols) m_hi = first + P.out_cols;       // never: unit_out + delay bounds what a finish owes
  if (m_hi < m_lo) m_hi = m_lo;
  for (int t0 = 0; t0 < P.out_cols; t0 += kThreads) {
    const int t = t0 + tid;
    const long long m = first + t;
    if (t < P.out_cols && (m < m_lo || m >= m_hi)) resample::put<OUT_F32>(P.out, orow + t, 0.0);
  }
  if (P.finish && tid == 0) P.out_counts[s] = (int)(m_hi - m_lo);

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int C = P.channels;
  for (long long m0 = m_lo; m0 < m_hi; m0 += P.tile) {
    const int Tn = (int)(m_hi - m0 < P.tile ? m_hi - m0 : P.tile);
    // stage frames j0 .. j0 + span: history below F0, the call's input from there, zero behind it
    const long long n0_first = (m0 * P.q) / P.p;
    const long long n0_last = ((m0 + Tn - 1) * P.q) / P.p;
    const long long j0 = n0_first - P.left;
    int span = (int)(n0_last - n0_first) + P.width;
    if (span > kSpanMax) span = kSpanMax;   // never: the host sizes the tile (span_bound)
    for (int e = tid; e < span; e += kThreads) {
      const long long j = j0 + e;
      double v = 0.0;
      if (j < F0) {
        const long long at = j - (F0 - P.hist);
        if (at >= 0) v = hist[at];          // always: the delay bounds how far back a push reaches
      } else if (j - F0 < avail) {
        v = resample::frame<SRC_F32>(P.in, (irow + (j - F0)) * C, C);
      }
      lds[e] = v;
    }
    __syncthreads();
    // resample_kernel's runs of same-phase outputs: class u = outputs m0 + u + v p, run g = its outputs v in [256 g, 256 g + 256)
    const int V = (Tn + P.p - 1) / P.p;
    const int G = (V + 64 * kK - 1) / (64 * kK);
    const int classes = Tn < P.p ? Tn : P.p;
    for (int w = wave; w < classes * G; w += kWaves) {
      const int u = w / G, g = w - u * G;
      const int Vu = (Tn - u + P.p - 1) / P.p;
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
        case 1: resample::fir<1>(lds, taps, P.width, xo, acc); break;
        case 2: resample::fir<2>(lds, taps, P.width, xo, acc); break;
        case 3: resample::fir<3>(lds, taps, P.width, xo, acc); break;
        default: resample::fir<4>(lds, taps, P.width, xo, acc); break;
      }
#pragma unroll
      for (int k = 0; k < kK; ++k) {
        const int v = v0 + 64 * k + lane;
        if (k < nk && v < Vu) resample::put<OUT_F32>(P.out, orow + (m0 - first) + u + (long long)v * P.p, acc[k]);
      }
    }
    __syncthreads();   // the tile's reads of LDS -- and, with the last tile, of the lane's history -- are done
  }

  if (P.finish) {   // the start of the next utterance
    for (int e0 = 0; e0 < P.words; e0 += kThreads)
      if (e0 + tid < P.words) st[e0 + tid] = 0;
    return;
  }
  // the history moves on by the call's frames: the last `hist` of (history, input).  A pass reads its 256 values, then writes them
  // `avail` frames further down; what a later pass reads lies above everything written so far.
  for (int e0 = 0; e0 < P.hist; e0 += kThreads) {
    const int e = e0 + tid;
    double v = 0.0;
    if (e < P.hist) {
      const long long g = (long long)e + avail;
      v = g < P.hist ? hist[g] : resample::frame<SRC_F32>(P.in, (irow + (g - P.hist)) * C, C);
    }
    __syncthreads();
    if (e < P.hist) hist[e] = v;
  }
  if (tid == 0) st[0] = H + P.K;
}

// started[s] = lane s is active and has taken a unit since the start of its utterance
__global__ void started_kernel(const long long* __restrict__ state, int words, const int* __restrict__ active, int S, int* __restrict__ started) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) started[s] = (!active || active[s] != 0) && state[(size_t)s * words] > 0;
}

}  // namespace rstream
}  // namespace rced
