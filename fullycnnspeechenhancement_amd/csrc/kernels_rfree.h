// Free-running resampler lanes (include/rced.h, "free-running resampler" section): the polyphase FIR of
// kernels_resample.h for audio that arrives in pieces of any size.  A lane counts in frames, not in units: it emits every output as
// soon as its last tap has arrived -- after F frames exactly A(F) = ceil((F - right) p / q) of them, rfree_plan.h -- and keeps the
// finished outputs in a ring, from which the call hands out what the caller asks for.  Nothing is delayed.
//
// One workgroup per lane and launch.  Of a lane the device keeps 2 + hist 8-byte words and the ring: the frames taken so far, the
// ring's read position (samples handed out so far), the last hist = width - 1 source frames as the fp64 values resample_kernel
// stages, and `cap` samples of the output's type.  Output m of the utterance lives in ring slot (prefill + m) mod cap, the read
// position R in slot R mod cap: all zero is the start of an utterance with `prefill` zeros in the ring.  The workgroup walks the new
// outputs in tiles of at most `tile`, stages the frames a tile reaches in LDS -- out of the history, out of the call's own input,
// zero past a finished utterance's end -- and runs resample_kernel's loop over them: resample::fir_tile and put<>, the same chain of
// `width` FMAs in ascending tap order for every output.  Behind the barrier that ends the last tile it copies the samples taken out
// of the ring, and only then writes the lane's state: nothing is read and written by different workgroups.
// The loops that store to global memory run a trip count the whole workgroup shares, with the bound as a mask inside, as in
// kernels_rstream.h (tools/isa_lint.py).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels_resample.h"
#include "rfree_plan.h"

namespace rced {
namespace rfree {

using resample::kThreads;

struct Params {
  const void* in;           // [S][in_cols][channels]
  int in_cols, channels;
  const int* counts;        // [S] frames of this call or nullptr (in_cols each); push: < 0 idle; finish: outside 0 .. in_cols left alone
  const int* take;          // push: [S] samples to hand out or nullptr (out_cols each)
  int finish;
  long long* state;         // [S][words]
  int words, hist, cap, prefill;
  const double* table;      // [p][width]
  int p, q, left, width, right;
  double ratio;             // (double)sr_out / sr_in
  int tile;
  void* out;                // [S][out_cols]
  int out_cols;
  int* out_counts;          // finish: [S] samples owed
};

template <bool SRC_F32, bool OUT_F32>
__global__ __launch_bounds__(kThreads) void rfree_kernel(const Params P) {
  using Elt = typename std::conditional<OUT_F32, float, short>::type;
  __shared__ double lds[kSpanMax];
  const int s = blockIdx.x, tid = threadIdx.x;
  int cnt = P.counts ? P.counts[s] : P.in_cols;
  const long long orow = (long long)s * P.out_cols;
  Elt* const out = static_cast<Elt*>(P.out);
  if (!P.finish && cnt > P.in_cols) cnt = P.in_cols;
  if (cnt < 0 || cnt > P.in_cols) {   // idle: the state is not touched, the input row not read
    for (int t0 = 0; t0 < P.out_cols; t0 += kThreads)
      if (t0 + tid < P.out_cols) out[orow + t0 + tid] = (Elt)0;
    if (P.finish && tid == 0) P.out_counts[s] = 0;
    return;
  }
  long long* st = P.state + (size_t)s * P.words;
  const double* hist = reinterpret_cast<const double*>(st + kHead);
  Elt* const ring = reinterpret_cast<Elt*>(st + kHead + P.hist);
  const long long F0 = st[0], R = st[1];
  __syncthreads();   // every thread holds F0 and R before thread 0 replaces them
  const long long irow = (long long)s * P.in_cols;
  // outputs [A0, A1) of the offline result are new with this call; the ring holds `have` samples before it
  const long long A0 = emitted(F0, P.p, P.q, P.right);
  long long A1 = P.finish ? (long long)((double)(F0 + cnt) * P.ratio) : emitted(F0 + cnt, P.p, P.q, P.right);
  if (A1 < A0) A1 = A0;
  long long have = P.prefill + A0 - R;
  have = have < 0 ? 0 : (have > P.cap ? P.cap : have);   // never: the state is the kernel's own
  // a push writes them into the ring, a finish behind the ring's samples into the lane's row
  if (P.finish && A1 - A0 > P.out_cols - have) A1 = A0 + (P.out_cols - have);   // never: finish_max bounds what a finish owes

  const int C = P.channels;
  for (long long m0 = A0; m0 < A1; m0 += P.tile) {
    const int Tn = (int)(A1 - m0 < P.tile ? A1 - m0 : P.tile);
    const resample::Reach reach = resample::reach_of(m0, Tn, P.p, P.q, P.left, P.width);
    resample::stage_lane<SRC_F32>(lds, reach, F0, hist, P.hist, P.in, irow, cnt, C, tid);
    __syncthreads();
    resample::fir_tile(lds, P.table, P.p, P.q, P.width, m0, Tn, reach.n0_first, tid, [&](long long t, double y) {
      const long long m = m0 + t;
      if (P.finish) resample::put<OUT_F32>(P.out, orow + have + (m - A0), y);
      else resample::put<OUT_F32>(ring, (P.prefill + m) % P.cap, y);
    });
    __syncthreads();   // the tile's reads of LDS are done; with the last tile the ring holds every new output
  }

  const long long fresh = A1 - A0;
  if (P.finish) {   // the whole ring in front of what was computed, zeros behind; then the start of the next utterance
    for (int t0 = 0; t0 < P.out_cols; t0 += kThreads) {
      const int t = t0 + tid;
      if (t < have) out[orow + t] = ring[(R + t) % P.cap];
      else if (t < P.out_cols && t >= have + fresh) out[orow + t] = (Elt)0;
    }
    if (tid == 0) P.out_counts[s] = (int)(have + fresh);
    __syncthreads();   // the ring and the history have been read
    for (int e0 = 0; e0 < P.words; e0 += kThreads)
      if (e0 + tid < P.words) st[e0 + tid] = 0;
    return;
  }
  long long total = have + fresh;
  if (total > P.cap) total = P.cap;   // never, if the caller takes what it is owed: the ring would have overrun
  long long tk = P.take ? P.take[s] : P.out_cols;
  tk = tk < 0 ? 0 : (tk > P.out_cols ? P.out_cols : tk);
  if (tk > total) tk = total;   // an underrun hands out zeros and does not move past what is there
  for (int t0 = 0; t0 < P.out_cols; t0 += kThreads) {
    const int t = t0 + tid;
    if (t < P.out_cols) out[orow + t] = t < tk ? ring[(R + t) % P.cap] : (Elt)0;
  }
  resample::shift_history<SRC_F32>(reinterpret_cast<double*>(st + kHead), P.hist, P.in, irow, cnt, C, tid);
  if (tid == 0) {
    st[0] = F0 + cnt;
    st[1] = R + tk;
  }
}

}  // namespace rfree
}  // namespace rced
