// The arithmetic of a denoiser lane at a framing (W, S, window name) -- include/rced.h, "streaming at a framing"; DESIGN.md 3.4j --,
// apart from the device: the delay, what a lane keeps between pushes and where, the rows of a finish, what a finish owes, and the
// refusals.  Host only, no HIP: stream_api.hip plans with it at create, kernels_stream_fr.h takes its constants and index functions
// (plain constexpr), tests/stream_fr_plan_check.cpp checks it as a program of its own.
//
// Hop = S samples, R = ceil(W / S).  Frame t covers samples tS .. tS + W - 1: its last sample lies in hop t + R - 1, so after H hops
// the frames 0 .. H - R are complete, and a push of K hops completes frames H - R + 1 .. H + K - R (a negative index: a zero row).
// A mask needs 4 future frames and a rebuilt hop h its frames h - R + 1 .. h, so a push to a lane at H hops hands out hops
// H - R - 3 .. H + K - R - 4: the delay is D = (R + 3) S samples.
#pragma once
#include <cstddef>
#include <cstdio>

namespace rced {
namespace stream_fr {

constexpr int kMaxWindow = 256;    // rfft(256) would crop a longer frame
constexpr int kMaxOverlap = 8;     // R at most: state and delay stay finite (W = 256 at S = 32 and up)
constexpr int kKeep = 7;           // frames kept in front of the new ones: 3 past + 4 future of the first layer
constexpr int kFuture = 4;
constexpr int kMaxHops = 64;
constexpr int kBins = 129;

// per-lane state, floats; all zero = the start of an utterance
constexpr int kStHops = 0;                          // int: hops pushed
constexpr int kStSample = 1;                        // the last input sample (pre-emphasis carry)
constexpr int kStCarry = 2;                         // the de-emphasis carry: the last output sample (word 3 is unused)
constexpr int kStTail = 4;                          // the last (R - 1) S input samples, pre-emphasised, oldest first (W - S where S divides W)
constexpr int kStPend = kStTail + kMaxWindow;       // numerator addends of the next W - S output samples, summed in ascending frame order
constexpr int kStPhase = kStPend + kMaxWindow;      // phase of the 7 kept frames [7, 129, 2]
constexpr int kStMag = kStPhase + kKeep * kBins * 2;   // magnitude of the 7 kept frames [7, 129]
constexpr int kStFloats = (kStMag + kKeep * kBins + 3) & ~3;
static_assert(kStPhase % 2 == 0 && kStFloats % 2 == 0, "phase pairs stay 8-byte aligned");

enum { kPlanOk = 0, kPlanArg = 1 };
enum { kRebuildReference = 0, kRebuildOla = 1 };

constexpr int overlap(int W, int S) { return (W + S - 1) / S; }                       // R
constexpr int delay_hops(int W, int S) { return overlap(W, S) + 3; }
constexpr int delay(int W, int S) { return delay_hops(W, S) * S; }                    // D
constexpr int tail_len(int W, int S) { return (overlap(W, S) - 1) * S; }              // < W: frame H - R + 1 starts that far back
constexpr int pend_len(int W, int S) { return W - S; }                                // frames <= h reach sample hS + W - 1
// A finish is a push of this many hops made of the tail and zeros: its outputs are hops H - R - 3 .. H, and hop H holds the tail.
constexpr int finish_slots(int W, int S) { return overlap(W, S) + kFuture; }
constexpr int finish_max(int W, int S) { return finish_slots(W, S) * S; }             // floats per lane of a finish's output: D + S
constexpr int kMaxFinishSlots = kMaxOverlap + kFuture;

// ceil(|L - W| / S + 1) (audio_feature.py:70); 0 for an empty signal
constexpr int num_frames(long long L, int W, int S) {
  return L <= 0 ? 0 : (int)(((L >= W ? L - W : W - L) + S - 1) / S + 1);
}
// frames complete after H hops
constexpr long long complete(long long H, int W, int S) { return H - overlap(W, S) + 1 > 0 ? H - overlap(W, S) + 1 : 0; }
// samples a finish hands out after H hops and a tail of r: L - max(0, S H - D)
constexpr long long owed(long long H, int r, int W, int S) {
  return H * S + r - (H * S - delay(W, S) > 0 ? H * S - delay(W, S) : 0);
}
// ... and where they start among the finish_max samples a finish computes (hops H - R - 3 .. H; those below hop 0 are skipped)
constexpr int finish_skip(long long H, int W, int S) { return H < delay_hops(W, S) ? (int)(delay_hops(W, S) - H) * S : 0; }

// The window's framing (what rced_framing_check refuses, with its words), then the overlap.  window_name is checked by the caller's
// rced_framing_check too; `reference_ok`: whether the window has no zero at its ends (hamming alone).
inline int check(int W, int S, int window_name, int rebuild, char* err, size_t err_len) {
  static const char* const names[4] = {"hamming", "hanning", "blackman", "bartlett"};
  if (W < 2 || W > kMaxWindow) {
    snprintf(err, err_len, "window must lie in [2, 256] samples (rfft(256) would crop a longer frame), got %d", W);
    return kPlanArg;
  }
  if (S < 1 || S > W) {
    snprintf(err, err_len, "stride must lie in [1, window = %d] samples, got %d", W, S);
    return kPlanArg;
  }
  if (window_name < 0 || window_name > 3) {
    snprintf(err, err_len, "window name must be RCED_WINDOW_HAMMING .. RCED_WINDOW_BARTLETT (0..3), got %d", window_name);
    return kPlanArg;
  }
  if (rebuild != kRebuildReference && rebuild != kRebuildOla) {
    snprintf(err, err_len, "rebuild must be RCED_STREAM_REBUILD_REFERENCE (0) or RCED_STREAM_REBUILD_OLA (1), got %d", rebuild);
    return kPlanArg;
  }
  if (rebuild == kRebuildReference && window_name != 0) {
    snprintf(err, err_len,
             "the reference rebuild divides every frame by its window, and the ends of a %s window are zero: the result is not "
             "finite (or off by 1e17); it is built for hamming only -- use the overlap-add rebuild",
             names[window_name]);
    return kPlanArg;
  }
  if (overlap(W, S) > kMaxOverlap) {
    snprintf(err, err_len,
             "a stream keeps ceil(window / stride) <= %d frames in flight: window %d at stride %d is an overlap of %d frames (delay and "
             "state grow with it); the offline entries serve it",
             kMaxOverlap, W, S, overlap(W, S));
    return kPlanArg;
  }
  return kPlanOk;
}

}  // namespace stream_fr
}  // namespace rced
