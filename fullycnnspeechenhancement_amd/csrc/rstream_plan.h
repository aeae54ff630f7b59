// The arithmetic of a resampler lane stream (include/rced.h, "streaming resampler" section), apart from the device:
// the delay, the history a lane keeps, the tiling of a push and the sizes of its buffers, from a ratio's table geometry.
// Host only, no HIP: rstream_api.hip plans with it at create, tests/rstream_plan_check.cpp checks it as a program of its own.
#pragma once
#include <cstddef>
#include <cstdio>

#include "resample_plan.h"

namespace rced {
namespace rstream {

using resample::kMaxPush;
using resample::kMaxStateBytes;
using resample::kRun;
using resample::kSpanMax;
using resample::kTileMax;
using resample::span_bound;

struct Plan {
  int p = 1, q = 1, left = 0, width = 1, right = 0;
  int unit_in = 1, unit_out = 1, max_units = 1;
  int delay = 0;      // D: outputs the stream lags the offline result by
  int hist = 0;       // source frames a lane keeps between pushes
  int tile = 1;       // outputs per staging pass
  int finish_max = 1; // outputs a finish can owe, at most: unit_out + delay
  int words = 1;      // 8-byte words of state per lane: the units pushed, then the history
};

enum { kPlanOk = 0, kPlanArg = 1 };

// The smallest D for which every output a push emits reaches only frames already pushed.  Output m of the offline result
// reaches frame floor(m q / p) + right at most; a push that brings the lane to H units emits up to m = H unit_out - 1 - D and
// holds H unit_in = H unit_out q / p frames: ceil((D + 1) q / p) >= right + 1, that is D = floor(right p / q).
inline long long min_delay(int p, int q, int right) { return ((long long)right * p) / q; }

// the first frame a push reaches lies ceil(D q / p) + left before the push's own first frame
inline long long history(int p, int q, int left, long long delay) { return (delay * q + p - 1) / p + left; }

// p / q in lowest terms with its table's `left` and `width`; delay < 0: the smallest, else that many samples (the denoiser's down
// lanes run a whole hop behind).  kPlanArg with a message in `err`.
inline int plan(int p, int q, int left, int width, int unit_in, int unit_out, int max_units, int lanes, int delay, Plan* out, char* err,
                size_t err_len) {
  if (resample::not_a_table(p, q, left, width, err, err_len)) return kPlanArg;
  if (unit_in < 1 || unit_out < 1 || (long long)unit_in * p != (long long)unit_out * q) {
    snprintf(err, err_len, "units of %d frames in and %d samples out do not stand in the ratio %d / %d (unit_in * %d must equal unit_out * %d)",
             unit_in, unit_out, p, q, p, q);
    return kPlanArg;
  }
  if (max_units < 1 || (long long)max_units * unit_in > kMaxPush || (long long)max_units * unit_out > kMaxPush) {
    snprintf(err, err_len, "max_units must be >= 1 and a push at most %lld frames and samples per lane, got %d units of %d / %d", kMaxPush,
             max_units, unit_in, unit_out);
    return kPlanArg;
  }
  if (resample::bad_lanes(lanes, err, err_len)) return kPlanArg;
  Plan P;
  P.p = p;
  P.q = q;
  P.left = left;
  P.width = width;
  P.right = width - 1 - left;
  P.unit_in = unit_in;
  P.unit_out = unit_out;
  P.max_units = max_units;
  const long long dmin = min_delay(p, q, P.right);
  if (delay >= 0 && delay < dmin) {
    snprintf(err, err_len, "a delay of %d samples is less than the ratio %d / %d needs (%lld)", delay, p, q, dmin);
    return kPlanArg;
  }
  const long long d = delay < 0 ? dmin : delay;
  const long long hist = history(p, q, left, d);
  if (resample::too_wide(p, q, width, err, err_len)) return kPlanArg;
  if (d > kMaxPush || hist > kMaxPush || (size_t)lanes * (size_t)(1 + hist) * 8 > kMaxStateBytes) {
    snprintf(err, err_len, "the ratio %d / %d needs %lld frames of history per lane: too much for %d lanes", p, q, hist, lanes);
    return kPlanArg;
  }
  P.delay = (int)d;
  P.hist = (int)hist;
  P.tile = resample::tile_for(p, q, width);
  P.finish_max = unit_out + (int)d;
  P.words = 1 + (int)hist;
  *out = P;
  return kPlanOk;
}

}  // namespace rstream
}  // namespace rced
