// What the three resampling families (resample_api.hip, rstream_plan.h, rfree_plan.h) and their kernels (kernels_resample.h) share of
// the arithmetic of a ratio's tiling: the limits of a workgroup, the span of a tile, the tile of a ratio, and the refusals of a plan
// that every lane family makes in the same words.  Host only, no HIP: the two *_plan_check.cpp programs build it with a plain compiler.
#pragma once
#include <cstddef>
#include <cstdio>

namespace rced {
namespace resample {

constexpr int kK = 4;                  // same-phase outputs per lane and run
constexpr int kRun = 64 * kK;          // outputs of one phase a wave takes at a time
constexpr int kSpanMax = 6144;         // staged frames per workgroup: 48 KB of fp64
constexpr int kTileMax = 4096;         // outputs per workgroup and staging pass, at most
constexpr long long kMaxPush = 1 << 24;   // frames or outputs of one lane and push
constexpr size_t kMaxStateBytes = (size_t)1 << 32;

// the span of `tile` consecutive outputs is at most ((tile - 1) q) / p + 1 + width frames
constexpr long long span_bound(long long tile, int p, int q, int width) { return ((tile - 1) * q) / p + 1 + width; }

// outputs per workgroup: the largest tile whose span fits, a whole number of full runs (kRun outputs of every phase) where it holds one
inline int tile_for(int p, int q, int width) {
  long long t = ((long long)(kSpanMax - width - 1) * p) / q + 1;
  if (t > kTileMax) t = kTileMax;
  const long long run = (long long)kRun * p;
  if (t >= run) t -= t % run;
  return (int)t;
}

// The refusals of a lane plan, each true with its message in `err`; a plan makes them in its own order.
inline bool not_a_table(int p, int q, int left, int width, char* err, size_t err_len) {
  if (p >= 1 && q >= 1 && left >= 0 && width >= 1 && left < width) return false;
  snprintf(err, err_len, "not a phase table: p %d q %d left %d width %d", p, q, left, width);
  return true;
}
inline bool bad_lanes(int lanes, char* err, size_t err_len) {
  if (lanes >= 1 && lanes <= 65536) return false;
  snprintf(err, err_len, "lanes must be 1..65536, got %d", lanes);
  return true;
}
inline bool too_wide(int p, int q, int width, char* err, size_t err_len) {
  if (span_bound(1, p, q, width) <= kSpanMax) return false;
  snprintf(err, err_len, "the ratio %d / %d: one output reaches %d frames, more than a workgroup stages (%d)", p, q, width, kSpanMax);
  return true;
}

}  // namespace resample
}  // namespace rced
