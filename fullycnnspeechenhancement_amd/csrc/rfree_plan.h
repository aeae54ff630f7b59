// The arithmetic of a free-running resampler lane (include/rced.h, "free-running resampler" section), apart from the
// device: how many outputs a lane has emitted after F frames, the history it keeps, the tiling of a push, the ring of finished outputs
// and the sizes of its buffers, from a ratio's table geometry.  Host only, no HIP: rstream_api.hip plans with it at create,
// tests/rfree_plan_check.cpp checks it as a program of its own.
#pragma once
#include <cstddef>
#include <cstdio>

#include "resample_plan.h"

namespace rced {
namespace rfree {

using resample::kMaxPush;
using resample::kMaxStateBytes;
using resample::kRun;
using resample::kSpanMax;
using resample::kTileMax;
using resample::span_bound;

constexpr int kHead = 2;   // 8-byte words in front of a lane's history: the frames taken, the ring's read position

struct Plan {
  int p = 1, q = 1, left = 0, width = 1, right = 0;
  int max_in = 1, max_take = 1, prefill = 0, out_bytes = 4;
  int hist = 0;        // source frames a lane keeps between pushes: width - 1
  int tile = 1;        // outputs per staging pass
  int push_max = 1;    // outputs one push adds to the ring, at most
  int flush_max = 1;   // outputs a finish computes, at most
  int cap = 1;         // the ring's capacity in samples: prefill + push_max + max_take
  int finish_max = 1;  // samples a finish can owe, at most: cap + flush_max
  int words = kHead;   // 8-byte words of state per lane: kHead, the history, the ring
};

enum { kPlanOk = 0, kPlanArg = 1 };

// Outputs a lane can have emitted after F frames: output m reaches frame floor(m q / p) + right at most, so m is ready when
// floor(m q / p) <= F - 1 - right, that is m < (F - right) p / q.  constexpr: the kernel computes it with this very function.
constexpr long long emitted(long long F, int p, int q, int right) {
  return F > right ? ((F - right) * p + q - 1) / q : 0;
}

// A(F + n) - A(F) <= ceil(n p / q) for every F (ceil(a + b) <= ceil(a) + ceil(b))
inline long long push_bound(long long n, int p, int q) { return (n * p + q - 1) / q; }

// what a finish with n last frames computes: the offline length, at most floor((F + n) p / q) + 1 with the rounding of its double
// product, less A(F) >= (F - right) p / q
inline long long flush_bound(long long n, int p, int q, int right) { return ((n + right) * p) / q + 1; }

// p / q in lowest terms with its table's `left` and `width`; out_bytes 2 or 4.  kPlanArg with a message in `err`.
inline int plan(int p, int q, int left, int width, int max_in, int max_take, int prefill, int out_bytes, int lanes, Plan* out, char* err,
                size_t err_len) {
  if (resample::not_a_table(p, q, left, width, err, err_len)) return kPlanArg;
  if (out_bytes != 2 && out_bytes != 4) {
    snprintf(err, err_len, "an output sample has 2 or 4 bytes, got %d", out_bytes);
    return kPlanArg;
  }
  if (max_in < 1 || max_in > kMaxPush || push_bound(max_in, p, q) > kMaxPush) {
    snprintf(err, err_len, "max_frames must be >= 1 and a push at most %lld frames and samples per lane, got %d", kMaxPush, max_in);
    return kPlanArg;
  }
  if (max_take < 1 || max_take > kMaxPush) {
    snprintf(err, err_len, "max_take must be 1..%lld samples, got %d", kMaxPush, max_take);
    return kPlanArg;
  }
  if (prefill < 0 || prefill > kMaxPush) {
    snprintf(err, err_len, "prefill must be 0..%lld samples, got %d", kMaxPush, prefill);
    return kPlanArg;
  }
  if (resample::bad_lanes(lanes, err, err_len) || resample::too_wide(p, q, width, err, err_len)) return kPlanArg;
  Plan P;
  P.p = p;
  P.q = q;
  P.left = left;
  P.width = width;
  P.right = width - 1 - left;
  P.max_in = max_in;
  P.max_take = max_take;
  P.prefill = prefill;
  P.out_bytes = out_bytes;
  P.hist = width - 1;
  const long long push_max = push_bound(max_in, p, q);
  const long long flush_max = flush_bound(max_in, p, q, P.right);
  const long long cap = (long long)prefill + push_max + max_take;
  const long long words = kHead + P.hist + (cap * out_bytes + 7) / 8;
  if (flush_max > kMaxPush || cap + flush_max > 4 * kMaxPush || (size_t)lanes * (size_t)words * 8 > kMaxStateBytes) {
    snprintf(err, err_len, "the ratio %d / %d needs %lld words of state per lane: too much for %d lanes", p, q, words, lanes);
    return kPlanArg;
  }
  P.tile = resample::tile_for(p, q, width);
  P.push_max = (int)push_max;
  P.flush_max = (int)flush_max;
  P.cap = (int)cap;
  P.finish_max = (int)(cap + flush_max);
  P.words = (int)words;
  *out = P;
  return kPlanOk;
}

}  // namespace rfree
}  // namespace rced
