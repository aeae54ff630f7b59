// The arithmetic of csrc/stream_fr_plan.h as a program of its own (tests/test_stream_fr_host.py compiles it with the host compiler
// under AddressSanitizer and UBSan and runs it): a sweep over (W, S, L, K) of the delay, the frames complete and still to come, what a
// finish owes and where it finds it, the state's layout, and a lane walked push by push with the plan's index functions -- every frame
// that covers an output sample is in the pending sum or in the push, exactly once, and every index stays inside its array.
// Arguments: groups of (W, S, delay, finish_max) as the library reports them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fullycnnspeechenhancement_amd/csrc/stream_fr_plan.h"

namespace sf = rced::stream_fr;

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (failures < 20) {                    \
        printf("FAIL %s: ", #cond);           \
        printf(__VA_ARGS__);                  \
        printf("\n");                         \
      }                                       \
      ++failures;                             \
    }                                         \
  } while (0)

// frames t >= 0 (t < T where T >= 0) that cover sample i
static int covering(long long i, int W, int S, long long T) {
  int n = 0;
  if (i < 0) return 0;
  for (long long t = i / S; t >= 0 && t * S + W > i; --t)
    if (T < 0 || t < T) ++n;
  return n;
}

// One lane pushed in pushes of ks[0], ks[1], ... hops up to `hops` hops, then finished with a tail of r samples: the number of
// frames added into every output sample, through the pending sum, against the frames that cover it.
static void walk(int W, int S, const int* ks, int nk, int hops, int r) {
  const int R = sf::overlap(W, S), pl = sf::pend_len(W, S), tl = sf::tail_len(W, S);
  std::vector<int> pend(pl, 0), tail_from(tl, -1);   // addends pending; the sample index each tail slot holds
  long long H = 0, emitted = 0;
  int round = 0;
  auto run = [&](int K, long long T, long long fresh) {
    const long long hb = H - sf::delay_hops(W, S);
    // the front end: frame H - R + 1 + h reads samples (h - R + 1) S .. + W - 1 relative to the first new one
    for (int h = 0; h < K; ++h) {
      const long long t = H - R + 1 + h;
      if (t < 0 || (T >= 0 && t >= T)) continue;
      for (int k = 0; k < W; ++k) {
        const long long g = (long long)(h - R + 1) * S + k;
        if (g < 0) {
          CHECK(tl + g >= 0 && tl + g < tl, "tail index %lld of %d (W %d S %d)", tl + g, tl, W, S);
          if (tl + g >= 0 && tl + g < tl) CHECK(tail_from[tl + g] == H * S + g, "tail slot %lld holds %d, want %lld", tl + g, tail_from[tl + g], H * S + g);
        } else {
          CHECK(g < fresh || g < (long long)K * S + W, "sample %lld past the push", g);
        }
      }
    }
    // the back end: output j = sample hb S + j gathers slots q - m
    std::vector<int> num((size_t)K * S + pl, 0);
    for (int j = 0; j < K * S + pl; ++j) {
      const int q = j / S, rem = j - q * S, mmax = (W - 1 - rem) / S;
      int n = j < pl ? pend[j] : 0;
      for (int m = mmax; m >= 0; --m) {
        const long long p = q - m, t = hb + p;
        CHECK(rem + m * S >= 0 && rem + m * S < W, "frame sample %d of %d", rem + m * S, W);
        if (p >= 0 && p < K && t >= 0 && (T < 0 || t < T)) ++n;
        if (p < 0 && t >= 0) CHECK(j < pl, "a frame of an earlier push reaches sample %d, past the pending %d", j, pl);
      }
      num[j] = n;
    }
    for (int j = 0; j < K * S; ++j) {
      const long long i = hb * S + j;
      // during a push T is unknown: every frame that covers i and is complete with its 4 followers is there, and that is all of them
      CHECK(num[j] == covering(i, W, S, T), "sample %lld of W %d S %d after %lld hops: %d addends, %d frames cover it", i, W, S, H, num[j],
            covering(i, W, S, T));
    }
    emitted += (long long)K * S;
    for (int j = 0; j < pl; ++j) pend[j] = num[(size_t)K * S + j];
    for (int x = 0; x < tl; ++x) {
      const long long g = (long long)K * S - tl + x;
      tail_from[x] = g >= 0 ? (int)(H * S + g) : tail_from[x + K * S];
    }
    H += K;
  };
  while (H < hops) {
    int K = ks[round++ % nk];
    if (K > hops - H) K = (int)(hops - H);
    run(K, -1, (long long)K * S);
  }
  const long long L = H * S + r, T = sf::num_frames(L, W, S);
  const long long owed = sf::owed(H, r, W, S), before = emitted, Hf = H;
  const int skip = sf::finish_skip(H, W, S);
  CHECK(sf::complete(H, W, S) == (H - R + 1 > 0 ? H - R + 1 : 0), "complete");
  CHECK(L == 0 || (T - sf::complete(H, W, S) >= 0 && T - sf::complete(H, W, S) <= (L >= W ? 2 : R + 1)), "frames to come: T %lld after %lld hops", T, H);
  CHECK(L == 0 || (T - 1) * S + W >= L, "cut");
  CHECK(owed >= 0 && owed <= sf::delay(W, S) + S - 1 && owed <= sf::finish_max(W, S), "owed %lld", owed);
  CHECK(skip + owed <= (long long)sf::finish_slots(W, S) * S, "a finish computes %d samples, %d + %lld needed", sf::finish_slots(W, S) * S, skip, owed);
  // what the pushes handed out and what the finish owes make the utterance, delayed by D
  CHECK((before > sf::delay(W, S) ? before - sf::delay(W, S) : 0) + owed == L, "L %lld: %lld out, %lld owed", L, before, owed);
  run(sf::finish_slots(W, S), T, r);
  // the first owed sample is sample L - owed of the utterance
  CHECK((Hf - sf::delay_hops(W, S)) * S + skip == L - owed || owed == 0, "the owed samples start at %lld, want %lld", (Hf - sf::delay_hops(W, S)) * S + skip,
        L - owed);
}

int main(int argc, char** argv) {
  char err[512];
  int plans = 0;
  static_assert(sf::kStTail + sf::kMaxWindow <= sf::kStPend && sf::kStPend + sf::kMaxWindow <= sf::kStPhase &&
                    sf::kStPhase + 2 * sf::kKeep * sf::kBins <= sf::kStMag && sf::kStMag + sf::kKeep * sf::kBins <= sf::kStFloats,
                "the state's parts do not overlap");
  static_assert(sf::delay(256, 128) == 640 && sf::finish_max(256, 128) == 768 && sf::delay(160, 80) == 400, "the default framing's numbers");
  const int mixed[] = {1, 8, 2, 5, 3, 7}, one[] = {1}, all[] = {64};
  for (int W = 2; W <= 256; W += (W < 24 ? 1 : 13)) {
    for (int S = 1; S <= W; S += (S < 12 ? 1 : 7)) {
      const int rc = sf::check(W, S, 0, sf::kRebuildOla, err, sizeof err);
      const int R = sf::overlap(W, S);
      CHECK((rc == sf::kPlanOk) == (R <= sf::kMaxOverlap), "W %d S %d R %d: rc %d", W, S, R, rc);
      if (rc) {
        CHECK(strstr(err, "overlap of") != nullptr, "message: %s", err);
        continue;
      }
      ++plans;
      CHECK(sf::delay(W, S) == (R + 3) * S, "delay");
      CHECK(sf::tail_len(W, S) < W && sf::tail_len(W, S) >= W - S && sf::tail_len(W, S) <= sf::kMaxWindow, "tail %d", sf::tail_len(W, S));
      CHECK(sf::pend_len(W, S) >= 0 && sf::pend_len(W, S) < sf::kMaxWindow, "pend");
      CHECK(sf::finish_slots(W, S) <= sf::kMaxFinishSlots && sf::finish_max(W, S) >= sf::delay(W, S) + S - 1, "finish");
      const int lens[] = {1, S - 1, S, S + 1, W - 1, W, W + 1, sf::delay(W, S), sf::delay(W, S) + 1, 12 * S + W + 7, 3 * W + S};
      for (int L : lens) {
        if (L < 1) continue;
        walk(W, S, mixed, 6, L / S, L % S);
        walk(W, S, one, 1, L / S, L % S);
      }
      walk(W, S, all, 1, 130, S - 1);
    }
  }
  // the refusals' words
  CHECK(sf::check(257, 128, 0, 1, err, sizeof err) && strstr(err, "window must lie in [2, 256]"), "%s", err);
  CHECK(sf::check(100, 101, 0, 1, err, sizeof err) && strstr(err, "stride must lie in [1, window = 100]"), "%s", err);
  CHECK(sf::check(160, 80, 4, 1, err, sizeof err) && strstr(err, "window name"), "%s", err);
  CHECK(sf::check(160, 80, 0, 2, err, sizeof err) && strstr(err, "rebuild must be"), "%s", err);
  CHECK(sf::check(160, 80, 1, 0, err, sizeof err) && strstr(err, "hanning window are zero"), "%s", err);
  CHECK(sf::check(256, 16, 0, 1, err, sizeof err) && strstr(err, "overlap of 16 frames"), "%s", err);
  CHECK(sf::check(160, 80, 0, 0, err, sizeof err) == sf::kPlanOk && sf::check(256, 32, 3, 1, err, sizeof err) == sf::kPlanOk, "accepted");
  printf("%d framings swept, %d failures\n", plans, failures);
  int lib = 0;
  for (int a = 1; a + 3 < argc; a += 4, ++lib) {
    const int W = atoi(argv[a]), S = atoi(argv[a + 1]), d = atoi(argv[a + 2]), fm = atoi(argv[a + 3]);
    CHECK(d == sf::delay(W, S) && fm == sf::finish_max(W, S), "the library reports delay %d, finish_max %d for %d / %d", d, fm, W, S);
  }
  printf("%d framings of the library, %d failures\n", lib, failures);
  return failures ? 1 : 0;
}
