// Stand-alone check of the resampler lanes' plan (csrc/rstream_plan.h): delay, history, tiling, buffer sizes and refusals, for the
// table geometries of the usual ratios and a sweep of others.  Built and run by test_rstream_host.py with the host compiler and
// AddressSanitizer and UBSan; exits non-zero if any property fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../fullycnnspeechenhancement_amd/csrc/rstream_plan.h"

using namespace rced::rstream;

static int g_fail = 0, g_plans = 0;
static char g_ctx[96];
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++g_fail;                                           \
      printf("FAIL %s: %s -- ", g_ctx, #cond);            \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
    }                                                     \
  } while (0)

static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

// the columns of a ratio's phase table as DESIGN.md 3.4f defines them: |s (d - r / p)| < 64, phase 0 furthest back, p - 1 furthest on
static void geometry(int sr_in, int sr_out, int* p, int* q, int* left, int* width) {
  const int g = gcd(sr_in, sr_out);
  *p = sr_out / g;
  *q = sr_in / g;
  if (*p == 1 && *q == 1) {
    *left = 0;
    *width = 1;
    return;
  }
  const double ratio = (double)sr_out / sr_in, s = ratio < 1.0 ? ratio : 1.0;
  long long l = 0, r = 0;
  for (long long d = (long long)std::ceil(64.0 / s) + 1; d >= 1; --d)
    if (std::fabs(s * (double)-d) < 64.0) { l = d; break; }
  for (long long d = (long long)std::ceil(64.0 / s) + 1; d >= 1; --d)
    if (std::fabs(s * ((double)d - (double)(*p - 1) / *p)) < 64.0) { r = d; break; }
  *left = (int)l;
  *width = (int)(l + 1 + r);
}

static long long last_frame(const Plan& P, long long m) { return (m * P.q) / P.p - P.left + P.width - 1; }
static long long first_frame(const Plan& P, long long m) { return (m * P.q) / P.p - P.left; }

static void check_table(int sr_in, int sr_out, int p, int q, int left, int width, int unit_in, int unit_out, int max_units, int want_delay);

static void check_plan(int sr_in, int sr_out, int unit_in, int unit_out, int max_units, int want_delay) {
  int p, q, left, width;
  geometry(sr_in, sr_out, &p, &q, &left, &width);
  check_table(sr_in, sr_out, p, q, left, width, unit_in, unit_out, max_units, want_delay);
}

static void check_table(int sr_in, int sr_out, int p, int q, int left, int width, int unit_in, int unit_out, int max_units, int want_delay) {
  snprintf(g_ctx, sizeof g_ctx, "%d -> %d, units %d / %d", sr_in, sr_out, unit_in, unit_out);
  Plan P;
  char err[256] = "";
  const int rc = plan(p, q, left, width, unit_in, unit_out, max_units, 4, -1, &P, err, sizeof err);
  CHECK(rc == kPlanOk, "plan -> %d: %s", rc, err);
  if (rc != kPlanOk) return;
  ++g_plans;
  if (want_delay >= 0) CHECK(P.delay == want_delay, "delay %d, expected %d", P.delay, want_delay);
  CHECK(P.right == width - 1 - left && P.words == 1 + P.hist && P.finish_max == unit_out + P.delay, "sizes");
  // by brute force over pushes of one unit: D serves every push, D - 1 does not; the history covers the furthest reach back
  bool ok = true, less_ok = P.delay > 0;
  long long back = 0;
  for (long long H = 1; H <= 64; ++H) {
    const long long frames = H * unit_in;
    for (long long m = (H - 1) * unit_out - P.delay; m < H * unit_out - P.delay; ++m) {
      if (m < 0) continue;
      if (last_frame(P, m) > frames - 1) ok = false;
      const long long b = (H - 1) * unit_in - first_frame(P, m);
      if (b > back) back = b;
    }
    const long long m = H * unit_out - P.delay;   // the output a delay of D - 1 would emit as well
    if (m >= 0 && last_frame(P, m) > frames - 1) less_ok = false;
  }
  CHECK(ok, "an output of a push reaches a frame not pushed yet at delay %d", P.delay);
  CHECK(!less_ok, "delay %d is not minimal", P.delay);
  CHECK(back <= P.hist, "a push reaches %lld frames back, the history holds %d", back, P.hist);
  CHECK(back == P.hist || P.delay == 0, "the history holds %d frames, %lld are reached", P.hist, back);
  // a staging pass fits a workgroup's span, and one more output would not (or the tile is capped)
  CHECK(P.tile >= 1 && P.tile <= kTileMax && span_bound(P.tile, p, q, width) <= kSpanMax, "tile %d spans %lld frames", P.tile,
        span_bound(P.tile, p, q, width));
  for (long long m0 = 0; m0 < 3LL * P.tile; m0 += 7) {
    const long long span = ((m0 + P.tile - 1) * q) / p - (m0 * q) / p + width;
    CHECK(span <= kSpanMax, "outputs %lld .. + %d span %lld frames", m0, P.tile, span);
  }
  // what a finish owes fits its row: M - max(0, H unit_out - D) with M <= the outputs of H units and a tail short of a unit
  for (long long H = 0; H <= 8; ++H)
    for (int c = 0; c < unit_in; c += (unit_in > 16 ? unit_in / 16 : 1)) {
      const long long M = (long long)((double)(H * unit_in + c) * ((double)sr_out / sr_in));
      const long long lo = H * unit_out - P.delay > 0 ? H * unit_out - P.delay : 0;
      CHECK(M - lo <= P.finish_max && M - lo >= 0, "H %lld tail %d: %lld owed, the row holds %d", H, c, M - lo, P.finish_max);
    }
  printf("%-22s p %3d q %3d left %4d width %4d  D %4d  history %5d  tile %4d  finish row %4d\n", g_ctx, p, q, left, width, P.delay, P.hist,
         P.tile, P.finish_max);
}

static void check_refusal(const char* what, int p, int q, int left, int width, int unit_in, int unit_out, int max_units, int lanes,
                          const char* needle) {
  snprintf(g_ctx, sizeof g_ctx, "refusal: %s", what);
  Plan P;
  char err[256] = "";
  const int rc = plan(p, q, left, width, unit_in, unit_out, max_units, lanes, -1, &P, err, sizeof err);
  CHECK(rc == kPlanArg, "plan -> %d", rc);
  CHECK(strstr(err, needle) != nullptr, "message '%s' lacks '%s'", err, needle);
}

// With arguments "sr_in sr_out p q left width unit_in unit_out" (any number of such groups): the same checks on the geometry the
// library's rced_resample_taps reports, which must also be this file's own.
int main(int argc, char** argv) {
  for (int a = 1; a + 8 <= argc; a += 8) {
    int v[8];
    for (int i = 0; i < 8; ++i) v[i] = atoi(argv[a + i]);
    int p, q, left, width;
    geometry(v[0], v[1], &p, &q, &left, &width);
    snprintf(g_ctx, sizeof g_ctx, "%d -> %d, the library's table", v[0], v[1]);
    CHECK(p == v[2] && q == v[3] && left == v[4] && width == v[5], "library p %d q %d left %d width %d, here %d %d %d %d", v[2], v[3], v[4], v[5],
          p, q, left, width);
    check_table(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], 8, -1);
  }
  check_plan(16000, 8000, 256, 128, 8, 63);
  check_plan(48000, 8000, 768, 128, 8, 63);
  check_plan(12000, 8000, 192, 128, 8, -1);
  check_plan(8000, 16000, 128, 256, 8, 128);
  check_plan(8000, 48000, 128, 768, 8, 384);
  check_plan(8000, 12000, 128, 192, 8, -1);
  check_plan(44100, 8000, 441, 80, 8, -1);
  check_plan(8000, 44100, 80, 441, 8, -1);
  check_plan(8000, 8000, 128, 128, 8, 0);
  check_plan(8000, 8000, 1, 1, 64, 0);
  check_plan(16000, 8000, 2, 1, 4096, 63);        // the smallest units, long pushes
  check_plan(32000, 8000, 512, 128, 8, -1);
  check_plan(96000, 8000, 12, 1, 8, -1);
  check_plan(8000, 10000, 4, 5, 8, -1);
  check_plan(22050, 8000, 441, 160, 2, -1);
  check_plan(8000, 22050, 160, 441, 2, -1);
  check_plan(192000, 8000, 3072, 128, 2, -1);
  check_refusal("units", 1, 2, 127, 255, 256, 127, 8, 4, "do not stand in the ratio 1 / 2");
  check_refusal("unit 0", 1, 2, 127, 255, 0, 0, 8, 4, "do not stand in the ratio");
  check_refusal("max_units", 1, 2, 127, 255, 256, 128, 0, 4, "max_units");
  check_refusal("push too long", 1, 2, 127, 255, 1 << 22, 1 << 21, 8, 4, "max_units");
  check_refusal("lanes", 1, 2, 127, 255, 256, 128, 8, 0, "lanes");
  check_refusal("lanes", 1, 2, 127, 255, 256, 128, 8, 65537, "lanes");
  check_refusal("span", 1, 48, 3072, 6145, 48, 1, 8, 4, "one output reaches 6145 frames");
  check_refusal("table", 1, 2, 255, 255, 256, 128, 8, 4, "not a phase table");
  {   // a delay of the caller's: a whole hop for the denoiser's down lanes; less than the ratio needs is refused
    snprintf(g_ctx, sizeof g_ctx, "48000 -> 8000 at a delay of 128");
    Plan P;
    char err[256] = "";
    CHECK(plan(1, 6, 383, 767, 768, 128, 8, 4, 128, &P, err, sizeof err) == kPlanOk, "%s", err);
    CHECK(P.delay == 128 && P.hist == 128 * 6 + 383 && P.finish_max == 256 && P.words == 1 + P.hist, "delay %d history %d", P.delay, P.hist);
    CHECK(plan(1, 6, 383, 767, 768, 128, 8, 4, 62, &P, err, sizeof err) == kPlanArg && strstr(err, "less than"), "%s", err);
  }
  printf("%d plans, %d failures\n", g_plans, g_fail);
  return g_fail ? 1 : 0;
}
