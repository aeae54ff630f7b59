// Stand-alone check of the free-running resampler lanes' plan (csrc/rfree_plan.h): the outputs emitted after F frames, the history,
// the tiling, the ring and buffer sizes and the refusals, for the table geometries of the usual ratios and a sweep of others.  Built
// and run by test_rfree_host.py with the host compiler and AddressSanitizer and UBSan; exits non-zero if any property fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../fullycnnspeechenhancement_amd/csrc/rfree_plan.h"

using namespace rced::rfree;

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

// want_*: what the library reported for the same arguments, or -1
static void check_table(int sr_in, int sr_out, int p, int q, int left, int width, int max_in, int max_take, int prefill, int out_bytes,
                        int want_hist, int want_tile, int want_cap, int want_finish) {
  snprintf(g_ctx, sizeof g_ctx, "%d -> %d, %d in / %d out / %d prefill", sr_in, sr_out, max_in, max_take, prefill);
  Plan P;
  char err[256] = "";
  const int rc = plan(p, q, left, width, max_in, max_take, prefill, out_bytes, 4, &P, err, sizeof err);
  CHECK(rc == kPlanOk, "plan -> %d: %s", rc, err);
  if (rc != kPlanOk) return;
  ++g_plans;
  const int right = width - 1 - left;
  CHECK(P.right == right && P.hist == width - 1, "right %d history %d", P.right, P.hist);
  CHECK(P.cap == prefill + P.push_max + max_take && P.finish_max == P.cap + P.flush_max, "ring %d, finish row %d", P.cap, P.finish_max);
  CHECK(P.words == kHead + P.hist + (int)(((long long)P.cap * out_bytes + 7) / 8), "words %d", P.words);
  if (want_hist >= 0)
    CHECK(P.hist == want_hist && P.tile == want_tile && P.cap == want_cap && P.finish_max == want_finish,
          "the library reports history %d tile %d ring %d finish row %d, the plan %d %d %d %d", want_hist, want_tile, want_cap, want_finish,
          P.hist, P.tile, P.cap, P.finish_max);
  // A(F) one output at a time; the history an output not yet emitted reaches back; what a push of max_in and a finish add
  long long m = 0, back = 0;
  const long long top = right + 900;
  bool closed = true, pushes = true, finishes = true;
  for (long long F = 0; F <= top; ++F) {
    while ((m * q) / p + right <= F - 1) ++m;
    if (emitted(F, p, q, right) != m) closed = false;
    const long long b = F - ((m * q) / p - left);
    if (b > back) back = b;
    if (emitted(F + max_in, p, q, right) - m > P.push_max) pushes = false;
    for (int c = 0; c <= max_in; c += (max_in > 16 ? max_in / 16 : 1)) {
      const long long M = (long long)((double)(F + c) * ((double)sr_out / sr_in));
      if (M - m > P.flush_max || (M < m && right > 0)) finishes = false;
    }
  }
  CHECK(closed, "A(F) is not the count of outputs whose last tap has arrived");
  CHECK(back == P.hist || (width == 1 && back <= 0), "outputs reach %lld frames back, the history holds %d", back, P.hist);
  CHECK(pushes, "a push of %d frames adds more than %d outputs", max_in, P.push_max);
  CHECK(finishes, "a finish computes more than %d outputs, or fewer than none", P.flush_max);
  // a staging pass fits a workgroup's span
  CHECK(P.tile >= 1 && P.tile <= kTileMax && span_bound(P.tile, p, q, width) <= kSpanMax, "tile %d spans %lld frames", P.tile,
        span_bound(P.tile, p, q, width));
  for (long long m0 = 0; m0 < 3LL * P.tile; m0 += 7) {
    const long long span = ((m0 + P.tile - 1) * q) / p - (m0 * q) / p + width;
    CHECK(span <= kSpanMax, "outputs %lld .. + %d span %lld frames", m0, P.tile, span);
  }
  printf("%-44s p %3d q %3d left %4d width %4d  history %4d  tile %4d  push %5d  ring %5d  finish row %5d\n", g_ctx, p, q, left, width,
         P.hist, P.tile, P.push_max, P.cap, P.finish_max);
}

static void check_plan(int sr_in, int sr_out, int max_in, int max_take, int prefill, int out_bytes) {
  int p, q, left, width;
  geometry(sr_in, sr_out, &p, &q, &left, &width);
  check_table(sr_in, sr_out, p, q, left, width, max_in, max_take, prefill, out_bytes, -1, -1, -1, -1);
}

static void check_refusal(const char* what, int p, int q, int left, int width, int max_in, int max_take, int prefill, int out_bytes, int lanes,
                          const char* needle) {
  snprintf(g_ctx, sizeof g_ctx, "refusal: %s", what);
  Plan P;
  char err[256] = "";
  const int rc = plan(p, q, left, width, max_in, max_take, prefill, out_bytes, lanes, &P, err, sizeof err);
  CHECK(rc == kPlanArg, "plan -> %d", rc);
  CHECK(strstr(err, needle) != nullptr, "message '%s' lacks '%s'", err, needle);
}

// With arguments "sr_in sr_out p q left width max_frames max_take prefill history tile capacity finish_max" (any number of such
// groups; float32 out): the same checks on the geometry and the sizes the library reports, which must also be this file's own.
int main(int argc, char** argv) {
  for (int a = 1; a + 13 <= argc; a += 13) {
    int v[13];
    for (int i = 0; i < 13; ++i) v[i] = atoi(argv[a + i]);
    int p, q, left, width;
    geometry(v[0], v[1], &p, &q, &left, &width);
    snprintf(g_ctx, sizeof g_ctx, "%d -> %d, the library's table", v[0], v[1]);
    CHECK(p == v[2] && q == v[3] && left == v[4] && width == v[5], "library p %d q %d left %d width %d, here %d %d %d %d", v[2], v[3], v[4], v[5],
          p, q, left, width);
    check_table(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], 4, v[9], v[10], v[11], v[12]);
  }
  check_plan(44100, 8000, 441, 128, 0, 4);
  check_plan(8000, 44100, 128, 441, 1323, 4);
  check_plan(48000, 8000, 480, 128, 0, 4);
  check_plan(8000, 48000, 128, 480, 1440, 4);
  check_plan(16000, 8000, 256, 128, 0, 2);
  check_plan(8000, 16000, 128, 256, 384, 2);
  check_plan(22050, 8000, 1024, 512, 0, 4);
  check_plan(8000, 8000, 100, 128, 0, 4);
  check_plan(8000, 8000, 128, 100, 124, 4);
  check_plan(44100, 8000, 40000, 8000, 0, 4);    // a push of several staging passes
  check_plan(8000, 44100, 1, 1, 0, 2);           // the smallest push and take
  check_plan(96000, 8000, 7, 3, 5, 4);
  check_plan(8000, 10000, 4, 5, 8, 2);
  check_plan(192000, 8000, 3072, 128, 0, 4);
  check_refusal("max_frames", 1, 2, 127, 255, 0, 128, 0, 4, 4, "max_frames");
  check_refusal("push too long", 1, 2, 127, 255, 1 << 25, 128, 0, 4, 4, "max_frames");
  check_refusal("max_take", 1, 2, 127, 255, 256, 0, 0, 4, 4, "max_take");
  check_refusal("prefill", 1, 2, 127, 255, 256, 128, -1, 4, 4, "prefill");
  check_refusal("sample size", 1, 2, 127, 255, 256, 128, 0, 3, 4, "2 or 4 bytes");
  check_refusal("lanes", 1, 2, 127, 255, 256, 128, 0, 4, 0, "lanes");
  check_refusal("lanes", 1, 2, 127, 255, 256, 128, 0, 4, 65537, "lanes");
  check_refusal("state", 1, 2, 127, 255, 1 << 24, 1 << 24, 1 << 24, 4, 65536, "too much");
  check_refusal("span", 1, 48, 3072, 6145, 48, 1, 0, 4, 4, "one output reaches 6145 frames");
  check_refusal("table", 1, 2, 255, 255, 256, 128, 0, 4, 4, "not a phase table");
  printf("%d plans, %d failures\n", g_plans, g_fail);
  return g_fail ? 1 : 0;
}
