// Stand-alone check of the workspace carve (csrc/host_carve.h, the offset arithmetic behind host_ws.h's Carve::bind): takes of mixed
// element types and counts get 256-byte aligned parts in call order that are long enough and do not overlap, and the carve of
// rced_wave_loss_run puts its six parts where the hand-written carve it replaced put them.  No device, no HIP runtime: bind() is never
// called.  Built and run by test_host_ws_host.py with the host compiler under AddressSanitizer and UBSan; exits non-zero on a failure.
#include <cstdio>
#include <cstdlib>

#include "../fullycnnspeechenhancement_amd/csrc/host_carve.h"

static int checks = 0, failures = 0;

static void check(bool ok, const char* what, size_t got, size_t want) {
  ++checks;
  if (ok) return;
  ++failures;
  std::printf("FAILED %s: got %zu, want %zu\n", what, got, want);
}

static size_t round256(size_t v) { return (v + 255) / 256 * 256; }   // align256, restated

// the properties of any carve: `need[k]` = count * sizeof(T) of take k, `ptr[k]` = the pointer variable it booked
static void check_parts(const Carve& c, int n, const size_t* need, void* const* ptr, const char* name) {
  check(c.n == n, "number of parts", (size_t)c.n, (size_t)n);
  size_t end = 0;
  for (int k = 0; k < n; ++k) {
    check(c.slot[k] == ptr[k], "slot is the pointer of take k, in call order", (size_t)k, (size_t)k);
    check(c.at[k] % 256 == 0, "offset is a multiple of 256", c.at[k] % 256, 0);
    check(c.at[k] >= end, "part starts at or past the end of the one before", c.at[k], end);
    check(c.at[k] == round256(end), "part starts at the next 256-byte boundary", c.at[k], round256(end));
    const size_t next = k + 1 < n ? c.at[k + 1] : c.bytes;
    check(next - c.at[k] >= need[k], "part is at least count * sizeof(T) long", next - c.at[k], need[k]);
    end = c.at[k] + need[k];
    std::printf("%s part %d: at %zu, %zu bytes asked\n", name, k, c.at[k], need[k]);
  }
  check(c.bytes == round256(end), "bytes is the end of the last part", c.bytes, round256(end));
  check(c.bytes % 256 == 0, "bytes is a multiple of 256", c.bytes % 256, 0);
}

static void mixed_takes() {
  float *f1, *f64, *f65;
  double *d33, *d0;
  int *i0, *i7, *i64;
  Carve c;
  c.take(&f1, 1);
  c.take(&d33, 33);    // 264 bytes: two blocks
  c.take(&i0, 0);      // nothing: the next part starts where this one does
  c.take(&f64, 64);    // 256 bytes exactly
  c.take(&i7, 7);
  c.take(&d0, 0);
  c.take(&f65, 65);    // one element past a block
  c.take(&i64, 64);    // 256 bytes exactly, last
  const size_t need[8] = {4, 264, 0, 256, 28, 0, 260, 256};
  void* const ptr[8] = {&f1, &d33, &i0, &f64, &i7, &d0, &f65, &i64};
  check_parts(c, 8, need, ptr, "mixed");
  const size_t at[8] = {0, 256, 768, 768, 1024, 1280, 1280, 1792};
  for (int k = 0; k < 8; ++k) check(c.at[k] == at[k], "offset of the mixed takes, worked out by hand", c.at[k], at[k]);
  check(c.bytes == 2048, "bytes of the mixed takes", c.bytes, 2048);
  Carve none;
  check(none.n == 0 && none.bytes == 0, "an empty carve asks for nothing", none.bytes, 0);
}

// rced_wave_loss_run's carve against the hand-written one it replaced (restated): y, u, ws1, ws2, scal, frames
static void wave_loss(int N, int L, int slices) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t sig = up((size_t)N * L * sizeof(float)), part = up((size_t)N * slices * 2 * sizeof(double));
  const size_t scal = up((size_t)N * 4 * sizeof(double)), fr = up((size_t)N * sizeof(int));
  const size_t hand[6] = {0, sig, 2 * sig, 2 * sig + part, 2 * sig + 2 * part, 2 * sig + 2 * part + scal};
  const size_t hand_bytes = 2 * sig + 2 * part + scal + fr;
  float *y, *u;
  double *ws1, *ws2, *sc;
  int* frames;
  Carve c;
  c.take(&y, (size_t)N * L);
  c.take(&u, (size_t)N * L);
  c.take(&ws1, (size_t)N * slices * 2);
  c.take(&ws2, (size_t)N * slices * 2);
  c.take(&sc, (size_t)N * 4);
  c.take(&frames, (size_t)N);
  const size_t need[6] = {(size_t)N * L * 4, (size_t)N * L * 4, (size_t)N * slices * 16, (size_t)N * slices * 16, (size_t)N * 32, (size_t)N * 4};
  void* const ptr[6] = {&y, &u, &ws1, &ws2, &sc, &frames};
  char name[64];
  std::snprintf(name, sizeof name, "wave loss (N %d, L %d, slices %d)", N, L, slices);
  check_parts(c, 6, need, ptr, name);
  for (int k = 0; k < 6; ++k) check(c.at[k] == hand[k], "offset equals the hand carve's", c.at[k], hand[k]);
  check(c.bytes == hand_bytes, "bytes equals the hand carve's", c.bytes, hand_bytes);
}

int main() {
  mixed_takes();
  wave_loss(1, 256, 1);
  wave_loss(3, 1280, 2);
  wave_loss(2, 128, 1);
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
