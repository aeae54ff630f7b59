// C ABI of the sample-rate conversion (include/rced.h, "resample" section): the phase table of a ratio, built on the host in
// float64 from the definition in DESIGN.md 3.4f, and the launch of kernels_resample.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/rced.h"
#include "host_util.h"
#include "kernels_resample.h"
#include "rced_internal.h"

using namespace rced;

namespace {

constexpr double kZero = 64.0;                     // zero crossings on either side
constexpr double kRolloff = 0.9475937167399596;
constexpr double kBeta = 14.769656459379492;
constexpr size_t kMaxTableBytes = 1u << 20;

struct Ratio {   // one per p / q, built once per process
  int p = 1, q = 1, left = 0, width = 1;
  std::vector<double> table;                       // [p][width]
  double* dev[kMaxDevices] = {};                   // uploaded once per device
};
std::map<std::pair<int, int>, std::unique_ptr<Ratio>> g_ratios;
std::mutex g_mu;

int gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

double bessel_i0(double x) {   // sum_k ((x / 2)^k / k!)^2: positive terms, converged to double precision
  const double y = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= y / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// h(tau) = rho sinc(rho tau) I0(beta sqrt(1 - (tau / Z)^2)) / I0(beta) for |tau| < Z (strictly), 0 elsewhere; sinc is numpy's
double kernel_h(double tau, double i0_beta) {
  if (!(std::fabs(tau) < kZero)) return 0.0;
  const double x = kRolloff * tau;
  const double y = M_PI * (x == 0.0 ? 1.0e-20 : x);
  const double u = tau / kZero;
  return kRolloff * (std::sin(y) / y) * bessel_i0(kBeta * std::sqrt(1.0 - u * u)) / i0_beta;
}

double tau_of(double s, long long d, int r, int p) { return s * ((double)d - (double)r / (double)p); }

// The table of sr_new / sr_orig (both > 0): found or built.  RCED_ERR_ARG where it would exceed kMaxTableBytes.
int ratio_for(int sr_orig, int sr_new, Ratio** out) {
  const int g = gcd(sr_new, sr_orig);
  const int p = sr_new / g, q = sr_orig / g;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_ratios.find({p, q});
  if (it != g_ratios.end()) {
    *out = it->second.get();
    return RCED_OK;
  }
  std::unique_ptr<Ratio> R(new Ratio);
  R->p = p;
  R->q = q;
  if (p == 1 && q == 1) {   // the same rate: the downmixing copy
    R->table.assign(1, 1.0);
  } else {
    const double ratio = (double)sr_new / (double)sr_orig, s = ratio < 1.0 ? ratio : 1.0;
    // columns d = -left .. right around n0: every d some phase reaches (phase 0 reaches furthest back, phase p - 1 furthest on)
    const long long reach = (long long)std::ceil(kZero / s) + 1;
    long long left = 0, right = 0;
    for (long long d = reach; d >= 1; --d)
      if (std::fabs(tau_of(s, -d, 0, p)) < kZero) {
        left = d;
        break;
      }
    for (long long d = reach; d >= 1; --d)
      if (std::fabs(tau_of(s, d, p - 1, p)) < kZero) {
        right = d;
        break;
      }
    if ((unsigned long long)p * (left + 1 + right) * sizeof(double) > kMaxTableBytes)
      return rced_fail(RCED_ERR_ARG, "resampling %d Hz -> %d Hz (%d / %d) needs a phase table of %llu bytes, more than 1 MiB: not built",
                       sr_orig, sr_new, p, q, (unsigned long long)p * (left + 1 + right) * sizeof(double));
    R->left = (int)left;
    R->width = (int)(left + 1 + right);
    if (resample::span_bound(1, p, q, R->width) > resample::kSpanMax)
      return rced_fail(RCED_ERR_ARG, "resampling %d Hz -> %d Hz (%d / %d): one output reaches %d frames, more than a workgroup stages (%d)",
                       sr_orig, sr_new, p, q, R->width, resample::kSpanMax);
    const double i0_beta = bessel_i0(kBeta);
    R->table.resize((size_t)p * R->width);
    for (int r = 0; r < p; ++r)
      for (int c = 0; c < R->width; ++c) R->table[(size_t)r * R->width + c] = s * kernel_h(tau_of(s, c - R->left, r, p), i0_beta);
  }
  *out = R.get();
  g_ratios[{p, q}] = std::move(R);
  return RCED_OK;
}

int device_table(Ratio* R, int device, const double** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!R->dev[device])
    if (int rc = upload(&R->dev[device], R->table, "resampling table")) return rc;
  *out = R->dev[device];
  return RCED_OK;
}

}  // namespace

int rced_resample_table(int sr_orig, int sr_new, int* p, int* q, int* left, int* width, int device, const double** table_dev) {
  Ratio* R = nullptr;
  if (int rc = ratio_for(sr_orig, sr_new, &R)) return rc;
  *p = R->p;
  *q = R->q;
  *left = R->left;
  *width = R->width;
  return table_dev ? device_table(R, device, table_dev) : RCED_OK;
}

extern "C" {

long long rced_resample_length(long long n, int sr_orig, int sr_new) {
  if (n < 0 || sr_orig <= 0 || sr_new <= 0) return -1;
  return (long long)((double)n * ((double)sr_new / (double)sr_orig));
}

int rced_resample_taps(int sr_orig, int sr_new, int* p, int* q, int* left, int* width, double* table_host, size_t n_doubles) {
  if (int rc = check_rates(sr_orig, sr_new)) return rc;
  Ratio* R = nullptr;
  if (int rc = ratio_for(sr_orig, sr_new, &R)) return rc;
  if (p) *p = R->p;
  if (q) *q = R->q;
  if (left) *left = R->left;
  if (width) *width = R->width;
  if (table_host) {
    if (n_doubles < R->table.size())
      return rced_fail(RCED_ERR_ARG, "the table of %d -> %d holds %zu doubles, the buffer %zu", sr_orig, sr_new, R->table.size(), n_doubles);
    memcpy(table_host, R->table.data(), R->table.size() * sizeof(double));
  }
  return RCED_OK;
}

int rced_resample(const void* src_dev, int src_dtype, int channels, long long src_frames, const long long* begin_dev, const int* count_dev,
                  int N, int sr_orig, int sr_new, void* out_dev, int out_dtype, const long long* out_begin_dev, int row_stride, int L,
                  int device, void* stream) {
  if (N < 0 || L < 0 || src_frames < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (int rc = check_channels(channels)) return rc;
  if (int rc = check_rates(sr_orig, sr_new)) return rc;
  if (int rc = check_pcm_dtypes(src_dtype, out_dtype)) return rc;
  if (!out_begin_dev && row_stride < L) return rced_fail(RCED_ERR_ARG, "row_stride %d < L %d", row_stride, L);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (L > resample::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  Ratio* R = nullptr;
  if (int rc = ratio_for(sr_orig, sr_new, &R)) return rc;
  if (N == 0 || L == 0) return RCED_OK;
  if (!begin_dev || !count_dev || !out_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (!src_dev && src_frames > 0) return rced_fail(RCED_ERR_ARG, "null source of %lld frames", src_frames);
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  resample::Params P;
  if (int rc = device_table(R, device, &P.table)) return rc;
  P.src = src_dev;
  P.src_frames = src_frames;
  P.channels = channels;
  P.begin = begin_dev;
  P.count = count_dev;
  P.p = R->p;
  P.q = R->q;
  P.left = R->left;
  P.width = R->width;
  P.ratio = (double)sr_new / (double)sr_orig;
  P.tile = resample::tile_for(R->p, R->q, R->width);
  P.out = out_dev;
  P.out_begin = out_begin_dev;
  P.row_stride = row_stride;
  P.L = L;
  const dim3 grid((L + P.tile - 1) / P.tile, N), block(resample::kThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_pcm_types(src_dtype, out_dtype, [&](auto sf, auto of) -> int {
    LAUNCH((resample::resample_kernel<decltype(sf)::value, decltype(of)::value>), grid, block, 0, st, P);
    return RCED_OK;
  });
}

}  // extern "C"
