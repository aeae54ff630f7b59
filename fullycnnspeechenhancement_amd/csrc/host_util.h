// Host-side helpers every translation unit of the library shares: error return, device selection, vector upload, and the bf16
// roundings behind every packed three-part A-fragment stream.  Host only: no device code, no kernel header.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rced.h"

int rced_fail(int code, const char* fmt, ...);   // rced_api.hip: sets the thread's error text, returns `code`

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return rced_fail(e_ == hipErrorOutOfMemory ? RCED_ERR_ALLOC : RCED_ERR_HIP, "%s: %s", #expr, \
                       hipGetErrorString(e_));                                                 \
  } while (0)

// A launch on `st`, then the error it may have left: the pair every entry is made of
#define LAUNCH(kernel, grid, block, lds, st, ...)                  \
  do {                                                             \
    hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__); \
    HIP_TRY(hipGetLastError());                                    \
  } while (0)

constexpr int kMaxDevices = 16;   // the length of every per-device table of the library (check_device's limit)

struct DeviceGuard {  // run on the given device, restore the caller's current device after
  int prev = -1;
  bool ok = false;
  DeviceGuard() = default;            // idle until enter()
  explicit DeviceGuard(int dev) { enter(dev); }
  void enter(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; return; }
    ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Is there a device, is the index one of them; `limit`: the length of a per-device table the caller indexes with it
inline int check_device(int device, int limit = INT_MAX) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return rced_fail(RCED_ERR_HIP, "no HIP device visible (this library has no CPU fallback)");
  if (n > limit) n = limit;
  if (device < 0 || device >= n) return rced_fail(RCED_ERR_ARG, "device %d out of range [0,%d)", device, n);
  return RCED_OK;
}

// check_device, then a DeviceGuard for the rest of the scope: `OnDevice on(device, limit); if (on.rc) return on.rc;`
struct OnDevice {
  int rc;
  DeviceGuard g;
  explicit OnDevice(int device, int limit = INT_MAX) : rc(check_device(device, limit)) {
    if (rc) return;
    g.enter(device);
    if (!g.ok) rc = rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  }
};

// A DeviceGuard for the rest of the scope, or its failure returned: for push / finish / reset paths, which ask for no device count
// (OnDevice does; it is for create paths)
#define ON_DEVICE(dev)        \
  DeviceGuard guard_(dev);    \
  if (!guard_.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", dev)

// One lane of [lanes][per_lane] elements of per-lane state, or (-1) all of them, back to zero behind the work queued on `last`
template <class T>
int reset_lanes(T* state, size_t per_lane, int lanes, int lane, int device, hipStream_t last) {
  if (lane < -1 || lane >= lanes) return rced_fail(RCED_ERR_ARG, "lane must be -1 (all) or 0..%d, got %d", lanes - 1, lane);
  ON_DEVICE(device);
  const size_t one = per_lane * sizeof(T);
  if (lane < 0) HIP_TRY(hipMemsetAsync(state, 0, one * lanes, last));
  else HIP_TRY(hipMemsetAsync(state + (size_t)lane * per_lane, 0, one, last));
  return RCED_OK;
}

template <class... A>
const void* kernel_ptr(void (*kernel)(A...)) { return reinterpret_cast<const void*>(kernel); }

// Each {kernel_ptr(kernel), bytes} may ask for that much dynamic LDS from now on; stops at the first failure.  `what`: "istft LDS"
inline int set_dynamic_lds(std::initializer_list<std::pair<const void*, int>> kernels, const char* what) {
  for (const auto& k : kernels) {
    const hipError_t e = hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, k.second);
    if (e != hipSuccess) return rced_fail(RCED_ERR_HIP, "hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
  }
  return RCED_OK;
}

// The refusals of a PCM format, in the words every resampling entry uses
inline int check_rates(int sr_in, int sr_out) {
  return sr_in <= 0 || sr_out <= 0 ? rced_fail(RCED_ERR_ARG, "sample rates must be positive, got %d -> %d", sr_in, sr_out) : RCED_OK;
}
inline int check_channels(int channels) {
  return channels < 1 ? rced_fail(RCED_ERR_ARG, "channels must be >= 1, got %d", channels) : RCED_OK;
}
inline int check_pcm_dtypes(int src_dtype, int out_dtype) {
  if (src_dtype != RCED_PCM_S16 && src_dtype != RCED_PCM_F32)
    return rced_fail(RCED_ERR_ARG, "src_dtype must be RCED_PCM_S16 or RCED_PCM_F32, got %d", src_dtype);
  if (out_dtype != RCED_PCM_S16 && out_dtype != RCED_PCM_F32)
    return rced_fail(RCED_ERR_ARG, "out_dtype must be RCED_PCM_S16 or RCED_PCM_F32, got %d", out_dtype);
  return RCED_OK;
}

// f(SRC_F32, OUT_F32) with the two PCM types as std::true_type / std::false_type: a kernel template's <SRC_F32, OUT_F32> from dtypes;
// what f returns (the code of its launch)
template <class F>
int with_pcm_types(int src_dtype, int out_dtype, F f) {
  const bool sf = src_dtype == RCED_PCM_F32, of = out_dtype == RCED_PCM_F32;
  if (sf && of) return f(std::true_type(), std::true_type());
  if (sf) return f(std::true_type(), std::false_type());
  if (of) return f(std::false_type(), std::true_type());
  return f(std::false_type(), std::false_type());
}

// A host vector as a fresh device allocation.  *dev is written only after the copy succeeded (a caller may test it for "built");
// on failure the allocation is freed.
template <class T>
int upload(T** dev, const std::vector<T>& host, const char* what) {
  T* p = nullptr;
  HIP_TRY(hipMalloc(&p, host.size() * sizeof(T)));
  const hipError_t e = hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return rced_fail(RCED_ERR_HIP, "hipMemcpy(%s): %s", what, hipGetErrorString(e));
  }
  *dev = p;
  return RCED_OK;
}

inline unsigned short bf16_rne(float f) {   // round to nearest even
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
inline float bf16_to_float(unsigned short b) {
  const unsigned u = (unsigned)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// three bf16 parts of a value (round to nearest at every step): v = h + m + l to 2^-24
inline void split3(float v, unsigned short* h, unsigned short* mm, unsigned short* l) {
  *h = bf16_rne(v);
  const float r1 = v - bf16_to_float(*h);
  *mm = bf16_rne(r1);
  *l = bf16_rne(r1 - bf16_to_float(*mm));
}
// ... stored into a [part][lane][8] bf16 tile: slot `at` of the parts h, m, l
inline void put3(unsigned short* d, size_t at, float v, size_t part_stride = 512) {
  split3(v, &d[at], &d[at + part_stride], &d[at + 2 * part_stride]);
}
