// The two per-device stores of the host runtime, each defined here once: the grow-only workspace of a (device, stream), and the
// tables a device gets built once.  Host only.
#pragma once
#include <map>
#include <mutex>

#include "host_carve.h"
#include "host_util.h"

// One device buffer per (device, stream) that only grows.  Launches on one stream are ordered, so the buffer of a stream is never
// shared by two calls in flight.  A call whose size fits gets the pointer: no allocation, no synchronisation -- which is what lets
// an entry be stream-captured after one warm-up call at its shape.  A call that needs more waits for the stream, frees and allocates.
// One object is one buffer family: entries that bind to different objects never move each other's buffer (a captured graph keeps
// reading the address it was captured with).  Nothing is freed at exit; the destructor makes no HIP call.
struct StreamWorkspace {
  template <class T>
  int get(int device, void* stream, size_t bytes, T** out) {
    std::lock_guard<std::mutex> lk(mu_);
    Buf& w = bufs_[device][stream];
    if (w.bytes < bytes) {
      if (w.p) {
        HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));   // an earlier call may still read it
        (void)hipFree(w.p);
        w = Buf();
      }
      HIP_TRY(hipMalloc(&w.p, bytes));
      w.bytes = bytes;
    }
    *out = static_cast<T*>(w.p);
    return RCED_OK;
  }

 private:
  struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
  };
  std::map<void*, Buf> bufs_[kMaxDevices];
  std::mutex mu_;
};

inline int Carve::bind(int device, void* stream, StreamWorkspace& ws) {
  char* base = nullptr;
  if (int rc = ws.get(device, stream, bytes, &base)) return rc;
  for (int i = 0; i < n; ++i) {
    char* p = base + at[i];
    memcpy(slot[i], &p, sizeof p);
  }
  return RCED_OK;
}

// What a device gets built once, in `Variants` forms: T says what "built" means (bool built() const) and how to give back a build
// that failed half way (void release()).  build(T&) fills a local, under the lock; only a complete one is published, and a failure
// leaves the slot empty for the next call to try again.
template <class T, int Variants = 1>
struct DeviceOnce {
  template <class Build>
  int get(int device, int variant, Build build, T** out) {
    std::lock_guard<std::mutex> lk(mu_);
    T& pub = slot_[device][variant];
    if (!pub.built()) {
      T t;
      if (int rc = build(t)) {
        t.release();
        return rc;
      }
      pub = t;
    }
    *out = &pub;
    return RCED_OK;
  }

 private:
  T slot_[kMaxDevices][Variants];
  std::mutex mu_;
};
