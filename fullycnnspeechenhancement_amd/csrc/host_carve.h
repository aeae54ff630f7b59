// An entry's workspace, carved: the offset arithmetic alone.  No HIP call and no HIP header -- tests/host_ws_check.cpp includes this
// file on its own; host_ws.h defines bind().
#pragma once
#include <cassert>
#include <cstddef>
#include <cstring>

struct StreamWorkspace;   // host_ws.h

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// take() books `count` elements of T at the next 256-byte boundary, in the order of the calls; bind() gets the whole from a
// StreamWorkspace and points every booked pointer at its part.  At most 8 buffers.
struct Carve {
  void* slot[8];
  size_t at[8], bytes = 0;
  int n = 0;
  template <class T>
  void take(T** p, size_t count) {
    assert(n < 8);
    slot[n] = p;
    at[n++] = bytes;
    bytes += align256(count * sizeof(T));
  }
  int bind(int device, void* stream, StreamWorkspace& ws);
};
