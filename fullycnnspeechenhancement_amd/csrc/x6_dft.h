// The K = 256 DFT GEMM at fp32 quality on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16), once: operands in three bf16 parts, six
// products per term, smallest first.  What defines the arithmetic of the STFT / ISTFT (kernels_audio_x6.h), the streaming kernels
// (kernels_stream.h) and STOI's band spectra (kernels_stoi.h) is here and nowhere else: the split's rounding (split2), the order of
// the six products (mma2), the fragment layout [mt][chunk][part][lane][8] (pack_x6 writes it on the host, load_a reads it) and the
// chunk loop with its prefetch (gemm_block).
// Inline functions and constants only -- no kernel, no kernel header -- so every translation unit may include it, inside an unnamed
// namespace as well (stream_api.hip; host_util.h must then have been included before, at file scope).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "host_util.h"

namespace rced {
namespace x6dft {

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kK = 256;                              // the GEMM's depth
constexpr int kChunks = kK / 32;                     // in eight K = 32 chunks
constexpr int kPackPerMT = kChunks * 3 * 64 * 8;     // bf16 per M-tile: [chunk][part][lane][8]

__device__ __forceinline__ f32x4 mfma32(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
struct Parts {
  s16x8 h, m, l;
};
// the six products of one chunk for two independent chains, smallest first (kernels_fused_v3_l23.h mma2)
__device__ __forceinline__ void mma2(const s16x8 (&a)[3], const Parts& b0, f32x4& c0, const Parts& b1, f32x4& c1) {
  c0 = mfma32(a[1], b0.m, c0);
  c1 = mfma32(a[1], b1.m, c1);
  c0 = mfma32(a[2], b0.h, c0);
  c1 = mfma32(a[2], b1.h, c1);
  c0 = mfma32(a[0], b0.l, c0);
  c1 = mfma32(a[0], b1.l, c1);
  c0 = mfma32(a[1], b0.h, c0);
  c1 = mfma32(a[1], b1.h, c1);
  c0 = mfma32(a[0], b0.m, c0);
  c1 = mfma32(a[0], b1.m, c1);
  c0 = mfma32(a[0], b0.h, c0);
  c1 = mfma32(a[0], b1.h, c1);
}
// two fp32 values -> three packed bf16 pairs, x = h + m + l to 2^-24 (round to nearest at every step)
struct P3 {
  unsigned h, m, l;
};
__device__ __forceinline__ P3 split2(float x0, float x1) {
  P3 p;
  const bf16x2 bh = {(__bf16)x0, (__bf16)x1};
  p.h = __builtin_bit_cast(unsigned, bh);
  const float r0 = x0 - __builtin_bit_cast(float, p.h << 16), r1 = x1 - __builtin_bit_cast(float, p.h & 0xffff0000u);
  const bf16x2 bm = {(__bf16)r0, (__bf16)r1};
  p.m = __builtin_bit_cast(unsigned, bm);
  const float s0 = r0 - __builtin_bit_cast(float, p.m << 16), s1 = r1 - __builtin_bit_cast(float, p.m & 0xffff0000u);
  const bf16x2 bl = {(__bf16)s0, (__bf16)s1};
  p.l = __builtin_bit_cast(unsigned, bl);
  return p;
}
// ... stored into a B image: the three parts of the pair at byte `byte_off` of images `part_bytes` apart
__device__ __forceinline__ void put_pair(char* img, int part_bytes, int byte_off, float x0, float x1) {
  const P3 q = split2(x0, x1);
  char* d = img + byte_off;
  *reinterpret_cast<unsigned*>(d) = q.h;
  *reinterpret_cast<unsigned*>(d + part_bytes) = q.m;
  *reinterpret_cast<unsigned*>(d + 2 * part_bytes) = q.l;
}

// The A operand, [mt][chunk][part][lane][8] bf16, from a coefficient function coef(row, k): lane holds row 16 mt + (lane & 15),
// k = 32 chunk + 8 (lane >> 4) + e
template <class F>
std::vector<unsigned short> pack_x6(int mtiles, F coef) {
  std::vector<unsigned short> p((size_t)mtiles * kPackPerMT, 0);
  for (int mt = 0; mt < mtiles; ++mt)
    for (int c = 0; c < kChunks; ++c)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int row = 16 * mt + (lane & 15), k = 32 * c + 8 * (lane >> 4) + e;
          const size_t at = (size_t)mt * kPackPerMT + ((size_t)(c * 3) * 64 + lane) * 8 + e;
          put3(p.data(), at, (float)coef(row, k));
        }
  return p;
}
// a wave's A fragments of one M-tile: [chunk][part], lane's 16 bytes each (8 x 3 x 4 = 96 VGPRs)
struct AFrag {
  s16x8 a[kChunks][3];
};
__device__ __forceinline__ void load_a(AFrag& A, const unsigned short* pack, int mt, int lane) {
  const u32x4* src = reinterpret_cast<const u32x4*>(pack + (size_t)mt * kPackPerMT) + lane;
#pragma unroll
  for (int c = 0; c < kChunks; ++c)
#pragma unroll
    for (int q = 0; q < 3; ++q) A.a[c][q] = __builtin_bit_cast(s16x8, src[(c * 3 + q) * 64]);
}

// D[16 rows of the M-tile][64 frames] += A x B over K = 256.  B: three bf16 images in LDS; `lane_off` = this lane's byte offset
// (frame n of an N-tile, k-quad kq), `tile_stride` = bytes between N-tiles, chunk_off(c) = byte offset of chunk c inside a frame's row.
template <class ChunkOff>
__device__ __forceinline__ void gemm_block(const AFrag& A, const char* img, int part_bytes, int lane_off, int tile_stride, ChunkOff chunk_off,
                                           f32x4 (&acc)[4]) {
  Parts b[2][4];
  auto ld = [&](int c, int r) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const char* p = img + lane_off + t * tile_stride + chunk_off(c);
      b[r][t].h = *reinterpret_cast<const s16x8*>(p);
      b[r][t].m = *reinterpret_cast<const s16x8*>(p + part_bytes);
      b[r][t].l = *reinterpret_cast<const s16x8*>(p + 2 * part_bytes);
    }
  };
  ld(0, 0);
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    if (c + 1 < kChunks) ld(c + 1, (c + 1) & 1);
    mma2(A.a[c], b[c & 1][0], acc[0], b[c & 1][1], acc[1]);
    mma2(A.a[c], b[c & 1][2], acc[2], b[c & 1][3], acc[3]);
  }
}

}  // namespace x6dft
}  // namespace rced
