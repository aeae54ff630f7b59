// Overlap-add ISTFT (least-squares weighted overlap-add, Griffin & Lim 1984): the opt-in rebuild next to the reference's
// (kernels_audio_x6.h istft_x6_kernel).  For an utterance of F frames, x_t = irfft(mag_t * phase_t, 256), w = hamming(256):
//   e[i] = sum_{t<F} w[i - 128t] x_t[i - 128t] / sum_{t<F} w[i - 128t]^2,  i < 128 (F + 1);   y[i] = e[i] + 0.97 y[i-1], y[0] = e[0].
// Hop h (samples 128h .. 128h + 127) = first half of frame h + second half of frame h - 1; hops 0 and F have one frame only.
// The GEMM is x6_dft.h's, unchanged; the staging is slot_pair's, the de-emphasis deemph_scan's (kernels_audio_x6.h).
//   Coefficients: 16 M-tiles, row r = sample r of a frame, K = 256 exactly (slot 1 = re of bin 128; im of bins 0 and 128 is ignored by
//     irfft at nfft = 256: no rank-1 term).  Folded in: 1 / 256, irfft's factor 2, w[r] and the INTERIOR denominator
//     D[r & 127] = w[r & 127]^2 + w[(r & 127) + 128]^2.  The two single-frame hops are put right per sample: x D[s] / w[s]^2 (hop 0),
//     x D[s] / w[s + 128]^2 (hop F): the table `fix` [2][128].  A row's error scales with the row, so the edge samples are conditioned as
//     the reference's 1 / w is (12.5 at s = 0), no worse.
//   Ownership: wave v owns M-tiles v and v + 8 -- samples 16v .. 16v + 15 of BOTH halves of every frame -- in two passes over the same
//     staged images, so both addends of an output sample come from one wave: frame h - 1 sits one lane, or one N-tile, below frame h,
//     a lane shuffle away.  The first pass's addend is stored to the output staging (LDS, behind the images), the second pass's is
//     added to it in place by the lane that stored it: no atomics, no ordering beyond the barriers the staging needs anyway, and
//     a + b in either order of arrival is the same bits.
//   A fragments: 2 x 96 VGPRs resident do not fit next to the B double buffer (96) and the accumulators under 256 (the kernel takes
//     250 with ONE resident, no scratch); one AFrag is kept and reloaded between the passes, and the passes alternate their order
//     from block to block (.. v, v + 8 | v + 8, v | ..), so a block costs ONE reload (12 KB per wave from the L2), not two.
//   Seam: the second half of a block's last frame stays in four registers of the lanes that computed it and enters the next block's
//     frame 0 through the same shuffle.  Hop F falls out of the walk: blocks cover hops 0 .. F, i.e. F / 64 + 1 of them; when F is a
//     multiple of 64 the last one holds hop F alone and runs no GEMM.
//   Frames at or past F are never loaded (after the net a padded frame is not zero, and it would bleed into hop F): they are staged as
//     zeros, so utterance n's result depends on F and its own frames only -- not on T, N, its row or its neighbours.
// One workgroup per utterance; there is no split over frame ranges (the de-emphasis carry and the seam make a range's start depend on
// everything before it; the reference rebuild's split form pays a second pass over the signal for it).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_audio_x6.h"

namespace rced {
namespace audio {
namespace x6 {

constexpr int kOlaMTx = 16;
constexpr int kOlaPackX = kOlaMTx * kPackPerMT;   // bf16
constexpr int kOlaLdsBytes = 3 * kXPartB + (kFramesPerWg * kORow + 2 * kThreadsX) * 4;   // the three images, the output staging, the scan's arrays: 139,264
static_assert(kOlaLdsBytes <= 160 * 1024, "one workgroup's LDS");

// frame h - 1's value for the lane that holds frame h = 16 t + n: one lane below, or -- n = 0 -- lane 15 of the N-tile below (`below`:
// that tile's accumulators, for t = 0 the previous block's last)
__device__ __forceinline__ f32x4 frame_below(const f32x4 same, const f32x4 below, int lane) {
  const int up = (lane - 1) & 63, top = lane | 15;   // (what a lane hands over cannot depend on who asks: two shuffles, one kept)
  const f32x4 a = f32x4{__shfl(same.x, up, 64), __shfl(same.y, up, 64), __shfl(same.z, up, 64), __shfl(same.w, up, 64)};
  const f32x4 b = f32x4{__shfl(below.x, top, 64), __shfl(below.y, top, 64), __shfl(below.z, top, 64), __shfl(below.w, top, 64)};
  return (lane & 15) ? a : b;
}

// mag [N,T,129], phase [N,T,129,2], frames [N] or null (= T each; clamped into [0, T]) -> y [N, (T+1)*128], every column written.
// grid (N).  cpack: kOlaPackX bf16; fix: [2][128] fp32, the single-frame factors of hop 0 and hop F.
__global__ __launch_bounds__(kThreadsX) void istft_ola_x6_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                                  const int* __restrict__ frames, const unsigned short* __restrict__ cpack,
                                                                  const float* __restrict__ fix, int T, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  float* obuf = reinterpret_cast<float*>(xs + 3 * kXPartB);   // [hop][kORow], behind the images: it fills while they are still read
  float* sa = obuf + kFramesPerWg * kORow;      // the scan's affine maps
  float* sb = sa + kThreadsX;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x;
  const int F = frames ? min(max(frames[utt], 0), T) : T;
  float* yo = y + (size_t)utt * (T + 1) * kStep;
  const int s0 = 16 * wave + 4 * kq;   // this lane's four samples of a hop
  AFrag A;
  int held = wave;                     // the M-tile A holds: wave (first halves) or wave + 8 (second halves)
  if (F > 0) load_a(A, cpack, held, lane);
  f32x4 seam = f32x4{0.f, 0.f, 0.f, 0.f};   // second half of the previous block's frames 48..63 (lane n = 15: frame 63)
  float carry = 0.f;                        // y just before the block
  // A lane's share of hop f0 + 16 t + n (its four samples, obuf + 16 t rows) arrives in two addends, from its own two passes: the
  // first is stored, the second added to it in place -- the lane's own words, no other lane touches them -- and, on the two
  // single-frame hops, the sum is put right (the interior denominator out, that frame's in).
  auto put = [&](float* at, int h, const f32x4 v, bool second) {
    f32x4 u = v;
    if (second) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(at);
      u = f32x4{o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w};
      if (h == 0 || h == F) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(fix + (h == 0 ? 0 : kStep) + s0);
        u = f32x4{u.x * g.x, u.y * g.y, u.z * g.z, u.w * g.w};
      }
    }
    *reinterpret_cast<f32x4*>(at) = u;
  };
  const int nblk = F > 0 ? F / kFramesPerWg + 1 : 0;
  for (int blk = 0; blk < nblk; ++blk) {
    const int f0 = blk * kFramesPerWg;
    float* mine = obuf + n * kORow + s0;   // + 16 t rows
    f32x4 acc[4];
    auto zero = [&]() {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // the pass of M-tile wave: first halves, frame = hop
    auto first_half = [&](bool second) {
#pragma unroll
      for (int t = 0; t < 4; ++t) put(mine + 16 * t * kORow, f0 + 16 * t + n, acc[t], second);
    };
    // the pass of M-tile wave + 8: second halves, frame = hop - 1
    auto second_half = [&](bool second) {
#pragma unroll
      for (int t = 0; t < 4; ++t) put(mine + 16 * t * kORow, f0 + 16 * t + n, frame_below(acc[t], t ? acc[t - 1] : seam, lane), second);
      seam = acc[3];
    };
    __syncthreads();      // the previous block's reads of the images, obuf, sa, sb are done
    if (f0 < F) {
      // stage X[frame][slot 2b + c] as three bf16 parts; zero at and past F
      for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
        const int fr = i >> 7, b = i & 127;
        float v0 = 0.f, v1 = 0.f, vi = 0.f;
        if (f0 + fr < F) slot_pair(mag, phase, ((size_t)utt * T + f0 + fr) * kBins + b, b, v0, v1, vi);
        put_pair(xs, kXPartB, fr * kXRowB + b * 4, v0, v1);
      }
      __syncthreads();
      const int lane_off = n * kXRowB + 16 * kq;
      auto chunk = [](int c) { return 64 * c; };
      // the tile A holds, then the other one; the order alternates from block to block, so a block reloads A once, not twice
      zero();
      gemm_block(A, xs, kXPartB, lane_off, 16 * kXRowB, chunk, acc);
      load_a(A, cpack, held ^ kWaves, lane);
      if (held & kWaves) second_half(false); else first_half(false);
      zero();
      gemm_block(A, xs, kXPartB, lane_off, 16 * kXRowB, chunk, acc);
      if (held & kWaves) first_half(true); else second_half(true);
      held ^= kWaves;
    } else {   // F is a multiple of 64: hop F alone, the seam's
      zero();
      second_half(false);
      first_half(true);
    }
    __syncthreads();
    // the block's hops in time order, one segment
    const int fl = tid >> 3;
    const bool live = f0 + fl <= F;
    f32x4 yv[kDeBlock / 4];
    deemph_scan(obuf, sa, sb, tid, live, 0, carry, yv);
    if (live) {
      float* dst = yo + (size_t)(f0 + fl) * kStep + kDeBlock * (tid & 7);
#pragma unroll
      for (int j4 = 0; j4 < kDeBlock / 4; ++j4) *reinterpret_cast<f32x4*>(dst + 4 * j4) = yv[j4];
    }
    carry = fmaf(sa[kThreadsX - 1], carry, sb[kThreadsX - 1]);   // (hops past F contribute zeros: unused)
  }
  // columns from 128 (F + 1) -- from 0 for an utterance of no frames -- to the end of the row
  const int z0 = F > 0 ? (F + 1) * kStep : 0, z1 = (T + 1) * kStep;
  for (int base = z0; base < z1; base += 4 * kThreadsX)   // (a uniform trip count: the lane's own bound guards the store, not the loop)
    if (base + 4 * tid < z1) *reinterpret_cast<f32x4*>(yo + base + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace x6
}  // namespace audio
}  // namespace rced
