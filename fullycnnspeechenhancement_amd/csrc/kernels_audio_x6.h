// STFT front-end / ISTFT rebuild at fp32 quality on the bf16 matrix pipe (three-part operands, six products per MFMA-sized term: the
// form of the CR-CED kernel, kernels_fused_v3.h).  Same reference rows as kernels_audio.h (N1: data_utils/audio_feature.py:22-44,
// N2: model_utils/utils.py:171-183); the fp32-MFMA kernels there stay in the library as the comparator (rced_stft_ex / rced_istft_ex with RCED_AUDIO_F32).
//
// Both transforms are dense DFT GEMMs with K = 256 exactly once the two identically-zero terms are dropped:
//   STFT : 258 real rows (re, im of 129 bins) -> 256: im of bin 0 and of bin 128 are zero for a real signal, so row 1 carries re of bin
//          128 instead: row 0 = re(0), row 1 = re(128), rows 2b, 2b + 1 = re(b), im(b), b = 1..127  -> 16 M-tiles.
//   ISTFT: K slots 2b + c (c = 0 re, 1 im), b = 0..127; slot 1 (im of bin 0: irfft ignores it) carries re of bin 128.  im of bin 128
//          (ignored at nfft = 256, used at the reference's shipped nfft = 512) is one rank-1 update on the VALU.  Only samples 128..255
//          of a frame survive de_frame (utils.py:139-147) -- 8 M-tiles, not 16; samples 0..127 of frame 0 are a 33-k-MAC side kernel.
// Decomposition: ONE M-TILE PER WAVE with its A fragments resident in registers (8 chunks x 3 parts x 4 = 96 VGPRs, read once per
// workgroup), workgroups of 8 waves, each walking the 64-frame blocks of one utterance: the operand that is re-read per block is the
// small one (the signal).  The fp32 kernels re-fetched 278 KB of A fragments from the L2 per 64 frames: 570 MB per call at config 3.
// The signal block is split into its three bf16 parts ONCE, when it is staged (rows of 128 samples + 16 bytes of pad: a lane group's
// sixteen frames sit on sixteen different bank slots).
// The GEMM itself -- split, product order, fragment layout, chunk loop -- is x6_dft.h.  What is audio's but not one kernel's is a device
// function here, called by these kernels and by the streaming ones (kernels_stream.h): stft_store, slot_pair, rank1_add,
// head_spectrum / head_sample / head_deemph, deemph_scan.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_audio.h"
#include "x6_dft.h"

namespace rced {
namespace audio {
namespace x6 {

using namespace x6dft;   // mfma32, Parts, mma2, P3, split2, put_pair, AFrag, load_a, gemm_block, kChunks, kPackPerMT

constexpr int kWaves = 8, kThreadsX = kWaves * 64;
static_assert(kFrame == kK, "a frame is the GEMM's depth");
constexpr int kStftMTx = 16, kIstftMTx = 8;
constexpr int kStftPackX = kStftMTx * kPackPerMT;    // bf16
constexpr int kIstftPackX = kIstftMTx * kPackPerMT;  // bf16 (+ the rank-1 column and the head table, fp32: audio_api.hip)

// ---- STFT -------------------------------------------------------------------------------------------------------------------------
constexpr int kSegRowB = 2 * kStep + 16;                       // bytes per 128 samples of one part: 272
constexpr int kSegPartB = (kFramesPerWg + 1) * kSegRowB;       // 65 rows: 17,680
constexpr int kSegPairs = (kFramesPerWg + 1) * (kStep / 2);    // sample pairs of a block's segment: 4,160
constexpr int kSegIter = (kSegPairs + kThreadsX - 1) / kThreadsX;   // per thread: 9
// The raw samples a thread needs for its pairs of one block: s[g-1], s[g], s[g+1], g = 128 f0 + 2 (tid + 512 it).  Fetched one block AHEAD
// (27 registers), so that the loads' latency -- nine dependent trips to the L2 / HBM per block when they sat in the staging loop -- lies
// under the previous block's MFMAs.
struct SegRaw {
  float m[kSegIter], z[kSegIter], p[kSegIter];
};
__device__ __forceinline__ void seg_fetch(SegRaw& R, const float* __restrict__ s, int len, int f0, int tid) {
#pragma unroll
  for (int it = 0; it < kSegIter; ++it) {
    const int g = f0 * kStep + 2 * (tid + it * kThreadsX);
    const bool in = tid + it * kThreadsX < kSegPairs && g < len;
    R.z[it] = in ? s[g] : 0.f;
    R.m[it] = in && g > 0 ? s[g - 1] : 0.f;
    R.p[it] = in && g + 1 < len ? s[g + 1] : 0.f;
  }
}
// The STFT epilogue: one frame's accumulators of M-tile mt -> magnitude and unit phase at `row` (= the frame's index * 129; phase may be
// null).  Rows 4kq + {0,1} / {2,3} = (re, im) of bins 8 mt + 2kq + {0, 1}; M-tile 0, kq 0: rows 0, 1 = re of bin 0, re of bin 128.
// !live: a frame past the utterance leaves as a zero spectrum (padding_batch), phase 1 + 0j.
// fused_sq: re^2 + im^2 under the magnitude's root with one rounding (fma) or with two.  The one difference between the offline
// epilogue (fused: what the compiler's contraction had made of it) and the streaming one (not fused) since each was written; it was
// silent in two copies of the text, and each kernel keeps the bits it has always given.
__device__ __forceinline__ void stft_store(const f32x4 v, bool live, bool fused_sq, int mt, int kq, size_t row, float* __restrict__ mag,
                                           float* __restrict__ phase) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float re = live ? (h ? v.z : v.x) : 0.f, im = live ? (h ? v.w : v.y) : 0.f;
    const int b = 8 * mt + 2 * kq + h;
    if (b == 0) {   // (re(0), re(128)): two bins with zero imaginary part
      const float re128 = im;
      const float m128 = fabsf(re128);
      mag[row + kBins - 1] = m128;
      if (phase) *reinterpret_cast<f32x2*>(phase + 2 * (row + kBins - 1)) = m128 > 0.f ? f32x2{re128 / m128, 0.f} : f32x2{1.f, 0.f};
      im = 0.f;
    }
    float m2;
    {
#pragma clang fp contract(off)   // (__fmul_rn / __fadd_rn would not do: to this compiler they are the plain operators, and it fuses them)
      const float im2 = im * im;
      m2 = fused_sq ? fmaf(re, re, im2) : re * re + im2;
    }
    const float m = sqrtf(m2);
    mag[row + b] = m;
    if (phase) {
      const float inv = m > 0.f ? 1.f / m : 0.f;
      *reinterpret_cast<f32x2*>(phase + 2 * (row + b)) = m > 0.f ? f32x2{re * inv, im * inv} : f32x2{1.f, 0.f};
    }
  }
}

// grid (N, 2 M-groups, S frame ranges); pack: kStftPackX bf16
__global__ __launch_bounds__(kThreadsX) void stft_x6_kernel(const float* __restrict__ pcm, const int* __restrict__ lengths,
                                                             const unsigned short* __restrict__ apack, int L, int T, float* __restrict__ mag,
                                                             float* __restrict__ phase) {
  __shared__ __attribute__((aligned(16))) char seg[3 * kSegPartB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x, mt = blockIdx.y * kWaves + wave;
  const int len = lengths ? min(lengths[utt], L) : L;
  const int nf = len > 0 ? num_frames(len) : 0;
  const float* s = pcm + (size_t)utt * L;
  AFrag A;
  load_a(A, apack, mt, lane);
  const int nblk = (T + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  SegRaw R;
  if (blk0 < blk1) seg_fetch(R, s, len, blk0 * kFramesPerWg, tid);
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    __syncthreads();   // the previous block's reads of seg are done
    // stage the pre-emphasised, zero-padded segment [128 f0, 128 (f0 + 65)) as three bf16 parts, two samples per store.
    // e[0] = s[0], e[g] = s[g] - 0.97 s[g-1] as ONE float32 multiply and ONE float32 subtract (audio_feature.py:54 works in float32)
#pragma unroll
    for (int it = 0; it < kSegIter; ++it) {
      const int p = tid + it * kThreadsX;
      if (p < kSegPairs) {
        const int g = f0 * kStep + 2 * p;
        float e0 = 0.f, e1 = 0.f;
        if (g < len) {
          e0 = g == 0 ? R.z[it] : __fsub_rn(R.z[it], __fmul_rn(kPre, R.m[it]));
          if (g + 1 < len) e1 = __fsub_rn(R.p[it], __fmul_rn(kPre, R.z[it]));
        }
        put_pair(seg, kSegPartB, (p >> 6) * kSegRowB + (p & 63) * 4, e0, e1);
      }
    }
    __syncthreads();
    if (blk + 1 < blk1) seg_fetch(R, s, len, f0 + kFramesPerWg, tid);   // in flight during this block's MFMAs
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // sample k = 32c + 8kq + e of frame 16t + n: row (16t + n) + (c >> 2), byte 64 (c & 3) + 16 kq
    gemm_block(A, seg, kSegPartB, n * kSegRowB + 16 * kq, 16 * kSegRowB, [](int c) { return (c >> 2) * kSegRowB + 64 * (c & 3); }, acc);
    // (Staging the results in LDS and writing whole rows -- 256 contiguous bytes per frame instead of one lane per frame -- was measured:
    // 0.212 against 0.202 ms; the stores are not what this kernel waits for.)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int fr = f0 + 16 * t + n;
      if (fr < T) stft_store(acc[t], fr < nf, true, mt, kq, ((size_t)utt * T + fr) * kBins, mag, phase);
    }
  }
}

// ---- ISTFT ------------------------------------------------------------------------------------------------------------------------
constexpr int kXRowB = 2 * kFrame + 16;                        // bytes per frame of one part: 256 slots + pad = 528
constexpr int kXPartB = kFramesPerWg * kXRowB;                 // 33,792
constexpr int kORow = kStep + 4;                               // floats per frame of the output staging (conflict-free 16-byte stores)
constexpr int kIstftLdsBytes = 3 * kXPartB + (kFramesPerWg + 2 * kBins + kStep) * 4;   // images + xim + xk (frame 0's spectrum, fp32) + the head
static_assert(kFramesPerWg * kORow * 4 + 2 * kThreadsX * 4 <= 3 * kXPartB, "output staging + scan arrays alias the (dead) images");

// X = m * (re, im) at index o of a spectrum (merge_magphase, utils.py:119-126); m: magnitudes or masks
__device__ __forceinline__ f32x2 spec_at(const float* __restrict__ m, const float* __restrict__ phase, size_t o) {
  const float a = m[o];
  const f32x2 p = *reinterpret_cast<const f32x2*>(phase + 2 * o);
  return f32x2{a * p.x, a * p.y};
}
// K slots 2b, 2b + 1 of a frame, b < 128, o = the index of the frame's bin b: (re, im) of bin b, except that slot 1 (im of bin 0: irfft
// ignores it) carries re of bin 128; vi = im of bin 128 (b = 0 only), the rank-1 term's operand
__device__ __forceinline__ void slot_pair(const float* __restrict__ m, const float* __restrict__ phase, size_t o, int b, float& v0, float& v1,
                                          float& vi) {
  const f32x2 x = spec_at(m, phase, o);
  v0 = x.x;
  v1 = x.y;
  if (b == 0) {
    const f32x2 x8 = spec_at(m, phase, o + kBins - 1);
    v1 = x8.x;
    vi = x8.y;
  }
}
// + the rank-1 term of im(bin 128); rows = samples 128 + 16 wave + 4kq + j of frame 16 t + n; ci = this lane's four coefficients
__device__ __forceinline__ void rank1_add(f32x4 (&acc)[4], const f32x4 ci, const float* xim, int n) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float xi = xim[16 * t + n];
    acc[t].x = fmaf(ci.x, xi, acc[t].x);
    acc[t].y = fmaf(ci.y, xi, acc[t].y);
    acc[t].z = fmaf(ci.z, xi, acc[t].z);
    acc[t].w = fmaf(ci.w, xi, acc[t].w);
  }
}
// The head: samples 0..127 of frame 0, the only frame whose first half survives de_frame; K = 258 on the VALU, once per utterance.
// head_spectrum: the frame's 129 bins at index o0 -> xk[k = 2b + c], fp32, by `nthreads` threads; head_sample: sample n from it, chead:
// [k (258)][n (128)] fp32 (1 / nfft, irfft's factor 2, 1 / hamming folded in); head_deemph: y[0] = x[0], serial, returns y[127]
__device__ __forceinline__ void head_spectrum(float* xk, const float* __restrict__ m, const float* __restrict__ phase, size_t o0, int tid,
                                              int nthreads) {
  for (int b = tid; b < kBins; b += nthreads) {
    const f32x2 x = spec_at(m, phase, o0 + b);
    xk[2 * b] = x.x;
    xk[2 * b + 1] = x.y;
  }
}
__device__ __forceinline__ float head_sample(const float* __restrict__ chead, const float* xk, int n) {
  float s = 0.f;
#pragma unroll 6
  for (int k = 0; k < 2 * kBins; ++k) s = fmaf(chead[k * kStep + n], xk[k], s);
  return s;
}
__device__ __forceinline__ float head_deemph(float* h) {
  float run = 0.f;
#pragma unroll 16
  for (int j = 0; j < kStep; ++j) {
    run = fmaf(kPre, run, h[j]);
    h[j] = run;
  }
  return run;
}
// De-emphasis y[i] = x[i] + 0.97 y[i-1] of the 64 x 128 samples staged in obuf ([frame][kORow], time order) as a blocked affine scan:
// thread i owns samples 16 (i & 7) .. of frame i >> 3 (!live: zeros) and returns them in y; its segment starts at thread seg0 with
// `carry` = y just before it (a scan never reaches behind seg0).  sa, sb: 512 floats each; they are left holding every thread's
// composed map, so fmaf(sa[i], carry, sb[i]) is y after thread i's last sample.
__device__ __forceinline__ void deemph_scan(const float* obuf, float* sa, float* sb, int tid, bool live, int seg0, float carry,
                                            f32x4 (&y)[kDeBlock / 4]) {
  float pw[kDeBlock + 1];
  pw[0] = 1.f;
#pragma unroll
  for (int j = 1; j <= kDeBlock; ++j) pw[j] = pw[j - 1] * kPre;
  const float* src = obuf + (tid >> 3) * kORow + kDeBlock * (tid & 7);
  float run = 0.f;
#pragma unroll
  for (int j4 = 0; j4 < kDeBlock / 4; ++j4) {
    const f32x4 v = live ? *reinterpret_cast<const f32x4*>(src + 4 * j4) : f32x4{0.f, 0.f, 0.f, 0.f};
    run = fmaf(kPre, run, v.x);
    y[j4].x = run;
    run = fmaf(kPre, run, v.y);
    y[j4].y = run;
    run = fmaf(kPre, run, v.z);
    y[j4].z = run;
    run = fmaf(kPre, run, v.w);
    y[j4].w = run;
  }
  float Am = pw[kDeBlock], Bm = run;   // this thread's map: y_out = Am * y_in + Bm
  sa[tid] = Am;
  sb[tid] = Bm;
  __syncthreads();
  for (int d = 1; d < kThreadsX; d <<= 1) {
    const bool take = tid - d >= seg0;
    float a2 = 1.f, b2 = 0.f;
    if (take) {
      a2 = sa[tid - d];
      b2 = sb[tid - d];
    }
    __syncthreads();
    if (take) {   // compose: (earlier map) then (mine)
      Bm = fmaf(Am, b2, Bm);
      Am = Am * a2;
      sa[tid] = Am;
      sb[tid] = Bm;
    }
    __syncthreads();
  }
  const float yin = tid == seg0 ? carry : fmaf(sa[tid - 1], carry, sb[tid - 1]);
#pragma unroll
  for (int j4 = 0; j4 < kDeBlock / 4; ++j4)
    y[j4] = f32x4{fmaf(pw[4 * j4 + 1], yin, y[j4].x), fmaf(pw[4 * j4 + 2], yin, y[j4].y), fmaf(pw[4 * j4 + 3], yin, y[j4].z),
                  fmaf(pw[4 * j4 + 4], yin, y[j4].w)};
}
// mag [N,T,129], phase [N,T,129,2] -> x [N, (T+1)*128].  grid (N, 1, S).  cpack: kIstftPackX bf16; cim: 128 floats, the coefficients of
// im(bin 128) for samples 128..255 (zero at nfft = 256); chead: [k = 2b + c (258)][n (128)] fp32 for samples 0..127 of frame 0.
// FUSED (S = 1: one workgroup walks the whole utterance): de_frame AND de_emphasis (utils.py:139-147, 104-113) here too -- the block's
// 8,192 samples go through LDS, a blocked affine scan (16 samples per thread, 512 threads, the carry across blocks in a register) turns
// them into y[i] = x[i] + 0.97 y[i-1], and they leave with coalesced 16-byte stores: no second pass over the signal in HBM, no
// scattered 16-byte stores from the MFMA layout.  !FUSED: the frames' second halves only (istft_head_kernel + deemphasis_kernel follow).
template <bool FUSED>
__global__ __launch_bounds__(kThreadsX) void istft_x6_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                              const unsigned short* __restrict__ cpack, const float* __restrict__ cim,
                                                              const float* __restrict__ chead, int T, float* __restrict__ x) {
  extern __shared__ __attribute__((aligned(16))) char xs[];
  float* xim = reinterpret_cast<float*>(xs + 3 * kXPartB);
  float* xk = xim + kFramesPerWg;        // frame 0's spectrum (fp32, k = 2b + c)
  float* hbuf = xk + 2 * kBins;          // samples 0..127 of frame 0
  float* obuf = reinterpret_cast<float*>(xs);                       // [frame][kORow]: aliases the images once the GEMM has read them
  float* sa = obuf + kFramesPerWg * kORow;                          // the scan's affine maps
  float* sb = sa + kThreadsX;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, kq = lane >> 4;
  const int utt = blockIdx.x;
  AFrag A;
  load_a(A, cpack, wave, lane);
  const f32x4 ci = *reinterpret_cast<const f32x4*>(cim + 16 * wave + 4 * kq);   // rows 4kq .. 4kq+3 of this wave's M-tile
  float* xo = x + (size_t)utt * (T + 1) * kStep;
  const int nblk = (T + kFramesPerWg - 1) / kFramesPerWg, per = (nblk + (int)gridDim.z - 1) / (int)gridDim.z;
  const int blk0 = blockIdx.z * per, blk1 = min(nblk, blk0 + per);
  float carry = 0.f;   // y just before the block (FUSED)
  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * kFramesPerWg;
    __syncthreads();
    if (FUSED && blk == 0) head_spectrum(xk, mag, phase, (size_t)utt * T * kBins, tid, kThreadsX);
    // stage X[frame][slot 2b + c] as three bf16 parts; im of bin 128 to xim (fp32); zero past T
    for (int i = tid; i < kFramesPerWg * 128; i += kThreadsX) {
      const int fr = i >> 7, b = i & 127;
      float v0 = 0.f, v1 = 0.f, vi = 0.f;
      if (f0 + fr < T) slot_pair(mag, phase, ((size_t)utt * T + f0 + fr) * kBins + b, b, v0, v1, vi);
      if (b == 0) xim[fr] = vi;
      put_pair(xs, kXPartB, fr * kXRowB + b * 4, v0, v1);
    }
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm_block(A, xs, kXPartB, n * kXRowB + 16 * kq, 16 * kXRowB, [](int c) { return 64 * c; }, acc);
    rank1_add(acc, ci, xim, n);
    if constexpr (!FUSED) {   // de_frame (utils.py:139-147): sample 128 + s of frame fr goes to out[128 fr + 128 + s]
      const int n0 = kStep + 16 * wave + 4 * kq;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int fr = f0 + 16 * t + n;
        if (fr < T) *reinterpret_cast<f32x4*>(xo + (size_t)fr * kStep + n0) = acc[t];
      }
    } else {
      if (blk == 0 && tid < kStep) hbuf[tid] = head_sample(chead, xk, tid);   // waves 0, 1
      __syncthreads();   // every wave has read its last fragment: the images are dead
#pragma unroll
      for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(obuf + (16 * t + n) * kORow + 16 * wave + 4 * kq) = acc[t];
      if (blk == 0 && tid == 0) head_deemph(hbuf);   // 128 serial steps, once per utterance
      __syncthreads();
      if (blk == 0) {
        if (tid < kStep) xo[tid] = hbuf[tid];
        carry = hbuf[kStep - 1];
      }
      // the block's 8,192 samples in time order, one segment
      const int fl = tid >> 3;
      const bool live = f0 + fl < T;
      f32x4 y[kDeBlock / 4];
      deemph_scan(obuf, sa, sb, tid, live, 0, carry, y);
      if (live) {
        float* dst = xo + (size_t)(f0 + fl + 1) * kStep + kDeBlock * (tid & 7);
#pragma unroll
        for (int j4 = 0; j4 < kDeBlock / 4; ++j4) *reinterpret_cast<f32x4*>(dst + 4 * j4) = y[j4];
      }
      carry = fmaf(sa[kThreadsX - 1], carry, sb[kThreadsX - 1]);   // (frames past T contribute zeros: unused)
    }
  }
}

// the head of every utterance, for the !FUSED path: thread n = sample n; chead: the fp32 kernels' coefficients
__global__ __launch_bounds__(kStep) void istft_head_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                            const float* __restrict__ chead, int T, float* __restrict__ x) {
  __shared__ float xk[2 * kBins];
  const int n = threadIdx.x, utt = blockIdx.x;
  head_spectrum(xk, mag, phase, (size_t)utt * T * kBins, n, kStep);
  __syncthreads();
  x[(size_t)utt * (T + 1) * kStep + n] = head_sample(chead, xk, n);
}

}  // namespace x6
}  // namespace audio
}  // namespace rced
