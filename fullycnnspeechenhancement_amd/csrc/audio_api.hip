// C ABI of the STFT front-end / ISTFT rebuild (include/rced.h, "audio" section): host side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/rced.h"
#include <cstdlib>
#include <cstring>

#include "host_ws.h"
#include "kernels_audio.h"
#include "kernels_audio_x6.h"
#include "kernels_ola_x6.h"
#include "kernels_framing.h"
#include "kernels_wave_loss.h"
#include "kernels_wave_loss_fr.h"
#include "kernels_mr_stft.h"
#include "rced_internal.h"

using namespace rced;

namespace {

struct AudioTables {   // per device, built once
  float* stft = nullptr;
  float* istft512 = nullptr;
  float* istft256 = nullptr;
  // the three-part bf16 form (kernels_audio_x6.h): A fragments, the rank-1 column of im(bin 128), the head table
  unsigned short* stft_x6 = nullptr;
  unsigned short* istft_x6[2] = {nullptr, nullptr};   // [nfft == 512]
  float* cim[2] = {nullptr, nullptr};
  float* chead[2] = {nullptr, nullptr};
  // overlap-add (kernels_ola_x6.h): 16 M-tiles of A fragments, the single-frame factors of hops 0 and F
  unsigned short* ola_x6 = nullptr;
  float* ola_fix = nullptr;
  // the rebuild's adjoint (kernels_wave_loss.h): the STFT's 16 M-tiles with kappa_b / 256 folded in, the reciprocal denominators [3][128]
  unsigned short* adj_x6 = nullptr;
  float* adj_inv = nullptr;
  bool built() const { return stft; }   // the first one uploaded: a published entry has all of them, and the LDS attributes
  void release() {   // of a build that failed half way
    for (void* p : {(void*)stft, (void*)istft512, (void*)istft256, (void*)stft_x6, (void*)ola_x6, (void*)ola_fix, (void*)adj_x6, (void*)adj_inv})
      (void)hipFree(p);
    for (int v = 0; v < 2; ++v)
      for (void* p : {(void*)istft_x6[v], (void*)cim[v], (void*)chead[v]}) (void)hipFree(p);
  }
};
DeviceOnce<AudioTables> g_tab;

double hamming(int k) { return 0.54 - 0.46 * std::cos(2.0 * M_PI * k / (audio::kFrame - 1)); }   // np.hamming(256)

std::vector<float> pack_stft() {   // [st][mt][lane][e]; row m = 2b + {0: re, 1: im}; window folded in
  std::vector<float> p(audio::kStftPack, 0.f);
  for (int st = 0; st < audio::kStftSteps; ++st)
    for (int mt = 0; mt < audio::kStftMT; ++mt)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 2; ++e) {
          const int m = 16 * mt + (lane & 15), k = 8 * st + 2 * (lane >> 4) + e, b = m >> 1;
          if (b >= audio::kBins) continue;
          const double th = 2.0 * M_PI * ((b * k) % audio::kFrame) / audio::kFrame;
          p[((size_t)st * audio::kStftMT + mt) * 128 + lane * 2 + e] =
              (float)(hamming(k) * ((m & 1) ? -std::sin(th) : std::cos(th)));
        }
  return p;
}

std::vector<float> pack_istft(int nfft) {   // [st][mt][lane][e]; row = sample n; k = 2b + {re, im}
  std::vector<float> p(audio::kIstftPack, 0.f);
  for (int st = 0; st < audio::kIstftSteps; ++st)
    for (int mt = 0; mt < audio::kIstftMT; ++mt)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 2; ++e) {
          const int n = 16 * mt + (lane & 15), k = 8 * st + 2 * (lane >> 4) + e, b = k >> 1, c = k & 1;
          if (b >= audio::kBins) continue;
          // numpy.fft.irfft: bin 0 (and the Nyquist bin nfft/2) count once and lose their imaginary part
          const bool edge = b == 0 || 2 * b == nfft;
          if (edge && c) continue;
          const double th = 2.0 * M_PI * ((long long)b * n % nfft) / nfft;
          const double coef = (edge ? 1.0 : 2.0) / nfft / hamming(n);   // de_window folded in
          p[((size_t)st * audio::kIstftMT + mt) * 128 + lane * 2 + e] = (float)(coef * (c ? -std::sin(th) : std::cos(th)));
        }
  return p;
}

using x6dft::pack_x6;
// STFT rows (kernels_audio_x6.h): 0 = re(0), 1 = re(128), 2b / 2b + 1 = re / im of bin b
double stft_coef(int row, int k) {
  const int b = row == 1 ? 128 : row >> 1;
  const bool im = row >= 2 && (row & 1);
  const double th = 2.0 * M_PI * ((b * k) % audio::kFrame) / audio::kFrame;
  return hamming(k) * (im ? -std::sin(th) : std::cos(th));
}
// ISTFT coefficient of spectrum term (bin b, c = 0 re / 1 im) for output sample n (numpy.fft.irfft: bin 0 and the Nyquist bin nfft / 2
// count once and lose their imaginary part; 1 / nfft and the 1 / hamming de-window folded in)
double istft_coef(int nfft, int n, int b, int c) {
  const bool edge = b == 0 || 2 * b == nfft;
  if (edge && c) return 0.0;
  const double th = 2.0 * M_PI * ((long long)b * n % nfft) / nfft;
  return (edge ? 1.0 : 2.0) / nfft / hamming(n) * (c ? -std::sin(th) : std::cos(th));
}

constexpr const char* kWhat = "audio tables";

int build_x6(AudioTables& t) {
  if (int rc = upload(&t.stft_x6, pack_x6(audio::x6::kStftMTx, stft_coef), kWhat)) return rc;
  for (int v = 0; v < 2; ++v) {
    const int nfft = v ? 512 : 256;
    // rows = samples 128..255; slot k = 2b + c, slot 1 = re of bin 128
    auto coef = [&](int row, int k) { return k == 1 ? istft_coef(nfft, 128 + row, 128, 0) : istft_coef(nfft, 128 + row, k >> 1, k & 1); };
    if (int rc = upload(&t.istft_x6[v], pack_x6(audio::x6::kIstftMTx, coef), kWhat)) return rc;
    std::vector<float> cim(128), head((size_t)2 * audio::kBins * 128);
    for (int r = 0; r < 128; ++r) cim[r] = (float)istft_coef(nfft, 128 + r, 128, 1);
    for (int k = 0; k < 2 * audio::kBins; ++k)
      for (int n = 0; n < 128; ++n) head[(size_t)k * 128 + n] = (float)istft_coef(nfft, n, k >> 1, k & 1);
    if (int rc = upload(&t.cim[v], cim, kWhat)) return rc;
    if (int rc = upload(&t.chead[v], head, kWhat)) return rc;
  }
  {   // overlap-add: rows = samples 0..255 of a frame, the synthesis window over the interior denominator folded in
    auto den = [](int s) { return hamming(s) * hamming(s) + hamming(s + 128) * hamming(s + 128); };
    auto coef = [&](int row, int k) {
      return (k == 1 ? istft_coef(256, row, 128, 0) : istft_coef(256, row, k >> 1, k & 1)) * hamming(row) * hamming(row) / den(row & 127);
    };
    if (int rc = upload(&t.ola_x6, pack_x6(audio::x6::kOlaMTx, coef), kWhat)) return rc;
    std::vector<float> fix(2 * 128);
    for (int s = 0; s < 128; ++s) {
      fix[s] = (float)(den(s) / (hamming(s) * hamming(s)));
      fix[128 + s] = (float)(den(s) / (hamming(s + 128) * hamming(s + 128)));
    }
    if (int rc = upload(&t.ola_fix, fix, kWhat)) return rc;
    // the adjoint: G = rfft(w u) projected with kappa_b / 256 (irfft's weights: bins 0 and 128 count once); u = g_e / the denominator
    auto adj = [](int row, int k) { return stft_coef(row, k) * (row < 2 ? 1.0 : 2.0) / audio::kFrame; };
    if (int rc = upload(&t.adj_x6, pack_x6(audio::x6::kStftMTx, adj), kWhat)) return rc;
    std::vector<float> inv(3 * 128);
    for (int s = 0; s < 128; ++s) {
      inv[s] = (float)(1.0 / den(s));
      inv[128 + s] = (float)(1.0 / (hamming(s) * hamming(s)));
      inv[256 + s] = (float)(1.0 / (hamming(s + 128) * hamming(s + 128)));
    }
    if (int rc = upload(&t.adj_inv, inv, kWhat)) return rc;
  }
  return set_dynamic_lds({{kernel_ptr(audio::x6::istft_x6_kernel<true>), audio::x6::kIstftLdsBytes},
                          {kernel_ptr(audio::x6::istft_ola_x6_kernel), audio::x6::kOlaLdsBytes},
                          {kernel_ptr(audio::x6::istft_x6_kernel<false>), audio::x6::kIstftLdsBytes}},
                         "istft LDS");
}

// frame-range split of an utterance over workgroups: enough workgroups for every CU when the batch is small
int range_split(int N, int T) {
  const int nblk = (T + audio::kFramesPerWg - 1) / audio::kFramesPerWg;
  int s = 1;
  while (s < nblk && N * s < 256) s *= 2;
  return s < nblk ? s : nblk;
}

int build_tables(AudioTables& t) {
  if (int rc = upload(&t.stft, pack_stft(), kWhat)) return rc;
  if (int rc = upload(&t.istft512, pack_istft(512), kWhat)) return rc;
  if (int rc = upload(&t.istft256, pack_istft(256), kWhat)) return rc;
  return build_x6(t);
}

// What the STFT and rebuild entries refuse alike, in the order each of them refuses it.  skip_T0: a call without frames has nothing
// to do (an overlap-add rebuild still zeroes its output); pointers: the ones the call will read or write are there; nfft, L: of the
// entries that take one.  kNothingToDo: the caller returns RCED_OK without a launch.
constexpr int kNothingToDo = -1;
int audio_args(int N, int T, bool skip_T0, bool pointers, int nfft = 512, int L = 1) {
  if (N < 0 || L < 0 || T < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (nfft != 512 && nfft != 256) return rced_fail(RCED_ERR_ARG, "nfft must be 512 (reference default) or 256");
  if (N == 0 || (skip_T0 && T == 0)) return kNothingToDo;
  if (L == 0) return rced_fail(RCED_ERR_ARG, "empty signals (L = 0) with T > 0");
  if (!pointers) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  return RCED_OK;
}

// The device's tables (built on first use: host_ws.h), with the device current for as long as `g` lives
int tables(int device, DeviceGuard& g, AudioTables** out) {
  g.enter(device);
  if (int rc = check_device(device, kMaxDevices)) return rc;
  if (int rc = g_tab.get(device, 0, build_tables, out)) return rc;
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  return RCED_OK;
}

// ---- any framing (kernels_framing.h) ----------------------------------------------------------------------------------------------
// numpy's hamming / hanning / blackman / bartlett at length W >= 2, as numpy evaluates them (over n = 1 - W + 2k), in double
double window_at(int name, int W, int k) {
  const double n = 1.0 - W + 2.0 * k, a = M_PI * n / (W - 1);
  switch (name) {
    case RCED_WINDOW_HAMMING: return 0.54 + 0.46 * std::cos(a);
    case RCED_WINDOW_HANNING: return 0.5 + 0.5 * std::cos(a);
    case RCED_WINDOW_BLACKMAN: return 0.42 + 0.5 * std::cos(a) + 0.08 * std::cos(2.0 * a);
    default: return n <= 0 ? 1.0 + n / (W - 1) : 1.0 - n / (W - 1);   // bartlett
  }
}

const char* const kWindowNames[4] = {"hamming", "hanning", "blackman", "bartlett"};

int framing_check(int W, int S, int name) {
  if (W < 2 || W > audio::fr::kMaxWindow)
    return rced_fail(RCED_ERR_ARG, "window must lie in [2, 256] samples (rfft(256) would crop a longer frame), got %d", W);
  if (S < 1 || S > W) return rced_fail(RCED_ERR_ARG, "stride must lie in [1, window = %d] samples, got %d", W, S);
  if (name < 0 || name > 3) return rced_fail(RCED_ERR_ARG, "window name must be RCED_WINDOW_HAMMING .. RCED_WINDOW_BARTLETT (0..3), got %d", name);
  return RCED_OK;
}

int reference_rebuild_check(int name) {
  if (name != RCED_WINDOW_HAMMING)
    return rced_fail(RCED_ERR_ARG,
                     "the reference rebuild divides every frame by its window, and the ends of a %s window are zero: the result is not "
                     "finite (or off by 1e17); it is built for hamming only -- use the overlap-add rebuild",
                     name >= 0 && name <= 3 ? kWindowNames[name] : "?");
  return RCED_OK;
}

// One pack per (kind, window length, window name) and device, with the fp32 table that goes with it; the stride enters no pack.
enum { kFrStft = 0, kFrOla = 1, kFrRef256 = 2, kFrRef512 = 3, kFrAdjoint = 4, kFrMrSynth = 5 };
struct FrPack {
  unsigned short* pack = nullptr;
  float* aux = nullptr;   // rebuilds: [2][256], the coefficients of im(bin 128) (row scale folded in), then w^2; kFrStft, kFrAdjoint: none
  int pins = 0;           // streams at this framing (rced_fr_tables_pin): a pinned pack is never dropped
};
std::map<int, FrPack> g_fr[kMaxDevices];
bool g_fr_attr[kMaxDevices] = {};
// Held by an _fr entry from its look-up to its last launch: a pack or a frame buffer is never freed (below) between the moment a call
// has its pointer and the moment its kernels are queued.
std::mutex g_fr_mu;
constexpr size_t kFrMaxPacks = 64;   // 25 MB; past it every pack of the device that no stream has pinned is dropped (after the device has gone idle) and rebuilt on demand

double irfft_coef(int nfft, int n, int b, int c) {   // istft_coef without a window
  const bool edge = b == 0 || 2 * b == nfft;
  if (edge && c) return 0.0;
  const double th = 2.0 * M_PI * ((long long)b * n % nfft) / nfft;
  return (edge ? 1.0 : 2.0) / nfft * (c ? -std::sin(th) : std::cos(th));
}

int build_fr(FrPack& e, int kind, int W, int name) {
  std::vector<double> w(audio::kFrame, 0.0);
  for (int k = 0; k < W; ++k) w[k] = window_at(name, W, k);
  if (kind == kFrStft || kind == kFrAdjoint) {
    // kFrAdjoint (kernels_wave_loss_fr.h): the rebuild's adjoint, G = rfft(w u) with irfft's weights kappa_b / 256 folded in
    auto coef = [&](int row, int k) {
      const int b = row == 1 ? 128 : row >> 1;
      const bool im = row >= 2 && (row & 1);
      const double th = 2.0 * M_PI * ((b * k) % audio::kFrame) / audio::kFrame;
      const double scale = kind == kFrAdjoint ? (row < 2 ? 1.0 : 2.0) / audio::kFrame : 1.0;
      return w[k] * scale * (im ? -std::sin(th) : std::cos(th));
    };
    return upload(&e.pack, pack_x6(audio::fr::kFrMT, coef), kWhat);
  }
  if (kind == kFrMrSynth) {
    // kernels_mr_stft.h: the transpose of the STFT's pack -- rows = samples, K slot 2b + c, slot 1 = re of bin 128 (the imaginary parts
    // of bins 0 and 128 are zero), w[row](cos, -sin), zero rows past W; no 1 / 256 and no kappa: it is the analysis' adjoint
    auto coef = [&](int row, int k) {
      const int b = k == 1 ? 128 : k >> 1;
      const bool im = k >= 2 && (k & 1);
      const double th = 2.0 * M_PI * ((b * row) % audio::kFrame) / audio::kFrame;
      return w[row] * (im ? -std::sin(th) : std::cos(th));
    };
    return upload(&e.pack, pack_x6(audio::fr::kFrMT, coef), kWhat);
  }
  const int nfft = kind == kFrRef512 ? 512 : 256;
  auto scale = [&](int r) { return r >= W ? 0.0 : kind == kFrOla ? w[r] : 1.0 / w[r]; };
  auto coef = [&](int row, int k) { return scale(row) * (k == 1 ? irfft_coef(nfft, row, 128, 0) : irfft_coef(nfft, row, k >> 1, k & 1)); };
  if (int rc = upload(&e.pack, pack_x6(audio::fr::kFrMT, coef), kWhat)) return rc;
  std::vector<float> aux(2 * audio::kFrame);
  for (int r = 0; r < audio::kFrame; ++r) {
    aux[r] = (float)(scale(r) * irfft_coef(nfft, r, 128, 1));    // zero at nfft = 256: irfft ignores im of the Nyquist bin
    aux[audio::kFrame + r] = (float)(w[r] * w[r]);
  }
  return upload(&e.aux, aux, kWhat);
}

int fr_key(int kind, int W, int name) { return (kind * 4 + name) * 512 + W; }

int fr_pack(int device, int kind, int W, int name, FrPack* out) {   // g_fr_mu held
  if (int rc = check_device(device, kMaxDevices)) return rc;
  if (!g_fr_attr[device]) {
    if (int rc = set_dynamic_lds({{kernel_ptr(audio::fr::stft_fr_kernel), audio::fr::kStftFrLdsBytes},
                                  {kernel_ptr(audio::fr::frames_fr_kernel), audio::fr::kFramesFrLdsBytes},
                                  {kernel_ptr(wloss::fr::adjoint_kernel<true>), audio::fr::kStftFrLdsBytes},
                                  {kernel_ptr(wloss::fr::adjoint_kernel<false>), audio::fr::kStftFrLdsBytes},
                                  {kernel_ptr(mrstft::analysis_kernel), audio::fr::kStftFrLdsBytes},
                                  {kernel_ptr(mrstft::synth_kernel), audio::fr::kStftFrLdsBytes}},
                                 "framing LDS"))
      return rc;
    g_fr_attr[device] = true;
  }
  std::map<int, FrPack>& m = g_fr[device];
  const int key = fr_key(kind, W, name);
  auto it = m.find(key);
  if (it == m.end()) {
    if (m.size() >= kFrMaxPacks) {
      HIP_TRY(hipDeviceSynchronize());   // a kernel in flight may still read one
      for (auto kv = m.begin(); kv != m.end();) {
        if (kv->second.pins) {
          ++kv;
          continue;
        }
        (void)hipFree(kv->second.pack);
        (void)hipFree(kv->second.aux);
        kv = m.erase(kv);
      }
    }
    FrPack e;
    if (int rc = build_fr(e, kind, W, name)) {
      (void)hipFree(e.pack);
      return rc;
    }
    it = m.emplace(key, e).first;
  }
  *out = it->second;
  return RCED_OK;
}

// The frames between the two steps of a rebuild, [N, T, 256] fp32: the stream's workspace (host_ws.h), one family for both rebuilds
StreamWorkspace g_fr_frames;
StreamWorkspace g_wave_ws;   // rced_wave_loss's workspace, carved in rced_wave_loss_run
StreamWorkspace g_wave_fr_ws;   // rced_wave_loss_fr's, carved in rced_wave_loss_fr_run

// frames_fr_kernel, then rebuild_fr_kernel<OLA>
template <bool OLA>
int rebuild_fr(const float* mag_dev, const float* phase_dev, const int* frames_dev, int N, int T, int kind, int W, int S, int name,
               float* audio_dev, int device, void* stream) {
  DeviceGuard g(device);
  std::lock_guard<std::mutex> lk(g_fr_mu);
  FrPack p;
  if (int rc = fr_pack(device, kind, W, name, &p)) return rc;
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* Y = nullptr;
  if (T > 0) {
    if (int rc = g_fr_frames.get(device, stream, (size_t)N * T * audio::kFrame * sizeof(float), &Y)) return rc;
    const int nblk = (T + audio::kFramesPerWg - 1) / audio::kFramesPerWg;
    if (nblk > 65535) return rced_fail(RCED_ERR_ARG, "T > 65535 * 64 frames per call");
    LAUNCH(audio::fr::frames_fr_kernel, dim3(N, 2, nblk), dim3(audio::x6::kThreadsX), audio::fr::kFramesFrLdsBytes, st, mag_dev, phase_dev,
           frames_dev, (const unsigned short*)p.pack, (const float*)p.aux, T, W, Y);
  }
  LAUNCH(audio::fr::rebuild_fr_kernel<OLA>, dim3(N), dim3(audio::x6::kThreadsX), 0, st, (const float*)Y, frames_dev,
         (const float*)p.aux + audio::kFrame, T, W, S, (long long)(W - S) + (long long)T * S, audio_dev);
  return RCED_OK;
}

}  // namespace

int rced_audio_x6_tables_get(int device, int nfft, rced_audio_x6_tables* out) {
  DeviceGuard g;
  AudioTables* t = nullptr;
  if (int rc = tables(device, g, &t)) return rc;
  const int v = nfft == 512;
  out->stft = t->stft_x6;
  out->istft = t->istft_x6[v];
  out->cim = t->cim[v];
  out->chead = t->chead[v];
  out->ola = t->ola_x6;
  out->ola_fix = t->ola_fix;
  return RCED_OK;
}

int rced_fr_tables_pin(int device, int window, int window_name, int ola, int nfft, rced_fr_tables* out) {
  DeviceGuard g(device);
  std::lock_guard<std::mutex> lk(g_fr_mu);
  const int kind = ola ? kFrOla : nfft == 512 ? kFrRef512 : kFrRef256;
  FrPack a, c;
  if (int rc = fr_pack(device, kFrStft, window, window_name, &a)) return rc;
  g_fr[device][fr_key(kFrStft, window, window_name)].pins++;   // (before the second look-up, which may drop what is not pinned)
  if (int rc = fr_pack(device, kind, window, window_name, &c)) {
    g_fr[device][fr_key(kFrStft, window, window_name)].pins--;
    return rc;
  }
  g_fr[device][fr_key(kind, window, window_name)].pins++;
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  out->stft = a.pack;
  out->rebuild = c.pack;
  out->cim = c.aux;
  out->w2 = c.aux + audio::kFrame;
  return RCED_OK;
}

void rced_fr_tables_unpin(int device, int window, int window_name, int ola, int nfft) {
  std::lock_guard<std::mutex> lk(g_fr_mu);
  const int kind = ola ? kFrOla : nfft == 512 ? kFrRef512 : kFrRef256;
  for (int key : {fr_key(kFrStft, window, window_name), fr_key(kind, window, window_name)}) {
    auto it = g_fr[device].find(key);
    if (it != g_fr[device].end() && it->second.pins > 0) it->second.pins--;
  }
}

extern "C" {

int rced_stft_num_frames(int length) { return length > 0 ? audio::num_frames(length) : 0; }

int rced_stft(const float* pcm_dev, const int* lengths_dev, int N, int L, int T, float* mag_dev, float* phase_dev,
              int device, void* stream) {
  return rced_stft_ex(pcm_dev, lengths_dev, N, L, T, mag_dev, phase_dev, device, stream, RCED_AUDIO_X6);
}

int rced_stft_ex(const float* pcm_dev, const int* lengths_dev, int N, int L, int T, float* mag_dev, float* phase_dev,
                 int device, void* stream, int kernels) {
  if (kernels != RCED_AUDIO_X6 && kernels != RCED_AUDIO_F32) return rced_fail(RCED_ERR_ARG, "kernels must be RCED_AUDIO_X6 (1) or RCED_AUDIO_F32 (0), got %d", kernels);
  if (int rc = audio_args(N, T, true, pcm_dev && mag_dev, 512, L)) return rc == kNothingToDo ? RCED_OK : rc;
  DeviceGuard g;
  AudioTables* t = nullptr;
  if (int rc = tables(device, g, &t)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (kernels == RCED_AUDIO_X6) {
    LAUNCH(audio::x6::stft_x6_kernel, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), 0, st, pcm_dev, lengths_dev,
           (const unsigned short*)t->stft_x6, L, T, mag_dev, phase_dev);
  } else {
    const dim3 grid((T + audio::kFramesPerWg - 1) / audio::kFramesPerWg, N);
    LAUNCH(audio::stft_kernel, grid, dim3(audio::kThreads), 0, st, pcm_dev, lengths_dev, (const float*)t->stft, L, T, mag_dev, phase_dev);
  }
  return RCED_OK;
}

int rced_istft(const float* mag_dev, const float* phase_dev, int N, int T, int nfft, float* audio_dev, int device,
               void* stream) {
  return rced_istft_ex(mag_dev, phase_dev, N, T, nfft, audio_dev, device, stream, RCED_AUDIO_X6);
}

int rced_istft_ex(const float* mag_dev, const float* phase_dev, int N, int T, int nfft, float* audio_dev, int device,
                  void* stream, int kernels) {
  if (kernels != RCED_AUDIO_X6 && kernels != RCED_AUDIO_F32) return rced_fail(RCED_ERR_ARG, "kernels must be RCED_AUDIO_X6 (1) or RCED_AUDIO_F32 (0), got %d", kernels);
  if (int rc = audio_args(N, T, true, mag_dev && phase_dev && audio_dev, nfft)) return rc == kNothingToDo ? RCED_OK : rc;
  DeviceGuard g;
  AudioTables* t = nullptr;
  if (int rc = tables(device, g, &t)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (kernels == RCED_AUDIO_X6) {
    const int v = nfft == 512, split = range_split(N, T);
    if (split == 1) {   // one workgroup per utterance: de_frame and de_emphasis inside the kernel
      LAUNCH(audio::x6::istft_x6_kernel<true>, dim3(N, 1, 1), dim3(audio::x6::kThreadsX), audio::x6::kIstftLdsBytes, st, mag_dev, phase_dev,
             (const unsigned short*)t->istft_x6[v], (const float*)t->cim[v], (const float*)t->chead[v], T, audio_dev);
      return RCED_OK;
    }
    // (every launch of this entry was followed by a check of its own before: the head's was the one after the else)
    LAUNCH(audio::x6::istft_x6_kernel<false>, dim3(N, 1, split), dim3(audio::x6::kThreadsX), audio::x6::kIstftLdsBytes, st, mag_dev, phase_dev,
           (const unsigned short*)t->istft_x6[v], (const float*)t->cim[v], (const float*)t->chead[v], T, audio_dev);
    LAUNCH(audio::x6::istft_head_kernel, dim3(N), dim3(audio::kStep), 0, st, mag_dev, phase_dev, (const float*)t->chead[v], T, audio_dev);
  } else {
    const dim3 grid((T + audio::kFramesPerWg - 1) / audio::kFramesPerWg, N);
    LAUNCH(audio::istft_frames_kernel, grid, dim3(audio::kThreads), 0, st, mag_dev, phase_dev,
           (const float*)(nfft == 512 ? t->istft512 : t->istft256), T, audio_dev);
  }
  LAUNCH(audio::deemphasis_kernel, dim3(N), dim3(audio::kThreads), 0, st, audio_dev, (T + 1) * audio::kStep);
  return RCED_OK;
}

int rced_istft_ola(const float* mag_dev, const float* phase_dev, const int* frames_dev, int N, int T, float* audio_dev, int device,
                   void* stream) {
  if (int rc = audio_args(N, T, false, audio_dev && (T == 0 || (mag_dev && phase_dev)))) return rc == kNothingToDo ? RCED_OK : rc;
  DeviceGuard g;
  AudioTables* t = nullptr;
  if (int rc = tables(device, g, &t)) return rc;
  // one workgroup per utterance walks its blocks: the add across frames, the seam, the de-emphasis and the zero tail in one launch
  LAUNCH(audio::x6::istft_ola_x6_kernel, dim3(N), dim3(audio::x6::kThreadsX), audio::x6::kOlaLdsBytes, static_cast<hipStream_t>(stream),
         mag_dev, phase_dev, frames_dev, (const unsigned short*)t->ola_x6, (const float*)t->ola_fix, T, audio_dev);
  return RCED_OK;
}

int rced_wave_loss(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                   const int* lengths_dev, int N, int T, double w_sse, double w_si_sdr, int skip_edges, double inv_batch,
                   double* terms_dev, float* grad_dev, int device, void* stream) {
  return rced_wave_loss_run(mag_dev, phase_dev, frames_dev, clean_dev, clean_stride, lengths_dev, N, T, w_sse, w_si_sdr, skip_edges, inv_batch,
                            terms_dev, grad_dev, 0, device, stream);
}

}  // extern "C"

// What rced_wave_loss and rced_wave_loss_fr refuse alike, before any device work; kNothingToDo for N = 0
static int wave_loss_args(const float* mag_dev, const float* phase_dev, const float* clean_dev, int clean_stride, const int* lengths_dev, int N,
                          int T, double w_sse, double w_si_sdr, int skip_edges, double inv_batch, const double* terms_dev) {
  if (N < 0 || T < 0 || clean_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!(w_sse >= 0.0) || !(w_si_sdr >= 0.0) || !std::isfinite(w_sse) || !std::isfinite(w_si_sdr))
    return rced_fail(RCED_ERR_ARG, "the weights must be finite and >= 0, got w_sse = %g, w_si_sdr = %g", w_sse, w_si_sdr);
  if (!(inv_batch > 0.0) || !std::isfinite(inv_batch)) return rced_fail(RCED_ERR_ARG, "inv_batch must be finite and > 0, got %g", inv_batch);
  if (skip_edges != 0 && skip_edges != 1) return rced_fail(RCED_ERR_ARG, "skip_edges must be 0 or 1, got %d", skip_edges);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (T > (1 << 22)) return rced_fail(RCED_ERR_ARG, "T > 2^22 frames");
  if (N == 0) return kNothingToDo;
  if (!terms_dev || !lengths_dev || (clean_stride > 0 && !clean_dev) || (T > 0 && (!mag_dev || !phase_dev)))
    return rced_fail(RCED_ERR_ARG, "null pointer");
  return RCED_OK;
}

int rced_wave_loss_fr_run(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                          const int* lengths_dev, int N, int T, int W, int S, int name, double w_sse, double w_si_sdr, int skip_edges,
                          double inv_batch, double* terms_dev, float* grad_dev, int accumulate, int device, void* stream) {
  if (int rc = framing_check(W, S, name)) return rc;
  if (int rc = wave_loss_args(mag_dev, phase_dev, clean_dev, clean_stride, lengths_dev, N, T, w_sse, w_si_sdr, skip_edges, inv_batch, terms_dev))
    return rc == kNothingToDo ? RCED_OK : rc;
  const int nblk = (T + audio::kFramesPerWg - 1) / audio::kFramesPerWg;
  if (nblk > 65535) return rced_fail(RCED_ERR_ARG, "T > 65535 * 64 frames per call");
  DeviceGuard g(device);
  std::lock_guard<std::mutex> lk(g_fr_mu);
  FrPack ola, adj;
  // (a look-up may drop every pack that no stream has pinned, once: the third one finds, or rebuilds, the first)
  if (int rc = fr_pack(device, kFrOla, W, name, &ola)) return rc;
  if (int rc = fr_pack(device, kFrAdjoint, W, name, &adj)) return rc;
  if (int rc = fr_pack(device, kFrOla, W, name, &ola)) return rc;
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const long long L = wloss::fr::row_stride(T, W, S);   // floats per row of y and u: whole 16-byte groups
  const int slices = wloss::num_slices((int)L);         // (L < 2^31: T <= 2^22, S <= 256)
  float *y, *u, *Y;    // [N, L]: the rebuild, the scaled reverse scan; [N, T, 256]: the frames between the rebuild's two steps
  double *ws1, *ws2;   // [N, slices, 2]
  double* scal;        // [N, 4]
  int* frames;         // [N]
  Carve ws;
  ws.take(&y, (size_t)N * L);
  ws.take(&u, (size_t)N * L);
  ws.take(&Y, (size_t)N * T * audio::kFrame);
  ws.take(&ws1, (size_t)N * slices * 2);
  ws.take(&ws2, (size_t)N * slices * 2);
  ws.take(&scal, (size_t)N * 4);
  ws.take(&frames, (size_t)N);
  if (int rc = ws.bind(device, stream, g_wave_fr_ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* w2 = ola.aux + audio::kFrame;
  LAUNCH(wloss::fr::counts_kernel, dim3((N + 255) / 256), dim3(256), 0, st, frames_dev, lengths_dev, N, T, W, S, frames);
  if (T > 0)
    LAUNCH(audio::fr::frames_fr_kernel, dim3(N, 2, nblk), dim3(audio::x6::kThreadsX), audio::fr::kFramesFrLdsBytes, st, mag_dev, phase_dev,
           (const int*)frames, (const unsigned short*)ola.pack, (const float*)ola.aux, T, W, Y);
  LAUNCH(audio::fr::rebuild_fr_kernel<true>, dim3(N), dim3(audio::x6::kThreadsX), 0, st, (const float*)Y, (const int*)frames, w2, T, W, S, L, y);
  LAUNCH(wloss::sums_kernel<0>, dim3(slices, N), dim3(wloss::kSumThreads), 0, st, (const float*)y, (int)L, clean_dev, clean_stride, lengths_dev,
         (const int*)frames, skip_edges, W, S, (const double*)nullptr, ws1, slices);
  LAUNCH(wloss::sums_kernel<1>, dim3(slices, N), dim3(wloss::kSumThreads), 0, st, (const float*)y, (int)L, clean_dev, clean_stride, lengths_dev,
         (const int*)frames, skip_edges, W, S, (const double*)ws1, ws2, slices);
  LAUNCH(wloss::terms_kernel, dim3(N), dim3(wloss::kSumThreads), 0, st, (const double*)ws1, (const double*)ws2, lengths_dev,
         (const int*)frames, clean_stride, skip_edges, W, S, slices, terms_dev, 3, scal);
  if (grad_dev && T > 0) {
    LAUNCH(wloss::fr::reverse_kernel<false>, dim3(N), dim3(audio::x6::kThreadsX), 0, st, (const float*)y, L, clean_dev, clean_stride, lengths_dev,
           (const int*)frames, skip_edges, W, S, (const double*)scal, 2.0 * w_sse * inv_batch, w_si_sdr * inv_batch, w2, (const float*)nullptr,
           u);
    if (accumulate)
      LAUNCH(wloss::fr::adjoint_kernel<true>, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes, st,
             (const float*)u, L, (const int*)frames, (const unsigned short*)adj.pack, phase_dev, T, W, S, grad_dev);
    else
      LAUNCH(wloss::fr::adjoint_kernel<false>, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes, st,
             (const float*)u, L, (const int*)frames, (const unsigned short*)adj.pack, phase_dev, T, W, S, grad_dev);
  }
  return RCED_OK;
}

int rced_wave_loss_run(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                       const int* lengths_dev, int N, int T, double w_sse, double w_si_sdr, int skip_edges, double inv_batch,
                       double* terms_dev, float* grad_dev, int accumulate, int device, void* stream) {
  if (int rc = wave_loss_args(mag_dev, phase_dev, clean_dev, clean_stride, lengths_dev, N, T, w_sse, w_si_sdr, skip_edges, inv_batch, terms_dev))
    return rc == kNothingToDo ? RCED_OK : rc;
  DeviceGuard g;
  AudioTables* t = nullptr;
  if (int rc = tables(device, g, &t)) return rc;
  const int L = (T + 1) * audio::kStep, slices = wloss::num_slices(L);
  float *y, *u;        // [N, (T+1)*128]: the rebuild, the scaled reverse scan
  double *ws1, *ws2;   // [N, slices, 2]
  double* scal;        // [N, 4]
  int* frames;         // [N]
  Carve ws;
  ws.take(&y, (size_t)N * L);
  ws.take(&u, (size_t)N * L);
  ws.take(&ws1, (size_t)N * slices * 2);
  ws.take(&ws2, (size_t)N * slices * 2);
  ws.take(&scal, (size_t)N * 4);
  ws.take(&frames, (size_t)N);
  if (int rc = ws.bind(device, stream, g_wave_ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(wloss::frames_kernel, dim3((N + 255) / 256), dim3(256), 0, st, frames_dev, lengths_dev, N, T, frames);
  LAUNCH(audio::x6::istft_ola_x6_kernel, dim3(N), dim3(audio::x6::kThreadsX), audio::x6::kOlaLdsBytes, st, mag_dev, phase_dev,
         (const int*)frames, (const unsigned short*)t->ola_x6, (const float*)t->ola_fix, T, y);
  LAUNCH(wloss::sums_kernel<0>, dim3(slices, N), dim3(wloss::kSumThreads), 0, st, (const float*)y, L, clean_dev, clean_stride, lengths_dev,
         (const int*)frames, skip_edges, audio::kFrame, audio::kStep, (const double*)nullptr, ws1, slices);
  LAUNCH(wloss::sums_kernel<1>, dim3(slices, N), dim3(wloss::kSumThreads), 0, st, (const float*)y, L, clean_dev, clean_stride, lengths_dev,
         (const int*)frames, skip_edges, audio::kFrame, audio::kStep, (const double*)ws1, ws2, slices);
  LAUNCH(wloss::terms_kernel, dim3(N), dim3(wloss::kSumThreads), 0, st, (const double*)ws1, (const double*)ws2, lengths_dev,
         (const int*)frames, clean_stride, skip_edges, audio::kFrame, audio::kStep, slices, terms_dev, 3, scal);
  if (grad_dev && T > 0) {
    LAUNCH(wloss::reverse_kernel, dim3(N), dim3(audio::x6::kThreadsX), 0, st, (const float*)y, L, clean_dev, clean_stride, lengths_dev,
           (const int*)frames, skip_edges, (const double*)scal, 2.0 * w_sse * inv_batch, w_si_sdr * inv_batch,
           (const float*)t->adj_inv, u);
    if (accumulate)
      LAUNCH(wloss::adjoint_kernel<true>, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), 0, st, (const float*)u, L,
             (const int*)frames, (const unsigned short*)t->adj_x6, phase_dev, T, grad_dev);
    else
      LAUNCH(wloss::adjoint_kernel<false>, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), 0, st, (const float*)u, L,
             (const int*)frames, (const unsigned short*)t->adj_x6, phase_dev, T, grad_dev);
  }
  return RCED_OK;
}

// ---- the multi-resolution STFT term (kernels_mr_stft.h) ----------------------------------------------------------
static StreamWorkspace g_mr_ws;           // rced_mr_stft's workspace
static StreamWorkspace g_wave_mr_ws;      // rced_wave_loss_mr's: the rebuild's part, carved as rced_wave_loss_fr's
static StreamWorkspace g_wave_mr_ws2;     // ... and the term's part, carved by mr_take

static int mr_check(const rced_mr_args* mr) {
  if (!mr) return rced_fail(RCED_ERR_ARG, "the multi-resolution arguments are NULL");
  if (!(mr->w_mr >= 0.0) || !std::isfinite(mr->w_mr)) return rced_fail(RCED_ERR_ARG, "w_mr must be finite and >= 0, got %g", mr->w_mr);
  if (mr->n_res < 1 || mr->n_res > mrstft::kMaxRes) return rced_fail(RCED_ERR_ARG, "n_res must lie in [1, 4] resolutions, got %d", mr->n_res);
  for (int r = 0; r < mr->n_res; ++r)
    if (int rc = framing_check(mr->window[r], mr->stride[r], mr->window_name[r])) return rc;
  return RCED_OK;
}

struct MrPlan {
  mrstft::Params P;
  FrPack ana[mrstft::kMaxRes], syn[mrstft::kMaxRes];
  int Jmx = 0, nslmax = 1;   // the most frames of any resolution, and its 64-frame slices
  size_t scratch = 0;        // floats of the frame scratch, every resolution
  float *ysp = nullptr, *ym = nullptr, *cm = nullptr, *frsc = nullptr, *gmr = nullptr;
  double* part = nullptr;
  int2* rng = nullptr;
};

// The shapes for N rows whose ranges are at most Lmax samples wide
static void mr_shape(const rced_mr_args* mr, long long Lmax, int N, MrPlan& pl) {
  pl.P.K = mr->n_res;
  for (int r = 0; r < mr->n_res; ++r) {
    const int W = mr->window[r], S = mr->stride[r], Wp = (W + 15) & ~15;
    const int Jmax = Lmax >= W ? (int)((Lmax - W) / S) + 1 : 0;
    pl.P.r[r] = mrstft::Res{W, S, Wp, Jmax, (long long)pl.scratch};
    pl.scratch += (size_t)N * Jmax * Wp;
    pl.Jmx = std::max(pl.Jmx, Jmax);
  }
  pl.nslmax = std::max(1, (pl.Jmx + audio::kFramesPerWg - 1) / audio::kFramesPerWg);
}

// seven buffers: a Carve of their own.  gmr_floats: the fp32 row set the gather writes when the caller's gradient is not that row set
static void mr_take(Carve& ws, MrPlan& pl, int N, bool grad, size_t gmr_floats) {
  const size_t bins = (size_t)N * pl.Jmx * audio::kBins;
  ws.take(&pl.ysp, 2 * bins);
  ws.take(&pl.ym, bins);
  ws.take(&pl.cm, bins);
  ws.take(&pl.part, (size_t)N * pl.P.K * pl.nslmax * 3);
  ws.take(&pl.rng, (size_t)N);
  ws.take(&pl.frsc, grad ? pl.scratch : 0);
  ws.take(&pl.gmr, gmr_floats);
}

// the packs of every resolution (g_fr_mu held).  A look-up may drop every pack that no stream has pinned, once: the second round
// finds, or rebuilds, what the first one lost
static int mr_packs(const rced_mr_args* mr, int device, bool grad, MrPlan& pl) {
  for (int round = 0; round < 2; ++round)
    for (int r = 0; r < mr->n_res; ++r) {
      if (int rc = fr_pack(device, kFrStft, mr->window[r], mr->window_name[r], &pl.ana[r])) return rc;
      if (grad)
        if (int rc = fr_pack(device, kFrMrSynth, mr->window[r], mr->window_name[r], &pl.syn[r])) return rc;
    }
  return RCED_OK;
}

static int mr_split(int N, int Jmax) {
  const int nblk = (Jmax + audio::kFramesPerWg - 1) / audio::kFramesPerWg;
  int s = 1;
  while (s < nblk && (long long)N * s < 512) s *= 2;
  return std::max(1, std::min(s, nblk));
}

// Per resolution analysis, sums and -- with a gradient -- synthesis, before the next resolution reuses the spectra; then the terms and
// the gather: 2 K + 1 launches, 3 K + 2 with a gradient.  pl.rng holds the ranges.  g [N, gstride]: columns below gwidth are written.
static int mr_run(const MrPlan& pl, const float* est, long long est_stride, const float* ref, long long ref_stride, int N, double scale,
                  double* out, int out_stride, int detail, float* g, long long gwidth, long long gstride, hipStream_t st) {
  const size_t pstride = (size_t)pl.P.K * pl.nslmax * 3;
  for (int r = 0; r < pl.P.K; ++r) {
    const mrstft::Res& q = pl.P.r[r];
    if (q.Jmax == 0) continue;   // no row is as long as this window
    double* part = pl.part + (size_t)r * pl.nslmax * 3;
    LAUNCH(mrstft::analysis_kernel, dim3(2 * N, 2, mr_split(2 * N, q.Jmax)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes, st, est,
           est_stride, ref, ref_stride, (const int2*)pl.rng, (const unsigned short*)pl.ana[r].pack, N, q.W, q.S, q.Jmax, pl.ysp, pl.ym, pl.cm);
    LAUNCH(mrstft::sums_kernel, dim3((q.Jmax + audio::kFramesPerWg - 1) / audio::kFramesPerWg, N), dim3(mrstft::kSumThreads), 0, st,
           (const int2*)pl.rng, q.W, q.S, q.Jmax, (const float*)pl.ym, (const float*)pl.cm, part, pstride);
    if (g)
      LAUNCH(mrstft::synth_kernel, dim3(N, 2, mr_split(N, q.Jmax)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes, st,
             (const int2*)pl.rng, (const unsigned short*)pl.syn[r].pack, (const float*)pl.ysp, (const float*)pl.ym, (const float*)pl.cm,
             (const double*)part, pstride, scale / pl.P.K, q.W, q.S, q.Wp, q.Jmax, pl.frsc + q.off);
  }
  LAUNCH(mrstft::terms_kernel, dim3(N), dim3(64), 0, st, (const int2*)pl.rng, pl.P, (const double*)pl.part, pl.nslmax, out, out_stride, detail);
  if (g && gwidth > 0)
    LAUNCH(mrstft::gather_kernel, dim3((unsigned)((gwidth + 255) / 256), N), dim3(256), 0, st, (const int2*)pl.rng, pl.P,
           (const float*)pl.frsc, gwidth, gstride, g);
  return RCED_OK;
}

static int mr_stft_run(const float* est_dev, int est_stride, const float* ref_dev, int ref_stride, const int* lengths_dev, int N,
                       const rced_mr_args* mr, double inv_batch, double* terms_dev, float* grad_dev, int device, void* stream) {
  if (int rc = mr_check(mr)) return rc;
  if (N < 0 || est_stride < 0 || ref_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!(inv_batch > 0.0) || !std::isfinite(inv_batch)) return rced_fail(RCED_ERR_ARG, "inv_batch must be finite and > 0, got %g", inv_batch);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (N == 0) return RCED_OK;
  if (!terms_dev || !lengths_dev || (est_stride > 0 && !est_dev) || (ref_stride > 0 && !ref_dev)) return rced_fail(RCED_ERR_ARG, "null pointer");
  DeviceGuard g(device);
  std::lock_guard<std::mutex> lk(g_fr_mu);
  MrPlan pl;
  if (int rc = mr_packs(mr, device, grad_dev != nullptr, pl)) return rc;
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const int width = std::min(est_stride, ref_stride);
  mr_shape(mr, width, N, pl);
  Carve ws;
  mr_take(ws, pl, N, grad_dev != nullptr, 0);
  if (int rc = ws.bind(device, stream, g_mr_ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(mrstft::ranges_kernel, dim3((N + 255) / 256), dim3(256), 0, st, lengths_dev, N, width, pl.rng);
  return mr_run(pl, est_dev, est_stride, ref_dev, ref_stride, N, mr->w_mr * inv_batch, terms_dev, 2 + 3 * mr->n_res, 1, grad_dev, est_stride,
                est_stride, st);
}

int rced_wave_loss_mr_run(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                          const int* lengths_dev, int N, int T, int W, int S, int name, double w_sse, double w_si_sdr, int skip_edges,
                          double inv_batch, const rced_mr_args* mr, double* terms_dev, float* grad_dev, int accumulate, int device,
                          void* stream) {
  if (int rc = framing_check(W, S, name)) return rc;
  if (int rc = mr_check(mr)) return rc;
  if (int rc = wave_loss_args(mag_dev, phase_dev, clean_dev, clean_stride, lengths_dev, N, T, w_sse, w_si_sdr, skip_edges, inv_batch, terms_dev))
    return rc == kNothingToDo ? RCED_OK : rc;
  const int nblk = (T + audio::kFramesPerWg - 1) / audio::kFramesPerWg;
  if (nblk > 65535) return rced_fail(RCED_ERR_ARG, "T > 65535 * 64 frames per call");
  const bool grad = grad_dev && T > 0;
  DeviceGuard g(device);
  std::lock_guard<std::mutex> lk(g_fr_mu);
  FrPack ola, adj;
  MrPlan pl;
  for (int round = 0; round < 2; ++round) {   // (the second round finds, or rebuilds, what a dropping look-up of the first one lost)
    if (int rc = fr_pack(device, kFrOla, W, name, &ola)) return rc;
    if (int rc = fr_pack(device, kFrAdjoint, W, name, &adj)) return rc;
    if (int rc = mr_packs(mr, device, grad, pl)) return rc;
  }
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  const long long L = wloss::fr::row_stride(T, W, S);   // floats per row of y, u and g_mr: whole 16-byte groups
  const int slices = wloss::num_slices((int)L);
  float *y, *u, *Y;
  double *ws1, *ws2, *scal;
  int* frames;
  Carve ws;
  ws.take(&y, (size_t)N * L);
  ws.take(&u, (size_t)N * L);
  ws.take(&Y, (size_t)N * T * audio::kFrame);
  ws.take(&ws1, (size_t)N * slices * 2);
  ws.take(&ws2, (size_t)N * slices * 2);
  ws.take(&scal, (size_t)N * 4);
  ws.take(&frames, (size_t)N);
  if (int rc = ws.bind(device, stream, g_wave_mr_ws)) return rc;
  mr_shape(mr, std::min<long long>(L, clean_stride), N, pl);   // R lies below the clean row's end and below n_out <= L
  Carve ws2c;
  mr_take(ws2c, pl, N, grad, grad ? (size_t)N * L : 0);
  if (int rc = ws2c.bind(device, stream, g_wave_mr_ws2)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* w2 = ola.aux + audio::kFrame;
  LAUNCH(wloss::fr::counts_kernel, dim3((N + 255) / 256), dim3(256), 0, st, frames_dev, lengths_dev, N, T, W, S, frames);
  if (T > 0)
    LAUNCH(audio::fr::frames_fr_kernel, dim3(N, 2, nblk), dim3(audio::x6::kThreadsX), audio::fr::kFramesFrLdsBytes, st, mag_dev, phase_dev,
           (const int*)frames, (const unsigned short*)ola.pack, (const float*)ola.aux, T, W, Y);
  LAUNCH(audio::fr::rebuild_fr_kernel<true>, dim3(N), dim3(audio::x6::kThreadsX), 0, st, (const float*)Y, (const int*)frames, w2, T, W, S, L, y);
  LAUNCH(wloss::sums_kernel<0>, dim3(slices, N), dim3(wloss::kSumThreads), 0, st, (const float*)y, (int)L, clean_dev, clean_stride, lengths_dev,
         (const int*)frames, skip_edges, W, S, (const double*)nullptr, ws1, slices);
  LAUNCH(wloss::sums_kernel<1>, dim3(slices, N), dim3(wloss::kSumThreads), 0, st, (const float*)y, (int)L, clean_dev, clean_stride, lengths_dev,
         (const int*)frames, skip_edges, W, S, (const double*)ws1, ws2, slices);
  LAUNCH(wloss::terms_kernel, dim3(N), dim3(wloss::kSumThreads), 0, st, (const double*)ws1, (const double*)ws2, lengths_dev,
         (const int*)frames, clean_stride, skip_edges, W, S, slices, terms_dev, 5, scal);
  LAUNCH(mrstft::wave_ranges_kernel, dim3((N + 255) / 256), dim3(256), 0, st, lengths_dev, (const int*)frames, N, clean_stride, skip_edges, W, S,
         pl.rng);
  if (int rc = mr_run(pl, y, L, clean_dev, clean_stride, N, mr->w_mr * inv_batch, terms_dev + 3, 5, 0, grad ? pl.gmr : nullptr, L, L, st)) return rc;
  if (grad) {
    LAUNCH(wloss::fr::reverse_kernel<true>, dim3(N), dim3(audio::x6::kThreadsX), 0, st, (const float*)y, L, clean_dev, clean_stride, lengths_dev,
           (const int*)frames, skip_edges, W, S, (const double*)scal, 2.0 * w_sse * inv_batch, w_si_sdr * inv_batch, w2, (const float*)pl.gmr, u);
    if (accumulate)
      LAUNCH(wloss::fr::adjoint_kernel<true>, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes, st,
             (const float*)u, L, (const int*)frames, (const unsigned short*)adj.pack, phase_dev, T, W, S, grad_dev);
    else
      LAUNCH(wloss::fr::adjoint_kernel<false>, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes, st,
             (const float*)u, L, (const int*)frames, (const unsigned short*)adj.pack, phase_dev, T, W, S, grad_dev);
  }
  return RCED_OK;
}

extern "C" {

int rced_framing_check(int window, int stride, int window_name) { return framing_check(window, stride, window_name); }

int rced_istft_fr_check(int window, int stride, int window_name) {
  if (int rc = framing_check(window, stride, window_name)) return rc;
  return reference_rebuild_check(window_name);
}

int rced_stft_num_frames_fr(int length, int window, int stride) {
  if (framing_check(window, stride, RCED_WINDOW_HAMMING)) return -1;
  return length > 0 ? audio::fr::num_frames(length, window, stride) : 0;
}

int rced_stft_fr(const float* pcm_dev, const int* lengths_dev, int N, int L, int T, int window, int stride, int window_name, float* mag_dev,
                 float* phase_dev, int device, void* stream) {
  if (int rc = framing_check(window, stride, window_name)) return rc;
  if (int rc = audio_args(N, T, true, pcm_dev && mag_dev, 512, L)) return rc == kNothingToDo ? RCED_OK : rc;
  DeviceGuard g(device);
  std::lock_guard<std::mutex> lk(g_fr_mu);
  FrPack p;
  if (int rc = fr_pack(device, kFrStft, window, window_name, &p)) return rc;
  if (!g.ok) return rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", device);
  LAUNCH(audio::fr::stft_fr_kernel, dim3(N, 2, range_split(N, T)), dim3(audio::x6::kThreadsX), audio::fr::kStftFrLdsBytes,
         static_cast<hipStream_t>(stream), pcm_dev, lengths_dev, (const unsigned short*)p.pack, L, T, window, stride, mag_dev, phase_dev);
  return RCED_OK;
}

int rced_istft_fr(const float* mag_dev, const float* phase_dev, int N, int T, int nfft, int window, int stride, float* audio_dev, int device,
                  void* stream) {
  if (int rc = framing_check(window, stride, RCED_WINDOW_HAMMING)) return rc;
  if (int rc = audio_args(N, T, true, mag_dev && phase_dev && audio_dev, nfft)) return rc == kNothingToDo ? RCED_OK : rc;
  return rebuild_fr<false>(mag_dev, phase_dev, nullptr, N, T, nfft == 512 ? kFrRef512 : kFrRef256, window, stride, RCED_WINDOW_HAMMING, audio_dev,
                           device, stream);
}

int rced_istft_ola_fr(const float* mag_dev, const float* phase_dev, const int* frames_dev, int N, int T, int window, int stride, int window_name,
                      float* audio_dev, int device, void* stream) {
  if (int rc = framing_check(window, stride, window_name)) return rc;
  if (int rc = audio_args(N, T, false, audio_dev && (T == 0 || (mag_dev && phase_dev)))) return rc == kNothingToDo ? RCED_OK : rc;
  return rebuild_fr<true>(mag_dev, phase_dev, frames_dev, N, T, kFrOla, window, stride, window_name, audio_dev, device, stream);
}

int rced_mr_stft_check(const rced_mr_args* mr) { return mr_check(mr); }

int rced_mr_stft(const float* est_dev, int est_stride, const float* ref_dev, int ref_stride, const int* lengths_dev, int N,
                 const rced_mr_args* mr, double inv_batch, double* terms_dev, float* grad_dev, int device, void* stream) {
  return mr_stft_run(est_dev, est_stride, ref_dev, ref_stride, lengths_dev, N, mr, inv_batch, terms_dev, grad_dev, device, stream);
}

int rced_wave_loss_mr(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                      const int* lengths_dev, int N, int T, int window, int stride, int window_name, double w_sse, double w_si_sdr,
                      int skip_edges, double inv_batch, const rced_mr_args* mr, double* terms_dev, float* grad_dev, int device,
                      void* stream) {
  return rced_wave_loss_mr_run(mag_dev, phase_dev, frames_dev, clean_dev, clean_stride, lengths_dev, N, T, window, stride, window_name, w_sse,
                               w_si_sdr, skip_edges, inv_batch, mr, terms_dev, grad_dev, 0, device, stream);
}

int rced_wave_loss_fr(const float* mag_dev, const float* phase_dev, const int* frames_dev, const float* clean_dev, int clean_stride,
                      const int* lengths_dev, int N, int T, int window, int stride, int window_name, double w_sse, double w_si_sdr,
                      int skip_edges, double inv_batch, double* terms_dev, float* grad_dev, int device, void* stream) {
  return rced_wave_loss_fr_run(mag_dev, phase_dev, frames_dev, clean_dev, clean_stride, lengths_dev, N, T, window, stride, window_name, w_sse,
                               w_si_sdr, skip_edges, inv_batch, terms_dev, grad_dev, 0, device, stream);
}

}  // extern "C"
