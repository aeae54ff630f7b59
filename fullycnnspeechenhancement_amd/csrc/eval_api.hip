// C ABI of the evaluation loop's device pieces (include/rced.h, "evaluation" section): host side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/rced.h"
#include "host_ws.h"
#include "kernels_bsseval.h"
#include "kernels_conv.h"
#include "kernels_eval.h"
#include "kernels_sepm.h"
#include "kernels_stoi.h"
#include "rced_internal.h"

using namespace rced;

namespace {

// One buffer family (host_ws.h) per score, and one for the slice partials [N, slices, 2] double of rced_sdr and rced_mix_snr: none
// ever moves the buffer another entry's captured graph reads.
StreamWorkspace g_ws_slices, g_ws_stoi, g_ws_si_sdr, g_ws_seg_snr, g_ws_llr, g_ws_wss, g_ws_bss, g_ws_fwseg, g_ws_cepd;

// Two padded row matrices scored pair by pair, row n of `ref` against row n of `est`: what every score's entry takes first
struct Pairs {
  const float* ref;
  int ref_stride;
  const float* est;
  int est_stride, N;
  int cap() const { return ref_stride < est_stride ? ref_stride : est_stride; }   // the samples every row holds in both
};

// what every pair-scoring entry refuses; `outputs`: the results it was asked for have somewhere to go
int check_pairs(const Pairs& p, bool outputs, int max_len, const char* max_text) {
  if (p.N < 0 || p.ref_stride < 0 || p.est_stride < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!p.ref || !p.est || !outputs) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (p.N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (p.cap() > max_len) return rced_fail(RCED_ERR_ARG, "rows longer than %s samples", max_text);
  return RCED_OK;
}

// ---- STOI tables: built on the host once per process, uploaded once per device ---------------------------------------------------
struct StoiTables {
  double* tab = nullptr;             // resampler taps [0, 365), first window [368, 624)
  unsigned short* apack = nullptr;   // the windowed DFT matrix, three bf16 parts, MFMA fragment order
  bool built() const { return tab; }
  void release() {
    (void)hipFree(tab);
    (void)hipFree(apack);
  }
};
DeviceOnce<StoiTables> g_stoi;

double bessel_i0(double x) {         // power series: converges to the last bit in < 30 terms for x <= 6
  double s = 1.0, t = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 60; ++k) {
    t *= q / ((double)k * k);
    s += t;
    if (t < 1e-18 * s) break;
  }
  return s;
}

// np.hanning(258)[1:-1]
double stoi_window(int k) { return 0.5 - 0.5 * std::cos(2.0 * M_PI * (k + 1) / (stoi::kFrame + 1)); }

// 5 * h / sum(h), h = kaiser(365, 0.1102 (60 - 8.7)) * 2 p fc sinc(2 fc t), p = 5, fc = 1 / 10, t = -182 .. 182
std::vector<double> stoi_taps() {
  const int L = stoi::kTapHalf;
  const double beta = 0.1102 * (60.0 - 8.7), fc = 1.0 / 10.0;
  std::vector<double> h(stoi::kTaps);
  double sum = 0.0;
  for (int i = 0; i < stoi::kTaps; ++i) {
    const double t = i - L, a = t / L;
    const double kaiser = bessel_i0(beta * std::sqrt(1.0 - a * a)) / bessel_i0(beta);
    const double px = M_PI * 2.0 * fc * t;
    const double sinc = t == 0.0 ? 1.0 : std::sin(px) / px;
    h[i] = kaiser * (2.0 * 5.0 * fc * sinc);
    sum += h[i];
  }
  for (double& v : h) v = v / sum * 5.0;
  return h;
}

// row 4 q + {0, 1, 2, 3} = re, im of the first bin of pair slot q, re, im of its second (kernels_stoi.h); k = sample 0 .. 255
double stoi_coef(int row, int k) {
  const int q = row >> 2, second = (row >> 1) & 1, im = row & 1;
  if (q >= stoi::kSlots) return 0.0;
  int band = 0;
  while (stoi::band_slot(band + 1) <= q) ++band;
  const int bin = stoi::band_lo(band) + 2 * (q - stoi::band_slot(band)) + second;
  if (bin >= stoi::band_lo(band + 1)) return 0.0;
  const double th = 2.0 * M_PI * ((bin * k) % 512) / 512.0;
  return stoi_window(k) * (im ? -std::sin(th) : std::cos(th));
}

int stoi_tables(int device, StoiTables** out) {
  return g_stoi.get(device, 0, [](StoiTables& t) -> int {
    std::vector<double> tab(stoi::kTabLen, 0.0);
    const std::vector<double> taps = stoi_taps();
    std::copy(taps.begin(), taps.end(), tab.begin());
    for (int k = 0; k < stoi::kFrame; ++k) tab[stoi::kTabWin + k] = stoi_window(k);
    const std::vector<unsigned short> pack = x6dft::pack_x6(stoi::kMTiles, stoi_coef);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(stoi::band_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                stoi::kBandLdsBytes));
    if (int rc = upload(&t.tab, tab, "STOI tables")) return rc;
    return upload(&t.apack, pack, "STOI tables");
  }, out);
}

// ---- WSS tables: built on the host in fp64 once per process and rate, uploaded once per device -----------------------------------
struct WssTables {
  double* coef = nullptr;            // the DFT's cos / -sin columns in MFMA fragment order (sepm::wss_coef_len)
  double* filt = nullptr;            // [25][kBins] critical-band filters
  int* range = nullptr;              // [25][2]: a filter's nonzero bins [lo, hi)
  bool built() const { return coef; }
  void release() {
    for (void* p : {(void*)coef, (void*)filt, (void*)range}) (void)hipFree(p);
  }
};
DeviceOnce<WssTables, 2> g_wss;      // [device][fs == 16000]

const double kWssCentre[sepm::kBands] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,   540.0,   617.372,
                                         703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16,
                                         1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
const double kWssWidth[sepm::kBands] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    77.3724, 86.0056,
                                        95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776,
                                        217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

int sepm_dft_size(int W) {
  int nfft = 1;
  while (nfft < 2 * W) nfft *= 2;
  return nfft;
}

// The DFT's columns for bins bin0 .. bin0 + kBins - 1 as sepm::dft_gemm streams them: wave w, step s, tile q, part (cos, -sin),
// lane: B[k = 4 s + (lane >> 4)][bin = bin0 + 16 (4 w + q) + (lane & 15)]
std::vector<double> sepm_dft_stream(int W, int bin0) {
  const int S = W / 4, nfft = sepm_dft_size(W), nb = nfft / 2;
  std::vector<double> coef(sepm::wss_coef_len(W));
  size_t at = 0;
  for (int w = 0; w < sepm::kWaves; ++w)
    for (int s = 0; s < S; ++s)
      for (int q = 0; q < sepm::kBinTilesPerWave; ++q)
        for (int part = 0; part < 2; ++part)
          for (int lane = 0; lane < 64; ++lane) {
            const int k = 4 * s + (lane >> 4), bin = bin0 + 16 * (sepm::kBinTilesPerWave * w + q) + (lane & 15);
            const double th = 2.0 * M_PI * (double)(((long long)bin * k) % nfft) / (double)nfft;
            coef[at++] = bin < nb ? (part ? -std::sin(th) : std::cos(th)) : 0.0;
          }
  return coef;
}

int wss_tables(int device, int fs, WssTables** out) {
  return g_wss.get(device, fs == 16000, [fs](WssTables& t) -> int {
    const int W = eval::seg_window(fs), nb = sepm_dft_size(W) / 2;
    const double fmax = fs / 2.0;
    const std::vector<double> coef = sepm_dft_stream(W, 0);
    std::vector<double> filt((size_t)sepm::kBands * sepm::kBins, 0.0);
    std::vector<int> range(2 * sepm::kBands, 0);
    const double floor_g = std::exp(-30.0 / (2.0 * 2.303));
    for (int i = 0; i < sepm::kBands; ++i) {
      const double f0 = std::floor(kWssCentre[i] / fmax * nb), bw = kWssWidth[i] / fmax * nb;
      int lo = nb, hi = 0;
      for (int j = 0; j < nb; ++j) {
        const double r = (j - f0) / bw, g = std::exp(-11.0 * (r * r) + std::log(kWssWidth[0]) - std::log(kWssWidth[i]));
        if (!(g > floor_g)) continue;
        if (j >= sepm::kPowLd || j >= sepm::kBins) return rced_fail(RCED_ERR_STATE, "WSS filter %d reaches bin %d", i, j);
        filt[(size_t)i * sepm::kBins + j] = g;
        lo = j < lo ? j : lo;
        hi = j + 1;
      }
      range[2 * i] = lo < hi ? lo : 0;
      range[2 * i + 1] = hi;
    }
    if (int rc = upload(&t.coef, coef, "WSS tables")) return rc;
    if (int rc = upload(&t.filt, filt, "WSS tables")) return rc;
    return upload(&t.range, range, "WSS tables");
  }, out);
}

// ---- fwSNRseg: WSS's tables, and at 16 kHz the stream of the upper 256 bins, uploaded once per device -----------------------------
struct FwsegTables {
  const WssTables* wss = nullptr;
  double* coef_hi = nullptr;         // bins 256 .. 511 at 16 kHz; NULL at 8 kHz, whose 256 bins WSS's stream covers
  bool built() const { return wss; }
  void release() { (void)hipFree(coef_hi); }
};
DeviceOnce<FwsegTables, 2> g_fwseg;

int fwseg_tables(int device, int fs, FwsegTables** out) {
  WssTables* w = nullptr;
  if (int rc = wss_tables(device, fs, &w)) return rc;   // outside g_fwseg's lock
  return g_fwseg.get(device, fs == 16000, [fs, w](FwsegTables& t) -> int {
    const int W = eval::seg_window(fs), nb = sepm_dft_size(W) / 2;
    if (nb != (fs == 16000 ? 2 : 1) * sepm::kBins) return rced_fail(RCED_ERR_STATE, "fwSNRseg: %d bins at %d Hz", nb, fs);
    // the magnitudes of every bin stand in LDS: a little over 64 KB a workgroup
    if (fs == 16000) {
      constexpr auto kernel = sepm::fwseg_spectrum_kernel<1, 2>;
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sepm::fwseg_lds_bytes(W, 1, nb)));
      if (int rc = upload(&t.coef_hi, sepm_dft_stream(W, sepm::kBins), "fwSNRseg tables")) return rc;
    } else {
      constexpr auto kernel = sepm::fwseg_spectrum_kernel<2, 1>;
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sepm::fwseg_lds_bytes(W, 2, nb)));
    }
    t.wss = w;
    return RCED_OK;
  }, out);
}

// what rced_llr, rced_wss, rced_fwseg and rced_cepd check alike; *nfcap = the frames of the longest utterance the strides allow, at least 1
int sepm_args(const Pairs& p, int fs, const double* out_dev, const double* frames_out, int frames_stride, int* nfcap) {
  if (fs != 8000 && fs != 16000) return rced_fail(RCED_ERR_ARG, "sample_rate must be 8000 or 16000, got %d", fs);
  if (int rc = check_pairs(p, out_dev, eval::kMaxLen, "2^30")) return rc;
  const int most = eval::seg_frames(p.cap(), eval::seg_window(fs));
  if (frames_out && frames_stride < most)
    return rced_fail(RCED_ERR_ARG, "frames_stride %d < %d, the frames of an utterance as long as the rows", frames_stride, most);
  *nfcap = most > 0 ? most : 1;
  return RCED_OK;
}

// rank every frame value inside its utterance, then the mean of the lowest 95 %
int lowest_mean(const double* d, double* sorted, const int* lengths_dev, int N, int cap, int W, int nfcap, double* out_dev,
                int* nf_out, hipStream_t st) {
  LAUNCH(sepm::rank_kernel, dim3((nfcap + sepm::kThreads - 1) / sepm::kThreads, N), dim3(sepm::kThreads), 0, st, d, lengths_dev, cap, W,
         nfcap, sorted);
  LAUNCH(sepm::lowest_mean_kernel, dim3(N), dim3(sepm::kThreads), 0, st, (const double*)sorted, lengths_dev, cap, W, nfcap, out_dev,
         nf_out);
  return RCED_OK;
}

}  // namespace

extern "C" {

int rced_stoi_ex(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int fs_sig,
                 int which, double* stoi_dev, double* estoi_dev, int* detail_dev, int device, void* stream) {
  if (which <= 0 || (which & ~(RCED_STOI_CLASSIC | RCED_STOI_EXTENDED)))
    return rced_fail(RCED_ERR_ARG, "which must be RCED_STOI_CLASSIC, RCED_STOI_EXTENDED or both, got %d", which);
  const bool classic = which & RCED_STOI_CLASSIC, extended = which & RCED_STOI_EXTENDED;
  if (fs_sig != 8000 && fs_sig != stoi::kFs) return rced_fail(RCED_ERR_ARG, "fs_sig must be 8000 or 10000, got %d", fs_sig);
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  if (int rc = check_pairs(p, (!classic || stoi_dev) && (!extended || estoi_dev), stoi::kMaxLen, "2^28")) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  StoiTables* t = nullptr;
  if (int rc = stoi_tables(device, &t)) return rc;
  const int cap = p.cap(), l10 = stoi::len10k(cap, fs_sig);
  const int fcap = stoi::num_frames(l10) > 0 ? stoi::num_frames(l10) : 1;
  const int mcap = fcap > stoi::kSeg ? fcap - stoi::kSeg : 1;
  const int rstride = (l10 + 1) & ~1;
  // one layout whatever `which` asks for: a shape's size never depends on it
  double *r, *e, *tob, *dseg, *dseg_ext;
  int *kept, *cnt;
  Carve ws;
  ws.take(&r, (size_t)N * 2 * rstride);
  ws.take(&e, (size_t)N * fcap);
  ws.take(&tob, (size_t)N * 2 * fcap * 16);
  ws.take(&dseg, (size_t)N * mcap);          // classic
  ws.take(&dseg_ext, (size_t)N * mcap);      // extended
  ws.take(&kept, (size_t)N * fcap);
  ws.take(&cnt, (size_t)N * 4);
  if (int rc = ws.bind(device, stream, g_ws_stoi)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (l10 > 0)
    LAUNCH(stoi::resample_kernel, dim3((l10 + 255) / 256, 2, N), dim3(256), 0, st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev,
           cap, fs_sig, (const double*)t->tab, r, rstride);
  LAUNCH(stoi::energy_kernel, dim3((fcap + 3) / 4, N), dim3(256), 0, st, (const double*)r, rstride, lengths_dev, cap, fs_sig,
         (const double*)t->tab, e, fcap);
  LAUNCH(stoi::mask_kernel, dim3(N), dim3(64), 0, st, (const double*)e, lengths_dev, cap, fs_sig, fcap, kept, cnt);
  if (fcap - 1 >= stoi::kSeg) {
    LAUNCH(stoi::band_kernel, dim3((fcap - 1 + stoi::kBlockFrames - 1) / stoi::kBlockFrames, 2, N), dim3(stoi::kThreads),
           stoi::kBandLdsBytes, st, (const double*)r, rstride, (const int*)kept, (const int*)cnt, fcap, (const unsigned short*)t->apack,
           (const double*)t->tab, tob);
    if (classic)
      LAUNCH(stoi::segment_kernel, dim3((mcap + 15) / 16, N), dim3(256), 0, st, (const double*)tob, (const int*)cnt, fcap, mcap,
             1.0 + std::pow(10.0, 15.0 / 20.0), dseg);
    if (extended)
      LAUNCH(stoi::segment_ext_kernel, dim3((mcap + 15) / 16, N), dim3(256), 0, st, (const double*)tob, (const int*)cnt, fcap, mcap,
             dseg_ext);
  }
  if (classic)
    LAUNCH(stoi::final_kernel, dim3(N), dim3(256), 0, st, (const double*)dseg, (const int*)cnt, mcap, (double)stoi::kBands, stoi_dev,
           detail_dev);
  if (extended)
    LAUNCH(stoi::final_kernel, dim3(N), dim3(256), 0, st, (const double*)dseg_ext, (const int*)cnt, mcap, (double)stoi::kSeg, estoi_dev,
           classic ? nullptr : detail_dev);
  return RCED_OK;
}

int rced_stoi(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int fs_sig,
              double* stoi_dev, int* detail_dev, int device, void* stream) {
  return rced_stoi_ex(ref_dev, ref_stride, est_dev, est_stride, lengths_dev, N, fs_sig, RCED_STOI_CLASSIC, stoi_dev, nullptr, detail_dev,
                      device, stream);
}

int rced_si_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
                double* out_dev, double* parts_dev, int device, void* stream) {
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  if (int rc = check_pairs(p, out_dev, eval::kMaxLen, "2^30")) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int cap = p.cap(), slices = eval::num_slices(cap) > 0 ? eval::num_slices(cap) : 1;
  const size_t pass = (size_t)N * slices * 2;            // doubles per pass: [N, slices, 2]; the two passes lie back to back, unpadded
  double* ws1 = nullptr;
  if (int rc = g_ws_si_sdr.get(device, stream, 2 * pass * sizeof(double), &ws1)) return rc;
  double* ws2 = ws1 + pass;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(eval::si_sdr_dot_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev,
         cap, ws1, slices);
  LAUNCH(eval::si_sdr_energy_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride,
         lengths_dev, cap, (const double*)ws1, ws2, slices);
  LAUNCH(eval::si_sdr_final_kernel, dim3(N), dim3(eval::kThreads), 0, st, (const double*)ws1, (const double*)ws2, lengths_dev, cap,
         slices, out_dev, parts_dev);
  return RCED_OK;
}

int rced_seg_snr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int fs,
                 double* out_dev, int* frames_dev, int device, void* stream) {
  const int W = fs > 0 ? eval::seg_window(fs) : 0;
  if (W < eval::kSegMinW || W > eval::kSegMaxW)
    return rced_fail(RCED_ERR_ARG, "fs = %d gives frames of %d samples: outside [%d, %d]", fs, W, eval::kSegMinW, eval::kSegMaxW);
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  if (int rc = check_pairs(p, out_dev, eval::kMaxLen, "2^30")) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int cap = p.cap(), nfcap = eval::seg_frames(cap, W) > 0 ? eval::seg_frames(cap, W) : 1;
  const int blocks = (nfcap + eval::kSegFramesPerBlock - 1) / eval::kSegFramesPerBlock;
  double* snr = nullptr;
  if (int rc = g_ws_seg_snr.get(device, stream, (size_t)N * nfcap * sizeof(double), &snr)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(eval::seg_snr_frame_kernel, dim3(blocks, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride,
         lengths_dev, cap, W, snr, nfcap);
  LAUNCH(eval::seg_snr_mean_kernel, dim3(N), dim3(eval::kThreads), 0, st, (const double*)snr, lengths_dev, cap, W, nfcap, out_dev,
         frames_dev);
  return RCED_OK;
}

int rced_llr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int sample_rate,
             double limit, double* out_dev, double* frames_out, int frames_stride, int* nf_out, int device, void* stream) {
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  int nfcap = 0;
  if (int rc = sepm_args(p, sample_rate, out_dev, frames_out, frames_stride, &nfcap)) return rc;
  if (limit != limit) return rced_fail(RCED_ERR_ARG, "limit is nan");
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int cap = p.cap(), W = eval::seg_window(sample_rate), P = sepm::lpc_order(sample_rate);
  double *lags, *d, *sorted;
  Carve ws;
  ws.take(&lags, (size_t)N * nfcap * 2 * sepm::kMaxLags);
  ws.take(&d, (size_t)N * nfcap);
  ws.take(&sorted, (size_t)N * nfcap);
  if (int rc = ws.bind(device, stream, g_ws_llr)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(sepm::llr_frame_kernel, dim3((nfcap + sepm::kLlrFramesPerBlock - 1) / sepm::kLlrFramesPerBlock, N), dim3(sepm::kThreads), 0, st,
         ref_dev, ref_stride, est_dev, est_stride, lengths_dev, cap, W, P, lags, nfcap);
  const dim3 per_frame((nfcap + sepm::kThreads - 1) / sepm::kThreads, N);
  if (P == 10)
    LAUNCH(sepm::llr_recursion_kernel<10>, per_frame, dim3(sepm::kThreads), 0, st, (const double*)lags, lengths_dev, cap, W, nfcap, limit,
           d, frames_out, frames_stride);
  else
    LAUNCH(sepm::llr_recursion_kernel<16>, per_frame, dim3(sepm::kThreads), 0, st, (const double*)lags, lengths_dev, cap, W, nfcap, limit,
           d, frames_out, frames_stride);
  return lowest_mean(d, sorted, lengths_dev, N, cap, W, nfcap, out_dev, nf_out, st);
}

int rced_wss(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int sample_rate,
             double* out_dev, double* frames_out, int frames_stride, int* nf_out, int device, void* stream) {
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  int nfcap = 0;
  if (int rc = sepm_args(p, sample_rate, out_dev, frames_out, frames_stride, &nfcap)) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  WssTables* t = nullptr;
  if (int rc = wss_tables(device, sample_rate, &t)) return rc;
  const int cap = p.cap(), W = eval::seg_window(sample_rate);
  double *energy, *d, *sorted;
  Carve ws;
  ws.take(&energy, (size_t)N * 2 * nfcap * sepm::kBands);
  ws.take(&d, (size_t)N * nfcap);
  ws.take(&sorted, (size_t)N * nfcap);
  if (int rc = ws.bind(device, stream, g_ws_wss)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (W == sepm::kMaxW)           // 16 kHz: 16 frames of 480 samples fill the LDS; 8 kHz: 32 frames of 240
    LAUNCH(sepm::wss_spectrum_kernel<1>, dim3((nfcap + 15) / 16, 2, N), dim3(sepm::kThreads), sepm::wss_lds_bytes(W, 1), st, ref_dev,
           ref_stride, est_dev, est_stride, lengths_dev, cap, W, (const double*)t->coef, (const double*)t->filt, (const int*)t->range,
           energy, nfcap);
  else
    LAUNCH(sepm::wss_spectrum_kernel<2>, dim3((nfcap + 31) / 32, 2, N), dim3(sepm::kThreads), sepm::wss_lds_bytes(W, 2), st, ref_dev,
           ref_stride, est_dev, est_stride, lengths_dev, cap, W, (const double*)t->coef, (const double*)t->filt, (const int*)t->range,
           energy, nfcap);
  LAUNCH(sepm::wss_slope_kernel, dim3((nfcap + sepm::kThreads - 1) / sepm::kThreads, N), dim3(sepm::kThreads), 0, st,
         (const double*)energy, lengths_dev, cap, W, nfcap, d, frames_out, frames_stride);
  return lowest_mean(d, sorted, lengths_dev, N, cap, W, nfcap, out_dev, nf_out, st);
}

int rced_fwseg(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
               int sample_rate, double* out_dev, double* frames_out, int frames_stride, int* nf_out, int device, void* stream) {
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  int nfcap = 0;
  if (int rc = sepm_args(p, sample_rate, out_dev, frames_out, frames_stride, &nfcap)) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  FwsegTables* t = nullptr;
  if (int rc = fwseg_tables(device, sample_rate, &t)) return rc;
  const int cap = p.cap(), W = eval::seg_window(sample_rate);
  double *bands, *d;
  Carve ws;
  ws.take(&bands, (size_t)N * 2 * nfcap * sepm::kBands);
  ws.take(&d, (size_t)N * nfcap);
  if (int rc = ws.bind(device, stream, g_ws_fwseg)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr auto spectrum_16k = sepm::fwseg_spectrum_kernel<1, 2>;
  constexpr auto spectrum_8k = sepm::fwseg_spectrum_kernel<2, 1>;
  if (W == sepm::kMaxW)           // 16 kHz: 16 frames, 512 bins in two passes; 8 kHz: 32 frames, 256 bins in one
    LAUNCH(spectrum_16k, dim3((nfcap + 15) / 16, 2, N), dim3(sepm::kThreads),
           sepm::fwseg_lds_bytes(W, 1, 2 * sepm::kBins), st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev, cap, W,
           (const double*)t->wss->coef, (const double*)t->coef_hi, (const double*)t->wss->filt, (const int*)t->wss->range, bands, nfcap);
  else
    LAUNCH(spectrum_8k, dim3((nfcap + 31) / 32, 2, N), dim3(sepm::kThreads),
           sepm::fwseg_lds_bytes(W, 2, sepm::kBins), st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev, cap, W,
           (const double*)t->wss->coef, (const double*)t->coef_hi, (const double*)t->wss->filt, (const int*)t->wss->range, bands, nfcap);
  LAUNCH(sepm::fwseg_band_kernel, dim3((nfcap + sepm::kThreads - 1) / sepm::kThreads, N), dim3(sepm::kThreads), 0, st,
         (const double*)bands, lengths_dev, cap, W, nfcap, d, frames_out, frames_stride);
  LAUNCH(eval::seg_snr_mean_kernel, dim3(N), dim3(eval::kThreads), 0, st, (const double*)d, lengths_dev, cap, W, nfcap, out_dev, nf_out);
  return RCED_OK;
}

int rced_cepd(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N, int sample_rate,
              int order, double* out_dev, double* frames_out, int frames_stride, int* nf_out, int device, void* stream) {
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  int nfcap = 0;
  if (int rc = sepm_args(p, sample_rate, out_dev, frames_out, frames_stride, &nfcap)) return rc;
  if (order < 1 || order > sepm::kMaxOrder) return rced_fail(RCED_ERR_ARG, "order must lie in [1, %d], got %d", sepm::kMaxOrder, order);
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int cap = p.cap(), W = eval::seg_window(sample_rate);
  double *lags, *d, *sorted;
  Carve ws;
  ws.take(&lags, (size_t)N * nfcap * 2 * sepm::kMaxLags);
  ws.take(&d, (size_t)N * nfcap);
  ws.take(&sorted, (size_t)N * nfcap);
  if (int rc = ws.bind(device, stream, g_ws_cepd)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(sepm::llr_frame_kernel, dim3((nfcap + sepm::kLlrFramesPerBlock - 1) / sepm::kLlrFramesPerBlock, N), dim3(sepm::kThreads), 0, st,
         ref_dev, ref_stride, est_dev, est_stride, lengths_dev, cap, W, order, lags, nfcap);
  const dim3 per_frame((nfcap + sepm::kThreads - 1) / sepm::kThreads, N);
#define CEPD_ORDER(P)                                                                                                                  \
  case P:                                                                                                                              \
    LAUNCH(sepm::cepd_recursion_kernel<P>, per_frame, dim3(sepm::kThreads), 0, st, (const double*)lags, lengths_dev, cap, W, nfcap, d, \
           frames_out, frames_stride);                                                                                                 \
    break;
  switch (order) {
    CEPD_ORDER(1) CEPD_ORDER(2) CEPD_ORDER(3) CEPD_ORDER(4) CEPD_ORDER(5) CEPD_ORDER(6) CEPD_ORDER(7) CEPD_ORDER(8)
    CEPD_ORDER(9) CEPD_ORDER(10) CEPD_ORDER(11) CEPD_ORDER(12) CEPD_ORDER(13) CEPD_ORDER(14) CEPD_ORDER(15) CEPD_ORDER(16)
  }
#undef CEPD_ORDER
  return lowest_mean(d, sorted, lengths_dev, N, cap, W, nfcap, out_dev, nf_out, st);
}

int rced_bss_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
                 int filter_length, double* sdr_dev, double* filter_dev, double* energies_dev, int device, void* stream) {
  const int F = filter_length;
  if (F < 1 || F > bss::kMaxTaps) return rced_fail(RCED_ERR_ARG, "filter_length must lie in [1, %d], got %d", bss::kMaxTaps, F);
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  if (int rc = check_pairs(p, sdr_dev, eval::kMaxLen, "2^30")) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int cap = p.cap(), slices = bss::corr_slices(cap) > 0 ? bss::corr_slices(cap) : 1;
  const int pslices = bss::out_slices(cap, F) > 0 ? bss::out_slices(cap, F) : 1;
  double *part, *c, *pws;
  Carve ws;
  ws.take(&part, (size_t)N * 2 * slices * F);
  ws.take(&c, (size_t)N * F);
  ws.take(&pws, (size_t)N * pslices * 2);
  if (int rc = ws.bind(device, stream, g_ws_bss)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(bss::correlate_kernel, dim3(slices, 2, N), dim3(bss::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev,
         cap, F, part, slices);
  LAUNCH(bss::solve_kernel, dim3(N), dim3(64), 0, st, (const double*)part, lengths_dev, cap, F, slices, c, filter_dev);
  LAUNCH(bss::project_kernel, dim3(pslices, N), dim3(bss::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev, cap,
         F, (const double*)c, pws, pslices);
  LAUNCH(bss::final_kernel, dim3(N), dim3(64), 0, st, (const double*)pws, lengths_dev, cap, F, pslices, sdr_dev, energies_dev);
  return RCED_OK;
}

int rced_sdr(const float* ref_dev, int ref_stride, const float* est_dev, int est_stride, const int* lengths_dev, int N,
             double* sdr_dev, double* energies_dev, int device, void* stream) {
  const Pairs p{ref_dev, ref_stride, est_dev, est_stride, N};
  if (int rc = check_pairs(p, sdr_dev, eval::kMaxLen, "2^30")) return rc;
  if (N == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int cap = p.cap(), slices = eval::num_slices(cap) > 0 ? eval::num_slices(cap) : 1;
  double* ws = nullptr;
  if (int rc = g_ws_slices.get(device, stream, (size_t)N * slices * 2 * sizeof(double), &ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(eval::sdr_partial_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, ref_dev, ref_stride, est_dev, est_stride, lengths_dev,
         cap, ws, slices);
  LAUNCH(eval::sdr_final_kernel, dim3(N), dim3(64), 0, st, (const double*)ws, lengths_dev, cap, slices, sdr_dev, energies_dev);
  return RCED_OK;
}

int rced_mix_snr(const float* speech_dev, const int* speech_len_dev, int N, int Ls, const float* noise_dev,
                 const int* noise_len_dev, int Ln, const int* start_dev, const double* gains_dev, int n_gains, double snr_db,
                 float* mix_dev, int device, void* stream) {
  if (N < 0 || Ls < 0 || Ln < 0 || n_gains < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (!speech_dev || !noise_dev || !mix_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (n_gains > 0 && !gains_dev) return rced_fail(RCED_ERR_ARG, "n_gains = %d without gains", n_gains);
  if (n_gains > 31) return rced_fail(RCED_ERR_ARG, "n_gains > 31: a tile index has at most 31 bits");
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (Ls > eval::kMaxLen || Ln > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0 || Ls == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  const int slices = eval::num_slices(Ls);
  double* ws = nullptr;
  if (int rc = g_ws_slices.get(device, stream, (size_t)N * slices * 2 * sizeof(double), &ws)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(eval::mix_partial_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, speech_dev, speech_len_dev, Ls, noise_dev,
         noise_len_dev, Ln, start_dev, gains_dev, n_gains, ws, slices);
  LAUNCH(eval::mix_apply_kernel, dim3(slices, N), dim3(eval::kThreads), 0, st, speech_dev, speech_len_dev, Ls, noise_dev, noise_len_dev,
         Ln, start_dev, gains_dev, n_gains, (const double*)ws, slices, std::pow(10.0, snr_db / 10.0), mix_dev);
  return RCED_OK;
}

int rced_gather_pcm(const void* arena_dev, int arena_dtype, long long arena_samples, const long long* begin_dev, const int* count_dev,
                    int N, int L, float* rows_dev, int row_stride, int device, void* stream) {
  if (N < 0 || L < 0 || arena_samples < 0) return rced_fail(RCED_ERR_ARG, "negative shape");
  if (arena_dtype != RCED_PCM_S16 && arena_dtype != RCED_PCM_F32)
    return rced_fail(RCED_ERR_ARG, "arena_dtype must be RCED_PCM_S16 or RCED_PCM_F32, got %d", arena_dtype);
  if (row_stride < L) return rced_fail(RCED_ERR_ARG, "row_stride %d < L %d", row_stride, L);
  if (N > 65535) return rced_fail(RCED_ERR_ARG, "N > 65535 utterances per call");
  if (L > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "rows longer than 2^30 samples");
  if (N == 0 || L == 0) return RCED_OK;
  if (!begin_dev || !count_dev || !rows_dev) return rced_fail(RCED_ERR_ARG, "null pointer");
  if (!arena_dev && arena_samples > 0) return rced_fail(RCED_ERR_ARG, "null arena of %lld samples", arena_samples);
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(eval::num_slices(L), N), block(eval::kThreads);
  static_assert(eval::kSlice == eval::kThreads * eval::kGatherPerLane, "a column block of the gather is one slice");
  if (arena_dtype == RCED_PCM_F32)
    LAUNCH(eval::gather_pcm_kernel<true>, grid, block, 0, st, arena_dev, arena_samples, begin_dev, count_dev, L, rows_dev, row_stride);
  else
    LAUNCH(eval::gather_pcm_kernel<false>, grid, block, 0, st, arena_dev, arena_samples, begin_dev, count_dev, L, rows_dev, row_stride);
  return RCED_OK;
}

int rced_convolve(const float* x_dev, int x_stride, const int* x_len_dev, const float* h_dev, int h_stride, const int* h_len_dev,
                  const int* shift_dev, int N, int L, float* y_dev, int y_stride, int device, void* stream) {
  static_assert(conv::kMaxTaps == RCED_CONV_MAX_TAPS, "the header's bound is the kernel's");
  if (!x_dev) return rced_fail(RCED_ERR_ARG, "x_dev is a null pointer");
  if (!h_dev) return rced_fail(RCED_ERR_ARG, "h_dev is a null pointer");
  if (!y_dev) return rced_fail(RCED_ERR_ARG, "y_dev is a null pointer");
  if (x_stride < 0) return rced_fail(RCED_ERR_ARG, "x_stride %d is negative", x_stride);
  if (h_stride < 0) return rced_fail(RCED_ERR_ARG, "h_stride %d is negative", h_stride);
  if (y_stride < 0) return rced_fail(RCED_ERR_ARG, "y_stride %d is negative", y_stride);
  if (L < 0) return rced_fail(RCED_ERR_ARG, "L %d is negative", L);
  if (L > x_stride) return rced_fail(RCED_ERR_ARG, "L %d > x_stride %d", L, x_stride);
  if (L > y_stride) return rced_fail(RCED_ERR_ARG, "L %d > y_stride %d", L, y_stride);
  if (L > eval::kMaxLen) return rced_fail(RCED_ERR_ARG, "L: rows longer than 2^30 samples");
  if (!h_len_dev && h_stride > RCED_CONV_MAX_TAPS)
    return rced_fail(RCED_ERR_ARG, "h_stride %d > RCED_CONV_MAX_TAPS = %d taps without h_len_dev", h_stride, RCED_CONV_MAX_TAPS);
  if (N < 0 || N > 65535) return rced_fail(RCED_ERR_ARG, "N = %d outside [0, 65535] rows per call", N);
  if (N == 0 || L == 0) return RCED_OK;
  OnDevice on(device, kMaxDevices);
  if (on.rc) return on.rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LAUNCH(conv::convolve_kernel, dim3(conv::out_slices(L), N), dim3(conv::kThreads), 0, st, x_dev, x_stride, x_len_dev, h_dev, h_stride,
         h_len_dev, shift_dev, L, y_dev, y_stride);
  return RCED_OK;
}

}  // extern "C"
