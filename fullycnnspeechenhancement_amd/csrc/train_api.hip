// C ABI of the training step (include/rced.h, "training" section): host-side orchestration.
// Replaces FullyCNNTrainer.creat_graph + train_step (model_utils/trainer.py:156-192): forward with
// train-mode BatchNorm, loss = sum((target - pred)^2) / batch_size, backward, TF-form Adam, moving
// statistics update.  Here: the handle, TrainPass (the layer loops of every form of the step) and the C ABI.  The small
// kernels are in kernels_train.h, the MFMA ones in kernels_train_mfma.h, their launchers in train_mfma_dispatch.h and
// train_launch.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/rced.h"
#include "kernels_generic.h"
#include "kernels_train.h"
#include "rced_internal.h"
#include "rced_spec.h"
#include "train_launch.h"
#include "train_plan.h"

using namespace rced;

namespace {
constexpr int kReduceGrid = 512;
using rced::tmd::kPairGrid;
using rced::tmd::tm_packet_floats;
using rced::tmd::WgDet;
using namespace rced::train;   // bn_finish and its modes, step_epilogue, the exchange kernels
constexpr float kAdamB1 = 0.9f, kAdamB2 = 0.999f, kAdamEps = 1e-8f;   // tf.train.AdamOptimizer defaults
constexpr float kBnMomentum = 0.99f;                                  // tf.layers.batch_normalization default

struct LayerOff {   // float offsets into the variable blob
  size_t kernel, bias, gamma, beta, mmean, mvar;
  int cin, cout, cout4, cin4, K;
};
struct TrainPass;   // one run of the step's layer loops (below); the synchronised step keeps one open between its calls
}  // namespace

struct rced_trainer {
  int variant = 0, device = 0, batch_size = 1;
  // what sizes the persistent grids: the device's CUs and RCED_TRAIN_MAX_GRID=n (a test knob, read at create: no tile-walking
  // launcher gets more than n workgroups, so a small batch walks several tiles per workgroup; 0 = no cap), with the record of
  // what the last step's launchers used (rced_train_grid_stats)
  rced::tmd::GridSeen grid_seen{};
  rced::tmd::Cus cus{256, 0, &grid_seen};
  // The MFMA kernels stage channel pairs, so odd channel counts (R-CED V2: 15, 19, 21, 23, 25) are trained in an
  // even-padded internal layout: `inet` = the net with every hidden cout rounded up to even.  A phantom channel has
  // zero kernel / bias / gamma / beta, so it is 0 after conv, BatchNorm and ReLU, contributes nothing downstream,
  // receives zero gradients and is not trainable; variables cross the ABI in the reference's own (unpadded) layout.
  const NetSpec* net = nullptr;   // = &inet
  NetSpec inet{};
  size_t nvars = 0;               // floats in the internal blob
  size_t xvars = 0;               // floats in the external (reference) blob
  std::vector<int> x2i;           // external float index -> internal float index
  std::vector<LayerOff> off;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  unsigned char* trainable = nullptr;
  std::vector<float*> wf, wt, bias4, mu, rstd;   // per layer
  std::vector<float*> pk_fwd, pk_bwd;            // per layer: MFMA A-fragment packets (1xk layers with an MFMA kernel)
  // RCED_TRAIN_MFMA / FUSE_ACT / FUSE_DZ / FUSE_SUMS / FUSE_BWD / X6 (=0: direct-conv kernels only / materialise activations / dz by
  // bn_bwd_apply / sums of plain layers from bwd_route2 / separate wgrad and dgrad / every convolution on the fp32 MFMA), and what
  // they make of this net: which launcher runs where (train_plan.h).  Fixed at create.
  plan::TrainSwitches sw{true, true, true, true, true, true};
  plan::TrainPlan plan{};
  bool det = true;             // RCED_TRAIN_DET=0: weight gradients by fp32 atomics (the round-1 behaviour; not reproducible bit for bit)
  float* wpart = nullptr;      // per-wave slices of the wgrad kernels' partial sums (deterministic mode; tmd::WgDet)
  size_t wpart_floats = 0;
  int wg_error = 0;            // tmd::wg_launch could not grow wpart: the step fails instead of using atomics
  float* pk_first = nullptr;   // A fragments of the 8xk first layer (rebuilt every step)
  std::vector<float*> pk_fwd_x6;   // the forward packets of the layers that run in the three-part bf16 form (tmm::conv_x6_fwd)
  std::vector<float*> pk_bwd_x6;   // the dgrad packets of the fused backward kernels whose dgrad half runs in that form (tmm::bwd_x6)
  float* pk_fin = nullptr, *pk_fin_bwd = nullptr;     // Toeplitz A fragments of the 1x129 output layer (rebuilt every step)
  float* zero32 = nullptr;
  double *part = nullptr, *sums = nullptr;
  int* tiny_host = nullptr;    // [layers] pinned, host-mapped: 1 = some |gamma| of the layer is below kTinyGamma (written by
  int* tiny_dev = nullptr;     // step_epilogue behind every Adam step, read by the host at the start of the next step)
  // activations for P pixels
  size_t cap_px = 0;
  std::vector<float*> out, z, G;   // out/G indexed by tensor id (0 unused), z by layer
  float* D = nullptr;
  long long global_step = 0;
  // every BatchNorm layer's (S1, S2) = (sum z, sum z^2) of the last forward ([layers][2 * kMaxC] doubles): what the moving
  // statistics are updated from behind Adam, and what a shard hands out.  The sharded step: x2i on the device, and where
  // the layers' sums go in the fp64 exchange buffer (tab.soff, xstats doubles)
  double* stash = nullptr;
  LayerTable tab{};
  int* x2i_dev = nullptr;
  size_t xstats = 0;
  // the synchronised step: the pass that rced_train_sync_begin opened and rced_train_sync_end / _abort has not closed yet
  std::unique_ptr<TrainPass> pending;
  // the wave objective (rced_train_step_wave / _grad_wave): the per-utterance terms [rows][3] of the last such pass, growing only
  double* wave_terms = nullptr;
  int wave_rows = 0;
  std::vector<void*> owned;       // every device allocation made by rced_train_create
  std::vector<void*> act_bases;   // the allocations behind out / z / G / D, made for a pixel count (ensure_acts)
  template <class T>
  hipError_t alloc(T** p, size_t bytes) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
    if (e == hipSuccess) owned.push_back(*p);
    return e;
  }
  void free_acts() {
    for (void* p : act_bases) (void)hipFree(p);
    act_bases.clear();
    out.clear(); z.clear(); G.clear();
    D = nullptr;
    cap_px = 0;
  }
  rced_trainer();    // (both below TrainPass: `pending` needs the complete type)
  ~rced_trainer();
};

namespace {

int ensure_acts(rced_trainer* t, size_t P) {
  if (P <= t->cap_px) return RCED_OK;
  HIP_TRY(hipDeviceSynchronize());
  t->free_acts();
  const NetSpec& net = *t->net;
  const int L = net.n_layers;
  t->out.assign(L + 1, nullptr);
  t->G.assign(L + 1, nullptr);
  t->z.assign(L, nullptr);
  int maxc = 1;
  // (Round 3 measured a different start offset inside its allocation for every tensor -- so that the tensors a kernel streams
  // in lockstep do not walk the same HBM channel sequence -- as run-to-run noise; the switch is gone.)
  auto alloc = [&](float** out_ptr, size_t bytes) -> int {
    void* base = nullptr;
    HIP_TRY(hipMalloc(&base, bytes));
    t->act_bases.push_back(base);
    *out_ptr = reinterpret_cast<float*>(base);
    return RCED_OK;
  };
  for (int l = 0; l < L; ++l) {
    const int c = net.layer[l].cout;
    maxc = std::max(maxc, c);
    if (int rc = alloc(&t->z[l], P * c * sizeof(float))) return rc;
    if (t->plan.layer[l].out == plan::Out::Stored) {
      if (int rc = alloc(&t->out[l + 1], P * c * sizeof(float))) return rc;
    } else   // virtual: rebuilt from z by its consumer (BnReluXform); a plain conv layer (decode_final): its output IS z
      t->out[l + 1] = t->plan.layer[l].out == plan::Out::Virtual ? nullptr : t->z[l];
    if (int rc = alloc(&t->G[l + 1], P * c * sizeof(float))) return rc;
  }
  if (int rc = alloc(&t->D, P * maxc * sizeof(float))) return rc;
  t->cap_px = P;
  return RCED_OK;
}

int launch_conv(const float* x, float* y, const float* w, const float* shift, const float* skip, int frames, int T, int F,
                int cin, int cout, int cout4, int kh, int kw, int pt, int pl, hipStream_t st) {
  const size_t row = (size_t)kh * (F + kw - 1) * cin * sizeof(float);
  if (row > 64 * 1024) return rced_fail(RCED_ERR_ARG, "layer needs %zu B of LDS", row);
  const int fpw = generic_frames_per_wg(F, cout4, kh, row);
  hipLaunchKernelGGL(conv_layer_generic, dim3((frames + fpw - 1) / fpw), dim3(kGenericThreads), row * fpw, st, x, y, w,
                     shift, skip, (const float*)nullptr, T, F, cin, cout, cout4, kh, kw, 0, pt, pl, fpw, frames);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

int reduce_channels(rced_trainer* t, const float* a, const float* b, const float* mu, const float* rstd, size_t P, int C,
                    double* sums, hipStream_t st) {
  hipLaunchKernelGGL(train::chan_reduce, dim3(kReduceGrid), dim3(train::kThreads), 0, st, a, b, mu, rstd, P, C, t->part);
  hipLaunchKernelGGL(train::reduce_finish, dim3(2 * C), dim3(train::kThreads), 0, st, (const double*)t->part, kReduceGrid, C, sums);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

}  // namespace

extern "C" {

int rced_train_create(int variant, const float* blob, size_t n_floats, int batch_size, int device, rced_trainer** out) {
  if (!out) return rced_fail(RCED_ERR_ARG, "out is NULL");
  *out = nullptr;
  const NetSpec* net = net_spec(variant);
  if (!net) return rced_fail(RCED_ERR_ARG, "unknown variant %d", variant);
  if (!blob || n_floats != net_num_weights(*net)) return rced_fail(RCED_ERR_ARG, "blob must hold %zu floats", net_num_weights(*net));
  if (batch_size <= 0) return rced_fail(RCED_ERR_ARG, "batch_size must be positive");
  OnDevice on(device);
  if (on.rc) return on.rc;
  std::unique_ptr<rced_trainer> owner(new rced_trainer());   // deleted on every early return below
  rced_trainer* t = owner.get();
  t->variant = variant;
  t->device = device;
  t->batch_size = batch_size;
  t->xvars = n_floats;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) t->cus.n = prop.multiProcessorCount;
    auto env = [](const char* name, bool* v) { if (const char* e = getenv(name)) *v = atoi(e) != 0; };
    env("RCED_TRAIN_MFMA", &t->sw.mfma);
    env("RCED_TRAIN_FUSE_ACT", &t->sw.fuse_act);
    env("RCED_TRAIN_FUSE_DZ", &t->sw.fuse_dz);
    env("RCED_TRAIN_FUSE_SUMS", &t->sw.fuse_sums);
    env("RCED_TRAIN_FUSE_BWD", &t->sw.fuse_bwd);
    env("RCED_TRAIN_X6", &t->sw.x6);
    env("RCED_TRAIN_DET", &t->det);
    if (const char* e = getenv("RCED_TRAIN_MAX_GRID")) t->cus.cap = std::max(0, atoi(e));
  }
  const NetSpec* xnet = net;     // the reference's layout (what crosses the ABI)
  t->inet = *xnet;
  const int L = xnet->n_layers;
  if (t->sw.mfma)
    for (int l = 0; l < L; ++l)
      if (xnet->layer[l].use_norm) t->inet.layer[l].cout = (xnet->layer[l].cout + 1) & ~1;
  t->net = net = &t->inet;
  size_t o = 0;
  t->off.resize(L);
  for (int l = 0; l < L; ++l) {
    const LayerSpec& s = net->layer[l];
    LayerOff& f = t->off[l];
    f.cin = layer_cin(*net, l);
    f.cout = s.cout;
    f.cout4 = (s.cout + 3) & ~3;
    f.cin4 = (f.cin + 3) & ~3;
    f.K = s.kh * s.kw * f.cin;
    f.kernel = o; o += (size_t)f.K * s.cout;
    f.bias = o; o += s.cout;
    if (s.use_norm) {
      f.gamma = o; o += s.cout;
      f.beta = o; o += s.cout;
      f.mmean = o; o += s.cout;
      f.mvar = o; o += s.cout;
    } else {
      f.gamma = f.beta = f.mmean = f.mvar = 0;
    }
  }
  t->nvars = o;
  // external -> internal index map (graph order: kernel [kh][kw][cin][cout], bias, gamma, beta, moving_mean, moving_variance),
  // the trainable mask and the internal start values (phantom entries: 0, moving_variance 1)
  std::vector<unsigned char> mask(t->nvars, 0);
  std::vector<float> start(t->nvars, 0.f);
  t->x2i.reserve(n_floats);
  for (int l = 0; l < L; ++l) {
    const LayerSpec& xs = xnet->layer[l];
    const LayerOff& f = t->off[l];
    const int xcin = layer_cin(*xnet, l), taps = xs.kh * xs.kw;
    for (int r = 0; r < taps; ++r)
      for (int ci = 0; ci < xcin; ++ci)
        for (int co = 0; co < xs.cout; ++co) {
          const size_t i = f.kernel + ((size_t)r * f.cin + ci) * f.cout + co;
          t->x2i.push_back((int)i);
          mask[i] = 1;
        }
    for (int co = 0; co < xs.cout; ++co) { t->x2i.push_back((int)(f.bias + co)); mask[f.bias + co] = 1; }
    if (xs.use_norm) {
      for (int co = 0; co < xs.cout; ++co) { t->x2i.push_back((int)(f.gamma + co)); mask[f.gamma + co] = 1; }
      for (int co = 0; co < xs.cout; ++co) { t->x2i.push_back((int)(f.beta + co)); mask[f.beta + co] = 1; }
      for (int co = 0; co < xs.cout; ++co) t->x2i.push_back((int)(f.mmean + co));
      for (int co = 0; co < xs.cout; ++co) t->x2i.push_back((int)(f.mvar + co));
      for (int co = 0; co < f.cout; ++co) start[f.mvar + co] = 1.f;
    }
  }
  if (t->x2i.size() != n_floats) return rced_fail(RCED_ERR_ARG, "blob layout: %zu floats mapped, %zu given", t->x2i.size(), n_floats);
  for (size_t e = 0; e < n_floats; ++e) start[t->x2i[e]] = blob[e];
  n_floats = t->nvars;   // from here on: the internal blob
  blob = start.data();
  // which launcher runs where: decided here, once; a net the kernels that were built cannot train is refused now
  plan::LayerAvail avail[kMaxLayers];
  for (int l = 0; l < L; ++l) {
    const LayerSpec& s = net->layer[l];
    const LayerOff& f = t->off[l];
    const size_t wgrad_lds = ((size_t)s.kh * (kFeatureDim + s.kw - 1) * f.cin + (size_t)kFeatureDim * s.cout) * sizeof(float);
    avail[l] = plan::layer_avail(*net, l, f.K * s.cout <= train::kWgradMaxOut * train::kThreads && wgrad_lds <= 64 * 1024);
  }
  static_assert(plan::kPlanOk == RCED_OK && plan::kPlanErrArg == RCED_ERR_ARG && plan::kPlanErrState == RCED_ERR_STATE, "the planner's codes are the ABI's");
  {
    char why[160];
    if (int rc = plan::plan_train(*net, t->sw, avail, &t->plan, why, sizeof why)) return rced_fail(rc, "%s", why);
  }
  const size_t bytes = n_floats * sizeof(float);
  HIP_TRY(t->alloc(&t->params, bytes));
  HIP_TRY(t->alloc(&t->grads, bytes));
  HIP_TRY(t->alloc(&t->m, bytes));
  HIP_TRY(t->alloc(&t->v, bytes));
  HIP_TRY(t->alloc(&t->trainable, n_floats));
  HIP_TRY(hipMemcpy(t->params, blob, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(t->m, 0, bytes));
  HIP_TRY(hipMemset(t->v, 0, bytes));
  HIP_TRY(hipMemcpy(t->trainable, mask.data(), n_floats, hipMemcpyHostToDevice));
  HIP_TRY(t->alloc(&t->zero32, 64 * sizeof(float)));
  HIP_TRY(hipMemset(t->zero32, 0, 64 * sizeof(float)));
  HIP_TRY(t->alloc(&t->part, (size_t)std::max(kReduceGrid, kPairGrid) * train::kMaxC * 2 * sizeof(double)));
  HIP_TRY(t->alloc(&t->sums, train::kMaxC * 2 * sizeof(double)));
  // the per-layer table of the kernels behind Adam and of the sharded step, whose exchange layout is the reference's blob
  // order for the gradient and (S1, S2)[xcout] + P per BatchNorm layer
  for (int l = 0; l < kMaxLayers; ++l) {
    const bool bn = l < L && xnet->layer[l].use_norm;
    t->tab.gamma[l] = bn ? (int)t->off[l].gamma : 0;
    t->tab.mmean[l] = bn ? (int)t->off[l].mmean : 0;
    t->tab.mvar[l] = bn ? (int)t->off[l].mvar : 0;
    t->tab.cout[l] = bn ? net->layer[l].cout : 0;
    t->tab.xcout[l] = bn ? xnet->layer[l].cout : 0;
    t->tab.soff[l] = bn ? (int)t->xstats : -1;
    if (bn) t->xstats += 2 * (size_t)xnet->layer[l].cout + 1;
  }
  HIP_TRY(t->alloc(&t->x2i_dev, t->xvars * sizeof(int)));
  HIP_TRY(hipMemcpy(t->x2i_dev, t->x2i.data(), t->xvars * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(t->alloc(&t->stash, (size_t)kMaxLayers * 2 * train::kMaxC * sizeof(double)));
  HIP_TRY(hipMemset(t->stash, 0, (size_t)kMaxLayers * 2 * train::kMaxC * sizeof(double)));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->tiny_host), kMaxLayers * sizeof(int), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&t->tiny_dev), t->tiny_host, 0));
  for (int l = 0; l < kMaxLayers; ++l) {
    t->tiny_host[l] = 0;
    if (l < L && net->layer[l].use_norm)
      for (int c = 0; c < net->layer[l].cout; ++c)
        if (!(std::fabs(blob[t->off[l].gamma + c]) >= kTinyGamma)) t->tiny_host[l] = 1;    // (phantom channels: gamma 0)
  }
  t->wf.assign(L, nullptr); t->wt.assign(L, nullptr); t->bias4.assign(L, nullptr);
  t->mu.assign(L, nullptr); t->rstd.assign(L, nullptr);
  t->pk_fwd.assign(L, nullptr); t->pk_bwd.assign(L, nullptr); t->pk_fwd_x6.assign(L, nullptr); t->pk_bwd_x6.assign(L, nullptr);
  for (int l = 0; l < L; ++l) {
    const LayerSpec& s = net->layer[l];
    const LayerOff& f = t->off[l];
    HIP_TRY(t->alloc(&t->wf[l], (size_t)f.K * f.cout4 * sizeof(float)));
    HIP_TRY(t->alloc(&t->wt[l], (size_t)s.kh * s.kw * s.cout * f.cin4 * sizeof(float)));
    HIP_TRY(t->alloc(&t->bias4[l], 64 * sizeof(float)));
    HIP_TRY(t->alloc(&t->mu[l], 64 * sizeof(float)));
    HIP_TRY(t->alloc(&t->rstd[l], 64 * sizeof(float)));
    if (avail[l].first && !t->pk_first) HIP_TRY(t->alloc(&t->pk_first, first_packet_floats(s) * sizeof(float)));
    if (avail[l].output && !t->pk_fin_bwd) HIP_TRY(t->alloc(&t->pk_fin_bwd, fin_dgrad_pack_floats(f.cin) * sizeof(float)));
    if (avail[l].output && !t->pk_fin) HIP_TRY(t->alloc(&t->pk_fin, fin_pack_alloc_floats(f.cin) * sizeof(float)));
    if (avail[l].fwd) HIP_TRY(t->alloc(&t->pk_fwd[l], tm_packet_floats(f.cin, s.kw, s.cout) * sizeof(float)));
    if (t->sw.x6 && avail[l].fwd && avail[l].x6)
      HIP_TRY(t->alloc(&t->pk_fwd_x6[l], rced::tmd::tm_packet_x6_floats(f.cin, s.kw, s.cout) * sizeof(float)));
    if (avail[l].dgrad) HIP_TRY(t->alloc(&t->pk_bwd[l], tm_packet_floats(s.cout, s.kw, f.cin) * sizeof(float)));
    if (t->pk_bwd[l] && tmm::bwd_x6(f.cin, s.kw, s.cout))   // (compiled into the fused kernel of this shape: not a per-trainer switch)
      HIP_TRY(t->alloc(&t->pk_bwd_x6[l], rced::tmd::tm_packet_x6_floats(s.cout, s.kw, f.cin) * sizeof(float)));
  }
  *out = owner.release();
  return RCED_OK;
}

void rced_train_destroy(rced_trainer* t) { delete t; }

long long rced_train_global_step(rced_trainer* t) { return t ? t->global_step : -1; }

int rced_train_grid_stats(rced_trainer* t, int* max_grid, int* max_tiles_per_workgroup) {
  if (!t || !max_grid || !max_tiles_per_workgroup) return rced_fail(RCED_ERR_ARG, "rced_train_grid_stats: NULL argument");
  *max_grid = t->grid_seen.max_grid;
  *max_tiles_per_workgroup = t->grid_seen.max_walk;
  return RCED_OK;
}

namespace {
// What an entry point does first: `Enter in(t, "rced_train_..."); if (in.rc) return in.rc;`.  The trainer is not null; no
// synchronised pass is pending on it (between rced_train_sync_begin and rced_train_sync_end / _abort the handle's buffers
// belong to the open pass); its device is current until the scope ends.  rc0: an earlier refusal, handed on as it is.
int refuse_pending(const rced_trainer* t, const char* what) {
  if (!t->pending) return RCED_OK;
  return rced_fail(RCED_ERR_STATE, "%s: a synchronised pass is pending on this trainer (rced_train_sync_begin without "
                                   "rced_train_sync_end or rced_train_sync_abort)", what);
}
struct Enter {
  int rc;
  DeviceGuard g;
  Enter(const rced_trainer* t, const char* what, int rc0 = RCED_OK) : rc(rc0) {
    if (!rc && !t) rc = rced_fail(RCED_ERR_ARG, "trainer is NULL");
    if (!rc) rc = refuse_pending(t, what);
    if (rc) return;
    g.enter(t->device);
    if (!g.ok) rc = rced_fail(RCED_ERR_HIP, "hipSetDevice(%d) failed", t->device);
  }
};
// ... and in front of it where a batch comes in: x [N, T, 129, 1] and its second tensor (the target; rced_train_forward: where
// the prediction goes), decided before the handle is looked into
int check_batch(const rced_trainer* t, const float* x_dev, const float* second, int N, int T) {
  if (!t) return rced_fail(RCED_ERR_ARG, "trainer is NULL");
  if (N <= 0 || T <= 0) return rced_fail(RCED_ERR_ARG, "a shard must have N >= 1 and T >= 1 (got %d x %d)", N, T);
  if (!x_dev || !second) return rced_fail(RCED_ERR_ARG, "input or target is NULL");
  return RCED_OK;
}

// internal (even-padded) device array -> the reference's layout on the host, and back (phantom entries become 0)
int download_external(rced_trainer* t, const float* dev, float* host) {
  std::vector<float> tmp(t->nvars);
  HIP_TRY(hipMemcpy(tmp.data(), dev, t->nvars * sizeof(float), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < t->xvars; ++e) host[e] = tmp[t->x2i[e]];
  return RCED_OK;
}
int upload_external(rced_trainer* t, const float* host, float* dev) {
  std::vector<float> tmp(t->nvars, 0.f);
  for (size_t e = 0; e < t->xvars; ++e) tmp[t->x2i[e]] = host[e];
  HIP_TRY(hipMemcpy(dev, tmp.data(), t->nvars * sizeof(float), hipMemcpyHostToDevice));
  return RCED_OK;
}
}  // namespace

int rced_train_get_variables(rced_trainer* t, float* blob_host, size_t n_floats) {
  if (!t || !blob_host || n_floats != t->xvars) return rced_fail(RCED_ERR_ARG, "bad arguments");
  Enter in(t, "rced_train_get_variables");
  if (in.rc) return in.rc;
  return download_external(t, t->params, blob_host);
}

int rced_train_get_gradients(rced_trainer* t, float* blob_host, size_t n_floats) {
  if (!t || !blob_host || n_floats != t->xvars) return rced_fail(RCED_ERR_ARG, "bad arguments");
  Enter in(t, "rced_train_get_gradients");
  if (in.rc) return in.rc;
  return download_external(t, t->grads, blob_host);
}

int rced_train_get_state(rced_trainer* t, float* m_blob_host, float* v_blob_host, size_t n_floats, long long* global_step) {
  if (!t || !m_blob_host || !v_blob_host || n_floats != t->xvars) return rced_fail(RCED_ERR_ARG, "bad arguments");
  Enter in(t, "rced_train_get_state");
  if (in.rc) return in.rc;
  if (int rc = download_external(t, t->m, m_blob_host)) return rc;
  if (int rc = download_external(t, t->v, v_blob_host)) return rc;
  if (global_step) *global_step = t->global_step;
  return RCED_OK;
}

int rced_train_set_state(rced_trainer* t, const float* m_blob_host, const float* v_blob_host, size_t n_floats,
                         long long global_step) {
  if (!t || !m_blob_host || !v_blob_host || n_floats != t->xvars || global_step < 0)
    return rced_fail(RCED_ERR_ARG, "bad arguments");
  Enter in(t, "rced_train_set_state");
  if (in.rc) return in.rc;
  if (int rc = upload_external(t, m_blob_host, t->m)) return rc;
  if (int rc = upload_external(t, v_blob_host, t->v)) return rc;
  t->global_step = global_step;
  return RCED_OK;
}

}  // extern "C"

namespace {
// Adam (TF form, trainer.py:175-179) from t->grads, global_step += 1, and behind it the per-layer epilogue: the moving
// statistics from s -- the stash of this step's forward over P pixels, or (P = 0) an exchange buffer, which carries its
// own pixel counts -- and the tiny-gamma scan.
// global_step: the reference fetches it in the same sess.run as train_op (trainer.py:186-191); TF1 orders a read and an
// assign_add in one run only through control dependencies, and slim.learning.create_train_op makes train_op =
// (increment global_step, then return the loss), so the fetched value is unordered against the increment in principle.
// This library returns the POST-increment value, deterministically: after the first step train_step returns 1 and
// the loop's next learning rate is noam(1) (trainer.py:215, step = global_step + 1 = 2).  See DESIGN.md 3.5.
void optimizer_step(rced_trainer* t, float lr, const double* s, double P, hipStream_t st) {
  t->global_step += 1;
  const double tt = (double)t->global_step;
  const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)kAdamB2, tt)) / (1.0 - std::pow((double)kAdamB1, tt)));
  hipLaunchKernelGGL(train::adam_step, dim3((unsigned)((t->nvars + train::kThreads - 1) / train::kThreads)),
                     dim3(train::kThreads), 0, st, t->params, (const float*)t->grads, t->m, t->v,
                     (const unsigned char*)t->trainable, t->nvars, lr_t, kAdamB1, kAdamB2, kAdamEps);
  hipLaunchKernelGGL(step_epilogue, dim3(kMaxLayers), dim3(64), 0, st, t->params, t->tab, s, P == 0.0 ? 1 : 0, P, kBnMomentum,
                     t->tiny_dev);
}

// pred_dev != nullptr: forward only (rced_train_forward) -- batch-statistics BatchNorm, nothing is updated, the
// prediction is copied to pred_dev.  g_out != nullptr: one shard of the sharded step (rced_train_grad) -- forward, loss and
// backward as in the step, nothing is updated either; the gradient and every BatchNorm layer's (sum z, sum z^2, pixels) go
// into (or, accumulate, are added to) g_out / s_out.  Otherwise the full step.  In every form the forward leaves a BatchNorm
// layer's (sum z, sum z^2) in t->stash and touches no variable: the moving statistics are written behind Adam, from the
// stash (the step) or from the exchange buffer (rced_train_apply), so a pass that fails leaves the trainer as it was.
//
// The pass is a TrainPass: begin() packs the weights, advance() walks the forward and the backward loop, end() hands the
// result out.  Every bn_finish call site of the two loops is an EXCHANGE POINT, described by a FinishPoint.  The straight
// paths (the three forms above) finish it on the spot with one launch (point_straight).  The synchronised step (xs != nullptr)
// stops there instead: point_out reduces the records to the raw 2 C sums in xs, advance() returns, the caller replaces xs by
// the sum over all shards, and the next advance() finishes the layer from xs with the pixel count of all shards
// (point_finish) and goes on.  Both forms run the same per-layer pieces (fwd_conv / fwd_act, bwd_route / bwd_rest).
struct FinishPoint {
  int nparts = 0, C = 0, mode = kFinPlain;   // the records in t->part, the layer's channels, how bn_finish finishes them
  FinishArgs fa{};
  double* sums = nullptr;                    // where the finished sums go
};

struct TrainPass {
  enum class Stage { Fwd, FwdResume, Bwd, BwdResume, Done };
  rced_trainer* const t;
  const float* const x_dev;
  const float* const y_dev;
  float* const pred_dev;
  const int N, T;
  const float lr;
  const hipStream_t st;
  const bool forward_only, shard;
  const NetSpec& net;
  const plan::TrainPlan& plan;   // which launcher runs where, and who stores / accumulates / zeroes what: train_plan.h
  const int L, F, frames;
  const size_t P;              // this pass's pixels
  const double bnP;            // the pixels BatchNorm's statistics are over: P, or all shards' (the synchronised step)
  double* const xs;            // the synchronised step's exchange buffer (2 * train::kMaxC doubles, the caller's), or nullptr
  WgDet wd{};
  tmm::XformArgs xa_tmp{nullptr, nullptr, nullptr, nullptr};
  int tiny[kMaxLayers] = {};
  std::vector<int> src_parts;  // [l]: the records of layer l's BatchNorm-backward sums that its consumer's dgrad left in t->part (Sums::DgradZ / FusedX)
  std::vector<double> hp;      // the loss kernel's partial sums, on the host after end()'s synchronise
  const rced_wave_args* wave = nullptr;   // the wave objective's terms (rced.h), or nullptr: the spectral loss alone, today's pass
  const int* wave_fr = nullptr;           // (window, stride, window name) of the _fr entries: the wave terms through the general kernels
  const rced_mr_args* wave_mr = nullptr;  // the _mr entries: the multi-resolution STFT term next to them (then with wave_fr)
  std::vector<double> hw;      // [N][3], with wave_mr [N][5]: the wave terms per utterance, on the host after end()'s synchronise
  Stage stage = Stage::Fwd;
  int layer = 0;
  FinishPoint pt{};

  TrainPass(rced_trainer* t_, const float* x, const float* y, float* pred, int N_, int T_, float lr_, void* stream, bool shard_,
            double pixels_total, double* xs_)
      : t(t_), x_dev(x), y_dev(y), pred_dev(pred), N(N_), T(T_), lr(lr_), st(static_cast<hipStream_t>(stream)),
        forward_only(pred != nullptr), shard(shard_), net(*t_->net),
        plan(t_->plan), L(t_->net->n_layers), F(kFeatureDim), frames(N_ * T_), P((size_t)N_ * T_ * kFeatureDim),
        bnP(xs_ ? pixels_total : (double)((size_t)N_ * T_ * kFeatureDim)), xs(xs_) {}

  static dim3 blocks(size_t n) { return dim3((unsigned)std::min<size_t>((n + train::kThreads - 1) / train::kThreads, 65535)); }
  dim3 pair_grid(int C) const {   // channel-aligned kernels: rows = 256 / (C/2) pixels per workgroup pass
    const size_t rows = train::kThreads / (C / 2);
    return dim3((unsigned)std::min<size_t>((P + rows - 1) / rows, kPairGrid));
  }
  // a virtual tensor is read as its producer's z plus that layer's BatchNorm parameters (BnReluXform)
  const float* conv_in(int id) const { return id == 0 ? x_dev : (plan.virt(id) ? t->z[id - 1] : t->out[id]); }
  const tmm::XformArgs* xform_of(int id, tmm::XformArgs* xa) const {
    if (id <= 0 || !plan.virt(id)) return nullptr;
    const LayerOff& pf = t->off[id - 1];
    *xa = tmm::XformArgs{t->mu[id - 1], t->rstd[id - 1], t->params + pf.gamma, t->params + pf.beta};
    return xa;
  }
  const float* tensor(int id) const { return id < 0 ? nullptr : (id == 0 ? x_dev : t->out[id]); }
  static int no_kernel(int l, const char* what) { return rced_fail(RCED_ERR_STATE, "layer %d: the planned %s kernel was not built", l, what); }
  hipError_t zero_grad(int id) const { return hipMemsetAsync(t->G[id], 0, P * net.layer[id - 1].cout * sizeof(float), st); }

  // ---- the exchange point in its three forms
  void launch_finish(const double* part, int nparts, double* sums, int mode, const FinishArgs& fa) const {
    hipLaunchKernelGGL(bn_finish, dim3(1), dim3(1024), 0, st, part, nparts, pt.C, sums, mode, fa);
  }
  void point_straight() const { launch_finish(t->part, pt.nparts, pt.sums, pt.mode, pt.fa); }
  // The records reduced in bn_finish's order, raw, into xs.  Forward: also into the layer's stash (pt.sums), which
  // rced_train_apply's moving statistics come from (this shard's own sums, as in the per-shard mode).  Backward: d beta and d gamma of THIS
  // shard -- the mode's expressions are linear in the raw sums once mu and rstd are those of all shards, so the usual sum
  // of the shards' gradients makes them the batch's.
  void point_out() const {
    FinishArgs a{};
    int mode = kFinPlain;
    if (pt.mode != kFinStats) { a = pt.fa; mode = pt.mode; }
    a.raw_out = xs;
    launch_finish(t->part, pt.nparts, pt.sums, mode, a);
  }
  // xs holds the sum over all shards: finished as ONE record (0.0 + v = v) with the pass's pixel count bnP
  void point_finish() const {
    FinishArgs a = pt.fa;
    a.g_beta = a.g_gamma = nullptr;
    launch_finish(xs, 1, t->sums, pt.mode, a);
  }

  int begin() {
    if (int rc = ensure_acts(t, P)) return rc;
    if (t->det && !forward_only && !t->wpart) {
      // Sized BEFORE the forward for the most any wgrad launcher can ask for: slices = workgroups (CUs x at most 4 resident per
      // CU, or the cap on the grids) x 8 waves x 2 pixel parities, slice stride = the net's largest kernel + bias.  A failure to allocate is therefore
      // reported here, before this step has launched anything; growing inside tmd::wg_launch remains as a last resort (it
      // synchronises, and if it fails the step returns RCED_ERR_ALLOC below).
      size_t maxps = 0;
      for (int l = 0; l < L; ++l) {
        const LayerSpec& s = net.layer[l];
        const int cin = s.src == 0 ? 1 : (net.layer[s.src - 1].cout + 1) & ~1, cout = (s.cout + 1) & ~1;   // (R-CED V2: even-padded)
        maxps = std::max(maxps, (size_t)s.kh * s.kw * cin * cout + cout + 4);
      }
      const int max_wgs = t->cus.cap > 0 ? std::min(t->cus.n * 4, t->cus.cap) : t->cus.n * 4;
      t->wpart_floats = (size_t)max_wgs * 8 * 2 * maxps;
      HIP_TRY(hipMalloc(&t->wpart, t->wpart_floats * sizeof(float)));
    }
    // deterministic weight gradients: the wgrad launchers write slices into t->wpart; otherwise fp32 atomics
    t->wg_error = 0;
    t->grid_seen = {};
    wd = t->det ? WgDet{&t->wpart, &t->wpart_floats, &t->wg_error} : WgDet{};
    for (int l = 0; l < kMaxLayers; ++l) tiny[l] = t->tiny_host[l];     // as of the end of the previous step (it synchronised)
    src_parts.assign(L, 0);
    stage = Stage::Fwd;
    layer = 0;

    // ---- weights in the layouts the direct-convolution kernels want, and the MFMA kernels' packets
    for (int l = 0; l < L; ++l) {
      const LayerSpec& s = net.layer[l];
      const LayerOff& f = t->off[l];
      if (plan.layer[l].repack_fwd) {
        hipLaunchKernelGGL(train::repack_fwd, dim3((f.K * f.cout4 + 255) / 256), dim3(256), 0, st, t->params + f.kernel, f.K,
                           s.cout, f.cout4, t->wf[l]);
        hipLaunchKernelGGL(train::repack_fwd, dim3(1), dim3(64), 0, st, t->params + f.bias, 1, s.cout, f.cout4, t->bias4[l]);
      }
      if (plan.layer[l].repack_dgrad) {
        const int nt = s.kh * s.kw * s.cout * f.cin4;
        hipLaunchKernelGGL(train::repack_dgrad, dim3((nt + 255) / 256), dim3(256), 0, st, t->params + f.kernel, s.kh, s.kw,
                           f.cin, s.cout, f.cin4, t->wt[l]);
      }
    }
    for (int l = 0; l < L; ++l) {
      const LayerSpec& s = net.layer[l];
      const LayerOff& f = t->off[l];
      if (plan.layer[l].fwd == plan::Fwd::X6) {
        const int n = rced::tmd::tm_packet_x6_threads(f.cin, s.kw, s.cout);
        hipLaunchKernelGGL(tmm::pack_packet_x6, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)(t->params + f.kernel),
                           (const float*)(t->params + f.bias), s.kw, f.cin, s.cout, rced::tmd::tm_packet_parities(s.cout), t->pk_fwd_x6[l]);
      } else if (plan.layer[l].fwd == plan::Fwd::Mfma) {
        const int n = (int)tm_packet_floats(f.cin, s.kw, s.cout);
        hipLaunchKernelGGL(tmm::pack_packet, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)(t->params + f.kernel),
                           (const float*)(t->params + f.bias), s.kw, f.cin, s.cout, 0, rced::tmd::tm_packet_parities(s.cout),
                           t->pk_fwd[l]);
      }
      if (plan.layer[l].pack_dgrad && t->pk_bwd_x6[l]) {
        // the fused backward kernel of this shape runs its dgrad half in the three-part bf16 form: its packet in that form too
        // (the fp32 packet below stays: the separate dgrad kernel takes it when the fused one is not used)
        const int n = rced::tmd::tm_packet_x6_threads(s.cout, s.kw, f.cin);
        hipLaunchKernelGGL(tmm::pack_packet_x6, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)(t->params + f.kernel),
                           (const float*)nullptr, s.kw, s.cout, f.cin, rced::tmd::tm_packet_parities(f.cin), t->pk_bwd_x6[l], 1);
      }
      if (plan.layer[l].pack_dgrad) {
        const int n = (int)tm_packet_floats(s.cout, s.kw, f.cin);
        hipLaunchKernelGGL(tmm::pack_packet, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)(t->params + f.kernel),
                           (const float*)nullptr, s.kw, s.cout, f.cin, 1, rced::tmd::tm_packet_parities(f.cin), t->pk_bwd[l]);
      }
    }
    return RCED_OK;
  }

  // ---- forward (is_training=True), layer l up to its statistics: *have = the layer stops at an exchange point (pt)
  int fwd_conv(int l, bool* have) {
    const LayerSpec& s = net.layer[l];
    const LayerOff& f = t->off[l];
    const plan::LayerPlan& pl = plan.layer[l];
    const bool stats = s.use_norm != 0;
    *have = false;
    int stat_parts = 0;   // the (sum z, sum z^2) records the conv kernel left in t->part (Stats::Conv)
    switch (pl.fwd) {
      case plan::Fwd::X6:
        stat_parts = rced::tmd::tm_conv_x6(f.cin, s.kw, s.cout, stats, conv_in(s.src), t->pk_fwd_x6[l], t->z[l], frames, t->cus,
                                           t->part, xform_of(s.src, &xa_tmp), st);
        break;
      case plan::Fwd::Mfma:
        stat_parts = tm_conv(true, f.cin, s.kw, s.cout, false, stats, conv_in(s.src), t->pk_fwd[l], t->z[l], frames, t->cus, t->part,
                             xform_of(s.src, &xa_tmp), nullptr, st);
        break;
      case plan::Fwd::First:
        stat_parts = first_fwd(s, x_dev, t->params + f.kernel, t->params + f.bias, t->pk_first, t->z[l], frames, T, t->cus, stats,
                               t->part, st);
        break;
      case plan::Fwd::Output:
        stat_parts = fin_forward(f.cin, tensor(s.src), t->params + f.kernel, t->params + f.bias, t->pk_fin, t->z[l], frames, st, t->sw.x6);
        break;
      case plan::Fwd::Generic:
        if (int rc = launch_conv(tensor(s.src), t->z[l], t->wf[l], t->bias4[l], nullptr, frames, T, F, f.cin, s.cout, f.cout4, s.kh,
                                 s.kw, (s.kh - 1) / 2, (s.kw - 1) / 2, st))
          return rc;
        stat_parts = 1;
        break;
    }
    if (stat_parts <= 0) return no_kernel(l, "forward");
    double* const stash = t->stash + (size_t)l * 2 * train::kMaxC;   // the layer's (S1, S2) stay here: for step_epilogue, or a shard's exchange buffer
    if (pl.stats == plan::Stats::Conv) {
      pt = FinishPoint{};
      pt.nparts = stat_parts; pt.C = s.cout; pt.mode = kFinStats;
      FinishArgs& fa = pt.fa;
      fa.P = bnP; fa.eps = kBnEps;
      fa.mu_out = t->mu[l]; fa.rstd_out = t->rstd[l];
      pt.sums = stash;
      *have = true;
    } else if (pl.stats == plan::Stats::Reduce) {
      if (int rc = reduce_channels(t, t->z[l], t->z[l], nullptr, nullptr, P, s.cout, stash, st)) return rc;
      hipLaunchKernelGGL(train::bn_stats_finish, dim3(1), dim3(64), 0, st, (const double*)stash, (double)P, s.cout, kBnEps,
                         t->mu[l], t->rstd[l]);
    }
    return RCED_OK;
  }
  // ... and from its statistics on: BatchNorm, skips, ReLU
  void fwd_act(int l) {
    const LayerSpec& s = net.layer[l];
    const LayerOff& f = t->off[l];
    const plan::LayerPlan& pl = plan.layer[l];
    const size_t n = P * s.cout;
    if (pl.bn_act == plan::BnAct::Pair) {
      // a virtual post-ReLU skip source: rebuilt from its producer's z inside bn_act_fwd2
      tmm::XformArgs vs{nullptr, nullptr, nullptr, nullptr};
      if (pl.vskip) xform_of(s.skip_post, &vs);
      hipLaunchKernelGGL(train::bn_act_fwd2, pair_grid(s.cout), dim3(train::kThreads), 0, st, (const float2*)t->z[l],
                         s.use_norm ? (const float*)t->mu[l] : nullptr, (const float*)t->rstd[l],
                         (const float*)(t->params + f.gamma), (const float*)(t->params + f.beta),
                         (const float2*)tensor(s.skip_pre), (const float2*)(pl.vskip ? t->z[s.skip_post - 1] : tensor(s.skip_post)),
                         s.use_act, P, s.cout, (float2*)t->out[l + 1], pl.vskip ? vs.mu : nullptr, vs.rstd, vs.gamma, vs.beta);
    } else if (pl.bn_act == plan::BnAct::Scalar) {
      hipLaunchKernelGGL(train::bn_act_fwd, blocks(n), dim3(train::kThreads), 0, st, (const float*)t->z[l],
                         s.use_norm ? (const float*)t->mu[l] : nullptr, (const float*)t->rstd[l],
                         (const float*)(t->params + f.gamma), (const float*)(t->params + f.beta), tensor(s.skip_pre),
                         tensor(s.skip_post), s.use_act, n, s.cout, t->out[l + 1]);
    }
  }
  // ---- the forward's end: the prediction out (forward only), or the loss and what the backward starts from
  int fwd_end() {
    HIP_TRY(hipGetLastError());
    if (forward_only) {
      HIP_TRY(hipMemcpyAsync(pred_dev, t->out[L], P * sizeof(float), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
      return RCED_OK;
    }
    // ---- loss and its gradient (trainer.py:146-147,153); with a wave objective the spectral term at its weight, if it has one,
    // then the wave terms on the prediction, their gradient added to (or, without a spectral term, written as) G[L]
    const bool spectral = !wave || wave->w_spectral > 0.0;
    hp.assign(kReduceGrid, 0.0);
    if (spectral) {
      hipLaunchKernelGGL(train::loss_fwd_bwd, dim3(kReduceGrid), dim3(train::kThreads), 0, st, (const float*)t->out[L], y_dev,
                         P, (wave ? (float)wave->w_spectral : 1.f) / (float)t->batch_size, t->G[L], t->part);
      HIP_TRY(hipMemcpyAsync(hp.data(), t->part, kReduceGrid * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (wave && (wave->w_sse > 0.0 || wave->w_si_sdr > 0.0 || (wave_mr && wave_mr->w_mr > 0.0))) {
      if (t->wave_rows < N) {
        if (t->wave_terms) {
          HIP_TRY(hipStreamSynchronize(st));
          (void)hipFree(t->wave_terms);
          t->wave_terms = nullptr;
          t->wave_rows = 0;
        }
        HIP_TRY(hipMalloc(&t->wave_terms, (size_t)N * 5 * sizeof(double)));   // (3 columns, 5 with the multi-resolution term)
        t->wave_rows = N;
      }
      if (int rc = wave_mr ? rced_wave_loss_mr_run(t->out[L], wave->phase_dev, wave->frames_dev, wave->clean_dev, wave->clean_stride,
                                                   wave->lengths_dev, N, T, wave_fr[0], wave_fr[1], wave_fr[2], wave->w_sse, wave->w_si_sdr,
                                                   wave->skip_edges, 1.0 / (double)t->batch_size, wave_mr, t->wave_terms, t->G[L],
                                                   spectral ? 1 : 0, t->device, st)
               : wave_fr ? rced_wave_loss_fr_run(t->out[L], wave->phase_dev, wave->frames_dev, wave->clean_dev, wave->clean_stride,
                                                   wave->lengths_dev, N, T, wave_fr[0], wave_fr[1], wave_fr[2], wave->w_sse, wave->w_si_sdr,
                                                   wave->skip_edges, 1.0 / (double)t->batch_size, t->wave_terms, t->G[L], spectral ? 1 : 0,
                                                   t->device, st)
                           : rced_wave_loss_run(t->out[L], wave->phase_dev, wave->frames_dev, wave->clean_dev, wave->clean_stride,
                                                wave->lengths_dev, N, T, wave->w_sse, wave->w_si_sdr, wave->skip_edges,
                                                1.0 / (double)t->batch_size, t->wave_terms, t->G[L], spectral ? 1 : 0, t->device, st))
        return rc;
      hw.assign((size_t)N * (wave_mr ? 5 : 3), 0.0);
      HIP_TRY(hipMemcpyAsync(hw.data(), t->wave_terms, hw.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    // ---- backward.  G[id] collects d loss / d tensor id from every consumer (the conv reading it, skip adds); the plan says
    // which writer stores, which add, and which tensors are zeroed first.
    HIP_TRY(hipMemsetAsync(t->grads, 0, t->nvars * sizeof(float), st));
    for (int id = 1; id < L; ++id)
      if (plan.zero_first[id]) HIP_TRY(zero_grad(id));
    return RCED_OK;
  }

  // the exact sums of a tiny-gamma layer again from (g, z), see kTinyGamma: bwd_route2 without outputs; returns its records
  int tiny_recompute(int l) const {
    const LayerSpec& s = net.layer[l];
    const LayerOff& f = t->off[l];
    const dim3 grid = pair_grid(s.cout);
    hipLaunchKernelGGL(train::bwd_route2, grid, dim3(train::kThreads), 0, st, (const float2*)t->G[l + 1],
                       (const float2*)t->z[l], (const float*)(s.use_norm ? t->mu[l] : nullptr), (const float*)t->rstd[l],
                       (const float*)(t->params + f.gamma), (const float*)(t->params + f.beta), (const float2*)nullptr, s.use_act, P,
                       s.cout, (float2*)nullptr, (float2*)nullptr, (float2*)nullptr, t->part);
    return (int)grid.x;
  }

  // ---- backward, layer l up to its BatchNorm-backward sums: *have = the layer stops at an exchange point (pt)
  int bwd_route(int l, bool* have) {
    const LayerSpec& s = net.layer[l];
    const LayerOff& f = t->off[l];
    const plan::LayerPlan& pl = plan.layer[l];
    const size_t n = P * s.cout;
    const float* mu = s.use_norm ? t->mu[l] : nullptr;
    *have = false;
    pt = FinishPoint{};
    pt.C = s.cout; pt.sums = t->sums;
    FinishArgs& fb = pt.fa;
    fb.mu = mu; fb.rstd = t->rstd[l]; fb.gamma = t->params + f.gamma; fb.beta = t->params + f.beta;
    fb.g_beta = t->grads + f.beta; fb.g_gamma = t->grads + f.gamma;
    float* const g_pre = s.skip_pre > 0 ? t->G[s.skip_pre] : nullptr;
    float* const g_post = s.skip_post > 0 && !pl.skip_alias ? t->G[s.skip_post] : nullptr;
    if (pl.zero_before_skip) HIP_TRY(zero_grad(plan::skip_of(s)));
    if (pl.route == plan::Route::Pair) {
      const dim3 grid = pair_grid(s.cout);
      hipLaunchKernelGGL(train::bwd_route2, grid, dim3(train::kThreads), 0, st, (const float2*)t->G[l + 1],
                         (const float2*)t->z[l], mu, (const float*)t->rstd[l], (const float*)(t->params + f.gamma),
                         (const float*)(t->params + f.beta), (const float2*)tensor(s.skip_pre), s.use_act, P, s.cout,
                         (float2*)g_pre, (float2*)g_post, (float2*)(pl.lazy_mask ? nullptr : t->D),
                         s.use_norm ? t->part : (double*)nullptr, (const int*)nullptr, pl.skip_first ? 1 : 0);
      if (pl.sums == plan::Sums::Route2) {
        pt.nparts = (int)grid.x; pt.mode = kFinPlain;
        *have = true;
      }
    } else if (pl.route == plan::Route::Scalar) {
      hipLaunchKernelGGL(train::bwd_route, blocks(n), dim3(train::kThreads), 0, st, (const float*)t->G[l + 1],
                         (const float*)t->z[l], mu, (const float*)t->rstd[l], (const float*)(t->params + f.gamma),
                         (const float*)(t->params + f.beta), tensor(s.skip_pre), s.use_act, n, s.cout, g_pre, g_post, t->D);
      if (pl.sums == plan::Sums::RouteReduce) {
        if (int rc = reduce_channels(t, t->D, t->z[l], mu, t->rstd[l], P, s.cout, t->sums, st)) return rc;
        hipLaunchKernelGGL(sums_to_float, dim3(1), dim3(64), 0, st, (const double*)t->sums, s.cout, 0, t->grads + f.beta);
        hipLaunchKernelGGL(sums_to_float, dim3(1), dim3(64), 0, st, (const double*)t->sums, s.cout, 1, t->grads + f.gamma);
      }
    } else if (pl.sums == plan::Sums::DgradZ || pl.sums == plan::Sums::FusedX) {
      const bool from_x = pl.sums == plan::Sums::FusedX;   // (sum d_u, sum d_u * x) rather than (.., sum d_u * z)
      pt.nparts = src_parts[l]; pt.mode = from_x ? kFinX : kFinZ;
      *have = true;
      // |gamma| tiny somewhere in this layer (known on the host since the previous step's step_epilogue, and a matter of the
      // variables alone: every shard decides alike): the sums exactly, from (g, z), in place of the fused kernel's; see
      // kTinyGamma.  Never taken in a real training run.
      if (from_x && tiny[l] != 0) {
        pt.nparts = tiny_recompute(l); pt.mode = kFinPlain;
      }
    }
    return RCED_OK;
  }
  // ... and from its sums (t->sums, over bnP pixels) on: BatchNorm backward, wgrad, dgrad
  int bwd_rest(int l) {
    const LayerSpec& s = net.layer[l];
    const LayerOff& f = t->off[l];
    const plan::LayerPlan& pl = plan.layer[l];
    const size_t n = P * s.cout;
    const float* mu = s.use_norm ? t->mu[l] : nullptr;
    // BatchNorm backward: either applied in place on D (bn_bwd_apply*), or (fuse_dz) folded into the staging of the wgrad and
    // dgrad kernels, which read (d_u, z) and never materialise dz (tile_commit_bnbwd).  With lazy_mask d_u is not materialised
    // either: the consumers read the incoming gradient g and apply the ReLU mask themselves.  passthrough: d_u IS g.
    const float* dsrc = pl.lazy_mask || pl.passthrough ? t->G[l + 1] : t->D;      // what wgrad / dgrad read as their "dz" input
    const tmm::BnBwdArgs ba_l{t->z[l], mu, t->rstd[l], t->params + f.gamma, t->sums, bnP,
                              pl.lazy_mask ? t->params + f.beta : nullptr};
    const tmm::BnBwdArgs* ba = pl.fuse_dz ? &ba_l : nullptr;
    if (s.use_norm && !pl.fuse_dz) {
      if (s.cout % 2 == 0)
        hipLaunchKernelGGL(train::bn_bwd_apply2, pair_grid(s.cout), dim3(train::kThreads), 0, st, (float2*)t->D,
                           (const float2*)t->z[l], mu, (const float*)t->rstd[l], (const float*)(t->params + f.gamma),
                           (const double*)t->sums, bnP, P, s.cout);
      else
        hipLaunchKernelGGL(train::bn_bwd_apply, blocks(n), dim3(train::kThreads), 0, st, t->D, (const float*)t->z[l], mu,
                           (const float*)t->rstd[l], (const float*)(t->params + f.gamma), (const double*)t->sums, bnP, n,
                           s.cout);
    }
    // dW and dbias = sum dz (the MFMA wgrad kernels produce both)
    int launched = 1;
    switch (pl.wgrad) {
      case plan::Wgrad::Fused:   // with the dgrad, below
        break;
      case plan::Wgrad::Mfma:
        launched = tm_wgrad(wd, f.cin, s.kw, s.cout, conv_in(s.src), dsrc, t->grads + f.kernel, t->grads + f.bias, frames, t->cus,
                            xform_of(s.src, &xa_tmp), ba, st);
        break;
      case plan::Wgrad::First:
        launched = first_wgrad(wd, s, x_dev, dsrc, t->grads + f.kernel, t->grads + f.bias, frames, T, t->cus, ba, st);
        break;
      case plan::Wgrad::Output:
        launched = fin_wgrad(wd, f.cin, tensor(s.src), dsrc, t->grads + f.kernel, t->grads + f.bias, frames, t->cus, st);
        break;
      case plan::Wgrad::Generic: {
        if (int rc = reduce_channels(t, t->D, t->D, nullptr, nullptr, P, s.cout, t->sums, st)) return rc;
        hipLaunchKernelGGL(sums_to_float, dim3(1), dim3(64), 0, st, (const double*)t->sums, s.cout, 0, t->grads + f.bias);
        const int fpw = 16;
        const size_t lds = ((size_t)s.kh * (F + s.kw - 1) * f.cin + (size_t)F * s.cout) * sizeof(float);
        hipLaunchKernelGGL(train::conv_wgrad, dim3((frames + fpw - 1) / fpw), dim3(train::kThreads), lds, st, tensor(s.src),
                           (const float*)t->D, T, F, f.cin, s.cout, s.kh, s.kw, frames, fpw, t->grads + f.kernel);
        break;
      }
    }
    if (launched == 0) return no_kernel(l, "wgrad");
    // dx into G[src], as a forward conv of dz with the flipped / transposed kernel and the other SAME half
    if (pl.zero_before_dgrad) HIP_TRY(zero_grad(s.src));
    const int pv = s.src - 1;      // the layer that produced this dgrad's output tensor
    const tmm::SumArgs sa_p = pl.src_sums ? tmm::SumArgs{t->z[pv], t->mu[pv], t->rstd[pv], t->params + t->off[pv].gamma, t->params + t->off[pv].beta}
                                          : rced::tmd::kNoSums;
    const float* acc_from = pl.acc_from > 0 ? t->G[pl.acc_from] : nullptr;
    int grid = 1;                  // the launcher's grid (= the records of layer pv's sums when src_sums), 0: no such kernel
    switch (pl.dgrad) {
      case plan::Dgrad::None:
        break;
      case plan::Dgrad::Fused:
        grid = tm_bwd_fused(wd, f.cin, s.kw, s.cout, pl.src_sums, conv_in(s.src), dsrc, t->pk_bwd_x6[l] ? t->pk_bwd_x6[l] : t->pk_bwd[l],
                            t->G[s.src], t->grads + f.kernel, t->grads + f.bias, frames, t->cus, t->part, xform_of(s.src, &xa_tmp), ba, st);
        break;
      case plan::Dgrad::Output:
        grid = fin_dgrad(f.cin, dsrc, t->params + f.kernel, t->pk_fin_bwd, t->G[s.src], frames, st, t->sw.x6);
        break;
      case plan::Dgrad::MfmaSums:
      case plan::Dgrad::MfmaAccSums:
        grid = tm_conv(false, s.cout, s.kw, f.cin, pl.accumulate, false, dsrc, t->pk_bwd[l], t->G[s.src], frames, t->cus, t->part,
                       nullptr, ba, st, &sa_p, acc_from);
        break;
      case plan::Dgrad::Mfma:
        grid = tm_conv(false, s.cout, s.kw, f.cin, pl.accumulate, false, dsrc, t->pk_bwd[l], t->G[s.src], frames, t->cus, nullptr,
                       nullptr, ba, st, nullptr, acc_from);
        break;
      case plan::Dgrad::Generic:
        if (int rc = launch_conv(t->D, t->G[s.src], t->wt[l], t->zero32, t->G[s.src], frames, T, F, s.cout, f.cin, f.cin4, s.kh, s.kw,
                                 (s.kh - 1) - (s.kh - 1) / 2, (s.kw - 1) - (s.kw - 1) / 2, st))
          return rc;
        break;
    }
    if (grid <= 0) return no_kernel(l, "dgrad");
    if (pl.src_sums) src_parts[pv] = grid;
    return RCED_OK;
  }

  // The two loops, to the end of the backward (the straight paths), or (xs) to the next exchange point: then the stage is
  // FwdResume / BwdResume, and the next call finishes that layer from xs and goes on.  done(): nothing is left to run.
  bool done() const { return stage == Stage::Done; }
  int advance() {
    while (stage != Stage::Done) {
      bool have = false;
      switch (stage) {
        case Stage::Fwd:
          if (layer == L) {
            if (int rc = fwd_end()) return rc;
            stage = forward_only ? Stage::Done : Stage::Bwd;
            layer = L - 1;
            break;
          }
          if (int rc = fwd_conv(layer, &have)) return rc;
          if (have && xs) {
            point_out();
            stage = Stage::FwdResume;
            return RCED_OK;
          }
          if (have) point_straight();
          fwd_act(layer++);
          break;
        case Stage::FwdResume:
          point_finish();
          fwd_act(layer++);
          stage = Stage::Fwd;
          break;
        case Stage::Bwd:
          if (layer < 0) {
            stage = Stage::Done;
            break;
          }
          if (int rc = bwd_route(layer, &have)) return rc;
          if (have && xs) {
            point_out();
            stage = Stage::BwdResume;
            return RCED_OK;
          }
          if (have) point_straight();
          if (int rc = bwd_rest(layer--)) return rc;
          break;
        case Stage::BwdResume:
          point_finish();
          stage = Stage::Bwd;
          if (int rc = bwd_rest(layer--)) return rc;
          break;
        case Stage::Done:
          break;
      }
    }
    return RCED_OK;
  }

  // g_out != nullptr (a shard): the gradient and every BatchNorm layer's (sum z, sum z^2, pixels) go into (or, accumulate,
  // are added to) g_out / s_out.  Otherwise Adam.  The one synchronise, and the loss.
  int end(float* g_out, double* s_out, int accumulate, double* loss_out, double* parts_out = nullptr) {
    if (forward_only) return RCED_OK;
    if (t->wg_error) {   // (cannot happen with the up-front size above unless the runtime reports > 4 workgroups per CU)
      (void)hipStreamSynchronize(st);   // nothing of this step is left in flight behind the error
      return rced_fail(RCED_ERR_ALLOC, "deterministic weight gradients: the per-wave slice buffer could not be grown; the step was "
                                       "abandoned before the optimizer ran: the variables, the moving statistics%s are as they were",
                       shard ? " and the exchange buffers" : " and the Adam slots");
    }
    if (shard) {
      hipLaunchKernelGGL(shard_grad_out, dim3((unsigned)((t->xvars + train::kThreads - 1) / train::kThreads)), dim3(train::kThreads), 0, st,
                         (const float*)t->grads, (const int*)t->x2i_dev, t->xvars, g_out, accumulate);
      hipLaunchKernelGGL(shard_stats_out, dim3(kMaxLayers), dim3(kShardThreads), 0, st, (const double*)t->stash, t->tab, (double)P, s_out,
                         accumulate);
    } else {
      optimizer_step(t, lr, t->stash, (double)P, st);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    double loss = 0.0;
    for (double v : hp) loss += v;
    if (!wave) {
      if (loss_out) *loss_out = loss / (double)t->batch_size;
      return RCED_OK;
    }
    double sse = 0.0, si = 0.0, mr = 0.0;   // in row order
    const size_t cols = wave_mr ? 5 : 3;
    for (int n = 0; n < (int)(hw.size() / cols); ++n) {
      sse += hw[(size_t)n * cols];
      if (hw[(size_t)n * cols + 2] != 0.0) si += hw[(size_t)n * cols + 1];
      if (wave_mr && hw[(size_t)n * cols + 4] != 0.0) mr += hw[(size_t)n * cols + 3];
    }
    if (loss_out) {
      if (wave_mr) *loss_out = (wave->w_spectral * loss + wave->w_sse * sse - wave->w_si_sdr * si + wave_mr->w_mr * mr) / (double)t->batch_size;
      else *loss_out = (wave->w_spectral * loss + wave->w_sse * sse - wave->w_si_sdr * si) / (double)t->batch_size;
    }
    if (parts_out && wave_mr) parts_out[3] = mr;
    if (parts_out) {
      parts_out[0] = loss;
      parts_out[1] = sse;
      parts_out[2] = si;
    }
    return RCED_OK;
  }
};

// what rced_train_step_wave / rced_train_grad_wave refuse in their struct, before any device work
// w_mr: the multi-resolution term's weight (checked by rced_mr_stft_check), 0 for the entries without one
int check_wave(const rced_wave_args* w, const float* y_dev, double w_mr = 0.0) {
  if (!w) return rced_fail(RCED_ERR_ARG, "the wave objective's arguments are NULL");
  const double ws[3] = {w->w_spectral, w->w_sse, w->w_si_sdr};
  for (double v : ws)
    if (!(v >= 0.0) || !std::isfinite(v))
      return rced_fail(RCED_ERR_ARG, "the objective's weights must be finite and >= 0, got %g, %g, %g", ws[0], ws[1], ws[2]);
  if (ws[0] == 0.0 && ws[1] == 0.0 && ws[2] == 0.0 && w_mr == 0.0) return rced_fail(RCED_ERR_ARG, "the objective's weights are all zero");
  if (w->skip_edges != 0 && w->skip_edges != 1) return rced_fail(RCED_ERR_ARG, "skip_edges must be 0 or 1, got %d", w->skip_edges);
  if (ws[0] > 0.0 && !y_dev) return rced_fail(RCED_ERR_ARG, "the target is NULL and the spectral term has a weight");
  if ((ws[1] > 0.0 || ws[2] > 0.0 || w_mr > 0.0) && (!w->phase_dev || !w->lengths_dev || w->clean_stride < 0 || (w->clean_stride > 0 && !w->clean_dev)))
    return rced_fail(RCED_ERR_ARG, "a wave term has a weight: it needs phase_dev, clean_dev (rows of clean_stride >= 0) and lengths_dev");
  return RCED_OK;
}

// args_rc: what the entry point made of its arguments (check_batch and its own)
int train_run(rced_trainer* t, const char* what, int args_rc, const float* x_dev, const float* y_dev, float* pred_dev, int N, int T,
              float lr, double* loss_out, void* stream, float* g_out = nullptr, double* s_out = nullptr, int accumulate = 0,
              const rced_wave_args* wave = nullptr, double* parts_out = nullptr, const int* wave_fr = nullptr,
              const rced_mr_args* wave_mr = nullptr) {
  Enter in(t, what, args_rc);
  if (in.rc) return in.rc;
  TrainPass pass(t, x_dev, y_dev, pred_dev, N, T, lr, stream, g_out != nullptr, 0.0, nullptr);
  pass.wave = wave;
  pass.wave_fr = wave_fr;
  pass.wave_mr = wave_mr;
  if (int rc = pass.begin()) return rc;
  if (int rc = pass.advance()) return rc;
  return pass.end(g_out, s_out, accumulate, loss_out, parts_out);
}

constexpr int kSyncDoubles = 2 * train::kMaxC;   // the exchange buffer of a synchronised pass: (S1, S2) of a layer's channels
}  // namespace

rced_trainer::rced_trainer() = default;
rced_trainer::~rced_trainer() {
  DeviceGuard g(device);
  pending.reset();
  for (void* p : owned) (void)hipFree(p);
  if (wpart) (void)hipFree(wpart);   // (made by the first step, regrown by tmd::wg_launch)
  if (wave_terms) (void)hipFree(wave_terms);
  if (tiny_host) (void)hipHostFree(tiny_host);
  free_acts();
}

extern "C" {

int rced_train_step(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr, double* loss_out,
                    void* stream) {
  return train_run(t, "rced_train_step", check_batch(t, x_dev, y_dev, N, T), x_dev, y_dev, nullptr, N, T, lr, loss_out, stream);
}

int rced_train_forward(rced_trainer* t, const float* x_dev, float* pred_dev, int N, int T, void* stream) {
  const int rc = pred_dev ? check_batch(t, x_dev, pred_dev, N, T) : rced_fail(RCED_ERR_ARG, "the prediction buffer is NULL");
  return train_run(t, "rced_train_forward", rc, x_dev, nullptr, pred_dev, N, T, 0.f, nullptr, stream);
}

int rced_train_exchange_size(rced_trainer* t, size_t* n_floats, size_t* n_doubles) {
  if (!t || !n_floats || !n_doubles) return rced_fail(RCED_ERR_ARG, "trainer or output pointer is NULL");
  *n_floats = t->xvars;
  *n_doubles = t->xstats;
  return RCED_OK;
}

int rced_train_grad(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                    int accumulate, double* loss_out, void* stream) {
  int rc = check_batch(t, x_dev, y_dev, N, T);
  if (!rc && (!g_dev || !s_dev)) rc = rced_fail(RCED_ERR_ARG, "an exchange buffer is NULL");
  return train_run(t, "rced_train_grad", rc, x_dev, y_dev, nullptr, N, T, 0.f, loss_out, stream, g_dev, s_dev, accumulate != 0);
}

// y_dev may be NULL when the spectral term has no weight: check_batch is then given x_dev in its place
int rced_train_step_wave(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr, const rced_wave_args* wave,
                         double* loss_out, double* parts_out, void* stream) {
  int rc = check_wave(wave, y_dev);
  if (!rc) rc = check_batch(t, x_dev, y_dev ? y_dev : x_dev, N, T);
  return train_run(t, "rced_train_step_wave", rc, x_dev, y_dev, nullptr, N, T, lr, loss_out, stream, nullptr, nullptr, 0, wave, parts_out);
}

int rced_train_grad_wave(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                         int accumulate, const rced_wave_args* wave, double* loss_out, double* parts_out, void* stream) {
  int rc = check_wave(wave, y_dev);
  if (!rc) rc = check_batch(t, x_dev, y_dev ? y_dev : x_dev, N, T);
  if (!rc && (!g_dev || !s_dev)) rc = rced_fail(RCED_ERR_ARG, "an exchange buffer is NULL");
  return train_run(t, "rced_train_grad_wave", rc, x_dev, y_dev, nullptr, N, T, 0.f, loss_out, stream, g_dev, s_dev, accumulate != 0, wave,
                   parts_out);
}

int rced_train_step_wave_fr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr, const rced_wave_args* wave,
                            int window, int stride, int window_name, double* loss_out, double* parts_out, void* stream) {
  const int fr[3] = {window, stride, window_name};
  int rc = rced_framing_check(window, stride, window_name);
  if (!rc) rc = check_wave(wave, y_dev);
  if (!rc) rc = check_batch(t, x_dev, y_dev ? y_dev : x_dev, N, T);
  return train_run(t, "rced_train_step_wave_fr", rc, x_dev, y_dev, nullptr, N, T, lr, loss_out, stream, nullptr, nullptr, 0, wave, parts_out, fr);
}

int rced_train_grad_wave_fr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                            int accumulate, const rced_wave_args* wave, int window, int stride, int window_name, double* loss_out,
                            double* parts_out, void* stream) {
  const int fr[3] = {window, stride, window_name};
  int rc = rced_framing_check(window, stride, window_name);
  if (!rc) rc = check_wave(wave, y_dev);
  if (!rc) rc = check_batch(t, x_dev, y_dev ? y_dev : x_dev, N, T);
  if (!rc && (!g_dev || !s_dev)) rc = rced_fail(RCED_ERR_ARG, "an exchange buffer is NULL");
  return train_run(t, "rced_train_grad_wave_fr", rc, x_dev, y_dev, nullptr, N, T, 0.f, loss_out, stream, g_dev, s_dev, accumulate != 0, wave,
                   parts_out, fr);
}

int rced_train_step_wave_mr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float lr, const rced_wave_args* wave,
                            int window, int stride, int window_name, const rced_mr_args* mr, double* loss_out, double* parts_out,
                            void* stream) {
  const int fr[3] = {window, stride, window_name};
  int rc = rced_framing_check(window, stride, window_name);
  if (!rc) rc = rced_mr_stft_check(mr);
  if (!rc) rc = check_wave(wave, y_dev, mr->w_mr);
  if (!rc) rc = check_batch(t, x_dev, y_dev ? y_dev : x_dev, N, T);
  return train_run(t, "rced_train_step_wave_mr", rc, x_dev, y_dev, nullptr, N, T, lr, loss_out, stream, nullptr, nullptr, 0, wave, parts_out, fr,
                   mr);
}

int rced_train_grad_wave_mr(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, float* g_dev, double* s_dev,
                            int accumulate, const rced_wave_args* wave, int window, int stride, int window_name, const rced_mr_args* mr,
                            double* loss_out, double* parts_out, void* stream) {
  const int fr[3] = {window, stride, window_name};
  int rc = rced_framing_check(window, stride, window_name);
  if (!rc) rc = rced_mr_stft_check(mr);
  if (!rc) rc = check_wave(wave, y_dev, mr->w_mr);
  if (!rc) rc = check_batch(t, x_dev, y_dev ? y_dev : x_dev, N, T);
  if (!rc && (!g_dev || !s_dev)) rc = rced_fail(RCED_ERR_ARG, "an exchange buffer is NULL");
  return train_run(t, "rced_train_grad_wave_mr", rc, x_dev, y_dev, nullptr, N, T, 0.f, loss_out, stream, g_dev, s_dev, accumulate != 0, wave,
                   parts_out, fr, mr);
}

int rced_train_apply(rced_trainer* t, const float* g_dev, const double* s_dev, float lr, void* stream) {
  if (!t) return rced_fail(RCED_ERR_ARG, "trainer is NULL");
  if (!g_dev || !s_dev) return rced_fail(RCED_ERR_ARG, "an exchange buffer is NULL");
  Enter in(t, "rced_train_apply");
  if (in.rc) return in.rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(t->grads, 0, t->nvars * sizeof(float), st));
  hipLaunchKernelGGL(shard_grad_in, dim3((unsigned)((t->xvars + train::kThreads - 1) / train::kThreads)), dim3(train::kThreads), 0, st,
                     g_dev, (const int*)t->x2i_dev, t->xvars, t->grads);
  optimizer_step(t, lr, s_dev, 0.0, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return RCED_OK;
}

// ---- the synchronised step: rced_train_grad as a pass that stops at every BatchNorm layer, in both directions ----
int rced_train_sync_points(rced_trainer* t, int* n_points, size_t* n_doubles) {
  if (!t || !n_points || !n_doubles) return rced_fail(RCED_ERR_ARG, "trainer or output pointer is NULL");
  int bn = 0;
  for (int l = 0; l < t->net->n_layers; ++l) bn += t->net->layer[l].use_norm != 0;
  *n_points = 2 * bn;
  *n_doubles = kSyncDoubles;
  return RCED_OK;
}

int rced_train_sync_begin(rced_trainer* t, const float* x_dev, const float* y_dev, int N, int T, double pixels_total,
                          double* xs_dev, void* stream) {
  if (int rc = check_batch(t, x_dev, y_dev, N, T)) return rc;
  if (!xs_dev) return rced_fail(RCED_ERR_ARG, "the exchange buffer is NULL");
  if (!(pixels_total >= (double)N * T * kFeatureDim))
    return rced_fail(RCED_ERR_ARG, "pixels_total = %g is less than this shard's own %g pixels", pixels_total, (double)N * T * kFeatureDim);
  Enter in(t, "rced_train_sync_begin");
  if (in.rc) return in.rc;
  for (int l = 0; l < t->net->n_layers; ++l) {   // every BatchNorm layer's sums must pass through bn_finish: the MFMA plans
    const plan::LayerPlan& pl = t->plan.layer[l];
    if (t->net->layer[l].use_norm && (pl.stats != plan::Stats::Conv || pl.sums == plan::Sums::RouteReduce || pl.sums == plan::Sums::None))
      return rced_fail(RCED_ERR_STATE, "layer %d: the synchronised step needs the layer's sums as records (the chan_reduce forms "
                                       "under RCED_TRAIN_MFMA=0 have no exchange point)", l);
  }
  std::unique_ptr<TrainPass> pass(new TrainPass(t, x_dev, y_dev, nullptr, N, T, 0.f, stream, true, pixels_total, xs_dev));
  if (int rc = pass->begin()) return rc;
  if (int rc = pass->advance()) {
    (void)hipStreamSynchronize(pass->st);
    return rc;
  }
  t->pending = std::move(pass);
  return RCED_OK;
}

int rced_train_sync_next(rced_trainer* t, int* more) {
  if (!t || !more) return rced_fail(RCED_ERR_ARG, "trainer or output pointer is NULL");
  *more = 0;
  if (!t->pending) return rced_fail(RCED_ERR_STATE, "rced_train_sync_next: no synchronised pass is pending on this trainer");
  ON_DEVICE(t->device);
  if (t->pending->done()) return RCED_OK;
  if (int rc = t->pending->advance()) {   // the pass is over: nothing of it stays in flight, the handle is free again
    (void)hipStreamSynchronize(t->pending->st);
    t->pending.reset();
    return rc;
  }
  *more = t->pending->done() ? 0 : 1;
  return RCED_OK;
}

int rced_train_sync_end(rced_trainer* t, float* g_dev, double* s_dev, double* loss_out, int accumulate) {
  if (!t) return rced_fail(RCED_ERR_ARG, "trainer is NULL");
  if (!g_dev || !s_dev) return rced_fail(RCED_ERR_ARG, "an exchange buffer is NULL");
  if (!t->pending) return rced_fail(RCED_ERR_STATE, "rced_train_sync_end: no synchronised pass is pending on this trainer");
  if (!t->pending->done())
    return rced_fail(RCED_ERR_STATE, "rced_train_sync_end: the pending pass has exchange points left (rced_train_sync_next until "
                                     "*more is 0, or rced_train_sync_abort)");
  ON_DEVICE(t->device);
  const std::unique_ptr<TrainPass> pass = std::move(t->pending);
  const int rc = pass->end(g_dev, s_dev, accumulate != 0, loss_out);
  if (rc) (void)hipStreamSynchronize(pass->st);
  return rc;
}

int rced_train_sync_abort(rced_trainer* t) {
  if (!t) return rced_fail(RCED_ERR_ARG, "trainer is NULL");
  if (!t->pending) return RCED_OK;
  DeviceGuard g(t->device);
  const std::unique_ptr<TrainPass> pass = std::move(t->pending);
  HIP_TRY(hipStreamSynchronize(pass->st));   // what the pass has launched reads the caller's batch
  return RCED_OK;
}

int rced_train_sync_reduce(rced_trainer* t, const double* gathered_dev, int shards, size_t stride, double* xs_dev, void* stream) {
  if (!t || !gathered_dev || !xs_dev) return rced_fail(RCED_ERR_ARG, "trainer or buffer is NULL");
  if (shards < 1 || stride < (size_t)kSyncDoubles)
    return rced_fail(RCED_ERR_ARG, "needs shards >= 1 and rows at least %d doubles apart (got %d, %zu)", kSyncDoubles, shards, stride);
  ON_DEVICE(t->device);
  hipLaunchKernelGGL(sync_reduce, dim3(1), dim3(kSyncDoubles), 0, static_cast<hipStream_t>(stream), gathered_dev, shards, stride,
                     kSyncDoubles, xs_dev);
  HIP_TRY(hipGetLastError());
  return RCED_OK;
}

int rced_train_copy_variables(rced_trainer* dst, rced_trainer* src, void* stream) {
  if (!dst || !src) return rced_fail(RCED_ERR_ARG, "trainer is NULL");
  if (dst == src) return RCED_OK;
  if (dst->variant != src->variant || dst->device != src->device || dst->nvars != src->nvars)
    return rced_fail(RCED_ERR_ARG, "the two trainers must be of one variant on one device");
  if (int rc = refuse_pending(src, "rced_train_copy_variables")) return rc;
  Enter in(dst, "rced_train_copy_variables");
  if (in.rc) return in.rc;
  HIP_TRY(hipMemcpyAsync(dst->params, src->params, src->nvars * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  // which layers take the exact recomputation is a matter of the variables: src's flags are those of its last step, which
  // synchronised
  for (int l = 0; l < kMaxLayers; ++l) dst->tiny_host[l] = src->tiny_host[l];
  return RCED_OK;
}

// module.py:11-34 with is_training=True, as ONE op on device pointers: z = conv(x) + bias; BatchNorm with the statistics of
// this batch (mean and biased variance over N*T*F, eps 1e-3 -- tf.layers.batch_normalization(training=True)); + skip; ReLU.
// The layerwise kernels of the training step (direct convolution, fp64 channel sums), not the MFMA path: a single op has
// no packed-weight state to keep between calls.
int rced_conv_bn_relu_train(const float* x, float* y, const float* kernel, const float* bias, const float* gamma_beta,
                            const float* skip_input, int use_act, int N, int T, int F, int cin, int cout, int kh, int kw,
                            float* batch_mean_var_out, int device, void* stream) {
  if (N < 0 || T < 0 || F <= 0 || cin <= 0 || cout <= 0 || cout > train::kThreads || kh <= 0 || kw <= 0)
    return rced_fail(RCED_ERR_ARG, "bad shape");
  if (N == 0 || T == 0) return RCED_OK;
  if (!x || !y || !kernel || !bias || !gamma_beta) return rced_fail(RCED_ERR_ARG, "null pointer");
  OnDevice on(device);
  if (on.rc) return on.rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int frames = N * T, K = kh * kw * cin, cout4 = (cout + 3) & ~3;
  const size_t P = (size_t)frames * F, n = P * cout;
  // one scratch allocation: z | repacked kernel | bias4 | mu | rstd | partial sums | sums
  const size_t fl = n + (size_t)K * cout4 + cout4 + 2 * (size_t)cout;
  const size_t dbl = (size_t)kReduceGrid * cout * 2 + 2 * (size_t)cout;
  float* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, ((fl + 1) & ~(size_t)1) * sizeof(float) + dbl * sizeof(double)));
  float *z = buf, *wf = z + n, *b4 = wf + (size_t)K * cout4, *mu = b4 + cout4, *rstd = mu + cout;
  double* part = reinterpret_cast<double*>(buf + ((fl + 1) & ~(size_t)1));
  double* sums = part + (size_t)kReduceGrid * cout * 2;
  int rc = RCED_OK;
  hipLaunchKernelGGL(train::repack_fwd, dim3((K * cout4 + 255) / 256), dim3(256), 0, st, kernel, K, cout, cout4, wf);
  hipLaunchKernelGGL(train::repack_fwd, dim3(1), dim3(256), 0, st, bias, 1, cout, cout4, b4);
  rc = launch_conv(x, z, wf, b4, nullptr, frames, T, F, cin, cout, cout4, kh, kw, (kh - 1) / 2, (kw - 1) / 2, st);
  if (rc == RCED_OK) {
    hipLaunchKernelGGL(train::chan_reduce, dim3(kReduceGrid), dim3(train::kThreads), 0, st, (const float*)z, (const float*)z,
                       (const float*)nullptr, (const float*)nullptr, P, cout, part);
    hipLaunchKernelGGL(train::reduce_finish, dim3(2 * cout), dim3(train::kThreads), 0, st, (const double*)part, kReduceGrid, cout, sums);
    hipLaunchKernelGGL(train::bn_stats_finish, dim3((cout + 63) / 64), dim3(64), 0, st, (const double*)sums, (double)P, cout, kBnEps,
                       mu, rstd);
    if (batch_mean_var_out)
      hipLaunchKernelGGL(train::batch_mean_var, dim3((cout + 63) / 64), dim3(64), 0, st, (const double*)sums, (double)P, cout,
                         batch_mean_var_out);
    auto blocks = dim3((unsigned)std::min<size_t>((n + train::kThreads - 1) / train::kThreads, 65535));
    hipLaunchKernelGGL(train::bn_act_fwd, blocks, dim3(train::kThreads), 0, st, (const float*)z, (const float*)mu, (const float*)rstd,
                       gamma_beta, gamma_beta + cout, skip_input, (const float*)nullptr, use_act, n, cout, y);
    if (hipGetLastError() != hipSuccess) rc = rced_fail(RCED_ERR_HIP, "single-op training launch failed");
  }
  (void)hipStreamSynchronize(st);
  (void)hipFree(buf);
  return rc;
}

}  // extern "C"
