// Stand-alone check of the training step's launch plan (csrc/train_plan.h): the three nets (R-CED V2 in its even-padded
// internal form) under all 64 combinations of the six plan switches.  Built and run by test_train_plan_host.py with the
// host compiler and AddressSanitizer and UBSan; exits non-zero if any property fails.
#include <cstdio>
#include <vector>

#include "../fullycnnspeechenhancement_amd/csrc/train_plan.h"

using namespace rced;
using namespace rced::plan;

static int g_fail = 0;
static char g_ctx[96];
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++g_fail;                                           \
      printf("FAIL %s: %s -- ", g_ctx, #cond);            \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
    }                                                     \
  } while (0)

static NetSpec internal_net(int variant, bool mfma) {   // as rced_train_create pads it
  NetSpec n = *net_spec(variant);
  for (int l = 0; l < n.n_layers && mfma; ++l)
    if (n.layer[l].use_norm) n.layer[l].cout = (n.layer[l].cout + 1) & ~1;
  return n;
}
static TrainSwitches switches(int bits) { return {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0}; }
enum { kMfma = 1, kFuseAct = 2, kFuseDz = 4, kFuseSums = 8, kFuseBwd = 16, kX6 = 32 };

static bool build(int variant, int bits, NetSpec* net, TrainPlan* p) {
  const TrainSwitches sw = switches(bits);
  *net = internal_net(variant, sw.mfma);
  LayerAvail av[kMaxLayers];
  for (int l = 0; l < net->n_layers; ++l) av[l] = layer_avail(*net, l, true);   // (the three nets fit train::conv_wgrad)
  char err[160] = "";
  const int rc = plan_train(*net, sw, av, p, err, sizeof err);
  CHECK(rc == kPlanOk, "plan_train -> %d: %s", rc, err);   // 1. the refusals are unreachable for the shipped nets
  return rc == kPlanOk;
}

struct Writer { int layer; bool store, zero_before; int acc_from; };
// the writers of G[id] in backward order: a layer's skip routing comes before its own dgrad
static std::vector<Writer> writers(const NetSpec& net, const TrainPlan& p, int id) {
  std::vector<Writer> w;
  for (int l = net.n_layers - 1; l >= 0; --l) {
    const LayerPlan& q = p.layer[l];
    if (skip_of(net.layer[l]) == id && q.route != Route::None && !q.skip_alias) w.push_back({l, q.skip_first, q.zero_before_skip, 0});
    if (net.layer[l].src == id) w.push_back({l, !q.accumulate, q.zero_before_dgrad, q.accumulate ? q.acc_from : 0});
  }
  return w;
}

static void check_plan(const NetSpec& net, const TrainSwitches& sw, const TrainPlan& p) {
  const int L = net.n_layers;
  CHECK(p.n_layers == L, "%d", p.n_layers);
  for (int l = 0; l < L; ++l) {
    const LayerSpec& s = net.layer[l];
    const LayerPlan& q = p.layer[l];
    const bool src_virt = p.virt(s.src);
    // 2. one kernel of each kind, and the one the layer's place in the net calls for: the first-layer and output-layer kernels
    // exactly there, the 1xk MFMA kernels in between, a dgrad exactly where there is an input gradient, fused wgrad and dgrad together
    const bool first = l == 0, last = l == L - 1;
    CHECK((q.fwd == Fwd::First) == (sw.mfma && first) && (q.fwd == Fwd::Output) == (sw.mfma && last), "layer %d forward kind %d", l, (int)q.fwd);
    CHECK((q.fwd == Fwd::X6 || q.fwd == Fwd::Mfma) == (sw.mfma && !first && !last) && (q.fwd != Fwd::X6 || sw.x6), "layer %d forward kind %d", l, (int)q.fwd);
    CHECK((q.wgrad == Wgrad::First) == (sw.mfma && first) && (q.wgrad == Wgrad::Output) == (sw.mfma && last), "layer %d wgrad kind %d", l, (int)q.wgrad);
    CHECK((q.wgrad == Wgrad::Mfma || q.wgrad == Wgrad::Fused) == (sw.mfma && !first && !last) && (q.wgrad != Wgrad::Fused || sw.fuse_bwd), "layer %d wgrad kind %d", l, (int)q.wgrad);
    CHECK((s.src > 0) == (q.dgrad != Dgrad::None) && (q.dgrad == Dgrad::Output) == (sw.mfma && last), "layer %d dgrad kind %d", l, (int)q.dgrad);
    CHECK((q.wgrad == Wgrad::Fused) == (q.dgrad == Dgrad::Fused), "layer %d", l);
    CHECK((q.dgrad == Dgrad::MfmaSums || q.dgrad == Dgrad::MfmaAccSums || (q.dgrad == Dgrad::Fused && q.src_sums)) == q.src_sums && (!q.src_sums || sw.fuse_sums), "layer %d", l);
    CHECK((q.dgrad == Dgrad::MfmaAccSums || q.dgrad == Dgrad::Generic) ? q.accumulate : (q.dgrad == Dgrad::Mfma || !q.accumulate), "layer %d", l);
    CHECK((q.bn_act != BnAct::None) == (q.out == Out::Stored) && (q.stats != Stats::None) == (s.use_norm != 0), "layer %d", l);
    // 3. a virtual tensor is read only by kinds that rebuild it
    if (src_virt) {
      CHECK(q.fwd == Fwd::X6 || q.fwd == Fwd::Mfma, "layer %d forward reads a virtual tensor", l);
      CHECK(q.wgrad == Wgrad::Mfma || q.wgrad == Wgrad::Fused, "layer %d wgrad reads a virtual tensor", l);
    }
    if (s.skip_pre > 0) CHECK(!p.virt(s.skip_pre), "layer %d adds a virtual tensor before its ReLU", l);
    if (p.virt(s.skip_post)) CHECK(q.bn_act == BnAct::Pair && q.vskip, "layer %d", l);
    if (q.vskip) CHECK(s.skip_post > 0 && p.virt(s.skip_post), "layer %d", l);
    if (!sw.mfma) {
      CHECK(!p.virt(l + 1) && q.fwd == Fwd::Generic && q.wgrad == Wgrad::Generic && (q.dgrad == Dgrad::Generic || q.dgrad == Dgrad::None), "layer %d", l);
      CHECK(!q.fuse_dz && !q.lazy_mask && !q.passthrough && !q.skip_alias, "layer %d", l);
    }
    // 4. dz rebuilt in staging: only kernels that do so read it
    if (q.fuse_dz) {
      CHECK(q.wgrad == Wgrad::Mfma || q.wgrad == Wgrad::Fused || q.wgrad == Wgrad::First, "layer %d wgrad", l);
      CHECK(q.dgrad != Dgrad::Generic && q.dgrad != Dgrad::Output, "layer %d dgrad", l);
    }
    if (q.lazy_mask) CHECK(q.fuse_dz, "layer %d", l);
    // 5. every BatchNorm layer has one sums source, and one that can know the whole gradient
    CHECK((s.use_norm != 0) == (q.sums != Sums::None), "layer %d", l);
    CHECK((q.sums == Sums::Route2) == (s.use_norm && q.route == Route::Pair) && (q.sums == Sums::RouteReduce) == (s.use_norm && q.route == Route::Scalar), "layer %d", l);
    int givers = 0;
    for (int c = 0; c < L; ++c)
      if (net.layer[c].src == l + 1 && p.layer[c].src_sums) {
        ++givers;
        const Dgrad d = p.layer[c].dgrad;
        CHECK(q.sums == (d == Dgrad::Fused ? Sums::FusedX : Sums::DgradZ), "layer %d <- %d", l, c);
        CHECK(d == Dgrad::Fused || d == Dgrad::MfmaSums || d == Dgrad::MfmaAccSums, "layer %d <- %d", l, c);
        const std::vector<Writer> w = writers(net, p, l + 1);
        CHECK(!w.empty() && w.back().layer == c, "layer %d: its sums come from layer %d, which is not the last writer of its gradient", l, c);
        CHECK(q.lazy_mask && q.route == Route::None, "layer %d", l);
      }
    CHECK(givers == ((q.sums == Sums::DgradZ || q.sums == Sums::FusedX) ? 1 : 0), "layer %d: %d dgrads leave its sums", l, givers);
    if (q.skip_alias) CHECK(s.skip_post > 0 && skip_of(s) == s.skip_post, "layer %d", l);
  }
  // 6. every gradient tensor: first writer stores or a memset precedes it, every later writer accumulates
  for (int id = 1; id < L; ++id) {
    const std::vector<Writer> w = writers(net, p, id);
    CHECK(!w.empty(), "G[%d] has no writer", id);
    int aliased_from = 0;
    for (int l = 0; l < L; ++l)
      if (p.layer[l].skip_alias && skip_of(net.layer[l]) == id) { CHECK(!aliased_from, "G[%d] aliased twice", id); aliased_from = l + 1; }
    bool have = p.zero_first[id];
    int reads_alias = 0;
    for (size_t k = 0; k < w.size(); ++k) {
      if (w[k].zero_before) { CHECK(!have, "G[%d]: layer %d zeroes what is already there", id, w[k].layer); have = true; }
      if (w[k].store) CHECK(!have, "G[%d]: layer %d stores over earlier contributions", id, w[k].layer);
      else if (w[k].acc_from > 0) { CHECK(!have, "G[%d]: layer %d", id, w[k].layer); ++reads_alias; CHECK(w[k].acc_from == aliased_from, "G[%d]", id); }
      else CHECK(have, "G[%d]: layer %d adds to a tensor nobody has written", id, w[k].layer);
      have = true;
      if (w[k].acc_from > 0) {   // the source is complete: all of its own writers came earlier in backward order
        for (const Writer& sw2 : writers(net, p, w[k].acc_from)) CHECK(sw2.layer > w[k].layer, "G[%d] is read by layer %d before layer %d wrote it", w[k].acc_from, w[k].layer, sw2.layer);
        CHECK(w[k].acc_from > id, "G[%d]", id);
      }
    }
    CHECK(reads_alias == (aliased_from ? 1 : 0), "G[%d]: aliased contribution read %d times", id, reads_alias);
  }
}

// 7. what a switch must not touch
static bool same_forward(const LayerPlan& a, const LayerPlan& b) {
  return a.fwd == b.fwd && a.stats == b.stats && a.out == b.out && a.bn_act == b.bn_act && a.vskip == b.vskip && a.repack_fwd == b.repack_fwd;
}
static bool same_dz(const LayerPlan& a, const LayerPlan& b) { return a.fuse_dz == b.fuse_dz && a.lazy_mask == b.lazy_mask && a.passthrough == b.passthrough; }
static bool same_backward(const LayerPlan& a, const LayerPlan& b) {
  return same_dz(a, b) && a.route == b.route && a.sums == b.sums && a.wgrad == b.wgrad && a.dgrad == b.dgrad && a.src_sums == b.src_sums &&
         a.accumulate == b.accumulate && a.acc_from == b.acc_from && a.zero_before_dgrad == b.zero_before_dgrad && a.zero_before_skip == b.zero_before_skip &&
         a.skip_first == b.skip_first && a.skip_alias == b.skip_alias && a.repack_dgrad == b.repack_dgrad && a.pack_dgrad == b.pack_dgrad;
}
static void check_independence(int variant, int bits, const NetSpec& net, const TrainPlan& p) {
  for (int sw = kFuseAct; sw <= kX6; sw <<= 1) {
    if (!(bits & sw)) continue;
    NetSpec net0;
    TrainPlan p0;
    if (!build(variant, bits & ~sw, &net0, &p0)) continue;
    for (int l = 0; l < net.n_layers; ++l) {
      const LayerPlan &a = p.layer[l], &b = p0.layer[l];
      const bool zeros = p.zero_first[l + 1] == p0.zero_first[l + 1];
      if (sw == kX6) {   // only forward kinds (the output layer's kernels take the switch at launch)
        CHECK(same_backward(a, b) && zeros && p.virt(l + 1) == p0.virt(l + 1) && a.stats == b.stats && a.bn_act == b.bn_act, "x6 changes layer %d", l);
        CHECK(a.fwd == b.fwd || (a.fwd == Fwd::X6 && b.fwd == Fwd::Mfma), "x6 changes layer %d", l);
      }
      if (sw == kFuseBwd || sw == kFuseSums) CHECK(same_forward(a, b) && same_dz(a, b) && zeros, "switch %d changes layer %d", sw, l);
      if (sw == kFuseBwd) CHECK(b.wgrad != Wgrad::Fused && (a.wgrad == b.wgrad || a.wgrad == Wgrad::Fused), "fuse_bwd changes layer %d", l);
      if (sw == kFuseSums) CHECK(b.sums != Sums::DgradZ && b.sums != Sums::FusedX && !b.src_sums, "fuse_sums = 0 leaves sums in a dgrad, layer %d", l);
      if (sw == kFuseDz) { CHECK(same_forward(a, b) && zeros, "fuse_dz changes layer %d", l); CHECK(!b.fuse_dz && !b.lazy_mask && !b.skip_alias, "layer %d", l); }
      if (sw == kFuseAct) { CHECK(same_dz(a, b) && zeros && a.fwd == b.fwd && a.stats == b.stats, "fuse_act changes layer %d", l); CHECK(!p0.virt(l + 1), "layer %d", l); }
    }
  }
}

int main() {
  int plans = 0, virt = 0, fused = 0, from_dgrad = 0, aliased = 0;
  for (int variant = 1; variant <= 3; ++variant)
    for (int bits = 0; bits < 64; ++bits) {
      snprintf(g_ctx, sizeof g_ctx, "V%d mfma=%d act=%d dz=%d sums=%d bwd=%d x6=%d", variant, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1,
               (bits >> 4) & 1, (bits >> 5) & 1);
      NetSpec net;
      TrainPlan p;
      if (!build(variant, bits, &net, &p)) continue;
      ++plans;
      check_plan(net, switches(bits), p);
      check_independence(variant, bits, net, p);
      if (bits == 63)
        for (int l = 0; l < net.n_layers; ++l) {
          virt += p.virt(l + 1);
          fused += p.layer[l].wgrad == Wgrad::Fused;
          from_dgrad += p.layer[l].sums == Sums::DgradZ || p.layer[l].sums == Sums::FusedX;
          aliased += p.layer[l].skip_alias;
        }
    }
  // the default plans do use what the properties above are about (a planner that fused nothing would pass them all)
  snprintf(g_ctx, sizeof g_ctx, "defaults");
  CHECK(virt > 0 && fused > 0 && from_dgrad > 0 && aliased > 0, "virt %d fused %d sums-from-dgrad %d aliased %d", virt, fused, from_dgrad, aliased);
  printf("%d plans, %d failures; defaults over the three nets: %d virtual tensors, %d fused backward layers, %d sums from a dgrad, %d aliased skips\n",
         plans, g_fail, virt, fused, from_dgrad, aliased);
  return g_fail || plans != 192 ? 1 : 0;
}
