// The training step's launch plan: which kernel every layer gets in the forward and the backward pass, which tensors are
// never materialised, where a layer's BatchNorm-backward sums come from, and who stores, accumulates or zeroes each gradient
// tensor.  All of it follows from (net, switches, which kernels were built), so rced_train_create computes it once with
// plan_train and refuses a net it cannot plan; the step (train_api.hip: train_run) only executes it.  Host-pure: no HIP.
#pragma once
#include <cstddef>
#include <cstdio>

#include "rced_spec.h"
#include "train_shapes.h"

namespace rced {
namespace plan {

struct TrainSwitches { bool mfma, fuse_act, fuse_dz, fuse_sums, fuse_bwd, x6; };   // RCED_TRAIN_<name>, default all on

// What exists for a layer's shape (the `has` predicates of train_shapes.h, and the direct wgrad kernel's size limit)
struct LayerAvail {
  bool fwd;      // 1xk MFMA forward + wgrad kernels of (cin, kw, cout)
  bool x6;       // ... and the forward in the three-part bf16 form
  bool dgrad;    // 1xk MFMA kernel of the dgrad shape (cout, kw, cin)
  bool fused;    // wgrad + dgrad in one kernel
  bool first;    // the 8 x kw first-layer kernels
  bool output;   // the 1x129 output-layer kernels
  bool direct_wgrad;   // train::conv_wgrad can take the shape
};
inline LayerAvail layer_avail(const NetSpec& net, int l, bool direct_wgrad) {
  const LayerSpec& s = net.layer[l];
  const int cin = layer_cin(net, l);
  const bool k1 = s.kh == 1;
  return {k1 && tms::tm_has(true, cin, s.kw, s.cout), k1 && tms::tm_x6_has(cin, s.kw, s.cout), k1 && tms::tm_has(false, s.cout, s.kw, cin),
          k1 && tms::tm_fused_has(cin, s.kw, s.cout), tms::first_has(s, cin), tms::is_output_layer(s, cin), direct_wgrad};
}

enum class Fwd { X6, Mfma, First, Output, Generic };      // conv_x6_fwd / conv1xk_mfma / first_fwd / the output-layer GEMM / conv_layer_generic
enum class Stats { None, Conv, Reduce };                  // (sum z, sum z^2): the conv kernel's records / chan_reduce over z
enum class Out { IsZ, Virtual, Stored };                  // the layer's output tensor: z itself / rebuilt by its consumers from z / written by bn_act
enum class BnAct { None, Pair, Scalar };                  // bn_act_fwd2 / bn_act_fwd
enum class Route { None, Pair, Scalar };                  // G[l+1] -> d_u and the skip's gradient: nothing to route / bwd_route2 / bwd_route
enum class Sums { None, Route2, RouteReduce, DgradZ, FusedX };   // BatchNorm-backward sums: bwd_route2's records / bwd_route + chan_reduce /
                                                                 // the records the consumer's dgrad (z tile) or fused backward kernel (x tile) left
enum class Wgrad { Fused, Mfma, First, Output, Generic };
enum class Dgrad { None, Fused, Output, MfmaSums, MfmaAccSums, Mfma, Generic };

struct LayerPlan {
  Fwd fwd; Stats stats; Out out; BnAct bn_act;
  bool vskip;          // bn_act rebuilds its (virtual) post-ReLU skip source from the producer's z
  bool fuse_dz;        // wgrad / dgrad rebuild dz from (d_u, z) in their staging: no bn_bwd_apply
  bool lazy_mask;      // ... and apply the ReLU mask to the incoming gradient themselves: d_u is not written either
  bool passthrough;    // d_u IS the incoming gradient (the linear output layer)
  Route route; Sums sums;
  Wgrad wgrad; Dgrad dgrad;
  bool src_sums;       // the dgrad (or fused kernel) also leaves the sums of layer src - 1
  bool accumulate;     // the dgrad adds to G[src] (to G[acc_from] when that is > 0) instead of storing
  int acc_from;
  bool zero_before_dgrad, zero_before_skip;   // a memset right before this writer (nobody has written the tensor yet)
  bool skip_first;     // this layer's routing pass stores the first contribution to G[skip_of(layer)]
  bool skip_alias;     // that tensor's first contribution is G[l + 1] unchanged: not copied, the completing dgrad reads it (acc_from)
  bool repack_fwd, repack_dgrad, pack_dgrad;   // per-step weight layouts: direct kernels' / the MFMA dgrad packet
};
struct TrainPlan {
  int n_layers;
  LayerPlan layer[kMaxLayers];
  bool zero_first[kMaxLayers + 1];  // G[id] is zeroed before the backward loop
  bool virt(int id) const { return id > 0 && layer[id - 1].out == Out::Virtual; }   // tensor id is never materialised
};
inline int skip_of(const LayerSpec& s) { return s.skip_pre > 0 ? s.skip_pre : s.skip_post > 0 ? s.skip_post : -1; }   // (a layer has at most one skip)

constexpr int kPlanOk = 0, kPlanErrArg = 1, kPlanErrState = 4;   // == RCED_OK, RCED_ERR_ARG, RCED_ERR_STATE

// `net`: the internal (even-padded) net.  Returns kPlanOk, or the code of the refusal with its text in err.
inline int plan_train(const NetSpec& net, const TrainSwitches& sw, const LayerAvail* av, TrainPlan* out, char* err, size_t errlen) {
  const int L = net.n_layers;
  TrainPlan& P = *out;
  P = TrainPlan{};
  P.n_layers = L;
  auto fail = [&](int code, const char* fmt, int l) { snprintf(err, errlen, fmt, l); return code; };
  auto cin_of = [&](int l) { return layer_cin(net, l); };

  // ---- tensors that need not exist in HBM: output of a plain conv+BN+ReLU layer (no skip in or out) whose only consumer is
  // a 1xk layer with MFMA forward and wgrad kernels
  int consumers[kMaxLayers + 1] = {}, conv_user[kMaxLayers + 1], n_conv[kMaxLayers + 1] = {};
  {
    int uses[kMaxLayers + 1] = {}, post_uses[kMaxLayers + 1] = {};
    for (int id = 0; id <= L; ++id) conv_user[id] = -1;
    for (int l = 0; l < L; ++l) {
      const LayerSpec& s = net.layer[l];
      if (s.src > 0) { ++uses[s.src]; ++consumers[s.src]; ++n_conv[s.src]; conv_user[s.src] = l; }
      if (s.skip_pre > 0) { uses[s.skip_pre] += 2; ++consumers[s.skip_pre]; }   // a skip added before the ReLU disqualifies (its backward reads the tensor)
      // a skip added AFTER a ReLU (CR-CED's block skips) is read once, by bn_act_fwd2, which rebuilds it from the
      // producer's z just as well (same bytes, same arithmetic); its backward needs no values
      if (s.skip_post > 0) {
        ++consumers[s.skip_post];
        if (s.cout % 2 == 0 && s.skip_pre < 0) ++post_uses[s.skip_post]; else uses[s.skip_post] += 2;
      }
    }
    for (int id = 1; id < L && sw.mfma && sw.fuse_act; ++id) {
      const LayerSpec& p = net.layer[id - 1];
      const int c = conv_user[id];
      if (uses[id] != 1 || c < 0 || post_uses[id] > 1) continue;
      const LayerSpec& q = net.layer[c];
      if (p.use_norm && p.use_act && p.skip_pre < 0 && p.skip_post < 0 && p.cout % 2 == 0 && q.kh == 1 && q.cout % 2 == 0 && av[c].fwd)
        P.layer[id - 1].out = Out::Virtual;
    }
  }
  auto src_virt = [&](int l) { return P.virt(net.layer[l].src); };

  // ---- forward
  for (int l = 0; l < L; ++l) {
    const LayerSpec& s = net.layer[l];
    LayerPlan& p = P.layer[l];
    if (sw.mfma && sw.x6 && av[l].fwd && av[l].x6) p.fwd = Fwd::X6;
    else if (sw.mfma && av[l].fwd && tms::tm_variant_has(true, cin_of(l), s.cout, false, s.use_norm != 0, src_virt(l), false, false)) p.fwd = Fwd::Mfma;
    else if (sw.mfma && av[l].first) p.fwd = Fwd::First;
    else if (sw.mfma && av[l].output) p.fwd = Fwd::Output;
    // a virtual input exists only inside the MFMA kernels' staging: never hand its (null) pointer to the direct kernel
    else if (src_virt(l)) return fail(kPlanErrState, "layer %d: no MFMA forward kernel for a layer whose input is not materialised", l);
    else p.fwd = Fwd::Generic;
    p.repack_fwd = p.fwd == Fwd::Generic;
    p.stats = !s.use_norm ? Stats::None : (p.fwd == Fwd::X6 || p.fwd == Fwd::Mfma || p.fwd == Fwd::First) ? Stats::Conv : Stats::Reduce;
    p.out = P.virt(l + 1) ? Out::Virtual : (s.use_norm || s.use_act || s.skip_pre >= 0 || s.skip_post >= 0) ? Out::Stored : Out::IsZ;
    p.bn_act = p.out != Out::Stored ? BnAct::None : s.cout % 2 == 0 ? BnAct::Pair : BnAct::Scalar;
    p.vskip = p.bn_act != BnAct::None && P.virt(s.skip_post);
    if (p.vskip && p.bn_act != BnAct::Pair) return fail(kPlanErrState, "layer %d: a virtual skip source needs the pair kernel", l);
  }

  // ---- backward.  G[id] collects d loss / d tensor id from every consumer (the conv reading it, skip adds).  A tensor with
  // one consumer is stored by that consumer's MFMA dgrad (overwrite).  A tensor that some layer adds as a skip gets its first
  // contribution from that layer's bwd_route2 (the skip consumer comes later in the net than the convolution that reads the
  // tensor, so earlier in the backward loop), which can STORE it (lazy).  The others are zeroed before the loop.  written[id]
  // follows the loop; whoever must add to a tensor nobody has written yet zeroes it first (not reached in the three nets).
  auto overwrite = [&](int l) {   // layer l's dgrad may overwrite G[src] (MFMA kernels only; the generic kernel always +=)
    const LayerSpec& s = net.layer[l];
    return sw.mfma && (av[l].dgrad || av[l].output) && s.src > 0 && consumers[s.src] == 1;
  };
  bool written[kMaxLayers + 1] = {};
  {
    bool plain[kMaxLayers + 1] = {}, lazy[kMaxLayers + 1] = {};
    for (int l = 0; l < L; ++l) {
      const LayerSpec& s = net.layer[l];
      if (overwrite(l)) plain[s.src] = true;
      if (sw.mfma && s.cout % 2 == 0) {
        if (s.skip_pre > 0) lazy[s.skip_pre] = true;
        if (s.skip_post > 0) lazy[s.skip_post] = true;
      }
    }
    for (int id = 1; id < L; ++id) {
      written[id] = plain[id] || !lazy[id];
      P.zero_first[id] = !plain[id] && !lazy[id];
    }
  }
  auto fuse_dz_of = [&](int l) {
    const LayerSpec& s = net.layer[l];
    return sw.fuse_dz && sw.mfma && s.use_norm && s.cout % 2 == 0 &&
           (av[l].first || (cin_of(l) % 2 == 0 && av[l].fwd && (s.src == 0 || av[l].dgrad)));
  };
  // (a skip added AFTER the ReLU -- CR-CED's block outputs -- does not enter the mask: d_u = g [bn(z) > 0] there too, so those
  // layers' d_u need not be written either; bwd_route2 still routes g to the skip's source)
  auto lazy_mask_of = [&](int l) { return fuse_dz_of(l) && net.layer[l].use_act && net.layer[l].skip_pre < 0; };
  // Layer l adds tensor skip_post AFTER its ReLU: d tensor += G[l + 1] unchanged.  Where that would be the tensor's first
  // contribution and the one dgrad that completes it is an MFMA kernel, the copy is not made: that dgrad reads its accumulate
  // operand from G[l + 1] (out = acc_from + conv).  G[l + 1] is final by then -- its writers are the consumers of tensor
  // l + 1, all later layers -- and every G tensor is its own allocation.  (Even cout: only bwd_route2 leaves the skip out.)
  auto alias_ok = [&](int l) {
    const LayerSpec& s = net.layer[l];
    if (!sw.mfma || !sw.fuse_dz || s.cout % 2 != 0 || s.skip_post <= 0 || s.skip_pre > 0 || written[s.skip_post] || consumers[s.skip_post] != 2) return false;
    const int lc = n_conv[s.skip_post] == 1 ? conv_user[s.skip_post] : -1;
    return lc >= 0 && lc < l && av[lc].dgrad && net.layer[lc].cout % 2 == 0;
  };
  // a producer whose sums may come out of its consumer's dgrad: masked lazily, and nothing left to route -- no skip, or a
  // post-ReLU skip whose gradient is not copied.  Asked at the consumer; the producer finds `sums` set when its turn comes,
  // and nothing writes the skip's gradient tensor in between.
  auto sums_in_dgrad_ok = [&](int pl) { return lazy_mask_of(pl) && (net.layer[pl].skip_post < 0 || alias_ok(pl)); };
  int alias_src[kMaxLayers + 1] = {};
  for (int l = L - 1; l >= 0; --l) {
    const LayerSpec& s = net.layer[l];
    LayerPlan& p = P.layer[l];
    const int cin = cin_of(l);
    p.fuse_dz = fuse_dz_of(l);
    p.lazy_mask = lazy_mask_of(l);
    p.passthrough = sw.mfma && av[l].output && s.src > 0 && consumers[s.src] == 1;
    const int skip_id = skip_of(s);
    p.skip_alias = alias_ok(l);
    if (p.skip_alias) { alias_src[s.skip_post] = l + 1; written[s.skip_post] = true; }
    const bool from_dgrad = p.sums == Sums::DgradZ || p.sums == Sums::FusedX;   // set by the consumer, earlier in this loop
    if (p.passthrough) {
      p.route = Route::None;
    } else if (from_dgrad) {
      if (s.skip_post > 0 && !p.skip_alias)
        return fail(kPlanErrState, "layer %d: sums came out of the dgrad but its skip gradient still needs routing", l);
      p.route = Route::None;
    } else if (s.cout % 2 == 0) {
      p.route = Route::Pair;
      p.skip_first = skip_id > 0 && !written[skip_id];
      if (skip_id > 0) written[skip_id] = true;
      if (s.use_norm) p.sums = Sums::Route2;
    } else {
      p.route = Route::Scalar;
      p.zero_before_skip = skip_id > 0 && !written[skip_id];
      if (skip_id > 0) written[skip_id] = true;
      if (s.use_norm) p.sums = Sums::RouteReduce;
    }
    // wgrad and dgrad in one kernel where the layer's input tensor has this layer as its only consumer; x virtual and
    // "leaves the producer's sums" go together in the kernels that were built
    const int pl = s.src - 1;
    bool fused = false;
    if (sw.fuse_bwd && s.src > 0 && p.fuse_dz && av[l].dgrad && overwrite(l)) {
      const bool want_sums = sw.fuse_sums && sums_in_dgrad_ok(pl);
      if (P.virt(s.src) == want_sums && av[l].fused) {
        fused = true;
        p.src_sums = want_sums;
        if (want_sums) P.layer[pl].sums = Sums::FusedX;
      }
    }
    if (fused) p.wgrad = Wgrad::Fused;
    else if (sw.mfma && av[l].fwd) p.wgrad = Wgrad::Mfma;
    else if (sw.mfma && av[l].first) p.wgrad = Wgrad::First;
    else if (sw.mfma && av[l].output) p.wgrad = Wgrad::Output;
    else if (src_virt(l) || p.fuse_dz)   // the direct kernel needs the activation and dz in HBM
      return fail(kPlanErrState, "layer %d: no MFMA wgrad kernel for a layer with fused activation / dz", l);
    else if (!av[l].direct_wgrad) return fail(kPlanErrArg, "layer %d too large for conv_wgrad", l);
    else p.wgrad = Wgrad::Generic;

    // dx into G[src], as a forward conv of dz with the flipped / transposed kernel and the other SAME half
    auto variant = [&](bool accum, bool sa) { return tms::tm_variant_has(false, s.cout, cin, accum, false, false, p.fuse_dz, sa); };
    p.dgrad = Dgrad::None;
    if (s.src > 0 && fused) {
      p.dgrad = Dgrad::Fused;
    } else if (s.src > 0) {
      const bool mfma_dgrad = sw.mfma && av[l].dgrad, ow = overwrite(l);
      if (sw.mfma && av[l].output && consumers[s.src] == 1) {
        p.dgrad = Dgrad::Output;
      } else if (sw.fuse_sums && mfma_dgrad && ow && sums_in_dgrad_ok(pl) && variant(false, true)) {
        p.dgrad = Dgrad::MfmaSums;
      } else if (sw.fuse_sums && mfma_dgrad && !ow && p.fuse_dz && written[s.src] && n_conv[s.src] == 1 && sums_in_dgrad_ok(pl) && variant(true, true)) {
        // an accumulating dgrad that adds the LAST contribution to G[src] -- the conv consumer of a tensor comes before its
        // skip consumers in the net, so after them here -- sees the complete gradient in its epilogue (CR-CED's skip sources)
        p.dgrad = Dgrad::MfmaAccSums;
        p.accumulate = true;
        p.acc_from = alias_src[s.src];
      } else if (mfma_dgrad && variant(!ow, false)) {
        p.dgrad = Dgrad::Mfma;
        p.accumulate = !ow;
        p.acc_from = ow ? 0 : alias_src[s.src];
      } else if (alias_src[s.src]) {
        return fail(kPlanErrState, "layer %d: no accumulating MFMA dgrad kernel for an aliased skip gradient", l);
      } else if (p.fuse_dz) {
        return fail(kPlanErrState, "layer %d: no MFMA dgrad kernel for a layer with fused dz", l);
      } else {
        p.dgrad = Dgrad::Generic;
        p.accumulate = true;
      }
      if (p.dgrad == Dgrad::MfmaSums || p.dgrad == Dgrad::MfmaAccSums) { p.src_sums = true; P.layer[pl].sums = Sums::DgradZ; }
      if (p.accumulate && p.dgrad != Dgrad::MfmaAccSums && !written[s.src]) { p.zero_before_dgrad = true; written[s.src] = true; }
    }
    p.repack_dgrad = !sw.mfma || p.dgrad == Dgrad::Generic;   // (with every kernel direct, the first layer's is packed too, unused)
    p.pack_dgrad = sw.mfma && av[l].dgrad;                    // (also where the fused or the output-layer kernel takes the dgrad: their fallback's packet)
  }
  return kPlanOk;
}

}  // namespace plan
}  // namespace rced
