// Round growth, the planner (round_common.h): replay, prediction and the next round's plans.
#pragma once

#include "find_stage.h"
#include "round_common.h"
#include "round_xt.h"

namespace lgbm_amd {
namespace dev {

// the plan's LDS tables (RoundPlanLds bytes): node tables (gain, -inf when the node has no
// split; real feature; first child or -1), leaf tables (gain, real feature, node; accepted
// leaves / nodes) and the prediction's copies of the leaf tables (+ levels below the leaf)
struct PlanTables {
  double *ng, *tg, *sg;
  unsigned long long* qkey;  // the bottleneck prediction's region: order keys and nodes (PredictBottleneck)
  int *nrf, *nch, *nfi, *trf, *tnode, *acc, *accn, *srf, *snode, *svd, *qn;
  __device__ PlanTables(unsigned char* lds, int NN, int L) {
    ng = reinterpret_cast<double*>(lds);
    tg = ng + NN;
    sg = tg + L;
    qkey = reinterpret_cast<unsigned long long*>(sg + L);
    nrf = reinterpret_cast<int*>(qkey + NN);
    nch = nrf + NN;
    nfi = nch + NN;  // the node's best split feature (inner index; -1: none)
    trf = nfi + NN;
    tnode = trf + L;
    acc = tnode + L;
    accn = acc + L;
    srf = accn + L;
    snode = srf + L;
    svd = snode + L;
    qn = svd + L;
  }
};

// ordered keys of the replay's argmax (SplitInfo order over leaves): larger gain first (NaN =
// -inf), then smaller real feature, then lower leaf id -- two wave max-reductions over DPP
// lane moves instead of a shuffle butterfly carrying five values
__device__ __forceinline__ uint32_t TieKey(int rf, int leaf) {
  const uint32_t r = rf < 0 ? 0x3fffffu : min(static_cast<uint32_t>(rf), 0x3ffffeu);
  return ~((r << 10) | static_cast<uint32_t>(leaf));
}
// the argmax leaf among l <= s with take(l) (one wave; -1: none)
template <typename Take>
__device__ __forceinline__ int WaveArgmaxLeaf(const double* tg, const int* trf, int s, Take take) {
  const int lane = threadIdx.x & 63;
  unsigned long long gk = 0;
  uint32_t tk = 0;
  for (int l = lane; l <= s; l += kWave) {
    if (!take(l)) continue;
    const unsigned long long k = GainKey(tg[l]);
    const uint32_t t = TieKey(trf[l], l);
    if (k > gk || (k == gk && t > tk)) {
      gk = k;
      tk = t;
    }
  }
  const unsigned long long gm = WaveMaxDpp(gk);
  if (gm == 0) return -1;
  const uint32_t tm = WaveMaxDpp(gk == gm ? tk : 0u);
  return static_cast<int>((~tm) & 1023u);
}
__device__ __forceinline__ void WaveLdsSync() {  // lane 0's LDS stores before the wave's next loads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#ifndef LGBM_REPLAY_KEY32
#define LGBM_REPLAY_KEY32 1
#endif
#ifndef LGBM_REPLAY_PREFETCH
#define LGBM_REPLAY_PREFETCH 0  // (A/B: children loaded ahead -- 2.356 vs 2.343 ms/iter, not kept)
#endif
// Replay + prediction with one leaf per lane in registers (num_leaves <= 64, wave 0): a step
// is one 64-bit DPP max over the gain keys (the tie key's max only when gains tie exactly),
// reads of the winner's lane, and LDS reads of the node tables by the two lanes whose leaf
// changes -- no LDS round trip through every lane per step.  Same order and picks as the LDS
// tables' loop below.
struct RegLeaf {
  double g;
  int rf, node, ch;
  uint32_t k32;  // GainKey32(g): the argmax's first, 32-bit pass
#if LGBM_REPLAY_PREFETCH
  // the node's children (ch >= 0), loaded ahead: gain, real feature, first child of each
  double g0, g1;
  int rf0, rf1, ch0, ch1;
#endif
};
// order-preserving 32-bit key of a gain (NaN = -inf): the gain rounded to float, whose
// rounding is monotone -- a larger float key means a larger gain; equal float keys are
// resolved by the exact 64-bit keys
__device__ __forceinline__ uint32_t GainKey32(double g) {
  if (g != g) g = -INFINITY;
  const uint32_t b = __float_as_uint(static_cast<float>(g));
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ int RegArgmax(const RegLeaf& x, bool live) {
  const int lane = threadIdx.x & 63;
  // one 32-bit DPP max; the exact 64-bit / tie passes only when the float keys tie
#if LGBM_REPLAY_KEY32
  const uint32_t k = live ? x.k32 : 0u;
#else
  const uint32_t k = live ? 1u : 0u;  // (A/B: every live lane into the 64-bit pass)
#endif
  const uint32_t km = WaveMaxDpp(k);
  const unsigned long long t32 = __ballot(live && k == km);
  if (__popcll(t32) == 1) return __builtin_amdgcn_readfirstlane(static_cast<int>(__builtin_ctzll(t32)));
  const bool in = live && k == km;
  const unsigned long long gk = in ? GainKey(x.g) : 0ull;
  const unsigned long long gm = WaveMaxDpp(gk);
  const unsigned long long tied = __ballot(in && gk == gm);
  if (__popcll(tied) == 1) return __builtin_amdgcn_readfirstlane(static_cast<int>(__builtin_ctzll(tied)));
  const uint32_t tm = WaveMaxDpp((in && gk == gm) ? TieKey(x.rf, lane) : 0u);
  return static_cast<int>((~tm) & 1023u);
}
#if LGBM_REPLAY_PREFETCH
// the children of the lane's node, loaded now and used only when the lane next wins: the
// winner's children come from its registers (readlane) instead of an LDS round trip that the
// next argmax would wait for
__device__ __forceinline__ void RegPrefetch(RegLeaf* x, const double* ng, const int* nrf, const int* nch) {
  const int c = x->ch;
  x->g0 = c >= 0 ? ng[c] : -INFINITY;
  x->rf0 = c >= 0 ? nrf[c] : -1;
  x->ch0 = c >= 0 ? nch[c] : -1;
  x->g1 = c >= 0 ? ng[c + 1] : -INFINITY;
  x->rf1 = c >= 0 ? nrf[c + 1] : -1;
  x->ch1 = c >= 0 ? nch[c + 1] : -1;
}
__device__ __forceinline__ void RegSet(RegLeaf* x, int node, double g, int rf, int ch, const double* ng, const int* nrf,
                                       const int* nch) {
  x->node = node;
  x->g = g;
  x->k32 = GainKey32(g);
  x->rf = rf;
  x->ch = ch;
  RegPrefetch(x, ng, nrf, nch);
}
#endif
__device__ __forceinline__ void RegLoad(RegLeaf* x, int node, const double* ng, const int* nrf, const int* nch) {
  x->node = node;
  x->g = node >= 0 ? ng[node] : -INFINITY;
  x->k32 = GainKey32(x->g);
  x->rf = node >= 0 ? nrf[node] : -1;
  x->ch = node >= 0 ? nch[node] : -1;
#if LGBM_REPLAY_PREFETCH
  RegPrefetch(x, ng, nrf, nch);
#endif
}
// lanes w and nl take the children of lane w's node (c, c + 1)
__device__ __forceinline__ void RegTakeChildren(RegLeaf* x, int lane, int w, int nl, int c, const double* ng,
                                                const int* nrf, const int* nch) {
#if LGBM_REPLAY_PREFETCH
  const double g0 = ReadLane(x->g0, w), g1 = ReadLane(x->g1, w);
  const int rf0 = ReadLane(x->rf0, w), rf1 = ReadLane(x->rf1, w);
  const int ch0 = ReadLane(x->ch0, w), ch1 = ReadLane(x->ch1, w);
  if (lane == w) RegSet(x, c, g0, rf0, ch0, ng, nrf, nch);
  if (lane == nl) RegSet(x, c + 1, g1, rf1, ch1, ng, nrf, nch);
#else
  if (lane == w) RegLoad(x, c, ng, nrf, nch);
  if (lane == nl) RegLoad(x, c + 1, ng, nrf, nch);
#endif
}
// Deferred fold (per-node sampling, KArgs::round_bynode; extra_trees, KArgs::round_xt), wave 0,
// when the replay accepts split s of leaf w (node n, children c = left and c + 1 = right; the
// left keeps leaf id w, the right is leaf s + 1).  SerialTreeLearner::BeforeFindBestSplit /
// FindBestSplits / FindBestSplitsFromHistograms in the sequential order: unless the children
// are not scanned (depth, min_data, the tree's last split), the smaller child (fewer rows; a
// tie: the right one) is evaluated first -- per-node sampling: it takes draw d, the larger
// d + 1; extra_trees: per feature, its threshold draw comes first.  The parent's flag row moves
// to the larger child's leaf id (the smaller one keeps the stale row of its id), a feature the
// parent could not split is 0 for the smaller child and skipped, and a feature a child
// evaluates takes the child's flag and competes for its best split (per-node sampling: the
// scan's result, KArgs::node_fb; extra_trees: the drawn threshold's, XtEvalNum).  The
// children's bests go to cbest and the node tables.  xcnt: extra_trees draw counts per feature
// (LDS, at most kXtLaneFeatures * 64 features).
// (XT: compiled in only where the extra_trees replay runs -- k_round_plan; the replay's
// registers would otherwise set the occupancy of every scan workgroup of k_round_find)
constexpr int kXtLaneFeatures = 4;
template <bool XT>
__device__ bool DeferAccept(const KArgs& a, int s, int w, int n, int c, int* draw, double* ng, int* nrf, int* nfi,
                            int* xcnt, int my_node, const int* tnode) {
  const int lane = threadIdx.x & 63;
  const int L = a.p.num_leaves, NF = a.p.num_features, md = a.p.sp.min_data_in_leaf;
  // CEGB coupled penalties (KArgs::round_cegb): the split's feature, if the model had not used
  // it, refunds its coupled penalty to the other leaves' remembered candidates first
  // (CostEfficientGradientBoosting::UpdateLeafBestSplits, at SplitInner's start).  A refunded
  // leaf is never an expanded one: the plan expands only leaves no refund can change (below).
  // Leaf l's node: this lane's my_node (register replay, leaf = lane) or tnode[l].
  bool refunded = false;
  if (a.round_cegb && a.cegb_coupled != nullptr) {
    const int fsplit = nfi[n];
    if (fsplit >= 0 && !a.cegb_used[fsplit]) {
      refunded = true;
      const double refund = a.cegb_coupled[fsplit];
      for (int l = lane; l <= s; l += kWave) {
        if (l == w) continue;
        const int nd = tnode != nullptr ? tnode[l] : my_node;
        FeatureBest cand = a.cegb_mem[static_cast<size_t>(l) * NF + fsplit];
        cand.gain += refund;
        const double cg = ng[nd];
        const int crf = nrf[nd] < 0 ? 0x7fffffff : nrf[nd];
        const int nrf_c = cand.feature < 0 ? 0x7fffffff : cand.real_feature;
        if (cg > -INFINITY && (cand.gain > cg || (cand.gain == cg && nrf_c < crf))) {
          a.cbest[nd] = cand;
          ng[nd] = cand.gain;
          nrf[nd] = cand.real_feature;
          nfi[nd] = cand.feature;
        }
      }
      if (lane == 0) a.cegb_used[fsplit] = 1;
      __threadfence_block();  // (the children's folds below and later splits read the flag)
      WaveLdsSync();
    }
  }
  const RNode& P = a.rnode[n];
  // (data-parallel: the children's global counts -- the split's estimates -- as the reference's
  // GetGlobalDataCountInLeaf; this rank's rows otherwise)
  const bool dpc = a.p.data_parallel != 0;
  const int nl = dpc ? a.rnode[c].st.global_count : P.total_left;
  const int nr = dpc ? a.rnode[c + 1].st.global_count : P.count - P.total_left;
  const int depth = a.rnode[c].st.depth;
  const bool scanned = s + 1 < L - 1 && !(a.p.max_depth > 0 && depth >= a.p.max_depth) && !(nl < 2 * md && nr < 2 * md);
  if (!scanned) {
    if (lane < 2) {
      a.cbest[c + lane] = FeatureBestNone();
      ng[c + lane] = -INFINITY;
      nrf[c + lane] = -1;
      nfi[c + lane] = -1;
    }
    WaveLdsSync();
    return refunded;
  }
  const bool bn = a.round_bynode != 0, xt = XT && a.round_xt != 0;
  int d0 = 0;
  if (bn) {
    d0 = *draw;
    *draw = d0 + 2;
  }
  const bool small_left = nl < nr;
  const int small_leaf = small_left ? w : s + 1, large_leaf = small_left ? s + 1 : w;
  const int small_node = small_left ? c : c + 1, large_node = small_left ? c + 1 : c;
  int8_t* rw = a.leaf_rows + static_cast<size_t>(w) * NF;
  int8_t* rn = a.leaf_rows + static_cast<size_t>(s + 1) * NF;
  int8_t* rs = a.leaf_rows + static_cast<size_t>(small_leaf) * NF;
  int8_t* rl = a.leaf_rows + static_cast<size_t>(large_leaf) * NF;
  const int8_t* ms = bn ? a.node_mask + static_cast<size_t>(d0) * NF : nullptr;
  const int8_t* ml = bn ? ms + NF : nullptr;
  const int8_t* fs = a.splittable + static_cast<size_t>(small_node) * NF;
  const int8_t* fl = a.splittable + static_cast<size_t>(large_node) * NF;
  const bool cg = a.round_cegb != 0;
  const FeatureBest* bs = (bn || cg) ? a.node_fb + static_cast<size_t>(small_node) * NF : nullptr;
  const FeatureBest* bl = (bn || cg) ? a.node_fb + static_cast<size_t>(large_node) * NF : nullptr;
  const int ns = small_left ? nl : nr, nlg = small_left ? nr : nl;
  ChildStats css, csl;
  if (xt) {
    css = a.rnode[small_node].st;
    csl = a.rnode[large_node].st;
  }
  // (CEGB: the scans published the raw candidates -- remembered per leaf id for later refunds
  // -- and the penalties of the model's used set now are subtracted here)
  auto cegb_take = [&](FeatureBest* o, int leaf, int f, int rows) {
    a.cegb_mem[static_cast<size_t>(leaf) * NF + f] = *o;
    o->gain -= CegbScanDelta(a, f, rows);
  };
  ArgC cs = ArgNone(), cl = ArgNone();
  FeatureBest rec_s, rec_l;  // (extra_trees: this lane's best records of the two children)
  // (the flag rows are read before any is written: the children's rows are the parent's and the
  // new leaf's)
  if constexpr (XT) {
    if (xt) {
      // extra_trees, one child's evaluation live at a time: pass 0 the smaller child (its flags
      // kept in LDS), pass 1 the larger one and the rows
      __shared__ int8_t s_gs[kXtLaneFeatures * kWave];
      for (int pass = 0; pass < 2; ++pass) {
        const bool small = pass == 0;
        for (int f = lane; f < NF; f += kWave) {
          const int8_t parent = rw[f], stale = rn[f];
          const bool live = a.tree_mask[f] && parent;
          const bool es = !bn || ms[f], el = !bn || ml[f];
          const Feature F = a.feat[f];
          const bool drawn = F.num_bin - 2 > 0;
          const int cnt = xcnt[f];  // (the smaller child draws first)
          int8_t g = -1;
          if (live && (small ? es : el)) {
            const int k = cnt + 1 + (!small && es && drawn ? 1 : 0);
            const int thr = drawn ? XtThreshold(a, F, f, k) : 0;
            FeatureBest o;
            g = XtEvalNum(a, F, f, small ? small_node : large_node, small ? css : csl, small ? ns : nlg, thr, &o) ? 1 : 0;
            ArgC& cc = small ? cs : cl;
            if (o.feature >= 0 && (cc.idx < 0 || SplitBetter(o.gain, o.real_feature, cc.g, cc.rf))) {
              cc.g = o.gain;
              cc.rf = o.real_feature;
              cc.idx = f;
              if (small) rec_s = o;
              else rec_l = o;
            }
          }
          if (small) {
            s_gs[f] = g;
            continue;
          }
          int8_t vs = stale, vl = parent;
          if (a.tree_mask[f]) {
            if (!parent) {
              vs = 0;
            } else {
              if (s_gs[f] >= 0) vs = s_gs[f];
              if (g >= 0) vl = g;
            }
          }
          if (live) xcnt[f] = cnt + ((es && drawn) ? 1 : 0) + ((el && drawn) ? 1 : 0);
          rs[f] = vs;
          rl[f] = vl;
        }
        WaveLdsSync();
      }
    }
  }
  if (!xt) {
    for (int f = lane; f < NF; f += kWave) {
      const int8_t parent = rw[f], stale = rn[f];
      int8_t vs = stale, vl = parent;  // (the rows after the move: the larger child holds the parent's)
      if (a.tree_mask[f]) {
        if (!parent) {
          vs = 0;
        } else {
          // (the fold reads three fields of a record; CEGB copies it into the leaf's memory)
          if (!bn || ms[f]) {
            vs = fs[f];
            const FeatureBest& r = bs[f];
            double og = r.gain;
            const int orf = r.real_feature, ofe = r.feature;
            if (cg) {
              FeatureBest o = r;
              cegb_take(&o, small_leaf, f, ns);
              og = o.gain;
            }
            if (ofe >= 0 && (cs.idx < 0 || SplitBetter(og, orf, cs.g, cs.rf))) {
              cs.g = og;
              cs.rf = orf;
              cs.idx = f;
            }
          }
          if (!bn || ml[f]) {
            vl = fl[f];
            const FeatureBest& r = bl[f];
            double og = r.gain;
            const int orf = r.real_feature, ofe = r.feature;
            if (cg) {
              FeatureBest o = r;
              cegb_take(&o, large_leaf, f, nlg);
              og = o.gain;
            }
            if (ofe >= 0 && (cl.idx < 0 || SplitBetter(og, orf, cl.g, cl.rf))) {
              cl.g = og;
              cl.rf = orf;
              cl.idx = f;
            }
          }
        }
      }
      rs[f] = vs;
      rl[f] = vl;
    }
  }
  const ArgC bcs = ArgWaveBest(cs), bcl = ArgWaveBest(cl);
  const FeatureBest none = FeatureBestNone();
  if (xt) {
    // the lane holding a child's winner hands its record over through LDS; lanes 0 / 1 store
    // the children's bests (a uniform-address store from a lane picked at run time lost its
    // value to the other lanes' masked copies)
    __shared__ FeatureBest s_rec[2];
    if (bcs.idx >= 0 && (bcs.idx & (kWave - 1)) == lane) s_rec[0] = rec_s;
    if (bcl.idx >= 0 && (bcl.idx & (kWave - 1)) == lane) s_rec[1] = rec_l;
    WaveLdsSync();
    if (lane < 2) {
      const ArgC& b = lane == 0 ? bcs : bcl;
      const int node = lane == 0 ? small_node : large_node;
      const bool ok = b.idx >= 0 && b.g != -INFINITY;
      a.cbest[node] = ok ? s_rec[lane] : none;
      ng[node] = ok ? b.g : -INFINITY;
      nrf[node] = ok ? b.rf : -1;
      nfi[node] = ok ? b.idx : -1;
    }
  } else if (lane < 2) {
    const ArgC& b = lane == 0 ? bcs : bcl;
    const int node = lane == 0 ? small_node : large_node;
    FeatureBest o = none;
    if (b.idx >= 0 && b.g != -INFINITY) {
      o = (lane == 0 ? bs : bl)[b.idx];
      if (cg) o.gain = b.g;  // (the penalised gain)
    }
    a.cbest[node] = o;
    ng[node] = o.feature >= 0 ? o.gain : -INFINITY;
    nrf[node] = o.real_feature;
    nfi[node] = o.feature;
  }
  if (!xt && a.node_fb_cat != nullptr) {
    // a categorical winner's category set, from the node's copy (the whole wave)
    for (int side = 0; side < 2; ++side) {
      const ArgC& b = side == 0 ? bcs : bcl;
      if (b.idx < 0 || b.g == -INFINITY || a.node_cat_slot[b.idx] < 0) continue;
      const int node = side == 0 ? small_node : large_node;
      const uint32_t* src = a.node_fb_cat + (static_cast<size_t>(node) * a.node_cat_slots + a.node_cat_slot[b.idx]) * kMaxCatWords;
      uint32_t* dst = a.cbest_cat + static_cast<size_t>(node) * kMaxCatWords;
      for (int i = lane; i < kMaxCatWords; i += kWave) dst[i] = src[i];
    }
  }
  WaveLdsSync();
  return refunded;
}

// The replay (wave 0): returns s, the splits after it, and *done; acc / accn / tnode as the LDS
// path.  x keeps the replayed leaves for the prediction.
template <bool XT>
__device__ int ReplayRegs(const KArgs& a, int L, int s0, double* ng, int* nrf, const int* nch, int* nfi, int* tnode,
                          int* acc, int* accn, RegLeaf* xp, int* done_out, int* draw, int* xcnt, int* blocker) {
  const int lane = threadIdx.x & 63;
  RegLeaf& x = *xp;
  RegLoad(&x, lane <= s0 ? tnode[lane] : -1, ng, nrf, nch);
  int s = s0, done = 0;
  *blocker = -1;
  for (;;) {
    if (s >= L - 1) {
      done = 1;
      break;
    }
    const int w = RegArgmax(x, lane <= s);
    if (!(ReadLane(x.g, w) > 0.0)) {
      done = 1;
      break;
    }
    const int c = ReadLane(x.ch, w);
    if (c < 0) {
      *blocker = ReadLane(x.node, w);
      break;
    }
    const int nl = s + 1;
    if (lane == 0) {
      acc[s - s0] = w;
      accn[s - s0] = ReadLane(x.node, w);
    }
    bool refunded = false;
    if (a.round_bynode || a.round_cegb || (XT && a.round_xt)) {
      refunded = DeferAccept<XT>(a, s, w, ReadLane(x.node, w), c, draw, ng, nrf, nfi, xcnt, x.node, nullptr);
    }
    RegTakeChildren(&x, lane, w, nl, c, ng, nrf, nch);
    if (refunded) RegLoad(&x, lane <= nl ? x.node : -1, ng, nrf, nch);  // (refunded leaves' new bests)
    ++s;
  }
  if (lane <= s) tnode[lane] = x.node;
  *done_out = done;
  return s;
}

// the next round's expansions predicted past the blocker (wave 0, after ReplayRegs): returns
// the picks' count (s_pick); *done when the tree cannot go on
__device__ int PredictRegs(const KArgs& a, int L, int s, int used, int kround, const double* ng, const int* nrf,
                           const int* nch, int* s_pick, RegLeaf* xp, int* done_io) {
  const int lane = threadIdx.x & 63;
  RegLeaf& x = *xp;
  int done = *done_io, n = 0;
  if (!done) {
    const int need = L - 1 - s;
    int kmax = min(kround, a.round_need_div > 0 ? max(1, need / a.round_need_div) : need);
    kmax = min(kmax, a.round_emax - used - (need - 1));
    kmax = max(kmax, min(1, a.round_emax - used));
    if (kmax <= 0) done = 1;
    const int vmax = (a.round_bynode || a.round_xt || a.round_cegb) ? 0 : a.round_vmax;  // (deferred folds: the current leaves only)
    int vd = 0;
    for (int ss = s; !done && n < kmax && ss < L - 1; ++ss) {
      const int w = RegArgmax(x, lane <= ss);
      if (!(ReadLane(x.g, w) > 0.0)) break;
      const int c = ReadLane(x.ch, w), v = ReadLane(vd, w);
      const int nl = ss + 1;
      if (c >= 0) {
        RegTakeChildren(&x, lane, w, nl, c, ng, nrf, nch);
        if (lane == w || lane == nl) vd = v + 1;
      } else {
        if (v <= vmax) {
          if (lane == 0) s_pick[n] = ReadLane(x.node, w);
          ++n;
        }
        if (lane == w || lane == nl) RegLoad(&x, -1, ng, nrf, nch);
      }
    }
    if (n == 0) done = 1;
  }
  *done_io = done;
  return n;
}

// The next round's picks from order keys instead of the step walk (KArgs::round_predict; wave
// 0 after the replay, any num_leaves; the blocker is the first pick).  Best-first order pops a
// node only after its ancestors below the current leaf, so the known nodes come out by
// decreasing bottleneck m(v) -- the least gain on the path from the leaf to v: the frontier
// falls below m(v) only after v is reached -- and, within one bottleneck, by the least gain
// below it (m2), ancestors first.  Keys (m, m2, -depth) of float-rounded gains: ties and deeper
// bottleneck levels order approximately, which only changes the nodes expanded ahead, never
// the tree (the replay is exact).  A pick's pops before it are the region's nodes with gain > 0
// on the path and a larger key; picks stop at kmax or when the tree's remaining splits are used
// up, as the walk's.  Cost: one pass per level of the known region and two wave passes per pick
// instead of one argmax step per pop (the walk's 3 -> 18 us per plan late in a 63-leaf tree).
__device__ int PredictBottleneck(const KArgs& a, int L, int s, int used, int kround, const double* ng, const int* nch,
                                 const int* tnode, int blocker, unsigned long long* qkey, int* qn, int* s_pick,
                                 int* done_io) {
  const int lane = threadIdx.x & 63;
  int done = *done_io, n = 0;
  const int need = L - 1 - s;
  int kmax = 0;
  if (!done) {
    kmax = min(kround, a.round_need_div > 0 ? max(1, need / a.round_need_div) : need);
    kmax = min(kmax, a.round_emax - used - (need - 1));
    kmax = max(kmax, min(1, a.round_emax - used));
    if (kmax <= 0 || blocker < 0) done = 1;  // (unreachable: the budget keeps room for the blocker)
  }
  if (!done) {
    const int vmax = (a.round_bynode || a.round_xt || a.round_cegb) ? 0 : min(a.round_vmax, 14);
    constexpr uint32_t kPos = 0x80000000u;   // GainKey32(0.0): keys above are gains > 0
    constexpr uint32_t kNone = 0xfffffff0u;  // m2 before a gain below the bottleneck (low 4 bits: 15 - depth)
    for (int l = lane; l <= s; l += kWave) {  // the region's first level: the leaves' nodes
      const int nd = tnode[l];
      qn[l] = nd;
      qkey[l] = (static_cast<unsigned long long>(GainKey32(ng[nd])) << 32) | kNone | 15u;
    }
    WaveLdsSync();
    // the region level by level: an expanded node with m > 0 appends its children
    int head = 0, tail = s + 1;
    while (head < tail) {
      const int i = head + lane, t0 = tail;
      unsigned long long k = 0;
      int c = -1;
      if (i < t0) {
        k = qkey[i];
        c = nch[qn[i]];
      }
      const uint32_t km = static_cast<uint32_t>(k >> 32);
      const bool grow = i < t0 && c >= 0 && km > kPos;
      const unsigned long long bm = __ballot(grow);
      if (grow) {
        const int q = t0 + 2 * __popcll(bm & ((1ull << lane) - 1));
        const uint32_t km2 = static_cast<uint32_t>(k) & kNone;
        const uint32_t d = min(16u - (static_cast<uint32_t>(k) & 15u), 15u);  // the children's depth
        for (int j = 0; j < 2; ++j) {
          const uint32_t kc = GainKey32(ng[c + j]);
          const uint32_t m1 = kc <= km ? kc : km;
          const uint32_t m2 = kc <= km ? kNone : min(km2, kc & kNone);
          qn[q + j] = c + j;
          qkey[q + j] = (static_cast<unsigned long long>(m1) << 32) | m2 | (15u - d);
        }
      }
      tail = t0 + 2 * __popcll(bm);
      head = min(head + kWave, t0);
      WaveLdsSync();
    }
    const int R = tail;
    if (lane == 0) s_pick[0] = blocker;
    n = 1;
    for (; n < kmax; ++n) {
      // the best candidate left: unexpanded, within vmax levels, m > 0, not picked
      unsigned long long bk = 0;
      int bi = -1;
      for (int i = lane; i < R; i += kWave) {
        const int nd = qn[i];
        const unsigned long long k = qkey[i];
        if (nd < 0 || nd == blocker || static_cast<uint32_t>(k >> 32) <= kPos) continue;
        if (15 - static_cast<int>(k & 15u) > vmax || nch[nd] >= 0) continue;
        if (k > bk) {
          bk = k;
          bi = i;
        }
      }
      const unsigned long long gm = WaveMaxDpp(bk);
      if (gm == 0) break;
      // its pops before it: the region's nodes with m > 0 and a larger key
      int cnt = 0;
      for (int i = lane; i < R; i += kWave) {
        const unsigned long long k = qkey[i];
        cnt += (static_cast<uint32_t>(k >> 32) > kPos && k > gm) ? 1 : 0;
      }
      if (WaveSum(cnt) >= need) break;
      const unsigned long long own = __ballot(bi >= 0 && bk == gm);
      const int idx = ReadLane(bi, static_cast<int>(__builtin_ctzll(own)));
      if (lane == 0) {
        const int nd = qn[idx];
        s_pick[n] = nd;
        qn[idx] = -1 - nd;
      }
      WaveLdsSync();
    }
  }
  *done_io = done;
  return done ? 0 : n;
}

// One workgroup.  ROOT: the root's best split from its per-feature results (FindRoot), then
// the first plan.  Otherwise: fold the round's partition counts into its nodes, replay the
// best-first order over the leaves (wave 0, LDS tables): while the argmax leaf's node is
// expanded its split is accepted and its children nodes become the leaves w and s + 1 -- so a
// chain of speculative expansions is accepted in one replay.  Then the next round: the nodes
// the sequential order is predicted to need next, the leaf that ended the replay first,
// within the tree's expansion budget.
// Global loads are issued in few independent batches: every one is a ~1-2 us round trip.
// The finished tree to the host (KArgs::host_out): every split record in order (a numerical
// split's category words skipped), then the scalars with a system-scope release, so the host
// sees them only after the records.
__device__ void HostTreeOut(const KArgs& a, int nsplit, int rounds, int nodes, int draws) {
  constexpr int kRecWords = static_cast<int>(sizeof(SplitRecord) / 8);
  constexpr int kCatWord0 =
      static_cast<int>((__builtin_offsetof(SplitRecord, split) + __builtin_offsetof(DeviceSplit, cat_bits) + 7) / 8);
  static_assert(sizeof(SplitRecord) % 8 == 0, "8-byte words");
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.host_out + kHostOutHeaderWords);
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.rec);
  for (int i = threadIdx.x; i < nsplit * kRecWords; i += blockDim.x) {
    const int r = i / kRecWords, w = i - r * kRecWords;
    if (w >= kCatWord0 && !a.rec[r].split.is_categorical) continue;
    dst[i] = src[i];
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(&a.host_out[1], nsplit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&a.host_out[2], rounds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&a.host_out[3], nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&a.host_out[4], draws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&a.host_out[0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// (inline: the compiler refuses to inline an unhinted function into a caller once the two have
// more than 1100 basic blocks together, which the categorical scans are within a few blocks of;
// a called plan costs them a called function's register and stack budget)
template <bool ROOT, int NT, bool XT = false>
__device__ inline void RoundPlanBody(const KArgs& a, unsigned char* plan_lds) {
  constexpr int kPlanThreads = NT;
  __shared__ int s_done, s_s1, s_nexp, s_draw;
  __shared__ ArgC s_arg[kPlanThreads / kWave];
  __shared__ int s_pick[kMaxRoundExp];
  __shared__ int s_pc[kMaxRoundExp];
  // the next round's expansion plans and their children's nodes, composed in LDS by one thread
  // each and stored by every thread in 8-byte words (one thread storing a ~0.9 KB plan field by
  // field took ~3.5 us)
  __shared__ ExpPlan s_e[kMaxRoundExp];
  __shared__ RNode s_c[2 * kMaxRoundExp];
  Round* rd = a.rd;
  const int L = a.p.num_leaves, NF = a.p.num_features, NN = a.round_nodes, tid = threadIdx.x, lane = tid & 63;
  // node tables (gain, -inf when the node has no split; real feature; first child or -1),
  // leaf tables (gain, real feature, node; accepted leaves / nodes) and the prediction's copies
  // of the leaf tables (+ levels below the real leaf)
  const PlanTables T(plan_lds, NN, L);
  double *ng = T.ng, *tg = T.tg, *sg = T.sg;
  int *nrf = T.nrf, *nch = T.nch, *nfi = T.nfi, *trf = T.trf, *tnode = T.tnode, *acc = T.acc, *accn = T.accn,
      *srf = T.srf, *snode = T.snode, *svd = T.svd;
  const int s0 = rd->nsplit;
  const int nexp_prev = rd->nexp;
  const int round0 = rd->round, rounds0 = rd->rounds, accmax0 = rd->accepted_max;
  const int kcur = rd->k_cur;
  const int kround = (kcur > 0 && kcur < a.round_k) ? kcur : a.round_k;  // this tree's round width
  const int nn = rd->next_frow;  // nodes of the tree so far
  const int next_slot = rd->next_slot;
  const bool dp = a.p.data_parallel != 0;  // (global counts: the split's estimates)
  // LGBM_AMD_KTRACE: phase times of the plan (slots 16..24 of the round it ends)
  long long* ktr = (a.ktrace != nullptr && tid == 0 && rd->round < L) ? a.ktrace + static_cast<size_t>(rd->round) * kTraceSlots : nullptr;
  long long tprev = ktr != nullptr ? wall_clock64() : 0;
  if (ktr != nullptr) ktr[16] = tprev;
  auto stamp = [&](int k) {
    if (ktr != nullptr) {
      const long long now = wall_clock64();
      ktr[k] = now - tprev;
      tprev = now;
    }
  };
  if (ROOT) {
    ArgC c = ArgNone();
    for (int f = tid; f < NF; f += kPlanThreads) {
      const FeatureBest& fb = a.feat_best[FeatBestIndex(a, 0, f)];
      if (fb.feature >= 0 && (c.idx < 0 || SplitBetter(fb.gain, fb.real_feature, c.g, c.rf))) {
        c.g = fb.gain;
        c.rf = fb.real_feature;
        c.idx = f;
      }
    }
    c = ArgWaveBest(c);
    if (lane == 0) s_arg[tid >> 6] = c;
    // per-node sampling: the root leaf's row of the reference's flags takes the root scan's flags
    // of the features its sample (draw 0) evaluated; the others keep their (stale) values
    if (a.leaf_rows != nullptr && static_cast<int>(a.root[2]) >= 2 * a.p.sp.min_data_in_leaf) {
      const int8_t* rf0 = a.splittable + static_cast<size_t>(a.leaves[0].frow) * NF;
      for (int f = tid; f < NF; f += kPlanThreads) {
        if (!(a.tree_mask[f] && (a.node_mask == nullptr || a.node_mask[f]))) continue;
        if (a.round_dist) {  // (each rank wrote its own features' flags: the gathered records carry them all)
          const int fl = a.feat_best[FeatBestIndex(a, 0, f)].flag;
          if (fl >= 0) a.leaf_rows[f] = static_cast<int8_t>(fl);
        } else {
          a.leaf_rows[f] = rf0[f];
        }
      }
    }
    __syncthreads();
    ArgC b = s_arg[0];
    for (int k = 1; k < kPlanThreads / kWave; ++k) ArgTake(&b, s_arg[k]);
    if (b.idx >= 0 && b.g == -INFINITY) b.idx = -1;
    if (tid == 0) {
      // node 0: the root leaf and its best split
      FeatureBest fb = FeatureBestNone();
      if (b.idx >= 0) {
        fb = a.feat_best[FeatBestIndex(a, 0, b.idx)];
        const uint32_t* cat = FeatCat(a, 0, b.idx);
        if (fb.ncat > 0) {
          for (int w = 0; w < kMaxCatWords; ++w) a.cbest_cat[w] = cat[w];
        }
        ToDeviceSplit(fb, cat, &a.best[0]);
      } else {
        NoSplit(&a.best[0]);
      }
      a.cbest[0] = fb;
      // (per-node sampling: a root the reference learner does not scan makes no draw -- the
      // host advances its sampler by Round::bynode_next draws)
      if (a.round_bynode && static_cast<int>(a.root[2]) < 2 * a.p.sp.min_data_in_leaf) rd->bynode_next = 0;
      const Leaf R = a.leaves[0];
      RNode r;
      r.begin = R.begin;
      r.count = R.count;
      r.buf = R.buf;
      r.expanded = 0;
      r.child = -1;
      r.total_left = 0;
      r.st.sum_g = R.sum_g;
      r.st.sum_h = R.sum_h;
      r.st.output = R.output;
      r.st.cmin = R.cmin;
      r.st.cmax = R.cmax;
      r.st.global_count = R.global_count;
      r.st.depth = R.depth;
      r.st.slot = R.slot;
      r.st.leaf = 0;
      r.st.frow = 0;
      r.st.icmask = R.icmask;
      a.rnode[0] = r;
      if (a.round_vote) {  // (voting: the local root scan's sums)
        a.rnode_lsum[0] = R.lsum_g;
        a.rnode_lsum[1] = R.lsum_h;
      }
      ng[0] = b.idx >= 0 ? b.g : -INFINITY;
      nrf[0] = b.idx >= 0 ? b.rf : -1;
      nch[0] = -1;
      nfi[0] = b.idx >= 0 ? fb.feature : -1;
      tnode[0] = 0;
      tg[0] = ng[0];
      trf[0] = nrf[0];
    }
  } else {
    // the previous round's partition counts: its children's rows
    if (tid < nexp_prev) {
      const ExpPlan& E = rd->e[tid];
      const int tl = rd->cur[tid][0];
      const int pb = E.part_begin, pc = E.part_count, db = E.dst_buf, c = E.frow_child[0];
      a.rnode[E.node].total_left = tl;
      RNode* cn = a.rnode + c;
      cn[0].begin = pb;
      cn[0].count = tl;
      cn[0].buf = db;
      cn[1].begin = pb + tl;
      cn[1].count = pc - tl;
      cn[1].buf = db;
      if (a.round_vote) {
        // this rank's sums of the children (the local scan's, from k_round_split's fixed point)
        const double hg = static_cast<double>(static_cast<long long>(rd->loc_acc[tid][0])) * a.scales[2];
        const double hh = static_cast<double>(static_cast<long long>(rd->loc_acc[tid][1])) * a.scales[3];
        const int h = E.hist_left ? 0 : 1;
        double* pl = a.rnode_lsum + 2 * E.node;
        double* cl = a.rnode_lsum + 2 * c;
        cl[2 * h] = hg;
        cl[2 * h + 1] = hh;
        cl[2 * (1 - h)] = pl[0] - hg;
        cl[2 * (1 - h) + 1] = pl[1] - hh;
      }
    }
    // one batch of independent loads: every node's best and children, every leaf's node
    for (int n = tid; n < nn; n += kPlanThreads) {
      const FeatureBest& cb = a.cbest[n];
      const double g = cb.gain;
      const int rf = cb.real_feature, fi = cb.feature;
      const int ex = a.rnode[n].expanded, ch = a.rnode[n].child;
      ng[n] = fi >= 0 ? g : -INFINITY;
      nrf[n] = rf;
      nch[n] = ex ? ch : -1;
      nfi[n] = fi;
    }
    for (int l = tid; l <= s0 && l < L; l += kPlanThreads) tnode[l] = a.leaves[l].frow;
    __syncthreads();
    for (int l = tid; l <= s0 && l < L; l += kPlanThreads) {
      tg[l] = ng[tnode[l]];
      trf[l] = nrf[tnode[l]];
    }
  }
  __syncthreads();
  stamp(17);
  // replay of the sequential order by wave 0: the argmax leaf is split while its node is
  // expanded; its children nodes become leaves w and s + 1
  RegLeaf x;
  int done_w = 0, blocker_w = -1;
  int s_w = s0;
  int draw = rd->bynode_next;  // (per-node sampling: the next draw; wave 0 advances it)
  // (extra_trees: the draws counted so far -- the root scan's row 0 for the first plan, then
  // row 1 -- per feature, in LDS; wave 0 advances and stores them)
  __shared__ int s_xcnt[XT ? kXtLaneFeatures * kWave : 1];
  int* xcnt = s_xcnt;
  if (XT && a.round_xt && tid < kWave) {
    for (int f = lane; f < NF; f += kWave) xcnt[f] = a.xt_cum[(ROOT ? 0 : NF) + f];
  }
  if (tid < kWave && L <= kWave) {
    s_w = ReplayRegs<XT>(a, L, s0, ng, nrf, nch, nfi, tnode, acc, accn, &x, &done_w, &draw, xcnt, &blocker_w);
  } else if (tid < kWave) {
    for (;;) {
      if (s_w >= L - 1) {
        done_w = 1;
        break;
      }
      const int w = WaveArgmaxLeaf(tg, trf, s_w, [](int) { return true; });
      if (!(tg[w] > 0.0)) {
        done_w = 1;
        break;
      }
      const int n = tnode[w], c = nch[n];
      if (c < 0) {
        blocker_w = n;
        break;
      }
      bool refunded = false;
      if (a.round_bynode || a.round_cegb || (XT && a.round_xt)) {
        refunded = DeferAccept<XT>(a, s_w, w, n, c, &draw, ng, nrf, nfi, xcnt, -1, tnode);
      }
      if (lane == 0) {
        const int nl = s_w + 1;
        acc[s_w - s0] = w;
        accn[s_w - s0] = n;
        tnode[w] = c;
        tg[w] = ng[c];
        trf[w] = nrf[c];
        tnode[nl] = c + 1;
        tg[nl] = ng[c + 1];
        trf[nl] = nrf[c + 1];
      }
      WaveLdsSync();
      if (refunded) {  // (refunded leaves' new bests)
        for (int l = lane; l <= s_w + 1; l += kWave) {
          tg[l] = ng[tnode[l]];
          trf[l] = nrf[tnode[l]];
        }
        WaveLdsSync();
      }
      ++s_w;
    }
  }
  if (tid == 0) {
    s_s1 = s_w;
    s_draw = draw;
    if (a.round_bynode) rd->bynode_next = draw;
  }
  if (XT && a.round_xt && tid < kWave) {
    for (int f = lane; f < NF; f += kWave) a.xt_cum[NF + f] = xcnt[f];
  }
  __syncthreads();  // the accepted splits and the leaves' final nodes are in LDS
  const int s1 = s_s1, nacc = s1 - s0;
  stamp(18);
  // wave 0 predicts the next round while the other waves write the records of the accepted
  // splits and of the leaves the replay changed (from their final nodes; a leaf changed twice is
  // written twice with the same record) -- those do not depend on the prediction
  auto accepted_record = [&](int i) {
    if (i < nacc) {
      // an accepted split: its record (the node's best split, its partition counts)
      const int k = i;
      const int n = accn[k];
      const FeatureBest& cb = a.cbest[n];
      const int tl = a.rnode[n].total_left, cnt = a.rnode[n].count;
      SplitRecord& rec = a.rec[s0 + k];
      rec.leaf = acc[k];
      rec.left_count = dp ? cb.lc : tl;
      rec.right_count = dp ? cb.rc : cnt - tl;
      ToDeviceSplit(cb, a.cbest_cat + static_cast<size_t>(n) * kMaxCatWords, &rec.split);
    } else {
      const int i2 = i - nacc;
      const int k = i2 >> 1;
      const int l = (i2 & 1) == 0 ? acc[k] : s0 + k + 1;
      const int n = tnode[l];
      const RNode R = a.rnode[n];
      Leaf lf;
      lf.begin = R.begin;
      lf.count = R.count;
      lf.global_count = dp ? R.st.global_count : R.count;
      lf.depth = R.st.depth;
      lf.slot = R.st.slot;
      lf.buf = R.buf;
      lf.frow = n;
      lf.pad = 0;
      lf.icmask = R.st.icmask;
      lf.sum_g = R.st.sum_g;
      lf.sum_h = R.st.sum_h;
      lf.output = R.st.output;
      lf.lsum_g = a.round_vote ? a.rnode_lsum[2 * n] : 0.0;
      lf.lsum_h = a.round_vote ? a.rnode_lsum[2 * n + 1] : 0.0;
      lf.cmin = R.st.cmin;
      lf.cmax = R.st.cmax;
      a.leaves[l] = lf;
      DeviceSplit* d = &a.best[l];
      if (ng[n] != -INFINITY) ToDeviceSplit(a.cbest[n], a.cbest_cat + static_cast<size_t>(n) * kMaxCatWords, d);
      else NoSplit(d);
    }
  };
  if (tid < kWave) {
    int n = 0;
    if (a.round_predict) {
      n = PredictBottleneck(a, L, s1, (nn - 1) / 2, kround, ng, nch, tnode, blocker_w, T.qkey, T.qn, s_pick, &done_w);
      if (ktr != nullptr) ktr[24] = wall_clock64() - tprev;  // (the prediction alone)
    } else if (L <= kWave) {
      n = PredictRegs(a, L, s1, (nn - 1) / 2, kround, ng, nrf, nch, s_pick, &x, &done_w);
    } else if (!done_w) {
      // the sequential order predicted past the blocker from the splits known so far (copies of
      // the leaf tables): an expanded argmax joins its children, an unexpanded one is needed
      // next -- picked (within round_vmax levels below its leaf) with its children unknown.  The
      // blocker is the first pick.
      // budget: after this round, one expansion per split the tree may still need stays
      // available (each round then accepts at least its first pick, the blocker)
      const int need = L - 1 - s1, used = (nn - 1) / 2;
      int kmax = min(kround, a.round_need_div > 0 ? max(1, need / a.round_need_div) : need);
      kmax = min(kmax, a.round_emax - used - (need - 1));
      kmax = max(kmax, min(1, a.round_emax - used));
      if (kmax <= 0) done_w = 1;  // (unreachable: the budget keeps room for the blocker)
      for (int l = lane; l <= s1; l += kWave) {
        sg[l] = tg[l];
        srf[l] = trf[l];
        snode[l] = tnode[l];
        svd[l] = 0;
      }
      WaveLdsSync();
      const int vmax = (a.round_bynode || a.round_xt || a.round_cegb) ? 0 : a.round_vmax;  // (deferred folds: the current leaves only)
      for (int ss = s1; !done_w && n < kmax && ss < L - 1; ++ss) {
        const int w = WaveArgmaxLeaf(sg, srf, ss, [](int) { return true; });
        if (!(sg[w] > 0.0)) break;
        const int nd = snode[w], c = nch[nd], v = svd[w];
        if (lane == 0) {
          const int nl = ss + 1;
          if (c >= 0) {
            snode[w] = c;
            sg[w] = ng[c];
            srf[w] = nrf[c];
            svd[w] = v + 1;
            snode[nl] = c + 1;
            sg[nl] = ng[c + 1];
            srf[nl] = nrf[c + 1];
            svd[nl] = v + 1;
          } else {
            if (v <= vmax) s_pick[n] = nd;
            sg[w] = -INFINITY;
            srf[w] = -1;
            sg[nl] = -INFINITY;
            srf[nl] = -1;
            snode[nl] = -1;
          }
        }
        if (c < 0 && v <= vmax) ++n;
        WaveLdsSync();
      }
      if (n == 0) done_w = 1;  // (unreachable: the blocker is the first argmax)
    }
    if (lane == 0) {
      s_done = done_w;
      s_nexp = done_w ? 0 : n;
    }
    if constexpr (NT == kWave) {  // (one wave: the records after the prediction)
      for (int i = lane; i < 3 * nacc; i += kWave) accepted_record(i);
    }
  } else {
    for (int i = tid - kWave; i < 3 * nacc; i += NT - kWave) accepted_record(i);
  }
  __syncthreads();
  if (a.round_cegb && a.cegb_coupled != nullptr && !s_done && s_nexp > 1) {
    // CEGB coupled penalties: a pick past the blocker is expanded only if no refund can change
    // its best split, i.e. no feature of the tree the model has not used yet has a remembered
    // candidate that would beat it with its coupled penalty back (the blocker is accepted first
    // in the next replay, before any refund)
    __shared__ int s_unsafe[kMaxRoundExp];
    const int ne = s_nexp;
    if (tid < ne) s_unsafe[tid] = 0;
    __syncthreads();
    for (int i = tid; i < (ne - 1) * NF; i += kPlanThreads) {
      const int j = 1 + i / NF, f = i - (j - 1) * NF;
      if (!a.tree_mask[f] || a.cegb_used[f]) continue;
      const int node = s_pick[j];
      int leaf = -1;
      for (int l = 0; l <= s1 && l < L; ++l) {
        if (tnode[l] == node) leaf = l;
      }
      if (leaf < 0) continue;
      const FeatureBest& m = a.cegb_mem[static_cast<size_t>(leaf) * NF + f];
      const double g = m.gain + a.cegb_coupled[f];
      const int rf = m.feature < 0 ? 0x7fffffff : m.real_feature;
      const int crf = nrf[node] < 0 ? 0x7fffffff : nrf[node];
      if (g > ng[node] || (g == ng[node] && rf < crf)) s_unsafe[j] = 1;
    }
    __syncthreads();
    if (tid == 0) {
      int m = 1;
      for (int j = 1; j < ne; ++j) {
        if (!s_unsafe[j]) s_pick[m++] = s_pick[j];
      }
      s_nexp = m;
    }
    __syncthreads();
  }
  const int nexp = s_nexp;
  if (ktr != nullptr) {
    ktr[22] = nacc;
    ktr[23] = nexp;
  }
  // the next round's expansions, one thread each: independent loads (one round trip) of the
  // node, its best split, the split feature's record and interaction mask
  const int next_frow = nn;
  const int nbuf = a.round_vmax + 2;
  const int nent = s_done ? 0 : nexp;
  for (int it = tid; it < nent; it += kPlanThreads) {
    {
      const int j = it, node = s_pick[j];
      const int fi = nfi[node];
      const RNode P = a.rnode[node];
      const FeatureBest& cb = a.cbest[node];
      const double lsg = cb.lg, lsh = cb.lh, lo = cb.lo;
      const double rsg = cb.rg, rsh = cb.rh, ro = cb.ro;
      const int lcnt = cb.lc, rcnt = cb.rc, mono = cb.mono, iscat = cb.ncat > 0 ? 1 : 0;
      const IcMask fmask = a.feat_icmask != nullptr ? a.feat_icmask[fi] : kIcAll;
      ExpPlan& e = s_e[j];
      e.feat = a.feat[fi];
      ToDeviceSplit(cb, a.cbest_cat + static_cast<size_t>(node) * kMaxCatWords, &e.split);
      s_pc[j] = P.count;
      const int hl = lcnt <= rcnt ? 1 : 0;
      e.node = node;
      e.part_begin = P.begin;
      e.part_count = P.count;
      e.src_buf = P.buf;
      e.dst_buf = P.buf + 1 == nbuf ? 0 : P.buf + 1;
      e.hist_left = hl;
      e.slot_parent = P.st.slot;
      e.slot_new = next_slot + j;
      // (per-node sampling: the picked leaf's id -- its row of the reference's flags)
      int fp = node;
      if (a.leaf_rows != nullptr) {
        for (int l = 0; l <= s1 && l < L; ++l) {
          if (tnode[l] == node) fp = l;
        }
      }
      e.frow_parent = fp;
      e.frow_child[0] = next_frow + 2 * j;
      e.frow_child[1] = next_frow + 2 * j + 1;
      // children's statistics from the split (basic monotone constraints: the mid-point bound)
      const int depth = P.st.depth + 1;
      double pmin = P.st.cmin, pmax = P.st.cmax, rmin = P.st.cmin, rmax = P.st.cmax;
      if (!iscat) {
        const double mid = (lo + ro) / 2.0f;
        if (mono < 0) {
          pmin = fmax(pmin, mid);
          rmax = fmin(rmax, mid);
        } else if (mono > 0) {
          pmax = fmin(pmax, mid);
          rmin = fmax(rmin, mid);
        }
      }
      const IcMask icm = P.st.icmask & fmask;
      ChildStats lc, rc;
      lc.sum_g = lsg;
      lc.sum_h = lsh;
      lc.output = lo;
      lc.cmin = pmin;
      lc.cmax = pmax;
      lc.global_count = lcnt;
      lc.depth = depth;
      lc.slot = hl ? e.slot_new : P.st.slot;
      lc.leaf = P.st.leaf == 0 ? 0 : -1;  // (ids come with the replay; leaf 0 is the all-left path: ScanParentOutput)
      lc.frow = e.frow_child[0];
      lc.icmask = icm;
      rc.sum_g = rsg;
      rc.sum_h = rsh;
      rc.output = ro;
      rc.cmin = rmin;
      rc.cmax = rmax;
      rc.global_count = rcnt;
      rc.depth = depth;
      rc.slot = hl ? P.st.slot : e.slot_new;
      rc.leaf = -1;
      rc.frow = e.frow_child[1];
      rc.icmask = icm;
      e.lr[0] = lc;
      e.lr[1] = rc;
      a.rnode[node].expanded = 1;
      a.rnode[node].child = e.frow_child[0];
      RNode C;
      C.begin = C.count = 0;  // (set by the next plan, from the partition counts)
      C.buf = e.dst_buf;
      C.expanded = 0;
      C.child = -1;
      C.total_left = 0;
      C.st = lc;
      s_c[2 * j] = C;
      C.st = rc;
      s_c[2 * j + 1] = C;
    }
  }
  stamp(19);
  if (s_done) {
    if (tid == 0) {
      rd->done = 1;
      rd->nsplit = s1;
      rd->nexp = 0;
      rd->accepted_max = max(accmax0, nacc);
    }
    if (a.host_out != nullptr) {
      __syncthreads();  // (this plan's records are written)
      HostTreeOut(a, s1, rounds0, nn, s_draw);
    }
    return;
  }
  __syncthreads();
  stamp(20);
  if (tid < kWave) {
    // row blocks: one size for the round (at least blk_min_rows, at most the packed headroom),
    // one lane per expansion
    const int pcj = lane < nexp ? s_pc[lane] : 0;
    const unsigned urows = static_cast<unsigned>(WaveSum(pcj));
    // balanced over the grid: the smallest m with blocks of ceil(rows / (m * grid - nexp))
    // rows under the packed headroom; every workgroup then takes m blocks at most (one
    // partial block per expansion rounds up)
    // (the smallest m with ceil(rows / (m g - nexp)) <= cap, i.e. m g - nexp >= ceil(rows / cap);
    // rows and cap are below 2^31, so every dividend fits 32 unsigned bits: no 64-bit divisions)
    const unsigned g = static_cast<unsigned>(max(1, a.round_grid)), cap = static_cast<unsigned>(a.hist_rows_cap);
    const unsigned unexp = static_cast<unsigned>(nexp);
    const unsigned need = (urows + cap - 1u) / cap + unexp;
    const unsigned m = g <= unexp ? 1u : max(1u, (need + g - 1u) / g);
    long long rpb = m * g > unexp ? (urows + m * g - unexp - 1u) / (m * g - unexp) : cap;
    rpb = max(rpb, static_cast<long long>(a.blk_min_rows));
    rpb = min(rpb, static_cast<long long>(cap));
    rpb = max(rpb, 1ll);
    const unsigned rpb32 = static_cast<unsigned>(rpb);  // (32-bit divisions: a 64-bit one is a long call)
    const int nb = lane < nexp ? static_cast<int>((static_cast<unsigned>(pcj) + rpb32 - 1u) / rpb32) : 0;
    const int incl = WavePrefixIncl(nb);
    if (lane < nexp) {
      s_e[lane].blk_off = incl - nb;
      s_e[lane].nblk = nb;
    }
    if (lane == kWave - 1) {
      rd->rpb = static_cast<int>(rpb);
      rd->nblk = incl;
      rd->nexp = nexp;
      rd->nsplit = s1;
      rd->next_slot = next_slot + nexp;
      rd->next_frow = next_frow + 2 * nexp;
      rd->round = ROOT ? 1 : round0 + 1;  // (parity 0 of the first round holds the root histogram)
      rd->rounds = rounds0 + 1;
      rd->accepted_max = max(accmax0, nacc);
    }
  }
  if (tid < kMaxRoundExp) {
    rd->cur[tid][0] = rd->cur[tid][1] = 0;
    rd->loc_acc[tid][0] = rd->loc_acc[tid][1] = 0ull;
  }
  __syncthreads();
  // the plans and the children's nodes (contiguous from next_frow) in 8-byte words; a plan's
  // category set only when its split is categorical (the split kernel reads it only then)
  {
    constexpr int kEW = sizeof(ExpPlan) / 8, kCW = sizeof(RNode) / 8;
    static_assert(sizeof(ExpPlan) % 8 == 0 && sizeof(RNode) % 8 == 0, "8-byte words");
    // (the words lying wholly inside the category set: its offset need not be 8-aligned)
    constexpr int kCatOff = __builtin_offsetof(ExpPlan, split) + __builtin_offsetof(DeviceSplit, cat_bits);
    constexpr int kCat0 = (kCatOff + 7) / 8;
    constexpr int kCat1 = (kCatOff + 4 * kMaxCatWords) / 8;
    for (int i = tid; i < nexp * kEW; i += kPlanThreads) {
      const int j = i / kEW, w = i - j * kEW;
      if (w >= kCat0 && w < kCat1 && !s_e[j].split.is_categorical) continue;
      reinterpret_cast<unsigned long long*>(&rd->e[j])[w] = reinterpret_cast<const unsigned long long*>(&s_e[j])[w];
    }
    unsigned long long* cdst = reinterpret_cast<unsigned long long*>(a.rnode + next_frow);
    for (int i = tid; i < 2 * nexp * kCW; i += kPlanThreads) cdst[i] = reinterpret_cast<const unsigned long long*>(s_c)[i];
  }
  stamp(21);
}

}  // namespace dev
}  // namespace lgbm_amd
