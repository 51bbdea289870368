// Round growth, stages 2 and 3 (round_common.h): the split scans k_round_find, the distributed
// fold k_round_childbest and the plan kernel k_round_plan.
#include "round_plan.h"

namespace lgbm_amd {
namespace dev {

// ----------------------------------------------------------------------------- k_round_find
template <int KIND, int NT>
struct RoundFindShared {
  ScanShared<KIND, NT> scan;
  ArgC arg[NT / kWave];  // ChildBest's per-wave winners
};

// the best split of child y (2j + lr) of the round, node `node`, from its per-feature
// results, by the child's last split-scan workgroup (SplitInfo order: larger gain, then
// smaller real feature)
// (inline: as RoundPlanBody)
template <int KIND, int NT>
__device__ inline void ChildBest(const KArgs& a, int y, int node, RoundFindShared<KIND, NT>& sh) {
  const int NF = a.p.num_features, tid = threadIdx.x;
  const FeatureBest* fb0 = a.feat_best;
  constexpr int kB = 8;
  ArgC c = ArgNone();
#pragma unroll 1
  for (int i0 = tid; i0 < NF; i0 += kB * NT) {
    double cg[kB];
    int crf[kB], cf[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      const int i = i0 + k * NT;
      cf[k] = -1;
      if (i < NF) {
        const FeatureBest& r = fb0[RoundFbIndex(a, y, i)];
        cg[k] = r.gain;
        crf[k] = r.real_feature;
        cf[k] = r.feature;
      }
    }
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      if (cf[k] >= 0 && (c.idx < 0 || SplitBetter(cg[k], crf[k], c.g, c.rf))) {
        c.g = cg[k];
        c.rf = crf[k];
        c.idx = i0 + k * NT;
      }
    }
  }
  c = ArgWaveBest(c);
  if ((tid & 63) == 0) sh.arg[tid >> 6] = c;
  __syncthreads();
  ArgC b = sh.arg[0];
#pragma unroll
  for (int k = 1; k < NT / kWave; ++k) ArgTake(&b, sh.arg[k]);
  const size_t ci = static_cast<size_t>(node);
  FeatureBest* dst = a.cbest + ci;
  // (write-through: with KArgs::plan_in_find another workgroup of this launch plans from them)
  if (tid == 0) {
    if (b.idx >= 0 && b.g != -INFINITY) {
      const size_t wi = RoundFbIndex(a, y, b.idx);
      const FeatureBest w = fb0[wi];
      PublishRecord(dst, w);
      if (w.ncat > 0) {
        PublishCatCopy(a.cbest_cat + ci * kMaxCatWords, a.feat_cat + wi * kMaxCatWords);
      }
    } else {
      PublishRecord(dst, FeatureBestNone());
    }
  }
}

// split scan of one (feature, child of expansion j): grid (num_scan or categorical features,
// 2 x round_k); child y = 2j + lr (0 left, 1 right).  The histogrammed child takes the
// expansion's reduced histogram (or sums its few partials itself) into its new slot; the
// other one subtracts it from the parent's slot in place (exact int64).  Children of an
// expansion that cannot be split (max_depth, min_data_in_leaf) are not scanned.
template <int KIND, bool SIMPLE, int NT, bool VG = false, bool PIF = true>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT == kWave ? LGBM_FIND_WAVE_OCC : 1))) void k_round_find(KArgs a) {
  constexpr bool CAT = KIND >= 2;  // (3: the wide categorical variant)
  extern __shared__ double s_bins[];  // [2][max_feature_bins] dequantised (g, h), if they fit
  __shared__ RoundFindShared<KIND, NT> sh;
  __shared__ int s_last;
  Round* rd = a.rd;
  const long long t_entry = a.ktrace != nullptr ? wall_clock64() : 0;
  const int by = static_cast<int>(blockIdx.y);
  const int y = by, j = y >> 1, lr = y & 1;
  // voting-parallel rounds (KArgs::round_vote): Params::vote_phase 1 scans every feature on this
  // rank's histograms, sums and counts; 2 scans the features the vote elected for child y
  // (KArgs::vote_list) on their all-reduced histograms (KArgs::vote_hist)
  // (VG: the global scan is an instantiation of its own -- a run-time flag put the elected
  // feature's load in front of every scan's feature load: +10% on wide data)
  const bool vote_local = a.round_vote && a.p.vote_phase == 1;
  constexpr bool vote_global = VG;
  int f = CAT ? a.cat_list[blockIdx.x] : (a.feat_list != nullptr ? a.feat_list[blockIdx.x] : static_cast<int>(blockIdx.x));
  if constexpr (VG) f = a.vote_list[y * a.p.vote_k + blockIdx.x];
  const bool vote_empty = f < 0;  // (an empty elected slot, or a padded owner slot)
  if (vote_empty) f = 0;
  const int tid = threadIdx.x;
  const int NF = a.p.num_features;
  const int units = a.hist_units;
  // the round record, the expansion's plan and the feature in one batch of loads, the
  // finished-tree check included (it used to cost a round trip of its own)
  const int done = rd->done, nexp = rd->nexp, rround = rd->round;
  const ExpPlan& E = rd->e[j];
  const int pc = E.part_count, tl = rd->cur[j][0];
  const int e_gl0 = E.lr[0].global_count, e_gl1 = E.lr[1].global_count, e_hl = E.hist_left;
  const int e_slot_new = E.slot_new, e_slot_parent = E.slot_parent, e_frow = E.frow_child[lr];
  const int e_frow_parent = E.frow_parent, blk_off = E.blk_off, e_nblk = E.nblk;
  const ChildStats cl = E.lr[lr];
  const Feature F = a.feat[f];
  const int8_t tree_used = a.tree_mask[f];
  if (done) return;
  if (a.ktrace != nullptr && blockIdx.x == 0 && by == 0 && threadIdx.x == 0 && rround < a.p.num_leaves) {
    a.ktrace[static_cast<size_t>(rround) * kTraceSlots + 25] = wall_clock64();
  }
  const int parity = rround & 1;
  const int nbf = F.num_bin - F.offset;
  const double ig = a.scales[2], ih = a.scales[3];
  // LGBM_AMD_KTRACE: the planning workgroup's own path through the scan (slots 26..31: entry,
  // inputs loaded, histogram staged, scan done, child's arrival, child's fold done)
  const bool ktw = a.ktrace != nullptr && tid == 0 && rround < a.p.num_leaves;
  long long kt[6] = {0, 0, 0, 0, 0, 0};
  if (ktw) {
    kt[0] = t_entry;
    kt[1] = wall_clock64();
  }
  // this feature's bins of expansion j's reduce buffer for the next round (every expansion
  // slot: the next round may use any)
  const bool dp = a.p.data_parallel != 0;
  const bool owner = dp && !a.round_vote;  // (data-parallel: reduce-scattered to the feature owners)
  if (!CAT && lr == 0 && !owner && !vote_global) {
    long long* nxt = RoundScratch(a, parity + 1, j);
    for (int i = tid; i < 2 * nbf; i += NT) nxt[2 * F.hist_offset + i] = 0;
  }
  if (!CAT && owner && a.round_send != nullptr) {
    // data-parallel: the next round's owner-major send buffer, cleared by every workgroup's
    // share (this round's reduce-scatter has read it) -- no memset node per round
    const size_t total = static_cast<size_t>(a.p.world) * a.round_k * a.rs_block * 2;
    const size_t nwg = static_cast<size_t>(gridDim.x) * gridDim.y;
    const size_t per = (total + nwg - 1) / nwg;
    const size_t b0 = (static_cast<size_t>(by) * gridDim.x + blockIdx.x) * per;
    const size_t b1 = min(total, b0 + per);
    for (size_t i = b0 + tid; i < b1; i += NT) a.round_send[i] = 0;
  }
  if (j >= nexp || vote_empty) return;
  if (vote_global && CAT && !F.is_cat) return;  // (an elected numerical feature)
  // data-parallel: the children's global counts from the split's estimates (reference
  // data_parallel_tree_learner.cpp: global leaf counts from the SplitInfo)
  const int lc = dp ? e_gl0 : tl, rc = dp ? e_gl1 : pc - tl;
  const int md = SkipMinData(a);
  const bool skip = (a.p.max_depth > 0 && cl.depth >= a.p.max_depth) || (lc < 2 * md && rc < 2 * md);
  const bool is_hist = (lr == 0) == (e_hl != 0);
  const int slot = is_hist ? e_slot_new : e_slot_parent;
  const int frow = e_frow;
  const int nblk = a.round_fused ? e_nblk : RoundHistBlocks(a, rd, j);
  // (per-node sampling: the parent leaf's row of the reference's flags, KArgs::leaf_rows)
  // (voting: every feature is scanned and its local histogram built -- the vote may elect a
  // feature the parent's local scan could not split, whose local histogram the reference's
  // learner would not have built (VotingParallelTreeLearner::FindBestSplits builds the tree's
  // sample minus those, then copies the elected ones' histograms))
  const int8_t parent_flag = a.leaf_rows != nullptr ? a.leaf_rows[static_cast<size_t>(e_frow_parent) * NF + f]
                                                    : a.splittable[static_cast<size_t>(e_frow_parent) * NF + f];
  const int8_t parent_ok = a.round_vote ? 1 : parent_flag;
  FeatureBest* fb_out = &a.feat_best[RoundFbIndex(a, y, f)];
  int8_t* flags = a.splittable + static_cast<size_t>(frow) * NF;
  const SplitParams& p = a.p.sp;
  FeatureBest o = FeatureBestEmpty();
  bool write = true;
  if (KIND == 1 && F.is_cat) {
    write = false;  // the categorical kernel scans it
  } else if (skip) {
    // (both children keep gain -inf: never split)
  } else if (tree_used && !parent_ok) {
    // the parent could not split on f: neither child evaluates it (SerialTreeLearner::FindBestSplits)
    if (tid == 0) flags[f] = 0;
    o.flag = 0;
  } else if (tree_used && (!F.is_cat || F.num_bin <= kFindMaxCatBins)) {
    // interaction constraints: like a sampled-out feature, a disallowed one is not evaluated
    // but keeps its histogram (descendants subtract it); voting's local scan evaluates it (its
    // features are the tree's sample and the parent's flags only)
    bool used = true;
    if (a.feat_icmask != nullptr && !vote_local && !IcAny(cl.icmask & a.feat_icmask[f])) used = false;
    LeafCtx L;
    L.sg = cl.sum_g;
    L.sh = cl.sum_h + 2 * kEpsilon;
    L.n = lr == 0 ? lc : rc;
    L.c.min = cl.cmin;
    L.c.max = cl.cmax;
    L.parent_out = ScanParentOutput(cl.leaf == 0, cl.output, cl.sum_g, cl.sum_h, L.n, L.c, p);
    if (vote_local) {
      // this rank's rows of the child: the histogrammed child's sums from k_round_split, the
      // other one's as the parent's minus those (loaded here only: the extra loads in the
      // common batch cost the narrow one-wave scans of wide data ~20%)
      const unsigned long long loc0 = rd->loc_acc[j][0], loc1 = rd->loc_acc[j][1];
      const double pl_g = a.rnode_lsum[2 * E.node], pl_h = a.rnode_lsum[2 * E.node + 1];
      const double hg = static_cast<double>(static_cast<long long>(loc0)) * ig;
      const double hh = static_cast<double>(static_cast<long long>(loc1)) * ih;
      L.sg = is_hist ? hg : pl_g - hg;
      L.sh = (is_hist ? hh : pl_h - hh) + 2 * kEpsilon;
      L.n = lr == 0 ? tl : pc - tl;
    }
    const int nh = 2 * a.p.total_bins;
    long long* dst = vote_global ? a.vote_hist + static_cast<size_t>(y * a.p.vote_k + blockIdx.x) * 2 * a.p.max_feature_bins
                                 : a.hist + static_cast<size_t>(slot) * nh + 2 * F.hist_offset;
    const long long* src = vote_global ? dst
                           : owner ? a.round_owned + 2 * (static_cast<size_t>(j) * a.rs_block + a.owned_off[f])
                                   : RoundScratch(a, parity, j) + 2 * F.hist_offset;
    const size_t pstride = static_cast<size_t>(units) * a.p.total_bins;
    const unsigned long long* part = a.partials + static_cast<size_t>(blk_off) * pstride + static_cast<size_t>(units) * F.hist_offset;
    const bool stage = a.p.max_feature_bins <= kFindLdsBins;
    double* sg = s_bins;
    double* shv = s_bins + (stage ? a.p.max_feature_bins : 0);
    const bool subtract = !is_hist && !vote_global;
    const int nblk_direct = (!owner && !vote_global && nblk <= kDirectChunk) ? nblk : -1;
    // (the voting global scan reads the all-reduced bins in place and stores nothing back)
    StageHistogram<NT, !VG>(dst, src, part, pstride, units, nbf, nblk_direct, subtract, ig, ih, stage, sg, shv,
                            sh.scan.s_red);
    if (ktw) kt[2] = wall_clock64();
    if (used) {
      FinishLeafCtx(&L, p);
      o.feature = f;
      o.real_feature = F.real_index;
      HistView hv;
      hv.lg = stage ? sg : nullptr;
      hv.lh = stage ? shv : nullptr;
      hv.h = dst;
      hv.inv_g = ig;
      hv.inv_h = ih;
      bool splittable;
      if constexpr (!CAT) {
        if (a.round_xt) {  // (extra_trees: the prefixes the replay evaluates its drawn thresholds from)
          XtStorePrefix<NT>(F, hv, L, a.node_pre + static_cast<size_t>(frow) * a.p.total_bins + F.hist_offset,
                            &sh.scan.ssc);
        }
      }
      if constexpr (CAT) {
        splittable = FindCategoricalBlock(F, hv, L, p, &o, a.feat_cat + RoundFbIndex(a, y, f) * kMaxCatWords,
                                          &sh.scan.sc, &sh.scan.cat_sc);
      } else {
        splittable = FindNumericalBlock<SIMPLE, NT>(F, hv, L, p, cl.depth, a.p.monotone_penalty, &o, &sh.scan.sc,
                                                    &sh.scan.ssc, sh.scan.sc2, kNoRandThr);
      }
      if (tid == 0 && !vote_global) {  // (voting: the local scan's flags; categorical: thread 0 decides)
        flags[f] = splittable ? 1 : 0;
        o.flag = splittable ? 1 : 0;
      }
      // CEGB (GPUTreeLearner::CegbRounds: no refunds in a round tree), before the monotone
      // penalty as SerialTreeLearner::ComputeBestSplitForFeature
      if (a.p.cegb && !a.round_cegb) {  // (KArgs::round_cegb: the replay subtracts them)
        o.gain -= CegbScanDelta(a, f, L.n);
      }
      if (!CAT && !SIMPLE && F.monotone != 0) o.gain *= MonotonePenalty(cl.depth, a.p.monotone_penalty);
      if (o.gain == -INFINITY) o.feature = -1;
    }
  }
  if (ktw) kt[3] = wall_clock64();
  if (write && tid == 0) {
    PublishRecord(fb_out, o);
    if (a.node_fb != nullptr) PublishRecord(&a.node_fb[static_cast<size_t>(frow) * NF + f], o);
  }
  if constexpr (CAT) {
    // (per-node sampling: the category set kept per node, from this scan's slot)
    if (write && a.node_fb_cat != nullptr && a.node_cat_slot[f] >= 0) {
      __syncthreads();
      if (tid == 0 && o.ncat > 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        PublishCatCopy(a.node_fb_cat + (static_cast<size_t>(frow) * a.node_cat_slots + a.node_cat_slot[f]) * kMaxCatWords,
                       a.feat_cat + RoundFbIndex(a, y, f) * kMaxCatWords);
      }
    }
  }
  // (distributed: the results are gathered from every rank first, k_round_childbest folds them)
  if (KIND == 1 || a.round_dist) return;  // (the categorical kernel counts the arrivals)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ArrivalRelease();
  __syncthreads();
  // arrival: the child's last workgroup folds the child's per-feature results
  if (tid == 0) {
    if (ktw) kt[4] = wall_clock64();
    const unsigned nwg = gridDim.x;
    uint32_t* cc = a.child_cnt + static_cast<size_t>(y) * (kFindSub + 1) * kFindSubStride;
    int last = 0;
    if (nwg <= kRoundFlatMax) {
      if (atomicAdd(cc, 1u) == nwg - 1) {
        last = 1;
        *cc = 0u;  // (every other workgroup of the child has counted)
      }
    } else {
      const unsigned g = blockIdx.x % kFindSub;
      const unsigned members = (nwg - g + kFindSub - 1) / kFindSub;
      uint32_t* sub = cc + g * kFindSubStride;
      if (atomicAdd(sub, 1u) == members - 1) {
        *sub = 0u;
        uint32_t* top = cc + kFindSub * kFindSubStride;
        if (atomicAdd(top, 1u) == kFindSub - 1) {
          last = 1;
          *top = 0u;
        }
      }
    }
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  ChildBest<KIND, NT>(a, y, frow, sh);
  if (ktw) kt[5] = wall_clock64();
  // (PIF: an instantiation without the plan when the plan has its own kernel -- the replay's
  // registers otherwise set the occupancy of every scan workgroup)
  if (!PIF || !a.plan_in_find) return;
  // the last child of the round to finish plans the next round (its scans' results were
  // published write-through; one agent-scope acquire)
  if (!LastOfCount(&rd->child_done, 2u * static_cast<unsigned>(nexp), &s_last)) return;
  if (ktw) {
    for (int k = 0; k < 6; ++k) a.ktrace[static_cast<size_t>(rround) * kTraceSlots + 26 + k] = kt[k];
#if LGBM_FIND_PHASES
    for (int k = 0; k < 4; ++k) a.ktrace[static_cast<size_t>(rround) * kTraceSlots + 12 + k] = g_find_phase[k];
#endif
  }
  if constexpr (PIF) RoundPlanBody<false, NT>(a, reinterpret_cast<unsigned char*>(s_bins));
}

// (XT: the extra_trees replay's instantiation, launched only with KArgs::round_xt -- its
// registers and stack would slow every other plan)
template <bool ROOT, bool XT>
__global__ __launch_bounds__(kPlanThreads) void k_round_plan(KArgs a) {
  extern __shared__ unsigned char plan_lds[];
  if (a.rd->done) return;
  RoundPlanBody<ROOT, kPlanThreads, XT>(a, plan_lds);
}

namespace {
template <bool ROOT>
void LaunchRoundPlan(const KArgs& a, hipStream_t s) {
  const size_t lds = RoundPlanLds(a.p.num_leaves, a.round_nodes);
  if (a.round_xt) hipLaunchKernelGGL((k_round_plan<ROOT, true>), dim3(1), dim3(kPlanThreads), lds, s, a);
  else hipLaunchKernelGGL((k_round_plan<ROOT, false>), dim3(1), dim3(kPlanThreads), lds, s, a);
}
}  // namespace

size_t RoundPlanLds(int num_leaves, int nodes) {
  const size_t L = static_cast<size_t>(num_leaves), N = static_cast<size_t>(nodes);
  return (2 * N + 2 * L) * sizeof(double) + N * sizeof(int) * 4 + L * sizeof(int) * 7;
}

namespace {

template <bool VG, bool PIF>
void LaunchRoundFindT(const KArgs& a, hipStream_t s) {
  const int ny = 2 * a.round_k;
  size_t lds = FindBinsLds(a);
  if (a.plan_in_find) lds = std::max(lds, RoundPlanLds(a.p.num_leaves, a.round_nodes));
  // (voting global scan: every elected slot, numerical or categorical, in both kernels)
  const int ncat = (a.round_vote && a.p.vote_phase == 2) ? a.num_scan : a.p.has_cat;
  DispatchScans(a, [&](auto kind, auto simple, auto nt) {
    hipLaunchKernelGGL((k_round_find<kind(), simple(), nt(), VG, PIF>), dim3(kind() >= 2 ? ncat : a.num_scan, ny),
                       dim3(nt()), lds, s, a);
  });
}

void LaunchRoundFind(const KArgs& a, hipStream_t s) {
  if (a.round_vote && a.p.vote_phase == 2) LaunchRoundFindT<true, false>(a, s);
  else if (a.plan_in_find) LaunchRoundFindT<false, true>(a, s);
  else LaunchRoundFindT<false, false>(a, s);
}

}  // namespace

// distributed rounds: each child's best split from the gathered per-feature results; the last
// child to finish plans the next round (as k_round_find's last workgroup does on one process),
// so the gather is followed by one launch instead of a fold and a plan kernel
__global__ __launch_bounds__(kFindThreads) void k_round_childbest(KArgs a) {
  __shared__ RoundFindShared<0, kFindThreads> sh;
  __shared__ int s_last;
  extern __shared__ unsigned char plan_lds[];
  // every workgroup counts, an idle one too: the plan rewrites Round::nexp / done, so it may run
  // only once no workgroup of this launch can still read them (a workgroup dispatched late --
  // the GPU shared with other ranks' kernels -- would otherwise take the next round's nexp)
  Round* rd = a.rd;
  const int done = rd->done, nexp = rd->nexp;
  const int y = blockIdx.x;
  if (!done && y < 2 * nexp) {
    const int node = rd->e[y >> 1].frow_child[y & 1];
    ChildBest<0, kFindThreads>(a, y, node, sh);
    // deferred folds (per-node sampling, CEGB): every rank's copy of the child's per-feature
    // results and flags, from the gathered records (each rank scanned only its own features)
    if (a.round_dist && !a.round_vote && (a.node_fb != nullptr || a.leaf_rows != nullptr)) {
      const int NF = a.p.num_features;
      typedef __attribute__((address_space(1))) int8_t GlobalI8;
      for (int f = threadIdx.x; f < NF; f += blockDim.x) {
        if (!a.tree_mask[f]) continue;  // (no owner this tree)
        const size_t wi = RoundFbIndex(a, y, f);
        const FeatureBest r = a.feat_best[wi];
        if (a.node_fb != nullptr) PublishRecord(&a.node_fb[static_cast<size_t>(node) * NF + f], r);
        if (r.flag >= 0) {
          __hip_atomic_store((GlobalI8*)(a.splittable + static_cast<size_t>(node) * NF + f), static_cast<int8_t>(r.flag),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (a.node_fb_cat != nullptr && a.node_cat_slot[f] >= 0 && r.ncat > 0) {
          PublishCatCopy(a.node_fb_cat + (static_cast<size_t>(node) * a.node_cat_slots + a.node_cat_slot[f]) * kMaxCatWords,
                         a.feat_cat + wi * kMaxCatWords);
        }
      }
    }
  }
  if (!LastOfCount(&rd->child_done, gridDim.x, &s_last) || done) return;
  RoundPlanBody<false, kFindThreads>(a, plan_lds);
}

void PrepareRoundKernels(int max_lds) {
  PrepareRoundSplitKernels(max_lds);
  // the plans' node tables (RoundPlanLds) pass 64 KiB from ~400 leaves
  AllowLds(k_round_plan<true, false>, max_lds);
  AllowLds(k_round_plan<false, false>, max_lds);
  AllowLds(k_round_plan<true, true>, max_lds);
  AllowLds(k_round_plan<false, true>, max_lds);
  AllowLds(k_round_childbest, max_lds);
}

void RoundRootPlan(const KArgs& a, hipStream_t s) {
  LaunchRoundPlan<true>(a, s);
}

void RoundStep(const KArgs& a, hipStream_t s) {
  RoundSplitReduce(a, s);
  RoundFind(a, s);
  if (!a.plan_in_find) {
    LaunchRoundPlan<false>(a, s);
  }
}

void RoundFind(const KArgs& a, hipStream_t s) { LaunchRoundFind(a, s); }

void RoundFindElected(const KArgs& a, hipStream_t s) { LaunchRoundFind(a, s); }  // (a: vote_phase 2, num_scan vote_k)

void RoundChildBestAndPlan(const KArgs& a, hipStream_t s) {
  static_assert(kPlanThreads == kFindThreads, "the fold's workgroup runs the plan");
  hipLaunchKernelGGL(k_round_childbest, dim3(2 * a.round_k), dim3(kFindThreads), RoundPlanLds(a.p.num_leaves, a.round_nodes),
                     s, a);
}

}  // namespace dev
}  // namespace lgbm_amd
