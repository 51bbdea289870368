// The device learner's growth-mode rules (growth_plan.h).
#include "growth_plan.h"

#include <algorithm>
#include <sstream>

#include "cegb.h"
#include "lgbm_amd/json.h"
#include "lgbm_amd/split_info.h"

namespace lgbm_amd {

namespace {

// lazy CEGB penalties keep a paid bitset of one bit per (row, feature)
constexpr int kCegbLazyMaxFeatures = 8192;
// the extra_trees replay counts its draws in four 64-lane words
constexpr int kXtReplayMaxFeatures = 4 * 64;
// per-node tables of round growth: the nodes' category sets / the extra_trees prefix tables
constexpr double kNodeCatSetsMaxBytes = 2.0 * (1ull << 30);
constexpr double kXtPrefixMaxBytes = 8.0 * (1ull << 30);

}  // namespace

GrowthPlan PlanGrowth(const Config& c, const GrowthFacts& f) {
  GrowthPlan p;
  const bool distributed = f.distributed(), voting = f.voting(), any_cat = f.any_categorical();
  const bool bynode = c.feature_fraction_bynode < 1.0;
  const auto& ic = c.interaction_constraints_vector;
  const bool any_mono = std::any_of(c.monotone_constraints.begin(), c.monotone_constraints.end(),
                                    [](int8_t m) { return m != 0; });
  // intermediate monotone constraints re-bound leaves all over the tree after a split: the pick
  // walks the tree and the next split scan re-scans the re-bounded leaves
  const bool mono_inter = c.monotone_constraints_method == "intermediate" && any_mono;
  const bool cegb = CostEffectiveGB::Enabled(c);
  const bool cegb_coupled = !c.cegb_penalty_feature_coupled.empty();
  const bool cegb_lazy = !c.cegb_penalty_feature_lazy.empty();
  const bool forced = f.forced != ForcedSplits::kNone;

  // ---- residency: host-assisted when any rule holds (the first one is the reason logged)
  auto host = [&p](bool rule, const char* reason) {
    if (rule && p.device_resident) {
      p.device_resident = false;
      p.reason = reason;
    }
  };
  host(f.force_host, "forced");
  host(f.max_cat_bins > f.limits.max_cat_bins, "a categorical feature has more bins than the device scan takes");
  // (the distributed learners keep categorical extra_trees draws in the host loop; voting is one of them)
  host(c.extra_trees && any_cat && distributed, "extra_trees with categorical features on a distributed learner");
  host(ic.size() > static_cast<size_t>(f.limits.max_ic_constraints), "more interaction constraints than the device masks hold");
  host(mono_inter && (distributed || c.extra_trees || forced || c.num_leaves > f.limits.mono_inter_max_leaves),
       "intermediate monotone constraints with a distributed learner, extra_trees, forced splits or too many leaves");
  // (feature-parallel gathers the owners' forced records; data-parallel rejects forced splits as
  // the reference does, voting keeps them in its host loop)
  host(forced && ((distributed && !f.forced_gathered()) || f.forced == ForcedSplits::kRefused),
       "forced splits on a distributed learner that does not gather them, or without a device schedule");
  host(distributed && f.dist_host_assist && (bynode || cegb), "LGBM_AMD_DIST_HOST_ASSIST with per-node sampling or CEGB");
  host(cegb && cegb_lazy && (distributed || f.num_features > kCegbLazyMaxFeatures),
       "lazy CEGB penalties on a distributed learner or with too many features");
  p.mono_inter = mono_inter && p.device_resident;
  p.cegb = cegb && p.device_resident;

  // ---- the initial round width (LGBM_AMD_ROUND_K, 1 = one split per step)
  // Without LGBM_AMD_ROUND_K the width adapts per tree (RunRounds): 8 while the last tree's
  // speculation was accepted (expansions <= splits + 2: early trees), else 6 (A/B at 300
  // iterations of the headline, profiles/r04_round_width.md: K=8 saves 2 rounds on the first
  // trees for 2 more expansions, later it adds 8-10 unaccepted ones; fixed K 6 / 8 / 10 =
  // 2.040 / 2.072 / 2.132 ms, window of 20 after 5: 2.148 / 2.075)
  // Below 4M rows per rank the width stays 8: a round there is latency-bound and the extra
  // speculation is nearly free (r04_round_width.md: 1.25M / 2.5M rows 0.929 / 1.106 ms fixed
  // vs 0.943 / 1.120 adaptive; Epsilon 8.28 vs 8.44 ms, Bosch / LTR shapes equal)
  // (the rows per rank are averaged over the ranks at the first tree, RunRounds: every rank
  // must plan with the same width)
  // Trees of 90 leaves or more run num_leaves / 10 expansions per round (at most 16), fixed:
  // at 255 leaves width 16 halves the rounds per tree (41 -> 23) and saves 11-22% per
  // iteration on every 255-leaf shape measured (config #2 at 255 / 63 / 15 bins, the five
  // config #3 workloads; the same trees); at 127 leaves width 12 beats 8 and 16 (2.73 vs 2.88
  // / 2.80 ms: profiles/r06_round_width_255.md)
  p.round_width = tuning::kRoundWidth;
  p.width_adapts = true;
  if (c.num_leaves / tuning::kRoundLeavesPerWidth > tuning::kRoundWidth) {
    p.round_width = c.num_leaves / tuning::kRoundLeavesPerWidth;
    p.width_adapts = false;
  }
  if (f.has_round_k_knob) {
    p.round_width = f.round_k_knob;
    p.width_adapts = false;
  }
  p.round_width = std::max(1, std::min(f.limits.max_round_exp, p.round_width));
  const int width = f.round_k > 0 ? f.round_k : p.round_width;

  // ---- the order-dependent modes that round growth replays (KArgs::round_*), decided when the
  // round buffers are allocated and facts from then on
  if (f.round_allocated) {
    p.round_bynode = f.alloc_bynode;
    p.round_xt = f.alloc_xt;
    p.round_cegb = f.alloc_cegb;
  } else if (width > 1) {
    const bool base = ic.empty() && !voting;
    const bool simple = base && !any_cat;
    const double cat_bytes = static_cast<double>(f.split_rows) * f.num_categorical * kMaxCatWords * sizeof(uint32_t);
    const double pre_bytes = static_cast<double>(f.split_rows) * f.total_bins * f.limits.xt_pre_bytes;
    // per-node sampling: every rank draws the same samples; each node keeps its category sets
    p.round_bynode = bynode && base && cat_bytes <= kNodeCatSetsMaxBytes && !f.bynode_rounds_off;
    // extra_trees: one process, prefix tables per node
    p.round_xt = c.extra_trees && simple && !distributed && !cegb && c.forcedsplits_filename.empty() &&
                 f.num_features <= kXtReplayMaxFeatures && pre_bytes <= kXtPrefixMaxBytes && !f.xt_rounds_off;
    // coupled CEGB penalties: the replay subtracts them from raw candidates and refunds them
    p.round_cegb = cegb && cegb_coupled && !cegb_lazy && simple && !any_mono && !f.cegb_rounds_off;
  }

  // ---- growth: one split per step when the split order depends on more than each leaf's own
  // rows and the replay above does not cover it
  auto steps = [&p](bool rule, const char* reason) {
    if (rule && p.growth == Growth::kRounds) {
      p.growth = Growth::kSteps;
      p.growth_reason = reason;
    }
  };
  p.growth = Growth::kRounds;
  steps(!p.device_resident, "host-assisted");
  steps(width <= 1 || !f.round_allocated, "round width 1 or no round state");
  steps(distributed && !f.device_comm, "host collectives");
  steps(bynode && !(p.round_bynode && ic.empty()), "per-node sampling outside the round replay");
  steps(c.extra_trees && !p.round_xt, "extra_trees outside the round replay");
  steps(f.forced == ForcedSplits::kScheduled, "forced splits");
  steps(p.mono_inter, "intermediate monotone constraints");
  steps(p.cegb && (voting || cegb_lazy), "CEGB under voting or with lazy penalties");
  if (p.growth == Growth::kRounds && p.cegb && cegb_coupled && !p.round_cegb) {
    p.growth = Growth::kRoundsOnceSampleUsed;
    p.growth_reason = "coupled CEGB penalties until every feature of the tree's sample is used";
  }

  // ---- the next tree may be launched before GBDT asks for it when nothing between the two
  // Train() calls can change its inputs: GBDT allowed it, the tree grows in rounds of a single
  // process without per-tree host state, its records came through host_out, nothing is traced
  // or still being timed (opt-in: LGBM_AMD_SPECULATE=1)
  p.may_speculate = f.spec_allowed && p.growth == Growth::kRounds && !distributed && !f.bagging && f.speculate_knob &&
                    f.host_out && !bynode && !c.extra_trees && !cegb && !f.ktrace && f.timed_rounds &&
                    f.num_tree_per_iteration == 1;
  return p;
}

// ---------------------------------------------------------------- LGBM_AMD_GrowthPlan's JSON
void GrowthFactsFromJson(const std::string& text, GrowthFacts* f) {
  const Json j = Json::Parse(text);
  if (!j.is_object()) Log::Fatal("growth facts: a JSON object is expected");
  auto flag = [&j](const char* k, bool* v) { if (j.has(k)) *v = j[k].bool_value() || j[k].number_value() != 0; };
  auto num = [&j](const char* k, int* v) { if (j.has(k)) *v = j[k].int_value(); };
  if (j.has("kind")) {
    const std::string& k = j["kind"].string_value();
    if (k != "serial" && k != "data" && k != "feature" && k != "voting") Log::Fatal("growth facts: unknown kind %s", k.c_str());
    f->kind = k == "data" ? LearnerKind::kData : k == "feature" ? LearnerKind::kFeature
              : k == "voting" ? LearnerKind::kVoting : LearnerKind::kSerial;
  }
  if (j.has("forced")) {
    const std::string& k = j["forced"].string_value();
    if (k != "none" && k != "scheduled" && k != "refused") Log::Fatal("growth facts: unknown forced state %s", k.c_str());
    f->forced = k == "scheduled" ? ForcedSplits::kScheduled : k == "refused" ? ForcedSplits::kRefused : ForcedSplits::kNone;
  }
  num("world", &f->world);
  flag("force_host", &f->force_host);
  flag("dist_host_assist", &f->dist_host_assist);
  flag("device_comm", &f->device_comm);
  num("num_features", &f->num_features);
  num("num_categorical", &f->num_categorical);
  num("max_cat_bins", &f->max_cat_bins);
  num("total_bins", &f->total_bins);
  num("round_k", &f->round_k);
  num("split_rows", &f->split_rows);
  flag("round_allocated", &f->round_allocated);
  flag("alloc_bynode", &f->alloc_bynode);
  flag("alloc_xt", &f->alloc_xt);
  flag("alloc_cegb", &f->alloc_cegb);
  flag("bynode_rounds_off", &f->bynode_rounds_off);
  flag("xt_rounds_off", &f->xt_rounds_off);
  flag("cegb_rounds_off", &f->cegb_rounds_off);
  f->has_round_k_knob = j.has("round_k_knob");
  num("round_k_knob", &f->round_k_knob);
  flag("speculate_knob", &f->speculate_knob);
  flag("spec_allowed", &f->spec_allowed);
  flag("bagging", &f->bagging);
  flag("host_out", &f->host_out);
  flag("ktrace", &f->ktrace);
  num("num_tree_per_iteration", &f->num_tree_per_iteration);
  flag("timed_rounds", &f->timed_rounds);
}

std::string GrowthPlanToJson(const GrowthPlan& p) {
  auto str = [](const char* s) { return s == nullptr ? std::string("null") : "\"" + std::string(s) + "\""; };
  auto b = [](bool v) { return v ? "true" : "false"; };
  std::ostringstream o;
  o << "{\"device_resident\": " << b(p.device_resident) << ", \"reason\": " << str(p.reason)
    << ", \"mono_inter\": " << b(p.mono_inter) << ", \"cegb\": " << b(p.cegb)
    << ", \"round_bynode\": " << b(p.round_bynode) << ", \"round_xt\": " << b(p.round_xt)
    << ", \"round_cegb\": " << b(p.round_cegb) << ", \"growth\": "
    << str(p.growth == Growth::kRounds ? "rounds" : p.growth == Growth::kSteps ? "steps" : "rounds_once_sample_used")
    << ", \"growth_reason\": " << str(p.growth_reason) << ", \"round_width\": " << p.round_width
    << ", \"width_adapts\": " << b(p.width_adapts) << ", \"may_speculate\": " << b(p.may_speculate) << "}";
  return o.str();
}

}  // namespace lgbm_amd
