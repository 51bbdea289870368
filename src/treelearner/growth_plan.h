// How the device learner grows a tree, decided in one place: PlanGrowth is a pure function of the
// configuration and of GrowthFacts (what the learner knows that Config does not), so the rules
// can be read, and tested without a GPU (LGBM_AMD_GrowthPlan), as one list.  The learner fills
// the facts, applies the plan's side effects and keeps what is runtime state: the timing of
// rounds against steps (AutoGrowthRounds), which features a CEGB model has used (CegbRounds) and
// the per-tree round width.
#pragma once

#include <string>

#include "lgbm_amd/config.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {

enum class LearnerKind { kSerial, kData, kFeature, kVoting };
enum class ForcedSplits { kNone, kScheduled, kRefused };  // (kRefused: no device schedule was built)
enum class Growth { kRounds, kSteps, kRoundsOnceSampleUsed };

// limits of the device kernels, from their home in src/device/ (growth_limits.h)
struct GrowthLimits {
  int max_cat_bins = 0;           // dev::kFindMaxCatBins
  int max_ic_constraints = 0;     // dev::kMaxIcConstraints
  int mono_inter_max_leaves = 0;  // dev::kMonoInterMaxLeaves
  int max_round_exp = 0;          // dev::kMaxRoundExp
  int xt_pre_bytes = 0;           // sizeof(dev::XtPre)
};

struct GrowthFacts {
  GrowthLimits limits;
  // the learner
  LearnerKind kind = LearnerKind::kSerial;
  int world = 1;
  bool distributed() const { return kind != LearnerKind::kSerial && world > 1; }
  bool data_parallel() const { return kind == LearnerKind::kData && world > 1; }
  bool voting() const { return kind == LearnerKind::kVoting && world > 1; }
  // feature-parallel: each rank's forced records are gathered after the scans
  bool forced_gathered() const { return kind == LearnerKind::kFeature && world > 1; }
  bool force_host = false;        // ForceHostMode() or LGBM_AMD_HOST_ASSIST=1
  bool dist_host_assist = false;  // LGBM_AMD_DIST_HOST_ASSIST=1
  bool device_comm = false;       // a device communicator exists
  // the dataset
  int num_features = 0;
  int num_categorical = 0;
  int max_cat_bins = 0;  // the largest categorical feature's num_bin
  int total_bins = 0;
  bool any_categorical() const { return num_categorical > 0; }
  ForcedSplits forced = ForcedSplits::kNone;
  // round growth: the learner's width (0: not fixed yet, the plan's own) and node rows; once the
  // round buffers are allocated their three flags are facts (a later ResetConfig does not
  // reallocate them); LGBM_AMD_{BYNODE,XT,CEGB}_ROUNDS=0 and LGBM_AMD_ROUND_K
  int round_k = 0;
  int split_rows = 0;
  bool round_allocated = false;
  bool alloc_bynode = false, alloc_xt = false, alloc_cegb = false;
  bool bynode_rounds_off = false, xt_rounds_off = false, cegb_rounds_off = false;
  bool has_round_k_knob = false;
  int round_k_knob = 0;
  // speculation
  bool speculate_knob = false;  // LGBM_AMD_SPECULATE=1
  bool spec_allowed = false;    // GBDT's permission
  bool bagging = false;
  bool host_out = false;        // the last round tree's records came through KArgs::host_out
  bool ktrace = false;
  int num_tree_per_iteration = 1;
  bool timed_rounds = false;    // the growth timing settled on rounds
};

struct GrowthPlan {
  bool device_resident = true;
  const char* reason = nullptr;  // why host-assisted
  bool mono_inter = false;       // intermediate monotone constraints on the device
  bool cegb = false;             // CEGB penalties on the device
  bool round_bynode = false, round_xt = false, round_cegb = false;  // KArgs::round_*
  // kRoundsOnceSampleUsed: coupled CEGB penalties without round_cegb grow in rounds once every
  // feature of the tree's sample is used (GPUTreeLearner::CegbRounds decides per tree)
  Growth growth = Growth::kSteps;
  const char* growth_reason = nullptr;  // why not kRounds
  int round_width = 1;                  // the initial width
  bool width_adapts = false;
  bool may_speculate = false;
};

GrowthPlan PlanGrowth(const Config& config, const GrowthFacts& facts);

// the environment's share of the facts
inline void FillKnobFacts(GrowthFacts* f) {
  f->force_host = tuning::On(tuning::Knob::HostAssist);
  f->dist_host_assist = tuning::On(tuning::Knob::DistHostAssist);
  f->bynode_rounds_off = tuning::Off(tuning::Knob::ByNodeRounds);
  f->xt_rounds_off = tuning::Off(tuning::Knob::XtRounds);
  f->cegb_rounds_off = tuning::Off(tuning::Knob::CegbRounds);
  f->has_round_k_knob = tuning::Get(tuning::Knob::RoundK) != nullptr;
  f->round_k_knob = tuning::Int(tuning::Knob::RoundK, 0);
  f->speculate_knob = tuning::On(tuning::Knob::Speculate);
}

// LGBM_AMD_GrowthPlan: facts from a JSON object (absent keys keep their defaults), the plan as one
void GrowthFactsFromJson(const std::string& json, GrowthFacts* facts);
std::string GrowthPlanToJson(const GrowthPlan& plan);

}  // namespace lgbm_amd
