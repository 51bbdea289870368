// Host-only driver of the growth rules (src/treelearner/growth_plan.cpp) for the sanitizer
// test: a few rows of tests/test_growth_plan.py's table and the evaluator's JSON glue, built
// with growth_plan.cpp alone (no device code, no HIP runtime).
#include <cstdio>
#include <string>

#include "../../src/treelearner/growth_limits.h"

using namespace lgbm_amd;

static int failures = 0;

static void Expect(const char* what, const Config& c, const std::string& facts_json, bool device, Growth growth, int width) {
  GrowthFacts f;
  f.limits = DeviceGrowthLimits();
  GrowthFactsFromJson(facts_json, &f);
  const GrowthPlan p = PlanGrowth(c, f);
  const std::string out = GrowthPlanToJson(p);
  if (p.device_resident != device || p.growth != growth || p.round_width != width || out.empty()) {
    std::fprintf(stderr, "%s: %s\n", what, out.c_str());
    ++failures;
  }
}

int main() {
  const std::string serial = "{\"num_features\": 8, \"total_bins\": 120, \"round_k\": 8, \"split_rows\": 186, \"round_allocated\": true";
  Config c;
  c.num_leaves = 31;
  Expect("defaults", c, serial + "}", true, Growth::kRounds, 8);
  Expect("forced host", c, serial + ", \"force_host\": true}", false, Growth::kSteps, 8);
  Expect("wide categorical", c, serial + ", \"num_categorical\": 1, \"max_cat_bins\": 4097}", false, Growth::kSteps, 8);
  Expect("forced splits", c, serial + ", \"forced\": \"scheduled\"}", true, Growth::kSteps, 8);
  Expect("round width knob", c, serial + ", \"round_k\": 0, \"round_k_knob\": 999}", true, Growth::kRounds, 16);
  Config xt = c;
  xt.extra_trees = true;
  Expect("extra_trees without its tables", xt, serial + "}", true, Growth::kSteps, 8);
  Expect("extra_trees, voting, categorical", xt,
         serial + ", \"kind\": \"voting\", \"world\": 2, \"device_comm\": true, \"num_categorical\": 1, \"max_cat_bins\": 6}",
         false, Growth::kSteps, 8);
  Config ic = c;
  ic.interaction_constraints_vector.assign(257, std::vector<int>{0});
  Expect("257 constraints", ic, serial + "}", false, Growth::kSteps, 8);
  Config cegb = c;
  cegb.cegb_penalty_feature_coupled.assign(8, 1.0);
  Expect("coupled CEGB with a categorical feature", cegb, serial + ", \"num_categorical\": 1, \"max_cat_bins\": 6}", true,
         Growth::kRoundsOnceSampleUsed, 8);
  c.num_leaves = 255;
  Expect("255 leaves", c, "{\"num_features\": 8}", true, Growth::kSteps, 16);
  bool refused = false;
  try {
    GrowthFacts f;
    GrowthFactsFromJson("{\"kind\": \"quantum\"}", &f);
  } catch (const std::exception&) {
    refused = true;
  }
  if (!refused) ++failures;
  std::printf(failures == 0 ? "growth plan driver ok\n" : "growth plan driver: %d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
