// The device kernels' limits that the growth rules read (growth_plan.h), from their home in
// src/device/: the rules themselves stay free of the HIP headers.
#pragma once

#include "../device/kernels.h"
#include "growth_plan.h"

namespace lgbm_amd {

inline GrowthLimits DeviceGrowthLimits() {
  GrowthLimits l;
  l.max_cat_bins = dev::kFindMaxCatBins;
  l.max_ic_constraints = dev::kMaxIcConstraints;
  l.mono_inter_max_leaves = dev::kMonoInterMaxLeaves;
  l.max_round_exp = dev::kMaxRoundExp;
  l.xt_pre_bytes = static_cast<int>(sizeof(dev::XtPre));
  return l;
}

}  // namespace lgbm_amd
