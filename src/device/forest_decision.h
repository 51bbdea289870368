// The decision of one flattened-forest node on a raw feature value: the device's one statement
// of the rule, shared by the score kernel (src/device/predict_kernels.hip), the SHAP / leaf
// kernels (src/device/shap_kernels.hip) and the host evaluator of the path tables
// (src/boosting/shap_paths.cpp).  Same semantics as the host predictor: reference
// Tree::NumericalDecision / CategoricalDecision with the dense C API rows' |v| <= kZeroThreshold
// read as 0.  tests/helpers/forest_ref.py states the rule apart from the code.
#pragma once

#include <cmath>

#include "kernels.h"
#include "stored_order.h"  // (LGBM_AMD_HD)

namespace lgbm_amd {
namespace dev {

// true: the row goes to the left child of node `gi` (global node index) of tree `t`
LGBM_AMD_HD bool ForestGoesLeft(const ForestArgs& f, int t, int gi, double v) {
  constexpr double kZero = 1e-35f;  // kZeroThreshold
  if (fabs(v) <= kZero) v = 0.0;
  const int8_t dt = f.dtype[gi];
  const int mt = (dt >> 2) & 3;
  if (dt & 1) {  // categorical
    // NaN goes right whatever the missing type, as in the host predictor (whose int cast of a NaN
    // is negative); the casts are kept in range so that host and device agree on every value
    if (v != v || !(v > -1.0)) return false;
    const int iv = v >= 2147483647.0 ? 2147483647 : static_cast<int>(v);
    const int32_t* bound = f.cat_bound + f.cat_bound_off[t];
    const uint32_t* bits = f.cat_bits + f.cat_bits_off[t];
    const int ci = static_cast<int>(f.threshold[gi]);
    const int lo = bound[ci], nw = bound[ci + 1] - lo;
    const int w = iv >> 5;
    return w < nw && ((bits[lo + w] >> (iv & 31)) & 1u);
  }
  if (v != v && mt != 2) v = 0.0;
  if ((mt == 1 && fabs(v) <= kZero) || (mt == 2 && v != v)) return (dt & 2) != 0;
  return v <= f.threshold[gi];
}

}  // namespace dev
}  // namespace lgbm_amd
