// Batch prediction of a forest on raw feature values (reference Tree::GetLeaf /
// NumericalDecision / CategoricalDecision, include/LightGBM/tree.h:265-337,578-598, and
// GBDT::PredictRaw, src/boosting/gbdt_prediction.cpp:13-40).
//
// One thread per row walks every tree in model order, accumulating the raw score of each
// class in registers in the same order as the host predictor (bit-identical sums).  The
// flattened forest (a few hundred KB for 500 x 63-leaf trees) stays L2-resident and every
// wave reads the same node at the same time.  A node is decided by ForestGoesLeft
// (forest_decision.h), the device's one statement of the rule.
#include "device_common.h"
#include "forest_decision.h"

namespace lgbm_amd {
namespace dev {

namespace {

template <typename T, bool ROW_MAJOR>
__global__ __launch_bounds__(256) void k_predict_forest(ForestArgs f) {
  const int64_t row = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (row >= f.num_rows) return;
  double acc[kMaxPredClasses];
#pragma unroll
  for (int k = 0; k < kMaxPredClasses; ++k) acc[k] = 0.0;
  const T* x = static_cast<const T*>(f.data);
  for (int t = 0; t < f.num_trees; ++t) {
    const int n0 = f.node_off[t], n1 = f.node_off[t + 1];
    int leaf = 0;
    if (n1 > n0) {
      int node = 0;
      while (node >= 0) {
        const int gi = n0 + node;
        const int feat = f.feature[gi];
        const double v = ROW_MAJOR ? static_cast<double>(x[row * f.num_cols + feat])
                                   : static_cast<double>(x[static_cast<int64_t>(feat) * f.num_rows + row]);
        node = ForestGoesLeft(f, t, gi, v) ? f.left[gi] : f.right[gi];
      }
      leaf = ~node;
    }
    const double lv = f.leaf_value[f.leaf_off[t] + leaf];
    const int k = t % f.num_class;
#pragma unroll
    for (int c = 0; c < kMaxPredClasses; ++c) {
      if (c == k) acc[c] += lv;
    }
  }
  for (int c = 0; c < f.num_class; ++c) f.out[row * f.num_class + c] = acc[c];
}

}  // namespace

void PredictForest(const ForestArgs& f, hipStream_t s) {
  if (f.num_rows <= 0) return;
  const dim3 grid(static_cast<unsigned>((f.num_rows + 255) / 256));
  if (f.is_double) {
    if (f.row_major) hipLaunchKernelGGL((k_predict_forest<double, true>), grid, dim3(256), 0, s, f);
    else hipLaunchKernelGGL((k_predict_forest<double, false>), grid, dim3(256), 0, s, f);
  } else {
    if (f.row_major) hipLaunchKernelGGL((k_predict_forest<float, true>), grid, dim3(256), 0, s, f);
    else hipLaunchKernelGGL((k_predict_forest<float, false>), grid, dim3(256), 0, s, f);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
