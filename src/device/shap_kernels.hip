// Leaf indices and SHAP contributions of a flattened forest on raw feature values.
//
// k_predict_leaf is the walk of k_predict_forest (src/device/predict_kernels.hip) writing each
// tree's leaf index instead of summing leaf values (reference GBDT::PredictLeafIndex).
//
// k_shap_forest is TreeSHAP (Lundberg et al., arXiv:1706.06060; reference Tree::TreeSHAP,
// src/io/tree.cpp) in its per-leaf form, from the path tables of src/boosting/shap_paths.cpp: a
// leaf's contribution to phi[feature of element i] is UnwoundPathSum(path, D, i) * (one_i -
// zero_i) * leaf_value after the leaf's D merged path elements were ExtendPath'ed in table
// order (ShapLeafTerms, src/device/shap_leaf.h, shared with the leaves-on-lanes kernel of small
// batches, src/device/shap_leaf_kernels.hip).  One lane owns one row and a workgroup of
// kShapLanes rows walks every tree, leaf and
// element together: the tables are wave-uniform loads and nothing diverges; a lane differs from
// its neighbours only in the 0 / 1 one-fractions, which are selects.  Per lane:
//   * the decisions of all internal nodes of the current tree, as a bit mask in LDS
//     ([word][lane]), evaluated once per tree; an element's one-fraction is a compare of its
//     (node, direction) pairs with that mask;
//   * the path weights pweight[0..D] in LDS as [element][lane] (runtime-indexed: a private array
//     would live in scratch memory);
//   * the accumulator phi[feature] as [feature][lane], in LDS while it fits, else in a
//     workgroup-owned tile of global memory; it is written out transposed per class.
// A row belongs to one lane and leaves are visited in table order: no atomics, and the result
// does not depend on scheduling.  src/boosting/shap_paths.cpp has the same arithmetic on the
// host (EvalPathTables), which the tests hold against the recursive host predictor.
#include "device_common.h"
#include "shap_leaf.h"
#include "shap_plan.h"

namespace lgbm_amd {
namespace dev {

namespace {

template <typename T, bool ROW_MAJOR>
__global__ __launch_bounds__(256) void k_predict_leaf(ForestArgs f) {
  const int64_t row = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (row >= f.num_rows) return;
  for (int t = 0; t < f.num_trees; ++t) {
    const int n0 = f.node_off[t], n1 = f.node_off[t + 1];
    int leaf = 0;
    if (n1 > n0) {
      int node = 0;
      while (node >= 0) {
        const int gi = n0 + node;
        const double v = ForestValue<T, ROW_MAJOR>(f, row, f.feature[gi]);
        node = ForestGoesLeft(f, t, gi, v) ? f.left[gi] : f.right[gi];
      }
      leaf = ~node;
    }
    f.out[row * f.num_trees + t] = static_cast<double>(leaf);
  }
}

template <typename T, bool ROW_MAJOR, bool PHI_LDS>
__global__ __launch_bounds__(kShapLanes) void k_shap_forest(ForestArgs f, ShapArgs a) {
  extern __shared__ double shap_lds[];
  const int lane = threadIdx.x;
  const int F1 = a.num_features + 1;
  double* pw = shap_lds + lane;  // pw[e * kShapLanes]
  double* phi_tile = PHI_LDS ? shap_lds + a.max_path_len * kShapLanes
                             : a.phi_tiles + static_cast<size_t>(blockIdx.x) * F1 * kShapLanes;
  const int fs = PHI_LDS ? kPhiLdsStride : kShapLanes;
  double* phi = phi_tile + lane;  // phi[feature * fs]
  uint32_t* mask = reinterpret_cast<uint32_t*>(shap_lds + a.max_path_len * kShapLanes +
                                               (PHI_LDS ? F1 * kPhiLdsStride : 0)) + lane;  // mask[word * kShapLanes]
  for (int tile = blockIdx.x; tile < a.num_tiles; tile += gridDim.x) {
    const int64_t row0 = static_cast<int64_t>(tile) * kShapLanes;
    // (lanes past the last row recompute it, so that every loop stays wave-uniform; they store nothing)
    const int64_t row = min(row0 + lane, f.num_rows - 1);
    for (int k = 0; k < f.num_class; ++k) {
      for (int ft = 0; ft < F1; ++ft) phi[ft * fs] = 0.0;
      for (int t = k; t < f.num_trees; t += f.num_class) {
        phi[a.num_features * fs] += a.expected[t];
        const int l0 = a.tree_leaf_off[t], l1 = a.tree_leaf_off[t + 1];
        if (l0 == l1) continue;
        const int n0 = f.node_off[t], nn = f.node_off[t + 1] - n0;
        for (int w = 0; w * 32 < nn; ++w) {
          const int cnt = min(32, nn - w * 32);
          uint32_t m = 0;
          for (int b = 0; b < cnt; ++b) {
            const int gi = n0 + w * 32 + b;
            const double v = ForestValue<T, ROW_MAJOR>(f, row, f.feature[gi]);
            m |= ForestGoesLeft(f, t, gi, v) ? (1u << b) : 0u;
          }
          mask[w * kShapLanes] = m;
        }
        for (int l = l0; l < l1; ++l) {
          ShapLeafTerms<kShapLanes, kShapLanes>(a, l, pw, mask, [&](int e, double term) {
            phi[a.elem_feature[e] * fs] += term;
          });
        }
      }
      __syncthreads();
      const int cells = static_cast<int>(min(static_cast<int64_t>(kShapLanes), f.num_rows - row0)) * F1;
      for (int idx = lane; idx < cells; idx += kShapLanes) {
        const int r = idx / F1, ft = idx - r * F1;
        a.out[((row0 + r) * f.num_class + k) * F1 + ft] = phi_tile[ft * fs + r];
      }
      __syncthreads();
    }
  }
}

template <typename T, bool ROW_MAJOR>
void LaunchShap(const ForestArgs& f, const ShapArgs& a, hipStream_t s) {
  const bool lds = a.phi_tiles == nullptr;
  const size_t bytes = ShapLdsBytes(a, lds);
  const dim3 grid(static_cast<unsigned>(lds ? a.num_tiles : ShapTileGrid(a.num_tiles)));
  if (lds) hipLaunchKernelGGL((k_shap_forest<T, ROW_MAJOR, true>), grid, dim3(kShapLanes), bytes, s, f, a);
  else hipLaunchKernelGGL((k_shap_forest<T, ROW_MAJOR, false>), grid, dim3(kShapLanes), bytes, s, f, a);
}

}  // namespace

void PredictForestLeaf(const ForestArgs& f, hipStream_t s) {
  if (f.num_rows <= 0) return;
  const dim3 grid(static_cast<unsigned>((f.num_rows + 255) / 256));
  if (f.is_double) {
    if (f.row_major) hipLaunchKernelGGL((k_predict_leaf<double, true>), grid, dim3(256), 0, s, f);
    else hipLaunchKernelGGL((k_predict_leaf<double, false>), grid, dim3(256), 0, s, f);
  } else {
    if (f.row_major) hipLaunchKernelGGL((k_predict_leaf<float, true>), grid, dim3(256), 0, s, f);
    else hipLaunchKernelGGL((k_predict_leaf<float, false>), grid, dim3(256), 0, s, f);
  }
}

size_t ShapLdsBytes(const ShapArgs& a, bool phi_in_lds) {
  return ShapRowsLdsBytes(a.max_path_len, a.mask_words, a.num_features, phi_in_lds);
}

int ShapTileGrid(int num_tiles) { return std::max(1, std::min(num_tiles, 2048)); }

void ShapForest(const ForestArgs& f, const ShapArgs& a, hipStream_t s) {
  if (f.num_rows <= 0) return;
  if (f.is_double) {
    if (f.row_major) LaunchShap<double, true>(f, a, s);
    else LaunchShap<double, false>(f, a, s);
  } else {
    if (f.row_major) LaunchShap<float, true>(f, a, s);
    else LaunchShap<float, false>(f, a, s);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
