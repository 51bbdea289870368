// SHAP contributions of small batches: k_shap_leaf_lanes, the leaves-on-lanes arrangement of the
// per-leaf TreeSHAP whose rows-on-lanes arrangement is k_shap_forest (src/device/shap_kernels.hip;
// src/device/shap_plan.h picks between them).  A leaf's contribution depends only on its own path
// table and on the row's decisions in its tree, so with few rows the parallelism is in the leaves
// and trees:
//   * a workgroup owns one row (the grid runs over rows) and takes its classes in turn;
//   * the workgroup's W waves take the class's trees in batches of W, one tree per wave;
//   * decisions: lanes are internal nodes (ForestValue / ForestGoesLeft, the rule of every forest
//     kernel); a ballot turns 64 decisions into two mask words of the wave's LDS mask area;
//   * leaves: lanes are leaves, in strides of 64.  A lane runs ShapLeafTerms (src/device/shap_leaf.h,
//     the arithmetic of k_shap_forest) for its leaf with its own path length -- the lanes diverge
//     in it -- on its column of the wave's path weights ([element][lane]) and writes every
//     element's term to the wave's LDS slab at the element's position within the tree.  An element
//     belongs to one leaf: no write conflicts, no atomics;
//   * fold: after a barrier the batch's terms are added into the row's accumulator phi[F + 1] (LDS
//     while it fits, else a workgroup-owned global tile), tree after tree with a barrier between
//     them.  Within a tree a thread takes whole features: it walks the feature's group of the fold
//     list (src/boosting/shap_paths.h), which is in table order.  Every phi[f] so receives its
//     terms in tree order, then leaf and element order -- the order in which k_shap_forest adds
//     them -- and expected[t] goes to the bias slot in tree order: the result does not depend on
//     scheduling.
#include "device_common.h"
#include "shap_leaf.h"
#include "shap_plan.h"

namespace lgbm_amd {
namespace dev {

namespace {

template <typename T, bool ROW_MAJOR, bool PHI_LDS>
__global__ __launch_bounds__(kShapLeafMaxWaves * kShapLanes) void k_shap_leaf_lanes(ForestArgs f, ShapArgs a) {
  extern __shared__ double shap_leaf_lds[];
  const int tid = threadIdx.x, threads = blockDim.x;
  const int lane = tid & (kShapLanes - 1), wave = tid / kShapLanes, W = threads / kShapLanes;
  const int F1 = a.num_features + 1;
  const int mw = ShapLeafMaskWords(a.mask_words);
  // [W][max_path_len][64] path weights | [W][max_tree_elems] slabs | phi[F1] | [W][mw] masks
  double* pw = shap_leaf_lds + static_cast<size_t>(wave) * a.max_path_len * kShapLanes + lane;  // pw[e * kShapLanes]
  double* slabs = shap_leaf_lds + static_cast<size_t>(W) * a.max_path_len * kShapLanes;
  double* slab = slabs + static_cast<size_t>(wave) * a.max_tree_elems;
  double* phi_lds = slabs + static_cast<size_t>(W) * a.max_tree_elems;
  double* phi = PHI_LDS ? phi_lds : a.phi_rows + static_cast<size_t>(blockIdx.x) * F1;
  uint32_t* mask = reinterpret_cast<uint32_t*>(phi_lds + (PHI_LDS ? F1 : 0)) + wave * mw;
  for (int64_t row = blockIdx.x; row < f.num_rows; row += gridDim.x) {
    for (int k = 0; k < f.num_class; ++k) {
      const int per_class = (f.num_trees - k + f.num_class - 1) / f.num_class;  // trees k, k + num_class, ...
      for (int ft = tid; ft < F1; ft += threads) phi[ft] = 0.0;
      for (int b0 = 0; b0 < per_class; b0 += W) {
        const int t = k + (b0 + wave) * f.num_class;  // this wave's tree of the batch, if it has one
        int l0 = 0, l1 = 0;
        if (b0 + wave < per_class) {
          l0 = a.tree_leaf_off[t];
          l1 = a.tree_leaf_off[t + 1];
        }
        if (l1 > l0) {  // (a single-leaf tree has no leaves in the tables: the fold adds its expected value)
          const int n0 = f.node_off[t], nn = f.node_off[t + 1] - n0;
          for (int base = 0; base < nn; base += kShapLanes) {
            bool left = false;
            if (base + lane < nn) {
              const int gi = n0 + base + lane;
              left = ForestGoesLeft(f, t, gi, ForestValue<T, ROW_MAJOR>(f, row, f.feature[gi]));
            }
            const unsigned long long went = __ballot(left);
            if (lane == 0) {
              mask[base / 32] = static_cast<uint32_t>(went);
              mask[base / 32 + 1] = static_cast<uint32_t>(went >> 32);
            }
          }
        }
        __syncthreads();  // the masks are written (and phi is zero, the last batch's slabs are folded)
        if (l1 > l0) {
          const int eb = a.leaf_elem_off[l0];  // the tree's first element
          for (int l = l0 + lane; l < l1; l += kShapLanes) {
            ShapLeafTerms<kShapLanes, 1>(a, l, pw, mask, [&](int e, double term) { slab[e - eb] = term; });
          }
        }
        __syncthreads();
        const int batch = min(W, per_class - b0);
        for (int w = 0; w < batch; ++w) {
          const int tw = k + (b0 + w) * f.num_class;
          const double* terms = slabs + static_cast<size_t>(w) * a.max_tree_elems;
          if (tid == 0) phi[a.num_features] += a.expected[tw];
          for (int g = a.tree_group_off[tw] + tid, g1 = a.tree_group_off[tw + 1]; g < g1; g += threads) {
            const int ft = a.group_feature[g];
            double sum = phi[ft];
            for (int j = a.group_off[g], j1 = a.group_off[g + 1]; j < j1; ++j) sum += terms[a.fold_elem[j]];
            phi[ft] = sum;
          }
          __syncthreads();  // (the next tree may hold the same feature in another thread's group)
        }
      }
      for (int ft = tid; ft < F1; ft += threads) a.out[(row * f.num_class + k) * F1 + ft] = phi[ft];
      __syncthreads();
    }
  }
}

template <typename T, bool ROW_MAJOR>
void LaunchShapLeaves(const ForestArgs& f, const ShapArgs& a, hipStream_t s) {
  const bool lds = a.phi_rows == nullptr;
  const size_t bytes =
      ShapLeafLdsBytes(a.leaf_waves, a.max_path_len, a.max_tree_elems, a.mask_words, a.num_features, lds);
  const dim3 grid(static_cast<unsigned>(ShapLeafGrid(f.num_rows))), block(a.leaf_waves * kShapLanes);
  if (lds) hipLaunchKernelGGL((k_shap_leaf_lanes<T, ROW_MAJOR, true>), grid, block, bytes, s, f, a);
  else hipLaunchKernelGGL((k_shap_leaf_lanes<T, ROW_MAJOR, false>), grid, block, bytes, s, f, a);
}

}  // namespace

void ShapForestLeaves(const ForestArgs& f, const ShapArgs& a, hipStream_t s) {
  if (f.num_rows <= 0) return;
  if (f.is_double) {
    if (f.row_major) LaunchShapLeaves<double, true>(f, a, s);
    else LaunchShapLeaves<double, false>(f, a, s);
  } else {
    if (f.row_major) LaunchShapLeaves<float, true>(f, a, s);
    else LaunchShapLeaves<float, false>(f, a, s);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
