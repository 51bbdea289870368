// Leaf indices and SHAP contributions of a flattened forest on raw feature values.
//
// k_predict_leaf is the walk of k_predict_forest (src/device/predict_kernels.hip) writing each
// tree's leaf index instead of summing leaf values (reference GBDT::PredictLeafIndex).
//
// k_shap_forest is TreeSHAP (Lundberg et al., arXiv:1706.06060; reference Tree::TreeSHAP,
// src/io/tree.cpp) in its per-leaf form, from the path tables of src/boosting/shap_paths.cpp: a
// leaf's contribution to phi[feature of element i] is UnwoundPathSum(path, D, i) * (one_i -
// zero_i) * leaf_value after the leaf's D merged path elements were ExtendPath'ed in table
// order.  One lane owns one row and a workgroup of kShapLanes rows walks every tree, leaf and
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
#include "forest_decision.h"

namespace lgbm_amd {
namespace dev {

namespace {

constexpr int kPhiLdsStride = kShapLanes + 1;  // (+1: the transposed read-out is free of bank conflicts)

template <typename T, bool ROW_MAJOR>
__device__ __forceinline__ double ForestValue(const ForestArgs& f, int64_t row, int feat) {
  const T* x = static_cast<const T*>(f.data);
  return ROW_MAJOR ? static_cast<double>(x[row * f.num_cols + feat])
                   : static_cast<double>(x[static_cast<int64_t>(feat) * f.num_rows + row]);
}

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
          const int e0 = a.leaf_elem_off[l], D = a.leaf_elem_off[l + 1] - e0;
          // ExtendPath of the bias element, then of elements 1..D; ones: bit d = one-fraction of element d
          unsigned long long ones_lo = 0, ones_hi = 0;
          pw[0] = 1.0;
          for (int d = 1; d <= D; ++d) {
            const int e = e0 + d - 1;
            bool one = true;
            for (int p = a.elem_pair_off[e], p1 = a.elem_pair_off[e + 1]; p < p1; ++p) {
              const int pr = a.pairs[p], node = pr >> 1;
              const uint32_t went_left = (mask[(node >> 5) * kShapLanes] >> (node & 31)) & 1u;
              one = one && went_left == static_cast<uint32_t>(pr & 1);
            }
            if (d < 64) ones_lo |= static_cast<unsigned long long>(one) << d;
            else ones_hi |= static_cast<unsigned long long>(one) << (d - 64);
            const double zero = a.elem_zero[e];
            const double dp1 = static_cast<double>(d + 1);
            double carry = 0.0;  // pweight[i + 1] after its own scaling by the zero fraction
            for (int i = d - 1; i >= 0; --i) {
              const double p = pw[i * kShapLanes];
              const double up = p * (i + 1) / dp1;
              pw[(i + 1) * kShapLanes] = carry + (one ? up : 0.0);
              carry = zero * p * (d - i) / dp1;
            }
            pw[0] = carry;
          }
          // UnwoundPathSum of every element, both of its branches computed and selected
          const double lv = a.leaf_value[l];
          const double* ratio = a.ratio + ShapRatioOffset(D);
          const double Dp1 = static_cast<double>(D + 1);
          const double top = pw[D * kShapLanes];
          for (int i = 1; i <= D; ++i) {
            const int e = e0 + i - 1;
            const double zero = a.elem_zero[e];
            const bool one = ((i < 64 ? ones_lo >> i : ones_hi >> (i - 64)) & 1ull) != 0;
            double next_one = top, total = 0.0;
            for (int j = D - 1; j >= 0; --j) {
              const double p = pw[j * kShapLanes];
              const double r = ratio[j];
              const double q = (one ? next_one * Dp1 : p) / (one ? static_cast<double>(j + 1) : zero);
              total += one ? q : q / r;
              next_one = p - q * zero * r;
            }
            phi[a.elem_feature[e] * fs] += total * ((one ? 1.0 : 0.0) - zero) * lv;
          }
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
  size_t doubles = static_cast<size_t>(a.max_path_len) * kShapLanes;
  if (phi_in_lds) doubles += static_cast<size_t>(a.num_features + 1) * kPhiLdsStride;
  return doubles * sizeof(double) + static_cast<size_t>(a.mask_words) * kShapLanes * sizeof(uint32_t);
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
