// One leaf of the per-leaf TreeSHAP (src/boosting/shap_paths.h has the tables): the arithmetic that
// both contribution kernels run, k_shap_forest (src/device/shap_kernels.hip: a lane is a row, the
// leaves of a tree one after the other) and k_shap_leaf_lanes (src/device/shap_leaf_kernels.hip: a
// lane is a leaf).  EvalPathTables (src/boosting/shap_paths.cpp) is the same loops on the host,
// operation for operation.
#pragma once

#include "forest_decision.h"
#include "kernels.h"

namespace lgbm_amd {
namespace dev {

// the value of feature `feat` of `row` in the matrix the forest walks
template <typename T, bool ROW_MAJOR>
__device__ __forceinline__ double ForestValue(const ForestArgs& f, int64_t row, int feat) {
  const T* x = static_cast<const T*>(f.data);
  return ROW_MAJOR ? static_cast<double>(x[row * f.num_cols + feat])
                   : static_cast<double>(x[static_cast<int64_t>(feat) * f.num_rows + row]);
}

// Leaf `l` of the tables for one row: ExtendPath of the bias element and of the leaf's D merged
// elements in table order, then UnwoundPathSum of every element; emit(e, term) receives element
// e's term total * (one - zero) * leaf_value, in table order.
//   pw    the caller's path weights, element i at pw[i * PW] (runtime-indexed: LDS, not a private array)
//   mask  the row's decisions of the leaf's tree, bit (node & 31) of mask[(node >> 5) * MK] set
//         where the row goes left; an element's one-fraction is 1 where every one of its (node,
//         direction) pairs agrees with the mask, else 0
template <int PW, int MK, typename Emit>
__device__ __forceinline__ void ShapLeafTerms(const ShapArgs& a, int l, double* pw, const uint32_t* mask,
                                              Emit&& emit) {
  const int e0 = a.leaf_elem_off[l], D = a.leaf_elem_off[l + 1] - e0;
  // ExtendPath of the bias element, then of elements 1..D; ones: bit d = one-fraction of element d
  unsigned long long ones_lo = 0, ones_hi = 0;
  pw[0] = 1.0;
  for (int d = 1; d <= D; ++d) {
    const int e = e0 + d - 1;
    bool one = true;
    for (int p = a.elem_pair_off[e], p1 = a.elem_pair_off[e + 1]; p < p1; ++p) {
      const int pr = a.pairs[p], node = pr >> 1;
      const uint32_t went_left = (mask[(node >> 5) * MK] >> (node & 31)) & 1u;
      one = one && went_left == static_cast<uint32_t>(pr & 1);
    }
    if (d < 64) ones_lo |= static_cast<unsigned long long>(one) << d;
    else ones_hi |= static_cast<unsigned long long>(one) << (d - 64);
    const double zero = a.elem_zero[e];
    const double dp1 = static_cast<double>(d + 1);
    double carry = 0.0;  // pweight[i + 1] after its own scaling by the zero fraction
    for (int i = d - 1; i >= 0; --i) {
      const double p = pw[i * PW];
      const double up = p * (i + 1) / dp1;
      pw[(i + 1) * PW] = carry + (one ? up : 0.0);
      carry = zero * p * (d - i) / dp1;
    }
    pw[0] = carry;
  }
  // UnwoundPathSum of every element, both of its branches computed and selected
  const double lv = a.leaf_value[l];
  const double* ratio = a.ratio + ShapRatioOffset(D);
  const double Dp1 = static_cast<double>(D + 1);
  const double top = pw[D * PW];
  for (int i = 1; i <= D; ++i) {
    const int e = e0 + i - 1;
    const double zero = a.elem_zero[e];
    const bool one = ((i < 64 ? ones_lo >> i : ones_hi >> (i - 64)) & 1ull) != 0;
    double next_one = top, total = 0.0;
    for (int j = D - 1; j >= 0; --j) {
      const double p = pw[j * PW];
      const double r = ratio[j];
      const double q = (one ? next_one * Dp1 : p) / (one ? static_cast<double>(j + 1) : zero);
      total += one ? q : q / r;
      next_one = p - q * zero * r;
    }
    emit(e, total * ((one ? 1.0 : 0.0) - zero) * lv);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
