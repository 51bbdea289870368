// Which contribution kernel a prediction call takes, and the shape of its workgroup: plain
// arithmetic over the sizes of the model and the row count of the call, which host tests drive
// through LGBM_AMD_ShapPlan (tests/test_shap_plan.py).  Standard library and constants only.
//
//   rows-on-lanes    k_shap_forest (src/device/shap_kernels.hip): a lane is a row, a workgroup of
//                    one wave walks every tree, leaf and element.  Its latency is that of one tile
//                    whatever the row count, so it is the kernel of large calls.
//   leaves-on-lanes  k_shap_leaf_lanes (src/device/shap_leaf_kernels.hip): a workgroup is a row,
//                    each of its W waves a tree of the current batch, a lane a leaf.  The kernel of
//                    calls below tuning::kShapLeafMaxRows rows.
#pragma once

#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {
namespace dev {

constexpr int kPhiLdsStride = kShapLanes + 1;  // (+1: the transposed read-out is free of bank conflicts)
constexpr int kShapLeafWaveSteps = 3;
constexpr int kShapLeafWaveLadder[kShapLeafWaveSteps] = {4, 2, 1};  // W, widest first
constexpr int kShapLeafMaxWaves = kShapLeafWaveLadder[0];

enum ShapKernel : int { kShapKernelNone = -1, kShapKernelRows = 0, kShapKernelLeaves = 1 };
// what the caller asks for (ops.forest_predict's shap_kernel): the rule, or one kernel whatever the rows
enum ShapChoice : int { kShapChoiceAuto = 0, kShapChoiceRows = 1, kShapChoiceLeaves = 2 };

// what the plan reads of a forest and its path tables
struct ShapModel {
  int num_class;       // trees per iteration
  int max_leaves;      // leaves of the largest tree
  int max_tree_elems;  // path elements of the tree that has the most, over all of its leaves
  int max_path_len;    // longest path in elements, bias element included; 0: no tables (a node of data_count 0)
  int num_features;
};

struct ShapPlan {
  int kernel;        // ShapKernel; kShapKernelNone: the device cannot serve the call
  int waves;         // W of leaves-on-lanes (else 1: the one wave of a tile)
  int phi_in_lds;    // the accumulator is in LDS (else in a workgroup-owned global tile)
  size_t lds_bytes;  // dynamic LDS of a workgroup
};

constexpr int ShapMaskWords(int max_leaves) { return max_leaves > 1 ? (max_leaves - 1 + 31) / 32 : 0; }
// a wave's mask area holds whole ballots: two words per 64 internal nodes
constexpr int ShapLeafMaskWords(int mask_words) { return (mask_words + 1) / 2 * 2; }

// LDS of a rows-on-lanes workgroup: the path weights [element][lane], the accumulator tile
// ((F + 1) rows of kShapLanes + 1) while it is in LDS, the decision masks [word][lane]
inline size_t ShapRowsLdsBytes(int max_path_len, int mask_words, int num_features, bool phi_in_lds) {
  size_t doubles = static_cast<size_t>(max_path_len) * kShapLanes;
  if (phi_in_lds) doubles += static_cast<size_t>(num_features + 1) * kPhiLdsStride;
  return doubles * sizeof(double) + static_cast<size_t>(mask_words) * kShapLanes * sizeof(uint32_t);
}

// LDS of a leaves-on-lanes workgroup of W waves: per wave the path-weight columns of its 64 leaves
// ([element][lane]), the slab of its tree's terms and its mask area; once, the row's accumulator
// phi[F + 1] while it is in LDS
inline size_t ShapLeafLdsBytes(int waves, int max_path_len, int max_tree_elems, int mask_words, int num_features,
                               bool phi_in_lds) {
  size_t doubles = static_cast<size_t>(waves) * (static_cast<size_t>(max_path_len) * kShapLanes + max_tree_elems);
  if (phi_in_lds) doubles += static_cast<size_t>(num_features + 1);
  return doubles * sizeof(double) + static_cast<size_t>(waves) * ShapLeafMaskWords(mask_words) * sizeof(uint32_t);
}

// workgroups of a leaves-on-lanes launch over `rows` rows (a workgroup strides over the rows by it)
inline int ShapLeafGrid(int64_t rows) { return static_cast<int>(rows < 1 ? 1 : (rows > 16384 ? 16384 : rows)); }

// The rule.  Leaves-on-lanes where the call has fewer than leaf_max_rows rows (or the caller
// asks for it) and a workgroup of some W of the ladder fits in kShapLdsBytes, the widest such W,
// the accumulator in LDS if that still fits; else rows-on-lanes within its own limits (paths of at
// most kShapMaxPathLen elements, at most kMaxPredClasses trees per iteration, its path weights and
// masks within kShapLdsBytes); else none.  A caller who asks for a kernel that cannot serve the
// model gets none.
inline ShapPlan PlanShap(int64_t rows, const ShapModel& m, int choice,
                         int64_t leaf_max_rows = tuning::kShapLeafMaxRows) {
  ShapPlan none{kShapKernelNone, 0, 0, 0};
  if (m.num_class < 1 || m.num_class > kMaxPredClasses || m.max_path_len < 1 || m.max_path_len > kShapMaxPathLen) {
    return none;
  }
  const size_t budget = static_cast<size_t>(kShapLdsBytes);
  const int mask_words = ShapMaskWords(m.max_leaves);
  if (choice == kShapChoiceLeaves || (choice == kShapChoiceAuto && rows < leaf_max_rows)) {
    for (int k = 0; k < kShapLeafWaveSteps; ++k) {
      const int w = kShapLeafWaveLadder[k];
      for (int phi = 1; phi >= 0; --phi) {
        const size_t bytes = ShapLeafLdsBytes(w, m.max_path_len, m.max_tree_elems, mask_words, m.num_features, phi != 0);
        if (bytes <= budget) return {kShapKernelLeaves, w, phi, bytes};
      }
    }
    if (choice == kShapChoiceLeaves) return none;
  }
  if (ShapRowsLdsBytes(m.max_path_len, mask_words, m.num_features, false) > budget) return none;
  const size_t with_phi = ShapRowsLdsBytes(m.max_path_len, mask_words, m.num_features, true);
  if (with_phi <= budget) return {kShapKernelRows, 1, 1, with_phi};
  return {kShapKernelRows, 1, 0, ShapRowsLdsBytes(m.max_path_len, mask_words, m.num_features, false)};
}

}  // namespace dev
}  // namespace lgbm_amd
