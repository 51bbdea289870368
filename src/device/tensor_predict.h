// Prediction of a strided matrix in device memory (LGBM_AMD_BoosterPredictForDeviceMat:
// Booster.predict_device of a GPU tensor; kernels in src/device/tensor_predict_kernels.hip, host
// evaluator for tests without a GPU: LGBM_AMD_TensorPredictOnHost).  What the kernels and the
// evaluator share is stated here once:
//   - the plan: which route a window of trees takes and how many rows a workgroup's tile holds;
//   - the tile: the R rows of a workgroup by the S slots (the sorted features the window's trees
//     split on, FeatureSlots), elements in their own type, laid out [slot][row] with a pitch;
//   - the packed node: one 16-byte record per internal node in place of five arrays;
//   - the walk of one tree over a row of the tile, and the finish of a row of scores.
#pragma once

#include <cstdint>

#include "forest_decision.h"
#include "score_convert.h"
#include "tensor_bins.h"  // (WidenElement)

namespace lgbm_amd {
namespace dev {

// rows of a tile, tallest first: the plan takes the first whose tile fits the budget.  One step:
// a shorter tile holds more slots in the same LDS only with fewer waves on the CU, and was
// measured slower than the slots route (profiles/r21_tensor_predict.md: 128 and 64 rows)
constexpr int kTensorPredictSteps = 1;
constexpr int kTensorPredictLadder[kTensorPredictSteps] = {256};
// LDS bytes of a tile: three workgroups in the CU's 160 KiB.  The walk waits on dependent node
// loads that only other waves hide; 12 waves per CU is the fewest at which the tile kernel was
// measured ahead of the slots route; at 8 and at 6 it was behind
constexpr int kTensorPredictLdsBytes = 52 * 1024;
// a tree with more leaves than this cannot name its children in 16 bits (internal nodes
// 0 .. 32766, leaves ~0 .. ~32767)
constexpr int kPackedMaxLeaves = 32768;

constexpr int kTensorRouteTile = 0;   // k_predict_tile walks the tile
constexpr int kTensorRouteSlots = 1;  // k_tensor_to_slots, then the forest kernels of the sparse paths

// f(typed null pointer) for the element type of the C API's data_type code (0 float32, 1 float64,
// 4 float16, 5 bfloat16); false: the code is none of them
template <typename F>
inline bool DispatchTensorElement(int data_type, F&& f) {
  switch (data_type) {
    case 0: f(static_cast<const float*>(nullptr)); return true;
    case 1: f(static_cast<const double*>(nullptr)); return true;
    case 4: f(static_cast<const Float16Bits*>(nullptr)); return true;
    case 5: f(static_cast<const Bfloat16Bits*>(nullptr)); return true;
    default: return false;
  }
}

// elements between two slots of a tile of `rows` rows: the transposing write of the gather (lanes
// along the slots of one row) then lands on distinct banks -- an odd number of 4-byte words for
// 2- and 4-byte elements, one 8-byte element more for doubles
LGBM_AMD_HD int TensorTilePitch(int rows, int elem_size) { return rows + (elem_size == 2 ? 2 : 1); }

LGBM_AMD_HD int64_t TensorTileBytes(int num_slots, int rows, int elem_size) {
  return static_cast<int64_t>(num_slots) * TensorTilePitch(rows, elem_size) * elem_size;
}

struct TensorPredictPlan {
  int32_t route;  // kTensorRouteTile / kTensorRouteSlots
  int32_t rows;   // rows of a tile (route tile), of a workgroup of the slot gather otherwise
};

// predict_type: the C API's (0 normal, 1 raw scores, 2 leaf indices, 3 contributions)
LGBM_AMD_HD TensorPredictPlan PlanTensorPredict(int num_slots, int elem_size, int max_leaves, int predict_type) {
  TensorPredictPlan p{kTensorRouteSlots, kTensorPredictLadder[0]};
  if (predict_type == 3 || max_leaves > kPackedMaxLeaves) return p;
  for (int k = 0; k < kTensorPredictSteps; ++k) {
    if (TensorTileBytes(num_slots, kTensorPredictLadder[k], elem_size) <= kTensorPredictLdsBytes) {
      p.route = kTensorRouteTile;
      p.rows = kTensorPredictLadder[k];
      return p;
    }
  }
  return p;
}

// ---- early-stopped scores (pred_early_stop; reference src/boosting/prediction_early_stop.cpp and
// GBDT::PredictRaw, src/boosting/gbdt_prediction.cpp:13-32; the host's Predictor).  The option applies
// only to normal and raw scores of a booster whose objective does not need an accurate prediction
// (binary, multiclass, multiclassova, the ranking objectives); everywhere else it is ignored
// (GBDT::TensorStopRule decides).  A counter starts at the first iteration of the window; after every
// freq-th iteration, with all of that iteration's trees added, a row whose StopMargin is above the
// threshold (strictly) stops and keeps its sums, which FinishScoreRow then takes as they are.

// the margin of a row of class sums: 2 |s| for a binary booster (NumberOfClasses() == 1), the
// largest sum minus the second largest otherwise
LGBM_AMD_HD double StopMargin(const double* score, int num_class, bool binary) {
  if (binary) return 2.0 * __builtin_fabs(score[0]);
  double top = score[0] > score[1] ? score[0] : score[1], second = score[0] > score[1] ? score[1] : score[0];
  for (int k = 2; k < num_class; ++k) {
    const double s = score[k];
    if (s > top) {
      second = top;
      top = s;
    } else if (s > second) {
      second = s;
    }
  }
  return top - second;
}

// LDS bytes that a workgroup of the stop kernels takes beside its tile (src/device/early_stop.h:
// the period end): the moved rows' ids, a staging array of one class's sums -- one class at a
// time, since all 16 classes of 256 rows at once would be 32 KiB of the tile's 52; two arrays in
// turn when there are several classes, so that a class costs one barrier -- and the wave counts
// of two periods in turn (3104 bytes for one class, 5152 for more)
constexpr int kStopWaves = 4;  // waves of a workgroup of the stop kernels (256 rows)
LGBM_AMD_HD int TensorStopLdsBytes(int num_class) {
  const int rows = kTensorPredictLadder[0];
  return rows * 4 + (num_class > 1 ? 2 : 1) * rows * 8 + 2 * kStopWaves * 4;
}

// the plan of an early-stopped prediction: the same ladder in what the period end leaves of the budget
LGBM_AMD_HD TensorPredictPlan PlanTensorPredictStop(int num_slots, int elem_size, int max_leaves, int predict_type,
                                                    int num_class) {
  TensorPredictPlan p{kTensorRouteSlots, kTensorPredictLadder[0]};
  if (predict_type == 3 || max_leaves > kPackedMaxLeaves) return p;
  const int budget = kTensorPredictLdsBytes - TensorStopLdsBytes(num_class);
  for (int k = 0; k < kTensorPredictSteps; ++k) {
    if (TensorTileBytes(num_slots, kTensorPredictLadder[k], elem_size) <= budget) {
      p.route = kTensorRouteTile;
      p.rows = kTensorPredictLadder[k];
      return p;
    }
  }
  return p;
}

// One internal node.  theta: the threshold's bits (numerical), or the node's bitset as
// word offset into the forest's cat_bits | words << 32 (categorical); slot_dt: slot << 8 | decision
// type; children as in the tree, leaves as ~leaf
struct alignas(16) PackedNode {
  uint64_t theta;
  uint32_t slot_dt;
  int16_t left, right;
};

LGBM_AMD_HD PackedNode PackNode(int dt, double threshold, uint32_t bits_off, uint32_t bits_words, int slot, int left,
                                int right) {
  PackedNode n;
  if (dt & 1) {
    n.theta = static_cast<uint64_t>(bits_off) | (static_cast<uint64_t>(bits_words) << 32);
  } else {
    __builtin_memcpy(&n.theta, &threshold, sizeof(n.theta));
  }
  n.slot_dt = (static_cast<uint32_t>(slot) << 8) | (static_cast<uint32_t>(dt) & 255u);
  n.left = static_cast<int16_t>(left);
  n.right = static_cast<int16_t>(right);
  return n;
}

// the child that value v of the node's slot leads to
LGBM_AMD_HD int PackedNodeNext(const PackedNode& n, const uint32_t* cat_bits, double v) {
  const int dt = static_cast<int>(n.slot_dt & 255u);
  double threshold;
  __builtin_memcpy(&threshold, &n.theta, sizeof(threshold));
  const uint32_t* bits = nullptr;
  int nw = 0;
  if (dt & 1) {
    bits = cat_bits + static_cast<uint32_t>(n.theta);
    nw = static_cast<int>(n.theta >> 32);
  }
  return ForestGoesLeft(dt, threshold, bits, nw, v) ? n.left : n.right;
}

// the leaf of a tree (its num_nodes packed nodes at `nodes`) for the row whose slot values are at
// row_of_tile[slot * pitch]
template <typename T>
LGBM_AMD_HD int PackedTreeLeaf(const PackedNode* nodes, int num_nodes, const uint32_t* cat_bits, const T* row_of_tile,
                               int pitch) {
  if (num_nodes <= 0) return 0;
  int node = 0;
  while (node >= 0) {
    const PackedNode n = nodes[node];
    node = PackedNodeNext(n, cat_bits, WidenElement(row_of_tile[static_cast<int>(n.slot_dt >> 8) * pitch]));
  }
  return ~node;
}

// what the host predictor does to a row of raw scores (GBDT::Predict): the average of
// boosting=rf (divisor > 0: the iterations of the window), then the objective's output transform
// (conv_kind of ObjectiveFunction::DeviceOutputKind, or -1: none), by ConvertScoreRow itself
LGBM_AMD_HD void FinishScoreRow(double* score, int num_class, double divisor, int conv_kind, double conv_param) {
  if (divisor > 0.0) {
    for (int k = 0; k < num_class; ++k) score[k] /= divisor;
  }
  if (conv_kind > 0) ConvertScoreRow(conv_kind, conv_param, num_class, 1, 0, score, score);
}

}  // namespace dev
}  // namespace lgbm_amd
