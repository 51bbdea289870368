// Host side of device prediction: the forest flattened into the node arrays of dev::ForestArgs,
// and the per-leaf path tables of dev::ShapArgs that turn the recursive TreeSHAP
// (Tree::TreeShapRec) into loops a GPU can run (src/device/shap_kernels.hip).
//
// A leaf's root-to-leaf nodes are grouped by split feature, in order of first occurrence; each
// group is one path element: the feature, zero_fraction = the product over the group's nodes of
// data_count(child on the path) / data_count(node), and the (node, direction) pairs whose
// decisions must all agree with the path for one_fraction to be 1 (else 0).  The recursion's
// unwind of a repeated feature followed by its re-extension with multiplied fractions is the
// same merged element.  The bias element (feature -1, both fractions 1) is implicit.
#pragma once

#include <cstdint>
#include <vector>

#include "../device/kernels.h"
#include "lgbm_amd/tree.h"

namespace lgbm_amd {

struct FlatForest {
  std::vector<int32_t> node_off, leaf_off, feature, left, right, cat_bound_off, cat_bound, cat_bits_off;
  std::vector<double> threshold, leaf_value;
  std::vector<int8_t> dtype;
  std::vector<uint32_t> cat_bits;

  void Build(const std::vector<const Tree*>& trees);
  // the forest fields of `f` pointing at these host vectors
  void HostArgs(dev::ForestArgs* f) const;
};

// The distinct features a forest splits on, for sparse rows (src/device/csr_slots.h): used[] is
// sorted, slot_of[feature] its position there (-1: no tree splits on the feature), and `feature`
// is FlatForest::feature rewritten to slots, with which the forest kernels walk a compact
// [rows x used.size()] matrix.  (ShapArgs::elem_feature keeps the real feature.)
struct FeatureSlots {
  std::vector<int32_t> used, slot_of, feature;

  void Build(const FlatForest& flat, int num_features);
};

struct ShapPathTables {
  std::vector<int32_t> tree_leaf_off, leaf_elem_off, elem_feature, elem_pair_off, pairs;
  std::vector<double> leaf_value, elem_zero, expected, ratio;
  int max_path_len = 1;  // longest path in elements, bias element included
  int mask_words = 0;    // 32-bit words of the widest tree's decision mask

  // false: a node on some path has data_count 0 (its zero fraction would divide by zero)
  bool Build(const std::vector<const Tree*>& trees);
  // the table fields of `a` pointing at these host vectors
  void HostArgs(dev::ShapArgs* a) const;
  // the device kernel can run these tables (path length and LDS limits)
  bool FitsDevice() const;
};

// The contributions of f.num_rows rows (f.data: host memory) from the tables, with the kernel's
// arithmetic in the kernel's order: out[row][class][F + 1].  `f` and `a` point at host memory.
void EvalPathTables(const dev::ForestArgs& f, const dev::ShapArgs& a, double* out);

}  // namespace lgbm_amd
