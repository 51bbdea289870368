#include "shap_paths.h"

#include <algorithm>
#include <cstring>

#include "../device/forest_decision.h"
#include "lgbm_amd/log.h"

namespace lgbm_amd {

void FlatForest::Build(const std::vector<const Tree*>& trees) {
  const int nt = static_cast<int>(trees.size());
  node_off.assign(nt + 1, 0);
  leaf_off.assign(nt, 0);
  cat_bound_off.assign(nt, 0);
  cat_bits_off.assign(nt, 0);
  for (int i = 0; i < nt; ++i) {
    const Tree* tr = trees[i];
    node_off[i] = static_cast<int32_t>(feature.size());
    leaf_off[i] = static_cast<int32_t>(leaf_value.size());
    cat_bound_off[i] = static_cast<int32_t>(cat_bound.size());
    cat_bits_off[i] = static_cast<int32_t>(cat_bits.size());
    const int nl = tr->num_leaves();
    for (int j = 0; j + 1 < nl; ++j) {
      feature.push_back(tr->split_feature(j));
      threshold.push_back(tr->threshold(j));
      dtype.push_back(tr->decision_type(j));
      left.push_back(tr->left_child(j));
      right.push_back(tr->right_child(j));
    }
    for (int j = 0; j < nl; ++j) leaf_value.push_back(tr->LeafOutput(j));
    cat_bound.insert(cat_bound.end(), tr->cat_boundaries().begin(), tr->cat_boundaries().end());
    cat_bits.insert(cat_bits.end(), tr->cat_threshold().begin(), tr->cat_threshold().end());
  }
  node_off[nt] = static_cast<int32_t>(feature.size());
}

void FlatForest::HostArgs(dev::ForestArgs* f) const {
  f->num_trees = static_cast<int32_t>(leaf_off.size());
  f->node_off = node_off.data();
  f->leaf_off = leaf_off.data();
  f->feature = feature.data();
  f->threshold = threshold.data();
  f->dtype = dtype.data();
  f->left = left.data();
  f->right = right.data();
  f->leaf_value = leaf_value.data();
  f->cat_bound_off = cat_bound_off.data();
  f->cat_bound = cat_bound.data();
  f->cat_bits_off = cat_bits_off.data();
  f->cat_bits = cat_bits.data();
}

void FeatureSlots::Build(const FlatForest& flat, int num_features) {
  slot_of.assign(std::max(0, num_features), -1);
  for (const int32_t f : flat.feature) {
    if (f < 0 || f >= num_features) Log::Fatal("a tree splits on feature %d, the model has %d", f, num_features);
    slot_of[f] = 0;
  }
  used.clear();
  for (int f = 0; f < num_features; ++f) {
    if (slot_of[f] == 0) {
      slot_of[f] = static_cast<int32_t>(used.size());
      used.push_back(f);
    }
  }
  feature.resize(flat.feature.size());
  for (size_t i = 0; i < feature.size(); ++i) feature[i] = slot_of[flat.feature[i]];
}

bool ShapPathTables::Build(const std::vector<const Tree*>& trees) {
  const int nt = static_cast<int>(trees.size());
  tree_leaf_off.assign(1, 0);
  leaf_elem_off.assign(1, 0);
  elem_pair_off.assign(1, 0);
  max_path_len = 1;
  mask_words = 0;
  struct Step {
    int node;
    bool left;
  };
  std::vector<Step> steps;
  for (int t = 0; t < nt; ++t) {
    const Tree* tr = trees[t];
    expected.push_back(tr->ExpectedValue());
    const int nl = tr->num_leaves();
    if (nl > 1) {
      mask_words = std::max(mask_words, (nl - 1 + 31) / 32);
      // leaves in index order: each one's path by walking up from its parent
      std::vector<int> parent(nl - 1, -1), leaf_parent(nl, -1);
      for (int j = 0; j + 1 < nl; ++j) {
        for (const int c : {tr->left_child(j), tr->right_child(j)}) {
          if (c >= 0) parent[c] = j;
          else leaf_parent[~c] = j;
        }
      }
      for (int leaf = 0; leaf < nl; ++leaf) {
        steps.clear();
        int child = ~leaf;
        for (int node = leaf_parent[leaf]; node >= 0; node = parent[node]) {
          steps.push_back({node, tr->left_child(node) == child});
          child = node;
        }
        std::reverse(steps.begin(), steps.end());
        const int first_elem = static_cast<int>(elem_feature.size());
        std::vector<std::vector<int32_t>> elem_pairs;
        for (const Step& s : steps) {
          const int next = s.left ? tr->left_child(s.node) : tr->right_child(s.node);
          if (tr->data_count(s.node) == 0 || tr->data_count(next) == 0) return false;
          const double frac = tr->data_count(next) / static_cast<double>(tr->data_count(s.node));
          const int feat = tr->split_feature(s.node);
          int e = first_elem;
          while (e < static_cast<int>(elem_feature.size()) && elem_feature[e] != feat) ++e;
          if (e == static_cast<int>(elem_feature.size())) {
            elem_feature.push_back(feat);
            elem_zero.push_back(1.0);
            elem_pairs.emplace_back();
          }
          elem_zero[e] = frac * elem_zero[e];
          elem_pairs[e - first_elem].push_back(static_cast<int32_t>(s.node) << 1 | (s.left ? 1 : 0));
        }
        for (const auto& p : elem_pairs) {
          pairs.insert(pairs.end(), p.begin(), p.end());
          elem_pair_off.push_back(static_cast<int32_t>(pairs.size()));
        }
        leaf_elem_off.push_back(static_cast<int32_t>(elem_feature.size()));
        leaf_value.push_back(tr->LeafOutput(leaf));
        max_path_len = std::max(max_path_len, static_cast<int>(elem_feature.size()) - first_elem + 1);
      }
    }
    tree_leaf_off.push_back(static_cast<int32_t>(leaf_value.size()));
  }
  // (D - j) / (D + 1) for every path of D elements, at ShapRatioOffset(D) + j
  ratio.assign(dev::ShapRatioOffset(max_path_len) + 1, 0.0);
  for (int d = 1; d < max_path_len; ++d) {
    for (int j = 0; j < d; ++j) ratio[dev::ShapRatioOffset(d) + j] = (d - j) / static_cast<double>(d + 1);
  }
  return true;
}

void ShapPathTables::HostArgs(dev::ShapArgs* a) const {
  a->max_path_len = max_path_len;
  a->mask_words = mask_words;
  a->tree_leaf_off = tree_leaf_off.data();
  a->leaf_elem_off = leaf_elem_off.data();
  a->leaf_value = leaf_value.data();
  a->elem_feature = elem_feature.data();
  a->elem_zero = elem_zero.data();
  a->elem_pair_off = elem_pair_off.data();
  a->pairs = pairs.data();
  a->expected = expected.data();
  a->ratio = ratio.data();
}

bool ShapPathTables::FitsDevice() const {
  if (max_path_len > dev::kShapMaxPathLen) return false;
  dev::ShapArgs a{};
  a.max_path_len = max_path_len;
  a.mask_words = mask_words;
  return dev::ShapLdsBytes(a, false) <= static_cast<size_t>(dev::kShapLdsBytes);
}

void EvalPathTables(const dev::ForestArgs& f, const dev::ShapArgs& a, double* out) {
  const int F1 = a.num_features + 1;
  const double* x = static_cast<const double*>(f.data);
#pragma omp parallel
  {
    std::vector<double> pw(a.max_path_len);
    std::vector<uint32_t> mask(std::max(1, a.mask_words));
    std::vector<char> ones(a.max_path_len);
#pragma omp for schedule(static)
    for (int64_t row = 0; row < f.num_rows; ++row) {
      auto value = [&](int feat) {
        return f.row_major ? x[row * f.num_cols + feat] : x[static_cast<int64_t>(feat) * f.num_rows + row];
      };
      for (int k = 0; k < f.num_class; ++k) {
        double* phi = out + (row * f.num_class + k) * F1;
        std::fill(phi, phi + F1, 0.0);
        for (int t = k; t < f.num_trees; t += f.num_class) {
          phi[a.num_features] += a.expected[t];
          const int l0 = a.tree_leaf_off[t], l1 = a.tree_leaf_off[t + 1];
          if (l0 == l1) continue;
          const int n0 = f.node_off[t], nn = f.node_off[t + 1] - n0;
          std::fill(mask.begin(), mask.end(), 0u);
          for (int j = 0; j < nn; ++j) {
            if (dev::ForestGoesLeft(f, t, n0 + j, value(f.feature[n0 + j]))) mask[j >> 5] |= 1u << (j & 31);
          }
          for (int l = l0; l < l1; ++l) {
            const int e0 = a.leaf_elem_off[l], D = a.leaf_elem_off[l + 1] - e0;
            pw[0] = 1.0;
            for (int d = 1; d <= D; ++d) {
              const int e = e0 + d - 1;
              bool one = true;
              for (int p = a.elem_pair_off[e]; p < a.elem_pair_off[e + 1]; ++p) {
                const int pr = a.pairs[p], node = pr >> 1;
                const uint32_t went_left = (mask[node >> 5] >> (node & 31)) & 1u;
                one = one && went_left == static_cast<uint32_t>(pr & 1);
              }
              ones[d] = one;
              const double zero = a.elem_zero[e];
              const double dp1 = static_cast<double>(d + 1);
              double carry = 0.0;
              for (int i = d - 1; i >= 0; --i) {
                const double p = pw[i];
                const double up = p * (i + 1) / dp1;
                pw[i + 1] = carry + (one ? up : 0.0);
                carry = zero * p * (d - i) / dp1;
              }
              pw[0] = carry;
            }
            const double lv = a.leaf_value[l];
            const double* ratio = a.ratio + dev::ShapRatioOffset(D);
            const double Dp1 = static_cast<double>(D + 1);
            const double top = pw[D];
            for (int i = 1; i <= D; ++i) {
              const int e = e0 + i - 1;
              const double zero = a.elem_zero[e];
              const bool one = ones[i] != 0;
              double next_one = top, total = 0.0;
              for (int j = D - 1; j >= 0; --j) {
                const double p = pw[j];
                const double r = ratio[j];
                const double q = (one ? next_one * Dp1 : p) / (one ? static_cast<double>(j + 1) : zero);
                total += one ? q : q / r;
                next_one = p - q * zero * r;
              }
              phi[a.elem_feature[e]] += total * ((one ? 1.0 : 0.0) - zero) * lv;
            }
          }
        }
      }
    }
  }
}

}  // namespace lgbm_amd
