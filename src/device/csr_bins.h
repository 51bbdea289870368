// CSR rows into group bins (src/device/csr_bin_kernels.hip; host evaluator for tests without a
// GPU: LGBM_AMD_CsrToGroupBins).  The rule of one row, shared by the kernel and the evaluator,
// states what Dataset::PushSparseRow + PushColumnValue + FeatureGroup::Set do to it, restricted
// to the groups whose members are all numerical (a categorical member keeps its group on the
// host):
//   - every group bin of the row starts at 0;
//   - the stored entries (those between the row's pointers, relative to the chunk's first entry
//     and clamped to its num_entries: stored_order.h ClampedRange) are taken in stored order; one
//     whose column is negative, is not below num_total_features or maps to no feature of those
//     groups is dropped;
//   - the value as double goes through ValueToBinNumerical (BinMapper::ValueToBin: NaN to the NaN
//     bin or to 0.0, the binary search over the upper bounds);
//   - a bin equal to the feature's most frequent bin writes nothing (an earlier write to the cell,
//     by this or another member of the bundle, survives); any other bin writes
//     bin - (mfb == 0) + bin_offsets[sub], and the last write to a cell wins;
//   - after the entries, every feature of need_push_zeros_ (default bin != most frequent bin), in
//     that vector's order, that no stored entry of the row named -- whatever its value -- gets
//     the bin of 0.0 written by the same rule.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// (a plain C++ program can include this header: tests/native/csr_bins_driver.cpp)
#include "stored_order.h"

namespace lgbm_amd {
namespace dev {

// a numerical feature of a device-eligible group
struct CsrBinFeat {
  int32_t hi;       // search range [0, hi): num_bin - 1, minus the NaN bin
  int32_t nan_bin;  // NaN -> this bin (missing_type NaN), or -1: NaN -> 0.0
  int32_t mfb;      // most frequent bin (not stored)
  int32_t ub_off;   // upper bounds at ub[ub_off ...]
  uint32_t goff;    // group bin of the feature's bin 1 (its bin_offsets entry)
  int32_t group;    // eligible group (a column of the output)
  int32_t pz;       // position among the push-zeros features, or -1
  int32_t pad;
};

struct CsrBinTables {
  const int32_t* feat_of;  // [num_total_features] column -> CsrBinFeat, or -1
  int32_t num_total_features;
  const CsrBinFeat* feats;
  const double* ub;
  const int32_t* push_zero;  // [num_push_zero] CsrBinFeat of each push-zeros feature, in push order
  int32_t num_push_zero;
  int32_t num_groups;  // eligible groups
};

// BinMapper::ValueToBin of a numerical feature
LGBM_AMD_HD int ValueToBinNumerical(double value, int hi, int nan_bin, const double* u) {
  if (value != value) {
    if (nan_bin >= 0) return nan_bin;
    value = 0.0;
  }
  int lo = 0;
  while (lo < hi) {
    const int mid = (lo + hi - 1) / 2;
    if (value <= u[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// the group bin a feature bin writes, or false: the most frequent bin writes nothing
LGBM_AMD_HD bool GroupCellOfBin(int bin, int mfb, uint32_t goff, uint32_t* cell) {
  if (bin == mfb) return false;
  if (mfb == 0) bin -= 1;
  *cell = static_cast<uint32_t>(bin) + goff;
  return true;
}

// the feature a stored entry on column `col` belongs to, or -1: dropped
LGBM_AMD_HD int CsrEntryBinFeat(const CsrBinTables& t, int col) {
  return col >= 0 && col < t.num_total_features ? t.feat_of[col] : -1;
}

// what feature F writes for `value`: the eligible group and the cell, or false
LGBM_AMD_HD bool CsrFeatWrite(const CsrBinTables& t, const CsrBinFeat& F, double value, int* group, uint32_t* cell) {
  *group = F.group;
  return GroupCellOfBin(ValueToBinNumerical(value, F.hi, F.nan_bin, t.ub + F.ub_off), F.mfb, F.goff, cell);
}

// the kernel's result on the host, row-major: out[rows][num_groups]
template <typename T, typename P>
void EvalCsrToGroupBins(const P* indptr, int64_t entry_base, const int32_t* indices, const T* data, int64_t rows,
                        int64_t num_entries, const CsrBinTables& t, int32_t* out) {
  std::fill(out, out + rows * t.num_groups, 0);
  std::vector<char> named(static_cast<size_t>(std::max(0, t.num_push_zero)));
  for (int64_t r = 0; r < rows; ++r) {
    int32_t* o = out + r * t.num_groups;
    std::fill(named.begin(), named.end(), 0);
    int64_t s, e;
    ClampedRange(indptr, r, entry_base, num_entries, &s, &e);
    int group;
    uint32_t cell;
    for (int64_t i = s; i < e; ++i) {
      const int f = CsrEntryBinFeat(t, indices[i]);
      if (f < 0) continue;
      const CsrBinFeat& F = t.feats[f];
      if (F.pz >= 0) named[F.pz] = 1;
      if (CsrFeatWrite(t, F, static_cast<double>(data[i]), &group, &cell)) o[group] = static_cast<int32_t>(cell);
    }
    for (int k = 0; k < t.num_push_zero; ++k) {
      if (named[k]) continue;
      if (CsrFeatWrite(t, t.feats[t.push_zero[k]], 0.0, &group, &cell)) o[group] = static_cast<int32_t>(cell);
    }
  }
}

}  // namespace dev
}  // namespace lgbm_amd
