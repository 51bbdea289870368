// CSC columns into group bins (src/device/csc_bin_kernels.hip; host evaluator for tests without a
// GPU: LGBM_AMD_CscToGroupBins), and the bin sample of a CSC matrix taken column by column.
//
// The dataset is the one the host builds by transposing the matrix into rows (which appends to
// each row in ascending column order, and in stored order within a column: in ascending stored
// index) and pushing every row.  Put through the rule of one CSR row (src/device/csr_bins.h), for
// the groups whose members are all numerical:
//   - every group cell of every row starts at 0;
//   - the entries of a column are those between its pointers, clamped into [0, nelem]
//     (csc_slots.h CscColumnRange);
//   - a stored entry is dropped when its row index is outside [0, num_row), when its column is not
//     below num_total_features, or when the column maps to no feature of an eligible group;
//   - the value as double goes through ValueToBinNumerical; a bin equal to the feature's most
//     frequent bin writes nothing, any other writes bin - (mfb == 0) + goff into the cell
//     (row, group) (GroupCellOfBin, both shared with csr_bins.h);
//   - of several writes to one cell the one with the highest stored index wins: a cell stored twice
//     in one column, or two members of one bundle off their most frequent bins on one row (the
//     higher column wins; a higher column at its most frequent bin leaves the lower one's write);
//   - after all entries every feature of need_push_zeros_, in that vector's order, writes the bin
//     of 0.0 by the same rule into each row that no stored entry of its column names -- whatever
//     the entry's value: a stored 0, a stored NaN and one at the most frequent bin all name the row.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "csc_slots.h"
#include "csr_bins.h"

namespace lgbm_amd {
namespace dev {

// the row of a stored entry of a matrix of num_row rows, or -1: dropped
LGBM_AMD_HD int64_t CscBinEntryRow(int32_t index, int64_t num_row) { return CscEntryRow(index, 0, num_row); }

// the feature of column `col`, or -1: its entries are dropped
LGBM_AMD_HD int CscColumnBinFeat(const CsrBinTables& t, int64_t col) {
  return col >= 0 && col < t.num_total_features ? t.feat_of[col] : -1;
}

// the kernels' result on the host, row-major: out[num_row][t.num_groups]
template <typename T, typename P>
void EvalCscToGroupBins(const P* col_ptr, int64_t ncol, const int32_t* indices, const T* data, int64_t num_entries,
                        int64_t num_row, const CsrBinTables& t, int32_t* out) {
  std::fill(out, out + num_row * t.num_groups, 0);
  const int64_t rows = std::max<int64_t>(0, num_row);
  std::vector<char> named(static_cast<size_t>(std::max(0, t.num_push_zero)) * static_cast<size_t>(rows), 0);
  int group;
  uint32_t cell;
  for (int64_t col = 0; col < ncol; ++col) {
    const int f = CscColumnBinFeat(t, col);
    if (f < 0) continue;
    const CsrBinFeat& F = t.feats[f];
    int64_t s, e;
    CscColumnRange(col_ptr, static_cast<int>(col), num_entries, &s, &e);
    for (int64_t i = s; i < e; ++i) {
      const int64_t r = CscBinEntryRow(indices[i], num_row);
      if (r < 0) continue;
      if (F.pz >= 0) named[static_cast<size_t>(F.pz) * rows + r] = 1;
      if (CsrFeatWrite(t, F, static_cast<double>(data[i]), &group, &cell)) {
        out[r * t.num_groups + group] = static_cast<int32_t>(cell);
      }
    }
  }
  for (int k = 0; k < t.num_push_zero; ++k) {
    if (!CsrFeatWrite(t, t.feats[t.push_zero[k]], 0.0, &group, &cell)) continue;
    for (int64_t r = 0; r < rows; ++r) {
      if (!named[static_cast<size_t>(k) * rows + r]) out[r * t.num_groups + group] = static_cast<int32_t>(cell);
    }
  }
}

// The bin sample of a CSC matrix, column by column: pos[r] is the position of row r among the
// sampled rows, or -1.  Of column `col`, the stored entries on a sampled row inside the matrix whose
// value is not a zero (fabs(v) > zero_threshold, or NaN), ordered by sample position and, on one
// position, by stored index: what sampling the transposed rows one by one appends to the column.
template <typename T, typename P>
void CscColumnSample(const P* col_ptr, int col, const int32_t* indices, const T* data, int64_t num_entries,
                     const int32_t* pos, int64_t num_row, double zero_threshold, std::vector<double>* values,
                     std::vector<int>* positions) {
  values->clear();
  positions->clear();
  int64_t s, e;
  CscColumnRange(col_ptr, col, num_entries, &s, &e);
  std::vector<std::pair<int, double>> kept;
  bool ascends = true;
  for (int64_t i = s; i < e; ++i) {
    const int64_t r = CscBinEntryRow(indices[i], num_row);
    if (r < 0 || pos[r] < 0) continue;
    const double v = static_cast<double>(data[i]);
    if (!(std::fabs(v) > zero_threshold || std::isnan(v))) continue;
    ascends = ascends && (kept.empty() || kept.back().first <= pos[r]);
    kept.emplace_back(pos[r], v);
  }
  if (!ascends) {
    std::stable_sort(kept.begin(), kept.end(),
                     [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
  }
  values->reserve(kept.size());
  positions->reserve(kept.size());
  for (const auto& pv : kept) {
    positions->push_back(pv.first);
    values->push_back(pv.second);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
