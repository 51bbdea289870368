// Host-only driver of the CSC binning rule and the column-wise bin sample (src/device/csc_bins.h)
// for the sanitizer test: the hand-written tables of csr_bins_driver.cpp -- a bundle of two
// features, a feature whose zeros are pushed, a feature with a NaN bin, columns without a feature
// -- and a matrix with the edge cases of tests/test_csc_bins.py (an empty column, a column of one
// entry, cells stored twice, a column out of row order, both members of the bundle on one row,
// rows -1, num_row and 2^31 - 1, a column past num_total_features, stored zeros and NaN) through
// EvalCscToGroupBins and CscColumnSample, into buffers that end exactly where the matrix ends;
// then pointers that are negative, descend or pass the entries, and a matrix without rows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../src/device/csc_bins.h"

using lgbm_amd::dev::CscColumnSample;
using lgbm_amd::dev::CsrBinFeat;
using lgbm_amd::dev::CsrBinTables;
using lgbm_amd::dev::EvalCscToGroupBins;

static int failures = 0;

template <typename T, typename P>
static void Run(const char* what) {
  const double inf = std::numeric_limits<double>::infinity();
  // features: A (column 1) and B (column 3) in group 0, C (column 4, zeros pushed) in group 1,
  // D (column 6, NaN bin) in group 2
  const std::vector<double> ub = {1e-35, 1.0, 2.0, inf,  // A: 4 bins, most frequent 0
                                  1e-35, 5.0, inf,       // B: 3 bins, most frequent 0
                                  1e-35, 1.5, inf,       // C: 3 bins, most frequent 1 (the value 1.0)
                                  0.5, inf, NAN};        // D: 2 bins + the NaN bin, most frequent 0
  const std::vector<CsrBinFeat> feats = {{3, -1, 0, 0, 1u, 0, -1, 0},
                                         {2, -1, 0, 4, 4u, 0, -1, 0},
                                         {2, -1, 1, 7, 1u, 1, 0, 0},
                                         {1, 2, 0, 10, 1u, 2, -1, 0}};
  const std::vector<int32_t> feat_of = {-1, 0, -1, 1, 2, -1, 3, -1};
  const std::vector<int32_t> push_zero = {2};
  CsrBinTables t;
  t.feat_of = feat_of.data();
  t.num_total_features = static_cast<int32_t>(feat_of.size());
  t.feats = feats.data();
  t.ub = ub.data();
  t.push_zero = push_zero.data();
  t.num_push_zero = 1;
  t.num_groups = 3;
  const int64_t num_row = 5;
  const std::vector<P> col_ptr = {0, 1, 5, 5, 7, 14, 15, 17, 17, 18};
  const std::vector<int32_t> indices = {0,                             // column 0: no feature
                                        1, 2, 2, 4,                    // A: row 2 twice, the second a zero
                                        1, 4,                          // B: over A on row 1
                                        3, 3, 2, -1, 5, INT32_MAX, 4,  // C: row 3 twice, out of order, rows outside
                                        0,                             // column 5: no feature
                                        2, 3,                          // D
                                        0};                            // column 8: past num_total_features
  const std::vector<T> data = {9, 1.5, 1.5, 0, NAN, 7, 5, 9, 1, 1, 3, 3, 3, 0, 1, NAN, T(0.7), 1};
  const std::vector<int32_t> want = {0, 1, 0,   // the pushed zero of C
                                     5, 1, 0,   // B, the higher column, over A; C unnamed
                                     2, 0, 2,   // the first A survives the zero; C named and silent; D NaN
                                     0, 3, 1,   // the first C survives its most frequent value
                                     4, 1, 0};  // A's NaN is 0.0: nothing; B; C's stored zero
  const int64_t ncol = static_cast<int64_t>(col_ptr.size()) - 1, nelem = static_cast<int64_t>(data.size());
  std::vector<int32_t> out(num_row * 3, 7);
  EvalCscToGroupBins(col_ptr.data(), ncol, indices.data(), data.data(), nelem, num_row, t, out.data());
  for (size_t i = 0; i < want.size(); ++i) {
    if (out[i] != want[i]) {
      std::fprintf(stderr, "%s: cell %zu is %d, expected %d\n", what, i, out[i], want[i]);
      ++failures;
    }
  }
  // the bin sample of C over rows 0, 2, 3, 4 (positions 0 .. 3): row 3's two entries after row 2's,
  // the stored zero and the rows outside dropped
  const std::vector<int32_t> pos = {0, -1, 1, 2, 3};
  std::vector<double> values;
  std::vector<int> positions;
  CscColumnSample(col_ptr.data(), 4, indices.data(), data.data(), nelem, pos.data(), num_row, 1e-35, &values, &positions);
  const std::vector<double> want_values = {1, 9, 1};
  const std::vector<int> want_positions = {1, 2, 2};
  if (values != want_values || positions != want_positions) {
    std::fprintf(stderr, "%s: the sample of column 4 differs\n", what);
    ++failures;
  }
  // pointers that are negative, descend or pass the entries are clamped: nothing outside is read
  const std::vector<P> wild = {-5, 3, 1, 100, 2, 18, 0, 19, -1, 18};
  EvalCscToGroupBins(wild.data(), ncol, indices.data(), data.data(), nelem, num_row, t, out.data());
  for (int col = 0; col < ncol; ++col) {
    CscColumnSample(wild.data(), col, indices.data(), data.data(), nelem, pos.data(), num_row, 1e-35, &values, &positions);
    CscColumnSample(col_ptr.data(), col, indices.data(), data.data(), nelem, pos.data(), num_row, 1e-35, &values, &positions);
  }
  // fewer entries than the pointer says, no rows, no groups and no zeros to push
  EvalCscToGroupBins(col_ptr.data(), ncol, indices.data(), data.data(), nelem - 6, num_row, t, out.data());
  EvalCscToGroupBins(col_ptr.data(), ncol, indices.data(), data.data(), nelem, 0, t, out.data());
  CscColumnSample(col_ptr.data(), 4, indices.data(), data.data(), nelem, pos.data(), 0, 1e-35, &values, &positions);
  CsrBinTables none = t;
  none.num_groups = 0;
  none.num_push_zero = 0;
  none.num_total_features = 0;
  EvalCscToGroupBins(col_ptr.data(), ncol, indices.data(), data.data(), nelem, num_row, none, out.data());
}

int main() {
  Run<float, int32_t>("float32 int32");
  Run<float, int64_t>("float32 int64");
  Run<double, int32_t>("float64 int32");
  Run<double, int64_t>("float64 int64");
  if (failures != 0) return 1;
  std::printf("csc bins driver ok\n");
  return 0;
}
