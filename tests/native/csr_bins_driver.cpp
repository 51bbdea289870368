// Host-only driver of the CSR binning rule (src/device/csr_bins.h) for the sanitizer test: hand-
// written tables -- a bundle of two features, a feature whose zeros are pushed, a feature with a
// NaN bin, columns without a feature -- and rows with the edge cases of tests/test_csr_bins.py (an
// empty row, descending columns, a column stored twice, both members of the bundle, columns -1,
// past the end and 2^31 - 1, stored zeros and NaN) through EvalCsrToGroupBins, whole and for every
// window of rows, into buffers that end exactly where the matrix ends; then pointers that are
// negative, descend or pass the entries.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../src/device/csr_bins.h"

using lgbm_amd::dev::CsrBinFeat;
using lgbm_amd::dev::CsrBinTables;
using lgbm_amd::dev::EvalCsrToGroupBins;

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
  const std::vector<P> indptr = {0, 0, 2, 6, 13, 16};
  const std::vector<int32_t> indices = {3, 1,                               // row 1: descending, both of the bundle
                                        1, 1, 4, 6,                         // row 2: A twice, C at its most frequent bin
                                        4, 4, -1, 8, INT32_MAX, 6, 5,       // row 3: C twice, columns without a feature
                                        1, 3, 4};                           // row 4: NaN without a NaN bin, a stored zero
  const std::vector<T> data = {7, 1.5, 1.5, 0, 1, NAN, 9, 1, 3, 1, 1, T(0.7), 1, NAN, 5, 0};
  const std::vector<int32_t> want = {0, 1, 0,   // the pushed zero of C
                                     2, 1, 0,   // A, stored last, over B
                                     2, 0, 2,   // the first A survives the zero; C named and silent; D NaN
                                     0, 3, 1,   // the first C survives its most frequent value
                                     4, 1, 0};  // A's NaN is 0.0: nothing; B; C's stored zero
  const int64_t rows = static_cast<int64_t>(indptr.size()) - 1, nelem = static_cast<int64_t>(data.size());
  std::vector<int32_t> whole(rows * 3, 7);
  EvalCsrToGroupBins(indptr.data(), 0, indices.data(), data.data(), rows, nelem, t, whole.data());
  for (size_t i = 0; i < want.size(); ++i) {
    if (whole[i] != want[i]) {
      std::fprintf(stderr, "%s: cell %zu is %d, expected %d\n", what, i, whole[i], want[i]);
      ++failures;
    }
  }
  // every window of rows equals the slice of the whole, with and without an entry base
  for (int64_t r0 = 0; r0 <= rows; ++r0) {
    for (int64_t n = 0; r0 + n <= rows; ++n) {
      std::vector<int32_t> part(n * 3, 7), based(n * 3, 7);
      EvalCsrToGroupBins(indptr.data() + r0, 0, indices.data(), data.data(), n, nelem, t, part.data());
      const int64_t e0 = static_cast<int64_t>(indptr[r0]), e1 = static_cast<int64_t>(indptr[r0 + n]);
      const std::vector<int32_t> idx(indices.begin() + e0, indices.begin() + e1);  // (ends where the chunk ends)
      const std::vector<T> val(data.begin() + e0, data.begin() + e1);
      EvalCsrToGroupBins(indptr.data() + r0, e0, idx.data(), val.data(), n, e1 - e0, t, based.data());
      for (int64_t i = 0; i < n * 3; ++i) {
        if (part[i] != whole[r0 * 3 + i] || based[i] != whole[r0 * 3 + i]) {
          std::fprintf(stderr, "%s: window (%lld, %lld) differs at %lld\n", what, static_cast<long long>(r0),
                       static_cast<long long>(n), static_cast<long long>(i));
          ++failures;
        }
      }
    }
  }
  // pointers that are negative, descend or pass the entries are clamped: nothing outside is read
  const std::vector<P> wild = {-5, 3, 1, 100, 2, 16};
  std::vector<int32_t> out(rows * 3);
  EvalCsrToGroupBins(wild.data(), 0, indices.data(), data.data(), rows, nelem, t, out.data());
  // no groups, no zeros to push
  CsrBinTables none = t;
  none.num_groups = 0;
  none.num_push_zero = 0;
  none.num_total_features = 0;
  EvalCsrToGroupBins(indptr.data(), 0, indices.data(), data.data(), rows, nelem, none, out.data());
}

int main() {
  Run<float, int32_t>("float32 int32");
  Run<float, int64_t>("float32 int64");
  Run<double, int32_t>("float64 int32");
  Run<double, int64_t>("float64 int64");
  if (failures != 0) return 1;
  std::printf("csr bins driver ok\n");
  return 0;
}
