// Host-only driver of the CSC entry rule (src/device/csc_slots.h) for the sanitizer test: the
// hand-written hostile matrix of tests/test_csc_slots.py -- cells stored twice and three times,
// empty columns, a slot without a column, a pointer past the entries, and row indices -1, num_row
// and 2^31 - 1 -- through EvalCscToSlots for every row window, into a buffer that ends exactly
// where the matrix ends, so that a write outside it is a heap overflow.  Then PackColumnRuns
// (include/lgbm_amd/sparse_ptr.h), the packing of a set of columns for upload, against a direct
// computation: adjacent columns, an empty column between two used ones, a gap, used columns past
// the matrix's width, a single column.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lgbm_amd/sparse_ptr.h"
#include "../../src/device/csc_slots.h"

using lgbm_amd::dev::EvalCscToSlots;

static int failures = 0;

template <typename T, typename P>
static void Run(const char* what) {
  const int64_t num_row = 12;
  // columns 0 .. 4 of the matrix; the slots are columns 1, 3, 4 and a feature the matrix does not have
  const std::vector<P> col_ptr = {0, 0, 4, 7, 13, 40};  // (the last column ends past the entries)
  const std::vector<int32_t> indices = {5, 2, 5, 9,                               // column 1: row 5 twice
                                        0, 1, 2,                                   // column 2: no slot
                                        4, 4, 0, 4, 7, 7,                          // column 3: row 4 three times
                                        -1, 3, 12, 1, INT32_MAX, 11};              // column 4: rows outside
  const std::vector<T> data = {1, 2, 3, 0, 1.5, 2.5, 3.5, 4, 5, 6, 0, 7, 0, 9, 8, 9, NAN, 9, -2.5};
  const std::vector<int32_t> slot_col = {1, 3, 4, -1};
  const int ns = static_cast<int>(slot_col.size());
  const int64_t nelem = static_cast<int64_t>(data.size());
  std::vector<T> whole(num_row * ns, T(7));
  EvalCscToSlots(col_ptr.data(), slot_col.data(), indices.data(), data.data(), nelem, 0, num_row, ns, whole.data());
  std::vector<T> want(num_row * ns, T(0));
  want[5 * ns + 0] = 3;
  want[2 * ns + 0] = 2;
  want[0 * ns + 1] = 6;
  want[3 * ns + 2] = 8;
  want[1 * ns + 2] = NAN;
  want[11 * ns + 2] = T(-2.5);
  for (size_t i = 0; i < want.size(); ++i) {
    const bool same = std::isnan(want[i]) ? std::isnan(whole[i]) : want[i] == whole[i];
    if (!same) {
      std::fprintf(stderr, "%s: cell %zu is %g, expected %g\n", what, i, double(whole[i]), double(want[i]));
      ++failures;
    }
  }
  // every window of rows equals the slice of the whole (a buffer of exactly rows x slots)
  for (int64_t row0 = 0; row0 <= num_row; ++row0) {
    for (int64_t rows = 0; row0 + rows <= num_row; ++rows) {
      std::vector<T> part(rows * ns, T(7));
      EvalCscToSlots(col_ptr.data(), slot_col.data(), indices.data(), data.data(), nelem, row0, rows, ns, part.data());
      for (int64_t i = 0; i < rows * ns; ++i) {
        const T w = whole[row0 * ns + i];
        if (!(std::isnan(w) ? std::isnan(part[i]) : w == part[i])) {
          std::fprintf(stderr, "%s: window (%lld, %lld) differs at %lld\n", what, static_cast<long long>(row0),
                       static_cast<long long>(rows), static_cast<long long>(i));
          ++failures;
        }
      }
    }
  }
  // a pointer that is negative or descends is clamped as well: nothing is read outside the entries
  const std::vector<P> wild = {-5, 3, 1, 100, 2, 19};
  std::vector<T> out(num_row * ns);
  EvalCscToSlots(wild.data(), slot_col.data(), indices.data(), data.data(), nelem, 0, num_row, ns, out.data());
}

// `columns` of the matrix under col_ptr: the runs copy exactly the entries of the columns, in
// order, to where `placed` says each column lies, and no two runs could have been one
template <typename P>
static void Pack(const char* what, const std::vector<P>& col_ptr, const std::vector<int32_t>& columns,
                 const std::vector<lgbm_amd::ColumnRun>& want_runs) {
  const int64_t ncol = static_cast<int64_t>(col_ptr.size()) - 1;
  std::vector<lgbm_amd::ColumnRun> runs;
  std::vector<int64_t> placed;
  lgbm_amd::PackColumnRuns(columns, lgbm_amd::SparsePtr{col_ptr.data(), sizeof(P) == 8}, ncol, &runs, &placed);
  bool ok = placed.size() == columns.size() + 1 && runs.size() == want_runs.size();
  // the direct computation: entry by entry, column after column
  std::vector<int64_t> src_of;
  for (size_t j = 0; ok && j < columns.size(); ++j) {
    ok = placed[j] == static_cast<int64_t>(src_of.size());
    if (columns[j] < ncol) {
      for (int64_t i = col_ptr[columns[j]]; i < col_ptr[columns[j] + 1]; ++i) src_of.push_back(i);
    }
    ok = ok && placed[j + 1] == static_cast<int64_t>(src_of.size());
  }
  std::vector<int64_t> copied(src_of.size(), -1);
  for (size_t k = 0; ok && k < runs.size(); ++k) {
    ok = runs[k].src == want_runs[k].src && runs[k].dst == want_runs[k].dst && runs[k].len == want_runs[k].len &&
         runs[k].len > 0 && runs[k].dst >= 0 && runs[k].dst + runs[k].len <= static_cast<int64_t>(copied.size());
    for (int64_t i = 0; ok && i < runs[k].len; ++i) copied[runs[k].dst + i] = runs[k].src + i;
  }
  if (!ok || copied != src_of) {
    std::fprintf(stderr, "pack %s (%zu-byte pointer): wrong runs or places\n", what, sizeof(P));
    ++failures;
  }
}

template <typename P>
static void PackCases() {
  // columns 0 .. 6 hold 3, 2, 0, 4, 0, 1, 5 entries
  const std::vector<P> col_ptr = {0, 3, 5, 5, 9, 9, 10, 15};
  Pack<P>("adjacent columns merge", col_ptr, {0, 1}, {{0, 0, 5}});
  Pack<P>("an empty column between two used ones still merges", col_ptr, {1, 3}, {{3, 0, 6}});
  Pack<P>("an empty used column between two used ones", col_ptr, {1, 2, 3}, {{3, 0, 6}});
  Pack<P>("a gap gives two runs", col_ptr, {0, 3, 6}, {{0, 0, 3}, {5, 3, 4}, {10, 7, 5}});
  Pack<P>("used columns past the width", col_ptr, {5, 6, 7, 9}, {{9, 0, 6}});
  Pack<P>("only columns past the width", col_ptr, {7, 8}, {});
  Pack<P>("a single column", col_ptr, {3}, {{5, 0, 4}});
  Pack<P>("a single empty column", col_ptr, {4}, {});
  Pack<P>("no column", col_ptr, {}, {});
}

int main() {
  PackCases<int32_t>();
  PackCases<int64_t>();
  Run<float, int32_t>("float32 int32");
  Run<float, int64_t>("float32 int64");
  Run<double, int32_t>("float64 int32");
  Run<double, int64_t>("float64 int64");
  if (failures != 0) return 1;
  std::printf("csc slots driver ok\n");
  return 0;
}
