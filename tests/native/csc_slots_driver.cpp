// Host-only driver of the CSC entry rule (src/device/csc_slots.h) for the sanitizer test: the
// hand-written hostile matrix of tests/test_csc_slots.py -- cells stored twice and three times,
// empty columns, a slot without a column, a pointer past the entries, and row indices -1, num_row
// and 2^31 - 1 -- through EvalCscToSlots for every row window, into a buffer that ends exactly
// where the matrix ends, so that a write outside it is a heap overflow.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

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

int main() {
  Run<float, int32_t>("float32 int32");
  Run<float, int64_t>("float32 int64");
  Run<double, int32_t>("float64 int32");
  Run<double, int64_t>("float64 int64");
  if (failures != 0) return 1;
  std::printf("csc slots driver ok\n");
  return 0;
}
