// Host-only driver of the rule that plans the device build of the binned rows
// (src/device/storage_plan.h) for the sanitizer test: the table of tests/test_storage_plan.py.
#include <cstdint>
#include <cstdio>

#include "../../src/device/storage_plan.h"

using lgbm_amd::PlanStorage;
using lgbm_amd::StoragePlan;

struct Case {
  const char* name;
  int64_t rows, col_row_bytes, row_bytes, free_bytes;
  int keep;
  int64_t want[6];  // kept, window rows, window stride, window bytes, staging bytes, windows
};

static const int64_t GiB = int64_t{1} << 30, MiB = int64_t{1} << 20;

static const Case kCases[] = {
    {"kept at 8 GiB", GiB, 8, 8, 48 * GiB, -1, {1, GiB, GiB, 0, 64 * MiB, 1}},
    {"one row past 8 GiB", GiB + 1, 8, 8, 48 * GiB, -1, {0, GiB + 1, GiB + 4, 8 * GiB + 32, 64 * MiB, 1}},
    {"window fits exactly", 1000, 10, 0, 56384, 0, {0, 1000, 1000, 10000, 4096, 1}},
    {"window halved", 1000, 10, 0, 56000, 0, {0, 500, 500, 5000, 4096, 2}},
    {"one row, kept", 1, 40, 64, 0, -1, {1, 1, 4, 0, 4096, 1}},
    {"one row, no memory", 1, 40, 64, 0, 0, {0, 1, 4, 160, 4096, 1}},
    {"stride product past 2^31", 1000000000, 40, 40, 256 * GiB, -1, {0, 1000000000, 1000000000, 40000000000, 64 * MiB, 1}},
    {"six windows of a billion rows", 1000000000, 40, 40, 64 * GiB, -1, {0, 166666667, 166666668, 6666666720, 64 * MiB, 6}},
};

int main() {
  int failures = 0;
  for (const Case& c : kCases) {
    const StoragePlan p = PlanStorage(c.rows, c.col_row_bytes, c.row_bytes, c.free_bytes, c.keep);
    const int64_t got[6] = {p.keep_columns ? 1 : 0, p.window_rows, p.window_stride, p.window_bytes, p.staging_bytes, p.windows};
    for (int i = 0; i < 6; ++i) {
      if (got[i] != c.want[i]) {
        std::printf("%s: out[%d] = %lld, expected %lld\n", c.name, i, static_cast<long long>(got[i]),
                    static_cast<long long>(c.want[i]));
        ++failures;
      }
    }
  }
  if (failures != 0) {
    std::printf("storage plan driver: %d failures\n", failures);
    return 1;
  }
  std::printf("storage plan driver ok\n");
  return 0;
}
