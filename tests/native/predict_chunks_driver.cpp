// Host-only driver of the chunk-size rule of device prediction (src/boosting/predict_chunks.h)
// for the sanitizer test: the table of tests/test_predict_chunks.py with a tile of 64 rows, the
// pointers in vectors that end at their last entry, so that a scan past row nrow is reported.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../src/boosting/predict_chunks.h"

using lgbm_amd::MostChunkEntries;
using lgbm_amd::PlanPredictChunks;
using lgbm_amd::PredictChunkPlan;

static int failures = 0;

// chunk < 0: the plan must not fit
static void Case(const char* name, int64_t nrow, size_t budget, size_t fixed, int64_t forced,
                 const std::vector<int64_t>* ptr, int64_t chunk, int64_t entries) {
  const size_t per_entry = ptr != nullptr ? 12 : 0;
  const PredictChunkPlan p = PlanPredictChunks(nrow, budget, fixed, 100, per_entry, forced, 64, [&](int64_t rows) {
    return ptr != nullptr ? MostChunkEntries(*ptr, nrow, rows) : int64_t{0};
  });
  const bool ok = chunk < 0 ? !p.fits : (p.fits && p.chunk == chunk && p.entries == entries);
  if (!ok) {
    std::printf("%s: chunk %lld entries %lld fits %d, expected chunk %lld entries %lld\n", name,
                static_cast<long long>(p.chunk), static_cast<long long>(p.entries), p.fits ? 1 : 0,
                static_cast<long long>(chunk), static_cast<long long>(entries));
    ++failures;
  }
}

static std::vector<int64_t> Uniform(int64_t nrow) {
  std::vector<int64_t> ptr(nrow + 1);
  for (int64_t r = 0; r <= nrow; ++r) ptr[r] = 10 * r;
  return ptr;
}

int main() {
  const std::vector<int64_t> u4096 = Uniform(4096), u3000 = Uniform(3000), u1000 = Uniform(1000);
  std::vector<int64_t> skewed(4097);  // rows 0-63 hold 1000 entries each, the rest none
  for (int64_t r = 0; r <= 4096; ++r) skewed[r] = std::min<int64_t>(r, 64) * 1000;
  Case("whole budget", 100000, 1000000, 0, 0, nullptr, 9984, 0);
  Case("capped by rows", 5000, 1000000, 0, 0, nullptr, 5000, 0);
  Case("one tile exactly", 5000, 6400, 0, 0, nullptr, 64, 0);
  Case("one byte short", 5000, 6399, 0, 0, nullptr, -1, 0);
  Case("fixed over budget", 5000, 1000, 2000, 0, nullptr, -1, 0);
  Case("uniform entries halve once", 4096, 500000, 8, 0, &u4096, 2048, 20480);
  Case("rows not a tile multiple", 3000, 400000, 0, 0, &u3000, 1472, 14720);
  Case("skewed", 4096, 800000, 0, 0, &skewed, 256, 64000);
  Case("skewed, never fits", 4096, 760000, 0, 0, &skewed, -1, 0);
  Case("forced, tiny budget", 1000, 1, 0, 192, &u1000, 192, 1920);
  Case("forced over rows", 3000, 1000000, 0, 5000, nullptr, 3000, 0);
  Case("forced over rows, entries", 3000, 1, 0, 5000, &u3000, 3000, 30000);
  if (failures != 0) {
    std::printf("predict chunks driver: %d failures\n", failures);
    return 1;
  }
  std::printf("predict chunks driver ok\n");
  return 0;
}
