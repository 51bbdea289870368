// How many rows of a prediction pass through the device at a time (device_predict.cpp): one rule
// for dense, CSR and CSC inputs, plain arithmetic over byte counts that host tests drive
// (tests/test_predict_chunks.py, tests/native/predict_chunks_driver.cpp).  Standard library only.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace lgbm_amd {

struct PredictChunkPlan {
  int64_t chunk;    // rows of a chunk (the last one may be shorter)
  int64_t entries;  // the most stored entries that a chunk stages
  bool fits;        // false: not even one tile of rows fits the budget (the host predicts)
};

// the most stored entries of a chunk of `rows` of the nrow rows under ptr (nrow + 1 ascending entries)
template <typename Ptr>
int64_t MostChunkEntries(const Ptr& ptr, int64_t nrow, int64_t rows) {
  int64_t most = 0;
  for (int64_t r0 = 0; r0 < nrow; r0 += rows) {
    most = std::max<int64_t>(most, ptr[std::min(r0 + rows, nrow)] - ptr[r0]);
  }
  return most;
}

// nrow > 0 rows within `budget` bytes, of which `fixed` are held for the whole call, per_row > 0
// for every row of a chunk and per_entry for every stored entry that a chunk stages
// (most_entries(rows): the most of a chunk of `rows` rows; 0 for inputs that stage none).  A chunk
// is a multiple of `tile` rows, halved until it fits with its entries.  forced > 0 sets the chunk
// whatever fits (the test knob).
template <typename MostEntries>
PredictChunkPlan PlanPredictChunks(int64_t nrow, size_t budget, size_t fixed, size_t per_row, size_t per_entry,
                                   int64_t forced, int64_t tile, MostEntries&& most_entries) {
  PredictChunkPlan p{};
  p.chunk = budget > fixed ? static_cast<int64_t>((budget - fixed) / per_row) : 0;
  p.chunk = std::max(tile, p.chunk / tile * tile);
  if (forced > 0) p.chunk = forced;
  p.chunk = std::min(p.chunk, nrow);
  p.entries = most_entries(p.chunk);
  p.fits = true;
  while (forced <= 0 &&
         fixed + static_cast<size_t>(p.chunk) * per_row + static_cast<size_t>(p.entries) * per_entry > budget) {
    if (p.chunk <= tile) {
      p.fits = false;
      break;
    }
    p.chunk = std::max(tile, p.chunk / 2 / tile * tile);
    p.entries = most_entries(p.chunk);
  }
  return p;
}

}  // namespace lgbm_amd
