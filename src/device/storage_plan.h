// How the device learner's training storage is built on the device (storage_kernels.hip,
// src/treelearner/gpu_learner_storage.cpp): whether the column image is kept, how many rows a
// temporary column window holds where it is not, and how large the upload staging is.  Plain
// 64-bit arithmetic over byte counts that host tests drive (tests/test_storage_plan.py,
// tests/native/storage_plan_driver.cpp).  Standard library only.
#pragma once

#include <algorithm>
#include <cstdint>

namespace lgbm_amd {

// the column image is the learner's column copy below this size (LGBM_AMD_COLUMN_COPY forces it)
constexpr int64_t kStorageKeepColumnBytes = int64_t{8} << 30;
// window + staging take at most 1 / kStorageShareDiv of the memory that is free once the row
// image (and a kept column image) are allocated; the staging at most a quarter of that share
constexpr int64_t kStorageShareDiv = 4;
constexpr int64_t kStorageStagingMax = int64_t{64} << 20;
// ... except for this floor of the staging, below which an upload would make no progress
constexpr int64_t kStorageStagingMin = 4096;
// a window's columns start at multiples of this many rows (16-bit columns stay aligned)
constexpr int64_t kStorageWindowAlign = 4;

struct StoragePlan {
  bool keep_columns;      // the column image stays: it is built whole, source and result
  int64_t window_rows;    // rows of a window (rows when the image is kept)
  int64_t window_stride;  // rows between the columns of a window (window_rows, aligned up)
  int64_t window_bytes;   // device bytes of the temporary column window (0 when kept)
  int64_t staging_bytes;  // device bytes of the upload staging
  int64_t windows;        // passes over the rows
};

// rows >= 1 rows of col_row_bytes column bytes and row_bytes row-image bytes each (0: row-sparse
// storage, no row image), free_bytes of free device memory before any of it is allocated.
// keep: 1 / 0 forces the column image kept / not kept, -1 decides by kStorageKeepColumnBytes.
// The rows are cut into the fewest equal windows that fit the share with the staging (a window
// one byte too large is halved); a window of one row always passes.
inline StoragePlan PlanStorage(int64_t rows, int64_t col_row_bytes, int64_t row_bytes, int64_t free_bytes, int keep) {
  StoragePlan p{};
  rows = std::max<int64_t>(1, rows);
  const int64_t col_bytes = rows * col_row_bytes;
  p.keep_columns = keep >= 0 ? keep != 0 : col_bytes <= kStorageKeepColumnBytes;
  const int64_t resident = rows * row_bytes + (p.keep_columns ? col_bytes : 0);
  const int64_t share = std::max<int64_t>(0, free_bytes - resident) / kStorageShareDiv;
  p.staging_bytes = std::min(kStorageStagingMax, std::max(kStorageStagingMin, share / 4));
  p.window_rows = rows;
  if (!p.keep_columns && col_row_bytes > 0) {
    int64_t most = std::max<int64_t>(1, (share - p.staging_bytes) / col_row_bytes);
    if (most >= kStorageWindowAlign) most = most / kStorageWindowAlign * kStorageWindowAlign;  // (the stride fits too)
    const int64_t passes = (rows + most - 1) / most;
    p.window_rows = (rows + passes - 1) / passes;
  }
  p.window_stride = (p.window_rows + kStorageWindowAlign - 1) / kStorageWindowAlign * kStorageWindowAlign;
  p.window_bytes = p.keep_columns ? 0 : p.window_stride * col_row_bytes;
  p.windows = (rows + p.window_rows - 1) / p.window_rows;
  return p;
}

}  // namespace lgbm_amd
