// Host-side launch interface of the kernels that build the device learner's training storage
// from a Dataset's group columns (storage_kernels.hip): the column image, the row words packed
// from it, and the row-sparse lists.  Every launcher is stream-ordered; row x stride offsets are
// 64-bit throughout.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace lgbm_amd {
namespace dev {

constexpr int kStorageThreads = 256;
constexpr int kStorageTileRows = 256;    // rows of a pack tile: one per thread
constexpr int kStorageSliceWords = 32;   // words of a pack tile (a 128-B line of each row)
constexpr int kStorageScanPerThread = 4;
constexpr int kStorageScanRows = kStorageThreads * kStorageScanPerThread;  // rows of a scan block

// a column image: group g's column of `rows` entries (1 byte, or 2 where gwide[g]) starts at
// byte col_off[g] of col
struct StorageColumns {
  const uint8_t* col;
  const int64_t* col_off;  // [num_groups]
  const int8_t* gwide;     // [num_groups]
  int32_t num_groups;
  int64_t rows;
};

// the learner's row layout (KArgs::word_g0 / word_wide / words_per_row / row_words / nibbles)
struct StorageRowLayout {
  const int32_t* word_g0;
  const int8_t* word_wide;
  int32_t words_per_row;
  int32_t row_words;
  int32_t nibbles;
};

// dst[i] = src[i] for n entries of src_bytes (1, 2 or 4) each, as 1 byte or (dst_wide) 2
void StorageConvertColumn(const void* src, int src_bytes, uint8_t* dst, int dst_wide, int64_t n, hipStream_t s);
// dst[rows[i] - row0] = vals[i] for k stored entries of val_bytes each; dst holds nrows entries
void StorageScatterSparse(const int32_t* rows, const void* vals, int val_bytes, int64_t k, int64_t row0, int64_t nrows,
                          uint8_t* dst, int dst_wide, hipStream_t s);
// out[r * row_words + w] for every row of the columns and every word of the row stride
void StoragePackRows(const StorageColumns& c, const StorageRowLayout& l, uint32_t* out, hipStream_t s);
// sp_ptr[0 .. rows] of the rows' non-zero cells: counts per row, sums per block of
// kStorageScanRows rows into block_sums[StorageScanBlocks(rows)], their scan, the add
int64_t StorageScanBlocks(int64_t rows);
void StorageStoredPointers(const StorageColumns& c, int64_t* sp_ptr, int64_t* block_sums, hipStream_t s);
// sp_bin[sp_ptr[r] ..) = group_off[g] + bin of row r's non-zero cells, ascending groups
void StorageFillStored(const StorageColumns& c, const int32_t* group_off, const int64_t* sp_ptr, uint16_t* sp_bin,
                       hipStream_t s);
// [tile_rows, slice_words, threads, scan_rows]
void StorageLaunchInfo(int64_t* out);

}  // namespace dev
}  // namespace lgbm_amd
