// The device learner's training storage, built on the device from a Dataset's group columns
// (GPUTreeLearner::BuildDeviceStorage): the column image -- each group's column uploaded once, at
// the width the image wants or converted / scattered here --, the row words packed from it, and
// the row-sparse lists counted, scanned and filled from it.  No kernel here waits on another
// workgroup; every row x stride offset is 64-bit.
#include "device_common.h"
#include "storage_build.h"

namespace lgbm_amd {
namespace dev {

namespace {

// a 16-bit column may start at an odd byte of the image (an odd row count of 8-bit columns
// before it): its entries are read and written as two bytes
__device__ __forceinline__ uint32_t ColumnBin(const uint8_t* col, int wide, int64_t r) {
  if (!wide) return col[r];
  const uint8_t* p = col + 2 * r;
  return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8);
}

__device__ __forceinline__ void ColumnStore(uint8_t* col, int wide, int64_t r, uint32_t v) {
  if (!wide) {
    col[r] = static_cast<uint8_t>(v);
    return;
  }
  col[2 * r] = static_cast<uint8_t>(v);
  col[2 * r + 1] = static_cast<uint8_t>(v >> 8);
}

__device__ __forceinline__ uint32_t StagedValue(const void* src, int bytes, int64_t i) {
  if (bytes == 1) return static_cast<const uint8_t*>(src)[i];
  if (bytes == 2) return static_cast<const uint16_t*>(src)[i];
  return static_cast<const uint32_t*>(src)[i];
}

// exclusive scan of one value per thread of a kStorageThreads workgroup; *total: their sum
__device__ __forceinline__ int64_t BlockExclusiveScan(int64_t v, int64_t* sh, int64_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < kStorageThreads; off <<= 1) {
    const int64_t x = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const int64_t incl = sh[t];
  *total = sh[kStorageThreads - 1];
  __syncthreads();
  return incl - v;
}

}  // namespace

// ---------------------------------------------------------------- stage 1: the column image
__global__ __launch_bounds__(kStorageThreads) void k_storage_convert_column(const void* src, int src_bytes, uint8_t* dst,
                                                                            int dst_wide, int64_t n) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kStorageThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kStorageThreads + threadIdx.x; i < n; i += step) {
    ColumnStore(dst, dst_wide, i, StagedValue(src, src_bytes, i));
  }
}

// a host-sparse group's stored rows into its zeroed column (FeatureGroup::ForEachStored on the
// host): stored rows are distinct, so no two threads write one entry
__global__ __launch_bounds__(kStorageThreads) void k_storage_scatter_sparse(const int32_t* rows, const void* vals,
                                                                            int val_bytes, int64_t k, int64_t row0,
                                                                            int64_t nrows, uint8_t* dst, int dst_wide) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kStorageThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kStorageThreads + threadIdx.x; i < k; i += step) {
    const int64_t r = static_cast<int64_t>(rows[i]) - row0;
    if (r >= 0 && r < nrows) ColumnStore(dst, dst_wide, r, StagedValue(vals, val_bytes, i));
  }
}

// ---------------------------------------------------------------- stage 2a: row words
// A workgroup turns a tile of kStorageTileRows rows x a slice of up to kStorageSliceWords words.
//
// Reading: thread t owns row t of the tile and walks the slice's words; for a word it reads the
// word's groups (4, 2 or 8 of them) at its row.  The word index is uniform over the workgroup,
// so the group table is read through scalar loads, and the 64 lanes of a wave read 64 (or 128)
// consecutive bytes of one column: coalesced along the column.
// The turn: the bytes never meet in LDS.  A thread composes the whole 32-bit word in a register
// (shift by 8, 16 or 4 bits per slot, little-endian as the host writes them), so two nibbles of
// one byte, or four bytes of one word, are never written by different threads, and LDS sees
// 32-bit stores only.  Thread t stores word wl at tile[t * stride + wl] with stride = words | 1:
// an odd stride sends the lanes of a wave to distinct banks.
// Writing: the tile is read back in row-major order (consecutive threads take consecutive words
// of a row, then the next row; the stride's one pad word shifts a row by one bank, at most a
// two-way conflict where a wave crosses rows) and stored at r * row_words + w: with a slice as
// wide as the row stride the tile is one contiguous run of global memory, otherwise 128-B runs.
// One thread per row x 32 words keeps the tile at 256 x 33 x 4 = 33 KiB, four workgroups per CU
// of 160 KiB; a wider row takes more slices (blockIdx.y), never more LDS.  Padding words (from
// words_per_row to row_words, the (g, h) words of LGBM_AMD_GH_IN_ROWS included) are written as
// zero, so the image is written exactly once and needs no memset.
__global__ __launch_bounds__(kStorageThreads) void k_storage_pack_rows(StorageColumns c, StorageRowLayout l, uint32_t* out) {
  __shared__ uint32_t tile[kStorageTileRows * (kStorageSliceWords + 1)];
  static_assert(kStorageTileRows == kStorageThreads, "one tile row per thread");
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kStorageTileRows;
  const int w0 = blockIdx.y * kStorageSliceWords;
  const int nw = min(kStorageSliceWords, l.row_words - w0);
  const int stride = nw | 1;
  const int64_t r = r0 + threadIdx.x;
  const bool live = r < c.rows;
  for (int wl = 0; wl < nw; ++wl) {
    const int w = w0 + wl;
    uint32_t word = 0;
    if (live && w < l.words_per_row) {
      const int g0 = l.word_g0[w], g1 = min(l.word_g0[w + 1], c.num_groups);
      const int wide = l.word_wide[w];
      const int bits = l.nibbles ? 4 : (wide ? 16 : 8);
      const uint32_t mask = l.nibbles ? 15u : 0xffffu;
      for (int g = g0; g < g1; ++g) {
        word |= (ColumnBin(c.col + c.col_off[g], wide, r) & mask) << (bits * (g - g0));
      }
    }
    tile[threadIdx.x * stride + wl] = word;
  }
  __syncthreads();
  const int rows_here = static_cast<int>(min(static_cast<int64_t>(kStorageTileRows), c.rows - r0));
  const int total = rows_here * nw;
  uint32_t* dst = out + r0 * l.row_words + w0;
  for (int i = threadIdx.x; i < total; i += kStorageThreads) {
    const int rr = i / nw, ww = i - rr * nw;
    dst[static_cast<int64_t>(rr) * l.row_words + ww] = tile[rr * stride + ww];
  }
}

// ---------------------------------------------------------------- stage 2b: row-sparse lists
// counts of a block of kStorageScanRows rows into sp_ptr[r + 1] and their sum into block_sums
__global__ __launch_bounds__(kStorageThreads) void k_storage_count_stored(StorageColumns c, int64_t* sp_ptr,
                                                                          int64_t* block_sums) {
  __shared__ int64_t sh[kStorageThreads];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kStorageScanRows;
  int cnt[kStorageScanPerThread] = {};
  for (int g = 0; g < c.num_groups; ++g) {
    const uint8_t* col = c.col + c.col_off[g];
    const int wide = c.gwide[g];
#pragma unroll
    for (int j = 0; j < kStorageScanPerThread; ++j) {
      const int64_t r = base + j * kStorageThreads + threadIdx.x;  // (a wave reads along the column)
      if (r < c.rows) cnt[j] += ColumnBin(col, wide, r) != 0 ? 1 : 0;
    }
  }
  int64_t mine = 0;
#pragma unroll
  for (int j = 0; j < kStorageScanPerThread; ++j) {
    const int64_t r = base + j * kStorageThreads + threadIdx.x;
    if (r < c.rows) sp_ptr[r + 1] = cnt[j];
    mine += cnt[j];
  }
  int64_t total = 0;
  (void)BlockExclusiveScan(mine, sh, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// exclusive scan of the block sums in place: one workgroup walks them with a running carry
__global__ __launch_bounds__(kStorageThreads) void k_storage_scan_sums(int64_t* block_sums, int64_t nblocks) {
  __shared__ int64_t sh[kStorageThreads];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nblocks; b0 += kStorageThreads) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < nblocks ? block_sums[b] : 0;
    int64_t total = 0;
    const int64_t excl = BlockExclusiveScan(v, sh, &total);
    if (b < nblocks) block_sums[b] = carry + excl;
    carry += total;
  }
}

// the counts of a block into pointers: an inclusive scan of sp_ptr[r + 1] over the block's rows
// (each thread its kStorageScanPerThread consecutive rows) plus the block's offset
__global__ __launch_bounds__(kStorageThreads) void k_storage_scan_add(int64_t rows, int64_t* sp_ptr,
                                                                      const int64_t* block_sums) {
  __shared__ int64_t sh[kStorageThreads];
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kStorageScanRows + threadIdx.x * kStorageScanPerThread;
  int64_t v[kStorageScanPerThread];
  int64_t mine = 0;
#pragma unroll
  for (int j = 0; j < kStorageScanPerThread; ++j) {
    v[j] = first + j < rows ? sp_ptr[first + j + 1] : 0;
    mine += v[j];
  }
  int64_t total = 0;
  int64_t run = block_sums[blockIdx.x] + BlockExclusiveScan(mine, sh, &total);
#pragma unroll
  for (int j = 0; j < kStorageScanPerThread; ++j) {
    run += v[j];
    if (first + j < rows) sp_ptr[first + j + 1] = run;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) sp_ptr[0] = 0;
}

__global__ __launch_bounds__(kStorageThreads) void k_storage_fill_stored(StorageColumns c, const int32_t* group_off,
                                                                         const int64_t* sp_ptr, uint16_t* sp_bin) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kStorageThreads;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kStorageThreads + threadIdx.x; r < c.rows; r += step) {
    int64_t pos = sp_ptr[r];
    const int64_t end = sp_ptr[r + 1];
    for (int g = 0; g < c.num_groups && pos < end; ++g) {
      const uint32_t v = ColumnBin(c.col + c.col_off[g], c.gwide[g], r);
      if (v != 0) sp_bin[pos++] = static_cast<uint16_t>(static_cast<uint32_t>(group_off[g]) + v);
    }
  }
}

// ---------------------------------------------------------------- launchers
void StorageConvertColumn(const void* src, int src_bytes, uint8_t* dst, int dst_wide, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_storage_convert_column, dim3(GridFor(n)), dim3(kStorageThreads), 0, s, src, src_bytes, dst,
                     dst_wide, n);
}

void StorageScatterSparse(const int32_t* rows, const void* vals, int val_bytes, int64_t k, int64_t row0, int64_t nrows,
                          uint8_t* dst, int dst_wide, hipStream_t s) {
  if (k <= 0 || nrows <= 0) return;
  hipLaunchKernelGGL(k_storage_scatter_sparse, dim3(GridFor(k)), dim3(kStorageThreads), 0, s, rows, vals, val_bytes, k,
                     row0, nrows, dst, dst_wide);
}

void StoragePackRows(const StorageColumns& c, const StorageRowLayout& l, uint32_t* out, hipStream_t s) {
  if (c.rows <= 0 || l.row_words <= 0) return;
  const dim3 grid(static_cast<unsigned>((c.rows + kStorageTileRows - 1) / kStorageTileRows),
                  static_cast<unsigned>((l.row_words + kStorageSliceWords - 1) / kStorageSliceWords));
  hipLaunchKernelGGL(k_storage_pack_rows, grid, dim3(kStorageThreads), 0, s, c, l, out);
}

int64_t StorageScanBlocks(int64_t rows) { return std::max<int64_t>(1, (rows + kStorageScanRows - 1) / kStorageScanRows); }

void StorageStoredPointers(const StorageColumns& c, int64_t* sp_ptr, int64_t* block_sums, hipStream_t s) {
  const int64_t nblocks = StorageScanBlocks(c.rows);
  const dim3 grid(static_cast<unsigned>(nblocks));
  hipLaunchKernelGGL(k_storage_count_stored, grid, dim3(kStorageThreads), 0, s, c, sp_ptr, block_sums);
  hipLaunchKernelGGL(k_storage_scan_sums, dim3(1), dim3(kStorageThreads), 0, s, block_sums, nblocks);
  hipLaunchKernelGGL(k_storage_scan_add, grid, dim3(kStorageThreads), 0, s, c.rows, sp_ptr, block_sums);
}

void StorageFillStored(const StorageColumns& c, const int32_t* group_off, const int64_t* sp_ptr, uint16_t* sp_bin,
                       hipStream_t s) {
  if (c.rows <= 0) return;
  hipLaunchKernelGGL(k_storage_fill_stored, dim3(GridFor(c.rows)), dim3(kStorageThreads), 0, s, c, group_off, sp_ptr,
                     sp_bin);
}

void StorageLaunchInfo(int64_t* out) {
  out[0] = kStorageTileRows;
  out[1] = kStorageSliceWords;
  out[2] = kStorageThreads;
  out[3] = kStorageScanRows;
}

}  // namespace dev
}  // namespace lgbm_amd
