// The mechanism the sparse kernels share (csr_kernels.hip, csc_kernels.hip, csr_bin_kernels.hip,
// csc_bin_kernels.hip): the clamped range of a row or column, the rule that of several stored
// entries on one cell the last stored one wins, and the walk of a CSC column.  What an entry means
// is stated per path: csr_slots.h, csc_slots.h, csr_bins.h, csc_bins.h.  A plain C++ program can
// include this header (tests/native/*_driver.cpp); the device parts need hipcc.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include "device_common.h"
#define LGBM_AMD_HD __host__ __device__ __forceinline__
#else
#define LGBM_AMD_HD inline
#endif

namespace lgbm_amd {
namespace dev {

// A CSC column is cut into segments of kCscSegmentEntries stored entries, one wave each; the
// workgroups of a launch have kCscThreads threads and are about kCscGridBlocks, enough to fill the
// chip several times over, with at most kCscMaxGridY columns side by side in gridDim.y
constexpr int kCscThreads = 256;
constexpr int kCscSegmentEntries = 512;
constexpr int kCscGridBlocks = 8192;
constexpr int kCscMaxGridY = 65535;

// the entries [*s, *e) of row or column `i` of the pointer, relative to `base` (the entry that the
// arrays' element 0 holds), kept inside [0, num_entries] whatever ptr holds
template <typename Ptr>
LGBM_AMD_HD void ClampedRange(Ptr ptr, int64_t i, int64_t base, int64_t num_entries, int64_t* s, int64_t* e) {
  const int64_t a = static_cast<int64_t>(ptr[i]) - base;
  const int64_t b = static_cast<int64_t>(ptr[i + 1]) - base;
  *s = a < 0 ? 0 : (a > num_entries ? num_entries : a);
  *e = b < *s ? *s : (b > num_entries ? num_entries : b);
}

#if defined(__HIPCC__)

// A wave holds a batch of 64 consecutive stored entries, one per lane, and `key` names the cell of
// the lane's entry (the slot or group of a CSR row, the row index of a CSC column), or is negative:
// the lane has nothing to store.  True on exactly the highest lane of each distinct key that is
// not negative: lanes hold entries in stored order, so the highest lane of a key is its last
// stored entry, the one that wins on the host.  Every lane of the wave calls this (ballots).
__device__ __forceinline__ bool LastOfKey(int lane, int32_t key) {
  bool last = key >= 0;
  unsigned long long pending = __ballot(key >= 0);
  while (pending != 0ull) {
    const int32_t lead = ReadLane(key, __ffsll(pending) - 1);
    const unsigned long long same = __ballot(key == lead);
    if (key == lead && (same >> lane) > 1ull) last = false;
    pending &= ~same;
  }
  return last;
}

// Between two batches of one wave that may store to the same cell.  A workgroup fence makes the
// wave wait until its stores have been acknowledged (s_waitcnt vmcnt(0), which counts every lane's
// stores), so a later batch's store to a cell reaches memory after an earlier batch's; no other
// wave stores to the cell (one wave per CSR row, one wave per CSC column that is not ascending),
// so nothing wider than the workgroup has to be ordered.  Within a batch LastOfKey leaves one
// store per cell.  Together: the last stored entry wins on every run.
__device__ __forceinline__ void BatchFence() { __threadfence_block(); }

// The column-order pass of the threads with this blockIdx.x over the entries [s, e) of one
// column: *flag starts as all ones (non-zero: the row indices ascend strictly -- what scipy and
// torch build; no cell twice), and whoever finds a pair out of order clears it.
__device__ __forceinline__ void ClearUnlessAscending(const int32_t* indices, int64_t s, int64_t e, uint32_t* flag) {
  bool descends = false;
  for (int64_t i = s + blockIdx.x * static_cast<int64_t>(kCscThreads) + threadIdx.x; i + 1 < e;
       i += gridDim.x * static_cast<int64_t>(kCscThreads)) {
    descends |= indices[i] >= indices[i + 1];
  }
  if (descends) atomicAnd(flag, 0u);
}

// The walk of the entries [s, e) of one column by wave `wave` of the column's num_waves waves.
// entry(i, index) says whether the lane's entry i (row index `index`) is kept -- only one on a
// row of the matrix is, so never a negative index -- and does whatever else the path does per
// entry; store(i) writes a kept entry.
//   ascending: every segment belongs to one wave, whichever workgroup runs first -- wave w takes
//     segments w, w + num_waves, ... -- and every kept entry stores: no cell is stored twice, the
//     segments are independent.  skip(b, end) may drop the segment [b, end) unread.
//   otherwise: two segments could hold one cell, so wave 0 alone walks the column in stored order,
//     64 entries at a time, by LastOfKey on the row index and BatchFence.
// Either way no two waves store to one cell and the result does not depend on the dispatch order.
template <typename SkipSegment, typename Entry, typename Store>
__device__ __forceinline__ void WalkColumn(const int32_t* indices, int64_t s, int64_t e, bool ascending, int64_t wave,
                                           int64_t num_waves, int lane, SkipSegment skip, Entry entry, Store store) {
  if (ascending) {
    for (int64_t b = s + wave * kCscSegmentEntries; b < e; b += num_waves * kCscSegmentEntries) {
      const int64_t end = b + kCscSegmentEntries < e ? b + kCscSegmentEntries : e;
      if (skip(b, end)) continue;
      for (int64_t i = b + lane; i < end; i += kWave) {
        if (entry(i, indices[i])) store(i);
      }
    }
    return;
  }
  if (wave != 0) return;  // (the whole wave)
  for (int64_t b = s; b < e; b += kWave) {
    const int64_t i = b + lane;
    int32_t key = -1;  // the row index of a kept entry (a row of the matrix: not negative)
    if (i < e) {
      const int32_t index = indices[i];
      if (entry(i, index)) key = index;
    }
    if (LastOfKey(lane, key)) store(i);
    if (b + kWave < e) BatchFence();
  }
}

// the grid of a launch over num_items columns, the longest of `longest` entries: x covers the
// longest column at entries_per_block entries a workgroup, within about kCscGridBlocks in all
inline dim3 CscGrid(int64_t num_items, int64_t longest, int64_t entries_per_block) {
  const int64_t blocks = (longest + entries_per_block - 1) / entries_per_block;
  const int64_t cap = std::max<int64_t>(1, kCscGridBlocks / num_items);
  return dim3(static_cast<unsigned>(std::max<int64_t>(1, std::min(blocks, cap))),
              static_cast<unsigned>(std::min<int64_t>(num_items, kCscMaxGridY)));
}

#endif  // __HIPCC__

}  // namespace dev
}  // namespace lgbm_amd
