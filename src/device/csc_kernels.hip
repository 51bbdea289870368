// CSC columns into the compact matrix of the forest kernels (src/device/csc_slots.h: the rule of
// one stored entry; src/boosting/device_predict.cpp: GBDT::PredictCSCOnDevice).
//
// The matrix is the one k_csr_to_slots fills (src/device/csr_kernels.hip): column-major
// ([slot][row], column stride = the chunk's rows), zero-filled by a memset on the same stream.  A
// slot's values are the stored entries of one column of the CSC matrix, a contiguous run, so the
// lanes of a wave read consecutive entries (coalesced) and store into one column of the matrix.
//
// A column is cut into segments of kCscSegmentEntries entries and every segment belongs to one
// wave, whichever workgroup runs first: wave w of the column's 4 * gridDim.x waves takes the
// segments w, w + waves, ...  Two segments may hold the same cell only when the column stores a
// row twice, and then the last stored entry has to win on every run.  k_csc_column_order
// therefore writes one flag per slot in front: the column's row indices ascend strictly (what
// scipy and torch build; no cell twice, the segments are independent).  A column without the
// flag is walked by one wave alone in stored order, 64 entries at a time: within a batch the
// lanes on one row are found with ballots and only the highest stores, and between batches the
// wave waits for its stores (s_waitcnt vmcnt(0), as k_csr_to_slots does).  So no two waves ever
// store to one cell, and the result does not depend on the dispatch order.  The flag is read on
// the device: no host synchronisation between the launches.
//
// An entry whose row is outside the chunk [row0, row0 + num_rows) -- another chunk's, negative,
// past the matrix -- is dropped; of an ascending column a wave skips the segments that lie
// before or after the chunk by their first and last index.
#include "device_common.h"  // (first: the HIP runtime's function attributes, which csc_slots.h uses)

#include "csc_slots.h"

namespace lgbm_amd {
namespace dev {

namespace {

constexpr int kCscWaves = kCscThreads / kWave;
constexpr int kCscMaxGridY = 65535;
// workgroups of a launch, about: enough to fill the chip several times over
constexpr int kCscGridBlocks = 8192;

template <typename P>
__global__ __launch_bounds__(kCscThreads) void k_csc_column_order(CscSlotsArgs c) {
  for (int slot = blockIdx.y; slot < c.num_slots; slot += gridDim.y) {
    int64_t s, e;
    CscColumnRange(static_cast<const P*>(c.col_ptr), c.slot_col[slot], c.num_entries, &s, &e);
    bool descends = false;
    for (int64_t i = s + blockIdx.x * static_cast<int64_t>(kCscThreads) + threadIdx.x; i + 1 < e;
         i += gridDim.x * static_cast<int64_t>(kCscThreads)) {
      descends |= c.indices[i] >= c.indices[i + 1];
    }
    // (the flag starts as all ones; whoever finds a pair out of order clears it)
    if (descends) atomicAnd(&c.ascending[slot], 0u);
  }
}

template <typename T, typename P>
__global__ __launch_bounds__(kCscThreads) void k_csc_to_slots(CscSlotsArgs c) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = blockIdx.x * static_cast<int64_t>(kCscWaves) + (threadIdx.x >> 6);
  const int64_t stride = gridDim.x * static_cast<int64_t>(kCscWaves) * kCscSegmentEntries;
  const T* data = static_cast<const T*>(c.data);
  for (int slot = blockIdx.y; slot < c.num_slots; slot += gridDim.y) {
    int64_t s, e;
    CscColumnRange(static_cast<const P*>(c.col_ptr), c.slot_col[slot], c.num_entries, &s, &e);
    T* out = static_cast<T*>(c.out) + static_cast<int64_t>(slot) * c.num_rows;
    if (c.ascending[slot] != 0u) {
      for (int64_t b = s + wave * kCscSegmentEntries; b < e; b += stride) {
        const int64_t end = b + kCscSegmentEntries < e ? b + kCscSegmentEntries : e;
        // (ascending: a segment that ends before the chunk or starts after it holds none of its rows)
        if (c.indices[end - 1] < c.row0 || c.indices[b] >= c.row0 + c.num_rows) continue;
        for (int64_t i = b + lane; i < end; i += kWave) {
          const int64_t r = CscEntryRow(c.indices[i], c.row0, c.num_rows);
          if (r >= 0) out[r] = data[i];
        }
      }
      continue;
    }
    if (wave != 0) continue;  // (the whole wave)
    for (int64_t b = s; b < e; b += kWave) {
      const int64_t i = b + lane;
      int32_t index = 0;
      int64_t r = -1;
      T v = T(0);
      if (i < e) {
        index = c.indices[i];
        r = CscEntryRow(index, c.row0, c.num_rows);
        v = data[i];
      }
      // of the batch's lanes on one row only the highest (the last stored entry) writes
      const bool kept = r >= 0;
      bool write = kept;
      unsigned long long pending = __ballot(kept);
      while (pending != 0ull) {
        const int32_t lead = ReadLane(index, __ffsll(pending) - 1);
        const unsigned long long same = __ballot(kept && index == lead);
        if (kept && index == lead && (same >> lane) > 1ull) write = false;
        pending &= ~same;
      }
      if (write) out[r] = v;
      // (this batch's stores are done before the next batch's are issued)
      if (b + kWave < e) __threadfence_block();
    }
  }
}

dim3 Grid(const CscSlotsArgs& c, int64_t entries_per_block) {
  const int64_t blocks = (c.num_entries + entries_per_block - 1) / entries_per_block;
  const int64_t cap = std::max<int64_t>(1, kCscGridBlocks / c.num_slots);
  return dim3(static_cast<unsigned>(std::max<int64_t>(1, std::min(blocks, cap))),
              static_cast<unsigned>(std::min(c.num_slots, kCscMaxGridY)));
}

template <typename T, typename P>
void Launch(const CscSlotsArgs& c, hipStream_t s) {
  hipLaunchKernelGGL((k_csc_to_slots<T, P>), Grid(c, static_cast<int64_t>(kCscWaves) * kCscSegmentEntries),
                     dim3(kCscThreads), 0, s, c);
}

}  // namespace

void CscColumnOrder(const CscSlotsArgs& c, hipStream_t s) {
  if (c.num_slots <= 0) return;
  (void)hipMemsetAsync(c.ascending, 0xff, static_cast<size_t>(c.num_slots) * sizeof(uint32_t), s);
  if (c.num_entries <= 1) return;
  const dim3 grid = Grid(c, kCscThreads);
  if (c.col_ptr_is_64) hipLaunchKernelGGL((k_csc_column_order<int64_t>), grid, dim3(kCscThreads), 0, s, c);
  else hipLaunchKernelGGL((k_csc_column_order<int32_t>), grid, dim3(kCscThreads), 0, s, c);
}

void CscToSlots(const CscSlotsArgs& c, hipStream_t s) {
  if (c.num_rows <= 0 || c.num_slots <= 0) return;
  const size_t bytes = static_cast<size_t>(c.num_rows) * c.num_slots * (c.is_double ? 8 : 4);
  (void)hipMemsetAsync(c.out, 0, bytes, s);
  if (c.num_entries <= 0) return;
  if (c.is_double) {
    if (c.col_ptr_is_64) Launch<double, int64_t>(c, s);
    else Launch<double, int32_t>(c, s);
  } else {
    if (c.col_ptr_is_64) Launch<float, int64_t>(c, s);
    else Launch<float, int32_t>(c, s);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
