// CSC columns into the compact matrix of the forest kernels (src/device/csc_slots.h: the rule of
// one stored entry; src/boosting/device_predict.cpp: GBDT::PredictCSCOnDevice).
//
// The matrix is the one k_csr_to_slots fills (src/device/csr_kernels.hip): column-major
// ([slot][row], column stride = the chunk's rows), zero-filled by a memset on the same stream.  A
// slot's values are the stored entries of one column of the CSC matrix, a contiguous run, so the
// lanes of a wave read consecutive entries (coalesced) and store into one column of the matrix.
//
// A column is walked as src/device/stored_order.h says (WalkColumn): in segments shared among
// the column's 4 * gridDim.x waves when k_csc_column_order, in front, found its row indices
// ascending, else by one wave in stored order, so that of a cell stored twice the last stored
// entry wins on every run.  The flag is read on the device: no host synchronisation between the
// launches.
//
// An entry whose row is outside the chunk [row0, row0 + num_rows) -- another chunk's, negative,
// past the matrix -- is dropped; of an ascending column a wave skips the segments that lie
// before or after the chunk by their first and last index.
#include "device_common.h"  // (first: the HIP runtime's function attributes, which csc_slots.h uses)

#include "csc_slots.h"
#include "lgbm_amd/sparse_ptr.h"

namespace lgbm_amd {
namespace dev {

namespace {

constexpr int kCscWaves = kCscThreads / kWave;

template <typename P>
__global__ __launch_bounds__(kCscThreads) void k_csc_column_order(CscSlotsArgs c) {
  for (int slot = blockIdx.y; slot < c.num_slots; slot += gridDim.y) {
    int64_t s, e;
    CscColumnRange(static_cast<const P*>(c.col_ptr), c.slot_col[slot], c.num_entries, &s, &e);
    ClearUnlessAscending(c.indices, s, e, &c.ascending[slot]);
  }
}

template <typename T, typename P>
__global__ __launch_bounds__(kCscThreads) void k_csc_to_slots(CscSlotsArgs c) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = blockIdx.x * static_cast<int64_t>(kCscWaves) + (threadIdx.x >> 6);
  const int64_t num_waves = gridDim.x * static_cast<int64_t>(kCscWaves);
  const T* data = static_cast<const T*>(c.data);
  for (int slot = blockIdx.y; slot < c.num_slots; slot += gridDim.y) {
    int64_t s, e;
    CscColumnRange(static_cast<const P*>(c.col_ptr), c.slot_col[slot], c.num_entries, &s, &e);
    T* out = static_cast<T*>(c.out) + static_cast<int64_t>(slot) * c.num_rows;
    int64_t r = -1;
    T v = T(0);
    WalkColumn(
        c.indices, s, e, c.ascending[slot] != 0u, wave, num_waves, lane,
        // (ascending: a segment that ends before the chunk or starts after it holds none of its rows)
        [&](int64_t b, int64_t end) { return c.indices[end - 1] < c.row0 || c.indices[b] >= c.row0 + c.num_rows; },
        [&](int64_t i, int32_t index) {
          r = CscEntryRow(index, c.row0, c.num_rows);
          if (r >= 0) v = data[i];
          return r >= 0;
        },
        [&](int64_t) { out[r] = v; });
  }
}

template <typename T, typename P>
void Launch(const CscSlotsArgs& c, hipStream_t s) {
  const dim3 grid = CscGrid(c.num_slots, c.num_entries, static_cast<int64_t>(kCscWaves) * kCscSegmentEntries);
  hipLaunchKernelGGL((k_csc_to_slots<T, P>), grid, dim3(kCscThreads), 0, s, c);
}

}  // namespace

void CscColumnOrder(const CscSlotsArgs& c, hipStream_t s) {
  if (c.num_slots <= 0) return;
  (void)hipMemsetAsync(c.ascending, 0xff, static_cast<size_t>(c.num_slots) * sizeof(uint32_t), s);
  if (c.num_entries <= 1) return;
  const dim3 grid = CscGrid(c.num_slots, c.num_entries, kCscThreads);
  if (c.col_ptr_is_64) hipLaunchKernelGGL((k_csc_column_order<int64_t>), grid, dim3(kCscThreads), 0, s, c);
  else hipLaunchKernelGGL((k_csc_column_order<int32_t>), grid, dim3(kCscThreads), 0, s, c);
}

void CscToSlots(const CscSlotsArgs& c, hipStream_t s) {
  if (c.num_rows <= 0 || c.num_slots <= 0) return;
  const size_t bytes = static_cast<size_t>(c.num_rows) * c.num_slots * (c.is_double ? 8 : 4);
  (void)hipMemsetAsync(c.out, 0, bytes, s);
  if (c.num_entries <= 0) return;
  DispatchSparse(c.col_ptr_is_64 != 0, c.is_double != 0, c.col_ptr, c.data, [&](auto* ptr, auto* val) {
    Launch<std::decay_t<decltype(*val)>, std::decay_t<decltype(*ptr)>>(c, s);
  });
}

}  // namespace dev
}  // namespace lgbm_amd
