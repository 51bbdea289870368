// CSR rows into the compact matrix of the forest kernels (src/device/csr_slots.h: the rule of
// one stored entry; src/boosting/device_predict.cpp: GBDT::PredictCSROnDevice).
//
// The matrix is column-major ([slot][row]): the forest walk, fifty times the work of this
// scatter, reads it four times as fast as a row-major one, because the lanes of a wave
// (neighbouring rows) read one slot from consecutive addresses.  It is zero-filled by a memset on
// the same stream; k_csr_to_slots then writes every stored entry whose column has a slot.
//
// One wave per row reads 64 consecutive entries at a time (coalesced; half the time of one
// thread per row at 40 entries per row).  Of a row's entries on one column the last stored one
// wins (the host predictor's Predictor::Fill), on every run: src/device/stored_order.h, LastOfKey
// on the slot and BatchFence.  (profiles/r08_device_sparse_predict.md has the layouts and
// mappings measured.)
#include "csr_slots.h"
#include "device_common.h"
#include "lgbm_amd/sparse_ptr.h"

namespace lgbm_amd {
namespace dev {

namespace {

constexpr int kCsrThreads = 256;
constexpr int kCsrRowsPerBlock = kCsrThreads / kWave;

template <typename T, typename P>
__global__ __launch_bounds__(kCsrThreads) void k_csr_to_slots(CsrSlotsArgs c) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = blockIdx.x * static_cast<int64_t>(kCsrRowsPerBlock) + (threadIdx.x >> 6);
  if (row >= c.num_rows) return;  // (the whole wave)
  int64_t s, e;
  ClampedRange(static_cast<const P*>(c.indptr), row, c.entry_base, c.num_entries, &s, &e);
  const T* data = static_cast<const T*>(c.data);
  T* out = static_cast<T*>(c.out);
  for (int64_t b = s; b < e; b += kWave) {
    const int64_t i = b + lane;
    int slot = -1;
    T v = T(0);
    if (i < e) {
      slot = CsrEntrySlot(c.slot_of, c.num_features, c.indices[i]);
      v = data[i];
    }
    if (LastOfKey(lane, slot)) out[static_cast<int64_t>(slot) * c.num_rows + row] = v;
    if (b + kWave < e) BatchFence();
  }
}

template <typename T, typename P>
void Launch(const CsrSlotsArgs& c, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>((c.num_rows + kCsrRowsPerBlock - 1) / kCsrRowsPerBlock));
  hipLaunchKernelGGL((k_csr_to_slots<T, P>), grid, dim3(kCsrThreads), 0, s, c);
}

}  // namespace

void CsrToSlots(const CsrSlotsArgs& c, hipStream_t s) {
  if (c.num_rows <= 0 || c.num_slots <= 0) return;
  const size_t bytes = static_cast<size_t>(c.num_rows) * c.num_slots * (c.is_double ? 8 : 4);
  (void)hipMemsetAsync(c.out, 0, bytes, s);
  if (c.num_entries <= 0) return;
  DispatchSparse(c.indptr_is_64 != 0, c.is_double != 0, c.indptr, c.data, [&](auto* ptr, auto* val) {
    Launch<std::decay_t<decltype(*val)>, std::decay_t<decltype(*ptr)>>(c, s);
  });
}

}  // namespace dev
}  // namespace lgbm_amd
