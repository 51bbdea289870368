// CSR rows into the compact matrix the forest kernels read (src/device/csr_kernels.hip): the
// trees of a prediction window split on a set U of distinct features, usually far fewer than the
// matrix has columns; feature u of the sorted list used[] has slot u, and the compact matrix
// holds one column per slot.  The rule of one stored entry -- which slot it goes to, or none --
// and the address of a cell are shared by the kernel and the host evaluator below (tests without
// a GPU: LGBM_AMD_CsrToSlots).  Same semantics as the host predictor's Predictor::Fill: absent
// entries are 0, columns the model does not have are ignored, and of several stored entries on
// one column of a row the last one wins.
#pragma once

#include <algorithm>
#include <cstdint>

#include "stored_order.h"

namespace lgbm_amd {
namespace dev {

// the slot of a stored entry on column `col`, or -1: not a feature of the model, or one that no
// tree of the window splits on
LGBM_AMD_HD int CsrEntrySlot(const int32_t* slot_of, int num_features, int col) {
  return col >= 0 && col < num_features ? slot_of[col] : -1;
}

// the kernel's result on the host, row-major (the kernel's matrix is column-major): `out`
// ([rows][num_slots]) zero-filled, then every stored entry with a slot written in stored order; a
// row's entries are relative to the chunk's first entry and clamped to its num_entries
template <typename T, typename P>
void EvalCsrToSlots(const P* indptr, int64_t entry_base, const int32_t* indices, const T* data, int64_t rows,
                    int64_t num_entries, const int32_t* slot_of, int num_features, int num_slots, T* out) {
  std::fill(out, out + rows * num_slots, T(0));
  for (int64_t r = 0; r < rows; ++r) {
    int64_t s, e;
    ClampedRange(indptr, r, entry_base, num_entries, &s, &e);
    for (int64_t i = s; i < e; ++i) {
      const int slot = CsrEntrySlot(slot_of, num_features, indices[i]);
      if (slot >= 0) out[r * num_slots + slot] = data[i];
    }
  }
}

}  // namespace dev
}  // namespace lgbm_amd
