// CSC columns into the compact matrix the forest kernels read (src/device/csc_kernels.hip; see
// src/device/csr_slots.h for the matrix: one column per feature -- slot -- that the trees of a
// prediction window split on).  A CSC matrix is sorted by column already, so a slot's values are
// one contiguous run of stored entries.  The rule of a stored entry -- which rows of a chunk it
// belongs to, or none -- and the run of a slot are shared by the kernel and the host evaluator
// below (tests without a GPU: LGBM_AMD_CscToSlots).  Same meaning as the host's CSCToRows followed
// by Predictor::Fill: absent entries are 0, a stored zero and a stored NaN are values, columns the
// model does not have are ignored, and of several stored entries on one cell the last stored one
// wins.  An entry whose row index is outside the matrix is dropped.
#pragma once

#include <algorithm>
#include <cstdint>

// (a plain C++ program can include this header: tests/native/csc_slots_driver.cpp)
#include "stored_order.h"

namespace lgbm_amd {
namespace dev {

// the entries [*s, *e) of column `col` of the pointer (col < 0: the slot's feature is no column
// of the matrix, which has no entries), kept inside num_entries whatever col_ptr holds
template <typename Ptr>
LGBM_AMD_HD void CscColumnRange(Ptr col_ptr, int col, int64_t num_entries, int64_t* s, int64_t* e) {
  if (col < 0) {
    *s = *e = 0;
    return;
  }
  ClampedRange(col_ptr, col, 0, num_entries, s, e);
}

// the row of a stored entry inside the chunk of rows [row0, row0 + rows), or -1: another chunk's
// row, a negative index or one past the matrix (the caller's rows end at the matrix's last row)
LGBM_AMD_HD int64_t CscEntryRow(int32_t index, int64_t row0, int64_t rows) {
  const int64_t r = static_cast<int64_t>(index) - row0;
  return r >= 0 && r < rows ? r : -1;
}

// the kernel's result on the host, row-major (the kernel's matrix is column-major): `out`
// ([rows][num_slots]) zero-filled, then every kept entry written slot by slot in stored order
template <typename T, typename P>
void EvalCscToSlots(const P* col_ptr, const int32_t* slot_col, const int32_t* indices, const T* data,
                    int64_t num_entries, int64_t row0, int64_t rows, int num_slots, T* out) {
  std::fill(out, out + rows * num_slots, T(0));
  for (int slot = 0; slot < num_slots; ++slot) {
    int64_t s, e;
    CscColumnRange(col_ptr, slot_col[slot], num_entries, &s, &e);
    for (int64_t i = s; i < e; ++i) {
      const int64_t r = CscEntryRow(indices[i], row0, rows);
      if (r >= 0) out[r * num_slots + slot] = data[i];
    }
  }
}

}  // namespace dev
}  // namespace lgbm_amd
