// The host side of a CSR / CSC pointer array (indptr, col_ptr), which the C API hands over as
// int32 or int64 behind a void*: reading it, checking it before anything is uploaded, calling
// typed code with it, and packing a set of columns for upload.  Header-only, no GPU.
#pragma once

#include <cstdint>
#include <vector>

namespace lgbm_amd {

struct SparsePtr {
  const void* p;
  bool is_64;  // int64 entries (else int32)
  int64_t operator[](int64_t i) const {
    return is_64 ? static_cast<const int64_t*>(p)[i] : static_cast<int64_t>(static_cast<const int32_t*>(p)[i]);
  }
};

// whether the n + 1 entries of ptr are a non-decreasing sequence inside [0, nelem]: what a device
// path asks before it copies rows or columns by their pointer entries (else the host takes the
// matrix)
inline bool PointerValid(SparsePtr ptr, int64_t n, int64_t nelem) {
  if (ptr[0] < 0 || ptr[n] > nelem) return false;
  for (int64_t i = 0; i < n; ++i) {
    if (ptr[i + 1] < ptr[i]) return false;
  }
  return true;
}

// fn(const P* ptr, const T* data) with P = int64_t or int32_t and T = double or float
template <typename Fn>
void DispatchSparse(bool is_64, bool is_double, const void* ptr, const void* data, Fn&& fn) {
  if (is_double) {
    if (is_64) fn(static_cast<const int64_t*>(ptr), static_cast<const double*>(data));
    else fn(static_cast<const int32_t*>(ptr), static_cast<const double*>(data));
  } else {
    if (is_64) fn(static_cast<const int64_t*>(ptr), static_cast<const float*>(data));
    else fn(static_cast<const int32_t*>(ptr), static_cast<const float*>(data));
  }
}

// `len` entries from `src` in the caller's arrays to `dst` in the packed ones
struct ColumnRun {
  int64_t src, dst, len;
};

// The stored entries of `columns` (ascending) of a matrix of ncol columns under a valid pointer
// (above), packed one column after the other: column columns[j] lands at [placed[j], placed[j + 1])
// (a column the matrix does not have is empty), and `runs` are the copies that put them there,
// adjacent columns -- empty ones between them or not -- as one.
inline void PackColumnRuns(const std::vector<int32_t>& columns, SparsePtr ptr, int64_t ncol,
                           std::vector<ColumnRun>* runs, std::vector<int64_t>* placed) {
  runs->clear();
  placed->assign(columns.size() + 1, 0);
  for (size_t j = 0; j < columns.size(); ++j) {
    const int64_t at = (*placed)[j];
    (*placed)[j + 1] = at;
    if (columns[j] >= ncol) continue;
    const int64_t a = ptr[columns[j]], b = ptr[columns[j] + 1];
    (*placed)[j + 1] = at + (b - a);
    if (b == a) continue;
    if (!runs->empty() && runs->back().src + runs->back().len == a) runs->back().len += b - a;
    else runs->push_back({a, at, b - a});
  }
}

}  // namespace lgbm_amd
