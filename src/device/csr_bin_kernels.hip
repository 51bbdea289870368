// Feature binning of CSR matrices on the device (src/device/csr_bins.h: the rule of one row;
// reference Dataset::PushOneRow over a sparse row + FeatureGroup::PushData).
//
//   k_csr_to_group_bins  one wave per row, 64 consecutive stored entries per batch (coalesced):
//                        column -> feature (an int32 table over num_total_features), the value's
//                        bin by binary search over the upper bounds in global memory (they do
//                        not fit LDS for wide inputs), the group cell.  The rows of a chunk go
//                        into a zero-filled scratch of one column per group ([group][row], the
//                        group's bin_bytes per cell).  The last stored write to a cell wins on
//                        every run: src/device/stored_order.h, LastOfKey on the group and
//                        BatchFence.  The features whose zeros are pushed (default bin != most
//                        frequent bin) are flagged in a per-wave LDS bitset by the entries that
//                        name them; after the entries the unflagged ones write the bin of 0.0,
//                        64 per batch by the same store rule.
// The compaction of sparse groups (k_count_stored / k_scan_counts / k_write_stored), the dense
// groups' column copy-back and the host tables are shared with the CSC path:
// src/device/group_bin_scratch.h.  Rows stream through in chunks whose entries and scratch each
// stay under about 256 MiB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csr_bins.h"
#include "device_common.h"
#include "group_bin_scratch.h"
#include "lgbm_amd/c_api.h"
#include "lgbm_amd/dataset.h"
#include "lgbm_amd/device_binning.h"
#include "lgbm_amd/log.h"
#include "lgbm_amd/sparse_ptr.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {

namespace {

#define CSRBINCHECK(x) GROUPBINCHECK(x)

constexpr int kCsrBinThreads = 256;
constexpr int kCsrBinRowsPerBlock = kCsrBinThreads / kWave;

struct CsrBinArgs {
  CsrBinTables t;
  const CsrBinGroup* groups;
  const void* indptr;  // the chunk's num_rows + 1 pointers
  int64_t entry_base;  // the entry indices[0] / data[0] hold
  const int32_t* indices;
  const void* data;
  int64_t num_rows;
  int64_t num_entries;
  uint8_t* scratch;
};

// one batch of a wave's writes to the cells of `row` (group < 0: the lane writes nothing)
__device__ __forceinline__ void StoreBatch(const CsrBinArgs& c, int64_t row, int lane, int group, uint32_t cell) {
  if (dev::LastOfKey(lane, group)) StoreCell(c.scratch, c.groups[group], row, cell);
}

template <typename T, typename P>
__global__ __launch_bounds__(kCsrBinThreads) void k_csr_to_group_bins(CsrBinArgs c) {
  __shared__ uint32_t s_named[kCsrBinRowsPerBlock][kMaxPushZeroFeatures / 32];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = blockIdx.x * static_cast<int64_t>(kCsrBinRowsPerBlock) + (threadIdx.x >> 6);
  if (row >= c.num_rows) return;  // (the whole wave; no workgroup barrier below)
  uint32_t* named = s_named[threadIdx.x >> 6];
  const int npz = c.t.num_push_zero;
  if (npz > 0) {
    for (int j = lane; j < (npz + 31) / 32; j += kWave) named[j] = 0u;
    __threadfence_block();  // (the wave's LDS writes are done before its flags are set)
  }
  int64_t s, e;
  dev::ClampedRange(static_cast<const P*>(c.indptr), row, c.entry_base, c.num_entries, &s, &e);
  const T* data = static_cast<const T*>(c.data);
  for (int64_t b = s; b < e; b += kWave) {
    const int64_t i = b + lane;
    int group = -1;
    uint32_t cell = 0u;
    if (i < e) {
      const int f = dev::CsrEntryBinFeat(c.t, c.indices[i]);
      if (f >= 0) {
        const CsrBinFeat F = c.t.feats[f];
        if (F.pz >= 0) atomicOr(&named[F.pz >> 5], 1u << (F.pz & 31));
        if (!dev::CsrFeatWrite(c.t, F, static_cast<double>(data[i]), &group, &cell)) group = -1;
      }
    }
    StoreBatch(c, row, lane, group, cell);
    // (before the next batch stores -- and before the zeros read this batch's flags)
    if (b + kWave < e || npz > 0) dev::BatchFence();
  }
  for (int k0 = 0; k0 < npz; k0 += kWave) {
    const int k = k0 + lane;
    int group = -1;
    uint32_t cell = 0u;
    if (k < npz && ((named[k >> 5] >> (k & 31)) & 1u) == 0u) {
      const CsrBinFeat F = c.t.feats[c.t.push_zero[k]];
      if (!dev::CsrFeatWrite(c.t, F, 0.0, &group, &cell)) group = -1;
    }
    StoreBatch(c, row, lane, group, cell);
    if (k0 + kWave < npz) dev::BatchFence();
  }
}

// ---- host side

void LaunchCsrToGroupBins(const CsrBinArgs& c, bool is_f64, bool indptr_64) {
  const dim3 grid(static_cast<unsigned>((c.num_rows + kCsrBinRowsPerBlock - 1) / kCsrBinRowsPerBlock));
  const dim3 block(kCsrBinThreads);
  DispatchSparse(indptr_64, is_f64, c.indptr, c.data, [&](auto* ptr, auto* val) {
    hipLaunchKernelGGL((k_csr_to_group_bins<std::decay_t<decltype(*val)>, std::decay_t<decltype(*ptr)>>), grid, block, 0,
                       0, c);
  });
  CSRBINCHECK(hipGetLastError());
}

}  // namespace

void CsrBinLaunchInfo(int64_t* out) {
  out[0] = kWave;
  out[1] = kCsrBinRowsPerBlock;
  out[2] = kTileRows;
  out[3] = kMaxPushZeroFeatures;
}

void EvalCsrGroupBins(const Dataset& ds, const void* indptr, int indptr_type, const int32_t* indices,
                      const void* data, int data_type, int64_t nrow, int64_t nelem, int32_t* bins) {
  CheckTypes(indptr_type, data_type);
  const HostTables h(ds);
  const CsrBinTables t = h.View();
  const int ng = ds.num_groups();
  constexpr int64_t kRows = 4096;
  std::vector<int32_t> part(static_cast<size_t>(kRows) * std::max(1, t.num_groups));
  for (int64_t r0 = 0; r0 < nrow; r0 += kRows) {
    const int64_t rows = std::min(kRows, nrow - r0);
    DispatchSparse(indptr_type == C_API_DTYPE_INT64, data_type == C_API_DTYPE_FLOAT64, indptr, data,
                   [&](auto* ptr, auto* val) {
                     dev::EvalCsrToGroupBins(ptr + r0, 0, indices, val, rows, nelem, t, part.data());
                   });
    for (int64_t r = 0; r < rows; ++r) {
      for (int g = 0; g < ng; ++g) {
        bins[(r0 + r) * ng + g] = h.col_of[g] < 0 ? -1 : part[r * t.num_groups + h.col_of[g]];
      }
    }
  }
}

void CsrGroupBinsOnDevice(const Dataset& ds, const void* d_indptr, int indptr_type, const int32_t* d_indices,
                          const void* d_data, int data_type, int64_t nrow, int64_t nelem, int32_t* d_bins) {
  CheckTypes(indptr_type, data_type);
  if (nrow <= 0 || ds.num_groups() <= 0) return;
  const HostTables h(ds);
  if (static_cast<int>(h.push_zero.size()) > kMaxPushZeroFeatures) {
    Log::Fatal("csr group bins: %d features need their zeros pushed, the kernel takes %d",
               static_cast<int>(h.push_zero.size()), kMaxPushZeroFeatures);
  }
  DeviceScope sc;
  std::vector<CsrBinGroup> groups;
  const int64_t bytes = PlaceColumns(ds, h, nrow, &groups);
  CsrBinArgs c;
  c.t = UploadTables(h, &sc);
  c.groups = sc.Upload(groups);
  c.indptr = d_indptr;
  c.entry_base = 0;
  c.indices = d_indices;
  c.data = d_data;
  c.num_rows = nrow;
  c.num_entries = nelem;
  c.scratch = sc.Alloc<uint8_t>(static_cast<size_t>(bytes));
  CSRBINCHECK(hipMemsetAsync(c.scratch, 0, static_cast<size_t>(std::max<int64_t>(1, bytes)), 0));
  if (nelem > 0 || !h.push_zero.empty()) {
    if (!groups.empty()) LaunchCsrToGroupBins(c, data_type == C_API_DTYPE_FLOAT64, indptr_type == C_API_DTYPE_INT64);
  }
  const int32_t* d_col_of = sc.Upload(h.col_of);
  const int64_t cells = nrow * ds.num_groups();
  hipLaunchKernelGGL(k_expand_group_bins, dim3(static_cast<unsigned>((cells + 255) / 256)), dim3(256), 0, 0, c.scratch,
                     c.groups, d_col_of, ds.num_groups(), nrow, d_bins);
  CSRBINCHECK(hipGetLastError());
  CSRBINCHECK(hipDeviceSynchronize());
}

std::vector<char> DeviceBinCsrMatrix(Dataset* ds, const void* indptr, int indptr_type, const int32_t* indices,
                                     const void* data, int data_type, int64_t nrow, int64_t nelem, const Config& cfg) {
  CheckTypes(indptr_type, data_type);
  std::vector<char> done(static_cast<size_t>(ds->num_groups()), 0);
  const int device = BinningDevice(cfg);
  if (device < 0 || nrow <= 0 || nelem < 0) return done;
  const bool indptr_64 = indptr_type == C_API_DTYPE_INT64, is_f64 = data_type == C_API_DTYPE_FLOAT64;
  const SparsePtr ptr{indptr, indptr_64};
  if (!PointerValid(ptr, nrow, nelem)) return done;  // (before any upload: the host takes the matrix)
  const HostTables h(*ds);
  if (h.gid.empty() || static_cast<int>(h.push_zero.size()) > kMaxPushZeroFeatures) return done;
  std::vector<int32_t> sparse_groups;  // eligible groups stored sparse
  int64_t row_bytes = 0;
  for (size_t k = 0; k < h.gid.size(); ++k) {
    const FeatureGroup& fg = ds->group(h.gid[k]);
    row_bytes += fg.bin_bytes;
    if (fg.sparse) sparse_groups.push_back(static_cast<int32_t>(k));
  }
  const int nsg = static_cast<int>(sparse_groups.size());
  if (nsg > 65535) return done;  // (the compaction grids carry the group in y)
  // ---- chunks: rows [chunk_start[k], chunk_start[k + 1])
  const size_t esz = is_f64 ? sizeof(double) : sizeof(float), psz = indptr_64 ? sizeof(int64_t) : sizeof(int32_t);
  int64_t max_rows = std::max<int64_t>(1, std::min<int64_t>(nrow, kChunkBytes / row_bytes));
  if (const char* e = tuning::Get(tuning::Knob::BinChunkRows)) {
    if (std::atoll(e) > 0) max_rows = std::min<int64_t>(nrow, std::atoll(e));
  }
  const int64_t max_entries = kChunkBytes / static_cast<int64_t>(esz + sizeof(int32_t));
  std::vector<int64_t> chunk_start(1, 0);
  int64_t cap_rows = 0, cap_entries = 0;
  while (chunk_start.back() < nrow) {
    const int64_t r0 = chunk_start.back();
    int64_t r1 = std::min(nrow, r0 + max_rows);
    if (ptr[r1] - ptr[r0] > max_entries) {  // the last row that keeps the entries under the cap
      int64_t lo = r0 + 1, hi = r1;         // (at least one row)
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (ptr[mid] - ptr[r0] <= max_entries) lo = mid;
        else hi = mid - 1;
      }
      r1 = lo;
    }
    cap_rows = std::max(cap_rows, r1 - r0);
    cap_entries = std::max(cap_entries, ptr[r1] - ptr[r0]);
    chunk_start.push_back(r1);
  }
  DeviceScope sc;
  sc.Enter(device);
  std::vector<CsrBinGroup> groups;
  const int64_t scratch_bytes = PlaceColumns(*ds, h, cap_rows, &groups);
  CsrBinArgs c;
  c.t = UploadTables(h, &sc);
  c.groups = sc.Upload(groups);
  char* d_indptr = sc.Alloc<char>(psz * static_cast<size_t>(cap_rows + 1));
  int32_t* d_indices = sc.Alloc<int32_t>(static_cast<size_t>(cap_entries));
  char* d_data = sc.Alloc<char>(esz * static_cast<size_t>(cap_entries));
  c.scratch = sc.Alloc<uint8_t>(static_cast<size_t>(scratch_bytes));
  c.indptr = d_indptr;
  c.indices = d_indices;
  c.data = d_data;
  StoredCellLists lists(&sc, nsg, cap_rows);
  for (size_t ch = 0; ch + 1 < chunk_start.size(); ++ch) {
    const int64_t r0 = chunk_start[ch], rows = chunk_start[ch + 1] - r0;
    const int64_t e0 = ptr[r0], entries = ptr[r0 + rows] - e0;
    CSRBINCHECK(hipMemcpy(d_indptr, static_cast<const char*>(indptr) + psz * static_cast<size_t>(r0),
                          psz * static_cast<size_t>(rows + 1), hipMemcpyHostToDevice));
    if (entries > 0) {
      CSRBINCHECK(hipMemcpy(d_indices, indices + e0, sizeof(int32_t) * static_cast<size_t>(entries),
                            hipMemcpyHostToDevice));
      CSRBINCHECK(hipMemcpy(d_data, static_cast<const char*>(data) + esz * static_cast<size_t>(e0),
                            esz * static_cast<size_t>(entries), hipMemcpyHostToDevice));
    }
    // (the columns keep their places of cap_rows rows: a shorter chunk fills their heads)
    CSRBINCHECK(hipMemsetAsync(c.scratch, 0, static_cast<size_t>(std::max<int64_t>(1, scratch_bytes)), 0));
    c.entry_base = e0;
    c.num_rows = rows;
    c.num_entries = entries;
    if (entries > 0 || !h.push_zero.empty()) LaunchCsrToGroupBins(c, is_f64, indptr_64);
    lists.Append(ds, h, groups, c.groups, c.scratch, sparse_groups, rows, r0);
    for (size_t k = 0; k < h.gid.size(); ++k) {
      FeatureGroup& fg = ds->mutable_group(h.gid[k]);
      if (fg.sparse) continue;
      CSRBINCHECK(hipMemcpy(fg.data.data() + static_cast<size_t>(r0) * fg.bin_bytes, c.scratch + groups[k].off,
                            static_cast<size_t>(rows) * fg.bin_bytes, hipMemcpyDeviceToHost));
    }
  }
  for (int g : h.gid) done[g] = 1;
  NoteDeviceBinCall(true);
  return done;
}

}  // namespace lgbm_amd
