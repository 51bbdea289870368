// What the sparse binning paths share on the device (src/device/csr_bin_kernels.hip,
// src/device/csc_bin_kernels.hip): the scratch of one column per eligible group ([group][row], the
// group's bin_bytes per cell), the compaction of sparse groups (FeatureGroup::sparse) into
// ascending stored rows and their bins, the scratch as the int32 matrix of the ops, and the host
// tables of a dataset's eligible groups.
//
//   k_count_stored / k_scan_counts / k_write_stored
//                        the non-zero cells of a sparse group's scratch column are counted per
//                        (256-row tile, group), each group's counts scanned by a workgroup (the
//                        host places the groups' lists one behind the other from their totals),
//                        and every tile writes its cells at its offset in row order (ballot
//                        ranks: no atomics).  Only these lists cross back to the host.
//   k_expand_group_bins  the scratch as out[rows][groups of the dataset], -1 in host-only groups
//
// Included by HIP sources only; every kernel and helper has internal linkage (one copy per file).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "csr_bins.h"
#include "device_common.h"
#include "lgbm_amd/c_api.h"
#include "lgbm_amd/dataset.h"
#include "lgbm_amd/log.h"

namespace lgbm_amd {

namespace {

#define GROUPBINCHECK(x)                                                                              \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) Log::Fatal("HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

using dev::CsrBinFeat;
using dev::CsrBinTables;
using dev::kWave;

constexpr int kMaxPushZeroFeatures = 4096;  // (the CSR kernel: 512 B of flags per wave)
constexpr int kTileRows = 256;              // compaction tile (one workgroup)
constexpr int kScanThreads = 1024;
constexpr int64_t kChunkBytes = int64_t{256} << 20;

// an eligible group's column in the scratch
struct CsrBinGroup {
  long long off;  // byte offset of the column
  int32_t bytes;  // 1, 2 or 4 per cell
  int32_t pad;
};

__device__ __forceinline__ void StoreCell(uint8_t* scratch, const CsrBinGroup& G, int64_t row, uint32_t v) {
  uint8_t* o = scratch + G.off;
  if (G.bytes == 1) o[row] = static_cast<uint8_t>(v);
  else if (G.bytes == 2) reinterpret_cast<uint16_t*>(o)[row] = static_cast<uint16_t>(v);
  else reinterpret_cast<uint32_t*>(o)[row] = v;
}

__device__ __forceinline__ uint32_t LoadCell(const uint8_t* scratch, const CsrBinGroup& G, int64_t row) {
  const uint8_t* o = scratch + G.off;
  if (G.bytes == 1) return o[row];
  if (G.bytes == 2) return reinterpret_cast<const uint16_t*>(o)[row];
  return reinterpret_cast<const uint32_t*>(o)[row];
}

// stored (non-zero) cells of tile blockIdx.x of the column of sparse group blockIdx.y
__global__ __launch_bounds__(kTileRows) void k_count_stored(const uint8_t* scratch, const CsrBinGroup* groups,
                                                            const int32_t* sparse_groups, int64_t rows, int ntiles,
                                                            int32_t* counts) {
  const CsrBinGroup G = groups[sparse_groups[blockIdx.y]];
  const int64_t row = blockIdx.x * static_cast<int64_t>(kTileRows) + threadIdx.x;
  const int n = __syncthreads_count(row < rows && LoadCell(scratch, G, row) != 0u);
  if (threadIdx.x == 0) counts[static_cast<int64_t>(blockIdx.y) * ntiles + blockIdx.x] = n;
}

// exclusive scan of the tile counts of sparse group blockIdx.x (counts[group][tile]) into offsets,
// relative to the group's first stored cell, and the group's total
__global__ __launch_bounds__(kScanThreads) void k_scan_counts(const int32_t* counts, int ntiles, int32_t* offsets,
                                                              long long* totals) {
  __shared__ int s_wave[kScanThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int32_t* in = counts + static_cast<int64_t>(blockIdx.x) * ntiles;
  int32_t* out = offsets + static_cast<int64_t>(blockIdx.x) * ntiles;
  int carry = 0;  // (at most the chunk's rows)
  for (int base = 0; base < ntiles; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const int v = i < ntiles ? in[i] : 0;
    int incl = v;
    for (int o = 1; o < kWave; o <<= 1) {
      const int t = __shfl_up(incl, o, kWave);
      if (lane >= o) incl += t;
    }
    if (lane == kWave - 1) s_wave[w] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int j = 0; j < kScanThreads / kWave; ++j) {
      if (j < w) before += s_wave[j];
      total += s_wave[j];
    }
    if (i < ntiles) out[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// the stored cells of a tile, in row order, at the tile's offset behind the group's first cell
// first[group]: rows (of the whole matrix) into out_rows, bins packed at the group's width from
// byte val_off[group] of out_vals
__global__ __launch_bounds__(kTileRows) void k_write_stored(const uint8_t* scratch, const CsrBinGroup* groups,
                                                            const int32_t* sparse_groups, int64_t rows, int ntiles,
                                                            int64_t row0, const int32_t* offsets,
                                                            const long long* first, const long long* val_off,
                                                            int32_t* out_rows, uint8_t* out_vals) {
  __shared__ int s_n[kTileRows / kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const CsrBinGroup G = groups[sparse_groups[blockIdx.y]];
  const int64_t row = blockIdx.x * static_cast<int64_t>(kTileRows) + threadIdx.x;
  const uint32_t v = row < rows ? LoadCell(scratch, G, row) : 0u;
  const unsigned long long mask = __ballot(v != 0u);
  if (lane == 0) s_n[w] = __popcll(mask);
  __syncthreads();
  if (v == 0u) return;
  int rank = __popcll(mask & ((1ull << lane) - 1ull));
  for (int j = 0; j < w; ++j) rank += s_n[j];
  const long long k = offsets[static_cast<int64_t>(blockIdx.y) * ntiles + blockIdx.x] + rank;
  out_rows[first[blockIdx.y] + k] = static_cast<int32_t>(row0 + row);
  uint8_t* o = out_vals + val_off[blockIdx.y];
  if (G.bytes == 1) o[k] = static_cast<uint8_t>(v);
  else if (G.bytes == 2) reinterpret_cast<uint16_t*>(o)[k] = static_cast<uint16_t>(v);
  else reinterpret_cast<uint32_t*>(o)[k] = v;
}

// the scratch as the int32 matrix of LGBM_AMD_DatasetGetGroupBins: out[rows][num_ds_groups],
// -1 in the columns of host-only groups (col_of[g] < 0)
__global__ __launch_bounds__(256) void k_expand_group_bins(const uint8_t* scratch, const CsrBinGroup* groups,
                                                           const int32_t* col_of, int num_ds_groups, int64_t rows,
                                                           int32_t* out) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (i >= rows * num_ds_groups) return;
  const int64_t row = i / num_ds_groups;
  const int k = col_of[i % num_ds_groups];
  out[i] = k < 0 ? -1 : static_cast<int32_t>(LoadCell(scratch, groups[k], row));
}

// ---- host side

// the tables of a dataset: its eligible groups (every member numerical) and their features
struct HostTables {
  std::vector<int32_t> feat_of;
  std::vector<CsrBinFeat> feats;
  std::vector<double> ub;
  std::vector<int32_t> push_zero;
  std::vector<int> gid;         // dataset group of each eligible group
  std::vector<int32_t> col_of;  // eligible group of each dataset group, or -1

  explicit HostTables(const Dataset& ds) {
    feat_of.assign(static_cast<size_t>(std::max(0, ds.num_total_features())), -1);
    col_of.assign(static_cast<size_t>(ds.num_groups()), -1);
    std::vector<int32_t> feat_of_inner(static_cast<size_t>(ds.num_features()), -1);
    for (int g = 0; g < ds.num_groups(); ++g) {
      const FeatureGroup& fg = ds.group(g);
      bool ok = !fg.inner_features.empty();
      for (int inner : fg.inner_features) ok = ok && ds.FeatureBinMapper(inner)->bin_type() == BinType::Numerical;
      if (!ok) continue;
      col_of[g] = static_cast<int32_t>(gid.size());
      for (size_t k = 0; k < fg.inner_features.size(); ++k) {
        const int inner = fg.inner_features[k];
        const BinMapper* m = ds.FeatureBinMapper(inner);
        const bool nan_miss = m->missing_type() == MissingType::NaN;
        CsrBinFeat F;
        F.hi = m->num_bin() - 1 - (nan_miss ? 1 : 0);
        F.nan_bin = nan_miss ? m->num_bin() - 1 : -1;
        F.mfb = static_cast<int32_t>(m->GetMostFreqBin());
        F.ub_off = static_cast<int32_t>(ub.size());
        F.goff = fg.bin_offsets[k];
        F.group = static_cast<int32_t>(gid.size());
        F.pz = -1;
        F.pad = 0;
        const auto& u = m->upper_bounds();
        ub.insert(ub.end(), u.begin(), u.end());
        feat_of_inner[inner] = static_cast<int32_t>(feats.size());
        feat_of[ds.RealFeatureIndex(inner)] = static_cast<int32_t>(feats.size());
        feats.push_back(F);
      }
      gid.push_back(g);
    }
    for (int inner : ds.FeatureNeedPushZeros()) {
      const int32_t f = feat_of_inner[inner];
      if (f < 0) continue;
      feats[f].pz = static_cast<int32_t>(push_zero.size());
      push_zero.push_back(f);
    }
  }

  CsrBinTables View() const {
    CsrBinTables t;
    t.feat_of = feat_of.data();
    t.num_total_features = static_cast<int32_t>(feat_of.size());
    t.feats = feats.data();
    t.ub = ub.data();
    t.push_zero = push_zero.data();
    t.num_push_zero = static_cast<int32_t>(push_zero.size());
    t.num_groups = static_cast<int32_t>(gid.size());
    return t;
  }
};

// device buffers freed, and the caller's device restored, at scope exit (also when a HIP call throws)
struct DeviceScope {
  std::vector<void*> ptrs;
  int prev = -1;
  ~DeviceScope() {
    for (void* p : ptrs) (void)hipFree(p);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  void Enter(int dev) {
    GROUPBINCHECK(hipGetDevice(&prev));
    GROUPBINCHECK(hipSetDevice(dev));
  }
  template <typename T>
  T* Alloc(size_t n) {
    void* p = nullptr;
    GROUPBINCHECK(hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)));
    ptrs.push_back(p);
    return static_cast<T*>(p);
  }
  template <typename T>
  T* Upload(const std::vector<T>& v) {
    T* p = Alloc<T>(v.size());
    if (!v.empty()) GROUPBINCHECK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return p;
  }
  void Free(void* p) {
    if (p == nullptr) return;
    ptrs.erase(std::find(ptrs.begin(), ptrs.end(), p));
    (void)hipFree(p);
  }
};

CsrBinTables UploadTables(const HostTables& h, DeviceScope* sc) {
  CsrBinTables t = h.View();
  t.feat_of = sc->Upload(h.feat_of);
  t.feats = sc->Upload(h.feats);
  t.ub = sc->Upload(h.ub);
  t.push_zero = sc->Upload(h.push_zero);
  return t;
}

// the scratch columns of `rows` rows of the eligible groups [k0, k1): 16-byte aligned, in group
// order (the other groups keep offset 0 and are not touched); returns the scratch's bytes
int64_t PlaceColumns(const Dataset& ds, const HostTables& h, int64_t rows, std::vector<CsrBinGroup>* groups,
                     size_t k0 = 0, size_t k1 = SIZE_MAX) {
  groups->clear();
  int64_t off = 0;
  for (size_t k = 0; k < h.gid.size(); ++k) {
    CsrBinGroup G;
    G.off = 0;
    G.bytes = ds.group(h.gid[k]).bin_bytes;
    G.pad = 0;
    if (k >= k0 && k < k1) {
      G.off = off;
      off += (rows * G.bytes + 15) / 16 * 16;
    }
    groups->push_back(G);
  }
  return off;
}

void CheckTypes(int indptr_type, int data_type) {
  if (indptr_type != C_API_DTYPE_INT32 && indptr_type != C_API_DTYPE_INT64) Log::Fatal("Unknown indptr type");
  if (data_type != C_API_DTYPE_FLOAT32 && data_type != C_API_DTYPE_FLOAT64) Log::Fatal("Unknown data type in CSR");
}

// The sparse groups of a scratch into their FeatureGroups: the stored cells of rows [0, rows) of
// the scratch columns `sparse` (eligible groups) are appended, as rows row0 + ..., to sp_rows / data
// of their groups.  Buffers hold up to max_groups groups of cap_rows rows.
class StoredCellLists {
 public:
  StoredCellLists(DeviceScope* sc, int max_groups, int64_t cap_rows) : sc_(sc) {
    if (max_groups <= 0) return;
    const int cap_tiles = static_cast<int>((cap_rows + kTileRows - 1) / kTileRows);
    d_sparse_ = sc->Alloc<int32_t>(static_cast<size_t>(max_groups));
    d_counts_ = sc->Alloc<int32_t>(static_cast<size_t>(max_groups) * cap_tiles);
    d_offsets_ = sc->Alloc<int32_t>(static_cast<size_t>(max_groups) * cap_tiles);
    d_totals_ = sc->Alloc<long long>(static_cast<size_t>(max_groups));
    d_places_ = sc->Alloc<long long>(static_cast<size_t>(max_groups) * 2);
  }

  void Append(Dataset* ds, const HostTables& h, const std::vector<CsrBinGroup>& groups, const CsrBinGroup* d_groups,
              const uint8_t* scratch, const std::vector<int32_t>& sparse, int64_t rows, int64_t row0) {
    const int nsg = static_cast<int>(sparse.size());
    if (nsg == 0) return;
    GROUPBINCHECK(hipMemcpy(d_sparse_, sparse.data(), sizeof(int32_t) * nsg, hipMemcpyHostToDevice));
    const int ntiles = static_cast<int>((rows + kTileRows - 1) / kTileRows);
    const dim3 grid(static_cast<unsigned>(ntiles), static_cast<unsigned>(nsg));
    hipLaunchKernelGGL(k_count_stored, grid, dim3(kTileRows), 0, 0, scratch, d_groups, d_sparse_, rows, ntiles,
                       d_counts_);
    hipLaunchKernelGGL(k_scan_counts, dim3(static_cast<unsigned>(nsg)), dim3(kScanThreads), 0, 0, d_counts_, ntiles,
                       d_offsets_, d_totals_);
    GROUPBINCHECK(hipGetLastError());
    totals_.resize(static_cast<size_t>(nsg));
    places_.resize(static_cast<size_t>(nsg) * 2);
    GROUPBINCHECK(hipMemcpy(totals_.data(), d_totals_, sizeof(long long) * nsg, hipMemcpyDeviceToHost));
    long long* first = places_.data();
    long long* val_off = places_.data() + nsg;
    int64_t total = 0, val_bytes = 0;
    for (int k = 0; k < nsg; ++k) {
      first[k] = total;
      val_off[k] = val_bytes;
      total += totals_[k];
      val_bytes += (totals_[k] * groups[sparse[k]].bytes + 3) / 4 * 4;
    }
    if (total <= 0) return;
    if (total > out_rows_cap_) {
      sc_->Free(d_out_rows_);
      d_out_rows_ = sc_->Alloc<int32_t>(static_cast<size_t>(total));
      out_rows_cap_ = total;
    }
    if (val_bytes > out_vals_cap_) {
      sc_->Free(d_out_vals_);
      d_out_vals_ = sc_->Alloc<uint8_t>(static_cast<size_t>(val_bytes));
      out_vals_cap_ = val_bytes;
    }
    GROUPBINCHECK(hipMemcpy(d_places_, places_.data(), sizeof(long long) * places_.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_write_stored, grid, dim3(kTileRows), 0, 0, scratch, d_groups, d_sparse_, rows, ntiles, row0,
                       d_offsets_, d_places_, d_places_ + nsg, d_out_rows_, d_out_vals_);
    GROUPBINCHECK(hipGetLastError());
    h_rows_.resize(static_cast<size_t>(total));
    h_vals_.resize(static_cast<size_t>(val_bytes));
    GROUPBINCHECK(hipMemcpy(h_rows_.data(), d_out_rows_, sizeof(int32_t) * h_rows_.size(), hipMemcpyDeviceToHost));
    GROUPBINCHECK(hipMemcpy(h_vals_.data(), d_out_vals_, h_vals_.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < nsg; ++k) {
      FeatureGroup& fg = ds->mutable_group(h.gid[sparse[k]]);
      const size_t n = static_cast<size_t>(totals_[k]);
      fg.sp_rows.insert(fg.sp_rows.end(), h_rows_.begin() + first[k], h_rows_.begin() + first[k] + n);
      fg.data.insert(fg.data.end(), h_vals_.begin() + val_off[k], h_vals_.begin() + val_off[k] + n * fg.bin_bytes);
    }
  }

 private:
  DeviceScope* sc_;
  int32_t* d_sparse_ = nullptr;
  int32_t* d_counts_ = nullptr;
  int32_t* d_offsets_ = nullptr;
  long long* d_totals_ = nullptr;  // stored cells of each sparse group
  long long* d_places_ = nullptr;  // first cell, then first value byte, of each group's list
  int32_t* d_out_rows_ = nullptr;
  uint8_t* d_out_vals_ = nullptr;
  int64_t out_rows_cap_ = 0, out_vals_cap_ = 0;
  std::vector<long long> totals_, places_;
  std::vector<int32_t> h_rows_;
  std::vector<uint8_t> h_vals_;
};

}  // namespace

}  // namespace lgbm_amd
