// Feature binning of CSR matrices on the device (src/device/csr_bins.h: the rule of one row;
// reference Dataset::PushOneRow over a sparse row + FeatureGroup::PushData).
//
//   k_csr_to_group_bins  one wave per row, 64 consecutive stored entries per batch (coalesced):
//                        column -> feature (an int32 table over num_total_features), the value's
//                        bin by binary search over the upper bounds in global memory (they do
//                        not fit LDS for wide inputs), the group cell.  The rows of a chunk go
//                        into a zero-filled scratch of one column per group ([group][row], the
//                        group's bin_bytes per cell).  Of a batch's lanes writing one group only
//                        the highest stores (ballots), and between batches the wave waits for
//                        its stores (a workgroup fence), so the last stored write wins on every
//                        run, as in k_csr_to_slots.  The features whose zeros are pushed
//                        (default bin != most frequent bin) are flagged in a per-wave LDS bitset
//                        by the entries that name them; after the entries the unflagged ones
//                        write the bin of 0.0, 64 per batch by the same store rule.
//   k_count_stored / k_scan_counts / k_write_stored
//                        sparse groups (FeatureGroup::sparse) keep the rows whose bin is not 0,
//                        ascending, and their bins: the non-zero cells of the group's scratch
//                        column are counted per (256-row tile, group), each group's counts scanned
//                        by a workgroup (the host places the groups' lists one behind the other
//                        from their totals), and every tile writes its cells at its offset in row
//                        order (ballot ranks: no atomics).  Only these lists cross back to the host.
// Dense groups copy their column back as DeviceBinDenseMatrix does.  Rows stream through in
// chunks whose entries and scratch each stay under about 256 MiB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csr_bins.h"
#include "device_common.h"
#include "lgbm_amd/c_api.h"
#include "lgbm_amd/dataset.h"
#include "lgbm_amd/device_binning.h"
#include "lgbm_amd/log.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {

namespace {

#define CSRBINCHECK(x)                                                                                \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) Log::Fatal("HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

using dev::CsrBinFeat;
using dev::CsrBinTables;
using dev::kWave;

constexpr int kCsrBinThreads = 256;
constexpr int kCsrBinRowsPerBlock = kCsrBinThreads / kWave;
constexpr int kMaxPushZeroFeatures = 4096;  // 512 B of flags per wave
constexpr int kTileRows = 256;              // compaction tile (one workgroup)
constexpr int kScanThreads = 1024;
constexpr int64_t kChunkBytes = int64_t{256} << 20;

// an eligible group's column in the scratch
struct CsrBinGroup {
  long long off;  // byte offset of the column
  int32_t bytes;  // 1, 2 or 4 per cell
  int32_t pad;
};

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

// one batch of a wave's writes to the cells of `row` (group < 0: the lane writes nothing): of the
// lanes on one group only the highest, the last in stored order, stores
__device__ __forceinline__ void StoreBatch(const CsrBinArgs& c, int64_t row, int lane, int group, uint32_t cell) {
  bool write = group >= 0;
  unsigned long long pending = __ballot(group >= 0);
  while (pending != 0ull) {
    const int lead = dev::ReadLane(group, __ffsll(pending) - 1);
    const unsigned long long same = __ballot(group == lead);
    if (group == lead && (same >> lane) > 1ull) write = false;
    pending &= ~same;
  }
  if (write) StoreCell(c.scratch, c.groups[group], row, cell);
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
  dev::CsrBinRowRange(static_cast<const P*>(c.indptr), c.entry_base, c.num_entries, row, &s, &e);
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
    // (this batch's stores and flags are done before the next batch, or the zeros, are issued)
    if (b + kWave < e || npz > 0) __threadfence_block();
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
    if (k0 + kWave < npz) __threadfence_block();
  }
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
    CSRBINCHECK(hipGetDevice(&prev));
    CSRBINCHECK(hipSetDevice(dev));
  }
  template <typename T>
  T* Alloc(size_t n) {
    void* p = nullptr;
    CSRBINCHECK(hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)));
    ptrs.push_back(p);
    return static_cast<T*>(p);
  }
  template <typename T>
  T* Upload(const std::vector<T>& v) {
    T* p = Alloc<T>(v.size());
    if (!v.empty()) CSRBINCHECK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
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

// the scratch columns of `rows` rows: 16-byte aligned, in group order; returns the scratch's bytes
int64_t PlaceColumns(const Dataset& ds, const HostTables& h, int64_t rows, std::vector<CsrBinGroup>* groups) {
  groups->clear();
  int64_t off = 0;
  for (int g : h.gid) {
    CsrBinGroup G;
    G.off = off;
    G.bytes = ds.group(g).bin_bytes;
    G.pad = 0;
    groups->push_back(G);
    off += (rows * G.bytes + 15) / 16 * 16;
  }
  return off;
}

void LaunchCsrToGroupBins(const CsrBinArgs& c, bool is_f64, bool indptr_64) {
  const dim3 grid(static_cast<unsigned>((c.num_rows + kCsrBinRowsPerBlock - 1) / kCsrBinRowsPerBlock));
  const dim3 block(kCsrBinThreads);
  if (is_f64) {
    if (indptr_64) hipLaunchKernelGGL((k_csr_to_group_bins<double, int64_t>), grid, block, 0, 0, c);
    else hipLaunchKernelGGL((k_csr_to_group_bins<double, int32_t>), grid, block, 0, 0, c);
  } else {
    if (indptr_64) hipLaunchKernelGGL((k_csr_to_group_bins<float, int64_t>), grid, block, 0, 0, c);
    else hipLaunchKernelGGL((k_csr_to_group_bins<float, int32_t>), grid, block, 0, 0, c);
  }
  CSRBINCHECK(hipGetLastError());
}

void CheckTypes(int indptr_type, int data_type) {
  if (indptr_type != C_API_DTYPE_INT32 && indptr_type != C_API_DTYPE_INT64) Log::Fatal("Unknown indptr type");
  if (data_type != C_API_DTYPE_FLOAT32 && data_type != C_API_DTYPE_FLOAT64) Log::Fatal("Unknown data type in CSR");
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
    auto run = [&](auto* ptr, auto* val) { dev::EvalCsrToGroupBins(ptr + r0, 0, indices, val, rows, nelem, t, part.data()); };
    const bool f64 = data_type == C_API_DTYPE_FLOAT64;
    if (indptr_type == C_API_DTYPE_INT64) {
      if (f64) run(static_cast<const int64_t*>(indptr), static_cast<const double*>(data));
      else run(static_cast<const int64_t*>(indptr), static_cast<const float*>(data));
    } else {
      if (f64) run(static_cast<const int32_t*>(indptr), static_cast<const double*>(data));
      else run(static_cast<const int32_t*>(indptr), static_cast<const float*>(data));
    }
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
  auto ptr_at = [=](int64_t i) -> int64_t {
    return indptr_64 ? static_cast<const int64_t*>(indptr)[i] : static_cast<const int32_t*>(indptr)[i];
  };
  // indptr before any upload: inside [0, nelem] and non-decreasing, or the host takes the matrix
  if (ptr_at(0) < 0 || ptr_at(nrow) > nelem) return done;
  for (int64_t r = 0; r < nrow; ++r) {
    if (ptr_at(r + 1) < ptr_at(r)) return done;
  }
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
    if (ptr_at(r1) - ptr_at(r0) > max_entries) {  // the last row that keeps the entries under the cap
      int64_t lo = r0 + 1, hi = r1;               // (at least one row)
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (ptr_at(mid) - ptr_at(r0) <= max_entries) lo = mid;
        else hi = mid - 1;
      }
      r1 = lo;
    }
    cap_rows = std::max(cap_rows, r1 - r0);
    cap_entries = std::max(cap_entries, ptr_at(r1) - ptr_at(r0));
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
  const int cap_tiles = static_cast<int>((cap_rows + kTileRows - 1) / kTileRows);
  const int32_t* d_sparse_groups = sc.Upload(sparse_groups);
  int32_t* d_counts = nullptr;
  int32_t* d_offsets = nullptr;
  long long* d_totals = nullptr;  // [nsg]: stored cells of each sparse group in the chunk
  long long* d_places = nullptr;  // [2 * nsg]: first cell, then first value byte, of each group's list
  if (nsg > 0) {
    d_counts = sc.Alloc<int32_t>(static_cast<size_t>(nsg) * cap_tiles);
    d_offsets = sc.Alloc<int32_t>(static_cast<size_t>(nsg) * cap_tiles);
    d_totals = sc.Alloc<long long>(static_cast<size_t>(nsg));
    d_places = sc.Alloc<long long>(static_cast<size_t>(nsg) * 2);
  }
  int32_t* d_out_rows = nullptr;
  uint8_t* d_out_vals = nullptr;
  int64_t out_rows_cap = 0, out_vals_cap = 0;
  std::vector<long long> totals(static_cast<size_t>(nsg)), places(static_cast<size_t>(nsg) * 2);
  std::vector<int32_t> h_rows;
  std::vector<uint8_t> h_vals;
  for (size_t ch = 0; ch + 1 < chunk_start.size(); ++ch) {
    const int64_t r0 = chunk_start[ch], rows = chunk_start[ch + 1] - r0;
    const int64_t e0 = ptr_at(r0), entries = ptr_at(r0 + rows) - e0;
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
    if (nsg > 0) {
      const int ntiles = static_cast<int>((rows + kTileRows - 1) / kTileRows);
      const dim3 grid(static_cast<unsigned>(ntiles), static_cast<unsigned>(nsg));
      hipLaunchKernelGGL(k_count_stored, grid, dim3(kTileRows), 0, 0, c.scratch, c.groups, d_sparse_groups, rows,
                         ntiles, d_counts);
      hipLaunchKernelGGL(k_scan_counts, dim3(static_cast<unsigned>(nsg)), dim3(kScanThreads), 0, 0, d_counts, ntiles,
                         d_offsets, d_totals);
      CSRBINCHECK(hipGetLastError());
      CSRBINCHECK(hipMemcpy(totals.data(), d_totals, sizeof(long long) * nsg, hipMemcpyDeviceToHost));
      long long* first = places.data();
      long long* val_off = places.data() + nsg;
      int64_t total = 0, val_bytes = 0;
      for (int k = 0; k < nsg; ++k) {
        first[k] = total;
        val_off[k] = val_bytes;
        total += totals[k];
        val_bytes += (totals[k] * groups[sparse_groups[k]].bytes + 3) / 4 * 4;
      }
      if (total > 0) {
        if (total > out_rows_cap) {
          sc.Free(d_out_rows);
          d_out_rows = sc.Alloc<int32_t>(static_cast<size_t>(total));
          out_rows_cap = total;
        }
        if (val_bytes > out_vals_cap) {
          sc.Free(d_out_vals);
          d_out_vals = sc.Alloc<uint8_t>(static_cast<size_t>(val_bytes));
          out_vals_cap = val_bytes;
        }
        CSRBINCHECK(hipMemcpy(d_places, places.data(), sizeof(long long) * places.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_write_stored, grid, dim3(kTileRows), 0, 0, c.scratch, c.groups, d_sparse_groups, rows,
                           ntiles, r0, d_offsets, d_places, d_places + nsg, d_out_rows, d_out_vals);
        CSRBINCHECK(hipGetLastError());
        h_rows.resize(static_cast<size_t>(total));
        h_vals.resize(static_cast<size_t>(val_bytes));
        CSRBINCHECK(hipMemcpy(h_rows.data(), d_out_rows, sizeof(int32_t) * h_rows.size(), hipMemcpyDeviceToHost));
        CSRBINCHECK(hipMemcpy(h_vals.data(), d_out_vals, h_vals.size(), hipMemcpyDeviceToHost));
        for (int k = 0; k < nsg; ++k) {
          FeatureGroup& fg = ds->mutable_group(h.gid[sparse_groups[k]]);
          const size_t n = static_cast<size_t>(totals[k]);
          fg.sp_rows.insert(fg.sp_rows.end(), h_rows.begin() + first[k], h_rows.begin() + first[k] + n);
          fg.data.insert(fg.data.end(), h_vals.begin() + val_off[k], h_vals.begin() + val_off[k] + n * fg.bin_bytes);
        }
      }
    }
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
