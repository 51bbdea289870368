// Feature binning of CSC matrices on the device (src/device/csc_bins.h: the rule; the host path it
// replaces transposes the matrix into rows and pushes every row).
//
// The scratch is the one of the CSR path (src/device/group_bin_scratch.h): one zero-filled column
// per eligible group, [group][row] at the group's bin_bytes, here over all rows of the matrix and
// the groups of one window.  A feature's values are one contiguous run of stored entries.
//
//   k_csc_bin_column_order  one flag per column of the window: its row indices ascend strictly.
//   k_csc_to_group_bins  a column is walked as src/device/stored_order.h says (WalkColumn), lanes
//                        on consecutive entries: the row, the value's bin by binary search over the
//                        upper bounds in global memory, the group cell, a store into the group's
//                        column.  Launch m takes the m-th member, by ascending column, of every
//                        group of the window, and the stream orders the launches: a higher column
//                        of a bundle overwrites a lower one, no two waves of a launch store to one
//                        cell, and the result is the same on every run.  Entries of a feature whose
//                        zeros are pushed set their row's bit in the feature's bitset of named rows
//                        (atomicOr: the order does not matter).
//   k_csc_push_zeros     one thread per (row, group with such features): the features in push
//                        order, the last one whose bit is clear stores its bin of 0.0.
// Sparse groups are compacted and dense groups copied back as on the CSR path.  Windows are made
// of groups, not rows: as many as keep the scratch, the bitsets and the entries of their columns
// under about 256 MiB, so a sparse group's list is complete in one window.  Only the entries of a
// window's columns are uploaded, runs of adjacent columns as one copy; the column pointer stays
// on the host, which hands every column's clamped entry range to the kernels.
#include "device_common.h"  // (first: the HIP runtime's function attributes, which the rule headers use)

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csc_bins.h"
#include "group_bin_scratch.h"
#include "lgbm_amd/device_binning.h"
#include "lgbm_amd/sparse_ptr.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {

namespace {

using dev::kCscSegmentEntries;
using dev::kCscThreads;
constexpr int kCscWaves = kCscThreads / kWave;
constexpr int kCscBinMaxWindowGroups = 32768;

// one column of a window
struct CscBinItem {
  long long begin, end;  // its entries in the arrays on the device
  int32_t feat;          // CsrBinFeat
  int32_t pz_slot;       // its bitset of named rows in the window, or -1
};

// a feature whose zeros are pushed, and a group with such features: zfeats[begin, end) in push order
struct CscZeroFeat {
  int32_t slot;
  uint32_t cell;  // the group bin of 0.0
};
struct CscZeroGroup {
  int32_t group, begin, end, pad;
};

struct CscBinArgs {
  CsrBinTables t;
  const CsrBinGroup* groups;
  const CscBinItem* items;
  uint32_t* ascending;  // one flag per item
  int32_t num_items;
  const int32_t* indices;
  const void* data;
  int64_t num_row;
  uint8_t* scratch;
  uint32_t* named;      // [slot][named_words]
  int64_t named_words;  // (num_row + 31) / 32
  const CscZeroGroup* zgroups;
  const CscZeroFeat* zfeats;
};

__global__ __launch_bounds__(kCscThreads) void k_csc_bin_column_order(CscBinArgs c) {
  for (int it = blockIdx.y; it < c.num_items; it += gridDim.y) {
    const CscBinItem I = c.items[it];
    dev::ClearUnlessAscending(c.indices, I.begin, I.end, &c.ascending[it]);
  }
}

template <typename T>
__global__ __launch_bounds__(kCscThreads) void k_csc_to_group_bins(CscBinArgs c) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = blockIdx.x * static_cast<int64_t>(kCscWaves) + (threadIdx.x >> 6);
  const int64_t num_waves = gridDim.x * static_cast<int64_t>(kCscWaves);
  const T* data = static_cast<const T*>(c.data);
  for (int it = blockIdx.y; it < c.num_items; it += gridDim.y) {
    const CscBinItem I = c.items[it];
    const CsrBinFeat F = c.t.feats[I.feat];
    const CsrBinGroup G = c.groups[F.group];
    uint32_t* named = I.pz_slot >= 0 ? c.named + I.pz_slot * c.named_words : nullptr;
    int group;
    int64_t r = -1;
    uint32_t cell = 0u;
    dev::WalkColumn(
        c.indices, I.begin, I.end, c.ascending[it] != 0u, wave, num_waves, lane,
        [](int64_t, int64_t) { return false; },  // (all rows of the matrix: no segment is skipped)
        [&](int64_t i, int32_t index) {
          r = dev::CscBinEntryRow(index, c.num_row);
          if (r < 0) return false;
          if (named != nullptr) atomicOr(&named[r >> 5], 1u << (r & 31));
          return dev::CsrFeatWrite(c.t, F, static_cast<double>(data[i]), &group, &cell);
        },
        [&](int64_t) { StoreCell(c.scratch, G, r, cell); });
  }
}

// row blockIdx.x * kTileRows + threadIdx.x of the group zgroups[blockIdx.y]
__global__ __launch_bounds__(kTileRows) void k_csc_push_zeros(CscBinArgs c) {
  const int64_t row = blockIdx.x * static_cast<int64_t>(kTileRows) + threadIdx.x;
  if (row >= c.num_row) return;
  const CscZeroGroup Z = c.zgroups[blockIdx.y];
  bool any = false;
  uint32_t cell = 0u;
  for (int j = Z.begin; j < Z.end; ++j) {
    const CscZeroFeat f = c.zfeats[j];
    if (((c.named[f.slot * c.named_words + (row >> 5)] >> (row & 31)) & 1u) == 0u) {
      cell = f.cell;
      any = true;
    }
  }
  if (any) StoreCell(c.scratch, c.groups[Z.group], row, cell);
}

std::atomic<int64_t> g_csc_calls[2];  // device constructions, column samples

// the columns of a dataset's eligible groups among the ncol columns of a matrix: members[k] of
// eligible group k, (column, CsrBinFeat) by ascending column
std::vector<std::vector<std::pair<int, int32_t>>> GroupMembers(const HostTables& h, int64_t ncol) {
  std::vector<std::vector<std::pair<int, int32_t>>> members(h.gid.size());
  for (size_t col = 0; col < h.feat_of.size() && static_cast<int64_t>(col) < ncol; ++col) {
    const int32_t f = h.feat_of[col];
    if (f >= 0) members[h.feats[f].group].emplace_back(static_cast<int>(col), f);
  }
  return members;
}

// The kernels over the eligible groups [k0, k1) of one window.  begin / end: every column's entry
// range in d_indices / d_data.  The window's tables go up, the scratch (placed by `groups`) is
// filled on the null stream; c->groups is left pointing at the window's group table.
class CscWindow {
 public:
  CscWindow(const HostTables& h, const std::vector<std::vector<std::pair<int, int32_t>>>& members, DeviceScope* sc)
      : h_(h), members_(members), sc_(sc), t_(h.View()) {}

  // the push-zeros features of groups [k0, k1): bitsets this window needs
  int NumPushZero(size_t k0, size_t k1) const {
    int n = 0;
    for (int32_t f : h_.push_zero) n += h_.feats[f].group >= static_cast<int32_t>(k0) && h_.feats[f].group < static_cast<int32_t>(k1);
    return n;
  }

  void Run(CscBinArgs c, size_t k0, size_t k1, const std::vector<CsrBinGroup>& groups,
           const std::vector<long long>& begin, const std::vector<long long>& end, bool is_f64) {
    // ---- the zeros: slots of the window's push-zeros features, their groups in push order
    std::vector<int32_t> slot_of(h_.feats.size(), -1);
    std::vector<std::vector<CscZeroFeat>> zero_of(k1 - k0);
    int nslots = 0;
    for (int32_t f : h_.push_zero) {
      const CsrBinFeat& F = h_.feats[f];
      if (F.group < static_cast<int32_t>(k0) || F.group >= static_cast<int32_t>(k1)) continue;
      slot_of[f] = nslots++;
      int group;
      CscZeroFeat z;
      z.slot = slot_of[f];
      if (dev::CsrFeatWrite(t_, F, 0.0, &group, &z.cell)) zero_of[F.group - k0].push_back(z);
    }
    std::vector<CscZeroGroup> zgroups;
    std::vector<CscZeroFeat> zfeats;
    for (size_t k = k0; k < k1; ++k) {
      if (zero_of[k - k0].empty()) continue;
      CscZeroGroup Z;
      Z.group = static_cast<int32_t>(k);
      Z.begin = static_cast<int32_t>(zfeats.size());
      zfeats.insert(zfeats.end(), zero_of[k - k0].begin(), zero_of[k - k0].end());
      Z.end = static_cast<int32_t>(zfeats.size());
      Z.pad = 0;
      zgroups.push_back(Z);
    }
    // ---- the items: launch m takes the m-th member of every group
    std::vector<CscBinItem> items;
    std::vector<size_t> launch_start(1, 0);
    std::vector<long long> launch_longest;
    for (size_t m = 0;; ++m) {
      long long longest = 0;
      for (size_t k = k0; k < k1; ++k) {
        if (members_[k].size() <= m) continue;
        CscBinItem I;
        I.begin = begin[members_[k][m].first];
        I.end = end[members_[k][m].first];
        I.feat = members_[k][m].second;
        I.pz_slot = slot_of[I.feat];
        if (I.end <= I.begin) continue;
        longest = std::max(longest, I.end - I.begin);
        items.push_back(I);
      }
      if (items.size() > launch_start.back()) {
        launch_start.push_back(items.size());
        launch_longest.push_back(longest);
      }
      bool more = false;
      for (size_t k = k0; k < k1; ++k) more = more || members_[k].size() > m + 1;
      if (!more) break;
    }
    // (the buffers of a window are freed when it is done: the next window's differ in size)
    std::vector<void*> mine;
    auto keep = [&](auto* p) { mine.push_back(const_cast<void*>(static_cast<const void*>(p))); return p; };
    c.groups = keep(sc_->Upload(groups));
    c.items = keep(sc_->Upload(items));
    c.ascending = keep(sc_->Alloc<uint32_t>(items.size()));
    c.named_words = (c.num_row + 31) / 32;
    const size_t named_bytes = sizeof(uint32_t) * static_cast<size_t>(nslots) * static_cast<size_t>(c.named_words);
    c.named = keep(sc_->Alloc<uint32_t>(static_cast<size_t>(nslots) * static_cast<size_t>(c.named_words)));
    c.zgroups = keep(sc_->Upload(zgroups));
    c.zfeats = keep(sc_->Upload(zfeats));
    if (named_bytes > 0) GROUPBINCHECK(hipMemsetAsync(c.named, 0, named_bytes, 0));
    if (!items.empty()) {
      GROUPBINCHECK(hipMemsetAsync(c.ascending, 0xff, sizeof(uint32_t) * items.size(), 0));
      c.num_items = static_cast<int32_t>(items.size());
      long long longest = 0;
      for (long long l : launch_longest) longest = std::max(longest, l);
      hipLaunchKernelGGL(k_csc_bin_column_order, dev::CscGrid(c.num_items, longest, kCscThreads), dim3(kCscThreads), 0, 0, c);
      const CscBinItem* d_items = c.items;
      uint32_t* d_ascending = c.ascending;
      for (size_t m = 0; m + 1 < launch_start.size(); ++m) {
        c.items = d_items + launch_start[m];
        c.ascending = d_ascending + launch_start[m];
        c.num_items = static_cast<int32_t>(launch_start[m + 1] - launch_start[m]);
        const dim3 grid = dev::CscGrid(c.num_items, launch_longest[m], static_cast<int64_t>(kCscWaves) * kCscSegmentEntries);
        if (is_f64) hipLaunchKernelGGL((k_csc_to_group_bins<double>), grid, dim3(kCscThreads), 0, 0, c);
        else hipLaunchKernelGGL((k_csc_to_group_bins<float>), grid, dim3(kCscThreads), 0, 0, c);
      }
      GROUPBINCHECK(hipGetLastError());
    }
    if (!zgroups.empty() && c.num_row > 0) {
      const dim3 grid(static_cast<unsigned>((c.num_row + kTileRows - 1) / kTileRows), static_cast<unsigned>(zgroups.size()));
      hipLaunchKernelGGL(k_csc_push_zeros, grid, dim3(kTileRows), 0, 0, c);
      GROUPBINCHECK(hipGetLastError());
    }
    d_groups_ = c.groups;
    held_ = mine;
  }

  const CsrBinGroup* d_groups() const { return d_groups_; }

  // after the window's results have been read (a blocking copy or a synchronisation)
  void Release() {
    for (void* p : held_) sc_->Free(p);
    held_.clear();
  }

 private:
  const HostTables& h_;
  const std::vector<std::vector<std::pair<int, int32_t>>>& members_;
  DeviceScope* sc_;
  CsrBinTables t_;  // (host pointers: the bin of 0.0)
  const CsrBinGroup* d_groups_ = nullptr;
  std::vector<void*> held_;
};

void CheckCscTypes(int col_ptr_type, int data_type) {
  if (col_ptr_type != C_API_DTYPE_INT32 && col_ptr_type != C_API_DTYPE_INT64) Log::Fatal("Unknown col_ptr type");
  if (data_type != C_API_DTYPE_FLOAT32 && data_type != C_API_DTYPE_FLOAT64) Log::Fatal("Unknown data type in CSC");
}

// every column's clamped entry range (csc_slots.h CscColumnRange)
void ColumnRanges(SparsePtr col_ptr, int64_t ncol, int64_t nelem, std::vector<long long>* begin,
                  std::vector<long long>* end) {
  begin->assign(static_cast<size_t>(ncol), 0);
  end->assign(static_cast<size_t>(ncol), 0);
  for (int64_t col = 0; col < ncol; ++col) {
    int64_t s, e;
    dev::CscColumnRange(col_ptr, static_cast<int>(col), nelem, &s, &e);
    (*begin)[col] = s;
    (*end)[col] = e;
  }
}

}  // namespace

void NoteCscColumnSample() { g_csc_calls[1].fetch_add(1, std::memory_order_relaxed); }

void DeviceBinCscStats(int64_t* csc_calls, int64_t* column_samples) {
  if (csc_calls != nullptr) *csc_calls = g_csc_calls[0].load(std::memory_order_relaxed);
  if (column_samples != nullptr) *column_samples = g_csc_calls[1].load(std::memory_order_relaxed);
}

void CscBinLaunchInfo(int64_t* out) {
  out[0] = kCscSegmentEntries;
  out[1] = kMaxPushZeroFeatures;
  out[2] = kTileRows;
  out[3] = kCscThreads;
  out[4] = kWave;
}

bool CscPointerValid(const void* col_ptr, int col_ptr_type, int64_t ncol_ptr, int64_t nelem) {
  if (col_ptr == nullptr || ncol_ptr < 1 || nelem < 0) return false;
  if (col_ptr_type != C_API_DTYPE_INT32 && col_ptr_type != C_API_DTYPE_INT64) return false;
  return PointerValid(SparsePtr{col_ptr, col_ptr_type == C_API_DTYPE_INT64}, ncol_ptr - 1, nelem);
}

void EvalCscGroupBins(const Dataset& ds, const void* col_ptr, int col_ptr_type, const int32_t* indices,
                      const void* data, int data_type, int64_t ncol_ptr, int64_t nelem, int64_t num_row,
                      int32_t* bins) {
  CheckCscTypes(col_ptr_type, data_type);
  if (num_row <= 0) return;
  const HostTables h(ds);
  const CsrBinTables t = h.View();
  const int ng = ds.num_groups();
  std::vector<int32_t> part(static_cast<size_t>(num_row) * std::max(1, t.num_groups));
  DispatchSparse(col_ptr_type == C_API_DTYPE_INT64, data_type == C_API_DTYPE_FLOAT64, col_ptr, data,
                 [&](auto* ptr, auto* val) {
                   dev::EvalCscToGroupBins(ptr, ncol_ptr - 1, indices, val, nelem, num_row, t, part.data());
                 });
  for (int64_t r = 0; r < num_row; ++r) {
    for (int g = 0; g < ng; ++g) bins[r * ng + g] = h.col_of[g] < 0 ? -1 : part[r * t.num_groups + h.col_of[g]];
  }
}

void CscGroupBinsOnDevice(const Dataset& ds, const void* d_col_ptr, int col_ptr_type, const int32_t* d_indices,
                          const void* d_data, int data_type, int64_t ncol_ptr, int64_t nelem, int64_t num_row,
                          int32_t* d_bins) {
  CheckCscTypes(col_ptr_type, data_type);
  if (num_row <= 0 || ds.num_groups() <= 0) return;
  if (ncol_ptr < 1 || nelem < 0) Log::Fatal("csc group bins: no column pointer");
  const HostTables h(ds);
  if (static_cast<int>(h.push_zero.size()) > kMaxPushZeroFeatures) {
    Log::Fatal("csc group bins: %d features need their zeros pushed, the kernels take %d",
               static_cast<int>(h.push_zero.size()), kMaxPushZeroFeatures);
  }
  const bool ptr_64 = col_ptr_type == C_API_DTYPE_INT64;
  std::vector<char> col_ptr(static_cast<size_t>(ncol_ptr) * (ptr_64 ? sizeof(int64_t) : sizeof(int32_t)));
  GROUPBINCHECK(hipMemcpy(col_ptr.data(), d_col_ptr, col_ptr.size(), hipMemcpyDeviceToHost));
  std::vector<long long> begin, end;
  ColumnRanges(SparsePtr{col_ptr.data(), ptr_64}, ncol_ptr - 1, nelem, &begin, &end);
  DeviceScope sc;
  std::vector<CsrBinGroup> groups;
  const int64_t bytes = PlaceColumns(ds, h, num_row, &groups);
  CscBinArgs c = {};
  c.t = UploadTables(h, &sc);
  c.indices = d_indices;
  c.data = d_data;
  c.num_row = num_row;
  c.scratch = sc.Alloc<uint8_t>(static_cast<size_t>(bytes));
  GROUPBINCHECK(hipMemsetAsync(c.scratch, 0, static_cast<size_t>(std::max<int64_t>(1, bytes)), 0));
  const auto members = GroupMembers(h, ncol_ptr - 1);
  CscWindow window(h, members, &sc);
  window.Run(c, 0, h.gid.size(), groups, begin, end, data_type == C_API_DTYPE_FLOAT64);
  const int32_t* d_col_of = sc.Upload(h.col_of);
  const int64_t cells = num_row * ds.num_groups();
  hipLaunchKernelGGL(k_expand_group_bins, dim3(static_cast<unsigned>((cells + 255) / 256)), dim3(256), 0, 0, c.scratch,
                     window.d_groups(), d_col_of, ds.num_groups(), num_row, d_bins);
  GROUPBINCHECK(hipGetLastError());
  GROUPBINCHECK(hipDeviceSynchronize());
}

std::vector<char> DeviceBinCscMatrix(Dataset* ds, const void* col_ptr, int col_ptr_type, const int32_t* indices,
                                     const void* data, int data_type, int64_t ncol_ptr, int64_t nelem, int64_t num_row,
                                     const Config& cfg) {
  CheckCscTypes(col_ptr_type, data_type);
  std::vector<char> done(static_cast<size_t>(ds->num_groups()), 0);
  const int device = BinningDevice(cfg);
  if (device < 0 || num_row <= 0 || num_row != ds->num_data()) return done;
  // the pointer before any upload: inside [0, nelem] and non-decreasing, or the host takes the matrix
  if (!CscPointerValid(col_ptr, col_ptr_type, ncol_ptr, nelem)) return done;
  const HostTables h(*ds);
  if (h.gid.empty() || static_cast<int>(h.push_zero.size()) > kMaxPushZeroFeatures) return done;
  const bool ptr_64 = col_ptr_type == C_API_DTYPE_INT64, is_f64 = data_type == C_API_DTYPE_FLOAT64;
  const size_t esz = is_f64 ? sizeof(double) : sizeof(float);
  const int64_t ncol = ncol_ptr - 1;
  std::vector<long long> begin, end;  // in the caller's arrays
  ColumnRanges(SparsePtr{col_ptr, ptr_64}, ncol, nelem, &begin, &end);
  const auto members = GroupMembers(h, ncol);
  DeviceScope sc;
  CscWindow window(h, members, &sc);
  // ---- windows: eligible groups [win[w], win[w + 1])
  const int64_t named_bytes = (num_row + 31) / 32 * 4;
  int64_t forced = 0;
  if (const char* e = tuning::Get(tuning::Knob::BinChunkGroups)) forced = std::max<int64_t>(0, std::atoll(e));
  std::vector<size_t> win(1, 0);
  int64_t cap_entries = 0, cap_scratch = 0;
  int cap_sparse = 0;
  {
    int64_t bytes = 0, entries = 0, scratch = 0;
    int sparse = 0;
    for (size_t k = 0; k < h.gid.size(); ++k) {
      const FeatureGroup& fg = ds->group(h.gid[k]);
      int64_t g_entries = 0;
      for (const auto& cm : members[k]) g_entries += end[cm.first] - begin[cm.first];
      const int64_t g_scratch = (num_row * fg.bin_bytes + 15) / 16 * 16;
      const int64_t g_bytes = g_scratch + g_entries * static_cast<int64_t>(esz + sizeof(int32_t)) +
                              named_bytes * window.NumPushZero(k, k + 1);
      const size_t in_window = k - win.back();
      const bool full = forced > 0 ? static_cast<int64_t>(in_window) >= forced
                                   : (bytes + g_bytes > kChunkBytes || in_window >= kCscBinMaxWindowGroups);
      if (in_window > 0 && full) {
        win.push_back(k);
        bytes = entries = scratch = 0;
        sparse = 0;
      }
      bytes += g_bytes;
      entries += g_entries;
      scratch += g_scratch;
      sparse += fg.sparse ? 1 : 0;
      cap_entries = std::max(cap_entries, entries);
      cap_scratch = std::max(cap_scratch, scratch);
      cap_sparse = std::max(cap_sparse, sparse);
    }
    win.push_back(h.gid.size());
  }
  sc.Enter(device);
  CscBinArgs c = {};
  c.t = UploadTables(h, &sc);
  int32_t* d_indices = sc.Alloc<int32_t>(static_cast<size_t>(cap_entries));
  char* d_data = sc.Alloc<char>(esz * static_cast<size_t>(cap_entries));
  c.indices = d_indices;
  c.data = d_data;
  c.num_row = num_row;
  c.scratch = sc.Alloc<uint8_t>(static_cast<size_t>(cap_scratch));
  StoredCellLists lists(&sc, cap_sparse, num_row);
  std::vector<CsrBinGroup> groups;
  std::vector<long long> d_begin(static_cast<size_t>(ncol), 0), d_end(static_cast<size_t>(ncol), 0);
  std::vector<int32_t> cols, sparse_groups;
  std::vector<ColumnRun> runs;
  std::vector<int64_t> placed;
  std::vector<uint8_t> staged;
  for (size_t w = 0; w + 1 < win.size(); ++w) {
    const size_t k0 = win[w], k1 = win[w + 1];
    // ---- the entries of the window's columns, packed in column order; adjacent runs as one copy
    cols.clear();
    sparse_groups.clear();
    for (size_t k = k0; k < k1; ++k) {
      for (const auto& cm : members[k]) cols.push_back(cm.first);
      if (ds->group(h.gid[k]).sparse) sparse_groups.push_back(static_cast<int32_t>(k));
    }
    std::sort(cols.begin(), cols.end());
    PackColumnRuns(cols, SparsePtr{col_ptr, ptr_64}, ncol, &runs, &placed);
    for (size_t j = 0; j < cols.size(); ++j) {
      d_begin[cols[j]] = placed[j];
      d_end[cols[j]] = placed[j + 1];
    }
    for (const ColumnRun& r : runs) {
      GROUPBINCHECK(hipMemcpy(d_indices + r.dst, indices + r.src, sizeof(int32_t) * static_cast<size_t>(r.len),
                              hipMemcpyHostToDevice));
      GROUPBINCHECK(hipMemcpy(d_data + esz * static_cast<size_t>(r.dst),
                              static_cast<const char*>(data) + esz * static_cast<size_t>(r.src),
                              esz * static_cast<size_t>(r.len), hipMemcpyHostToDevice));
    }
    const int64_t scratch_bytes = PlaceColumns(*ds, h, num_row, &groups, k0, k1);
    GROUPBINCHECK(hipMemsetAsync(c.scratch, 0, static_cast<size_t>(std::max<int64_t>(1, scratch_bytes)), 0));
    window.Run(c, k0, k1, groups, d_begin, d_end, is_f64);
    lists.Append(ds, h, groups, window.d_groups(), c.scratch, sparse_groups, num_row, 0);
    // dense groups: their columns, a run of adjacent ones as one copy (many narrow groups of few
    // rows would otherwise pay a copy each)
    for (size_t k = k0; k < k1;) {
      if (ds->group(h.gid[k]).sparse) {
        ++k;
        continue;
      }
      size_t ke = k + 1;
      while (ke < k1 && !ds->group(h.gid[ke]).sparse) ++ke;
      const int64_t run_end = groups[ke - 1].off + num_row * groups[ke - 1].bytes;
      if (ke == k + 1) {
        GROUPBINCHECK(hipMemcpy(ds->mutable_group(h.gid[k]).data.data(), c.scratch + groups[k].off,
                                static_cast<size_t>(run_end - groups[k].off), hipMemcpyDeviceToHost));
      } else {
        staged.resize(static_cast<size_t>(run_end - groups[k].off));
        GROUPBINCHECK(hipMemcpy(staged.data(), c.scratch + groups[k].off, staged.size(), hipMemcpyDeviceToHost));
        for (size_t q = k; q < ke; ++q) {
          FeatureGroup& fg = ds->mutable_group(h.gid[q]);
          std::memcpy(fg.data.data(), staged.data() + (groups[q].off - groups[k].off),
                      static_cast<size_t>(num_row) * fg.bin_bytes);
        }
      }
      k = ke;
    }
    GROUPBINCHECK(hipDeviceSynchronize());
    window.Release();
  }
  for (int g : h.gid) done[g] = 1;
  g_csc_calls[0].fetch_add(1, std::memory_order_relaxed);
  return done;
}

}  // namespace lgbm_amd
