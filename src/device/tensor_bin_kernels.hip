// A Dataset from a matrix that already lies in device memory (LGBM_AMD_DatasetCreateFromDeviceMat:
// a GPU tensor handed to lgb.Dataset), read where it lies: float16, bfloat16, float32 or float64
// elements behind a pointer with a row and a column stride (row-major, column-major and sliced
// views alike).  The bin mappers are found on the host, as for a host matrix, from the sampled
// rows; everything that touches the whole matrix runs here.  The rule of a row is
// src/device/tensor_bins.h.
//
//   k_gather_sample         the sampled rows as doubles, column-major [column][sample].  A workgroup
//                           takes a 32 x 32 tile of (sample, column) and transposes it through LDS
//                           (33-double pitch): it reads along the matrix's smaller stride --
//                           consecutive columns of one sampled row of a row-major matrix, else
//                           neighbouring sampled rows of one column -- and writes consecutive
//                           sample positions of one column, 256 B per wave row either way.
//   k_tensor_to_group_bins  a workgroup of 256 threads takes a tile of 256 rows and a slice of
//                           consecutive groups.  The slice's upper bounds and category tables are
//                           staged in LDS once; its member columns then go through a value tile in
//                           batches of 64 B per row (8 float64, 16 float32, 32 half columns),
//                           loaded along the smaller stride and stored column by column with a
//                           pitch of 257 elements, so that the load phase (lanes across columns)
//                           and the bin phase (one thread per row) both spread over the banks.
//                           One thread per row then forms the cells of the slice's groups, carrying
//                           a group's cell across batches, and stores them coalesced.
//   k_gather_column         the columns of the groups that stay on the host (sparse storage, a
//                           categorical feature above the LDS table) as contiguous doubles
//
// Sizes (gfx950: 160 KiB of LDS per CU, 64 KiB per workgroup without opting in; binning is bound
// by the matrix read and the dependent LDS loads of the binary search, so resident waves matter
// more than registers).  A slice is closed when its tables would pass 4096 upper bounds (32 KiB:
// 16 features of 255 bins) or 2048 category words (8 KiB: one feature at kTensorMaxCategories);
// the value tile adds 16 KiB (8 KiB for the half types).  The launch asks for the widest slice of
// the dataset only: with max_bin=63 that is about 8 + 16 KiB and six workgroups (24 waves) per CU,
// at the cap 56 KiB and two.  A 64 B batch is half a cache line per row; slices are the fast grid
// dimension, so the workgroup that reads the other half runs next to this one and finds it in L2.
// Tables of a single group above the caps are read from global memory.
// Rows stream through in chunks of at most ~256 MiB of cells; each group column of a chunk is
// copied into the host FeatureGroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "bin_find.h"
#include "group_bin_scratch.h"
#include "lgbm_amd/c_api.h"
#include "lgbm_amd/common.h"
#include "lgbm_amd/dataset.h"
#include "lgbm_amd/device_binning.h"
#include "lgbm_amd/log.h"
#include "lgbm_amd/meta.h"
#include "lgbm_amd/network.h"
#include "lgbm_amd/tuning.h"
#include "sample_distinct.h"
#include "tensor_bins.h"

namespace lgbm_amd {

namespace {

using dev::Bfloat16Bits;
using dev::Float16Bits;
using dev::TensorBinFeat;

constexpr int kTensorTileRows = 256;   // rows of a workgroup (one thread each)
constexpr int kTensorTileRowBytes = 64;  // bytes of one row in a value batch
constexpr int kTensorMaxTileCols = 32;
constexpr int kTensorUbDoubles = 4096;   // upper bounds of a slice staged in LDS
constexpr int kTensorCatWords = 2 * dev::kTensorMaxCategories;  // (category, bin) words of a slice
constexpr int kGatherTile = 32;          // sampled rows x columns of a k_gather_sample workgroup
constexpr int kGatherThreads = 256;

template <typename T>
constexpr int TileCols() {
  return kTensorTileRowBytes / static_cast<int>(sizeof(T));
}

// a group the device takes: its cell column in the chunk output, and the end of its features
struct TensorBinGroup {
  long long off;  // byte offset of the column
  int32_t bytes;  // 1, 2 or 4 per cell
  int32_t fend;   // its features end here (they begin where the group before ends)
};

// consecutive groups [g0, g1), their features [f0, f1) and the ranges of their tables
struct TensorBinSlice {
  int32_t g0, g1, f0, f1;
  int32_t ub_lo, ub_n, cat_lo, cat_n;
};

template <typename T>
__global__ __launch_bounds__(kGatherThreads) void k_gather_sample(const T* x, long long rs, long long cs,
                                                                  const int32_t* idx, int ns, int c0, int nc,
                                                                  int ntile_s, double* out) {
  __shared__ double s_tile[kGatherTile][kGatherTile + 1];
  const int tx = threadIdx.x % kGatherTile, ty = threadIdx.x / kGatherTile;
  const int s0 = static_cast<int>(blockIdx.x % ntile_s) * kGatherTile;
  const int cb = static_cast<int>(blockIdx.x / ntile_s) * kGatherTile;
  const bool cols_fast = cs <= rs;
  for (int k = ty; k < kGatherTile; k += kGatherThreads / kGatherTile) {
    const int ds = cols_fast ? k : tx, dc = cols_fast ? tx : k;
    if (s0 + ds < ns && cb + dc < nc) {
      s_tile[ds][dc] = dev::WidenElement(x[rs * idx[s0 + ds] + cs * (c0 + cb + dc)]);
    }
  }
  __syncthreads();
  for (int k = ty; k < kGatherTile; k += kGatherThreads / kGatherTile) {
    if (s0 + tx < ns && cb + k < nc) out[static_cast<long long>(cb + k) * ns + s0 + tx] = s_tile[tx][k];
  }
}

template <typename T>
__global__ __launch_bounds__(kTensorTileRows) void k_tensor_to_group_bins(
    const T* x, int rows, long long rs, long long cs, int nslices, const TensorBinSlice* slices,
    const TensorBinGroup* groups, const TensorBinFeat* feats, const double* ub, const int32_t* cat, int ub_cap,
    int cat_cap, uint8_t* out) {
  constexpr int kCols = TileCols<T>(), kPitch = kTensorTileRows + 1;
  extern __shared__ double s_mem[];
  __shared__ int s_col[kTensorMaxTileCols];
  double* s_ub = s_mem;
  int32_t* s_cat = reinterpret_cast<int32_t*>(s_ub + ub_cap);
  T* s_val = reinterpret_cast<T*>(s_cat + cat_cap);  // (cat_cap is even: 8-byte aligned)
  const int tid = threadIdx.x;
  const TensorBinSlice S = slices[blockIdx.x % nslices];
  const int row0 = static_cast<int>(blockIdx.x / nslices) * kTensorTileRows;
  const bool ub_staged = S.ub_n <= ub_cap, cat_staged = S.cat_n <= cat_cap;
  if (ub_staged) {
    for (int j = tid; j < S.ub_n; j += kTensorTileRows) s_ub[j] = ub[S.ub_lo + j];
  }
  if (cat_staged) {
    for (int j = tid; j < S.cat_n; j += kTensorTileRows) s_cat[j] = cat[S.cat_lo + j];
  }
  const bool cols_fast = cs <= rs;
  const bool live = row0 + tid < rows;
  int g = S.g0;
  TensorBinGroup G = groups[g];
  uint32_t v = 0;
  auto store = [&]() {
    uint8_t* o = out + G.off;
    const int r = row0 + tid;
    if (G.bytes == 1) o[r] = static_cast<uint8_t>(v);
    else if (G.bytes == 2) reinterpret_cast<uint16_t*>(o)[r] = static_cast<uint16_t>(v);
    else reinterpret_cast<uint32_t*>(o)[r] = v;
  };
  for (int fb = S.f0; fb < S.f1; fb += kCols) {
    const int nb = min(kCols, S.f1 - fb);
    __syncthreads();  // (the batch before is consumed)
    if (tid < nb) s_col[tid] = feats[fb + tid].col;
    __syncthreads();  // (... and the tables are staged)
    for (int i = tid; i < kCols * kTensorTileRows; i += kTensorTileRows) {
      const int r = cols_fast ? i / kCols : i % kTensorTileRows;
      const int c = cols_fast ? i % kCols : i / kTensorTileRows;
      if (c < nb && row0 + r < rows) s_val[c * kPitch + r] = x[rs * (row0 + r) + cs * s_col[c]];
    }
    __syncthreads();
    if (!live) continue;
    for (int c = 0; c < nb; ++c) {
      const int f = fb + c;
      while (f >= G.fend) {
        store();
        G = groups[++g];
        v = 0;
      }
      const TensorBinFeat F = feats[f];
      const void* table;
      if (F.ncat >= 0) table = cat_staged ? s_cat + (F.tab_off - S.cat_lo) : cat + F.tab_off;
      else table = ub_staged ? static_cast<const void*>(s_ub + (F.tab_off - S.ub_lo)) : ub + F.tab_off;
      dev::TensorFeatWrite(F, dev::WidenElement(s_val[c * kPitch + tid]), table, &v);
    }
  }
  if (live) store();
}

// column cols[blockIdx.x / ntile_rows] of the chunk as doubles at out[that index][rows]
template <typename T>
__global__ __launch_bounds__(kTensorTileRows) void k_gather_column(const T* x, int rows, long long rs, long long cs,
                                                                   const int32_t* cols, int ntile_rows, double* out) {
  const int k = static_cast<int>(blockIdx.x / ntile_rows);
  const int r = static_cast<int>(blockIdx.x % ntile_rows) * kTensorTileRows + threadIdx.x;
  if (r < rows) out[static_cast<long long>(k) * rows + r] = dev::WidenElement(x[rs * r + cs * cols[k]]);
}

// ---- host side

// f(typed null pointer) for the element type of `data_type`
template <typename F>
void DispatchElement(int data_type, F&& f) {
  switch (data_type) {
    case C_API_DTYPE_FLOAT32: f(static_cast<const float*>(nullptr)); break;
    case C_API_DTYPE_FLOAT64: f(static_cast<const double*>(nullptr)); break;
    case C_API_DTYPE_FLOAT16: f(static_cast<const Float16Bits*>(nullptr)); break;
    case C_API_DTYPE_BFLOAT16: f(static_cast<const Bfloat16Bits*>(nullptr)); break;
    default: Log::Fatal("Unknown data type of a device matrix: %d", data_type);
  }
}

void CheckTensor(const DeviceTensor& t) {
  if (t.data == nullptr) Log::Fatal("device matrix: null data pointer");
  if (t.nrow <= 0 || t.ncol <= 0) Log::Fatal("device matrix: %d x %d", t.nrow, t.ncol);
  if (t.row_stride < 0 || t.col_stride < 0) Log::Fatal("device matrix: negative stride");
  DispatchElement(t.data_type, [](auto*) {});
}

// the tables of a dataset for a matrix of ncol columns: the groups the device takes, in dataset
// order, each one's members in ascending column order; the slices; the columns left to the host
struct TensorTables {
  std::vector<TensorBinFeat> feats;
  std::vector<TensorBinGroup> groups;
  std::vector<TensorBinSlice> slices;
  std::vector<double> ub;
  std::vector<int32_t> cat;
  std::vector<int> gid;            // dataset group of each device group
  std::vector<int32_t> col_of;     // device group of each dataset group, or -1
  std::vector<int32_t> host_cols;  // used columns of the other groups, ascending

  TensorTables(const Dataset& ds, int ncol) {
    col_of.assign(static_cast<size_t>(ds.num_groups()), -1);
    for (int g = 0; g < ds.num_groups(); ++g) {
      const FeatureGroup& fg = ds.group(g);
      std::vector<std::pair<int, int>> members;  // (column, sub-feature)
      bool ok = !fg.sparse && !fg.inner_features.empty();
      for (size_t k = 0; k < fg.inner_features.size(); ++k) {
        const int inner = fg.inner_features[k];
        const BinMapper* m = ds.FeatureBinMapper(inner);
        const int col = ds.RealFeatureIndex(inner);
        if (col >= ncol) ok = false;
        if (m->bin_type() == BinType::Categorical && m->num_bin() - 1 > dev::kTensorMaxCategories) ok = false;
        members.emplace_back(col, static_cast<int>(k));
      }
      if (!ok) {
        for (const auto& cm : members) {
          if (cm.first < ncol) host_cols.push_back(cm.first);
        }
        continue;
      }
      std::sort(members.begin(), members.end());
      for (const auto& cm : members) feats.push_back(Feat(ds, fg, cm.first, cm.second));
      col_of[g] = static_cast<int32_t>(gid.size());
      groups.push_back(TensorBinGroup{0, fg.bin_bytes, static_cast<int32_t>(feats.size())});
      gid.push_back(g);
    }
    std::sort(host_cols.begin(), host_cols.end());
    // slices: closed when the next group's tables would pass the LDS caps
    for (int k = 0; k < static_cast<int>(groups.size()); ++k) {
      const int f0 = k > 0 ? groups[k - 1].fend : 0, f1 = groups[k].fend;
      const int g_ub = UbBegin(f1) - UbBegin(f0), g_cat = CatBegin(f1) - CatBegin(f0);
      if (slices.empty() || slices.back().ub_n + g_ub > kTensorUbDoubles ||
          slices.back().cat_n + g_cat > kTensorCatWords) {
        slices.push_back(TensorBinSlice{k, k, f0, f0, UbBegin(f0), 0, CatBegin(f0), 0});
      }
      TensorBinSlice& S = slices.back();
      S.g1 = k + 1;
      S.f1 = f1;
      S.ub_n += g_ub;
      S.cat_n += g_cat;
    }
  }

  // LDS words the kernel launch stages: the widest slice within the caps
  int UbCap() const {
    int n = 0;
    for (const auto& S : slices) n = std::max(n, S.ub_n <= kTensorUbDoubles ? S.ub_n : 0);
    return n;
  }
  int CatCap() const {
    int n = 0;
    for (const auto& S : slices) n = std::max(n, S.cat_n <= kTensorCatWords ? S.cat_n : 0);
    return (n + 1) / 2 * 2;
  }

 private:
  // where the tables of the features from f on begin (tables are appended in feature order)
  int32_t UbBegin(int f) const {
    for (; f < static_cast<int>(feats.size()); ++f) {
      if (feats[f].ncat < 0) return feats[f].tab_off;
    }
    return static_cast<int32_t>(ub.size());
  }
  int32_t CatBegin(int f) const {
    for (; f < static_cast<int>(feats.size()); ++f) {
      if (feats[f].ncat >= 0) return feats[f].tab_off;
    }
    return static_cast<int32_t>(cat.size());
  }

  TensorBinFeat Feat(const Dataset& ds, const FeatureGroup& fg, int col, int sub) {
    const BinMapper* m = ds.FeatureBinMapper(fg.inner_features[sub]);
    TensorBinFeat F;
    F.col = col;
    F.mfb = static_cast<int32_t>(m->GetMostFreqBin());
    F.goff = fg.bin_offsets[sub];
    F.pad = 0;
    if (m->bin_type() == BinType::Categorical) {
      // the known categories ascending, their bins behind them (bin 0, category -1, is the
      // answer for everything else)
      std::vector<std::pair<int32_t, int32_t>> known;
      const auto& b2c = m->bin_2_categorical();
      for (int b = 1; b < static_cast<int>(b2c.size()); ++b) {
        if (b2c[b] >= 0) known.emplace_back(b2c[b], b);
      }
      std::sort(known.begin(), known.end());
      F.hi = 0;
      F.nan_bin = -1;
      F.ncat = static_cast<int32_t>(known.size());
      F.tab_off = static_cast<int32_t>(cat.size());
      for (const auto& kb : known) cat.push_back(kb.first);
      for (const auto& kb : known) cat.push_back(kb.second);
    } else {
      const bool nan_miss = m->missing_type() == MissingType::NaN;
      F.hi = m->num_bin() - 1 - (nan_miss ? 1 : 0);
      F.nan_bin = nan_miss ? m->num_bin() - 1 : -1;
      F.ncat = -1;
      F.tab_off = static_cast<int32_t>(ub.size());
      const auto& u = m->upper_bounds();
      ub.insert(ub.end(), u.begin(), u.end());
    }
    return F;
  }
};

std::atomic<int64_t> g_tensor_calls{0};

}  // namespace

void DeviceBinTensorStats(int64_t* tensor_calls, int64_t* bin_find_calls) {
  if (tensor_calls != nullptr) *tensor_calls = g_tensor_calls.load(std::memory_order_relaxed);
  if (bin_find_calls != nullptr) *bin_find_calls = DeviceBinFindCalls();
}

void TensorBinLaunchInfo(int64_t* out) {
  out[0] = kTensorTileRows;
  out[1] = kGatherTile;
  out[2] = dev::kTensorMaxCategories;
  out[3] = kTensorTileRowBytes;
  out[4] = kTensorBinMinValues;
}

bool UseDeviceBinFind(int64_t sample_cnt, int64_t ncol) {
  if (tuning::Off(tuning::Knob::DeviceBinFind) || Network::num_machines() > 1) return false;
  return tuning::On(tuning::Knob::DeviceBinFind) ||
         (sample_cnt >= kBinFindMinSampleRows && sample_cnt * ncol <= kBinFindMaxSampleValues);
}

namespace {

void AppendEvaluatedColumn(const double* col, int64_t n, SampleDistinctLists* out) {
  std::vector<double> d;
  std::vector<int32_t> c;
  out->nan_cnt.push_back(dev::EvalSampleDistinct(col, n, &d, &c));
  int kept = 0;
  for (int32_t v : c) kept += v;
  out->num_values.push_back(kept);
  out->distinct.insert(out->distinct.end(), d.begin(), d.end());
  out->counts.insert(out->counts.end(), c.begin(), c.end());
  out->begin.push_back(static_cast<int64_t>(out->distinct.size()));
}

}  // namespace

void EvalSampleDistinctLists(const double* sample, int64_t ns, int32_t ncol, SampleDistinctLists* out) {
  *out = SampleDistinctLists();
  for (int32_t j = 0; j < ncol; ++j) AppendEvaluatedColumn(sample + static_cast<int64_t>(j) * ns, ns, out);
}

void EvalSampleDistinctLists(const std::vector<std::vector<double>>& columns, SampleDistinctLists* out) {
  *out = SampleDistinctLists();
  for (const auto& v : columns) AppendEvaluatedColumn(v.data(), static_cast<int64_t>(v.size()), out);
}

void SampleDeviceTensor(const DeviceTensor& t, const std::vector<int>& rows, std::vector<std::vector<double>>* sv,
                        std::vector<std::vector<int>>* si, SampleDistinctLists* distinct) {
  CheckTensor(t);
  sv->assign(static_cast<size_t>(t.ncol), {});
  si->assign(static_cast<size_t>(t.ncol), {});
  const int ns = static_cast<int>(rows.size());
  if (ns == 0) {
    if (distinct != nullptr) EvalSampleDistinctLists(nullptr, 0, t.ncol, distinct);
    return;
  }
  for (int r : rows) {
    if (r < 0 || r >= t.nrow) Log::Fatal("device matrix: sampled row %d outside %d rows", r, t.nrow);
  }
  DeviceScope sc;
  sc.Enter(t.device_id);
  const int32_t* d_idx = sc.Upload(std::vector<int32_t>(rows.begin(), rows.end()));
  // columns per pass: at most ~256 MiB of doubles (and of the sort's scratch), whole column tiles
  const int64_t cell = static_cast<int64_t>(sizeof(double)) + (distinct != nullptr ? kBinFindScratchBytes : 0);
  const int64_t fit = kChunkBytes / (cell * ns);
  const int pass = static_cast<int>(std::min<int64_t>(t.ncol, std::max<int64_t>(kGatherTile, fit / kGatherTile * kGatherTile)));
  double* d_out = sc.Alloc<double>(static_cast<size_t>(pass) * ns);
  std::unique_ptr<DeviceSampleDistinct> finder;
  if (distinct != nullptr) {
    *distinct = SampleDistinctLists();
    finder.reset(new DeviceSampleDistinct(pass, ns));
  }
  std::vector<double> h(static_cast<size_t>(pass) * ns);
  const int ntile_s = (ns + kGatherTile - 1) / kGatherTile;
  for (int c0 = 0; c0 < t.ncol; c0 += pass) {
    const int nc = std::min(pass, t.ncol - c0);
    const unsigned grid = static_cast<unsigned>(ntile_s) * static_cast<unsigned>((nc + kGatherTile - 1) / kGatherTile);
    DispatchElement(t.data_type, [&](auto* p) {
      using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
      hipLaunchKernelGGL(k_gather_sample<T>, dim3(grid), dim3(kGatherThreads), 0, 0, static_cast<const T*>(t.data),
                         static_cast<long long>(t.row_stride), static_cast<long long>(t.col_stride), d_idx, ns, c0, nc,
                         ntile_s, d_out);
    });
    GROUPBINCHECK(hipGetLastError());
    GROUPBINCHECK(hipMemcpy(h.data(), d_out, sizeof(double) * static_cast<size_t>(nc) * ns, hipMemcpyDeviceToHost));
    if (finder != nullptr) finder->Launch(d_out, nc);  // (sorts d_out in place while the host filters its copy)
    // the zero / NaN filter of the host's row reader (DenseRowPairFun), sample positions ascending
#pragma omp parallel for schedule(static)
    for (int c = 0; c < nc; ++c) {
      const double* col = h.data() + static_cast<size_t>(c) * ns;
      auto& v = (*sv)[c0 + c];
      auto& at = (*si)[c0 + c];
      for (int i = 0; i < ns; ++i) {
        if (std::fabs(col[i]) > kZeroThreshold || std::isnan(col[i])) {
          v.push_back(col[i]);
          at.push_back(i);
        }
      }
    }
    if (finder != nullptr) finder->Collect(distinct);
  }
  if (distinct != nullptr) NoteDeviceBinFind();
}

void BinDeviceTensor(Dataset* ds, const DeviceTensor& t) {
  CheckTensor(t);
  const TensorTables h(*ds, t.ncol);
  DeviceScope sc;
  sc.Enter(t.device_id);
  const long long rs = t.row_stride, cs = t.col_stride;
  if (!h.groups.empty()) {
    int64_t row_bytes = 0;
    for (const auto& G : h.groups) row_bytes += G.bytes;
    const int64_t chunk = std::min<int64_t>(t.nrow, std::max<int64_t>(kTensorTileRows, kChunkBytes / row_bytes));
    std::vector<TensorBinGroup> groups = h.groups;
    int64_t out_bytes = 0;
    for (auto& G : groups) {  // a column of `chunk` cells per group, 16-byte aligned
      G.off = out_bytes;
      out_bytes += (chunk * G.bytes + 15) / 16 * 16;
    }
    const TensorBinGroup* d_groups = sc.Upload(groups);
    const TensorBinSlice* d_slices = sc.Upload(h.slices);
    const TensorBinFeat* d_feats = sc.Upload(h.feats);
    const double* d_ub = sc.Upload(h.ub);
    const int32_t* d_cat = sc.Upload(h.cat);
    uint8_t* d_out = sc.Alloc<uint8_t>(static_cast<size_t>(out_bytes));
    const int ub_cap = h.UbCap(), cat_cap = h.CatCap(), nslices = static_cast<int>(h.slices.size());
    for (int64_t r0 = 0; r0 < t.nrow; r0 += chunk) {
      const int rows = static_cast<int>(std::min<int64_t>(chunk, t.nrow - r0));
      const int64_t tiles = (rows + kTensorTileRows - 1) / kTensorTileRows;
      if (tiles * nslices > 0x7fffffffLL) Log::Fatal("device matrix: %d slices of groups are too many", nslices);
      DispatchElement(t.data_type, [&](auto* p) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
        const size_t lds = sizeof(double) * ub_cap + sizeof(int32_t) * cat_cap +
                           sizeof(T) * TileCols<T>() * (kTensorTileRows + 1);
        hipLaunchKernelGGL(k_tensor_to_group_bins<T>, dim3(static_cast<unsigned>(tiles * nslices)),
                           dim3(kTensorTileRows), lds, 0, static_cast<const T*>(t.data) + rs * r0, rows, rs, cs, nslices,
                           d_slices, d_groups, d_feats, d_ub, d_cat, ub_cap, cat_cap, d_out);
      });
      GROUPBINCHECK(hipGetLastError());
      for (size_t k = 0; k < groups.size(); ++k) {
        FeatureGroup& fg = ds->mutable_group(h.gid[k]);
        GROUPBINCHECK(hipMemcpy(fg.data.data() + static_cast<size_t>(r0) * fg.bin_bytes, d_out + groups[k].off,
                                static_cast<size_t>(rows) * fg.bin_bytes, hipMemcpyDeviceToHost));
      }
    }
    sc.Free(d_out);
  }
  if (!h.host_cols.empty()) {
    // the other groups: their columns as doubles, pushed as the host's column loop pushes them (a
    // row's pushes from one thread, in ascending column order)
    const int nh = static_cast<int>(h.host_cols.size());
    const int64_t chunk = std::min<int64_t>(
        t.nrow, std::max<int64_t>(kTensorTileRows, kChunkBytes / (static_cast<int64_t>(sizeof(double)) * nh)));
    const int32_t* d_cols = sc.Upload(h.host_cols);
    double* d_vals = sc.Alloc<double>(static_cast<size_t>(chunk) * nh);
    std::vector<double> vals(static_cast<size_t>(chunk) * nh);
    for (int64_t r0 = 0; r0 < t.nrow; r0 += chunk) {
      const int rows = static_cast<int>(std::min<int64_t>(chunk, t.nrow - r0));
      const int ntile_rows = (rows + kTensorTileRows - 1) / kTensorTileRows;
      if (static_cast<int64_t>(ntile_rows) * nh > 0x7fffffffLL) Log::Fatal("device matrix: %d host columns are too many", nh);
      DispatchElement(t.data_type, [&](auto* p) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
        hipLaunchKernelGGL(k_gather_column<T>, dim3(static_cast<unsigned>(ntile_rows) * nh), dim3(kTensorTileRows), 0, 0,
                           static_cast<const T*>(t.data) + rs * r0, rows, rs, cs, d_cols, ntile_rows, d_vals);
      });
      GROUPBINCHECK(hipGetLastError());
      GROUPBINCHECK(hipMemcpy(vals.data(), d_vals, sizeof(double) * static_cast<size_t>(rows) * nh, hipMemcpyDeviceToHost));
      common::OmpErrors errors;
#pragma omp parallel for schedule(static)
      for (int r = 0; r < rows; ++r) {
        errors.Run([&] {
          for (int k = 0; k < nh; ++k) {
            ds->PushColumnValue(static_cast<data_size_t>(r0 + r), h.host_cols[k], vals[static_cast<size_t>(k) * rows + r]);
          }
        });
      }
      errors.Check();
    }
  }
  g_tensor_calls.fetch_add(1, std::memory_order_relaxed);
}

void EvalTensorGroupBins(const Dataset& ds, const void* data, int data_type, int32_t nrow, int32_t ncol,
                         int64_t row_stride, int64_t col_stride, int32_t* bins) {
  CheckTensor(DeviceTensor{data, data_type, nrow, ncol, row_stride, col_stride, 0});
  const TensorTables h(ds, ncol);
  const int ng = ds.num_groups();
  DispatchElement(data_type, [&](auto* p) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
    const T* x = static_cast<const T*>(data);
    for (int64_t r = 0; r < nrow; ++r) {
      int32_t* o = bins + r * ng;
      for (int g = 0; g < ng; ++g) o[g] = h.col_of[g] < 0 ? -1 : 0;
      for (size_t k = 0; k < h.groups.size(); ++k) {
        uint32_t v = 0;
        for (int f = k > 0 ? h.groups[k - 1].fend : 0; f < h.groups[k].fend; ++f) {
          const TensorBinFeat& F = h.feats[f];
          const void* table = F.ncat >= 0 ? static_cast<const void*>(h.cat.data() + F.tab_off) : h.ub.data() + F.tab_off;
          dev::TensorFeatWrite(F, dev::WidenElement(x[row_stride * r + col_stride * F.col]), table, &v);
        }
        o[h.gid[k]] = static_cast<int32_t>(v);
      }
    }
  });
}

}  // namespace lgbm_amd
