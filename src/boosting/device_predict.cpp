// Dense-matrix prediction on the MI355X (the C API's LGBM_BoosterPredictForMat path for a
// booster trained with device_type=gpu, or predicted with device_type=gpu): the forest is
// flattened into node arrays and evaluated by src/device/predict_kernels.hip, one row per
// thread, with the host predictor's semantics (reference GBDT::PredictRaw / Predict,
// src/boosting/gbdt_prediction.cpp:13-64); output transforms stay on the host.  Leaf indices
// come from the same walk and SHAP contributions from the per-leaf path tables of shap_paths.h
// (src/device/shap_kernels.hip).  Rows go through the device in chunks, so that a contribution
// matrix larger than HBM still predicts: one driver (GBDT::PredictChunksOnDevice) stages, runs and
// copies back chunk after chunk for every input layout, and one rule (predict_chunks.h) sizes
// the chunks so that input, output and the accumulator tiles stay within four fifths of the
// free memory.
//
// CSR matrices (LGBM_BoosterPredictForCSR) take the same path: each chunk's rows are scattered on
// the device into a compact matrix with one column per feature the window's trees split on
// (FeatureSlots, src/device/csr_kernels.hip), and the forest is uploaded with its split features
// rewritten to those columns, so the same kernels walk it.
//
// CSC matrices (LGBM_BoosterPredictForCSC) fill the same compact matrix from the other side: a
// feature the trees split on is one column of the matrix, a contiguous run of stored entries.
// Only those runs are uploaded, once per call; every chunk of rows is then scattered from them
// (src/device/csc_kernels.hip).
#include <hip/hip_runtime_api.h>
#include <omp.h>

#include <atomic>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../device/csc_slots.h"
#include "../device/csr_slots.h"
#include "../device/kernels.h"
#include "predict_chunks.h"
#include "shap_paths.h"
#include "lgbm_amd/boosting.h"
#include "lgbm_amd/log.h"
#include "lgbm_amd/sparse_ptr.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {

namespace {

#define HIPCHECK(x)                                                                                 \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) Log::Fatal("HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

std::atomic<int64_t> g_device_predictions{0};

// device copies of host vectors, freed together
struct DeviceBuffers {
  std::vector<void*> ptrs;
  ~DeviceBuffers() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* Upload(const std::vector<T>& v, hipStream_t s) {
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>(1, v.size()) * sizeof(T)));
    ptrs.push_back(p);
    if (!v.empty()) HIPCHECK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return static_cast<T*>(p);
  }
  void* Alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>(1, bytes)));
    ptrs.push_back(p);
    return p;
  }
};


// the forest (and, for contributions, its path tables) of one prediction call on the device
class DeviceForest {
 public:
  // false: the contribution kernel cannot run this forest (the host predicts)
  // slots: the forest walks a compact matrix of the features it splits on (CSR rows, CSC columns)
  bool Upload(const std::vector<const Tree*>& trees, int num_class, int num_features, DevicePredictKind kind,
              hipStream_t s, bool slots = false) {
    kind_ = kind;
    flat_.Build(trees);
    if (kind == DevicePredictKind::Contrib && (!paths_.Build(trees) || !paths_.FitsDevice())) return false;
    f_.num_class = num_class;
    f_.num_trees = static_cast<int32_t>(trees.size());
    f_.node_off = b_.Upload(flat_.node_off, s);
    f_.leaf_off = b_.Upload(flat_.leaf_off, s);
    if (slots) {
      slots_.Build(flat_, num_features);
      f_.feature = b_.Upload(slots_.feature, s);
      slot_of_ = b_.Upload(slots_.slot_of, s);
    } else {
      f_.feature = b_.Upload(flat_.feature, s);
    }
    f_.threshold = b_.Upload(flat_.threshold, s);
    f_.dtype = b_.Upload(flat_.dtype, s);
    f_.left = b_.Upload(flat_.left, s);
    f_.right = b_.Upload(flat_.right, s);
    f_.leaf_value = b_.Upload(flat_.leaf_value, s);
    f_.cat_bound_off = b_.Upload(flat_.cat_bound_off, s);
    f_.cat_bound = b_.Upload(flat_.cat_bound, s);
    f_.cat_bits_off = b_.Upload(flat_.cat_bits_off, s);
    f_.cat_bits = b_.Upload(flat_.cat_bits, s);
    if (kind == DevicePredictKind::Contrib) {
      a_.num_features = num_features;
      a_.max_path_len = paths_.max_path_len;
      a_.mask_words = paths_.mask_words;
      a_.tree_leaf_off = b_.Upload(paths_.tree_leaf_off, s);
      a_.leaf_elem_off = b_.Upload(paths_.leaf_elem_off, s);
      a_.leaf_value = b_.Upload(paths_.leaf_value, s);
      a_.elem_feature = b_.Upload(paths_.elem_feature, s);
      a_.elem_zero = b_.Upload(paths_.elem_zero, s);
      a_.elem_pair_off = b_.Upload(paths_.elem_pair_off, s);
      a_.pairs = b_.Upload(paths_.pairs, s);
      a_.expected = b_.Upload(paths_.expected, s);
      a_.ratio = b_.Upload(paths_.ratio, s);
      phi_in_lds_ = dev::ShapLdsBytes(a_, true) <= static_cast<size_t>(dev::kShapLdsBytes);
    }
    return true;
  }
  int NumSlots() const { return static_cast<int>(slots_.used.size()); }
  const int32_t* SlotOf() const { return slot_of_; }
  // the sorted features of the slots
  const std::vector<int32_t>& Used() const { return slots_.used; }
  // doubles of one row's output
  int64_t OutPerRow() const {
    if (kind_ == DevicePredictKind::Leaf) return f_.num_trees;
    if (kind_ == DevicePredictKind::Contrib) return static_cast<int64_t>(f_.num_class) * (a_.num_features + 1);
    return f_.num_class;
  }
  // device bytes a launch over `rows` rows allocates besides its input and output
  size_t ScratchBytes(int64_t rows) const {
    if (kind_ != DevicePredictKind::Contrib || phi_in_lds_) return 0;
    const int tiles = static_cast<int>((rows + dev::kShapLanes - 1) / dev::kShapLanes);
    return static_cast<size_t>(dev::ShapTileGrid(tiles)) * (a_.num_features + 1) * dev::kShapLanes * sizeof(double);
  }
  // rows [0, rows) of d_data (compact: column stride `rows` when column-major) into d_out
  void Run(const void* d_data, bool is_double, bool row_major, int64_t rows, int ncol, double* d_out,
           hipStream_t s) {
    dev::ForestArgs f = f_;
    f.num_cols = ncol;
    f.is_double = is_double ? 1 : 0;
    f.row_major = row_major ? 1 : 0;
    f.num_rows = rows;
    f.data = d_data;
    f.out = d_out;
    if (kind_ == DevicePredictKind::Leaf) {
      dev::PredictForestLeaf(f, s);
    } else if (kind_ == DevicePredictKind::Contrib) {
      dev::ShapArgs a = a_;
      a.num_tiles = static_cast<int32_t>((rows + dev::kShapLanes - 1) / dev::kShapLanes);
      a.out = d_out;
      if (!phi_in_lds_) {
        const size_t need = ScratchBytes(rows);
        if (need > phi_bytes_) {
          phi_tiles_ = b_.Alloc(need);
          phi_bytes_ = need;
        }
        a.phi_tiles = static_cast<double*>(phi_tiles_);
      }
      dev::ShapForest(f, a, s);
    } else {
      dev::PredictForest(f, s);
    }
    HIPCHECK(hipGetLastError());
  }

 private:
  DevicePredictKind kind_ = DevicePredictKind::Raw;
  FlatForest flat_;
  ShapPathTables paths_;
  FeatureSlots slots_;
  const int32_t* slot_of_ = nullptr;
  DeviceBuffers b_;
  dev::ForestArgs f_{};
  dev::ShapArgs a_{};
  bool phi_in_lds_ = true;
  void* phi_tiles_ = nullptr;
  size_t phi_bytes_ = 0;
};

// the scatter of CSR rows [0, rows) (indptr on the device, entry_base = its first value) into d_mat
void RunCsrToSlots(const DeviceForest& forest, const void* d_indptr, bool indptr_is_64, const int32_t* d_indices,
                   const void* d_data, bool is_double, int64_t rows, int64_t entry_base, int64_t entries,
                   int num_features, void* d_mat, hipStream_t s) {
  dev::CsrSlotsArgs c{};
  tuning::PoisonArgs(&c);  // (every field set below)
  c.indptr_is_64 = indptr_is_64 ? 1 : 0;
  c.is_double = is_double ? 1 : 0;
  c.num_features = num_features;
  c.num_slots = forest.NumSlots();
  c.num_rows = rows;
  c.entry_base = entry_base;
  c.num_entries = entries;
  c.indptr = d_indptr;
  c.indices = d_indices;
  c.data = d_data;
  c.slot_of = forest.SlotOf();
  c.out = d_mat;
  dev::CsrToSlots(c, s);
  HIPCHECK(hipGetLastError());
}

// the scatter arguments of CSC arrays on the device; `d_ascending` holds a word per slot
dev::CscSlotsArgs CscArgs(const DeviceForest& forest, const void* d_col_ptr, bool col_ptr_is_64,
                          const int32_t* d_slot_col, const int32_t* d_indices, const void* d_data, bool is_double,
                          int64_t entries, uint32_t* d_ascending) {
  dev::CscSlotsArgs c{};
  tuning::PoisonArgs(&c);  // (every field set below, the chunk by RunCscToSlots)
  c.col_ptr_is_64 = col_ptr_is_64 ? 1 : 0;
  c.is_double = is_double ? 1 : 0;
  c.num_slots = forest.NumSlots();
  c.pad = 0;
  c.num_entries = entries;
  c.row0 = 0;
  c.num_rows = 0;
  c.col_ptr = d_col_ptr;
  c.slot_col = d_slot_col;
  c.indices = d_indices;
  c.data = d_data;
  c.ascending = d_ascending;
  c.out = nullptr;
  return c;
}

// the scatter of the rows [row0, row0 + rows) into d_mat (after dev::CscColumnOrder on the stream)
void RunCscToSlots(dev::CscSlotsArgs c, int64_t row0, int64_t rows, void* d_mat, hipStream_t s) {
  c.row0 = row0;
  c.num_rows = rows;
  c.out = d_mat;
  dev::CscToSlots(c, s);
  HIPCHECK(hipGetLastError());
}

// A row source is what differs between the input layouts under GBDT::PredictChunksOnDevice:
//   kSlots       the forest walks a compact matrix of the features it splits on
//   Measure      the device bytes of the input, next to the output and the accumulator tiles
//   MostEntries  the most stored entries staged with a chunk of `rows` rows (0: none are)
//   Prepare      after the plan: allocates / uploads into `b` what lives for the whole call
//   Stage        rows [r0, r0 + rows) onto the device, on the stream: the matrix the forest walks
struct SourceBytes {
  size_t fixed, per_row, per_entry;
};
struct ChunkMatrix {
  const void* data;
  bool row_major;
  int ncol;
};

struct DenseRows {
  const void* data;
  int64_t nrow;
  int ncol;
  size_t elem;  // bytes of a value: float32 / float64
  bool row_major;
  void* d_data = nullptr;

  static constexpr bool kSlots = false;
  SourceBytes Measure(const DeviceForest&) { return {0, static_cast<size_t>(ncol) * elem, 0}; }
  int64_t MostEntries(int64_t) const { return 0; }
  void Prepare(const DeviceForest&, const PredictChunkPlan& plan, DeviceBuffers* b, hipStream_t) {
    d_data = b->Alloc(static_cast<size_t>(plan.chunk) * ncol * elem);
  }
  ChunkMatrix Stage(const DeviceForest&, int64_t r0, int64_t rows, hipStream_t s) {
    const char* src = static_cast<const char*>(data);
    if (row_major) {
      HIPCHECK(hipMemcpyAsync(d_data, src + static_cast<size_t>(r0) * ncol * elem,
                              static_cast<size_t>(rows) * ncol * elem, hipMemcpyHostToDevice, s));
    } else if (rows == nrow) {
      HIPCHECK(hipMemcpyAsync(d_data, src, static_cast<size_t>(rows) * ncol * elem, hipMemcpyHostToDevice, s));
    } else {  // the chunk's rows of every column, compacted to a column stride of `rows`
      HIPCHECK(hipMemcpy2DAsync(d_data, static_cast<size_t>(rows) * elem, src + static_cast<size_t>(r0) * elem,
                                static_cast<size_t>(nrow) * elem, static_cast<size_t>(rows) * elem, ncol,
                                hipMemcpyHostToDevice, s));
    }
    return {d_data, row_major, ncol};
  }
};

// a chunk's rows are copied by their indptr entries and scattered into the compact matrix
struct CsrRows {
  SparsePtr ptr;
  const int32_t* indices;
  const void* data;
  int64_t nrow;
  int num_features;
  size_t elem;
  void *d_indptr = nullptr, *d_data = nullptr, *d_mat = nullptr;
  int32_t* d_indices = nullptr;

  static constexpr bool kSlots = true;
  size_t PtrBytes() const { return ptr.is_64 ? 8 : 4; }
  SourceBytes Measure(const DeviceForest& f) {
    return {PtrBytes(), static_cast<size_t>(f.NumSlots()) * elem + PtrBytes(), sizeof(int32_t) + elem};
  }
  int64_t MostEntries(int64_t rows) const { return MostChunkEntries(ptr, nrow, rows); }
  void Prepare(const DeviceForest& f, const PredictChunkPlan& plan, DeviceBuffers* b, hipStream_t) {
    d_indptr = b->Alloc(static_cast<size_t>(plan.chunk + 1) * PtrBytes());
    d_indices = static_cast<int32_t*>(b->Alloc(static_cast<size_t>(plan.entries) * sizeof(int32_t)));
    d_data = b->Alloc(static_cast<size_t>(plan.entries) * elem);
    d_mat = b->Alloc(static_cast<size_t>(plan.chunk) * f.NumSlots() * elem);
  }
  ChunkMatrix Stage(const DeviceForest& f, int64_t r0, int64_t rows, hipStream_t s) {
    const int64_t e0 = ptr[r0];
    const int64_t ne = ptr[r0 + rows] - e0;
    HIPCHECK(hipMemcpyAsync(d_indptr, static_cast<const char*>(ptr.p) + static_cast<size_t>(r0) * PtrBytes(),
                            static_cast<size_t>(rows + 1) * PtrBytes(), hipMemcpyHostToDevice, s));
    if (ne > 0) {
      HIPCHECK(hipMemcpyAsync(d_indices, indices + e0, static_cast<size_t>(ne) * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
      HIPCHECK(hipMemcpyAsync(d_data, static_cast<const char*>(data) + static_cast<size_t>(e0) * elem,
                              static_cast<size_t>(ne) * elem, hipMemcpyHostToDevice, s));
    }
    RunCsrToSlots(f, d_indptr, ptr.is_64, d_indices, d_data, elem == 8, rows, e0, ne, num_features, d_mat, s);
    return {d_mat, false, f.NumSlots()};
  }
};

// the stored entries of the columns the trees split on stay on the device for the call; a chunk's
// rows are scattered from them
struct CscRows {
  SparsePtr col_ptr;
  const int32_t* indices;
  const void* data;
  int64_t ncol;
  size_t elem;
  // the stored entries of the used columns, packed slot after slot: a pointer of nslot + 1
  // entries over them, and the runs of adjacent used columns, each one copy
  std::vector<int64_t> ptr;
  std::vector<ColumnRun> runs;
  std::vector<int32_t> slot_col;
  dev::CscSlotsArgs c{};
  void* d_mat = nullptr;

  static constexpr bool kSlots = true;
  SourceBytes Measure(const DeviceForest& f) {
    const int nslot = f.NumSlots();
    PackColumnRuns(f.Used(), col_ptr, ncol, &runs, &ptr);
    return {static_cast<size_t>(ptr[nslot]) * (sizeof(int32_t) + elem) +
                (static_cast<size_t>(nslot) + 1) * (sizeof(int64_t) + 2 * sizeof(int32_t)),
            static_cast<size_t>(nslot) * elem, 0};
  }
  int64_t MostEntries(int64_t) const { return 0; }
  void Prepare(const DeviceForest& f, const PredictChunkPlan& plan, DeviceBuffers* b, hipStream_t s) {
    const int nslot = f.NumSlots();
    const int64_t entries = ptr[nslot];
    slot_col.assign(nslot, -1);
    for (int k = 0; k < nslot; ++k) {
      if (f.Used()[k] < ncol) slot_col[k] = k;  // (else a matrix narrower than the model: it reads 0)
    }
    const int64_t* d_ptr = b->Upload(ptr, s);
    const int32_t* d_slot_col = b->Upload(slot_col, s);
    int32_t* d_indices = static_cast<int32_t*>(b->Alloc(static_cast<size_t>(entries) * sizeof(int32_t)));
    char* d_data = static_cast<char*>(b->Alloc(static_cast<size_t>(entries) * elem));
    uint32_t* d_ascending = static_cast<uint32_t*>(b->Alloc(static_cast<size_t>(nslot) * sizeof(uint32_t)));
    // (every run where it lies: packing the runs on the host first, for two large copies, was
    // measured slower at 266 runs -- profiles/r12_device_csc_predict.md)
    for (const ColumnRun& r : runs) {
      HIPCHECK(hipMemcpyAsync(d_indices + r.dst, indices + r.src, static_cast<size_t>(r.len) * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
      HIPCHECK(hipMemcpyAsync(d_data + static_cast<size_t>(r.dst) * elem,
                              static_cast<const char*>(data) + static_cast<size_t>(r.src) * elem,
                              static_cast<size_t>(r.len) * elem, hipMemcpyHostToDevice, s));
    }
    c = CscArgs(f, d_ptr, true, d_slot_col, d_indices, d_data, elem == 8, entries, d_ascending);
    dev::CscColumnOrder(c, s);
    HIPCHECK(hipGetLastError());
    d_mat = b->Alloc(static_cast<size_t>(plan.chunk) * nslot * elem);
  }
  ChunkMatrix Stage(const DeviceForest&, int64_t r0, int64_t rows, hipStream_t s) {
    RunCscToSlots(c, r0, rows, d_mat, s);
    return {d_mat, false, c.num_slots};
  }
};

}  // namespace

std::vector<const Tree*> GBDT::PredictWindowTrees(int start_iteration, int num_iteration) {
  InitPredict(start_iteration, num_iteration, false);
  const int t0 = start_iteration_for_pred_ * num_tree_per_iteration_;
  const int nt = num_iteration_for_pred_ * num_tree_per_iteration_;
  std::vector<const Tree*> trees(nt);
  for (int i = 0; i < nt; ++i) trees[i] = models_[t0 + i].get();
  return trees;
}

template <typename Source>
bool GBDT::PredictChunksOnDevice(Source* src, int64_t nrow, int start_iteration, int num_iteration,
                                 DevicePredictKind kind, double* out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return false;
  if (num_tree_per_iteration_ > dev::kMaxPredClasses || nrow <= 0) return false;
  const int ntpi = num_tree_per_iteration_;
  // (the forest is rebuilt per call: trees may have been edited in place)
  const std::vector<const Tree*> trees = PredictWindowTrees(start_iteration, num_iteration);
  hipStream_t s;
  HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  bool ran = false;
  {
    DeviceForest forest;
    if (forest.Upload(trees, ntpi, max_feature_idx_ + 1, kind, s, Source::kSlots)) {
      const int64_t per_out = forest.OutPerRow();
      const SourceBytes in = src->Measure(forest);
      // rows per chunk (predict_chunks.h): input, output and the accumulator tiles within most of
      // the free memory
      size_t free_b = 0, total_b = 0;
      HIPCHECK(hipMemGetInfo(&free_b, &total_b));
      const PredictChunkPlan plan = PlanPredictChunks(
          nrow, free_b - free_b / 5, forest.ScratchBytes(nrow) + in.fixed,
          in.per_row + static_cast<size_t>(per_out) * sizeof(double), in.per_entry,
          tuning::Int(tuning::Knob::PredictChunkRows, 0), dev::kShapLanes,
          [&](int64_t rows) { return src->MostEntries(rows); });
      if (plan.fits) {
        DeviceBuffers b;
        src->Prepare(forest, plan, &b, s);
        double* d_out = static_cast<double*>(b.Alloc(static_cast<size_t>(plan.chunk) * per_out * sizeof(double)));
        const bool convert = kind == DevicePredictKind::Normal;
        std::vector<double> raw_out(convert ? static_cast<size_t>(nrow) * per_out : 0);
        double* host_out = convert ? raw_out.data() : out;
        for (int64_t r0 = 0; r0 < nrow; r0 += plan.chunk) {
          const int64_t rows = std::min(plan.chunk, nrow - r0);
          const ChunkMatrix m = src->Stage(forest, r0, rows, s);
          forest.Run(m.data, src->elem == 8, m.row_major, rows, m.ncol, d_out, s);
          HIPCHECK(hipMemcpyAsync(host_out + r0 * per_out, d_out, static_cast<size_t>(rows) * per_out * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
          HIPCHECK(hipStreamSynchronize(s));
        }
        ran = true;
        ++g_device_predictions;
        if (convert) {
#pragma omp parallel for schedule(static)
          for (int64_t r = 0; r < nrow; ++r) {
            double* o = out + r * ntpi;
            std::memcpy(o, raw_out.data() + r * ntpi, sizeof(double) * ntpi);
            if (average_output_) {
              for (int k = 0; k < ntpi; ++k) o[k] /= num_iteration_for_pred_;
            }
            if (objective_ != nullptr) objective_->ConvertOutput(o, o);
          }
        }
      }
    }
  }
  HIPCHECK(hipStreamDestroy(s));
  return ran;
}

template <typename Forest>
void GBDT::UploadForDeviceBuffers(Forest* forest, DevicePredictKind kind, bool slots, int64_t nrow, int64_t out_len,
                                  int start_iteration, int num_iteration) {
  if (kind == DevicePredictKind::Normal) Log::Fatal("device buffers are predicted as raw scores, leaf indices or contributions");
  if (num_tree_per_iteration_ > dev::kMaxPredClasses) {
    Log::Fatal("forest prediction on the device handles at most %d trees per iteration", dev::kMaxPredClasses);
  }
  const std::vector<const Tree*> trees = PredictWindowTrees(start_iteration, num_iteration);
  if (!forest->Upload(trees, num_tree_per_iteration_, max_feature_idx_ + 1, kind, nullptr, slots)) {
    Log::Fatal("contributions on the device need paths of at most %d distinct features and data counts on every node",
               dev::kShapMaxPathLen - 1);
  }
  if (out_len != nrow * forest->OutPerRow()) {
    Log::Fatal("output holds %lld doubles, the prediction has %lld", static_cast<long long>(out_len),
               static_cast<long long>(nrow * forest->OutPerRow()));
  }
}

bool GBDT::PredictDenseOnDevice(const void* data, bool is_double, int64_t nrow, int ncol, bool row_major,
                                int start_iteration, int num_iteration, DevicePredictKind kind, double* out) {
  // (a matrix narrower than the model, let through by predict_disable_shape_check: the kernels index
  // a row by the model's features, and the host predictor reads the absent columns as 0)
  if (ncol <= max_feature_idx_) return false;
  DenseRows src{data, nrow, ncol, is_double ? 8u : 4u, row_major};
  return PredictChunksOnDevice(&src, nrow, start_iteration, num_iteration, kind, out);
}

void GBDT::PredictDeviceBuffers(const void* d_data, bool is_double, int64_t nrow, int ncol, int start_iteration,
                                int num_iteration, DevicePredictKind kind, double* d_out, int64_t out_len) {
  if (ncol != max_feature_idx_ + 1) {
    Log::Fatal("The number of features in data (%d) is not the same as it was in training data (%d).", ncol,
               max_feature_idx_ + 1);
  }
  DeviceForest forest;
  UploadForDeviceBuffers(&forest, kind, false, nrow, out_len, start_iteration, num_iteration);
  if (nrow > 0) forest.Run(d_data, is_double, true, nrow, ncol, d_out, nullptr);
  HIPCHECK(hipStreamSynchronize(nullptr));
  ++g_device_predictions;
}

bool GBDT::PredictCSROnDevice(const void* indptr, bool indptr_is_64, const int32_t* indices, const void* data,
                              bool is_double, int64_t nindptr, int64_t nelem, int start_iteration, int num_iteration,
                              DevicePredictKind kind, double* out) {
  const int64_t nrow = nindptr - 1;
  // (rows are copied by their indptr entries: a matrix whose indptr does not ascend within the
  // stored entries is left to the host)
  const SparsePtr ptr{indptr, indptr_is_64};
  if (nrow <= 0 || !PointerValid(ptr, nrow, nelem)) return false;
  CsrRows src{ptr, indices, data, nrow, max_feature_idx_ + 1, is_double ? 8u : 4u};
  return PredictChunksOnDevice(&src, nrow, start_iteration, num_iteration, kind, out);
}

void GBDT::PredictCSRDeviceBuffers(const void* d_indptr, bool indptr_is_64, const int32_t* d_indices,
                                   const void* d_data, bool is_double, int64_t nrow, int64_t nelem,
                                   int start_iteration, int num_iteration, DevicePredictKind kind, double* d_out,
                                   int64_t out_len) {
  if (nrow < 0 || nelem < 0) Log::Fatal("CSR device buffers: %lld rows, %lld entries", static_cast<long long>(nrow), static_cast<long long>(nelem));
  DeviceForest forest;
  UploadForDeviceBuffers(&forest, kind, true, nrow, out_len, start_iteration, num_iteration);
  if (nrow > 0) {
    DeviceBuffers b;
    void* d_mat = b.Alloc(static_cast<size_t>(nrow) * forest.NumSlots() * (is_double ? 8 : 4));
    // (the rows are clamped to nelem entries in the kernel: indptr stays on the device)
    RunCsrToSlots(forest, d_indptr, indptr_is_64, d_indices, d_data, is_double, nrow, 0, nelem, max_feature_idx_ + 1,
                  d_mat, nullptr);
    forest.Run(d_mat, is_double, false, nrow, forest.NumSlots(), d_out, nullptr);
    HIPCHECK(hipStreamSynchronize(nullptr));
  }
  ++g_device_predictions;
}

bool GBDT::PredictCSCOnDevice(const void* col_ptr, bool col_ptr_is_64, const int32_t* indices, const void* data,
                              bool is_double, int64_t ncol_ptr, int64_t nelem, int64_t num_row, int start_iteration,
                              int num_iteration, DevicePredictKind kind, double* out) {
  const int64_t ncol = ncol_ptr - 1;
  if (num_row <= 0 || ncol < 0 || nelem < 0) return false;
  // (columns are copied by their pointer entries: a matrix whose pointer does not ascend within
  // the stored entries is left to the host)
  const SparsePtr ptr{col_ptr, col_ptr_is_64};
  if (!PointerValid(ptr, ncol, nelem)) return false;
  CscRows src{ptr, indices, data, ncol, is_double ? 8u : 4u};
  return PredictChunksOnDevice(&src, num_row, start_iteration, num_iteration, kind, out);
}

void GBDT::PredictCSCDeviceBuffers(const void* d_col_ptr, bool col_ptr_is_64, const int32_t* d_indices,
                                   const void* d_data, bool is_double, int64_t ncol, int64_t nelem, int64_t nrow,
                                   int start_iteration, int num_iteration, DevicePredictKind kind, double* d_out,
                                   int64_t out_len) {
  if (nrow < 0 || nelem < 0 || ncol < 0) {
    Log::Fatal("CSC device buffers: %lld rows, %lld columns, %lld entries", static_cast<long long>(nrow),
               static_cast<long long>(ncol), static_cast<long long>(nelem));
  }
  DeviceForest forest;
  UploadForDeviceBuffers(&forest, kind, true, nrow, out_len, start_iteration, num_iteration);
  if (nrow > 0) {
    const int nslot = forest.NumSlots();
    // (the full pointer stays on the device: a slot names its feature's column, if the matrix has it)
    std::vector<int32_t> slot_col(nslot, -1);
    for (int k = 0; k < nslot; ++k) {
      if (forest.Used()[k] < ncol) slot_col[k] = forest.Used()[k];
    }
    DeviceBuffers b;
    const int32_t* d_slot_col = b.Upload(slot_col, nullptr);
    uint32_t* d_ascending = static_cast<uint32_t*>(b.Alloc(static_cast<size_t>(nslot) * sizeof(uint32_t)));
    void* d_mat = b.Alloc(static_cast<size_t>(nrow) * nslot * (is_double ? 8 : 4));
    const dev::CscSlotsArgs c = CscArgs(forest, d_col_ptr, col_ptr_is_64, d_slot_col, d_indices, d_data, is_double,
                                        nelem, d_ascending);
    dev::CscColumnOrder(c, nullptr);
    HIPCHECK(hipGetLastError());
    RunCscToSlots(c, 0, nrow, d_mat, nullptr);
    forest.Run(d_mat, is_double, false, nrow, nslot, d_out, nullptr);
    HIPCHECK(hipStreamSynchronize(nullptr));
  }
  ++g_device_predictions;
}

void GBDT::CsrToSlotsOnHost(const void* indptr, bool indptr_is_64, const int32_t* indices, const void* data,
                            bool is_double, int64_t nindptr, int64_t nelem, int start_iteration, int num_iteration,
                            int32_t* num_used, int32_t* used, void* matrix) {
  const std::vector<const Tree*> trees = PredictWindowTrees(start_iteration, num_iteration);
  FlatForest flat;
  flat.Build(trees);
  FeatureSlots slots;
  const int nf = max_feature_idx_ + 1;
  slots.Build(flat, nf);
  const int ns = static_cast<int>(slots.used.size());
  *num_used = ns;
  if (used != nullptr) std::copy(slots.used.begin(), slots.used.end(), used);
  if (matrix == nullptr || nindptr <= 1) return;
  const int64_t rows = nindptr - 1;
  const int32_t* so = slots.slot_of.data();
  DispatchSparse(indptr_is_64, is_double, indptr, data, [&](auto* ptr, auto* val) {
    using T = std::decay_t<decltype(*val)>;
    dev::EvalCsrToSlots(ptr, 0, indices, val, rows, nelem, so, nf, ns, static_cast<T*>(matrix));
  });
}

void GBDT::CscToSlotsOnHost(const void* col_ptr, bool col_ptr_is_64, const int32_t* indices, const void* data,
                            bool is_double, int64_t ncol_ptr, int64_t nelem, int64_t row0, int64_t rows,
                            int start_iteration, int num_iteration, int32_t* num_used, int32_t* used, void* matrix) {
  const std::vector<const Tree*> trees = PredictWindowTrees(start_iteration, num_iteration);
  FlatForest flat;
  flat.Build(trees);
  FeatureSlots slots;
  slots.Build(flat, max_feature_idx_ + 1);
  const int ns = static_cast<int>(slots.used.size());
  *num_used = ns;
  if (used != nullptr) std::copy(slots.used.begin(), slots.used.end(), used);
  if (matrix == nullptr || rows <= 0) return;
  std::vector<int32_t> slot_col(ns, -1);
  for (int k = 0; k < ns; ++k) {
    if (slots.used[k] < ncol_ptr - 1) slot_col[k] = slots.used[k];
  }
  const int32_t* sc = slot_col.data();
  DispatchSparse(col_ptr_is_64, is_double, col_ptr, data, [&](auto* ptr, auto* val) {
    using T = std::decay_t<decltype(*val)>;
    dev::EvalCscToSlots(ptr, sc, indices, val, nelem, row0, rows, ns, static_cast<T*>(matrix));
  });
}

int64_t GBDT::DevicePredictions() { return g_device_predictions.load(); }

void GBDT::ContribFromPathTables(const double* data, int64_t nrow, int ncol, int start_iteration, int num_iteration,
                                 double* out) {
  if (ncol != max_feature_idx_ + 1) Log::Fatal("path tables: %d columns, the model has %d", ncol, max_feature_idx_ + 1);
  const std::vector<const Tree*> trees = PredictWindowTrees(start_iteration, num_iteration);
  FlatForest flat;
  flat.Build(trees);
  ShapPathTables paths;
  if (!paths.Build(trees)) Log::Fatal("path tables: a node on a path has data_count 0");
  dev::ForestArgs f{};
  flat.HostArgs(&f);
  f.num_class = num_tree_per_iteration_;
  f.num_cols = ncol;
  f.is_double = 1;
  f.row_major = 1;
  f.num_rows = nrow;
  f.data = data;
  dev::ShapArgs a{};
  paths.HostArgs(&a);
  a.num_features = max_feature_idx_ + 1;
  EvalPathTables(f, a, out);
}

}  // namespace lgbm_amd
