// MI355X learner: refit of an existing forest's leaf values from the leaf matrix
// (GBDT::RefitTree; kernels in src/device/refit_kernels.hip).  The matrix is staged tree-major
// in windows of columns; per tree, one pass sums (g, h, count) per leaf over the tree's column
// and one adds the new leaf values to the training scores.  Nothing here reads the binned data.
#include "gpu_learner_internal.h"

#include "../device/refit_quant.h"
#include "lgbm_amd/tuning.h"

namespace lgbm_amd {

namespace {
constexpr size_t kRefitChunkBytes = size_t(64) << 20;  // rows of the window uploaded per staging launch

template <typename T>
T* RefitAlloc(size_t n) {
  void* p = nullptr;
  HIPCHECK(hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)));
  return static_cast<T*>(p);
}
}  // namespace

void GPUTreeLearner::RefitRelease() {
  RefitState& r = refit_;
  for (void* p : {r.staged, static_cast<void*>(r.chunk), static_cast<void*>(r.num_leaves), static_cast<void*>(r.flags),
                  static_cast<void*>(r.table), static_cast<void*>(r.values)}) {
    if (p != nullptr) (void)hipFree(p);
  }
  r = RefitState();
}

bool GPUTreeLearner::RefitStageWindow(const int32_t* leaf, int64_t nrow, int ncol, int col0, const int* num_leaves,
                                      int trees_per_iteration, int* cols_staged) {
  if (distributed_) return false;
  HIPCHECK(hipSetDevice(device_id_));
  HIPCHECK(hipStreamSynchronize(stream_));  // (nothing still reads the last window)
  RefitRelease();
  if (leaf == nullptr) return true;
  if (nrow != num_data_ || d_score_ == nullptr || col0 < 0 || col0 >= ncol || trees_per_iteration <= 0) return false;
  RefitState& r = refit_;
  const int left = ncol - col0;
  int max_leaves = 1;
  for (int c = col0; c < ncol; ++c) max_leaves = std::max(max_leaves, num_leaves[c]);
  // the width of the staged ids follows the remaining trees (so every window of a refit has the
  // same one); LGBM_AMD_REFIT_WIDE=1 forces int32
  r.wide = max_leaves > 65536 || tuning::On(tuning::Knob::RefitWide);
  const size_t elem = r.wide ? sizeof(int32_t) : sizeof(uint16_t);
  // columns per window: the staged columns and one upload chunk within most of the free memory
  // (as the device prediction sizes its row chunks), whole iterations
  int cols = 0;
  const int forced = tuning::Int(tuning::Knob::RefitWindow, 0);
  if (forced > 0) {
    cols = static_cast<int>(std::min<int64_t>(left, static_cast<int64_t>(forced) * trees_per_iteration));
  } else {
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = free_b - free_b / 5;
    const size_t fixed = kRefitChunkBytes + (size_t(4) << 20);
    const size_t per_col = static_cast<size_t>(nrow) * elem;
    const int64_t fit = budget > fixed ? static_cast<int64_t>((budget - fixed) / per_col) : 0;
    cols = static_cast<int>(std::min<int64_t>(left, fit / trees_per_iteration * trees_per_iteration));
    if (cols <= 0) {
      Log::Fatal("device refit: no room for the leaf columns of one iteration (%lld rows, %zu bytes free)",
                 static_cast<long long>(nrow), free_b);
    }
  }
  r.nrow = nrow;
  r.col0 = col0;
  r.cols = cols;
  const int64_t chunk_rows =
      std::max<int64_t>(dev::kRefitTile, std::min<int64_t>(nrow, static_cast<int64_t>(kRefitChunkBytes / (sizeof(int32_t) * cols))));
  r.staged = RefitAlloc<char>(static_cast<size_t>(cols) * nrow * elem);
  r.chunk = RefitAlloc<int32_t>(static_cast<size_t>(chunk_rows) * cols);
  r.num_leaves = RefitAlloc<int32_t>(cols);
  r.flags = RefitAlloc<uint32_t>(4);
  std::vector<int32_t> nl(num_leaves + col0, num_leaves + col0 + cols);
  HIPCHECK(hipMemcpyAsync(r.num_leaves, nl.data(), sizeof(int32_t) * cols, hipMemcpyHostToDevice, stream_));
  const uint32_t flags0[4] = {0u, 0xffffffffu, 0u, 0u};
  HIPCHECK(hipMemcpyAsync(r.flags, flags0, sizeof(flags0), hipMemcpyHostToDevice, stream_));
  for (int64_t r0 = 0; r0 < nrow; r0 += chunk_rows) {
    const int64_t rows = std::min(chunk_rows, nrow - r0);
    HIPCHECK(hipMemcpy2DAsync(r.chunk, sizeof(int32_t) * cols, leaf + static_cast<size_t>(r0) * ncol + col0,
                              sizeof(int32_t) * ncol, sizeof(int32_t) * cols, static_cast<size_t>(rows),
                              hipMemcpyHostToDevice, stream_));
    dev::RefitStageArgs a{};
    tuning::PoisonArgs(&a);  // (every field set below)
    a.src = r.chunk;
    a.src_stride = cols;
    a.rows = rows;
    a.row0 = r0;
    a.num_rows = nrow;
    a.cols = cols;
    a.wide = r.wide ? 1 : 0;
    a.num_leaves = r.num_leaves;
    a.out = r.staged;
    a.bad = r.flags;
    dev::RefitStage(a, stream_);
    HIPCHECK(hipGetLastError());
  }
  uint32_t bad[2] = {0u, 0u};
  HIPCHECK(hipMemcpyAsync(bad, r.flags, sizeof(bad), hipMemcpyDeviceToHost, stream_));
  HIPCHECK(hipStreamSynchronize(stream_));
  if (bad[0] != 0u) {
    const int tree = col0 + static_cast<int>(bad[1]);
    RefitRelease();
    Log::Fatal("refit: %u entries of the leaf matrix are outside their tree; the first such tree is tree %d (%d leaves)",
               bad[0], tree, num_leaves[tree]);
  }
  *cols_staged = cols;
  return true;
}

const void* GPUTreeLearner::RefitColumn(int col) const {
  const RefitState& r = refit_;
  if (r.staged == nullptr || col < r.col0 || col >= r.col0 + r.cols) {
    Log::Fatal("device refit: tree %d is not in the staged window [%d, %d)", col, r.col0, r.col0 + r.cols);
  }
  const size_t elem = r.wide ? sizeof(int32_t) : sizeof(uint16_t);
  return static_cast<const char*>(r.staged) + static_cast<size_t>(col - r.col0) * r.nrow * elem;
}

bool GPUTreeLearner::RefitLeafSums(int col, int tree_id, int num_leaves, double* sum_g, double* sum_h,
                                   data_size_t* count, int* scale_exp) {
  if (distributed_ || refit_.staged == nullptr || num_leaves <= 0) return false;
  RefitState& r = refit_;
  const void* column = RefitColumn(col);
  MaterializeSplitGradients();  // (gradients the fused kernel left packed)
  if (r.table_leaves < num_leaves) {
    if (r.table != nullptr) HIPCHECK(hipFree(r.table));
    if (r.values != nullptr) HIPCHECK(hipFree(r.values));
    r.table = RefitAlloc<long long>(3 * static_cast<size_t>(num_leaves) + 2);
    r.values = RefitAlloc<double>(num_leaves);
    r.table_leaves = num_leaves;
  }
  const size_t off = static_cast<size_t>(tree_id) * num_data_;
  dev::RefitSumArgs a{};
  tuning::PoisonArgs(&a);  // (every field set below)
  a.leaf = column;
  a.wide = r.wide ? 1 : 0;
  a.num_leaves = num_leaves;
  a.n = num_data_;
  a.grad = d_grad_ + off;
  a.hess = d_hess_ + off;
  a.absmax = r.flags + 2;
  a.table = r.table;
  dev::RefitLeafSums(a, stream_);
  HIPCHECK(hipGetLastError());
  const size_t words = 3 * static_cast<size_t>(num_leaves) + 2;
  r.host_table.resize(words);
  HIPCHECK(hipMemcpyAsync(r.host_table.data(), r.table, sizeof(long long) * words, hipMemcpyDeviceToHost, stream_));
  HIPCHECK(hipStreamSynchronize(stream_));
  const long long* t = r.host_table.data();
  const int eg = static_cast<int>(t[3 * num_leaves]), eh = static_cast<int>(t[3 * num_leaves + 1]);
  const double ig = dev::RefitScale(-eg), ih = dev::RefitScale(-eh);
  for (int l = 0; l < num_leaves; ++l) {
    sum_g[l] = static_cast<double>(t[l]) * ig;  // (|sums| < 2^53: exact)
    sum_h[l] = static_cast<double>(t[num_leaves + l]) * ih;
    count[l] = static_cast<data_size_t>(t[2 * num_leaves + l]);
  }
  scale_exp[0] = eg;
  scale_exp[1] = eh;
  return true;
}

bool GPUTreeLearner::RefitAddLeafValues(int col, int tree_id, const double* values, int num_leaves) {
  if (distributed_ || refit_.staged == nullptr || num_leaves <= 0 || refit_.table_leaves < num_leaves) return false;
  RefitState& r = refit_;
  grad_prefetched_ = false;  // (the scores change)
  HIPCHECK(hipMemcpyAsync(r.values, values, sizeof(double) * num_leaves, hipMemcpyHostToDevice, stream_));
  dev::RefitAddArgs a{};
  tuning::PoisonArgs(&a);  // (every field set below)
  a.leaf = RefitColumn(col);
  a.wide = r.wide ? 1 : 0;
  a.num_leaves = num_leaves;
  a.n = num_data_;
  a.values = r.values;
  a.score = d_score_ + static_cast<size_t>(tree_id) * num_data_;
  dev::RefitAddLeafValues(a, stream_);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(stream_));  // (`values` is the caller's)
  return true;
}

}  // namespace lgbm_amd
