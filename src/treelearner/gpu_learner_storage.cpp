// MI355X tree learner: the binned rows built on the device (src/device/storage_kernels.hip).
// Each group column of the Dataset crosses to the device once, into the column image (the
// learner's column copy where that is kept, a temporary window of rows where it is not); the row
// words and the row-sparse lists are made from the image by kernels.  The buffers are byte for
// byte those of the host branch (RowMajorBins, the column loop of UploadData, UploadSparseRows).
#include <atomic>

#include "../device/storage_build.h"
#include "../device/storage_plan.h"
#include "gpu_learner_internal.h"

namespace lgbm_amd {

namespace {
std::atomic<int64_t> g_device_builds{0}, g_host_builds{0};

struct Scratch {  // device memory of one build, freed when it ends
  std::vector<void*> ptrs;
  void* Get(size_t bytes) {
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>(1, bytes)));
    ptrs.push_back(p);
    return p;
  }
  ~Scratch() {
    for (void* p : ptrs) (void)hipFree(p);
  }
};
}  // namespace

void DeviceStorageStats(int64_t* device_builds, int64_t* host_builds) {
  *device_builds = g_device_builds.load();
  *host_builds = g_host_builds.load();
}

void GPUTreeLearner::CountStorageBuild(bool on_device) { (on_device ? g_device_builds : g_host_builds) += 1; }

// LGBM_AMD_DEVICE_STORAGE=0/1 forces the branch; unset, the device branch builds datasets of at
// least tuning::kDeviceStorageMinCells cells (rows x groups)
bool GPUTreeLearner::UseDeviceStorage(const Dataset* d) const {
  if (const char* e = tuning::Get(tuning::Knob::DeviceStorage)) return e[0] == '1';
  return static_cast<int64_t>(d->num_data()) * d->num_groups() >= tuning::kDeviceStorageMinCells;
}

// the column image of d's rows (col_image: the kept image, rows x column bytes; null: a window
// of rows at a time) and, with row_image, its rows as row_words 32-bit words each
void GPUTreeLearner::BuildDeviceStorage(const Dataset* d, int row_words, uint8_t* col_image, uint8_t* row_image) {
  const int64_t n = d->num_data();
  const int ng = d->num_groups();
  if (n <= 0) return;
  std::vector<int64_t> prefix(ng + 1, 0);
  for (int g = 0; g < ng; ++g) prefix[g + 1] = prefix[g] + (h_gwide_[g] ? 2 : 1);
  const int64_t row_bytes = row_image != nullptr ? 4 * static_cast<int64_t>(row_words) : 0;
  size_t free_now = 0, total = 0;
  HIPCHECK(hipMemGetInfo(&free_now, &total));
  // (the plan counts from the memory that was free before the images were allocated)
  int64_t free_before = static_cast<int64_t>(free_now) + n * row_bytes + (col_image != nullptr ? n * prefix[ng] : 0);
  if (const char* e = tuning::Get(tuning::Knob::StorageBudget)) free_before = std::atoll(e);
  const StoragePlan plan = PlanStorage(n, prefix[ng], row_bytes, free_before, col_image != nullptr ? 1 : 0);
  Scratch scratch;
  uint8_t* staging = static_cast<uint8_t*>(scratch.Get(static_cast<size_t>(plan.staging_bytes)));
  uint8_t* image = col_image != nullptr ? col_image : static_cast<uint8_t*>(scratch.Get(static_cast<size_t>(plan.window_bytes)));
  const int64_t stride = col_image != nullptr ? n : plan.window_stride;
  std::vector<int64_t> col_off(std::max(1, ng), 0);
  for (int g = 0; g < ng; ++g) col_off[g] = stride * prefix[g];
  int64_t* d_col_off = static_cast<int64_t*>(scratch.Get(sizeof(int64_t) * col_off.size()));
  HIPCHECK(hipMemcpy(d_col_off, col_off.data(), sizeof(int64_t) * col_off.size(), hipMemcpyHostToDevice));
  int8_t* d_gwide = static_cast<int8_t*>(scratch.Get(std::max(1, ng)));
  if (ng > 0) HIPCHECK(hipMemcpy(d_gwide, h_gwide_.data(), ng, hipMemcpyHostToDevice));
  const hipStream_t s = nullptr;  // (the copies below are ordered with the kernels on the null stream)
  for (int64_t r0 = 0; r0 < n; r0 += plan.window_rows) {
    const int64_t rows = std::min(plan.window_rows, n - r0);
    for (int g = 0; g < ng; ++g) {
      const FeatureGroup& grp = d->group(g);
      const int wide = h_gwide_[g], width = wide ? 2 : 1;
      uint8_t* dst = image + col_off[g];
      if (grp.sparse) {  // (zeroed column: the window's stored rows only)
        HIPCHECK(hipMemsetAsync(dst, 0, static_cast<size_t>(rows * width), s));
        const size_t k0 = static_cast<size_t>(std::lower_bound(grp.sp_rows.begin(), grp.sp_rows.end(), r0) - grp.sp_rows.begin());
        const size_t k1 = static_cast<size_t>(std::lower_bound(grp.sp_rows.begin(), grp.sp_rows.end(), r0 + rows) - grp.sp_rows.begin());
        // staged: a chunk's rows (int32), then its values
        const size_t chunk = std::max<size_t>(1, static_cast<size_t>(plan.staging_bytes) / (4 + grp.bin_bytes) / 4 * 4);
        for (size_t k = k0; k < k1; k += chunk) {
          const size_t m = std::min(chunk, k1 - k);
          HIPCHECK(hipMemcpy(staging, grp.sp_rows.data() + k, 4 * m, hipMemcpyHostToDevice));
          HIPCHECK(hipMemcpy(staging + 4 * chunk, grp.data.data() + k * grp.bin_bytes, m * grp.bin_bytes, hipMemcpyHostToDevice));
          dev::StorageScatterSparse(reinterpret_cast<const int32_t*>(staging), staging + 4 * chunk, grp.bin_bytes,
                                    static_cast<int64_t>(m), r0, rows, dst, wide, s);
        }
      } else if (grp.bin_bytes == width) {  // (already at the image's width: straight into place)
        HIPCHECK(hipMemcpy(dst, grp.data.data() + static_cast<size_t>(r0) * width, static_cast<size_t>(rows) * width,
                           hipMemcpyHostToDevice));
      } else {
        const int64_t chunk = std::max<int64_t>(1, plan.staging_bytes / grp.bin_bytes);
        for (int64_t c0 = 0; c0 < rows; c0 += chunk) {
          const int64_t m = std::min(chunk, rows - c0);
          HIPCHECK(hipMemcpy(staging, grp.data.data() + static_cast<size_t>(r0 + c0) * grp.bin_bytes,
                             static_cast<size_t>(m) * grp.bin_bytes, hipMemcpyHostToDevice));
          dev::StorageConvertColumn(staging, grp.bin_bytes, dst + c0 * width, wide, m, s);
        }
      }
    }
    if (row_image != nullptr) {
      const dev::StorageColumns cols{image, d_col_off, d_gwide, ng, rows};
      const dev::StorageRowLayout layout{d_word_g0_, d_word_wide_, args_.words_per_row, row_words, nibbles_ ? 1 : 0};
      dev::StoragePackRows(cols, layout, reinterpret_cast<uint32_t*>(row_image + r0 * row_bytes), s);
    }
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipStreamSynchronize(s));
}

// the row-sparse lists of the training rows from the kept column image (UploadSparseRows on the
// host): counts, their device-wide scan into sp_ptr, the fill in ascending group order
void GPUTreeLearner::BuildDeviceSparseRows() {
  const int64_t n = num_data_;
  Scratch scratch;
  int64_t* d_col_off = static_cast<int64_t*>(scratch.Get(sizeof(int64_t) * std::max(1, num_groups_)));
  int8_t* d_gwide = static_cast<int8_t*>(scratch.Get(std::max(1, num_groups_)));
  if (num_groups_ > 0) {
    HIPCHECK(hipMemcpy(d_col_off, h_col_off_.data(), sizeof(int64_t) * num_groups_, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_gwide, h_gwide_.data(), num_groups_, hipMemcpyHostToDevice));
  }
  std::vector<int32_t> goff(std::max(1, num_groups_), 0);
  for (int g = 0; g < num_groups_; ++g) goff[g] = static_cast<int32_t>(data_->group_bin_boundary(g));
  int32_t* d_goff = static_cast<int32_t*>(scratch.Get(sizeof(int32_t) * goff.size()));
  HIPCHECK(hipMemcpy(d_goff, goff.data(), sizeof(int32_t) * goff.size(), hipMemcpyHostToDevice));
  int64_t* d_sums = static_cast<int64_t*>(scratch.Get(sizeof(int64_t) * static_cast<size_t>(dev::StorageScanBlocks(n))));
  const dev::StorageColumns cols{d_bins_col_, d_col_off, d_gwide, num_groups_, n};
  d_sp_ptr_ = Alloc<int64_t>(static_cast<size_t>(n) + 1);
  dev::StorageStoredPointers(cols, d_sp_ptr_, d_sums, nullptr);
  HIPCHECK(hipGetLastError());
  int64_t stored = 0;
  HIPCHECK(hipMemcpy(&stored, d_sp_ptr_ + n, sizeof(int64_t), hipMemcpyDeviceToHost));
  d_sp_bin_ = Alloc<uint16_t>(static_cast<size_t>(std::max<int64_t>(1, stored)));
  dev::StorageFillStored(cols, d_goff, d_sp_ptr_, d_sp_bin_, nullptr);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(nullptr));
  SetSparseTeam(static_cast<double>(stored) / std::max<int64_t>(1, n));
}

// threads per row: a row of mean length fits the kSparsePer entries each thread loads up front
void GPUTreeLearner::SetSparseTeam(double mean) {
  sp_team_ = 4;
  while (sp_team_ < 64 && sp_team_ * dev::kSparsePerThread < mean) sp_team_ *= 2;
  Log::Info("device learner: row-sparse storage, %.2f stored bins per row (%d groups), %d threads per row", mean,
            num_groups_, sp_team_);
}

// test support: a copy of one storage buffer.  which 0: the row image, 1: the column image,
// 2: sp_ptr, 3: sp_bin, 4: the layout record (int64: row_words, groups, rows, row-sparse, then
// per group its byte in a row, width code 0 8-bit / 1 16-bit / 2 4-bit, nibble half, column offset)
bool GPUTreeLearner::DebugStorage(int data_idx, int which, std::vector<uint8_t>* out) {
  HIPCHECK(hipSetDevice(device_id_));
  HIPCHECK(hipDeviceSynchronize());
  out->clear();
  const void* src = nullptr;
  size_t bytes = 0;
  int64_t rows = num_data_;
  int row_words = args_.row_words;
  if (data_idx > 0) {
    const ValidSet* vs = nullptr;
    int seen = 0;
    for (const ValidSet& v : valid_) {
      if (v.bins != nullptr && ++seen == data_idx) vs = &v;
    }
    if (vs == nullptr) return false;
    rows = vs->num_data;
    row_words = args_.words_per_row;
    if (which == 0) src = vs->bins, bytes = static_cast<size_t>(rows) * row_words * 4;
  } else if (which == 0 && d_bins_ != nullptr) {
    src = d_bins_, bytes = static_cast<size_t>(rows) * row_words * 4;
  } else if (which == 1 && d_bins_col_ != nullptr) {
    src = d_bins_col_, bytes = static_cast<size_t>(h_col_off_[num_groups_]);
  } else if (which == 2 && d_sp_ptr_ != nullptr) {
    src = d_sp_ptr_, bytes = sizeof(int64_t) * (static_cast<size_t>(rows) + 1);
  } else if (which == 3 && d_sp_ptr_ != nullptr) {
    int64_t stored = 0;
    HIPCHECK(hipMemcpy(&stored, d_sp_ptr_ + rows, sizeof(int64_t), hipMemcpyDeviceToHost));
    src = d_sp_bin_, bytes = sizeof(uint16_t) * static_cast<size_t>(stored);
  }
  if (which == 4) {
    std::vector<int64_t> rec = {row_words, num_groups_, rows, data_idx == 0 && sparse_rows_ ? 1 : 0};
    int64_t col_off = 0;
    for (int g = 0; g < num_groups_; ++g) {
      rec.push_back(h_gbyte_[g]);
      rec.push_back(h_gnib_[g] != 0 ? 2 : h_gwide_[g]);
      rec.push_back(h_gnib_[g] != 0 ? (h_gnib_[g] & 1) : 0);
      rec.push_back(col_off);
      col_off += rows * (h_gwide_[g] ? 2 : 1);
    }
    out->resize(rec.size() * sizeof(int64_t));
    std::memcpy(out->data(), rec.data(), out->size());
    return true;
  }
  out->resize(bytes);
  if (bytes > 0) HIPCHECK(hipMemcpy(out->data(), src, bytes, hipMemcpyDeviceToHost));
  return true;
}

}  // namespace lgbm_amd
