// The device half of the bin finder's first step (src/device/bin_find_kernels.hip): the distinct
// values of every column of a bin sample that lies in device memory, by the rule of
// src/device/sample_distinct.h.  Used by SampleDeviceTensor (src/device/tensor_bin_kernels.hip).
#pragma once

#include <cstdint>

#include "lgbm_amd/bin.h"

namespace lgbm_amd {

// Scratch for passes of at most max_cols columns of ns samples on the current device, and the two
// steps of a pass on its null stream.  Beside the sample's 8 bytes it holds kBinFindScratchBytes
// per sample (the second key buffer and the run lengths).
constexpr int64_t kBinFindScratchBytes = 12;

class DeviceSampleDistinct {
 public:
  DeviceSampleDistinct(int max_cols, int ns);
  ~DeviceSampleDistinct();
  DeviceSampleDistinct(const DeviceSampleDistinct&) = delete;
  DeviceSampleDistinct& operator=(const DeviceSampleDistinct&) = delete;

  // sorts the column-major sample d_vals[nc][ns] (k_gather_sample's output: overwritten) and forms
  // its runs; returns once the kernel is enqueued
  void Launch(double* d_vals, int nc);
  // waits for it and appends the nc columns' lists to *out
  void Collect(SampleDistinctLists* out);

 private:
  int max_cols_, ns_, nc_ = 0;
  double* d_vals_ = nullptr;
  uint64_t* d_alt_ = nullptr;     // [max_cols][ns] the other key buffer
  int32_t* d_counts_ = nullptr;   // [max_cols][ns] run lengths
  int32_t* d_hdr_ = nullptr;      // [max_cols][5] runs, NaNs, values kept, where the run values lie, passes run
  long long* d_off_ = nullptr;    // [max_cols] first run of each column in the packed lists
  double* d_pack_d_ = nullptr;
  int32_t* d_pack_c_ = nullptr;
  int64_t pack_cap_ = 0;
};

}  // namespace lgbm_amd
