// Value -> bin mapping of dense, CSR and CSC matrices on the device (src/device/bin_kernels.hip,
// src/device/csr_bin_kernels.hip, src/device/csc_bin_kernels.hip; reference
// include/LightGBM/bin.h:132 ValueToBin).
#pragma once

#include <cstdint>
#include <vector>

#include "lgbm_amd/config.h"

namespace lgbm_amd {

class Dataset;

// the HIP device a dataset under `cfg` is binned on (gpu_device_id, else LOCAL_RANK, else 0), or
// -1: none visible
int BinningDevice(const Config& cfg);

// device binning for an nrow x ncol matrix: LGBM_AMD_DEVICE_BINNING=0 never, =1 whenever a HIP
// device is visible, otherwise for device_type=gpu and at least 4M values
bool UseDeviceBinning(const Config& cfg, int64_t nrow, int64_t ncol);

// Writes the group columns of every group whose members are all numerical columns of the
// matrix (float32 or float64, row- or column-major) into `ds`, bit-identical to pushing the
// rows on the host.  Returns per column whether it was handled (the caller pushes the rest).
std::vector<char> DeviceBinDenseMatrix(Dataset* ds, const void* data, bool is_f64, int32_t nrow, int32_t ncol,
                                       bool row_major, const Config& cfg);

// device binning for a CSR matrix of nelem stored entries: the same knob; without it,
// device_type=gpu and at least kCsrBinMinEntries stored entries.  (The device path was ahead at
// every size timed, down to 60K entries; from 1M entries on it is ahead by more than the
// run-to-run spread of a construction of a few milliseconds: profiles/r13_device_sparse_binning.md)
constexpr int64_t kCsrBinMinEntries = int64_t{1} << 20;
bool UseDeviceBinningCsr(const Config& cfg, int64_t nelem);

// Writes every group whose members are all numerical into `ds` from the rows of a CSR matrix
// (indptr: nrow + 1 entries, C_API_DTYPE_INT32 / INT64; data: nelem values, C_API_DTYPE_FLOAT32 /
// FLOAT64), bit-identical to Dataset::PushSparseRow of every row on the host: dense groups get
// their column, sparse groups their stored rows and bins appended chunk by chunk.  Returns per
// group of the dataset whether it was handled (the caller pushes the entries of the other groups);
// nothing is handled when no device is visible, indptr is not a non-decreasing sequence inside
// [0, nelem], or more than kMaxPushZeroFeatures features need their zeros pushed.
std::vector<char> DeviceBinCsrMatrix(Dataset* ds, const void* indptr, int indptr_type, const int32_t* indices,
                                     const void* data, int data_type, int64_t nrow, int64_t nelem, const Config& cfg);

// The rule of one CSR row (src/device/csr_bins.h) on the host with the dataset's mappers:
// bins[nrow][ds.num_groups()], -1 in the columns of groups with a categorical member.  No GPU.
void EvalCsrGroupBins(const Dataset& ds, const void* indptr, int indptr_type, const int32_t* indices,
                      const void* data, int data_type, int64_t nrow, int64_t nelem, int32_t* bins);

// ... and by k_csr_to_group_bins on CSR arrays in device memory, into d_bins (device, the same
// layout), on the current device's null stream; returns after it finished
void CsrGroupBinsOnDevice(const Dataset& ds, const void* d_indptr, int indptr_type, const int32_t* d_indices,
                          const void* d_data, int data_type, int64_t nrow, int64_t nelem, int32_t* d_bins);

// out[0]: stored entries a wave reads per batch; out[1]: rows per workgroup; out[2]: rows per
// compaction tile; out[3]: kMaxPushZeroFeatures
void CsrBinLaunchInfo(int64_t* out);

// device binning for a CSC matrix of nelem stored entries: the same knob; without it,
// device_type=gpu and at least kCscBinMinEntries stored entries.  (120K entries, 3K x 2000 at 2 %,
// was the smallest size timed at which the device path was ahead of the host path by more than the
// run-to-run spread on both the training set, 1.7x, and a reference= set, 4.1x; at 60K entries the
// host path was ahead: profiles/r14_device_csc_binning.md)
constexpr int64_t kCscBinMinEntries = 120000;
bool UseDeviceBinningCsc(const Config& cfg, int64_t nelem);

// whether col_ptr (ncol_ptr entries) is a non-decreasing sequence inside [0, nelem]
bool CscPointerValid(const void* col_ptr, int col_ptr_type, int64_t ncol_ptr, int64_t nelem);

// Writes every group whose members are all numerical into `ds` from the columns of a CSC matrix
// (col_ptr: ncol_ptr entries; indices: the row of each of the nelem entries; num_row rows),
// bit-identical to transposing the matrix into rows and Dataset::PushSparseRow of every row
// (src/device/csc_bins.h), an entry on a row outside the matrix dropped.  Groups go through in
// windows; a sparse group's list is complete in one.  Returns per group of the dataset whether it
// was handled; nothing is handled when no device is visible, col_ptr is not valid (above) or more
// than kMaxPushZeroFeatures features need their zeros pushed.
std::vector<char> DeviceBinCscMatrix(Dataset* ds, const void* col_ptr, int col_ptr_type, const int32_t* indices,
                                     const void* data, int data_type, int64_t ncol_ptr, int64_t nelem, int64_t num_row,
                                     const Config& cfg);

// The rule of src/device/csc_bins.h on the host with the dataset's mappers:
// bins[num_row][ds.num_groups()], -1 in the columns of groups with a categorical member.  No GPU.
void EvalCscGroupBins(const Dataset& ds, const void* col_ptr, int col_ptr_type, const int32_t* indices,
                      const void* data, int data_type, int64_t ncol_ptr, int64_t nelem, int64_t num_row,
                      int32_t* bins);

// ... and by the kernels on CSC arrays in device memory, into d_bins (device, the same layout), on
// the current device's null stream; returns after they finished
void CscGroupBinsOnDevice(const Dataset& ds, const void* d_col_ptr, int col_ptr_type, const int32_t* d_indices,
                          const void* d_data, int data_type, int64_t ncol_ptr, int64_t nelem, int64_t num_row,
                          int32_t* d_bins);

// out[0]: stored entries of a column that one wave takes (a segment); out[1]:
// kMaxPushZeroFeatures; out[2]: rows per compaction tile; out[3]: threads of a workgroup; out[4]:
// entries the single wave of a column with repeated or unsorted rows reads at a time
void CscBinLaunchInfo(int64_t* out);

// matrices that went through DeviceBinCscMatrix, and bin samples taken column by column
// (LGBM_DatasetCreateFromCSC), in this process
void DeviceBinCscStats(int64_t* csc_calls, int64_t* column_samples);
void NoteCscColumnSample();

// how many matrices went through DeviceBinDenseMatrix / DeviceBinCsrMatrix in this process
void DeviceBinStats(int64_t* dense_calls, int64_t* csr_calls);
void NoteDeviceBinCall(bool csr);  // (the two paths count themselves)

}  // namespace lgbm_amd
