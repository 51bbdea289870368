// Value -> bin mapping of dense, CSR and CSC matrices on the device (src/device/bin_kernels.hip,
// src/device/csr_bin_kernels.hip, src/device/csc_bin_kernels.hip) and of matrices already in
// device memory (src/device/tensor_bin_kernels.hip); reference
// include/LightGBM/bin.h:132 ValueToBin).
#pragma once

#include <cstdint>
#include <vector>

#include "lgbm_amd/config.h"

namespace lgbm_amd {

class Dataset;
struct SampleDistinctLists;  // (lgbm_amd/bin.h)

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

// A matrix that already lies in device memory (src/device/tensor_bin_kernels.hip): nrow x ncol
// elements of data_type (C_API_DTYPE_FLOAT32 / FLOAT64 / FLOAT16 / BFLOAT16) on device_id, element
// (r, c) at data[r * row_stride + c * col_stride] (strides in elements: row-major, column-major
// and sliced views alike).  Both calls below run on device_id's null stream, restore the caller's
// device and return after everything has finished.
struct DeviceTensor {
  const void* data;
  int data_type;
  int32_t nrow, ncol;
  int64_t row_stride, col_stride;
  int device_id;
};

// The bin sample of the matrix: rows `rows` (SampleRows) gathered on the device, copied back and
// filtered by the zero / NaN rule of the host's row reader into sv / si [ncol], the arguments of
// Dataset::ConstructFromSample -- the same values at the same sample positions as from a host copy.
// With `distinct`, every column's distinct values (BinMapper::SampleDistinct) are found on the
// device as well (src/device/bin_find_kernels.hip): each pass of columns is sorted after its copy
// to the host has been issued, while the host filters that copy, and only the runs come back.
void SampleDeviceTensor(const DeviceTensor& t, const std::vector<int>& rows, std::vector<std::vector<double>>* sv,
                        std::vector<std::vector<int>>* si, SampleDistinctLists* distinct = nullptr);

// Whether the bin finder of a GPU tensor's sample (sample_cnt rows x ncol columns) takes its
// distinct values from the device: LGBM_AMD_DEVICE_BIN_FIND=0 never, =1 always; otherwise for
// samples of at least kBinFindMinSampleRows rows and at most kBinFindMaxSampleValues values.  Never
// when loading is distributed (each rank finds the bins of its own block of columns from the host
// sample).  Every size timed inside that window was ahead of the host sort by more than the
// run-to-run spread (10K x 28: 2.5 against 3.0 ms; 200K x 28, the sample of 10M x 28: 169 against
// 177 ms); shorter columns sort too quickly on the host to pay for the launches, and above the
// window the runs of continuous columns -- as many as the sample has values, 12 bytes each -- cost
// more to copy back than 16 host threads need to sort: 50K x 200 (10M values) was a tie, 100K x 200
// behind by 5 %, 200K x 2000 by 30 % (profiles/r20_device_bin_finder.md).
constexpr int64_t kBinFindMinSampleRows = 10000;
constexpr int64_t kBinFindMaxSampleValues = 5600000;
bool UseDeviceBinFind(int64_t sample_cnt, int64_t ncol);

// the host evaluator of the kernels' rule (src/device/sample_distinct.h) on a column-major sample
// [ncol][ns], or on columns of their own lengths (LGBM_AMD_DEVICE_BIN_FIND=2).  No GPU.
void EvalSampleDistinctLists(const double* sample, int64_t ns, int32_t ncol, SampleDistinctLists* out);
void EvalSampleDistinctLists(const std::vector<std::vector<double>>& columns, SampleDistinctLists* out);

// out[0]: keys of a scatter tile of the sort; out[1]: threads of its workgroup (one per column);
// out[2]: entries per step of the compaction and of the run pass; out[3]: kBinFindMinSampleRows;
// out[4]: kBinFindMaxSampleValues
void BinFindLaunchInfo(int64_t* out);

// samples whose distinct values came from the device in this process
void NoteDeviceBinFind();
int64_t DeviceBinFindCalls();

// Writes every group of `ds` (its mappers found, or taken from a reference) from the matrix,
// bit-identical to the column loop of LGBM_DatasetCreateFromMat on a host copy: dense groups of
// numerical and categorical members by k_tensor_to_group_bins; the columns of the other groups
// (sparse storage, a categorical feature of more than kTensorMaxCategories categories) gathered as
// doubles and pushed through Dataset::PushColumnValue.  The caller calls FinishLoad.
void BinDeviceTensor(Dataset* ds, const DeviceTensor& t);

// The rule of src/device/tensor_bins.h on the host, for a host matrix of the same description, with
// the dataset's mappers: bins[nrow][ds.num_groups()], -1 in the columns of the groups that
// BinDeviceTensor hands to the host.  No GPU.
void EvalTensorGroupBins(const Dataset& ds, const void* data, int data_type, int32_t nrow, int32_t ncol,
                         int64_t row_stride, int64_t col_stride, int32_t* bins);

// A GPU tensor of fewer values goes through the host copy it went through before, unless it is
// bfloat16 (which has no host path) or LGBM_AMD_DEVICE_BINNING=1: 10K x 28 was the smallest size
// timed at which reading the tensor in place was ahead of the host copy (3.2 ms against 4.8 ms for the
// training set, 0.58 ms against 1.07 ms for a reference= set); at 1K x 28 it was behind by 0.35 ms
// and 0.4 ms, more than twice the run-to-run spread (profiles/r19_tensor_dataset.md).  The Python
// dispatch reads it from TensorBinLaunchInfo.
constexpr int64_t kTensorBinMinValues = 280000;

// out[0]: rows of a k_tensor_to_group_bins workgroup; out[1]: the (sample, column) tile edge of
// k_gather_sample; out[2]: kTensorMaxCategories; out[3]: bytes of a row in one value batch; out[4]:
// kTensorBinMinValues
void TensorBinLaunchInfo(int64_t* out);

// matrices that went through BinDeviceTensor in this process, and samples whose distinct values
// the device found (either pointer may be null)
void DeviceBinTensorStats(int64_t* tensor_calls, int64_t* bin_find_calls);

// how many matrices went through DeviceBinDenseMatrix / DeviceBinCsrMatrix in this process
void DeviceBinStats(int64_t* dense_calls, int64_t* csr_calls);
void NoteDeviceBinCall(bool csr);  // (the two paths count themselves)

}  // namespace lgbm_amd
