// A booster's forest prediction on caller-owned device buffers, for the stand-alone ops
// (src/capi/ops_api.cpp: LGBMAMD_OpForestPredict, ...CSR, ...CSC).  Defined in c_api.cpp, where
// the Booster behind a handle lives; they throw what the op reports.
#pragma once

#include <cstdint>

#include "lgbm_amd/c_api.h"

namespace lgbm_amd {

void BoosterPredictDeviceBuffers(BoosterHandle handle, const void* d_data, int data_type, int64_t nrow, int32_t ncol,
                                 int predict_type, int start_iteration, int num_iteration, double* d_out,
                                 int64_t out_len);
void BoosterPredictCSRDeviceBuffers(BoosterHandle handle, const void* d_indptr, int indptr_type,
                                    const int32_t* d_indices, const void* d_data, int data_type, int64_t nrow,
                                    int64_t nelem, int predict_type, int start_iteration, int num_iteration,
                                    double* d_out, int64_t out_len);
void BoosterPredictCSCDeviceBuffers(BoosterHandle handle, const void* d_col_ptr, int col_ptr_type,
                                    const int32_t* d_indices, const void* d_data, int data_type, int64_t ncol,
                                    int64_t nelem, int64_t nrow, int predict_type, int start_iteration,
                                    int num_iteration, double* d_out, int64_t out_len);

}  // namespace lgbm_amd
