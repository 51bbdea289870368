// The period end of the early-stopped prediction kernels (k_predict_tile_stop and
// k_predict_forest_stop, src/device/tensor_predict_kernels.hip; the rule is stated in
// src/device/tensor_predict.h).  A workgroup of 256 lanes holds up to 256 rows, a lane the id of
// one row and its class sums in registers.  After every stop_freq iterations:
//   1. a lane with a row evaluates StopMargin; the sums of a row that stops are stored at once, as
//      they are (the kernel finishes its rows after its last tree), and its lane gives the row up;
//   2. each wave counts its surviving rows (ballot, popcount) into LDS; after one barrier every
//      lane reads the four counts: their sum, the rows before its wave, the waves that hold rows;
//   3. where the survivors fit in fewer waves than hold them, they move to the lowest lanes: a
//      surviving lane writes its row id and, one class at a time, that class's sum at its rank in
//      the workgroup, and lane i < survivors takes over what lies at i.  One class at a time keeps
//      the staging at 2 or 4 KiB where all 16 classes at once would take 32 KiB from the tile; with
//      several classes two arrays take turns, so a class costs one barrier.  Where no wave would be
//      freed the rows stay: moving them then saves no walk.
// Waves without rows walk nothing afterwards and only arrive at these barriers.
//
// Barriers.  Every thread of the workgroup calls StopPeriodEnd at every period end, rows or not,
// and no thread leaves the kernel between two of them.  Each branch around a barrier is uniform
// over the workgroup: the class count is a kernel argument, and the counts come from LDS after the
// barrier of step 2, the same words for every wave, through readfirstlane.  The counts of two
// consecutive periods lie in different words, so a wave that is already at the next period's
// step 2 writes nothing that a slower wave still reads; the ids and the staging are written only
// after that step's barrier, which a wave reaches after its last read of them.
#pragma once

#include <hip/hip_runtime.h>

#include "tensor_predict.h"

namespace lgbm_amd {
namespace dev {

constexpr int kStopRows = kStopWaves * 64;  // rows and lanes of a workgroup

// TensorStopLdsBytes(num_class) bytes at an 8-byte boundary
struct StopLds {
  double* stage;    // [num_class > 1 ? 2 : 1][kStopRows] sums of one class, by rank
  int32_t* ids;     // [kStopRows] row ids, by rank
  int32_t* counts;  // [2][kStopWaves] surviving rows of each wave, by the period's parity
};

__device__ __forceinline__ StopLds CarveStopLds(void* base, int num_class) {
  StopLds l;
  l.stage = static_cast<double*>(base);
  l.ids = reinterpret_cast<int32_t*>(l.stage + (num_class > 1 ? 2 : 1) * kStopRows);
  l.counts = l.ids + kStopRows;
  return l;
}

// The end of period `period` (0, 1, ...) when trees remain.  rid: the lane's row of the workgroup,
// live: whether it has one, acc: the row's sums; store(rid) writes the sums of a row that stops.  Returns
// the rows that the workgroup still holds.
template <typename Store>
__device__ __forceinline__ int StopPeriodEnd(const TensorPredictArgs& a, const StopLds& l, int period,
                                             double (&acc)[kMaxPredClasses], int& rid, bool& live, Store&& store) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (live && StopMargin(acc, a.num_class, a.stop_binary != 0) > a.stop_margin) {
    store(rid);
    live = false;
  }
  const unsigned long long mine = __ballot(live);
  int32_t* counts = l.counts + (period & 1) * kStopWaves;
  if (lane == 0) counts[wave] = __popcll(mine);
  __syncthreads();
  int total = 0, before = 0, holding = 0;
#pragma unroll
  for (int w = 0; w < kStopWaves; ++w) {
    const int c = counts[w];
    if (w < wave) before += c;
    total += c;
    holding += c > 0 ? 1 : 0;
  }
  total = __builtin_amdgcn_readfirstlane(total);
  holding = __builtin_amdgcn_readfirstlane(holding);
  if (a.stop_compact != 0 && (total + 63) / 64 < holding) {
    const int rank = before + __popcll(mine & ((1ull << lane) - 1ull));
    if (live) l.ids[rank] = rid;
#pragma unroll
    for (int c = 0; c < kMaxPredClasses; ++c) {
      if (c < a.num_class) {
        double* buf = l.stage + (c & 1) * kStopRows;
        if (live) buf[rank] = acc[c];
        __syncthreads();
        if (tid < total) acc[c] = buf[tid];
      }
    }
    if (tid < total) rid = l.ids[tid];
    live = tid < total;
  }
  return total;
}

}  // namespace dev
}  // namespace lgbm_amd
