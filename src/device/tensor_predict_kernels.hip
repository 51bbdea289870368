// Prediction of a matrix that already lies in device memory (LGBM_AMD_BoosterPredictForDeviceMat:
// Booster.predict_device of a GPU tensor), read where it lies: float16, bfloat16, float32 or
// float64 elements behind a pointer with a row and a column stride.  The rule -- plan, tile,
// packed node, walk, finish -- is src/device/tensor_predict.h; LGBM_AMD_TensorPredictOnHost
// evaluates it without a GPU.
//
//   k_predict_tile     scores (raw, or through the average of boosting=rf and the objective's
//                      output transform) and leaf indices.  A workgroup of R threads takes R rows,
//                      one lane per row, so every class sum is the same doubles in the same order as
//                      the host predictor's.  It first gathers its tile: the R rows by the S slot
//                      columns (the features the window's trees split on), elements kept in their
//                      own type and laid out [slot][row].  Lanes run along the smaller stride of the
//                      matrix: along the slots of a row for a row-major matrix (2^k <= 64 lanes per
//                      row, the other lanes on the rows after it), along the rows of a slot
//                      otherwise; a general stride is read correctly and uncoalesced.  The pitch
//                      between slots (TensorTilePitch) spreads the transposing write of the first
//                      case over the banks.  The walk then reads a lane's value at
//                      [slot * pitch + lane]: lanes that ask for one slot read consecutive
//                      elements, two 2-byte lanes in one word, and one 16-byte packed node per
//                      step in place of the five arrays of k_predict_forest
//                      (src/device/predict_kernels.hip).  The finish runs ConvertScoreRow on the
//                      lane's class sums.
//   k_tensor_to_slots  the same gather in batches of 64 B per row (8 float64, 16 float32, 32 half
//                      slots), written as the compact column-major matrix that the CSR and CSC
//                      paths feed to k_predict_forest / k_predict_leaf / k_shap_forest: for
//                      contributions, for a window whose slots do not fit the smallest tile and for
//                      trees whose children do not fit 16 bits.
//   k_convert_scores   the finish of a row for the scores of that route.
//
// Sizes (gfx950: 160 KiB of LDS per CU).  A tile has 256 rows and at most kTensorPredictLdsBytes =
// 52 KiB: 51 float32, 103 half or 25 float64 slots, and three workgroups (12 waves) on a CU.  The
// walk is a chain of dependent loads (node, value, node, ...) that only other waves hide, so the
// budget is an occupancy: 28 float32 slots are 28 KiB, five workgroups and 20 waves per CU, and
// 2.4 times as fast as k_predict_forest on the same tensor; at 12 waves the tile kernel was still
// ahead of the slots route, at 8 behind it.  A ladder of shorter tiles (128 and 64 rows under
// 64 KiB) held more slots with 6 and 3 waves per CU and was measured 1.4 and 2.1 times
// slower than the slots route, which keeps full occupancy at the cost of writing and reading the
// compact matrix once; the plan has one step for that reason.
// profiles/r21_tensor_predict.md has the figures.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "tensor_predict.h"

namespace lgbm_amd {
namespace dev {

namespace {

constexpr int kSlotsTileRows = 256;    // rows of a k_tensor_to_slots workgroup (one thread each)
constexpr int kSlotsTileRowBytes = 64;  // bytes of one row in a batch of slots

// rows [row0, row0 + nr) by the nc slots at used[0 .. nc) into s_val[c * pitch + r]; the workgroup
// has one thread per row of the tile (a power of two, at least 64)
template <typename T>
__device__ __forceinline__ void GatherTile(const T* x, long long rs, long long cs, const int32_t* used, long long row0,
                                           int nr, int nc, int pitch, T* s_val) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (cs <= rs) {
    int shift = 0;  // 2^shift lanes along the slots of one row
    while ((1 << shift) < nc && shift < 6) ++shift;
    const int w = 1 << shift, lc = tid & (w - 1), lr = tid >> shift, rows_per_pass = nt >> shift;
    for (int c = lc; c < nc; c += w) {
      const long long col = cs * used[c];
      for (int r = lr; r < nr; r += rows_per_pass) s_val[c * pitch + r] = x[rs * (row0 + r) + col];
    }
  } else if (tid < nr) {
    const T* mine = x + rs * (row0 + tid);
    for (int c = 0; c < nc; ++c) s_val[c * pitch + tid] = mine[cs * used[c]];
  }
}

template <typename T, bool LEAF>
__global__ __launch_bounds__(256) void k_predict_tile(TensorPredictArgs a) {
  extern __shared__ double s_tile[];  // (8-byte aligned for every element type)
  T* s_val = reinterpret_cast<T*>(s_tile);
  const int R = blockDim.x, tid = threadIdx.x;
  const long long row0 = static_cast<long long>(blockIdx.x) * R;
  const int nr = static_cast<int>(min(static_cast<long long>(R), static_cast<long long>(a.num_rows) - row0));
  const int pitch = TensorTilePitch(R, static_cast<int>(sizeof(T)));
  GatherTile(static_cast<const T*>(a.data), a.row_stride, a.col_stride, a.used, row0, nr, a.num_slots, pitch, s_val);
  __syncthreads();
  if (tid >= nr) return;
  const T* mine = s_val + tid;
  const long long row = row0 + tid;
  double acc[kMaxPredClasses];
#pragma unroll
  for (int c = 0; c < kMaxPredClasses; ++c) acc[c] = 0.0;
  int k = 0;
  for (int t = 0; t < a.num_trees; ++t) {
    const int n0 = a.node_off[t];
    const int leaf = PackedTreeLeaf(a.nodes + n0, a.node_off[t + 1] - n0, a.cat_bits, mine, pitch);
    if (LEAF) {
      a.out[row * a.num_trees + t] = leaf;
    } else {
      const double lv = a.leaf_value[a.leaf_off[t] + leaf];
#pragma unroll
      for (int c = 0; c < kMaxPredClasses; ++c) {
        if (c == k) acc[c] += lv;
      }
      k = k + 1 == a.num_class ? 0 : k + 1;
    }
  }
  if (LEAF) return;
  // (a copy that the finish may index: the sums above stay in registers through the walk)
  double score[kMaxPredClasses];
#pragma unroll
  for (int c = 0; c < kMaxPredClasses; ++c) score[c] = acc[c];
  FinishScoreRow(score, a.num_class, a.divisor, a.conv_kind, a.conv_param);
  for (int c = 0; c < a.num_class; ++c) a.out[row * a.num_class + c] = score[c];
}

template <typename T>
__global__ __launch_bounds__(kSlotsTileRows) void k_tensor_to_slots(TensorPredictArgs a, int nbatch, void* d_mat) {
  using O = std::conditional_t<std::is_same<T, double>::value, double, float>;
  constexpr int kCols = kSlotsTileRowBytes / static_cast<int>(sizeof(T));
  constexpr int kPitch = kSlotsTileRows + (sizeof(T) == 2 ? 2 : 1);  // TensorTilePitch
  __shared__ T s_val[kCols * kPitch];
  const int tid = threadIdx.x;
  const int c0 = static_cast<int>(blockIdx.x % nbatch) * kCols;
  const long long row0 = static_cast<long long>(blockIdx.x / nbatch) * kSlotsTileRows;
  const int nr = static_cast<int>(min(static_cast<long long>(kSlotsTileRows), static_cast<long long>(a.num_rows) - row0));
  const int nc = min(kCols, a.num_slots - c0);
  GatherTile(static_cast<const T*>(a.data), a.row_stride, a.col_stride, a.used + c0, row0, nr, nc, kPitch, s_val);
  __syncthreads();
  if (tid >= nr) return;
  O* out = static_cast<O*>(d_mat) + row0 + tid;
  for (int c = 0; c < nc; ++c) {
    out[static_cast<long long>(c0 + c) * a.num_rows] = static_cast<O>(WidenElement(s_val[c * kPitch + tid]));
  }
}

__global__ __launch_bounds__(256) void k_convert_scores(TensorPredictArgs a) {
  const long long row = blockIdx.x * 256ll + threadIdx.x;
  if (row >= a.num_rows) return;
  double score[kMaxPredClasses];
  for (int c = 0; c < a.num_class; ++c) score[c] = a.out[row * a.num_class + c];
  FinishScoreRow(score, a.num_class, a.divisor, a.conv_kind, a.conv_param);
  for (int c = 0; c < a.num_class; ++c) a.out[row * a.num_class + c] = score[c];
}

}  // namespace

void PredictTensorTile(const TensorPredictArgs& a, hipStream_t s) {
  if (a.num_rows <= 0) return;
  const unsigned grid = static_cast<unsigned>((a.num_rows + a.tile_rows - 1) / a.tile_rows);
  DispatchTensorElement(a.data_type, [&](auto* p) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
    const size_t lds = static_cast<size_t>(TensorTileBytes(a.num_slots, a.tile_rows, static_cast<int>(sizeof(T))));
    if (a.leaf) hipLaunchKernelGGL((k_predict_tile<T, true>), dim3(grid), dim3(a.tile_rows), lds, s, a);
    else hipLaunchKernelGGL((k_predict_tile<T, false>), dim3(grid), dim3(a.tile_rows), lds, s, a);
  });
}

void TensorToSlots(const TensorPredictArgs& a, void* d_mat, hipStream_t s) {
  if (a.num_rows <= 0 || a.num_slots <= 0) return;
  DispatchTensorElement(a.data_type, [&](auto* p) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
    const int cols = kSlotsTileRowBytes / static_cast<int>(sizeof(T));
    const int nbatch = (a.num_slots + cols - 1) / cols;
    const long long tiles = (a.num_rows + kSlotsTileRows - 1) / kSlotsTileRows;
    hipLaunchKernelGGL(k_tensor_to_slots<T>, dim3(static_cast<unsigned>(tiles * nbatch)), dim3(kSlotsTileRows), 0, s, a,
                       nbatch, d_mat);
  });
}

void ConvertTensorScores(const TensorPredictArgs& a, hipStream_t s) {
  if (a.num_rows <= 0) return;
  hipLaunchKernelGGL(k_convert_scores, dim3(static_cast<unsigned>((a.num_rows + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace dev
}  // namespace lgbm_amd
