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
//   k_predict_tile_stop, k_predict_forest_stop
//                      early-stopped scores (pred_early_stop) of the two routes.  The window is
//                      walked in periods of stop_freq iterations.  A lane holds the id of a row of
//                      its workgroup and reads the tile at [slot * pitch + id] (the compact matrix
//                      at [slot * num_rows + row0 + id]): any lane can walk any row, so at a period
//                      end the rows that go on are moved to the lowest lanes and emptied waves
//                      stop walking (src/device/early_stop.h has the period end and its barriers).
//                      A row's raw sums are stored where it stops and the workgroup finishes its
//                      rows in place after its last tree, so neither route runs k_convert_scores.  The period end's LDS
//                      comes out of the tile's budget (PlanTensorPredictStop).
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
#include "early_stop.h"
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

// the trees of one period: stop_freq iterations, whole
__device__ __forceinline__ int StopPeriodTrees(const TensorPredictArgs& a, int num_trees) {
  return static_cast<int>(min(static_cast<long long>(a.stop_freq) * a.num_class, static_cast<long long>(num_trees)));
}

// A row of the stop kernels ends in two steps, so that no finish lies within the walk, where it
// would hold a second copy of the sums in registers beside those of the rows that go on (141
// registers and 3 waves per SIMD in place of k_predict_tile's 98 and 5): where the row stops, or
// after the last tree, its raw sums go to `out` as they are ...
__device__ __forceinline__ void StoreRawRow(const TensorPredictArgs& a, const double (&acc)[kMaxPredClasses],
                                            long long row) {
#pragma unroll
  for (int c = 0; c < kMaxPredClasses; ++c) {
    if (c < a.num_class) a.out[row * a.num_class + c] = acc[c];
  }
}

// ... and when the workgroup has walked its last tree, thread i finishes row i of its nr rows in
// place, whichever lane stored it (the barrier orders the workgroup's stores before these loads).
// Every thread of the workgroup calls it
__device__ __forceinline__ void FinishStoredRows(const TensorPredictArgs& a, long long row0, int nr) {
  if (!(a.divisor > 0.0) && a.conv_kind <= 0) return;  // (raw scores; the same in every thread)
  __syncthreads();
  if (static_cast<int>(threadIdx.x) >= nr) return;
  double* mine = a.out + (row0 + threadIdx.x) * a.num_class;
  double score[kMaxPredClasses];
  for (int c = 0; c < a.num_class; ++c) score[c] = mine[c];
  FinishScoreRow(score, a.num_class, a.divisor, a.conv_kind, a.conv_param);
  for (int c = 0; c < a.num_class; ++c) mine[c] = score[c];
}

template <typename T>
__global__ __launch_bounds__(kStopRows) void k_predict_tile_stop(TensorPredictArgs a) {
  extern __shared__ double s_tile[];  // the period end's arrays, then the tile
  const StopLds lds = CarveStopLds(s_tile, a.num_class);
  T* s_val = reinterpret_cast<T*>(s_tile + TensorStopLdsBytes(a.num_class) / 8);
  const int tid = threadIdx.x;
  const long long row0 = static_cast<long long>(blockIdx.x) * kStopRows;
  const int nr = static_cast<int>(min(static_cast<long long>(kStopRows), static_cast<long long>(a.num_rows) - row0));
  const int pitch = TensorTilePitch(kStopRows, static_cast<int>(sizeof(T)));
  GatherTile(static_cast<const T*>(a.data), a.row_stride, a.col_stride, a.used, row0, nr, a.num_slots, pitch, s_val);
  __syncthreads();
  int rid = tid;
  bool live = tid < nr;
  double acc[kMaxPredClasses];
#pragma unroll
  for (int c = 0; c < kMaxPredClasses; ++c) acc[c] = 0.0;
  const int per = StopPeriodTrees(a, a.num_trees);
  // (t0, per and the rows left are the same in every thread: all of them reach every period end)
  for (int t0 = 0, period = 0; t0 < a.num_trees; t0 += per, ++period) {
    const int t1 = min(t0 + per, a.num_trees);
    if (live) {
      const T* mine = s_val + rid;
      int k = 0;
      for (int t = t0; t < t1; ++t) {
        const int n0 = a.node_off[t];
        const int leaf = PackedTreeLeaf(a.nodes + n0, a.node_off[t + 1] - n0, a.cat_bits, mine, pitch);
        const double lv = a.leaf_value[a.leaf_off[t] + leaf];
#pragma unroll
        for (int c = 0; c < kMaxPredClasses; ++c) {
          if (c == k) acc[c] += lv;
        }
        k = k + 1 == a.num_class ? 0 : k + 1;
      }
    }
    if (t1 >= a.num_trees) break;
    if (StopPeriodEnd(a, lds, period, acc, rid, live, [&](int r) { StoreRawRow(a, acc, row0 + r); }) == 0) break;
  }
  if (live) StoreRawRow(a, acc, row0 + rid);
  FinishStoredRows(a, row0, nr);
}

template <typename T>
__global__ __launch_bounds__(kStopRows) void k_predict_forest_stop(ForestArgs f, TensorPredictArgs a) {
  __shared__ double s_stop[(2 * kStopRows * 8 + kStopRows * 4 + 2 * kStopWaves * 4) / 8];  // TensorStopLdsBytes at its most
  const StopLds lds = CarveStopLds(s_stop, a.num_class);
  const int tid = threadIdx.x;
  const long long row0 = static_cast<long long>(blockIdx.x) * kStopRows;
  const T* x = static_cast<const T*>(f.data) + row0;
  int rid = tid;
  bool live = row0 + tid < f.num_rows;
  double acc[kMaxPredClasses];
#pragma unroll
  for (int c = 0; c < kMaxPredClasses; ++c) acc[c] = 0.0;
  const int per = StopPeriodTrees(a, f.num_trees);
  for (int t0 = 0, period = 0; t0 < f.num_trees; t0 += per, ++period) {
    const int t1 = min(t0 + per, f.num_trees);
    if (live) {
      int k = 0;
      for (int t = t0; t < t1; ++t) {
        const int n0 = f.node_off[t], n1 = f.node_off[t + 1];
        int leaf = 0;
        if (n1 > n0) {
          int node = 0;
          while (node >= 0) {
            const int gi = n0 + node;
            const double v = static_cast<double>(x[static_cast<int64_t>(f.feature[gi]) * f.num_rows + rid]);
            node = ForestGoesLeft(f, t, gi, v) ? f.left[gi] : f.right[gi];
          }
          leaf = ~node;
        }
        const double lv = f.leaf_value[f.leaf_off[t] + leaf];
#pragma unroll
        for (int c = 0; c < kMaxPredClasses; ++c) {
          if (c == k) acc[c] += lv;
        }
        k = k + 1 == a.num_class ? 0 : k + 1;
      }
    }
    if (t1 >= f.num_trees) break;
    if (StopPeriodEnd(a, lds, period, acc, rid, live, [&](int r) { StoreRawRow(a, acc, row0 + r); }) == 0) break;
  }
  if (live) StoreRawRow(a, acc, row0 + rid);
  FinishStoredRows(a, row0, static_cast<int>(min(static_cast<long long>(kStopRows), static_cast<long long>(f.num_rows) - row0)));
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
    if (a.stop_freq > 0) {
      // (PlanTensorPredictStop: one height, and the period end's bytes within the same budget)
      hipLaunchKernelGGL(k_predict_tile_stop<T>, dim3(grid), dim3(kStopRows), lds + TensorStopLdsBytes(a.num_class), s, a);
      return;
    }
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

void PredictForestStop(const ForestArgs& f, const TensorPredictArgs& a, hipStream_t s) {
  if (f.num_rows <= 0) return;
  const dim3 grid(static_cast<unsigned>((f.num_rows + kStopRows - 1) / kStopRows));
  if (f.is_double) hipLaunchKernelGGL(k_predict_forest_stop<double>, grid, dim3(kStopRows), 0, s, f, a);
  else hipLaunchKernelGGL(k_predict_forest_stop<float>, grid, dim3(kStopRows), 0, s, f, a);
}

void ConvertTensorScores(const TensorPredictArgs& a, hipStream_t s) {
  if (a.num_rows <= 0) return;
  hipLaunchKernelGGL(k_convert_scores, dim3(static_cast<unsigned>((a.num_rows + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace dev
}  // namespace lgbm_amd
