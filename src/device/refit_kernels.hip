// Refit of an existing forest's leaf values on the device (GBDT::RefitTree): the leaf matrix says
// where every row lands, so a tree needs no walk -- one pass for its per-leaf sums and one for
// the score update, both over the tree's staged leaf column.
#include <algorithm>

#include "device_common.h"
#include "refit_quant.h"

namespace lgbm_amd {
namespace dev {

// ---------------------------------------------------------------- staging
// A chunk of rows of the row-major matrix -> the tree-major staged matrix, through padded LDS
// tiles (reads run along a row's trees, writes along a tree's rows).  Every entry is checked
// against its tree's leaf count here, once: an offender is counted, its column recorded, and
// leaf 0 staged in its place, so that whatever reads the staged matrix indexes inside the tree.
template <typename OUT>
__global__ __launch_bounds__(kRefitThreads) void k_refit_stage(RefitStageArgs a) {
  __shared__ int32_t tile[kRefitTile][kRefitTile + 1];
  const int tx = threadIdx.x % kRefitTile, ty = threadIdx.x / kRefitTile;
  constexpr int kStep = kRefitThreads / kRefitTile;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kRefitTile;
  const int c0 = blockIdx.y * kRefitTile;
  const int c = c0 + tx;
  const int32_t nl = c < a.cols ? a.num_leaves[c] : 0;
#pragma unroll
  for (int j = 0; j < kRefitTile; j += kStep) {
    const int64_t r = r0 + ty + j;
    int32_t v = 0;
    if (r < a.rows && c < a.cols) {
      v = a.src[r * a.src_stride + c];
      if (static_cast<uint32_t>(v) >= static_cast<uint32_t>(nl)) {
        atomicAdd(&a.bad[0], 1u);
        atomicMin(&a.bad[1], static_cast<uint32_t>(c));
        v = 0;
      }
    }
    tile[ty + j][tx] = v;
  }
  __syncthreads();
  OUT* out = static_cast<OUT*>(a.out);
#pragma unroll
  for (int j = 0; j < kRefitTile; j += kStep) {
    const int cc = c0 + ty + j;
    const int64_t r = r0 + tx;
    if (cc < a.cols && r < a.rows) out[static_cast<int64_t>(cc) * a.num_rows + a.row0 + r] = static_cast<OUT>(tile[tx][ty + j]);
  }
}

void RefitStage(const RefitStageArgs& a, hipStream_t s) {
  if (a.rows <= 0 || a.cols <= 0) return;
  const dim3 grid(static_cast<unsigned>((a.rows + kRefitTile - 1) / kRefitTile),
                  static_cast<unsigned>((a.cols + kRefitTile - 1) / kRefitTile));
  if (a.wide) {
    hipLaunchKernelGGL(k_refit_stage<int32_t>, grid, dim3(kRefitThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_refit_stage<uint16_t>, grid, dim3(kRefitThreads), 0, s, a);
  }
}

// ---------------------------------------------------------------- leaf sums
// bits of max |g| and max |h| over the rows (integer maxima: the same on every run)
__global__ __launch_bounds__(kRefitThreads) void k_refit_absmax(const float* __restrict__ g, const float* __restrict__ h,
                                                                int64_t n, uint32_t* absmax) {
  uint32_t mg = 0u, mh = 0u;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRefitThreads) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kRefitThreads) {
    mg = max(mg, RefitAbsBits(g[i]));
    mh = max(mh, RefitAbsBits(h[i]));
  }
  mg = WaveMaxDpp(mg);
  mh = WaveMaxDpp(mh);
  if ((threadIdx.x & 63) == 0) {
    if (mg != 0u) atomicMax(&absmax[0], mg);
    if (mh != 0u) atomicMax(&absmax[1], mh);
  }
}

// One tree's (sum g, sum h, count) per leaf.  Each row's g and h go to fixed point by the rule
// of refit_quant.h and are added as integers: into the workgroup's LDS tables (64-bit LDS
// atomics, as the histograms), whose non-zero entries are then added to the global table with
// 64-bit integer atomics; or, for trees of more than kRefitLdsLeaves leaves (LDS false),
// straight into the global table.  Integer sums do not depend on the order of the rows: the
// table is the same on every run.  h may be negative (negative weights): the sums are signed,
// carried in two's complement through the unsigned atomics.
template <typename LT, bool LDS>
__global__ __launch_bounds__(kRefitThreads) void k_refit_leaf_sums(RefitSumArgs a) {
  extern __shared__ unsigned long long lds[];
  const int L = a.num_leaves;
  const int eg = RefitScaleExp(a.absmax[0], a.n), eh = RefitScaleExp(a.absmax[1], a.n);
  const double sg = RefitScale(eg), sh = RefitScale(eh);
  unsigned long long* table = reinterpret_cast<unsigned long long*>(a.table);
  if (LDS) {
    for (int j = threadIdx.x; j < 3 * L; j += kRefitThreads) lds[j] = 0ull;
    __syncthreads();
  }
  unsigned long long* acc = LDS ? lds : table;
  const LT* leaf = static_cast<const LT*>(a.leaf);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRefitThreads;
  for (int64_t i0 = blockIdx.x * static_cast<int64_t>(kRefitThreads) + threadIdx.x; i0 < a.n;
       i0 += kRefitUnroll * stride) {
    uint32_t l[kRefitUnroll];
    float g[kRefitUnroll], h[kRefitUnroll];
#pragma unroll
    for (int k = 0; k < kRefitUnroll; ++k) {
      const int64_t i = i0 + k * stride;
      const bool in = i < a.n;
      l[k] = in ? static_cast<uint32_t>(leaf[i]) : 0xffffffffu;
      g[k] = in ? a.grad[i] : 0.f;
      h[k] = in ? a.hess[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kRefitUnroll; ++k) {
      if (l[k] < static_cast<uint32_t>(L)) {  // (staged ids are inside the tree; rows past n are not)
        atomicAdd(&acc[l[k]], static_cast<unsigned long long>(RefitQuantise(g[k], sg)));
        atomicAdd(&acc[L + l[k]], static_cast<unsigned long long>(RefitQuantise(h[k], sh)));
        atomicAdd(&acc[2 * L + l[k]], 1ull);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * L; j += kRefitThreads) {
      const unsigned long long v = lds[j];
      if (v != 0ull) atomicAdd(&table[j], v);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the scale exponents, next to the sums
    a.table[3 * L] = eg;
    a.table[3 * L + 1] = eh;
  }
}

int RefitSumGrid(int64_t n) {
  const int64_t per = static_cast<int64_t>(kRefitThreads) * kRefitUnroll;
  return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 2 * NumCUs())));
}

void RefitLeafSums(const RefitSumArgs& a, hipStream_t s) {
  const int L = a.num_leaves;
  (void)hipMemsetAsync(a.absmax, 0, 2 * sizeof(uint32_t), s);
  (void)hipMemsetAsync(a.table, 0, (3 * static_cast<size_t>(L) + 2) * sizeof(long long), s);
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_refit_absmax, dim3(GridFor(a.n)), dim3(kRefitThreads), 0, s, a.grad, a.hess, a.n, a.absmax);
  const dim3 grid(RefitSumGrid(a.n)), block(kRefitThreads);
  if (L <= kRefitLdsLeaves) {
    const size_t lds = 3 * static_cast<size_t>(L) * sizeof(unsigned long long);
    if (a.wide) {
      hipLaunchKernelGGL((k_refit_leaf_sums<int32_t, true>), grid, block, lds, s, a);
    } else {
      hipLaunchKernelGGL((k_refit_leaf_sums<uint16_t, true>), grid, block, lds, s, a);
    }
  } else if (a.wide) {
    hipLaunchKernelGGL((k_refit_leaf_sums<int32_t, false>), grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL((k_refit_leaf_sums<uint16_t, false>), grid, block, 0, s, a);
  }
}

// ---------------------------------------------------------------- score update
// score[i] += value[leaf[i]]: one double add per row, what the host's score updater does with
// the leaf partition.  The tree's values are staged in LDS (LDS false: more than
// kRefitValueLdsLeaves leaves, read from global memory)
template <typename LT, bool LDS>
__global__ __launch_bounds__(kRefitThreads) void k_refit_add_leaf_values(RefitAddArgs a) {
  extern __shared__ double vals[];
  const int L = a.num_leaves;
  if (LDS) {
    for (int j = threadIdx.x; j < L; j += kRefitThreads) vals[j] = a.values[j];
    __syncthreads();
  }
  const double* v = LDS ? vals : a.values;
  const LT* leaf = static_cast<const LT*>(a.leaf);
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRefitThreads) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kRefitThreads) {
    const uint32_t l = static_cast<uint32_t>(leaf[i]);
    if (l < static_cast<uint32_t>(L)) a.score[i] += v[l];
  }
}

void RefitAddLeafValues(const RefitAddArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const int L = a.num_leaves;
  // a few rows per thread, so that a workgroup's staging of the values is shared by more rows
  const dim3 grid(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((a.n + 1023) / 1024, 8 * NumCUs()))));
  const dim3 block(kRefitThreads);
  if (L <= kRefitValueLdsLeaves) {
    const size_t lds = static_cast<size_t>(L) * sizeof(double);
    if (a.wide) {
      hipLaunchKernelGGL((k_refit_add_leaf_values<int32_t, true>), grid, block, lds, s, a);
    } else {
      hipLaunchKernelGGL((k_refit_add_leaf_values<uint16_t, true>), grid, block, lds, s, a);
    }
  } else if (a.wide) {
    hipLaunchKernelGGL((k_refit_add_leaf_values<int32_t, false>), grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL((k_refit_add_leaf_values<uint16_t, false>), grid, block, 0, s, a);
  }
}

}  // namespace dev
}  // namespace lgbm_amd
