// Custom objectives and metrics on device tensors: the learner's scores out to a caller's
// buffer (k_export_scores, optionally through the objective's output transform of
// score_convert.h) and a caller's gradients / hessians of any floating dtype into the learner's
// float arrays (k_ingest_gradients).  Both walk flat class-major arrays with 64-bit indices on a
// grid-stride loop, kCustomPerThread independent loads in flight per thread as k_gradients has;
// every element is bounded by the length, so a caller's buffer needs no padding or alignment
// beyond its element's.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "device_common.h"
#include "score_convert.h"

namespace lgbm_amd {
namespace dev {

// raw copy, or a transform of each score on its own (every kind but the softmax)
__global__ __launch_bounds__(kCustomThreads) void k_export_scores(ExportArgs a) {
  const int64_t len = a.n * a.num_class;
  const int kind = a.convert != 0 ? a.kind : 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t base = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; base < len;
       base += kCustomPerThread * stride) {
    double v[kCustomPerThread];
#pragma unroll
    for (int k = 0; k < kCustomPerThread; ++k) {
      const int64_t i = base + k * stride;
      v[k] = i < len ? a.score[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kCustomPerThread; ++k) {
      const int64_t i = base + k * stride;
      if (i < len) a.out[i] = ConvertScoreValue(kind, a.param, v[k]);
    }
  }
}

// the softmax: a thread per row, its classes n apart
__global__ __launch_bounds__(kCustomThreads) void k_export_scores_rows(ExportArgs a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < a.n; i += stride) {
    ConvertScoreRow(a.kind, a.param, a.num_class, a.n, i, a.score, a.out);
  }
}

int CustomGridCap() { return 8 * NumCUs(); }

// workgroups for `len` elements, kCustomPerThread to a thread per loop trip
static int CustomGrid(int64_t len) { return GridFor((len + kCustomPerThread - 1) / kCustomPerThread); }

void ExportScores(const ExportArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.num_class <= 0) return;
  if (a.convert != 0 && a.kind == 4) {
    hipLaunchKernelGGL(k_export_scores_rows, dim3(GridFor(a.n)), dim3(kCustomThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_export_scores, dim3(CustomGrid(a.n * a.num_class)), dim3(kCustomThreads), 0, s, a);
  }
}

// an element of the caller's dtype as the float `tensor.to(torch.float32)` gives: float64 rounds
// to nearest-even (overflow to +-inf, -0.0 and subnormals kept), the 16-bit types widen exactly
__device__ __forceinline__ float ToFloat(float x) { return x; }
__device__ __forceinline__ float ToFloat(double x) { return static_cast<float>(x); }
__device__ __forceinline__ float ToFloat(__half x) { return __half2float(x); }
__device__ __forceinline__ float ToFloat(__hip_bfloat16 x) { return __bfloat162float(x); }

template <typename T>
__global__ __launch_bounds__(kCustomThreads) void k_ingest_gradients(IngestArgs a) {
  const T* __restrict__ g = static_cast<const T*>(a.grad);
  const T* __restrict__ h = static_cast<const T*>(a.hess);
  const int64_t len = a.len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t base = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; base < len;
       base += kCustomPerThread * stride) {
    float gv[kCustomPerThread], hv[kCustomPerThread];
#pragma unroll
    for (int k = 0; k < kCustomPerThread; ++k) {
      const int64_t i = base + k * stride;
      const bool ok = i < len;
      gv[k] = ok ? ToFloat(g[i]) : 0.f;
      hv[k] = ok ? ToFloat(h[i]) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kCustomPerThread; ++k) {
      const int64_t i = base + k * stride;
      if (i < len) {
        a.out_grad[i] = gv[k];
        a.out_hess[i] = hv[k];
      }
    }
  }
}

bool IngestGradients(const IngestArgs& a, hipStream_t s) {
  if (a.len <= 0) return true;
  const dim3 grid(CustomGrid(a.len)), block(kCustomThreads);
  switch (a.dtype) {
    case kGradF32: hipLaunchKernelGGL(k_ingest_gradients<float>, grid, block, 0, s, a); return true;
    case kGradF64: hipLaunchKernelGGL(k_ingest_gradients<double>, grid, block, 0, s, a); return true;
    case kGradF16: hipLaunchKernelGGL(k_ingest_gradients<__half>, grid, block, 0, s, a); return true;
    case kGradBF16: hipLaunchKernelGGL(k_ingest_gradients<__hip_bfloat16>, grid, block, 0, s, a); return true;
    default: return false;
  }
}

}  // namespace dev
}  // namespace lgbm_amd
