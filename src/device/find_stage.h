// What the two split-scan kernels -- k_find (split_kernels.hip, one split per step) and
// k_round_find (round_find.hip, round growth) -- do around the scan proper (split_scan.h), once:
// the histogram materialisation, the finished LeafCtx, the empty per-feature records, the scans'
// LDS, the CEGB delta, the launch ladder and the single-counter hand-off.  The kernels keep what
// differs between them: their control records (Step against Round / ExpPlan), skip rules,
// extra_trees handling and publication.
#pragma once

#include <type_traits>

#include "split_scan.h"

namespace lgbm_amd {
namespace dev {
namespace {

#ifndef LGBM_FIND_WAVE_OCC
// one-wave split scans: waves per SIMD the register budget allows.  2 (256 VGPRs): at 4 the
// non-root kernels spilled 72-76 bytes per lane, and trees grown with them changed with
// unrelated code edits (one-split-per-step categorical trees, voting ranks that disagreed)
// while the spill-free build stayed exact -- tests/test_gpu_distributed.py voting cases
#define LGBM_FIND_WAVE_OCC 2
#endif

// a scan workgroup's LDS next to the staged bins (NT threads; KIND 2 / 3: the categorical scans)
template <int KIND, int NT>
struct ScanShared {
  BlockScratch<NT> sc;
  ScanScratch<NT> ssc;
  Cand sc2[NT / kWave];
  typename std::conditional<KIND == 2, CatScratchT<kFindCatNarrow>,
                            typename std::conditional<KIND == 3, CatScratchT<kFindMaxCatBins>, int>::type>::type cat_sc;
  unsigned long long s_red[2 * NT];  // direct partial sums of narrow features
};

// a feature's result before its scan: no split, no flag written (-1); the caller names the feature
__device__ __forceinline__ FeatureBest FeatureBestEmpty() {
  FeatureBest o;
  o.gain = -INFINITY;
  o.feature = -1;
  o.real_feature = -1;
  o.thr = 0;
  o.default_left = 1;
  o.lc = o.rc = 0;
  o.mono = 0;
  o.ncat = 0;
  o.flag = -1;
  o.pad = 0;
  o.lg = o.lh = o.rg = o.rh = o.lo = o.ro = 0.0;
  return o;
}
// "not evaluated": no feature, everything else zero (flag 0, where the empty record has -1)
__device__ __forceinline__ FeatureBest FeatureBestNone() {
  FeatureBest none = {};
  none.gain = -INFINITY;
  none.feature = none.real_feature = -1;
  return none;
}

// the leaf's sums, count, range and parent output are set: what the scans derive from them
__device__ __forceinline__ void FinishLeafCtx(LeafCtx* L, const SplitParams& p) {
  L->cnt_factor = L->n / L->sh;
  const double gain_shift = LeafGain(L->sg, L->sh, p.lambda_l1, p.lambda_l2, p.max_delta_step, p.path_smooth, L->n,
                                     L->parent_out, p.use_l1, p.use_max_output, p.use_smoothing);
  L->min_gain_shift = gain_shift + p.min_gain_to_split;
}

// CEGB: what a split of n rows on f costs -- the split penalty, and the coupled one while the
// model has not used f (the lazy penalty is k_find's alone)
__device__ __forceinline__ double CegbScanDelta(const KArgs& a, int f, int n) {
  double delta = a.p.cegb_split * n;
  if (a.cegb_coupled != nullptr && !a.cegb_used[f]) delta += a.cegb_coupled[f];
  return delta;
}

// Materialises one feature's histogram of one leaf (nbf stored bins, interleaved int64 (g, h)) in
// dst and, with `stage`, dequantised by ig / ih in sg / shv (LDS).  The bins come from
//   nblk_direct >= 0: the sum of that many per-block partials at `part` (pstride words apart,
//                     `units` words per bin) -- a small leaf, whose partials no reduce kernel summed;
//   nblk_direct < 0:  src, the reduced histogram (src == dst: read in place);
// subtract: dst holds the parent's bins and becomes the parent minus those, in place (exact int64).
// STORE false: dst is left as it is (only staged) -- a template argument, so that no instantiation
// carries the branch.  Every thread of the workgroup calls it; it ends with the barrier that makes
// the stores visible to all of them.
template <int NT, bool STORE>
__device__ __forceinline__ void StageHistogram(long long* dst, const long long* src, const unsigned long long* part,
                                               const size_t pstride, const int units, const int nbf,
                                               const int nblk_direct, const bool subtract, const double ig,
                                               const double ih, const bool stage, double* sg, double* shv,
                                               unsigned long long* s_red) {
  const int tid = threadIdx.x;
  // (s_red is LDS, and typed so: through a plain pointer argument its reads were merged with
  // those of src into loads from a pointer picked at run time, flat instead of LDS and global)
  typedef __attribute__((address_space(3))) unsigned long long LdsU64;
  LdsU64* red = (LdsU64*)s_red;
  // a feature with fewer bins than threads sums its direct partials with every thread:
  // NT / nbf threads per bin stride over the row blocks, then combine in LDS
  // (one thread per bin walking hundreds of partials would be a chain of round trips)
  const bool spread = nblk_direct > 1 && 2 * nbf <= NT;
  // the parent's bins (first bin of each thread): loaded up front, so their round trip
  // overlaps the partial-sum loads instead of following them
  long long pg0 = 0, ph0 = 0;
  if (subtract && tid < nbf) {
    pg0 = dst[2 * tid];
    ph0 = dst[2 * tid + 1];
  }
  if (spread) {
    for (int j = tid; j < 2 * nbf; j += NT) red[j] = 0ull;
    __syncthreads();
    const int per = NT / nbf;
    const int i = tid % nbf, r = tid / nbf;
    if (r < per) {
      constexpr int kC = 8;
      long long g = 0, h = 0;
      for (int k0 = r; k0 < nblk_direct; k0 += per * kC) {
        unsigned long long v0[kC], v1[kC];
#pragma unroll
        for (int cc = 0; cc < kC; ++cc) {
          const int k = k0 + cc * per;
          const unsigned long long* q = part + k * pstride + static_cast<size_t>(units) * i;
          v0[cc] = k < nblk_direct ? q[0] : 0ull;
          v1[cc] = (k < nblk_direct && units == 2) ? q[1] : 0ull;
        }
#pragma unroll
        for (int cc = 0; cc < kC; ++cc) {
          long long pgv, phv;
          UnpackPartial(v0[cc], v1[cc], units, &pgv, &phv);
          g += pgv;
          h += phv;
        }
      }
      atomicAdd((unsigned long long*)&red[2 * i], static_cast<unsigned long long>(g));
      atomicAdd((unsigned long long*)&red[2 * i + 1], static_cast<unsigned long long>(h));
    }
    __syncthreads();
  }
  for (int i = tid; i < nbf; i += NT) {
    long long g = 0, h = 0;
    if (spread) {
      g = static_cast<long long>(red[2 * i]);
      h = static_cast<long long>(red[2 * i + 1]);
    } else if (nblk_direct >= 0) {
      // small leaf: sum the few per-block partials here (the reduce kernel skipped them),
      // chunks of kDirectChunk independent loads in flight
      for (int k0 = 0; k0 < nblk_direct; k0 += kDirectChunk) {
        unsigned long long v0[kDirectChunk], v1[kDirectChunk];
#pragma unroll
        for (int k = 0; k < kDirectChunk; ++k) {
          const unsigned long long* q = part + (k0 + k) * pstride + static_cast<size_t>(units) * i;
          v0[k] = k0 + k < nblk_direct ? q[0] : 0ull;
          v1[k] = (k0 + k < nblk_direct && units == 2) ? q[1] : 0ull;
        }
#pragma unroll
        for (int k = 0; k < kDirectChunk; ++k) {
          long long pgv, phv;
          UnpackPartial(v0[k], v1[k], units, &pgv, &phv);
          g += pgv;
          h += phv;
        }
      }
    } else {
      g = src[2 * i];
      h = src[2 * i + 1];
    }
    if (subtract) {
      g = (i == tid ? pg0 : dst[2 * i]) - g;
      h = (i == tid ? ph0 : dst[2 * i + 1]) - h;
    }
    if (STORE) {
      dst[2 * i] = g;
      dst[2 * i + 1] = h;
    }
    if (stage) {
      sg[i] = static_cast<double>(g) * ig;
      shv[i] = static_cast<double>(h) * ih;
    }
  }
  __syncthreads();  // the workgroup's stores become visible to all its threads
}

// "the last one goes on": every workgroup of a set of n counts once on `counter` after its
// write-through stores (PublishRecord) have drained; the last to arrive resets the counter for
// the next launch, takes one agent-scope acquire for the workgroup and returns true to all its
// threads.  (The two-level arrival counters of the scans have reset protocols of their own.)
__device__ __forceinline__ bool LastOfCount(uint32_t* counter, const unsigned n, int* s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ArrivalRelease();
  __syncthreads();
  if (threadIdx.x == 0) {
    int last = 0;
    if (atomicAdd(counter, 1u) == n - 1) {
      last = 1;
      *counter = 0u;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_last = last;
  }
  __syncthreads();
  return *s_last != 0;
}

// ---- host side: what the launches of both kernels decide alike

// plain gain formulas (no L1 / max_delta_step / path smoothing / monotone constraints)
__host__ __device__ __forceinline__ bool SimpleGains(const SplitParams& p) {
  return !p.use_l1 && !p.use_max_output && !p.use_smoothing && !p.use_mc;
}

// dynamic LDS of the staged bins: [2][max_feature_bins] doubles, if they fit
inline size_t FindBinsLds(const KArgs& a) {
  return a.p.max_feature_bins <= kFindLdsBins ? 2 * sizeof(double) * static_cast<size_t>(a.p.max_feature_bins) : 0;
}

// The scans' launch ladder: fn(KIND, SIMPLE, NT), as std::integral_constants, for the numerical
// kernel -- KIND 0, or 1 when the data has categorical features; SIMPLE by SimpleGains; NT one wave
// when every feature has at most kWave stored bins, else kFindThreads -- and then, with
// categorical features, for their kernel (KIND 2, or 3 the wide variant; never SIMPLE, always
// kFindThreads).
template <class Fn>
void DispatchScans(const KArgs& a, Fn&& fn) {
  using std::integral_constant;
  const bool simple = SimpleGains(a.p.sp);
  const bool narrow = a.p.max_feature_bins <= kWave;
  auto numerical = [&](auto kind) {
    auto with_nt = [&](auto nt) {
      if (simple) fn(kind, std::true_type{}, nt);
      else fn(kind, std::false_type{}, nt);
    };
    if (narrow) with_nt(integral_constant<int, kWave>{});
    else with_nt(integral_constant<int, kFindThreads>{});
  };
  if (!a.p.has_cat) {
    numerical(integral_constant<int, 0>{});
    return;
  }
  numerical(integral_constant<int, 1>{});
  if (a.p.wide_cat) fn(integral_constant<int, 3>{}, std::false_type{}, integral_constant<int, kFindThreads>{});
  else fn(integral_constant<int, 2>{}, std::false_type{}, integral_constant<int, kFindThreads>{});
}

}  // namespace
}  // namespace dev
}  // namespace lgbm_amd
