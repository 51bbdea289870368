// The first step of the bin finder on the device: the distinct values of every column of the bin
// sample (BinMapper::SampleDistinct; the rule in src/device/sample_distinct.h), from the
// column-major doubles that k_gather_sample leaves in device memory.  The host's boundary search
// (BinMapper::FindBinFromDistinct) sees only the (value, count) pairs that come back.
//
//   k_sample_distinct  one workgroup of 512 threads per column; the column never leaves it.
//     1. compaction   512 entries at a time: zeros and NaNs are dropped and counted (ballot ranks,
//                     a prefix over the eight wave totals), the others become order-preserving
//                     64-bit keys written in place over the column's front -- a tile's writes land
//                     at or before its first entry, behind a barrier after its reads.  The same
//                     read feeds all eight 256-bin digit histograms in LDS (8 KiB, LDS atomics).
//     2. radix sort   least significant digit first, 8 bits per pass, between the column and a
//                     second buffer.  A pass that would move nothing is skipped: one whose
//                     histogram has a single occupied bin, and one whose digit follows from the
//                     key's top bit in every key (0x00 under a set top bit, 0xFF under a clear
//                     one: keys that tie in the higher digits have the same top bit, so such a
//                     digit never decides an order).  The second form is what a narrower element
//                     type needs: a float32 widened to double has 29 zero low bits, a float16 42,
//                     a bfloat16 45, and the key of a negative value inverts them -- a column
//                     with both signs shows 0x00 and 0xFF there.  So 3 (float32) or 5 (the half
//                     types) of the 8 passes go without a kernel per element type.
//                     A pass scans its 256 counters into running bases (one wave, shuffles) and
//                     scatters tiles of 2048 keys (4 per thread, element it * 512 + tid of the
//                     tile, so loads and the ordered part of the stores are coalesced).  The keys
//                     of a tile are ordered by (it, wave, lane); a lane's rank among the lanes of
//                     its wave with the same digit comes from eight ballots (one per digit bit),
//                     the first of each such set posts the set's size at s_rank[it * 8 + wave]
//                     [digit], and 256 threads turn each digit's column of those 32 counts into
//                     absolute offsets while advancing the running base.  So the scatter is stable
//                     without any atomics, and a column is sorted the same way on every run.
//     3. runs         512 sorted keys at a time: a key that differs from its predecessor by more
//                     than one opens a run (the shared predicate); a block scan of the flags
//                     numbers the runs; the last key of a run writes the run's value into the
//                     other buffer and the first its position, from which a last sweep forms the
//                     lengths.
//   k_pack_distinct    the columns' runs one behind the other, so that only nd values and counts
//                     per column cross to the host
//
// Sizes: 8 KiB of histograms, 32 KiB of rank counters, 1 KiB of bases, 41 KiB in all, inside the
// 64 KiB a workgroup gets without opting in; the 160 KiB of a gfx950 CU hold three such workgroups
// (24 waves).  200 000 keys (the default
// bin_construct_sample_cnt) are 1.6 MB per buffer, so a pass's reads and writes stay in L2 /
// Infinity Cache.  Any sample size is handled; positions are int32 as the sample's indices are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "bin_find.h"
#include "device_common.h"
#include "lgbm_amd/device_binning.h"
#include "lgbm_amd/log.h"
#include "sample_distinct.h"

namespace lgbm_amd {

namespace {

#define BINFINDCHECK(x)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) Log::Fatal("HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

using dev::kWave;

constexpr int kSortThreads = 512;  // also the tile of the compaction and of the run pass
constexpr int kSortWaves = kSortThreads / kWave;
constexpr int kSortItems = 4;  // keys of a thread in a scatter tile
constexpr int kSortTile = kSortThreads * kSortItems;
constexpr int kSortRows = kSortItems * kSortWaves;  // (it, wave) pairs of a tile, in key order
constexpr int kDigits = 256;
constexpr int kPackThreads = 256;

// what a column's header holds
enum { kHdrRuns = 0, kHdrNaN = 1, kHdrKept = 2, kHdrInAlt = 3, kHdrPasses = 4, kHdrWords = 5 };

// lanes of `mask` below this one
__device__ __forceinline__ int RankInMask(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// the sum of s_wave[0 .. w) and of all kSortWaves entries
__device__ __forceinline__ void WavePrefix(const int* s_wave, int w, int* before, int* total) {
  int b = 0, t = 0;
  for (int j = 0; j < kSortWaves; ++j) {
    const int v = s_wave[j];
    if (j < w) b += v;
    t += v;
  }
  *before = b;
  *total = t;
}

__global__ __launch_bounds__(kSortThreads) void k_sample_distinct(unsigned long long* vals, unsigned long long* alt,
                                                                  int32_t* counts, int32_t* hdr, int ns) {
  __shared__ int s_hist[dev::kSampleKeyPasses][kDigits];
  __shared__ int s_rank[kSortRows][kDigits];
  __shared__ int s_base[kDigits];
  __shared__ int s_wave[2][kSortWaves];
  __shared__ int s_fill[dev::kSampleKeyPasses];  // keys whose digit is the one their top bit implies
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  const size_t col = static_cast<size_t>(blockIdx.x) * static_cast<size_t>(ns);
  unsigned long long* src = vals + col;
  unsigned long long* dst = alt + col;
  int32_t* cnt = counts + col;

  for (int j = tid; j < dev::kSampleKeyPasses * kDigits; j += kSortThreads) (&s_hist[0][0])[j] = 0;
  if (tid < dev::kSampleKeyPasses) s_fill[tid] = 0;
  __syncthreads();

  // ---- 1. keys of the entries that stay, in place; NaNs counted; the eight histograms
  int n = 0, na = 0;
  for (int base = 0; base < ns; base += kSortThreads) {
    const int i = base + tid;
    const double v = i < ns ? __longlong_as_double(static_cast<long long>(src[i])) : 0.0;
    const bool is_nan = dev::SampleIsNaN(v);
    const bool keep = !is_nan && dev::SampleKeeps(v);
    const unsigned long long m_keep = __ballot(keep), m_nan = __ballot(is_nan);
    if (lane == 0) {
      s_wave[0][w] = __popcll(m_keep);
      s_wave[1][w] = __popcll(m_nan);
    }
    const unsigned long long key = dev::SampleKey(v);
    for (int p = 0; p < dev::kSampleKeyPasses - 1; ++p) {
      const unsigned long long m = __ballot(keep && dev::SampleKeyDigit(key, p) == dev::SampleKeyFill(key));
      if (lane == 0 && m != 0ull) atomicAdd(&s_fill[p], __popcll(m));
    }
    __syncthreads();  // (every entry of the tile is read)
    int before, total, nan_before, nan_total;
    WavePrefix(s_wave[0], w, &before, &total);
    WavePrefix(s_wave[1], w, &nan_before, &nan_total);
    if (keep) {
      src[n + before + RankInMask(m_keep, lane)] = key;
      for (int p = 0; p < dev::kSampleKeyPasses; ++p) atomicAdd(&s_hist[p][dev::SampleKeyDigit(key, p)], 1);
    }
    n += total;
    na += nan_total;
    __syncthreads();  // (s_wave is read)
  }

  // ---- 2. the passes that move something
  int passes = 0;
  for (int p = 0; p < dev::kSampleKeyPasses; ++p) {
    const bool one_digit = __syncthreads_or(tid < kDigits && s_hist[p][tid] == n);  // (or no key at all)
    if (one_digit || (p < dev::kSampleKeyPasses - 1 && s_fill[p] == n)) continue;
    ++passes;
    if (w == 0) {
      int c[kDigits / kWave], sum = 0;
      for (int j = 0; j < kDigits / kWave; ++j) {
        c[j] = s_hist[p][lane * (kDigits / kWave) + j];
        sum += c[j];
      }
      int incl = sum;
      for (int o = 1; o < kWave; o <<= 1) {
        const int t = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += t;
      }
      int run = incl - sum;
      for (int j = 0; j < kDigits / kWave; ++j) {
        s_base[lane * (kDigits / kWave) + j] = run;
        run += c[j];
      }
    }
    for (int tb = 0; tb < n; tb += kSortTile) {
      for (int j = tid; j < kSortRows * kDigits; j += kSortThreads) (&s_rank[0][0])[j] = 0;
      __syncthreads();  // (... and s_base is written)
      unsigned long long key[kSortItems];
      int rank[kSortItems];
      for (int it = 0; it < kSortItems; ++it) {
        const int i = tb + it * kSortThreads + tid;
        const bool valid = i < n;
        key[it] = valid ? src[i] : 0ull;
        const int d = dev::SampleKeyDigit(key[it], p);
        unsigned long long peers = __ballot(valid);  // the valid lanes of the wave with this digit
        for (int b = 0; b < 8; ++b) {
          const bool bit = ((d >> b) & 1) != 0;
          const unsigned long long m = __ballot(bit);
          peers &= bit ? m : ~m;
        }
        rank[it] = valid ? RankInMask(peers, lane) : -1;
        if (rank[it] == 0) s_rank[it * kSortWaves + w][d] = __popcll(peers);
      }
      __syncthreads();
      if (tid < kDigits) {
        int run = s_base[tid];
        for (int r = 0; r < kSortRows; ++r) {
          const int c = s_rank[r][tid];
          s_rank[r][tid] = run;
          run += c;
        }
        s_base[tid] = run;
      }
      __syncthreads();
      for (int it = 0; it < kSortItems; ++it) {
        if (rank[it] >= 0) dst[s_rank[it * kSortWaves + w][dev::SampleKeyDigit(key[it], p)] + rank[it]] = key[it];
      }
      __syncthreads();  // (s_rank is read; the keys are written before the next pass reads them)
    }
    unsigned long long* t = src;
    src = dst;
    dst = t;
  }

  // ---- 3. runs: values into dst, first positions into cnt
  __syncthreads();
  int nd = 0;
  for (int base = 0; base < n; base += kSortThreads) {
    const int i = base + tid;
    const bool valid = i < n;
    const unsigned long long key = valid ? src[i] : 0ull;
    const bool start = valid && (i == 0 || dev::SampleOpensRun(src[i - 1], key));
    const bool last = valid && (i == n - 1 || dev::SampleOpensRun(key, src[i + 1]));
    const unsigned long long m = __ballot(start);
    if (lane == 0) s_wave[0][w] = __popcll(m);
    __syncthreads();
    int before, total;
    WavePrefix(s_wave[0], w, &before, &total);
    const int run = nd + before + RankInMask(m, lane) + (start ? 1 : 0) - 1;  // the run this key is in
    if (start) cnt[run] = i;
    if (last) dst[run] = static_cast<unsigned long long>(__double_as_longlong(dev::SampleKeyValue(key)));
    nd += total;
    __syncthreads();
  }
  // first positions into lengths
  for (int base = 0; base < nd; base += kSortThreads) {
    const int r = base + tid;
    int len = 0;
    if (r < nd) len = (r + 1 < nd ? cnt[r + 1] : n) - cnt[r];
    __syncthreads();  // (the next run's position is read before that run's length replaces it)
    if (r < nd) cnt[r] = len;
  }
  if (tid == 0) {
    int32_t* h = hdr + static_cast<size_t>(blockIdx.x) * kHdrWords;
    h[kHdrRuns] = nd;
    h[kHdrNaN] = na;
    h[kHdrKept] = n;
    h[kHdrInAlt] = dst == alt + col ? 1 : 0;
    h[kHdrPasses] = passes;
  }
}

// run i = (blockIdx.x % ntiles) * 256 + threadIdx.x of column blockIdx.x / ntiles to off[column] + i
// of the packed lists
__global__ __launch_bounds__(kPackThreads) void k_pack_distinct(const double* vals, const double* alt,
                                                                const int32_t* counts, const int32_t* hdr,
                                                                const long long* off, int ns, int ntiles,
                                                                double* out_d, int32_t* out_c) {
  const int c = static_cast<int>(blockIdx.x / ntiles);
  const int32_t* h = hdr + static_cast<size_t>(c) * kHdrWords;
  const int i = static_cast<int>(blockIdx.x % ntiles) * kPackThreads + threadIdx.x;
  if (i >= h[kHdrRuns]) return;
  const size_t at = static_cast<size_t>(c) * static_cast<size_t>(ns) + i;
  out_d[off[c] + i] = (h[kHdrInAlt] != 0 ? alt : vals)[at];
  out_c[off[c] + i] = counts[at];
}

template <typename T>
T* DeviceAlloc(size_t n) {
  void* p = nullptr;
  BINFINDCHECK(hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)));
  return static_cast<T*>(p);
}

std::atomic<int64_t> g_bin_find_calls{0};

}  // namespace

void NoteDeviceBinFind() { g_bin_find_calls.fetch_add(1, std::memory_order_relaxed); }
int64_t DeviceBinFindCalls() { return g_bin_find_calls.load(std::memory_order_relaxed); }

void BinFindLaunchInfo(int64_t* out) {
  out[0] = kSortTile;
  out[1] = kSortThreads;
  out[2] = kSortThreads;  // the tile of the compaction and of the run pass
  out[3] = kBinFindMinSampleRows;
  out[4] = kBinFindMaxSampleValues;
}

DeviceSampleDistinct::DeviceSampleDistinct(int max_cols, int ns) : max_cols_(max_cols), ns_(ns) {
  const size_t cells = static_cast<size_t>(max_cols) * static_cast<size_t>(ns);
  d_alt_ = DeviceAlloc<uint64_t>(cells);
  d_counts_ = DeviceAlloc<int32_t>(cells);
  d_hdr_ = DeviceAlloc<int32_t>(static_cast<size_t>(max_cols) * kHdrWords);
  d_off_ = DeviceAlloc<long long>(static_cast<size_t>(max_cols));
}

DeviceSampleDistinct::~DeviceSampleDistinct() {
  (void)hipFree(d_alt_);
  (void)hipFree(d_counts_);
  (void)hipFree(d_hdr_);
  (void)hipFree(d_off_);
  (void)hipFree(d_pack_d_);
  (void)hipFree(d_pack_c_);
}

void DeviceSampleDistinct::Launch(double* d_vals, int nc) {
  if (nc > max_cols_) Log::Fatal("bin finder: %d columns in a pass of %d", nc, max_cols_);
  d_vals_ = d_vals;
  nc_ = nc;
  hipLaunchKernelGGL(k_sample_distinct, dim3(static_cast<unsigned>(nc)), dim3(kSortThreads), 0, 0,
                     reinterpret_cast<unsigned long long*>(d_vals), reinterpret_cast<unsigned long long*>(d_alt_),
                     d_counts_, d_hdr_, ns_);
  BINFINDCHECK(hipGetLastError());
}

void DeviceSampleDistinct::Collect(SampleDistinctLists* out) {
  std::vector<int32_t> hdr(static_cast<size_t>(nc_) * kHdrWords);
  BINFINDCHECK(hipMemcpy(hdr.data(), d_hdr_, sizeof(int32_t) * hdr.size(), hipMemcpyDeviceToHost));
  std::vector<long long> off(static_cast<size_t>(nc_));
  int64_t total = 0;
  int most = 0;
  for (int c = 0; c < nc_; ++c) {
    const int nd = hdr[static_cast<size_t>(c) * kHdrWords + kHdrRuns];
    off[c] = total;
    total += nd;
    most = std::max(most, nd);
    out->begin.push_back(out->begin.back() + nd);
    out->nan_cnt.push_back(hdr[static_cast<size_t>(c) * kHdrWords + kHdrNaN]);
    out->num_values.push_back(hdr[static_cast<size_t>(c) * kHdrWords + kHdrKept]);
    out->sort_passes.push_back(hdr[static_cast<size_t>(c) * kHdrWords + kHdrPasses]);
  }
  if (total == 0) return;
  if (total > pack_cap_) {
    (void)hipFree(d_pack_d_);
    (void)hipFree(d_pack_c_);
    d_pack_d_ = nullptr;
    d_pack_c_ = nullptr;
    d_pack_d_ = DeviceAlloc<double>(static_cast<size_t>(total));
    d_pack_c_ = DeviceAlloc<int32_t>(static_cast<size_t>(total));
    pack_cap_ = total;
  }
  BINFINDCHECK(hipMemcpy(d_off_, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice));
  const int64_t ntiles = (most + kPackThreads - 1) / kPackThreads;
  if (ntiles * nc_ > 0x7fffffffLL) Log::Fatal("bin finder: %d columns of up to %d runs are too many for a pass", nc_, most);
  hipLaunchKernelGGL(k_pack_distinct, dim3(static_cast<unsigned>(ntiles * nc_)), dim3(kPackThreads), 0, 0, d_vals_,
                     reinterpret_cast<const double*>(d_alt_), d_counts_, d_hdr_, d_off_, ns_, static_cast<int>(ntiles),
                     d_pack_d_, d_pack_c_);
  BINFINDCHECK(hipGetLastError());
  const size_t at = out->distinct.size();
  out->distinct.resize(at + static_cast<size_t>(total));
  out->counts.resize(at + static_cast<size_t>(total));
  BINFINDCHECK(hipMemcpy(out->distinct.data() + at, d_pack_d_, sizeof(double) * static_cast<size_t>(total), hipMemcpyDeviceToHost));
  BINFINDCHECK(hipMemcpy(out->counts.data() + at, d_pack_c_, sizeof(int32_t) * static_cast<size_t>(total), hipMemcpyDeviceToHost));
}

}  // namespace lgbm_amd
