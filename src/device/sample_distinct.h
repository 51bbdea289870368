// The distinct values of one column of the bin sample (src/device/bin_find_kernels.hip; host
// evaluator for tests without a GPU: LGBM_AMD_SampleDistinct).  The rule of one column, shared by
// the kernels and the evaluator, states what BinMapper::FindBin does to its sample before the
// boundary search (BinMapper::SampleDistinct after the filter of the row readers):
//   - an entry with |v| <= kZeroThreshold (the float 1e-35f, -0.0 included) is a zero and is
//     dropped (DenseRowPairFun); a NaN is counted and dropped;
//   - the rest is sorted ascending: by the 64-bit key below, an order-preserving image of a double;
//   - a new run opens where !CheckDoubleEqualOrdered(v[i - 1], v[i]), that is where
//     v[i] > nextafter(v[i - 1], inf).  On sorted keys without zeros and NaNs that is a key
//     difference above 1 (DBL_MAX and inf are neighbours and merge; -0.0 / +0.0, the one place
//     where neighbouring keys are not neighbouring doubles, never get here);
//   - a run's value is its last, hence largest, element, its count the run's length.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "stored_order.h"

namespace lgbm_amd {
namespace dev {

constexpr double kSampleZeroThreshold = 1e-35f;  // kZeroThreshold

LGBM_AMD_HD bool SampleIsNaN(double v) { return v != v; }
// whether the sample keeps v (a NaN is kept by the row readers and counted apart here)
LGBM_AMD_HD bool SampleKeeps(double v) { return (v < 0 ? -v : v) > kSampleZeroThreshold; }

// a < b as doubles <=> SampleKey(a) < SampleKey(b) as unsigned (neither a NaN)
LGBM_AMD_HD uint64_t SampleKey(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return (b >> 63) != 0 ? ~b : b | 0x8000000000000000ull;
}
LGBM_AMD_HD double SampleKeyValue(uint64_t k) {
  const uint64_t b = (k >> 63) != 0 ? k & 0x7fffffffffffffffull : ~k;
  double v;
  __builtin_memcpy(&v, &b, sizeof(v));
  return v;
}
// whether `next` (>= prev) opens a new run after `prev`
LGBM_AMD_HD bool SampleOpensRun(uint64_t prev, uint64_t next) { return next - prev > 1; }

constexpr int kSampleKeyPasses = 8;  // 8-bit digits of a key, lowest first
LGBM_AMD_HD int SampleKeyDigit(uint64_t k, int pass) { return static_cast<int>((k >> (8 * pass)) & 255u); }
// the digit that the zero low bits of a widened narrower type (29 of a float32, 42 of a float16,
// 45 of a bfloat16) become: 0x00 in the key of a positive value, 0xFF in that of a negative one.
// Where every key of a column shows it in a digit, that digit follows from the top bit and the
// sort may skip its pass.
LGBM_AMD_HD int SampleKeyFill(uint64_t k) { return (k >> 63) != 0 ? 0 : 255; }

// the rule on the host: column `col` of n entries into distinct / counts; returns the NaN count
inline int EvalSampleDistinct(const double* col, int64_t n, std::vector<double>* distinct, std::vector<int32_t>* counts) {
  std::vector<uint64_t> keys;
  int na = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (SampleIsNaN(col[i])) ++na;
    else if (SampleKeeps(col[i])) keys.push_back(SampleKey(col[i]));
  }
  std::sort(keys.begin(), keys.end());
  distinct->clear();
  counts->clear();
  for (size_t i = 0; i < keys.size(); ++i) {
    if (i == 0 || SampleOpensRun(keys[i - 1], keys[i])) {
      distinct->push_back(SampleKeyValue(keys[i]));
      counts->push_back(1);
    } else {
      distinct->back() = SampleKeyValue(keys[i]);
      ++counts->back();
    }
  }
  return na;
}

}  // namespace dev
}  // namespace lgbm_amd
