// Fixed-point rule of the refit leaf sums (src/device/refit_kernels.hip), shared by the kernels
// and the host evaluator (tests without a GPU: LGBM_AMD_RefitLeafSums).  As the histograms do
// (hist_common.h), a row's g and h are scaled by a power of two and rounded to integers once;
// the per-leaf sums of those integers are exact and do not depend on the order of the rows.
//
// The scale of a component is 2^e, with e the largest exponent for which n * max|x| * 2^e < 2^53
// (so also < 2^62): no partial sum leaves int64, and every sum converts to a double without
// rounding.  Dequantised, a leaf's sum is then off by at most count * 2^-(e + 1), the roundings
// of its rows and nothing else.  With n rows a row keeps 53 - ceil(log2 n) bits below the
// maximum's leading bit: 33 bits at a million rows, more than the 24 of an fp32 gradient.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "forest_decision.h"

namespace lgbm_amd {
namespace dev {

// bits of |x|: non-negative floats order as their bit patterns (NaN above infinity)
LGBM_AMD_HD uint32_t RefitAbsBits(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, sizeof(b));
  return b & 0x7fffffffu;
}

// the exponent e of a component's scale from the bits of max |x| over the n rows.  All-zero (and
// non-finite) maxima give e = 0: a finite scale
LGBM_AMD_HD int RefitScaleExp(uint32_t max_bits, int64_t n) {
  if (max_bits == 0u || max_bits >= 0x7f800000u) return 0;
  int top = 0;  // max < 2^top
  const int be = static_cast<int>(max_bits >> 23);
  if (be != 0) {
    top = be - 126;  // 1.m * 2^(be - 127)
  } else {
    int k = 0;  // a subnormal: m * 2^-149, m < 2^k
    while ((max_bits >> k) != 0u) ++k;
    top = k - 149;
  }
  int b = 0;  // n <= 2^b
  while (b < 62 && (static_cast<int64_t>(1) << b) < n) ++b;
  return 53 - b - top;
}

// 2^e as a double (e within [-160, 210]: a normal number)
LGBM_AMD_HD double RefitScale(int e) {
  const uint64_t bits = static_cast<uint64_t>(1023 + e) << 52;
  double d;
  __builtin_memcpy(&d, &bits, sizeof(d));
  return d;
}

// a row's value in fixed point: the product is exact, the rounding (to nearest, ties to even) is
// the only quantisation.  Non-finite values (their maximum gave e = 0) count as 0
LGBM_AMD_HD long long RefitQuantise(float x, double scale) {
  const double v = static_cast<double>(x) * scale;
  if (!(v > -9.0e15 && v < 9.0e15)) return 0;  // (|finite x| * scale < 2^53 by RefitScaleExp)
  return static_cast<long long>(__builtin_rint(v));
}

// host evaluation of the leaf-sum kernels: sums[0..L) = sum g, sums[L..2L) = sum h (dequantised),
// counts[L], scale_exp[2].  False: a leaf id outside [0, L)
inline bool EvalRefitLeafSums(const int32_t* leaf, const float* grad, const float* hess, int64_t n, int num_leaves,
                              double* sums, int64_t* counts, int32_t* scale_exp) {
  uint32_t mg = 0u, mh = 0u;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t a = RefitAbsBits(grad[i]), b = RefitAbsBits(hess[i]);
    mg = a > mg ? a : mg;
    mh = b > mh ? b : mh;
  }
  const int eg = RefitScaleExp(mg, n), eh = RefitScaleExp(mh, n);
  const double sg = RefitScale(eg), sh = RefitScale(eh);
  for (int l = 0; l < num_leaves; ++l) counts[l] = 0;
  std::vector<long long> q(2 * static_cast<size_t>(num_leaves), 0);
  long long* qg = q.data();
  long long* qh = qg + num_leaves;
  bool ok = true;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t l = leaf[i];
    if (l < 0 || l >= num_leaves) {
      ok = false;
      continue;
    }
    qg[l] += RefitQuantise(grad[i], sg);
    qh[l] += RefitQuantise(hess[i], sh);
    ++counts[l];
  }
  const double ig = RefitScale(-eg), ih = RefitScale(-eh);
  for (int l = 0; l < num_leaves; ++l) {
    const long long a = qg[l], b = qh[l];
    sums[l] = static_cast<double>(a) * ig;
    sums[num_leaves + l] = static_cast<double>(b) * ih;
  }
  scale_exp[0] = eg;
  scale_exp[1] = eh;
  return ok;
}

}  // namespace dev
}  // namespace lgbm_amd
