// The objective's output transform of one row of raw scores (ObjectiveFunction::ConvertOutput in
// the device-evaluable forms of ObjectiveFunction::DeviceOutputKind), shared by the export kernel
// (src/device/custom_kernels.hip k_export_scores) and a host evaluator for tests without a GPU
// (LGBM_AMD_ConvertScores).  Scores are class-major: class k of row i is at [k * n + i].
//   0 identity                    (regression family)
//   1 1 / (1 + exp(-param * s))   (binary, cross_entropy with param 1)
//   2 sign(s) * s * s             (regression with reg_sqrt)
//   3 exp(s)                      (poisson, gamma, tweedie)
//   4 softmax over the row's classes: the maximum, exp(s - max) summed in class order, each
//     divided by the sum (common::Softmax)
//   5 kind 1 on every class       (multiclassova)
// The arithmetic is the host objectives', operation for operation (the 1.0f literals of the
// sigmoids are promoted to double there too), so on one exp the results are the same bits.
#pragma once

#include <cmath>
#include <cstdint>

// (a plain C++ program can include this header: tests/native/score_convert_driver.cpp)
#include "stored_order.h"

namespace lgbm_amd {
namespace dev {

constexpr int kConvertKinds = 6;

// the kinds that transform each score on its own
LGBM_AMD_HD double ConvertScoreValue(int kind, double param, double s) {
  switch (kind) {
    case 1:
    case 5:
      return 1.0f / (1.0f + std::exp(-param * s));
    case 2:
      return ((s > 0.0) - (s < 0.0)) * s * s;
    case 3:
      return std::exp(s);
    default:
      return s;
  }
}

// row i of `in` ([num_class][n]) into row i of `out` (same layout; out may be `in`)
LGBM_AMD_HD void ConvertScoreRow(int kind, double param, int num_class, int64_t n, int64_t i, const double* in,
                                 double* out) {
  if (kind != 4) {
    for (int k = 0; k < num_class; ++k) out[k * n + i] = ConvertScoreValue(kind, param, in[k * n + i]);
    return;
  }
  double mx = in[i];
  for (int k = 1; k < num_class; ++k) {
    const double v = in[k * n + i];
    mx = mx < v ? v : mx;  // (std::max)
  }
  double sum = 0.0;
  for (int k = 0; k < num_class; ++k) {
    const double e = std::exp(in[k * n + i] - mx);
    out[k * n + i] = e;
    sum += e;
  }
  for (int k = 0; k < num_class; ++k) out[k * n + i] /= sum;
}

// the host evaluator: every row of in[num_class][n] into out[num_class][n]
inline void EvalConvertScores(int kind, double param, int num_class, int64_t n, const double* in, double* out) {
  for (int64_t i = 0; i < n; ++i) ConvertScoreRow(kind, param, num_class, n, i, in, out);
}

}  // namespace dev
}  // namespace lgbm_amd
