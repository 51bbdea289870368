// Host-only driver of the objective output transforms (src/device/score_convert.h) for the
// sanitizer test: every kind over class-major scores with 1, 2, 3 and 17 classes and row counts
// around 0 and 64, the edge values of tests/test_score_convert.py (zeros of both signs, tiny and
// subnormal values, +-700, +-745.2, +-inf, NaN), from and into buffers that end exactly where the
// matrix ends, in place and into a second buffer; the two must agree bit for bit, the copy and the
// signed square with the plain formulas, and the rows of a softmax must sum to 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../src/device/score_convert.h"

using lgbm_amd::dev::EvalConvertScores;

static int failures = 0;

static bool SameBits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static void Run(int num_class, int64_t n) {
  const double inf = std::numeric_limits<double>::infinity();
  const double edges[] = {0.0, -0.0, 2.2250738585072014e-308, -2.2250738585072014e-308, 5e-324, -5e-324, 700.0, -700.0,
                          745.2, -745.2, 709.9, -709.9, inf, -inf, NAN, 1.0, -1.0, 36.8, -36.8, 0.5, -3.25};
  const int ne = static_cast<int>(sizeof(edges) / sizeof(edges[0]));
  std::vector<double> in(static_cast<size_t>(num_class) * n);
  for (int k = 0; k < num_class; ++k) {
    for (int64_t i = 0; i < n; ++i) in[k * n + i] = edges[(i * 7 + k * 3 + (i / ne)) % ne];
  }
  for (int kind = 0; kind < lgbm_amd::dev::kConvertKinds; ++kind) {
    const double param = kind == 5 ? 0.7 : 2.5;
    std::vector<double> out(in.size()), inplace(in);
    EvalConvertScores(kind, param, num_class, n, in.data(), out.data());
    EvalConvertScores(kind, param, num_class, n, inplace.data(), inplace.data());
    for (size_t j = 0; j < in.size(); ++j) {
      if (!SameBits(out[j], inplace[j])) {
        std::printf("kind %d K %d n %lld: in place differs at %zu\n", kind, num_class, static_cast<long long>(n), j);
        ++failures;
        break;
      }
      const double s = in[j];
      if (kind == 0 && !SameBits(out[j], s)) ++failures;
      if (kind == 2 && !SameBits(out[j], ((s > 0.0) - (s < 0.0)) * s * s)) ++failures;
      if ((kind == 1 || kind == 5) && !std::isnan(s) && !(out[j] >= 0.0 && out[j] <= 1.0)) ++failures;
    }
    if (kind == 4) {
      for (int64_t i = 0; i < n; ++i) {
        double sum = 0.0;
        for (int k = 0; k < num_class; ++k) sum += out[k * n + i];
        if (std::isfinite(sum) && std::fabs(sum - 1.0) > 1e-13) {
          std::printf("softmax K %d row %lld sums to %.17g\n", num_class, static_cast<long long>(i), sum);
          ++failures;
        }
      }
    }
  }
}

int main() {
  for (int num_class : {1, 2, 3, 17}) {
    for (int64_t n : {0, 1, 2, 63, 64, 65, 257}) Run(num_class, n);
  }
  if (failures != 0) {
    std::printf("score convert driver: %d failures\n", failures);
    return 1;
  }
  std::printf("score convert driver ok\n");
  return 0;
}
