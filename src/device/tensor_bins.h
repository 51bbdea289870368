// A strided matrix in device memory into group bins (src/device/tensor_bin_kernels.hip; host
// evaluator for tests without a GPU: LGBM_AMD_TensorGroupBinsOnHost).  The rule of one row, shared
// by the kernel and the evaluator, states what the column loop of LGBM_DatasetCreateFromMat
// (Dataset::PushColumnValue + FeatureGroup::Set) does to it in the groups the device takes:
//   - an element (float16, bfloat16, float32 or float64) is widened to double exactly;
//   - every group cell of the row starts at 0, and the group's members are taken in ascending
//     column order;
//   - a numerical member's value goes through ValueToBinNumerical (src/device/csr_bins.h), a
//     categorical member's through ValueToBinCategorical below;
//   - GroupCellOfBin: the most frequent bin writes nothing, any other bin writes
//     bin - (mfb == 0) + bin_offsets[sub], so a later non-default member of a bundle overwrites an
//     earlier one.
// A group is handed to the host when it is stored sparse (FeatureGroup::sparse: the host push
// builds its stored-row list), when a member's column is not in the matrix, or when a categorical
// member has more than kTensorMaxCategories categories.
#pragma once

#include <cstdint>

#include "csr_bins.h"

namespace lgbm_amd {
namespace dev {

// categories of one feature that the kernel's LDS table takes (8 bytes each)
constexpr int kTensorMaxCategories = 1024;

// the element types of a device matrix
struct Float16Bits {
  uint16_t bits;
};
struct Bfloat16Bits {
  uint16_t bits;
};

LGBM_AMD_HD double WidenElement(double v) { return v; }
LGBM_AMD_HD double WidenElement(float v) { return static_cast<double>(v); }
LGBM_AMD_HD double WidenElement(Bfloat16Bits v) {  // (the upper half of a float32)
  const uint32_t w = static_cast<uint32_t>(v.bits) << 16;
  float f;
  __builtin_memcpy(&f, &w, sizeof(f));
  return static_cast<double>(f);
}
LGBM_AMD_HD double WidenElement(Float16Bits v) {
  const uint64_t sign = static_cast<uint64_t>(v.bits >> 15) << 63;
  const uint32_t e = (v.bits >> 10) & 31u, m = v.bits & 1023u;
  uint64_t w;
  if (e == 0) {  // zero or subnormal: m * 2^-24
    const double s = static_cast<double>(m) * (1.0 / 16777216.0);
    __builtin_memcpy(&w, &s, sizeof(w));
  } else if (e == 31) {  // infinity / NaN
    w = 0x7ff0000000000000ull | (static_cast<uint64_t>(m) << 42);
  } else {
    w = (static_cast<uint64_t>(e + (1023 - 15)) << 52) | (static_cast<uint64_t>(m) << 42);
  }
  w |= sign;
  double d;
  __builtin_memcpy(&d, &w, sizeof(d));
  return d;
}

// BinMapper::ValueToBin of a categorical feature: NaN -> 0; the value truncated toward zero; a
// negative integer -> 0; an unknown category -> 0.  Values at or above 2^31 and infinities -> 0
// (the host's static_cast<int> is undefined there).  cats: the feature's n known categories in
// ascending order (all >= 0), bins: the bin of each.
LGBM_AMD_HD int ValueToBinCategorical(double value, int n, const int32_t* cats, const int32_t* bins) {
  if (!(value > -1.0 && value < 2147483648.0)) return 0;  // (NaN fails both comparisons)
  const int32_t iv = static_cast<int32_t>(value);
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (cats[mid] < iv) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && cats[lo] == iv ? bins[lo] : 0;
}

// a member feature of a group the device takes
struct TensorBinFeat {
  int32_t col;      // column of the matrix
  int32_t hi;       // numerical: search range [0, hi): num_bin - 1, minus the NaN bin
  int32_t nan_bin;  // numerical: NaN -> this bin (missing_type NaN), or -1: NaN -> 0.0
  int32_t mfb;      // most frequent bin (not stored)
  int32_t tab_off;  // numerical: upper bounds at ub[tab_off ...]; categorical: categories at
                    // cat[tab_off ... + ncat), their bins at cat[tab_off + ncat ... + 2 * ncat)
  uint32_t goff;    // group bin of the feature's bin 1 (its bin_offsets entry)
  int32_t ncat;     // known categories, or -1: numerical
  int32_t pad;
};

// what member F writes into its group's cell for `value` (table: F's own upper bounds, or its own
// categories followed by their bins)
LGBM_AMD_HD bool TensorFeatWrite(const TensorBinFeat& F, double value, const void* table, uint32_t* cell) {
  const int bin = F.ncat >= 0 ? ValueToBinCategorical(value, F.ncat, static_cast<const int32_t*>(table),
                                                      static_cast<const int32_t*>(table) + F.ncat)
                              : ValueToBinNumerical(value, F.hi, F.nan_bin, static_cast<const double*>(table));
  return GroupCellOfBin(bin, F.mfb, F.goff, cell);
}

}  // namespace dev
}  // namespace lgbm_amd
