// One definition of the pieces that every quantile selection of the library shares (mask_select.hip per segment,
// pooled_select.hip over the tiles of a picture, rank_order.hip for the order itself):
//   quantile_level   the host arithmetic of torch.quantile's rank and weight for one quality
//   quantile_lerp    ATen's lerp of the two order statistics
//   f2key / key2f    order-preserving uint32 keys of fp32 values, ascending
//   rank_sigma_bits  the canonical descending key of the rank order: -0.0 == +0.0, every NaN one key that sorts last
#pragma once
#include "common.h"
#include <cmath>

namespace vam {

// rank / weight of torch.quantile for one pr over n elements (the host arithmetic of channel_mask.py:138-139).
// mode: 0 = quantile, 1 = all zero (pr == 0), 2 = all one (pr >= 10)
static inline int quantile_level(double pr, long n, int* k_lo, int* k_hi, float* w, int* mode) {
  VAM_REQUIRE(pr >= 0.0 && pr == pr, "vam_variance_mask: pr must be >= 0");
  *k_lo = *k_hi = 0; *w = 0.f;
  if (pr >= 10.0) *mode = 2;                  // channel_mask.py:133-134
  else if (pr == 0.0) *mode = 1;              // :135-136
  else {
    *mode = 0;
    const double q_keep = pr * 0.1;            // python float arithmetic of :138-139
    // volatile: each step must round to fp32 exactly like ATen's tensor ops; a host-side
    // contraction of (qt*(n-1)) - lo into one fma changes w in the 5th digit and the
    // threshold by an ulp (caught by tests/golden thresholds).
    volatile float qt = (float)(1.0 - q_keep);       // scalar_tensor(q, float32)
    volatile float last = (float)(n - 1);
    volatile float rank = qt * last;                 // fp32 multiply (q * last_index)
    const float lo = floorf(rank);
    *k_lo = (int)lo;
    *k_hi = (int)ceilf(rank);
    *w = rank - lo;
    VAM_REQUIRE(*k_lo >= 0 && *k_hi < n, "vam_variance_mask: rank out of range");
  }
  return 0;
}

// thr = lerp(a, b, w) as ATen evaluates it (a fused fma on either side of w = 0.5); a = sorted[k_lo], b = sorted[k_hi]
__device__ __forceinline__ float quantile_lerp(float w, float lo_v, float hi_v) {
  const float d = hi_v - lo_v;
  return (w < 0.5f) ? __builtin_fmaf(w, d, lo_v) : __builtin_fmaf(w - 1.0f, d, hi_v);
}

__device__ __forceinline__ unsigned f2key(float f) {
  unsigned u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  unsigned u = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
  return __uint_as_float(u);
}

// Descending in sigma: +inf first, -0.0 == +0.0, every NaN behind -inf (whose key is 0xFF800000).
__device__ __forceinline__ unsigned rank_sigma_bits(float s) {
  unsigned u = __float_as_uint(s);
  unsigned d;
  if (s != s) {
    d = 0xFFFFFFFFu;                                      // every NaN: behind -inf (whose d is 0xFF800000)
  } else {
    if (u == 0x80000000u) u = 0u;                         // -0.0 == +0.0
    d = ~(u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u));   // descending in sigma
  }
  return d;
}
// The value of a non-NaN key of rank_sigma_bits (the all-ones key gives a NaN).
__device__ __forceinline__ float rank_bits_sigma(unsigned d) { return key2f(~d); }

}  // namespace vam
