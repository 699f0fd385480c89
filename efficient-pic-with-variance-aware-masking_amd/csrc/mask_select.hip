// Variance-aware mask: per (image, slice) segment, threshold = torch.quantile(sigma.ravel(),
// 1 - 0.1*pr) with linear interpolation, mask = sigma >= threshold
// (reference layers/channel_mask.py:132-151; ProgMask :18-49 is the same rule per block).
//
// Bit-exact restatement of ATen's quantile without a sort:
//   rank = float32(1 - 0.1*pr) * float32(n-1);  lo = floor(rank); hi = ceil(rank); w = rank - lo
//   a = sorted[lo], b = sorted[hi]            -> two order statistics by radix select on
//                                                 order-preserving uint32 keys (4 passes x 8 bit)
//   thr = w < 0.5 ? fma(w, b-a, a) : fma(w-1, b-a, b)    (ATen's lerp kernel is a fused fma)
//   any NaN in the segment -> thr = NaN -> mask all zero.
// One 1024-thread workgroup per segment; the segment's elements are loaded ONCE (16 B per
// lane, coalesced over the NHWC channel window) and stay in registers for every pass, so HBM
// traffic is the algorithmic 4 B read + 4 B written per element.  Histograms live in LDS.
#include "common.h"
#include "quantile.h"
#include <cmath>
#include <cstring>

namespace vam {

struct MaskArgs {
  const float* sigma;
  float* mask;
  float* thr;
  long batch_stride, slice_stride, mask_batch_stride, mask_slice_stride;
  int ld, ld_mask, n_slice, n_pix, C4;
  int k_lo, k_hi;
  float w;
  int mode;  // 0 = quantile, 1 = all zero (pr == 0), 2 = all one (pr >= 10)
};

// MAXV = float4 per thread kept in registers (0 = stream from memory every pass)
template <int MAXV>
__global__ __launch_bounds__(1024) void variance_mask_kernel(const MaskArgs a) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_k, sh_cnt, sh_min;
  __shared__ int sh_nan;

  const int seg = blockIdx.x;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  const float* src = a.sigma + b * a.batch_stride + j * a.slice_stride;
  float* dst = a.mask + b * a.mask_batch_stride + j * a.mask_slice_stride;
  const int nvec = a.n_pix * a.C4;
  const int tid = threadIdx.x;

  auto vec_ptr = [&](int i) -> const float* {
    int p = i / a.C4;
    return src + (long)p * a.ld + (i - p * a.C4) * 4;
  };
  auto out_ptr = [&](int i) -> float* {
    int p = i / a.C4;
    return dst + (long)p * a.ld_mask + (i - p * a.C4) * 4;
  };

  if (a.mode != 0) {
    const float v = a.mode == 2 ? 1.f : 0.f;
    for (int i = tid; i < nvec; i += 1024) *reinterpret_cast<float4*>(out_ptr(i)) = make_float4(v, v, v, v);
    if (tid == 0 && a.thr) a.thr[seg] = a.mode == 2 ? -INFINITY : INFINITY;
    return;
  }

  float4 reg[MAXV > 0 ? MAXV : 1];
  if (MAXV > 0) {
#pragma unroll
    for (int r = 0; r < MAXV; ++r) {
      int i = tid + r * 1024;
      reg[r] = (i < nvec) ? *reinterpret_cast<const float4*>(vec_ptr(i)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // visit every element of the segment: f(float)
  auto for_each = [&](auto&& f) {
    if (MAXV > 0) {
#pragma unroll
      for (int r = 0; r < MAXV; ++r) {
        if (tid + r * 1024 < nvec) { f(reg[r].x); f(reg[r].y); f(reg[r].z); f(reg[r].w); }
      }
    } else {
      for (int i = tid; i < nvec; i += 1024) {
        float4 v = *reinterpret_cast<const float4*>(vec_ptr(i));
        f(v.x); f(v.y); f(v.z); f(v.w);
      }
    }
  };

  if (tid == 0) sh_nan = 0;
  __syncthreads();
  {
    int nan = 0;
    for_each([&](float x) { nan |= (x != x) ? 1 : 0; });
    if (nan) atomicOr(&sh_nan, 1);
  }

  // ---- radix select of rank k_lo (ascending, 0-based)
  if (tid == 0) { sh_prefix = 0u; sh_k = (unsigned)a.k_lo; }
  for (int pass = 3; pass >= 0; --pass) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = sh_prefix;
    const int shift = pass * 8;
    const unsigned hi_mask = pass == 3 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for_each([&](float x) {
      unsigned k = f2key(x);
      if ((k & hi_mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    });
    __syncthreads();
    if (tid < 64) {
      unsigned h0 = hist[tid * 4], h1 = hist[tid * 4 + 1], h2 = hist[tid * 4 + 2], h3 = hist[tid * 4 + 3];
      unsigned c = h0 + h1 + h2 + h3;
      unsigned incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        unsigned t = __shfl_up(incl, o, 64);
        if (tid >= o) incl += t;
      }
      unsigned excl = incl - c;
      const unsigned k = sh_k;
      if (k >= excl && k < incl) {
        unsigned kk = k - excl;
        unsigned bin;
        if (kk < h0) bin = 0;
        else if ((kk -= h0) < h1) bin = 1;
        else if ((kk -= h1) < h2) bin = 2;
        else { kk -= h2; bin = 3; }
        sh_prefix = prefix | ((unsigned)(tid * 4 + bin) << shift);
        sh_k = kk;
      }
    }
    __syncthreads();
  }
  const unsigned key_lo = sh_prefix;
  unsigned key_hi = key_lo;
  if (a.k_hi != a.k_lo) {
    // sorted[k_lo+1]: equals key_lo when more than k_lo+1 elements are <= key_lo, else the
    // smallest key above it.
    if (tid == 0) { sh_cnt = 0u; sh_min = 0xFFFFFFFFu; }
    __syncthreads();
    unsigned cnt = 0u, mn = 0xFFFFFFFFu;
    for_each([&](float x) {
      unsigned k = f2key(x);
      if (k <= key_lo) ++cnt;
      else mn = mn < k ? mn : k;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_down(cnt, o, 64);
      unsigned t = __shfl_down(mn, o, 64);
      mn = mn < t ? mn : t;
    }
    if ((tid & 63) == 0) { atomicAdd(&sh_cnt, cnt); atomicMin(&sh_min, mn); }
    __syncthreads();
    key_hi = (sh_cnt > (unsigned)a.k_lo + 1u) ? key_lo : sh_min;
  }
  const float lo_v = key2f(key_lo), hi_v = key2f(key_hi);
  float thr = quantile_lerp(a.w, lo_v, hi_v);
  if (sh_nan) thr = __uint_as_float(0x7FC00000u);
  if (tid == 0 && a.thr) a.thr[seg] = thr;

  if (MAXV > 0) {
#pragma unroll
    for (int r = 0; r < MAXV; ++r) {
      int i = tid + r * 1024;
      if (i < nvec) {
        float4 v = reg[r];
        *reinterpret_cast<float4*>(out_ptr(i)) = make_float4(v.x >= thr ? 1.f : 0.f, v.y >= thr ? 1.f : 0.f,
                                                              v.z >= thr ? 1.f : 0.f, v.w >= thr ? 1.f : 0.f);
      }
    }
  } else {
    for (int i = tid; i < nvec; i += 1024) {
      float4 v = *reinterpret_cast<const float4*>(vec_ptr(i));
      *reinterpret_cast<float4*>(out_ptr(i)) = make_float4(v.x >= thr ? 1.f : 0.f, v.y >= thr ? 1.f : 0.f,
                                                            v.z >= thr ? 1.f : 0.f, v.w >= thr ? 1.f : 0.f);
    }
  }
}

// vam_variance_mask_levels: the same selection for several qualities over one load of the segment;
// vam_variance_layers: the same selections, then one pass that assigns each element its container layer
struct MaskLevelsArgs {
  const float* sigma;
  float* mask;
  float* thr;
  uint8_t* layer;                    // LAYERS: layer ids instead of masks
  long batch_stride, slice_stride, mask_batch_stride, mask_slice_stride, mask_level_stride;
  int ld, ld_mask, n_slice, n_pix, C4;
  int n_levels, any_select;          // any_select: some level needs the order statistics
  // per level (vam_variance_mask: one level)
  int k_lo[VAM_MAX_LAYER_LEVELS], k_hi[VAM_MAX_LAYER_LEVELS];
  float w[VAM_MAX_LAYER_LEVELS];
  int mode[VAM_MAX_LAYER_LEVELS];    // 0 = quantile, 1 = all zero (pr == 0), 2 = all one (pr >= 10)
};

// vam_variance_layers_per_image: the strides of MaskLevelsArgs, and the per-level fields from a device table with one
// record per image (a list of 32 qualities per image does not fit the kernel arguments of a batch)
struct MaskImageArgs {
  const float* sigma;
  float* thr;
  uint8_t* layer;
  const vam_layer_params* table;
  long batch_stride, slice_stride, mask_batch_stride, mask_slice_stride;
  int ld, ld_mask, n_slice, n_pix, C4;
};

// vam_variance_masks_per_image: MaskImageArgs' table, and the float masks of MaskLevelsArgs in place of layer ids (layer
// stays NULL: the kernel's LAYERS = false instantiations never read it).  max_levels = the levels `mask` and `thr` hold.
struct MaskImageMaskArgs : MaskImageArgs {
  float* mask;
  long mask_level_stride;
  int max_levels;
};

// vam_variance_mask_map: MaskImageArgs' table and thresholds (LAYERS = true: they stay in LDS), and in place of the layer
// ids ONE float mask in which pixel p of image b takes level level_map[b * map_batch_stride + p] of that image's list
// (mask_* then describe the float mask, as in MaskArgs; layer stays NULL)
struct MaskMapArgs : MaskImageArgs {
  float* mask;
  const uint8_t* level_map;
  long map_batch_stride;
};
template <class Args> struct lv_is_map { static constexpr bool value = false; };
template <> struct lv_is_map<MaskMapArgs> { static constexpr bool value = true; };

// the per-level fields of the argument kinds of variance_mask_levels_kernel
__device__ __forceinline__ int lv_count(const MaskLevelsArgs& a, int) { return a.n_levels; }
__device__ __forceinline__ int lv_any_select(const MaskLevelsArgs& a, int) { return a.any_select; }
__device__ __forceinline__ int lv_mode(const MaskLevelsArgs& a, int, int lv) { return a.mode[lv]; }
__device__ __forceinline__ int lv_k_lo(const MaskLevelsArgs& a, int, int lv) { return a.k_lo[lv]; }
__device__ __forceinline__ int lv_k_hi(const MaskLevelsArgs& a, int, int lv) { return a.k_hi[lv]; }
__device__ __forceinline__ float lv_w(const MaskLevelsArgs& a, int, int lv) { return a.w[lv]; }
__device__ __forceinline__ float* lv_mask(const MaskLevelsArgs& a) { return a.mask; }
__device__ __forceinline__ long lv_stride(const MaskLevelsArgs& a) { return a.mask_level_stride; }
__device__ __forceinline__ int lv_count(const MaskImageArgs& a, int b) {
  const int n = a.table[b].n_levels;                      // the host validates the table; a bad record selects nothing
  return n < 0 || n > VAM_MAX_LAYER_LEVELS ? 0 : n;
}
__device__ __forceinline__ int lv_any_select(const MaskImageArgs& a, int b) { return a.table[b].any_select; }
__device__ __forceinline__ int lv_mode(const MaskImageArgs& a, int b, int lv) { return a.table[b].mode[lv]; }
__device__ __forceinline__ int lv_k_lo(const MaskImageArgs& a, int b, int lv) { return a.table[b].k_lo[lv]; }
__device__ __forceinline__ int lv_k_hi(const MaskImageArgs& a, int b, int lv) { return a.table[b].k_hi[lv]; }
__device__ __forceinline__ float lv_w(const MaskImageArgs& a, int b, int lv) { return a.table[b].w[lv]; }
__device__ __forceinline__ float* lv_mask(const MaskImageArgs&) { return nullptr; }
__device__ __forceinline__ long lv_stride(const MaskImageArgs&) { return 0L; }
// the other fields of a MaskImageMaskArgs are its base's: image b's record
__device__ __forceinline__ int lv_count(const MaskImageMaskArgs& a, int b) {
  const int n = a.table[b].n_levels;                      // a record beyond what the buffers hold writes nothing
  return n < 0 || n > a.max_levels ? 0 : n;
}
__device__ __forceinline__ float* lv_mask(const MaskImageMaskArgs& a) { return a.mask; }
__device__ __forceinline__ long lv_stride(const MaskImageMaskArgs& a) { return a.mask_level_stride; }

// MAXV = float4 per thread kept in registers (0 = stream from memory every pass).  The segment is loaded once; each level
// then runs its own selection on the same registers and writes its own mask.  LAYERS: the levels' thresholds stay in
// LDS, and one last pass writes layer = the first level whose mask holds the element (mask_* name the layer array).
// Args: MaskLevelsArgs (one quality list in the kernel arguments) or MaskImageArgs (vam_variance_layers_per_image: image
// b's record of a device table) or MaskImageMaskArgs (vam_variance_masks_per_image: that record, float masks per level);
// the per-level fields are read through the lv_* accessors above, so the first kind compiles to the accesses it always made.
// MaskMapArgs (vam_variance_mask_map, LAYERS = true) replaces the last pass: one float mask, each pixel at its own level.
template <int MAXV, bool LAYERS, class Args = MaskLevelsArgs>
__global__ __launch_bounds__(1024) void variance_mask_levels_kernel(const Args a) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_k, sh_cnt, sh_min;
  __shared__ int sh_nan;
  __shared__ float sh_thr[LAYERS ? VAM_MAX_LAYER_LEVELS : 1];

  const int seg = blockIdx.x;
  const int segs = gridDim.x;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  const float* src = a.sigma + b * a.batch_stride + j * a.slice_stride;
  float* const dst0 = lv_mask(a) + b * a.mask_batch_stride + j * a.mask_slice_stride;
  const int nvec = a.n_pix * a.C4;
  const int tid = threadIdx.x;

  auto vec_ptr = [&](int i) -> const float* {
    int p = i / a.C4;
    return src + (long)p * a.ld + (i - p * a.C4) * 4;
  };
  auto out_ptr = [&](float* dst, int i) -> float* {
    int p = i / a.C4;
    return dst + (long)p * a.ld_mask + (i - p * a.C4) * 4;
  };

  float4 reg[MAXV > 0 ? MAXV : 1];
  if (MAXV > 0) {
#pragma unroll
    for (int r = 0; r < MAXV; ++r) {
      int i = tid + r * 1024;
      reg[r] = (i < nvec) ? *reinterpret_cast<const float4*>(vec_ptr(i)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // visit every element of the segment: f(float)
  auto for_each = [&](auto&& f) {
    if (MAXV > 0) {
#pragma unroll
      for (int r = 0; r < MAXV; ++r) {
        if (tid + r * 1024 < nvec) { f(reg[r].x); f(reg[r].y); f(reg[r].z); f(reg[r].w); }
      }
    } else {
      for (int i = tid; i < nvec; i += 1024) {
        float4 v = *reinterpret_cast<const float4*>(vec_ptr(i));
        f(v.x); f(v.y); f(v.z); f(v.w);
      }
    }
  };

  if (lv_any_select(a, b)) {
    if (tid == 0) sh_nan = 0;
    __syncthreads();
    int nan = 0;
    for_each([&](float x) { nan |= (x != x) ? 1 : 0; });
    if (nan) atomicOr(&sh_nan, 1);
  }

  for (int lv = 0; lv < lv_count(a, b); ++lv) {
    float* dst = dst0 + lv * lv_stride(a);
    float* thr_out = a.thr ? a.thr + (long)lv * segs : nullptr;
    if (lv_mode(a, b, lv) != 0) {
      const float v = lv_mode(a, b, lv) == 2 ? 1.f : 0.f;
      if (!LAYERS)
        for (int i = tid; i < nvec; i += 1024) *reinterpret_cast<float4*>(out_ptr(dst, i)) = make_float4(v, v, v, v);
      if (tid == 0 && thr_out) thr_out[seg] = lv_mode(a, b, lv) == 2 ? -INFINITY : INFINITY;
      continue;
    }
    const int k_lo = lv_k_lo(a, b, lv), k_hi = lv_k_hi(a, b, lv);
    const float w = lv_w(a, b, lv);
    __syncthreads();              // the previous level's readers of sh_prefix / sh_cnt / sh_min are done

    // ---- radix select of rank k_lo (ascending, 0-based)
    if (tid == 0) { sh_prefix = 0u; sh_k = (unsigned)k_lo; }
    for (int pass = 3; pass >= 0; --pass) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      const unsigned prefix = sh_prefix;
      const int shift = pass * 8;
      const unsigned hi_mask = pass == 3 ? 0u : (0xFFFFFFFFu << (shift + 8));
      for_each([&](float x) {
        unsigned k = f2key(x);
        if ((k & hi_mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      });
      __syncthreads();
      if (tid < 64) {
        unsigned h0 = hist[tid * 4], h1 = hist[tid * 4 + 1], h2 = hist[tid * 4 + 2], h3 = hist[tid * 4 + 3];
        unsigned c = h0 + h1 + h2 + h3;
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          unsigned t = __shfl_up(incl, o, 64);
          if (tid >= o) incl += t;
        }
        unsigned excl = incl - c;
        const unsigned k = sh_k;
        if (k >= excl && k < incl) {
          unsigned kk = k - excl;
          unsigned bin;
          if (kk < h0) bin = 0;
          else if ((kk -= h0) < h1) bin = 1;
          else if ((kk -= h1) < h2) bin = 2;
          else { kk -= h2; bin = 3; }
          sh_prefix = prefix | ((unsigned)(tid * 4 + bin) << shift);
          sh_k = kk;
        }
      }
      __syncthreads();
    }
    const unsigned key_lo = sh_prefix;
    unsigned key_hi = key_lo;
    if (k_hi != k_lo) {
      // sorted[k_lo+1]: equals key_lo when more than k_lo+1 elements are <= key_lo, else the
      // smallest key above it.
      if (tid == 0) { sh_cnt = 0u; sh_min = 0xFFFFFFFFu; }
      __syncthreads();
      unsigned cnt = 0u, mn = 0xFFFFFFFFu;
      for_each([&](float x) {
        unsigned k = f2key(x);
        if (k <= key_lo) ++cnt;
        else mn = mn < k ? mn : k;
      });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_down(cnt, o, 64);
        unsigned t = __shfl_down(mn, o, 64);
        mn = mn < t ? mn : t;
      }
      if ((tid & 63) == 0) { atomicAdd(&sh_cnt, cnt); atomicMin(&sh_min, mn); }
      __syncthreads();
      key_hi = (sh_cnt > (unsigned)k_lo + 1u) ? key_lo : sh_min;
    }
    const float lo_v = key2f(key_lo), hi_v = key2f(key_hi);
    float thr = quantile_lerp(w, lo_v, hi_v);
    if (sh_nan) thr = __uint_as_float(0x7FC00000u);
    if (tid == 0 && thr_out) thr_out[seg] = thr;
    if (LAYERS) {
      if (tid == 0) sh_thr[lv] = thr;
      continue;
    }

    if (MAXV > 0) {
#pragma unroll
      for (int r = 0; r < MAXV; ++r) {
        int i = tid + r * 1024;
        if (i < nvec) {
          float4 v = reg[r];
          *reinterpret_cast<float4*>(out_ptr(dst, i)) = make_float4(v.x >= thr ? 1.f : 0.f, v.y >= thr ? 1.f : 0.f,
                                                                     v.z >= thr ? 1.f : 0.f, v.w >= thr ? 1.f : 0.f);
        }
      }
    } else {
      for (int i = tid; i < nvec; i += 1024) {
        float4 v = *reinterpret_cast<const float4*>(vec_ptr(i));
        *reinterpret_cast<float4*>(out_ptr(dst, i)) = make_float4(v.x >= thr ? 1.f : 0.f, v.y >= thr ? 1.f : 0.f,
                                                                   v.z >= thr ? 1.f : 0.f, v.w >= thr ? 1.f : 0.f);
      }
    }
  }
  if (!LAYERS) return;

  __syncthreads();
  if constexpr (lv_is_map<Args>::value) {
    // ---- quality map: pixel p keeps x >= the threshold of ITS level (all one / all zero for the levels without one;
    // zero for a map entry beyond the image's list)
    __shared__ int sh_md[VAM_MAX_LAYER_LEVELS];
    const int n_lv = lv_count(a, b);
    if (tid < VAM_MAX_LAYER_LEVELS) sh_md[tid] = tid < n_lv ? lv_mode(a, b, tid) : 1;
    __syncthreads();
    float* const mdst = a.mask + b * a.mask_batch_stride + j * a.mask_slice_stride;
    const uint8_t* const lmap = a.level_map + b * a.map_batch_stride;
    auto put = [&](int i, float4 v) {
      const int p = i / a.C4;
      const int lv = (int)lmap[p];
      const int md = lv < VAM_MAX_LAYER_LEVELS ? sh_md[lv] : 1;
      float4 o;
      if (md != 0) {
        const float c = md == 2 ? 1.f : 0.f;
        o = make_float4(c, c, c, c);
      } else {
        const float thr = sh_thr[lv];
        o = make_float4(v.x >= thr ? 1.f : 0.f, v.y >= thr ? 1.f : 0.f, v.z >= thr ? 1.f : 0.f, v.w >= thr ? 1.f : 0.f);
      }
      *reinterpret_cast<float4*>(mdst + (long)p * a.ld_mask + (i - p * a.C4) * 4) = o;
    };
    if (MAXV > 0) {
#pragma unroll
      for (int r = 0; r < MAXV; ++r) {
        int i = tid + r * 1024;
        if (i < nvec) put(i, reg[r]);
      }
    } else {
      for (int i = tid; i < nvec; i += 1024) put(i, *reinterpret_cast<const float4*>(vec_ptr(i)));
    }
    return;
  }

  // ---- layer assignment: layer <= k  <=>  mask_k == 1 (the masks of a non-decreasing quality list are nested)
  uint8_t* const ldst = a.layer + b * a.mask_batch_stride + j * a.mask_slice_stride;
  auto layer_of = [&](float x) -> unsigned {
    for (int lv = 0; lv < lv_count(a, b); ++lv) {
      const int md = lv_mode(a, b, lv);
      if (md == 2 || (md == 0 && x >= sh_thr[lv])) return (unsigned)lv;
    }
    return 0xFFu;
  };
  auto put = [&](int i, float4 v) {
    int p = i / a.C4;
    const unsigned word = layer_of(v.x) | (layer_of(v.y) << 8) | (layer_of(v.z) << 16) | (layer_of(v.w) << 24);
    *reinterpret_cast<unsigned*>(ldst + (long)p * a.ld_mask + (i - p * a.C4) * 4) = word;
  };
  if (MAXV > 0) {
#pragma unroll
    for (int r = 0; r < MAXV; ++r) {
      int i = tid + r * 1024;
      if (i < nvec) put(i, reg[r]);
    }
  } else {
    for (int i = tid; i < nvec; i += 1024) put(i, *reinterpret_cast<const float4*>(vec_ptr(i)));
  }
}

}  // namespace vam

using namespace vam;

extern "C" int vam_variance_mask(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                 int n_slice, int n_pix, int C, double pr, float* mask_out, int ld_mask,
                                 long mask_batch_stride, long mask_slice_stride, float* thr_out, void* stream) {
  VAM_REQUIRE(sigma && mask_out && n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "vam_variance_mask: bad arguments");
  VAM_REQUIRE(C % 4 == 0 && ld % 4 == 0 && ld_mask % 4 == 0 && batch_stride % 4 == 0 && slice_stride % 4 == 0 && mask_batch_stride % 4 == 0 && mask_slice_stride % 4 == 0, "vam_variance_mask: C and strides must be multiples of 4");
  VAM_REQUIRE((((uintptr_t)sigma) & 15) == 0 && (((uintptr_t)mask_out) & 15) == 0, "vam_variance_mask: 16-byte alignment");
  VAM_REQUIRE(ld >= C && ld_mask >= C, "vam_variance_mask: pixel stride < C");
  const long n = (long)n_pix * C;
  // torch.quantile rejects inputs above 16M elements (ATen Sorting.cpp); so do we
  VAM_REQUIRE(n <= 16000000L, "vam_variance_mask: segment of %ld elements exceeds torch.quantile's 16M limit", n);
  VAM_REQUIRE(pr >= 0.0 && pr == pr, "vam_variance_mask: pr must be >= 0");
  MaskArgs a;
  a.sigma = sigma; a.mask = mask_out; a.thr = thr_out;
  a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.mask_batch_stride = mask_batch_stride; a.mask_slice_stride = mask_slice_stride;
  a.ld = ld; a.ld_mask = ld_mask; a.n_slice = n_slice; a.n_pix = n_pix; a.C4 = C / 4;
  a.k_lo = a.k_hi = 0; a.w = 0.f;
  if (pr >= 10.0) a.mode = 2;                 // channel_mask.py:133-134
  else if (pr == 0.0) a.mode = 1;             // :135-136
  else {
    a.mode = 0;
    const double q_keep = pr * 0.1;            // python float arithmetic of :138-139
    // volatile: each step must round to fp32 exactly like ATen's tensor ops; a host-side
    // contraction of (qt*(n-1)) - lo into one fma changes w in the 5th digit and the
    // threshold by an ulp (caught by tests/golden thresholds).
    volatile float qt = (float)(1.0 - q_keep);       // scalar_tensor(q, float32)
    volatile float last = (float)(n - 1);
    volatile float rank = qt * last;                 // fp32 multiply (q * last_index)
    const float lo = floorf(rank);
    a.k_lo = (int)lo;
    a.k_hi = (int)ceilf(rank);
    a.w = rank - lo;
    VAM_REQUIRE(a.k_lo >= 0 && a.k_hi < n, "vam_variance_mask: rank out of range");
  }
  const int segs = n_batch * n_slice;
  const int nvec = n_pix * (C / 4);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, 8.0 * (double)n * segs);
  if (nvec <= 4 * 1024)
    hipLaunchKernelGGL((variance_mask_kernel<4>), dim3(segs), dim3(1024), 0, s, a);
  else if (nvec <= 16 * 1024)
    hipLaunchKernelGGL((variance_mask_kernel<16>), dim3(segs), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL((variance_mask_kernel<0>), dim3(segs), dim3(1024), 0, s, a);
  return check_launch("variance_mask_kernel");
}

// rank / weight of torch.quantile for one pr (the host arithmetic of channel_mask.py:138-139)
static int mask_level_params(MaskLevelsArgs& a, int lv, double pr, long n) {
  return quantile_level(pr, n, &a.k_lo[lv], &a.k_hi[lv], &a.w[lv], &a.mode[lv]);
}

// layer_out != NULL: vam_variance_layers (mask_* then describe the uint8 layer array)
static int mask_launch(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice, int n_pix,
                       int C, const double* prs, int n_levels, float* mask_out, uint8_t* layer_out, int ld_mask,
                       long mask_batch_stride, long mask_slice_stride, long mask_level_stride, float* thr_out, void* stream) {
  const bool layers = layer_out != nullptr;
  VAM_REQUIRE(sigma && (mask_out || layers) && n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "vam_variance_mask: bad arguments");
  VAM_REQUIRE(C % 4 == 0 && ld % 4 == 0 && ld_mask % 4 == 0 && batch_stride % 4 == 0 && slice_stride % 4 == 0 && mask_batch_stride % 4 == 0 && mask_slice_stride % 4 == 0 && mask_level_stride % 4 == 0, "vam_variance_mask: C and strides must be multiples of 4");
  VAM_REQUIRE((((uintptr_t)sigma) & 15) == 0 && (((uintptr_t)mask_out) & 15) == 0 && (((uintptr_t)layer_out) & 3) == 0,
              "vam_variance_mask: 16-byte alignment (layers: 4-byte)");
  VAM_REQUIRE(ld >= C && ld_mask >= C, "vam_variance_mask: pixel stride < C");
  const int max_levels = layers ? VAM_MAX_LAYER_LEVELS : VAM_MAX_MASK_LEVELS;
  VAM_REQUIRE(prs && n_levels >= 1 && n_levels <= max_levels, "%s: 1..%d levels, got %d",
              layers ? "vam_variance_layers" : "vam_variance_mask_levels", max_levels, n_levels);
  for (int lv = 1; layers && lv < n_levels; ++lv)
    VAM_REQUIRE(prs[lv] >= prs[lv - 1], "vam_variance_layers: qualities must be non-decreasing (prs[%d] < prs[%d])", lv, lv - 1);
  const long n = (long)n_pix * C;
  // torch.quantile rejects inputs above 16M elements (ATen Sorting.cpp); so do we
  VAM_REQUIRE(n <= 16000000L, "vam_variance_mask: segment of %ld elements exceeds torch.quantile's 16M limit", n);
  MaskLevelsArgs a;
  a.sigma = sigma; a.mask = mask_out; a.thr = thr_out; a.layer = layer_out;
  a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.mask_batch_stride = mask_batch_stride; a.mask_slice_stride = mask_slice_stride; a.mask_level_stride = mask_level_stride;
  a.ld = ld; a.ld_mask = ld_mask; a.n_slice = n_slice; a.n_pix = n_pix; a.C4 = C / 4;
  a.n_levels = n_levels;
  a.any_select = 0;
  for (int lv = 0; lv < n_levels; ++lv) {
    const int rc = mask_level_params(a, lv, prs[lv], n);
    if (rc) return rc;
    a.any_select |= a.mode[lv] == 0;
  }
  const int segs = n_batch * n_slice;
  const int nvec = n_pix * (C / 4);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, (layers ? 5.0 : 4.0 + 4.0 * n_levels) * (double)n * segs);
  if (layers) {
    if (nvec <= 4 * 1024)
      hipLaunchKernelGGL((variance_mask_levels_kernel<4, true>), dim3(segs), dim3(1024), 0, s, a);
    else if (nvec <= 16 * 1024)
      hipLaunchKernelGGL((variance_mask_levels_kernel<16, true>), dim3(segs), dim3(1024), 0, s, a);
    else
      hipLaunchKernelGGL((variance_mask_levels_kernel<0, true>), dim3(segs), dim3(1024), 0, s, a);
    return check_launch("variance_layers_kernel");
  }
  if (nvec <= 4 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<4, false>), dim3(segs), dim3(1024), 0, s, a);
  else if (nvec <= 16 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<16, false>), dim3(segs), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL((variance_mask_levels_kernel<0, false>), dim3(segs), dim3(1024), 0, s, a);
  return check_launch("variance_mask_levels_kernel");
}

extern "C" int vam_variance_mask_levels(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                        int n_slice, int n_pix, int C, const double* prs, int n_levels, float* mask_out,
                                        int ld_mask, long mask_batch_stride, long mask_slice_stride, long mask_level_stride,
                                        float* thr_out, void* stream) {
  return mask_launch(sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, prs, n_levels, mask_out, nullptr,
                     ld_mask, mask_batch_stride, mask_slice_stride, mask_level_stride, thr_out, stream);
}

extern "C" int vam_variance_layers(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                                   int n_pix, int C, const double* prs, int n_levels, uint8_t* layer_out, int ld_layer,
                                   long layer_batch_stride, long layer_slice_stride, float* thr_out, void* stream) {
  VAM_REQUIRE(layer_out, "vam_variance_layers: layer_out is NULL");
  return mask_launch(sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, prs, n_levels, nullptr, layer_out,
                     ld_layer, layer_batch_stride, layer_slice_stride, 0, thr_out, stream);
}

extern "C" size_t vam_layer_params_size(void) { return sizeof(vam_layer_params); }

// the records of vam_variance_layers_per_image (sorted: non-decreasing lists of up to VAM_MAX_LAYER_LEVELS) and of
// vam_variance_masks_per_image (any order, up to VAM_MAX_MASK_LEVELS): mask_level_params' own arithmetic, one image at a time
static int image_params(const char* what, const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix, int C,
                        vam_layer_params* table_host, int max_levels, bool sorted) {
  const long n = (long)n_pix * C;
  VAM_REQUIRE(n <= 16000000L, "vam_variance_mask: segment of %ld elements exceeds torch.quantile's 16M limit", n);
  MaskLevelsArgs a;
  for (int b = 0; b < n_batch; ++b) {
    const int nl = n_levels[b];
    const double* p = prs + (long)b * levels_stride;
    VAM_REQUIRE(nl >= 1 && nl <= max_levels && nl <= levels_stride, "%s: image %d: 1..%d levels, got %d", what, b, max_levels, nl);
    vam_layer_params& t = table_host[b];
    std::memset(&t, 0, sizeof(t));
    t.n_levels = nl;
    for (int lv = 0; lv < nl; ++lv) {
      VAM_REQUIRE(!sorted || lv == 0 || p[lv] >= p[lv - 1], "%s: image %d: qualities must be non-decreasing (prs[%d] < prs[%d])",
                  what, b, lv, lv - 1);
      const int rc = mask_level_params(a, lv, p[lv], n);
      if (rc) return rc;
      t.k_lo[lv] = a.k_lo[lv]; t.k_hi[lv] = a.k_hi[lv]; t.w[lv] = a.w[lv]; t.mode[lv] = a.mode[lv];
      t.any_select |= a.mode[lv] == 0;
    }
  }
  return VAM_OK;
}

extern "C" int vam_variance_layer_params(const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix,
                                         int C, vam_layer_params* table_host) {
  VAM_REQUIRE(prs && n_levels && table_host && n_batch > 0 && levels_stride >= 1 && n_pix > 0 && C > 0,
              "vam_variance_layer_params: bad arguments");
  return image_params("vam_variance_layers_per_image", prs, n_levels, n_batch, levels_stride, n_pix, C, table_host,
                      VAM_MAX_LAYER_LEVELS, true);
}

extern "C" int vam_variance_mask_params(const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix,
                                        int C, vam_layer_params* table_host) {
  VAM_REQUIRE(prs && n_levels && table_host && n_batch > 0 && levels_stride >= 1 && n_pix > 0 && C > 0,
              "vam_variance_mask_params: bad arguments");
  return image_params("vam_variance_masks_per_image", prs, n_levels, n_batch, levels_stride, n_pix, C, table_host,
                      VAM_MAX_MASK_LEVELS, false);
}

extern "C" int vam_variance_layers_per_image(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                             int n_slice, int n_pix, int C, const vam_layer_params* table_dev,
                                             uint8_t* layer_out, int ld_layer, long layer_batch_stride,
                                             long layer_slice_stride, float* thr_out, void* stream) {
  VAM_REQUIRE(sigma && table_dev && layer_out && n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "vam_variance_layers_per_image: bad arguments");
  VAM_REQUIRE(C % 4 == 0 && ld % 4 == 0 && ld_layer % 4 == 0 && batch_stride % 4 == 0 && slice_stride % 4 == 0 && layer_batch_stride % 4 == 0 && layer_slice_stride % 4 == 0, "vam_variance_layers_per_image: C and strides must be multiples of 4");
  VAM_REQUIRE((((uintptr_t)sigma) & 15) == 0 && (((uintptr_t)layer_out) & 3) == 0 && (((uintptr_t)table_dev) & 3) == 0,
              "vam_variance_layers_per_image: 16-byte alignment (layers, table: 4-byte)");
  VAM_REQUIRE(ld >= C && ld_layer >= C, "vam_variance_layers_per_image: pixel stride < C");
  const long n = (long)n_pix * C;
  VAM_REQUIRE(n <= 16000000L, "vam_variance_mask: segment of %ld elements exceeds torch.quantile's 16M limit", n);
  MaskImageArgs a;
  a.sigma = sigma; a.thr = thr_out; a.layer = layer_out; a.table = table_dev;
  a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.mask_batch_stride = layer_batch_stride; a.mask_slice_stride = layer_slice_stride;
  a.ld = ld; a.ld_mask = ld_layer; a.n_slice = n_slice; a.n_pix = n_pix; a.C4 = C / 4;
  const int segs = n_batch * n_slice;
  const int nvec = n_pix * (C / 4);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, 5.0 * (double)n * segs);
  if (nvec <= 4 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<4, true, MaskImageArgs>), dim3(segs), dim3(1024), 0, s, a);
  else if (nvec <= 16 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<16, true, MaskImageArgs>), dim3(segs), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL((variance_mask_levels_kernel<0, true, MaskImageArgs>), dim3(segs), dim3(1024), 0, s, a);
  return check_launch("variance_layers_per_image_kernel");
}

extern "C" int vam_variance_masks_per_image(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                            int n_slice, int n_pix, int C, const vam_layer_params* table_dev, int max_levels,
                                            float* mask_out, int ld_mask, long mask_batch_stride, long mask_slice_stride,
                                            long mask_level_stride, float* thr_out, void* stream) {
  VAM_REQUIRE(sigma && table_dev && mask_out && n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "vam_variance_masks_per_image: bad arguments");
  VAM_REQUIRE(max_levels >= 1 && max_levels <= VAM_MAX_MASK_LEVELS, "vam_variance_masks_per_image: 1..%d levels, got %d",
              VAM_MAX_MASK_LEVELS, max_levels);
  VAM_REQUIRE(C % 4 == 0 && ld % 4 == 0 && ld_mask % 4 == 0 && batch_stride % 4 == 0 && slice_stride % 4 == 0 && mask_batch_stride % 4 == 0 && mask_slice_stride % 4 == 0 && mask_level_stride % 4 == 0, "vam_variance_masks_per_image: C and strides must be multiples of 4");
  VAM_REQUIRE((((uintptr_t)sigma) & 15) == 0 && (((uintptr_t)mask_out) & 15) == 0 && (((uintptr_t)table_dev) & 3) == 0,
              "vam_variance_masks_per_image: 16-byte alignment (table: 4-byte)");
  VAM_REQUIRE(ld >= C && ld_mask >= C, "vam_variance_masks_per_image: pixel stride < C");
  const long n = (long)n_pix * C;
  VAM_REQUIRE(n <= 16000000L, "vam_variance_mask: segment of %ld elements exceeds torch.quantile's 16M limit", n);
  MaskImageMaskArgs a;
  a.sigma = sigma; a.thr = thr_out; a.layer = nullptr; a.table = table_dev;
  a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.mask_batch_stride = mask_batch_stride; a.mask_slice_stride = mask_slice_stride;
  a.ld = ld; a.ld_mask = ld_mask; a.n_slice = n_slice; a.n_pix = n_pix; a.C4 = C / 4;
  a.mask = mask_out; a.mask_level_stride = mask_level_stride; a.max_levels = max_levels;
  const int segs = n_batch * n_slice;
  const int nvec = n_pix * (C / 4);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, (4.0 + 4.0 * max_levels) * (double)n * segs);
  if (nvec <= 4 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<4, false, MaskImageMaskArgs>), dim3(segs), dim3(1024), 0, s, a);
  else if (nvec <= 16 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<16, false, MaskImageMaskArgs>), dim3(segs), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL((variance_mask_levels_kernel<0, false, MaskImageMaskArgs>), dim3(segs), dim3(1024), 0, s, a);
  return check_launch("variance_masks_per_image_kernel");
}

extern "C" int vam_variance_mask_map(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                                     int n_pix, int C, const vam_layer_params* table_dev, const uint8_t* level_map,
                                     long map_batch_stride, float* mask_out, int ld_mask, long mask_batch_stride,
                                     long mask_slice_stride, float* thr_out, void* stream) {
  VAM_REQUIRE(sigma && table_dev && level_map && mask_out && n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "vam_variance_mask_map: bad arguments");
  VAM_REQUIRE(C % 4 == 0 && ld % 4 == 0 && ld_mask % 4 == 0 && batch_stride % 4 == 0 && slice_stride % 4 == 0 && mask_batch_stride % 4 == 0 && mask_slice_stride % 4 == 0, "vam_variance_mask_map: C and strides must be multiples of 4");
  VAM_REQUIRE((((uintptr_t)sigma) & 15) == 0 && (((uintptr_t)mask_out) & 15) == 0 && (((uintptr_t)table_dev) & 3) == 0,
              "vam_variance_mask_map: 16-byte alignment (table: 4-byte)");
  VAM_REQUIRE(ld >= C && ld_mask >= C, "vam_variance_mask_map: pixel stride < C");
  VAM_REQUIRE(map_batch_stride >= n_pix, "vam_variance_mask_map: map_batch_stride %ld < n_pix %d", map_batch_stride, n_pix);
  const long n = (long)n_pix * C;
  VAM_REQUIRE(n <= 16000000L, "vam_variance_mask: segment of %ld elements exceeds torch.quantile's 16M limit", n);
  MaskMapArgs a;
  a.sigma = sigma; a.thr = thr_out; a.layer = nullptr; a.table = table_dev;
  a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.mask_batch_stride = mask_batch_stride; a.mask_slice_stride = mask_slice_stride;
  a.ld = ld; a.ld_mask = ld_mask; a.n_slice = n_slice; a.n_pix = n_pix; a.C4 = C / 4;
  a.mask = mask_out; a.level_map = level_map; a.map_batch_stride = map_batch_stride;
  const int segs = n_batch * n_slice;
  const int nvec = n_pix * (C / 4);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, 8.0 * (double)n * segs);
  if (nvec <= 4 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<4, true, MaskMapArgs>), dim3(segs), dim3(1024), 0, s, a);
  else if (nvec <= 16 * 1024)
    hipLaunchKernelGGL((variance_mask_levels_kernel<16, true, MaskMapArgs>), dim3(segs), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL((variance_mask_levels_kernel<0, true, MaskMapArgs>), dim3(segs), dim3(1024), 0, s, a);
  return check_launch("variance_mask_map_kernel");
}
