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
//
// Every entry point of this file is one instantiation of variance_mask_select_kernel<MAXV, Args>: the argument kind says
// where the levels' ranks come from (the kernel arguments or a device table), where the masks go and which last pass runs.
#include "common.h"
#include "quantile.h"
#include <cmath>
#include <cstdio>
#include <cstring>

namespace vam {

// what every kind shares: the segments of sigma, and the window of the same layout that receives the float masks, the
// uint8 layer ids (PASS_LAYERS) or the one float mask of a quality map (PASS_MAP)
struct MaskGeom {
  const float* sigma;
  void* out;
  float* thr;
  long batch_stride, slice_stride, mask_batch_stride, mask_slice_stride;
  int ld, ld_mask, n_slice, n_pix, C4;
};

// what follows the levels' selections: nothing (every level stored its own mask), the layer id of every element, or one
// mask in which every pixel takes its own level
enum LastPass { PASS_NONE, PASS_LAYERS, PASS_MAP };

// vam_variance_mask: one level, its fields in the kernel arguments
struct OneLevel {
  int any_select;
  int k_lo[1], k_hi[1];
  float w[1];
  int mode[1];  // 0 = quantile, 1 = all zero (pr == 0), 2 = all one (pr >= 10)
};
struct MaskOneArgs : MaskGeom {
  static constexpr LastPass kLast = PASS_NONE;
  OneLevel rec;
  __device__ const OneLevel& record(int) const { return rec; }
  __device__ int count(const OneLevel&) const { return 1; }
  __device__ long level_stride() const { return 0L; }
};

// vam_variance_mask_levels (PASS_NONE) and vam_variance_layers (PASS_LAYERS): one quality list, its record in the kernel
// arguments; the host validated the count
template <LastPass LAST>
struct MaskListArgs : MaskGeom {
  static constexpr LastPass kLast = LAST;
  long mask_level_stride;
  vam_layer_params rec;
  __device__ const vam_layer_params& record(int) const { return rec; }
  __device__ int count(const vam_layer_params& r) const { return r.n_levels; }
  __device__ long level_stride() const { return mask_level_stride; }
};

// vam_variance_masks_per_image (PASS_NONE), vam_variance_layers_per_image (PASS_LAYERS) and vam_variance_mask_map (PASS_MAP):
// image b's record of a device table (a list of 32 qualities per image does not fit the kernel arguments of a batch).
// A record with more levels than the outputs hold (max_levels; thresholds in LDS: VAM_MAX_LAYER_LEVELS) selects nothing.
template <LastPass LAST>
struct MaskTableArgs : MaskGeom {
  static constexpr LastPass kLast = LAST;
  const vam_layer_params* table;
  long mask_level_stride;
  int max_levels;
  const uint8_t* level_map;  // PASS_MAP: pixel p of image b takes level level_map[b * map_batch_stride + p]
  long map_batch_stride;
  __device__ const vam_layer_params& record(int b) const { return table[b]; }
  __device__ int count(const vam_layer_params& r) const {
    const int cap = LAST == PASS_NONE ? max_levels : VAM_MAX_LAYER_LEVELS;
    return r.n_levels < 0 || r.n_levels > cap ? 0 : r.n_levels;
  }
  __device__ long level_stride() const { return mask_level_stride; }
};

// float4 i of a segment (or of its mask) with pixel stride ld
__device__ __forceinline__ long vec_offset(int i, int C4, int ld) {
  const int p = i / C4;
  return (long)p * ld + (i - p * C4) * 4;
}

// One segment in the hands of its workgroup.  MAXV = float4 per thread kept in registers (0 = stream from memory every pass)
template <int MAXV>
struct Segment {
  float4 reg[MAXV > 0 ? MAXV : 1];
  const float* src;
  int nvec, C4, ld, tid;

  __device__ __forceinline__ float4 at(int i) const { return *reinterpret_cast<const float4*>(src + vec_offset(i, C4, ld)); }
  __device__ __forceinline__ void load() {
    if constexpr (MAXV > 0) {
#pragma unroll
      for (int r = 0; r < MAXV; ++r) {
        int i = tid + r * 1024;
        reg[r] = (i < nvec) ? at(i) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
  // visit every float4 of the segment: f(index, float4)
  template <class F>
  __device__ __forceinline__ void for_each_vec(F&& f) const {
    if constexpr (MAXV > 0) {
#pragma unroll
      for (int r = 0; r < MAXV; ++r) {
        int i = tid + r * 1024;
        if (i < nvec) f(i, reg[r]);
      }
    } else {
      for (int i = tid; i < nvec; i += 1024) f(i, at(i));
    }
  }
  // visit every element of the segment: f(float)
  template <class F>
  __device__ __forceinline__ void for_each(F&& f) const {
    for_each_vec([&](int, float4 v) { f(v.x); f(v.y); f(v.z); f(v.w); });
  }
};

// what the passes of a selection hand on in LDS, next to the 256-bin histogram of a radix pass
struct SelectShared {
  unsigned prefix, k, cnt, min;
  int nan;
};

// sh.nan = the segment holds a NaN (read it behind a barrier: every select_threshold has several)
template <int MAXV>
__device__ __forceinline__ void scan_nan(const Segment<MAXV>& s, SelectShared& sh) {
  if (s.tid == 0) sh.nan = 0;
  __syncthreads();
  int nan = 0;
  s.for_each([&](float x) { nan |= (x != x) ? 1 : 0; });
  if (nan) atomicOr(&sh.nan, 1);
}

// lerp(sorted[k_lo], sorted[k_hi], w) of the segment, the same value in every thread
template <int MAXV>
__device__ __forceinline__ float select_threshold(const Segment<MAXV>& s, unsigned* hist, SelectShared& sh, int k_lo, int k_hi, float w) {
  const int tid = s.tid;
  // ---- radix select of rank k_lo (ascending, 0-based)
  if (tid == 0) { sh.prefix = 0u; sh.k = (unsigned)k_lo; }
  for (int pass = 3; pass >= 0; --pass) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = sh.prefix;
    const int shift = pass * 8;
    const unsigned hi_mask = pass == 3 ? 0u : (0xFFFFFFFFu << (shift + 8));
    s.for_each([&](float x) {
      // 16 float4 per thread: the key is formed anew in every pass (kept next to the values, the keys would spill)
      if constexpr (MAXV > 4) asm volatile("" : "+v"(x));
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
      const unsigned k = sh.k;
      if (k >= excl && k < incl) {
        unsigned kk = k - excl;
        unsigned bin;
        if (kk < h0) bin = 0;
        else if ((kk -= h0) < h1) bin = 1;
        else if ((kk -= h1) < h2) bin = 2;
        else { kk -= h2; bin = 3; }
        sh.prefix = prefix | ((unsigned)(tid * 4 + bin) << shift);
        sh.k = kk;
      }
    }
    __syncthreads();
  }
  const unsigned key_lo = sh.prefix;
  unsigned key_hi = key_lo;
  if (k_hi != k_lo) {
    // sorted[k_lo+1]: equals key_lo when more than k_lo+1 elements are <= key_lo, else the
    // smallest key above it.
    if (tid == 0) { sh.cnt = 0u; sh.min = 0xFFFFFFFFu; }
    __syncthreads();
    unsigned cnt = 0u, mn = 0xFFFFFFFFu;
    s.for_each([&](float x) {
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
    if ((tid & 63) == 0) { atomicAdd(&sh.cnt, cnt); atomicMin(&sh.min, mn); }
    __syncthreads();
    key_hi = (sh.cnt > (unsigned)k_lo + 1u) ? key_lo : sh.min;
  }
  return quantile_lerp(w, key2f(key_lo), key2f(key_hi));
}

__device__ __forceinline__ float4 mask_ge(float4 v, float thr) {
  return make_float4(v.x >= thr ? 1.f : 0.f, v.y >= thr ? 1.f : 0.f, v.z >= thr ? 1.f : 0.f, v.w >= thr ? 1.f : 0.f);
}

// a level without a threshold: every float4 of its mask is c (no value of the segment is read)
template <int MAXV>
__device__ __forceinline__ void fill_mask(const Segment<MAXV>& s, float* dst, int ld_mask, float c) {
  for (int i = s.tid; i < s.nvec; i += 1024) *reinterpret_cast<float4*>(dst + vec_offset(i, s.C4, ld_mask)) = make_float4(c, c, c, c);
}

// dst's float4 i = f(index, the segment's float4 i)
template <int MAXV, class F>
__device__ __forceinline__ void store_mask(const Segment<MAXV>& s, float* dst, int ld_mask, F&& f) {
  s.for_each_vec([&](int i, float4 v) { *reinterpret_cast<float4*>(dst + vec_offset(i, s.C4, ld_mask)) = f(i, v); });
}

// ---- layer assignment: layer <= k  <=>  mask_k == 1 (the masks of a non-decreasing quality list are nested)
template <int MAXV>
__device__ __forceinline__ void store_layers(const Segment<MAXV>& s, uint8_t* dst, int ld_layer, const vam_layer_params& rec,
                                             int n_lv, const float* sh_thr) {
  auto layer_of = [&](float x) -> unsigned {
    for (int lv = 0; lv < n_lv; ++lv) {
      const int md = rec.mode[lv];
      if (md == 2 || (md == 0 && x >= sh_thr[lv])) return (unsigned)lv;
    }
    return 0xFFu;
  };
  s.for_each_vec([&](int i, float4 v) {
    const unsigned word = layer_of(v.x) | (layer_of(v.y) << 8) | (layer_of(v.z) << 16) | (layer_of(v.w) << 24);
    *reinterpret_cast<unsigned*>(dst + vec_offset(i, s.C4, ld_layer)) = word;
  });
}

// ---- quality map: pixel p keeps x >= the threshold of ITS level (all one / all zero for the levels without one; zero for a
// map entry beyond the image's list)
template <int MAXV>
__device__ __forceinline__ void store_map(const Segment<MAXV>& s, float* dst, int ld_mask, const vam_layer_params& rec, int n_lv,
                                          const uint8_t* lmap, const float* sh_thr, int* sh_md) {
  if (s.tid < VAM_MAX_LAYER_LEVELS) sh_md[s.tid] = s.tid < n_lv ? rec.mode[s.tid] : 1;
  __syncthreads();
  store_mask(s, dst, ld_mask, [&](int i, float4 v) {
    const int lv = (int)lmap[i / s.C4];
    const int md = lv < VAM_MAX_LAYER_LEVELS ? sh_md[lv] : 1;
    if (md != 0) {
      const float c = md == 2 ? 1.f : 0.f;
      return make_float4(c, c, c, c);
    }
    return mask_ge(v, sh_thr[lv]);
  });
}

// The segment is loaded once; each level then runs its own selection on the same registers and either writes its own
// mask (PASS_NONE) or leaves its threshold in LDS for the last pass.
template <int MAXV, class Args>
__global__ __launch_bounds__(1024) void variance_mask_select_kernel(const Args a) {
  constexpr LastPass LAST = Args::kLast;
  __shared__ unsigned hist[256];
  __shared__ SelectShared sh;
  __shared__ float sh_thr[LAST != PASS_NONE ? VAM_MAX_LAYER_LEVELS : 1];
  [[maybe_unused]] __shared__ int sh_md[LAST == PASS_MAP ? VAM_MAX_LAYER_LEVELS : 1];

  const int seg = blockIdx.x;
  const int segs = gridDim.x;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  const int tid = threadIdx.x;
  const long out_off = b * a.mask_batch_stride + j * a.mask_slice_stride;
  const auto& rec = a.record(b);
  const int n_lv = a.count(rec);
  auto level_dst = [&](int lv) { return static_cast<float*>(a.out) + out_off + lv * a.level_stride(); };   // PASS_NONE

  Segment<MAXV> s;
  s.src = a.sigma + b * a.batch_stride + j * a.slice_stride;
  s.nvec = a.n_pix * a.C4; s.C4 = a.C4; s.ld = a.ld; s.tid = tid;
  if (LAST != PASS_NONE || rec.any_select) s.load();   // a list of qualities 0 and >= 10 only fills: it reads no sigma
  if (rec.any_select) scan_nan(s, sh);

  for (int lv = 0; lv < n_lv; ++lv) {
    const int md = rec.mode[lv];
    float thr;
    if (md != 0) {
      thr = md == 2 ? -INFINITY : INFINITY;
      if constexpr (LAST == PASS_NONE) {
        fill_mask(s, level_dst(lv), a.ld_mask, md == 2 ? 1.f : 0.f);
      }
    } else {
      if (lv > 0) __syncthreads();  // the previous level's readers of sh.prefix / sh.cnt / sh.min are done (the first has none)
      thr = select_threshold(s, hist, sh, rec.k_lo[lv], rec.k_hi[lv], rec.w[lv]);
      if (sh.nan) thr = __uint_as_float(0x7FC00000u);
      if constexpr (LAST == PASS_NONE) {
        store_mask(s, level_dst(lv), a.ld_mask, [&](int, float4 v) { return mask_ge(v, thr); });
      } else {
        if (tid == 0) sh_thr[lv] = thr;
      }
    }
    if (tid == 0 && a.thr) a.thr[(long)lv * segs + seg] = thr;
  }

  if constexpr (LAST != PASS_NONE) __syncthreads();
  if constexpr (LAST == PASS_LAYERS) store_layers(s, static_cast<uint8_t*>(a.out) + out_off, a.ld_mask, rec, n_lv, sh_thr);
  if constexpr (LAST == PASS_MAP)
    store_map(s, static_cast<float*>(a.out) + out_off, a.ld_mask, rec, n_lv, a.level_map + b * a.map_batch_stride, sh_thr, sh_md);
}

// ------------------------------------------------------------------------------------------------ host
// The rules every entry point shares, and the geometry they admit.  out: 16-byte aligned float masks (out_align 16) or 4-byte
// aligned layer ids; others: the entry's further pointers are there; table: a device table (4-byte aligned) or NULL for none.
static int check_segments(const char* what, const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                          int n_slice, int n_pix, int C, void* out, int out_align, int ld_out, long out_batch_stride,
                          long out_slice_stride, long out_level_stride, float* thr, bool others, const void* table, MaskGeom& g) {
  VAM_REQUIRE(sigma && out && others && n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "%s: bad arguments", what);
  VAM_REQUIRE(C % 4 == 0 && ld % 4 == 0 && ld_out % 4 == 0 && batch_stride % 4 == 0 && slice_stride % 4 == 0 &&
              out_batch_stride % 4 == 0 && out_slice_stride % 4 == 0 && out_level_stride % 4 == 0,
              "%s: C and strides must be multiples of 4", what);
  VAM_REQUIRE((((uintptr_t)sigma) & 15) == 0 && (((uintptr_t)out) & (out_align - 1)) == 0 && (((uintptr_t)table) & 3) == 0,
              "%s: alignment (sigma and float masks: 16-byte; layer ids and tables: 4-byte)", what);
  VAM_REQUIRE(ld >= C && ld_out >= C, "%s: pixel stride < C", what);
  const long n = (long)n_pix * C;
  // torch.quantile rejects inputs above 16M elements (ATen Sorting.cpp); so do we
  VAM_REQUIRE(n <= 16000000L, "%s: segment of %ld elements exceeds torch.quantile's 16M limit", what, n);
  g.sigma = sigma; g.out = out; g.thr = thr;
  g.batch_stride = batch_stride; g.slice_stride = slice_stride;
  g.mask_batch_stride = out_batch_stride; g.mask_slice_stride = out_slice_stride;
  g.ld = ld; g.ld_mask = ld_out; g.n_slice = n_slice; g.n_pix = n_pix; g.C4 = C / 4;
  return VAM_OK;
}

// rank / weight / mode of every quality of one list over segments of n elements (quantile_level per level), into a record
template <class Record>
static int fill_record(const char* what, const double* prs, int n_levels, int max_levels, bool sorted, long n, Record& rec) {
  VAM_REQUIRE(prs && n_levels >= 1 && n_levels <= max_levels, "%s: 1..%d levels, got %d", what, max_levels, n_levels);
  std::memset(&rec, 0, sizeof(rec));
  for (int lv = 0; lv < n_levels; ++lv) {
    VAM_REQUIRE(!sorted || lv == 0 || prs[lv] >= prs[lv - 1], "%s: qualities must be non-decreasing (prs[%d] < prs[%d])", what, lv, lv - 1);
    if (int rc = quantile_level(prs[lv], n, &rec.k_lo[lv], &rec.k_hi[lv], &rec.w[lv], &rec.mode[lv])) return rc;
    rec.any_select |= rec.mode[lv] == 0;
  }
  return VAM_OK;
}

// one workgroup per segment; bytes: the HBM traffic of the entry per element of sigma
template <class Args>
static int launch_by_size(const Args& a, int n_batch, double bytes, void* stream, const char* name) {
  const int segs = n_batch * a.n_slice;
  const int nvec = a.n_pix * a.C4;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, bytes * 4.0 * (double)nvec * segs);
  if (nvec <= 4 * 1024)
    hipLaunchKernelGGL((variance_mask_select_kernel<4, Args>), dim3(segs), dim3(1024), 0, s, a);
  else if (nvec <= 16 * 1024)
    hipLaunchKernelGGL((variance_mask_select_kernel<16, Args>), dim3(segs), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL((variance_mask_select_kernel<0, Args>), dim3(segs), dim3(1024), 0, s, a);
  return check_launch(name);
}

}  // namespace vam

using namespace vam;

extern "C" int vam_variance_mask(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                 int n_slice, int n_pix, int C, double pr, float* mask_out, int ld_mask,
                                 long mask_batch_stride, long mask_slice_stride, float* thr_out, void* stream) {
  MaskOneArgs a;
  if (int rc = check_segments("vam_variance_mask", sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, mask_out, 16,
                              ld_mask, mask_batch_stride, mask_slice_stride, 0, thr_out, true, nullptr, a)) return rc;
  if (int rc = fill_record("vam_variance_mask", &pr, 1, 1, false, (long)n_pix * C, a.rec)) return rc;
  return launch_by_size(a, n_batch, 8.0, stream, "variance_mask_select_kernel (vam_variance_mask)");
}

template <LastPass LAST>
static int list_launch(const char* what, const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                       int n_pix, int C, const double* prs, int n_levels, void* out, int ld_out, long out_batch_stride,
                       long out_slice_stride, long out_level_stride, float* thr_out, void* stream) {
  constexpr bool layers = LAST == PASS_LAYERS;
  MaskListArgs<LAST> a;
  if (int rc = check_segments(what, sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, out, layers ? 4 : 16, ld_out,
                              out_batch_stride, out_slice_stride, out_level_stride, thr_out, true, nullptr, a)) return rc;
  a.mask_level_stride = out_level_stride;
  if (int rc = fill_record(what, prs, n_levels, layers ? VAM_MAX_LAYER_LEVELS : VAM_MAX_MASK_LEVELS, layers, (long)n_pix * C, a.rec)) return rc;
  a.rec.n_levels = n_levels;
  return launch_by_size(a, n_batch, layers ? 5.0 : 4.0 + 4.0 * n_levels, stream, what);
}

extern "C" int vam_variance_mask_levels(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                        int n_slice, int n_pix, int C, const double* prs, int n_levels, float* mask_out,
                                        int ld_mask, long mask_batch_stride, long mask_slice_stride, long mask_level_stride,
                                        float* thr_out, void* stream) {
  return list_launch<PASS_NONE>("vam_variance_mask_levels", sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, prs,
                                n_levels, mask_out, ld_mask, mask_batch_stride, mask_slice_stride, mask_level_stride, thr_out, stream);
}

extern "C" int vam_variance_layers(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                                   int n_pix, int C, const double* prs, int n_levels, uint8_t* layer_out, int ld_layer,
                                   long layer_batch_stride, long layer_slice_stride, float* thr_out, void* stream) {
  return list_launch<PASS_LAYERS>("vam_variance_layers", sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, prs,
                                  n_levels, layer_out, ld_layer, layer_batch_stride, layer_slice_stride, 0, thr_out, stream);
}

extern "C" size_t vam_layer_params_size(void) { return sizeof(vam_layer_params); }

// the records of vam_variance_layers_per_image (sorted: non-decreasing lists of up to VAM_MAX_LAYER_LEVELS) and of
// vam_variance_masks_per_image (any order, up to VAM_MAX_MASK_LEVELS), one image at a time
static int image_params(const char* what, const char* entry, const double* prs, const int* n_levels, int n_batch, int levels_stride,
                        int n_pix, int C, vam_layer_params* table_host, int max_levels, bool sorted) {
  VAM_REQUIRE(prs && n_levels && table_host && n_batch > 0 && levels_stride >= 1 && n_pix > 0 && C > 0, "%s: bad arguments", what);
  const long n = (long)n_pix * C;
  VAM_REQUIRE(n <= 16000000L, "%s: segment of %ld elements exceeds torch.quantile's 16M limit", what, n);
  for (int b = 0; b < n_batch; ++b) {
    char image[96];
    std::snprintf(image, sizeof(image), "%s: image %d", entry, b);
    VAM_REQUIRE(n_levels[b] <= levels_stride || n_levels[b] > max_levels, "%s: 1..%d levels, got %d in rows of %d", image, max_levels,
                n_levels[b], levels_stride);
    if (int rc = fill_record(image, prs + (long)b * levels_stride, n_levels[b], max_levels, sorted, n, table_host[b])) return rc;
    table_host[b].n_levels = n_levels[b];
  }
  return VAM_OK;
}

extern "C" int vam_variance_layer_params(const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix,
                                         int C, vam_layer_params* table_host) {
  return image_params("vam_variance_layer_params", "vam_variance_layers_per_image", prs, n_levels, n_batch, levels_stride, n_pix, C,
                      table_host, VAM_MAX_LAYER_LEVELS, true);
}

extern "C" int vam_variance_mask_params(const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix,
                                        int C, vam_layer_params* table_host) {
  return image_params("vam_variance_mask_params", "vam_variance_masks_per_image", prs, n_levels, n_batch, levels_stride, n_pix, C,
                      table_host, VAM_MAX_MASK_LEVELS, false);
}

extern "C" int vam_variance_layers_per_image(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                             int n_slice, int n_pix, int C, const vam_layer_params* table_dev,
                                             uint8_t* layer_out, int ld_layer, long layer_batch_stride,
                                             long layer_slice_stride, float* thr_out, void* stream) {
  const char* what = "vam_variance_layers_per_image";
  MaskTableArgs<PASS_LAYERS> a = {};
  if (int rc = check_segments(what, sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, layer_out, 4, ld_layer,
                              layer_batch_stride, layer_slice_stride, 0, thr_out, table_dev != nullptr, table_dev, a)) return rc;
  a.table = table_dev;
  return launch_by_size(a, n_batch, 5.0, stream, what);
}

extern "C" int vam_variance_masks_per_image(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                            int n_slice, int n_pix, int C, const vam_layer_params* table_dev, int max_levels,
                                            float* mask_out, int ld_mask, long mask_batch_stride, long mask_slice_stride,
                                            long mask_level_stride, float* thr_out, void* stream) {
  const char* what = "vam_variance_masks_per_image";
  MaskTableArgs<PASS_NONE> a = {};
  if (int rc = check_segments(what, sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, mask_out, 16, ld_mask,
                              mask_batch_stride, mask_slice_stride, mask_level_stride, thr_out, table_dev != nullptr, table_dev, a)) return rc;
  VAM_REQUIRE(max_levels >= 1 && max_levels <= VAM_MAX_MASK_LEVELS, "%s: 1..%d levels, got %d", what, VAM_MAX_MASK_LEVELS, max_levels);
  a.table = table_dev; a.mask_level_stride = mask_level_stride; a.max_levels = max_levels;
  return launch_by_size(a, n_batch, 4.0 + 4.0 * max_levels, stream, what);
}

extern "C" int vam_variance_mask_map(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                                     int n_pix, int C, const vam_layer_params* table_dev, const uint8_t* level_map,
                                     long map_batch_stride, float* mask_out, int ld_mask, long mask_batch_stride,
                                     long mask_slice_stride, float* thr_out, void* stream) {
  const char* what = "vam_variance_mask_map";
  MaskTableArgs<PASS_MAP> a = {};
  VAM_REQUIRE(map_batch_stride >= n_pix, "%s: map_batch_stride %ld < n_pix %d", what, map_batch_stride, n_pix);
  if (int rc = check_segments(what, sigma, ld, batch_stride, slice_stride, n_batch, n_slice, n_pix, C, mask_out, 16, ld_mask,
                              mask_batch_stride, mask_slice_stride, 0, thr_out, table_dev && level_map, table_dev, a)) return rc;
  a.table = table_dev; a.level_map = level_map; a.map_batch_stride = map_batch_stride;
  return launch_by_size(a, n_batch, 8.0, stream, what);
}
