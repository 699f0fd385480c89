// Picture-wide quality marks of tiled pictures: ONE sigma threshold per (mark, slice) over the pool
// of all tiles' sigmas, bit-exact to torch.quantile of the pool, and from it every tile's own count.
//
// The pool of slice j is the multiset of the T * n sigmas of slice j of all T tiles.  It never exists as one array: the
// tiles are produced a group at a time, and each (tile, slice) segment is already sorted (vam_variance_rank).  So
//   vam_pool_keys         writes each segment in rank order as rank_order.hip's canonical uint32 keys (ascending key =
//                         descending sigma, -0.0 == +0.0, every NaN the all-ones key, last) into rows of keys[T][ns][n];
//   vam_pooled_select     finds an order statistic of T sorted rows WITHOUT a sort: it descends the 32 key bits, and for
//                         each candidate key sums a per-row lower_bound over the rows; then ATen's lerp (quantile.h);
//   vam_threshold_counts  counts, per (mark, tile, slice), the keys whose sigma is >= the threshold: one binary search.
// One workgroup per (slice, level); its result depends on its own block reductions only: no workgroup waits on another,
// no atomics, no allocation; every launch is capturable.
#include "common.h"
#include "quantile.h"
#include <cstdint>

namespace vam {
namespace {

constexpr int kSelThreads = 256;
constexpr long kPoolMaxN = 16000000L;      // torch.quantile's limit (ATen Sorting.cpp), as vam_variance_mask refuses it
constexpr long kPoolMaxSeg = 1L << 18;     // vam_variance_rank's largest segment

struct PoolKeyArgs {
  const float* sigma;
  const int32_t* perm;
  unsigned* keys;            // row (t0 + b, j) at ((t0 + b) * n_slice + j) * n
  long batch_stride, slice_stride;
  int ld, n_slice, n_pix, C, n, t0;
};

__global__ __launch_bounds__(256) void pool_keys_kernel(const PoolKeyArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const int seg = blockIdx.y;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  const int e = a.perm[(long)seg * a.n + r];
  unsigned key = 0xFFFFFFFFu;                              // not a permutation: read nothing outside the view
  if ((unsigned)e < (unsigned)a.n) {
    const int c = e / a.n_pix, p = e - c * a.n_pix;
    key = rank_sigma_bits(a.sigma[b * a.batch_stride + j * a.slice_stride + (long)p * a.ld + c]);
  }
  a.keys[((long)(a.t0 + b) * a.n_slice + j) * a.n + r] = key;
}

struct SelectArgs {
  const unsigned* keys;      // [T][n_slice][n], every row ascending
  float* thr;                // [n_levels][n_slice]
  int T, n_slice, n;
  int k_lo[VAM_MAX_LAYER_LEVELS], k_hi[VAM_MAX_LAYER_LEVELS];
  float w[VAM_MAX_LAYER_LEVELS];
  int mode[VAM_MAX_LAYER_LEVELS];
};

// #(keys of the row < key): the row is ascending
__device__ __forceinline__ int row_lower_bound(const unsigned* row, int n, unsigned key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Sum of v over the workgroup (a pool holds at most 16M elements: an int), the same value in every thread: wave-64 shuffles,
// then LDS across the waves.
__device__ __forceinline__ int block_sum(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();                                         // the previous call's readers of sh are done
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int i = 0; i < kSelThreads / 64; ++i) s += sh[i];
  return s;
}

// The m-th smallest key (0-based) of the pool of slice j: the largest x with #(key < x) <= m, one bit at a time.
__device__ unsigned pool_order_statistic(const SelectArgs& a, int j, int m, int* sh) {
  unsigned prefix = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cand = prefix | (1u << bit);
    int below = 0;
    for (int t = threadIdx.x; t < a.T; t += kSelThreads)
      below += row_lower_bound(a.keys + ((long)t * a.n_slice + j) * a.n, a.n, cand);
    if (block_sum(below, sh) <= m) prefix = cand;
  }
  return prefix;
}

__global__ __launch_bounds__(kSelThreads) void pooled_select_kernel(const SelectArgs a) {
  __shared__ int sh[kSelThreads / 64];
  const int j = blockIdx.x, lv = blockIdx.y;
  float* out = a.thr + (long)lv * a.n_slice + j;
  if (a.mode[lv] != 0) {
    if (threadIdx.x == 0) *out = a.mode[lv] == 2 ? -INFINITY : INFINITY;
    return;
  }
  int nan = 0;                                             // the NaNs are the all-ones key, at the end of their row
  for (int t = threadIdx.x; t < a.T; t += kSelThreads)
    nan += a.keys[((long)t * a.n_slice + j) * a.n + (a.n - 1)] == 0xFFFFFFFFu ? 1 : 0;
  nan = block_sum(nan, sh);
  // keys ascend as sigma descends: sorted_ascending_sigma[k] is the key of index N - 1 - k
  const int N = a.T * a.n;
  const unsigned key_lo = pool_order_statistic(a, j, N - 1 - a.k_lo[lv], sh);
  const unsigned key_hi = a.k_hi[lv] != a.k_lo[lv] ? pool_order_statistic(a, j, N - 1 - a.k_hi[lv], sh) : key_lo;
  float thr = quantile_lerp(a.w[lv], rank_bits_sigma(key_lo), rank_bits_sigma(key_hi));
  if (nan) thr = __uint_as_float(0x7FC00000u);
  if (threadIdx.x == 0) *out = thr;
}

struct CountArgs {
  const unsigned* keys;      // [T][n_slice][n]
  const float* thr;          // [n_levels][n_slice]
  int32_t* count;            // [n_levels][T][n_slice]
  int T, n_slice, n, n_levels;
};

// sigma >= thr holds on a prefix of a row (descending sigma, NaNs last), so the count is the first index where it fails.
// Compared as floats: -0.0 >= +0.0, and nothing is >= a NaN threshold.  A threshold of -inf is the mark "everything": n.
__global__ __launch_bounds__(256) void threshold_counts_kernel(const CountArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long rows = (long)a.T * a.n_slice;
  if (i >= rows * a.n_levels) return;
  const int lv = (int)(i / rows);
  const long row = i - lv * rows;
  const int j = (int)(row % a.n_slice);
  const float thr = a.thr[(long)lv * a.n_slice + j];
  const unsigned* keys = a.keys + row * a.n;
  int lo = 0, hi = a.n;
  if (__float_as_uint(thr) == 0xFF800000u) lo = a.n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rank_bits_sigma(keys[mid]) >= thr) lo = mid + 1;
    else hi = mid;
  }
  a.count[i] = lo;
}

int pool_shape(const char* what, int T, int n_slice, long n) {
  VAM_REQUIRE(T > 0 && n_slice > 0 && n > 0, "%s: need T, n_slice, n > 0", what);
  VAM_REQUIRE(n <= kPoolMaxSeg, "%s: a segment of %ld elements exceeds the supported %ld", what, n, kPoolMaxSeg);
  VAM_REQUIRE((long)T * n <= kPoolMaxN, "%s: a pool of %ld elements exceeds torch.quantile's 16M limit", what, (long)T * n);
  VAM_REQUIRE(n_slice <= 65535 && (long)T * n_slice <= (1L << 24), "%s: %ld rows exceed one launch", what, (long)T * n_slice);
  return VAM_OK;
}

}  // namespace
}  // namespace vam

using namespace vam;

extern "C" {

int vam_pool_keys(const float* sigma, int ld, long batch_stride, long slice_stride, const int32_t* perm, int n_batch,
                  int n_slice, int n_pix, int C, uint32_t* keys, int t0, int T, void* stream) {
  VAM_REQUIRE(sigma && perm && keys, "vam_pool_keys: need sigma, perm and keys");
  VAM_REQUIRE(n_batch > 0 && n_pix > 0 && C > 0 && ld >= C, "vam_pool_keys: need n_batch, n_pix, C > 0 and ld >= C");
  const long n = (long)n_pix * C;
  if (int rc = pool_shape("vam_pool_keys", T, n_slice, n)) return rc;
  VAM_REQUIRE(t0 >= 0 && (long)t0 + n_batch <= T, "vam_pool_keys: rows [%d, %ld) lie outside the %d tiles of the buffer", t0,
              (long)t0 + n_batch, T);
  VAM_REQUIRE((long)n_batch * n_slice <= 65535, "vam_pool_keys: %ld segments exceed one launch (65535)", (long)n_batch * n_slice);
  PoolKeyArgs a;
  a.sigma = sigma; a.perm = perm; a.keys = keys; a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.ld = ld; a.n_slice = n_slice; a.n_pix = n_pix; a.C = C; a.n = (int)n; a.t0 = t0;
  ProfScope ps(VAM_FAM_MASK, (hipStream_t)stream, 0, (double)n_batch * n_slice * n * 12.0);
  hipLaunchKernelGGL(pool_keys_kernel, dim3(cdiv(n, 256), n_batch * n_slice), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("pool_keys_kernel");
}

int vam_pooled_select(const uint32_t* keys, int T, int n_slice, int n, const double* prs, int n_levels, float* thr_out,
                      void* stream) {
  VAM_REQUIRE(keys && prs && thr_out, "vam_pooled_select: need keys, prs and thr_out");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "vam_pooled_select: 1..%d levels, got %d", VAM_MAX_LAYER_LEVELS,
              n_levels);
  if (int rc = pool_shape("vam_pooled_select", T, n_slice, n)) return rc;
  SelectArgs a;
  a.keys = keys; a.thr = thr_out; a.T = T; a.n_slice = n_slice; a.n = n;
  for (int lv = 0; lv < n_levels; ++lv) {
    VAM_REQUIRE(prs[lv] > 0.0, "vam_pooled_select: a mark quality is > 0, got prs[%d] = %g", lv, prs[lv]);
    VAM_REQUIRE(lv == 0 || prs[lv] >= prs[lv - 1], "vam_pooled_select: qualities must be non-decreasing (prs[%d] < prs[%d])", lv,
                lv - 1);
    if (int rc = quantile_level(prs[lv], (long)T * n, &a.k_lo[lv], &a.k_hi[lv], &a.w[lv], &a.mode[lv])) return rc;
  }
  ProfScope ps(VAM_FAM_MASK, (hipStream_t)stream, 0, 0);
  hipLaunchKernelGGL(pooled_select_kernel, dim3(n_slice, n_levels), dim3(kSelThreads), 0, (hipStream_t)stream, a);
  return check_launch("pooled_select_kernel");
}

int vam_threshold_counts(const uint32_t* keys, int T, int n_slice, int n, const float* thr, int n_levels, int32_t* count_out,
                         void* stream) {
  VAM_REQUIRE(keys && thr && count_out, "vam_threshold_counts: need keys, thr and count_out");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "vam_threshold_counts: 1..%d levels, got %d",
              VAM_MAX_LAYER_LEVELS, n_levels);
  if (int rc = pool_shape("vam_threshold_counts", T, n_slice, n)) return rc;
  CountArgs a;
  a.keys = keys; a.thr = thr; a.count = count_out; a.T = T; a.n_slice = n_slice; a.n = n; a.n_levels = n_levels;
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 0);
  hipLaunchKernelGGL(threshold_counts_kernel, dim3(cdiv((long)T * n_slice * n_levels, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("threshold_counts_kernel");
}

}  // extern "C"
