// Rank order of the progressive latents (embedded streams): per (image, slice) segment the
// permutation that sorts its n = C * h * w elements by descending sigma, and the gather / scatter that move symbols
// and table indexes between the NHWC views of the plans and that order.
//
// The variance mask of every quality keeps the elements with sigma >= a quantile, so all masks of a segment are
// prefixes of ONE ordering.  The ordering is pinned by a 64-bit key per element,
//     key = (~ordered_bits(sigma) << 32) | e,      e = c * h * w + y * w + x  (the [C, h, w] order of a stream),
// sorted ascending: descending sigma, equal values by ascending e, -0.0 == +0.0, +inf first, NaN last (all NaNs one
// value).  Keys are unique, so any correct sorting network gives numpy.argsort(-s, kind="stable") exactly.
//
// Bitonic network over NP = next power of two >= n keys, padded with sentinel keys (all ones, above every real key):
//   n <= 8192:  one 1024-thread workgroup per segment, the keys in 64 KiB of LDS, one launch (rank_chunk_kernel<true>)
//   larger:     the keys live in the caller's workspace; 8192-key chunks are sorted in LDS, every stage k > 8192 runs its
//               steps j >= 8192 as one global compare-exchange launch each (rank_global_step_kernel) and its steps
//               j <= 4096 in LDS again (rank_chunk_kernel<false>); the last stage writes the permutation.
// No allocation and no atomics; every launch is capturable.
//
// Scheduled streams: vam_stage_ids turns the layer ids of vam_variance_layers_per_image and a
// schedule's per-image stage maps into a stage id per element, and vam_variance_rank_staged sorts with that id as the
// major key,
//     key = (stage << 56) | (~ordered_bits(sigma) << 24) | e,      e < 2^18 in the low 24 bits,
// through the same network, chunks, workspace and passes (the STAGED template flag of the key build and the final write).
#include "common.h"
#include "quantile.h"
#include <cstdint>

namespace vam {
namespace {

typedef unsigned long long u64;
constexpr int kRankChunk = 8192;          // keys of one LDS chunk: 64 KiB
constexpr int kRankThreads = 1024;
constexpr long kRankMaxN = 1L << 18;
constexpr u64 kRankSentinel = ~0ull;

struct RankArgs {
  const float* sigma;
  const uint8_t* stage;   // STAGED: the ids of vam_stage_ids, pixel stride ld_stage, slice j at channel j * C
  u64* ws;
  int32_t* perm;
  long batch_stride, slice_stride;
  int ld, ld_stage, n_slice, n_pix, C, n, np, ch;
  int k;       // rank_chunk_kernel<false> / rank_global_step_kernel: the stage
  int j;       // rank_global_step_kernel: the step
};

__device__ __forceinline__ u64 rank_key(float s, unsigned e) { return ((u64)rank_sigma_bits(s) << 32) | e; }

// The scheduled key: e < 2^18 (kRankMaxN) leaves the low 24 bits to it; stage 0xFF with a NaN still lies below the
// all-ones sentinel because e never reaches 0xFFFFFF.
__device__ __forceinline__ u64 rank_key_staged(unsigned stage, float s, unsigned e) {
  return ((u64)stage << 56) | ((u64)rank_sigma_bits(s) << 24) | e;
}

// One compare-exchange step of the network on an LDS chunk whose first key has global index `base`.
__device__ __forceinline__ void lds_step(u64* keys, int ch, int base, int k, int j) {
  for (int t = threadIdx.x; t < (ch >> 1); t += kRankThreads) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int l = i + j;
    const bool up = ((base + i) & k) == 0;
    const u64 a = keys[i], b = keys[l];
    if ((a > b) == up) {
      keys[i] = b;
      keys[l] = a;
    }
  }
  __syncthreads();
}

// FIRST: build the keys of chunk blockIdx.x of segment blockIdx.y from sigma and run the stages k = 2 .. ch.
// else:  load the chunk from the workspace and run the steps j = ch/2 .. 1 of stage a.k.
// The chunk goes to the permutation when the network is complete (stage np done), else back to the workspace.
// STAGED: the stage id is the major key and e sits in the low 24 bits (vam_variance_rank_staged).
template <bool FIRST, bool STAGED>
__global__ __launch_bounds__(kRankThreads) void rank_chunk_kernel(const RankArgs a) {
  extern __shared__ u64 keys[];
  const int seg = blockIdx.y;
  const int base = blockIdx.x * a.ch;
  u64* ws = a.ws ? a.ws + (long)seg * a.np + base : nullptr;
  if (FIRST) {
    const int b = seg / a.n_slice, jj = seg - b * a.n_slice;
    const float* src = a.sigma + b * a.batch_stride + jj * a.slice_stride;
    const uint8_t* sid = STAGED ? a.stage + (long)b * a.n_pix * a.ld_stage + jj * a.C : nullptr;
    for (int t = threadIdx.x; t < a.ch; t += kRankThreads) {
      const int g = base + t;                              // memory order (pixel, channel): coalesced over the window
      u64 key = kRankSentinel;
      if (g < a.n) {
        const int p = g / a.C, c = g - p * a.C;
        const unsigned e = (unsigned)(c * a.n_pix + p);
        const float s = src[(long)p * a.ld + c];
        key = STAGED ? rank_key_staged(sid[(long)p * a.ld_stage + c], s, e) : rank_key(s, e);
      }
      keys[t] = key;
    }
    __syncthreads();
    for (int k = 2; k <= a.ch; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) lds_step(keys, a.ch, base, k, j);
  } else {
    for (int t = threadIdx.x; t < a.ch; t += kRankThreads) keys[t] = ws[t];
    __syncthreads();
    for (int j = a.ch >> 1; j > 0; j >>= 1) lds_step(keys, a.ch, base, a.k, j);
  }
  const bool done = FIRST ? a.np == a.ch : a.k == a.np;
  if (done) {
    int32_t* out = a.perm + (long)seg * a.n;
    for (int t = threadIdx.x; t < a.ch; t += kRankThreads)
      if (base + t < a.n)                                                 // the sentinels sit behind every real key
        out[base + t] = STAGED ? (int32_t)((unsigned)keys[t] & 0xFFFFFFu) : (int32_t)(unsigned)keys[t];
  } else {
    for (int t = threadIdx.x; t < a.ch; t += kRankThreads) ws[t] = keys[t];
  }
}

// Step j >= kRankChunk of stage k on the workspace: one compare-exchange per thread.
__global__ __launch_bounds__(256) void rank_global_step_kernel(const RankArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (a.np >> 1)) return;
  u64* keys = a.ws + (long)blockIdx.y * a.np;
  const int i = ((t & ~(a.j - 1)) << 1) | (t & (a.j - 1));
  const int l = i + a.j;
  const bool up = (i & a.k) == 0;
  const u64 x = keys[i], y = keys[l];
  if ((x > y) == up) {
    keys[i] = y;
    keys[l] = x;
  }
}

struct GatherArgs {
  const int32_t* in0;
  const int32_t* in1;
  const int32_t* perm;
  int32_t* out0;
  int32_t* out1;
  int ld0, ld1, n_slice, n_pix, C, n;
};

__global__ __launch_bounds__(256) void rank_gather_kernel(const GatherArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const int seg = blockIdx.y;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  const int e = a.perm[(long)seg * a.n + r];
  if ((unsigned)e >= (unsigned)a.n) return;                // not a permutation: touch nothing outside the views
  const int c = e / a.n_pix, p = e - c * a.n_pix;
  const long pix = (long)b * a.n_pix + p;
  a.out0[(long)seg * a.n + r] = a.in0[pix * a.ld0 + j * a.C + c];
  if (a.in1) a.out1[(long)seg * a.n + r] = a.in1[pix * a.ld1 + j * a.C + c];
}

struct ScatterArgs {
  const int32_t* ranked;
  const int32_t* perm;
  const int32_t* count;      // [n_levels][n_seg]
  int32_t* sym;
  uint8_t* id;
  int ld_sym, ld_id, n_slice, n_pix, C, n, n_levels, n_seg;
};

__global__ __launch_bounds__(256) void rank_scatter_kernel(const ScatterArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const int seg = blockIdx.y;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  const int e = a.perm[(long)seg * a.n + r];
  if ((unsigned)e >= (unsigned)a.n) return;
  int id = 0xFF;
  for (int g = a.n_levels - 1; g >= 0; --g)                // the smallest g with r < count[g]
    if (r < a.count[g * a.n_seg + seg]) id = g;
  const int v = r < a.count[(a.n_levels - 1) * a.n_seg + seg] ? a.ranked[(long)seg * a.n + r] : 0;
  const int c = e / a.n_pix, p = e - c * a.n_pix;
  const long pix = (long)b * a.n_pix + p;
  a.sym[pix * a.ld_sym + j * a.C + c] = v;
  a.id[pix * a.ld_id + j * a.C + c] = (uint8_t)id;
}

struct CountArgs {
  const uint8_t* layer;
  const int32_t* perm;
  int32_t* count;            // [n_levels][n_seg]
  int ld_layer, n_slice, n_pix, C, n, n_levels, n_seg;
};

// The layer ids of vam_variance_layers never decrease along the rank order (a mask is sigma >= threshold and the masks
// are nested), so #(id <= g) is the position of the first id > g: one binary search per (segment, level).
__global__ __launch_bounds__(256) void rank_counts_kernel(const CountArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_seg * a.n_levels) return;
  const int seg = t / a.n_levels, g = t - seg * a.n_levels;
  const int b = seg / a.n_slice, j = seg - b * a.n_slice;
  int lo = 0, hi = a.n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int e = a.perm[(long)seg * a.n + mid];
    int id = 0xFF;
    if ((unsigned)e < (unsigned)a.n) {
      const int c = e / a.n_pix, p = e - c * a.n_pix;
      id = a.layer[((long)b * a.n_pix + p) * a.ld_layer + j * a.C + c];
    }
    if (id <= g) lo = mid + 1;
    else hi = mid;
  }
  a.count[g * a.n_seg + seg] = lo;
}

struct StageArgs {
  const uint8_t* layer;
  const uint8_t* stage_map;  // [n_batch][VAM_MAX_LAYER_LEVELS][n_pix]
  const int32_t* n_stages;   // [n_batch]
  uint8_t* out;
  long total;                // n_batch * n_pix * Ct
  int ld_layer, ld_out, n_pix, Ct;
};

// stage(e) = the first stage whose map index at e's pixel reaches e's layer id (layer[e] <= k  <=>  mask_k[e] == 1), 0xFF
// when none does.  Stage count and maps come from device memory, so one captured launch serves every schedule.
__global__ __launch_bounds__(256) void stage_ids_kernel(const StageArgs a) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.total) return;
  const long pix = t / a.Ct;                                 // b * n_pix + p
  const int ch = (int)(t - pix * a.Ct);
  const int b = (int)(pix / a.n_pix), p = (int)(pix - (long)b * a.n_pix);
  const int l = a.layer[pix * a.ld_layer + ch];
  int ns = a.n_stages[b];
  if (ns < 1 || ns > VAM_MAX_LAYER_LEVELS) ns = 0;
  const uint8_t* map = a.stage_map + (long)b * VAM_MAX_LAYER_LEVELS * a.n_pix + p;
  int id = 0xFF;
  for (int k = 0; k < ns; ++k)
    if (map[(long)k * a.n_pix] >= l) {
      id = k;
      break;
    }
  a.out[pix * a.ld_out + ch] = (uint8_t)id;
}

int rank_shape(const char* what, int n_batch, int n_slice, int n_pix, int C, long* n_out) {
  VAM_REQUIRE(n_batch > 0 && n_slice > 0 && n_pix > 0 && C > 0, "%s: need n_batch, n_slice, n_pix, C > 0", what);
  VAM_REQUIRE((long)n_batch * n_slice <= 65535, "%s: %ld segments exceed one launch (65535)", what, (long)n_batch * n_slice);
  const long n = (long)n_pix * C;
  VAM_REQUIRE(n <= kRankMaxN, "%s: a segment of %ld elements exceeds the supported %ld (rank order is defined for "
              "segments up to 2^18 elements; code larger images in tiles)", what, n, kRankMaxN);
  *n_out = n;
  return VAM_OK;
}

int rank_np(long n) {
  int np = 2;
  while (np < n) np <<= 1;
  return np;
}

// vam_variance_rank (STAGED = false) and vam_variance_rank_staged: one network, one launch sequence.
template <bool STAGED>
int rank_launch(const char* what, const float* sigma, int ld, long batch_stride, long slice_stride, const uint8_t* stage,
                int ld_stage, int n_batch, int n_slice, int n_pix, int C, int32_t* perm_out, void* workspace,
                size_t workspace_bytes, void* stream) {
  long n;
  if (int rc = rank_shape(what, n_batch, n_slice, n_pix, C, &n)) return rc;
  VAM_REQUIRE(sigma && perm_out && ld >= C, "%s: need sigma, perm_out and ld >= C", what);
  const int np_ = rank_np(n);
  const size_t need = np_ > kRankChunk ? (size_t)n_batch * n_slice * np_ * sizeof(u64) : 0;
  VAM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (((uintptr_t)workspace) & 7) == 0),
              "%s: segments of %ld elements need an 8-byte aligned workspace of %zu bytes "
              "(vam_variance_rank_workspace), got %zu", what, n, need, workspace_bytes);
  RankArgs a;
  a.sigma = sigma; a.stage = stage; a.ws = need ? (u64*)workspace : nullptr; a.perm = perm_out;
  a.batch_stride = batch_stride; a.slice_stride = slice_stride;
  a.ld = ld; a.ld_stage = ld_stage; a.n_slice = n_slice; a.n_pix = n_pix; a.C = C; a.n = (int)n;
  a.np = rank_np(n); a.ch = a.np < kRankChunk ? a.np : kRankChunk;
  a.k = 0; a.j = 0;
  const int n_seg = n_batch * n_slice, chunks = a.np / a.ch;
  const size_t lds = (size_t)a.ch * sizeof(u64);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(VAM_FAM_MASK, s, 0, (double)n_seg * n * 8.0);
  hipLaunchKernelGGL((rank_chunk_kernel<true, STAGED>), dim3(chunks, n_seg), dim3(kRankThreads), lds, s, a);
  if (int rc = check_launch("rank_chunk_kernel<true>")) return rc;
  for (int k = 2 * kRankChunk; k <= a.np && chunks > 1; k <<= 1) {
    a.k = k;
    for (int j = k >> 1; j >= kRankChunk; j >>= 1) {
      a.j = j;
      hipLaunchKernelGGL(rank_global_step_kernel, dim3(cdiv(a.np >> 1, 256), n_seg), dim3(256), 0, s, a);
      if (int rc = check_launch("rank_global_step_kernel")) return rc;
    }
    hipLaunchKernelGGL((rank_chunk_kernel<false, STAGED>), dim3(chunks, n_seg), dim3(kRankThreads), lds, s, a);
    if (int rc = check_launch("rank_chunk_kernel<false>")) return rc;
  }
  return VAM_OK;
}

}  // namespace
}  // namespace vam

using namespace vam;

extern "C" {

size_t vam_variance_rank_workspace(int n_batch, int n_slice, int n_pix, int C) {
  long n;
  if (rank_shape("vam_variance_rank_workspace", n_batch, n_slice, n_pix, C, &n) != VAM_OK) return 0;
  const int np = rank_np(n);
  return np > kRankChunk ? (size_t)n_batch * n_slice * np * sizeof(u64) : 0;
}

int vam_variance_rank(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice, int n_pix,
                      int C, int32_t* perm_out, void* workspace, size_t workspace_bytes, void* stream) {
  return rank_launch<false>("vam_variance_rank", sigma, ld, batch_stride, slice_stride, nullptr, 0, n_batch, n_slice, n_pix, C,
                            perm_out, workspace, workspace_bytes, stream);
}

int vam_variance_rank_staged(const float* sigma, int ld, long batch_stride, long slice_stride, const uint8_t* stage,
                             int ld_stage, int n_batch, int n_slice, int n_pix, int C, int32_t* perm_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  VAM_REQUIRE(stage && ld_stage >= n_slice * C, "vam_variance_rank_staged: need stage and ld_stage >= n_slice * C");
  return rank_launch<true>("vam_variance_rank_staged", sigma, ld, batch_stride, slice_stride, stage, ld_stage, n_batch, n_slice,
                           n_pix, C, perm_out, workspace, workspace_bytes, stream);
}

int vam_stage_ids(const uint8_t* layer, int ld_layer, const uint8_t* stage_map, const int32_t* n_stages, int n_batch, int n_pix,
                  int C_total, uint8_t* stage_out, int ld_out, void* stream) {
  VAM_REQUIRE(layer && stage_map && n_stages && stage_out, "vam_stage_ids: need layer, stage_map, n_stages and stage_out");
  VAM_REQUIRE(n_batch > 0 && n_pix > 0 && C_total > 0 && ld_layer >= C_total && ld_out >= C_total,
              "vam_stage_ids: need n_batch, n_pix, C_total > 0 and pixel strides >= C_total");
  StageArgs a;
  a.layer = layer; a.stage_map = stage_map; a.n_stages = n_stages; a.out = stage_out;
  a.total = (long)n_batch * n_pix * C_total;
  a.ld_layer = ld_layer; a.ld_out = ld_out; a.n_pix = n_pix; a.Ct = C_total;
  VAM_REQUIRE(a.total <= (long)INT32_MAX * 256, "vam_stage_ids: %ld elements exceed one launch", a.total);
  ProfScope ps(VAM_FAM_MASK, (hipStream_t)stream, 0, (double)a.total * 2.0);
  hipLaunchKernelGGL(stage_ids_kernel, dim3((unsigned)cdiv(a.total, 256L)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("stage_ids_kernel");
}

int vam_rank_gather(const int32_t* in0, int ld0, const int32_t* in1, int ld1, const int32_t* perm, int n_batch, int n_slice,
                    int n_pix, int C, int32_t* out0, int32_t* out1, void* stream) {
  long n;
  if (int rc = rank_shape("vam_rank_gather", n_batch, n_slice, n_pix, C, &n)) return rc;
  VAM_REQUIRE(in0 && out0 && perm && ld0 >= n_slice * C, "vam_rank_gather: need in0, out0, perm and ld0 >= n_slice * C");
  VAM_REQUIRE(!in1 || (out1 && ld1 >= n_slice * C), "vam_rank_gather: in1 needs out1 and ld1 >= n_slice * C");
  GatherArgs a;
  a.in0 = in0; a.in1 = in1; a.perm = perm; a.out0 = out0; a.out1 = out1;
  a.ld0 = ld0; a.ld1 = ld1; a.n_slice = n_slice; a.n_pix = n_pix; a.C = C; a.n = (int)n;
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, (double)n_batch * n_slice * n * (in1 ? 20.0 : 12.0));
  hipLaunchKernelGGL(rank_gather_kernel, dim3(cdiv(n, 256), n_batch * n_slice), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("rank_gather_kernel");
}

int vam_rank_counts(const uint8_t* layer, int ld_layer, const int32_t* perm, int n_batch, int n_slice, int n_pix, int C,
                    int n_levels, int32_t* count_out, void* stream) {
  long n;
  if (int rc = rank_shape("vam_rank_counts", n_batch, n_slice, n_pix, C, &n)) return rc;
  VAM_REQUIRE(layer && perm && count_out && ld_layer >= n_slice * C, "vam_rank_counts: need layer, perm, count_out and ld_layer >= n_slice * C");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "vam_rank_counts: 1..%d levels, got %d", VAM_MAX_LAYER_LEVELS, n_levels);
  CountArgs a;
  a.layer = layer; a.perm = perm; a.count = count_out;
  a.ld_layer = ld_layer; a.n_slice = n_slice; a.n_pix = n_pix; a.C = C; a.n = (int)n; a.n_levels = n_levels;
  a.n_seg = n_batch * n_slice;
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 0);
  hipLaunchKernelGGL(rank_counts_kernel, dim3(cdiv((long)a.n_seg * n_levels, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("rank_counts_kernel");
}

int vam_rank_scatter(const int32_t* ranked, const int32_t* perm, const int32_t* count, int n_levels, int n_batch, int n_slice,
                     int n_pix, int C, int32_t* sym_out, int ld_sym, uint8_t* id_out, int ld_id, void* stream) {
  long n;
  if (int rc = rank_shape("vam_rank_scatter", n_batch, n_slice, n_pix, C, &n)) return rc;
  VAM_REQUIRE(ranked && perm && count && sym_out && id_out, "vam_rank_scatter: need ranked, perm, count, sym_out and id_out");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_MASK_LEVELS, "vam_rank_scatter: 1..%d levels, got %d", VAM_MAX_MASK_LEVELS, n_levels);
  VAM_REQUIRE(ld_sym >= n_slice * C && ld_id >= n_slice * C, "vam_rank_scatter: pixel strides must be >= n_slice * C");
  ScatterArgs a;
  a.ranked = ranked; a.perm = perm; a.count = count; a.sym = sym_out; a.id = id_out;
  a.ld_sym = ld_sym; a.ld_id = ld_id; a.n_slice = n_slice; a.n_pix = n_pix; a.C = C; a.n = (int)n;
  a.n_levels = n_levels; a.n_seg = n_batch * n_slice;
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, (double)a.n_seg * n * 13.0);
  hipLaunchKernelGGL(rank_scatter_kernel, dim3(cdiv(n, 256), a.n_seg), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("rank_scatter_kernel");
}

}  // extern "C"
