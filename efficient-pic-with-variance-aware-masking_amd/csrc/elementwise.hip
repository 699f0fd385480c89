// HBM-bound element-wise kernels of the hot path: model-edge layout changes, the fused
// Gaussian-conditional slice tail, build_indexes, the factorised-prior likelihood for z,
// and two tiny helpers.  All are coalesced 16-byte-per-lane streams over NHWC channel
// windows (pixel stride `ld`), grid-stride with <= 2048 blocks.
//
// This file is compiled with -ffp-contract=off: the reference evaluates these chains as
// separate fp32 ops (entropy_models.py:140-149,620-652) and a contracted fma would change
// bits.
#include "common.h"

namespace vam {

__device__ __forceinline__ float phi_c(float t) {
  // entropy_models.py:573-576: 0.5 * erfc(-(2**-0.5) * t)
  return 0.5f * erfcf(-0.70710678118654752440f * t);
}

__device__ __forceinline__ float gauss_lik(float absv, float sigma) {
  float s = fmaxf(sigma, 0.11f);                 // LowerBound(0.11), entropy_models.py:628
  float upper = phi_c((0.5f - absv) / s);
  float lower = phi_c((-0.5f - absv) / s);
  return fmaxf(upper - lower, 1e-9f);            // likelihood_lower_bound, :650
}

// wave-aggregated atomic accumulation of a per-lane double into acc[item].  Called from inside grid-stride loops: the
// lanes that have left the loop (a launch's last wave, or the last pass) are inactive here.  `__all` votes over the
// active lanes only; what a shuffle delivers from an inactive lane is not relied upon — a term enters the sum only if
// its source lane is in `live`.  The active lanes of a grid-stride pass are a prefix of the wave (the index grows with
// the lane), so lane 0 is active whenever any lane is and holds the wave's sum after the last step.
__device__ __forceinline__ void wave_accumulate(double v, int item, double* acc) {
  int first = __builtin_amdgcn_readfirstlane(item);
  if (__all(item == first)) {
    const unsigned long long live = __ballot(1);
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_down(v, o, 64);
      if (lane + o < 64 && ((live >> (lane + o)) & 1ull)) v += t;
    }
    if (lane == 0) atomicAdd(acc + first, v);
  } else {
    atomicAdd(acc + item, v);
  }
}

// ------------------------------------------------------------------ layout
__global__ void s2d_input_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W) {
  // out[b, Y, X, (py*2+px)*3 + c] = x[b, c, 2Y+py, 2X+px]; channels 12..15 = 0
  const int H2 = H / 2, W2 = W / 2;
  long total = (long)B * H2 * W2 * 4;  // one float4 (= 4 channels) per thread
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int q = (int)(i & 3);
    long pix = i >> 2;
    int X = (int)(pix % W2);
    long r = pix / W2;
    int Y = (int)(r % H2);
    int b = (int)(r / H2);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int ch = q * 4 + k;
      float val = 0.f;
      if (ch < 12) {
        int ph = ch / 3, c = ch - ph * 3;
        int py = ph >> 1, px = ph & 1;
        val = x[(((long)b * 3 + c) * H + 2 * Y + py) * W + 2 * X + px];
      }
      v[k] = val;
    }
    *reinterpret_cast<float4*>(out + pix * 16 + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int C, int HW,
                                    int ld) {
  // tile transpose through LDS: 32 pixels x 32 channels
  __shared__ float tile[32][33];
  int b = blockIdx.z;
  int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty 0..7
  for (int k = ty; k < 32; k += 8) {
    int c = c0 + k, p = p0 + tx;
    tile[k][tx] = (c < C && p < HW) ? src[((long)b * C + c) * HW + p] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    int p = p0 + k, c = c0 + tx;
    if (p < HW && c < C) dst[((long)b * HW + p) * ld + c] = tile[tx][k];
  }
}

__global__ void nhwc_to_nchw_kernel(const float* __restrict__ src, int ld, float* __restrict__ dst, int B, int C,
                                    int HW) {
  __shared__ float tile[32][33];
  int b = blockIdx.z;
  int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    int p = p0 + k, c = c0 + tx;
    tile[k][tx] = (c < C && p < HW) ? src[((long)b * HW + p) * ld + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    int c = c0 + k, p = p0 + tx;
    if (p < HW && c < C) dst[((long)b * C + c) * HW + p] = tile[tx][k];
  }
}

// ------------------------------------------------------------------ Gaussian slice tail
// pic.py:625-629, one element under mask value m: the likelihood is taken at round((r-mu)*m) with scale sigma*m, and
// yhat = round(r-mu)*m + mu (q = round(r-mu)).  Shared by gauss_tail_kernel and gauss_levels_eval_kernel.
__device__ __forceinline__ void masked_tail(float d, float q, float mu, float sg, float m, float& yh, float& absv, float& s,
                                            int& sym) {
  float in = d * m;
  float rq = rintf(in);
  absv = fabsf(rq);
  s = sg * m;
  yh = q * m + mu;
  sym = (int)rq;
}

struct TailArgs {
  const float *y, *y2, *mu, *sigma, *mask;
  float *yhat, *lik;
  int32_t* sym;
  double* log2sum;
  int ld_y, ld_y2, ld_mu, ld_sigma, ld_mask, ld_yhat, ld_lik, ld_sym;
  int pix_per_item, C4;  // C4 = C/4
  long n_vec;            // n_pix * C4
};

__global__ void gauss_tail_kernel(const TailArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p = i / a.C4;
    int c = (int)(i - p * a.C4) * 4;
    float4 y = *reinterpret_cast<const float4*>(a.y + p * a.ld_y + c);
    if (a.y2) {
      float4 y2 = *reinterpret_cast<const float4*>(a.y2 + p * a.ld_y2 + c);
      y.x -= y2.x; y.y -= y2.y; y.z -= y2.z; y.w -= y2.w;            // pic.py:583-584
    }
    float4 mu = *reinterpret_cast<const float4*>(a.mu + p * a.ld_mu + c);
    float4 sg = *reinterpret_cast<const float4*>(a.sigma + p * a.ld_sigma + c);
    float yv[4] = {y.x, y.y, y.z, y.w}, mv[4] = {mu.x, mu.y, mu.z, mu.w}, sv[4] = {sg.x, sg.y, sg.z, sg.w};
    float mk[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.mask) {
      float4 m = *reinterpret_cast<const float4*>(a.mask + p * a.ld_mask + c);
      mk[0] = m.x; mk[1] = m.y; mk[2] = m.z; mk[3] = m.w;
    }
    float yh[4], lk[4];
    int sy[4];
    double lsum = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float d = yv[k] - mv[k];
      float q = rintf(d);                         // torch.round = half-to-even
      float absv, s;
      if (a.mask) {
        masked_tail(d, q, mv[k], sv[k], mk[k], yh[k], absv, s, sy[k]);
      } else {
        // pic.py:545-546 + entropy_models.py:140-149,623-630: |(round(y-mu)+mu) - mu|
        float o = q + mv[k];
        absv = fabsf(o - mv[k]);
        s = sv[k];
        yh[k] = o;
        sy[k] = (int)q;
      }
      lk[k] = gauss_lik(absv, s);
      lsum += log2((double)lk[k]);
    }
    if (a.yhat) *reinterpret_cast<float4*>(a.yhat + p * a.ld_yhat + c) = make_float4(yh[0], yh[1], yh[2], yh[3]);
    if (a.lik) *reinterpret_cast<float4*>(a.lik + p * a.ld_lik + c) = make_float4(lk[0], lk[1], lk[2], lk[3]);
    if (a.sym) *reinterpret_cast<int4*>(a.sym + p * a.ld_sym + c) = make_int4(sy[0], sy[1], sy[2], sy[3]);
    if (a.log2sum) wave_accumulate(lsum, (int)(p / a.pix_per_item), a.log2sum);
  }
}

// The progressive tail of n_levels masks over one shared (y, y2, mu, sigma) window (vam_gauss_levels_eval): the shared
// operands are loaded once per element, level l's mask once; per level the element math of gauss_tail_kernel's masked
// branch, and level l's per-image log2 sum goes to log2sum[l * n_items + item].  Level l's arrays sit at base + l * ls.
struct TailLevelsArgs {
  const float *y, *y2, *mu, *sigma, *mask;
  float *yhat, *lik;
  int32_t* sym;
  double* log2sum;
  int ld_y, ld_y2, ld_mu, ld_sigma, ld_mask, ld_yhat, ld_lik, ld_sym;
  long ls_mask, ls_yhat, ls_lik, ls_sym;
  int pix_per_item, n_items, n_levels, C4;
  long n_vec;
};

__global__ void gauss_levels_eval_kernel(const TailLevelsArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p = i / a.C4;
    int c = (int)(i - p * a.C4) * 4;
    float4 y = *reinterpret_cast<const float4*>(a.y + p * a.ld_y + c);
    if (a.y2) {
      float4 y2 = *reinterpret_cast<const float4*>(a.y2 + p * a.ld_y2 + c);
      y.x -= y2.x; y.y -= y2.y; y.z -= y2.z; y.w -= y2.w;            // pic.py:583-584
    }
    float4 mu = *reinterpret_cast<const float4*>(a.mu + p * a.ld_mu + c);
    float4 sg = *reinterpret_cast<const float4*>(a.sigma + p * a.ld_sigma + c);
    float yv[4] = {y.x, y.y, y.z, y.w}, mv[4] = {mu.x, mu.y, mu.z, mu.w}, sv[4] = {sg.x, sg.y, sg.z, sg.w};
    float dv[4], qv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dv[k] = yv[k] - mv[k];
      qv[k] = rintf(dv[k]);                       // torch.round = half-to-even
    }
    const int item = (int)(p / a.pix_per_item);
    for (int lv = 0; lv < a.n_levels; ++lv) {
      float4 m = *reinterpret_cast<const float4*>(a.mask + lv * a.ls_mask + p * a.ld_mask + c);
      float mk[4] = {m.x, m.y, m.z, m.w};
      float yh[4], lk[4];
      int sy[4];
      double lsum = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float absv, s;
        masked_tail(dv[k], qv[k], mv[k], sv[k], mk[k], yh[k], absv, s, sy[k]);
        lk[k] = gauss_lik(absv, s);
        lsum += log2((double)lk[k]);
      }
      if (a.yhat) *reinterpret_cast<float4*>(a.yhat + lv * a.ls_yhat + p * a.ld_yhat + c) = make_float4(yh[0], yh[1], yh[2], yh[3]);
      if (a.lik) *reinterpret_cast<float4*>(a.lik + lv * a.ls_lik + p * a.ld_lik + c) = make_float4(lk[0], lk[1], lk[2], lk[3]);
      if (a.sym) *reinterpret_cast<int4*>(a.sym + lv * a.ls_sym + p * a.ld_sym + c) = make_int4(sy[0], sy[1], sy[2], sy[3]);
      if (a.log2sum) wave_accumulate(lsum, lv * a.n_items + item, a.log2sum);
    }
  }
}

// The decoder's side of the levels tail (vam_gauss_levels_decode): q = float(sym) is the decoded round(r - mu) and level l's
// mask is (layer <= k_l); yhat_l through masked_tail's expression q * m + mu, so it equals gauss_levels_eval_kernel's.
struct DecodeLevelsArgs {
  const int32_t* sym;
  const uint8_t* layer;
  const float* mu;
  float* yhat;
  int ld_sym, ld_layer, ld_mu, ld_yhat;
  long ls_yhat;
  int ks[VAM_MAX_MASK_LEVELS];
  int n_levels, C4;
  long n_vec;
};

__global__ void gauss_levels_decode_kernel(const DecodeLevelsArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p = i / a.C4;
    int c = (int)(i - p * a.C4) * 4;
    int4 sy = *reinterpret_cast<const int4*>(a.sym + p * a.ld_sym + c);
    unsigned ly = *reinterpret_cast<const unsigned*>(a.layer + p * a.ld_layer + c);
    float4 mu = *reinterpret_cast<const float4*>(a.mu + p * a.ld_mu + c);
    float qv[4] = {(float)sy.x, (float)sy.y, (float)sy.z, (float)sy.w}, mv[4] = {mu.x, mu.y, mu.z, mu.w};
    int lv4[4] = {(int)(ly & 255u), (int)((ly >> 8) & 255u), (int)((ly >> 16) & 255u), (int)(ly >> 24)};
    for (int lv = 0; lv < a.n_levels; ++lv) {
      const int k = a.ks[lv];
      float yh[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m = lv4[e] <= k ? 1.f : 0.f;
        yh[e] = qv[e] * m + mv[e];
      }
      *reinterpret_cast<float4*>(a.yhat + lv * a.ls_yhat + p * a.ld_yhat + c) = make_float4(yh[0], yh[1], yh[2], yh[3]);
    }
  }
}

// The rate-only tail (vam_gauss_layer_bits): the in-mask likelihood of every element — masked_tail /
// gauss_lik with m = 1, the float gauss_levels_eval_kernel gets for an element inside a mask — binned by the element's
// container layer.  A workgroup's pixels belong to one item; its four waves keep one row of n_levels + 1 fp64 bins (and
// counts) each in LDS, filled with LDS atomics, and the workgroup flushes one global fp64 atomic per non-empty bin.
struct LayerBitsArgs {
  const float *y, *y2, *mu, *sigma;
  const uint8_t* layer;
  double* bits;
  long long* count;
  int ld_y, ld_y2, ld_mu, ld_sigma, ld_layer;
  int n_levels, C4, blocks_per_item;
  long vec_per_item;     // pix_per_item * C4
};

constexpr int LAYER_BINS = VAM_MAX_LAYER_LEVELS + 1;

__global__ __launch_bounds__(256) void gauss_layer_bits_kernel(const LayerBitsArgs a) {
  __shared__ double sh_bits[4][LAYER_BINS];
  __shared__ unsigned sh_cnt[4][LAYER_BINS];
  const int nb = a.n_levels + 1;                           // slot n_levels: layer == 0xFF
  const int item = blockIdx.x / a.blocks_per_item, blk = blockIdx.x - item * a.blocks_per_item;
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * LAYER_BINS; i += 256) {
    (&sh_bits[0][0])[i] = 0.0;
    (&sh_cnt[0][0])[i] = 0u;
  }
  __syncthreads();
  const long v0 = (long)item * a.vec_per_item;
  for (long j = (long)blk * 256 + threadIdx.x; j < a.vec_per_item; j += (long)a.blocks_per_item * 256) {
    const long i = v0 + j;
    long p = i / a.C4;
    int c = (int)(i - p * a.C4) * 4;
    float4 y = *reinterpret_cast<const float4*>(a.y + p * a.ld_y + c);
    if (a.y2) {
      float4 y2 = *reinterpret_cast<const float4*>(a.y2 + p * a.ld_y2 + c);
      y.x -= y2.x; y.y -= y2.y; y.z -= y2.z; y.w -= y2.w;            // pic.py:583-584
    }
    float4 mu = *reinterpret_cast<const float4*>(a.mu + p * a.ld_mu + c);
    float4 sg = *reinterpret_cast<const float4*>(a.sigma + p * a.ld_sigma + c);
    unsigned ly = *reinterpret_cast<const unsigned*>(a.layer + p * a.ld_layer + c);
    float yv[4] = {y.x, y.y, y.z, y.w}, mv[4] = {mu.x, mu.y, mu.z, mu.w}, sv[4] = {sg.x, sg.y, sg.z, sg.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float d = yv[k] - mv[k];
      float q = rintf(d);                         // torch.round = half-to-even
      float yh, absv, s;
      int sy;
      masked_tail(d, q, mv[k], sv[k], 1.f, yh, absv, s, sy);
      const float lk = gauss_lik(absv, s);
      const int l = (int)((ly >> (8 * k)) & 255u);
      const int bin = l < a.n_levels ? l : a.n_levels;     // 0xFF (and any id beyond the list) -> the last slot
      __hip_atomic_fetch_add(&sh_bits[wave][bin], log2((double)lk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&sh_cnt[wave][bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < nb) {
    const unsigned n = sh_cnt[0][t] + sh_cnt[1][t] + sh_cnt[2][t] + sh_cnt[3][t];
    if (n) {
      const double v = (sh_bits[0][t] + sh_bits[1][t]) + (sh_bits[2][t] + sh_bits[3][t]);
      atomicAdd(a.bits + (long)item * nb + t, v);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.count) + (long)item * nb + t, (unsigned long long)n);
    }
  }
}

// ------------------------------------------------------------------ build_indexes
// entropy_models.py:654-659 for one scale: n_table - 1 - #{t < n_table - 1: max(s, .11) <= T_t}.  Shared by
// build_indexes_kernel and the pricing kernel (coded_bits_kernel), which must name the same table.
__device__ __forceinline__ int scale_index(float s, const float* tbl, int n_table) {
  float v = fmaxf(s, 0.11f);
  int cnt = 0;
  for (int t = 0; t < n_table - 1; ++t) cnt += (v <= tbl[t]) ? 1 : 0;   // entropy_models.py:657-658
  return n_table - 1 - cnt;
}

__global__ void build_indexes_kernel(const float* __restrict__ sigma, int ld_sigma, const float* __restrict__ mask,
                                     int ld_mask, const float* __restrict__ table, int n_table,
                                     int32_t* __restrict__ idx, int ld_idx, long n_vec, int C4) {
  __shared__ float tbl[256];
  for (int i = threadIdx.x; i < n_table; i += blockDim.x) tbl[i] = table[i];
  __syncthreads();
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p = i / C4;
    int c = (int)(i - p * C4) * 4;
    float4 sg = *reinterpret_cast<const float4*>(sigma + p * ld_sigma + c);
    float s[4] = {sg.x, sg.y, sg.z, sg.w};
    if (mask) {
      float4 m = *reinterpret_cast<const float4*>(mask + p * ld_mask + c);
      s[0] *= m.x; s[1] *= m.y; s[2] *= m.z; s[3] *= m.w;
    }
    int r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = scale_index(s[k], tbl, n_table);
    *reinterpret_cast<int4*>(idx + p * ld_idx + c) = make_int4(r[0], r[1], r[2], r[3]);
  }
}

// ------------------------------------------------------------------ coded-size pricing
// What encode_one (csrc/rans.cpp) charges for `symbol` under table t: 16 - log2(freq) of the entry it codes, and for a
// value outside the table the escape entry plus one count nibble and n_bypass <= 8 raw nibbles (enc_put_bits).
struct CoderTables {
  const double* cost;
  const int32_t *sizes, *offsets;
  int n_cdfs, stride;
};

__device__ __forceinline__ double symbol_cost(int symbol, int t, const CoderTables& T) {
  if (t < 0 || t >= T.n_cdfs) return __longlong_as_double(0x7FF8000000000000LL);
  int max_value = T.sizes[t] - 2;
  max_value = max_value < 0 ? 0 : (max_value >= T.stride ? T.stride - 1 : max_value);   // the host builder rejects such tables
  long long value = (long long)symbol - (long long)T.offsets[t];
  const double* row = T.cost + (long)t * T.stride;
  if (value >= 0 && value < max_value) return row[value];
  const unsigned raw = value < 0 ? (unsigned)(-2 * value - 1) : (unsigned)(2 * (value - max_value));
  int n_bypass = 0;
  while (n_bypass < 8 && (raw >> (n_bypass * 4)) != 0u) ++n_bypass;
  return row[max_value] + 4.0 * (double)(1 + n_bypass);
}

struct CodedBitsArgs {
  const float *y, *y2, *mu, *sigma, *scale_table;
  const int32_t *sym, *idx;
  const uint8_t* layer;
  double* bits;
  long long* count;
  CoderTables T;
  int ld_y, ld_y2, ld_mu, ld_sigma, ld_sym, ld_idx, ld_layer, idx_base, n_table;
  int n_levels, S4, n_slices, blocks_per_stream, pix_per_item;
  long vec_per_stream;   // pix_per_item * S4
};

// One workgroup stays inside one stream (item, slice of 4 * S4 channels); bins as in gauss_layer_bits_kernel: a row of
// n_levels + 1 fp64 sums and counts per wave in LDS, one global atomic per non-empty bin.  SYMS: the (symbol, index) pair
// is read; else it is derived from (y, y2, mu, sigma) with masked_tail (m = 1) and scale_index.
template <bool SYMS>
__global__ __launch_bounds__(256) void coded_bits_kernel(const CodedBitsArgs a) {
  __shared__ double sh_bits[4][LAYER_BINS];
  __shared__ unsigned sh_cnt[4][LAYER_BINS];
  __shared__ float tbl[256];
  const int nb = a.n_levels + 1;                           // slot n_levels: layer == 0xFF
  const int stream = blockIdx.x / a.blocks_per_stream, blk = blockIdx.x - stream * a.blocks_per_stream;
  const int item = stream / a.n_slices, slice = stream - item * a.n_slices;
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * LAYER_BINS; i += 256) {
    (&sh_bits[0][0])[i] = 0.0;
    (&sh_cnt[0][0])[i] = 0u;
  }
  if (!SYMS)
    for (int i = threadIdx.x; i < a.n_table; i += 256) tbl[i] = a.scale_table[i];
  __syncthreads();
  const long p0 = (long)item * a.pix_per_item;
  const int c0 = slice * a.S4 * 4;
  for (long j = (long)blk * 256 + threadIdx.x; j < a.vec_per_stream; j += (long)a.blocks_per_stream * 256) {
    const long pp = j / a.S4;
    const long p = p0 + pp;
    const int c = c0 + (int)(j - pp * a.S4) * 4;
    int sy[4], ix[4];
    if (SYMS) {
      const int4 s4 = *reinterpret_cast<const int4*>(a.sym + p * a.ld_sym + c);
      sy[0] = s4.x; sy[1] = s4.y; sy[2] = s4.z; sy[3] = s4.w;
      if (a.idx) {
        const int4 i4 = *reinterpret_cast<const int4*>(a.idx + p * a.ld_idx + c);
        ix[0] = i4.x; ix[1] = i4.y; ix[2] = i4.z; ix[3] = i4.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) ix[k] = a.idx_base + c + k;
      }
    } else {
      float4 y = *reinterpret_cast<const float4*>(a.y + p * a.ld_y + c);
      if (a.y2) {
        float4 y2 = *reinterpret_cast<const float4*>(a.y2 + p * a.ld_y2 + c);
        y.x -= y2.x; y.y -= y2.y; y.z -= y2.z; y.w -= y2.w;            // pic.py:583-584
      }
      float4 mu = *reinterpret_cast<const float4*>(a.mu + p * a.ld_mu + c);
      float4 sg = *reinterpret_cast<const float4*>(a.sigma + p * a.ld_sigma + c);
      float yv[4] = {y.x, y.y, y.z, y.w}, mv[4] = {mu.x, mu.y, mu.z, mu.w}, sv[4] = {sg.x, sg.y, sg.z, sg.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float d = yv[k] - mv[k];
        float q = rintf(d);                         // torch.round = half-to-even
        float yh, absv, s;
        masked_tail(d, q, mv[k], sv[k], 1.f, yh, absv, s, sy[k]);
        ix[k] = scale_index(s, tbl, a.n_table);
      }
    }
    const unsigned ly = a.layer ? *reinterpret_cast<const unsigned*>(a.layer + p * a.ld_layer + c) : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int l = (int)((ly >> (8 * k)) & 255u);
      const int bin = l < a.n_levels ? l : a.n_levels;     // 0xFF (and any id beyond the list) -> the last slot
      __hip_atomic_fetch_add(&sh_bits[wave][bin], symbol_cost(sy[k], ix[k], a.T), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&sh_cnt[wave][bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < nb) {
    const unsigned n = sh_cnt[0][t] + sh_cnt[1][t] + sh_cnt[2][t] + sh_cnt[3][t];
    if (n) {
      const double v = (sh_bits[0][t] + sh_bits[1][t]) + (sh_bits[2][t] + sh_bits[3][t]);
      atomicAdd(a.bits + (long)stream * nb + t, v);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.count) + (long)stream * nb + t, (unsigned long long)n);
    }
  }
}

// ------------------------------------------------------------------ factorised prior (z)
__device__ __forceinline__ float softplusf(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// params per tensor, channel-major as in the state_dict:
//  m0[C*3] b0[C*3] f0[C*3] | m1[C*9] b1[C*3] f1[C*3] | m2.. | m3.. | m4[C*3] b4[C] | quantiles[C*3]
__device__ __forceinline__ float eb_logits(const float* sp /*61 preprocessed floats*/, float x) {
  float l[3], t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = sp[k] * x + sp[3 + k];
    l[k] = v + sp[6 + k] * tanhf(v);
  }
  const float* q = sp + 9;
#pragma unroll
  for (int layer = 0; layer < 3; ++layer) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = q[k * 3 + 0] * l[0];
      v = v + q[k * 3 + 1] * l[1];
      v = v + q[k * 3 + 2] * l[2];
      v = v + q[9 + k];
      t[k] = v + q[12 + k] * tanhf(v);
    }
    l[0] = t[0]; l[1] = t[1]; l[2] = t[2];
    q += 15;
  }
  float v = q[0] * l[0];
  v = v + q[1] * l[1];
  v = v + q[2] * l[2];
  return v + q[3];
}

// EntropyBottleneck.loss (entropy_models.py:398-401): sum_c,k |logits_cumulative(quantiles[c,k]) - target[k]| with the
// network's own parameters held constant (stop_gradient), and its gradient w.r.t. the quantiles.  One thread per
// (channel, quantile): the scalar 1-3-3-3-3-1 network is evaluated together with its derivative d logits / d x.
__global__ void eb_aux_loss_kernel(const float* __restrict__ params, int C, float t0, float t1, float t2,
                                   double* __restrict__ loss, float* __restrict__ dq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * C) return;
  const int c = i / 3, k3 = i - 3 * c;
  const float* m0 = params;
  const float* b0 = m0 + C * 3;
  const float* f0 = b0 + C * 3;
  const float* base = f0 + C * 3;
  const float* p = base;                                 // skip the three middle layers to reach the quantiles
  for (int layer = 0; layer < 3; ++layer) p += C * 9 + C * 3 + C * 3;
  const float* m4 = p;
  const float* b4 = m4 + C * 3;
  const float* qn = b4 + C;
  const float x = qn[c * 3 + k3];
  float l[3], dl[3];
  for (int k = 0; k < 3; ++k) {
    const float a = softplusf(m0[c * 3 + k]);
    const float v = a * x + b0[c * 3 + k];
    const float f = tanhf(f0[c * 3 + k]), th = tanhf(v);
    l[k] = v + f * th;
    dl[k] = a * (1.0f + f * (1.0f - th * th));
  }
  for (int layer = 0; layer < 3; ++layer) {
    const float* m = base;
    const float* b = m + C * 9;
    const float* f = b + C * 3;
    float t[3], dt[3];
    for (int k = 0; k < 3; ++k) {
      float v = b[c * 3 + k], dv = 0.f;
      for (int j = 0; j < 3; ++j) {
        const float w = softplusf(m[c * 9 + k * 3 + j]);
        v += w * l[j];
        dv += w * dl[j];
      }
      const float ff = tanhf(f[c * 3 + k]), th = tanhf(v);
      t[k] = v + ff * th;
      dt[k] = dv * (1.0f + ff * (1.0f - th * th));
    }
    for (int k = 0; k < 3; ++k) { l[k] = t[k]; dl[k] = dt[k]; }
    base = f + C * 3;
  }
  float v = b4[c], dv = 0.f;
  for (int j = 0; j < 3; ++j) {
    const float w = softplusf(m4[c * 3 + j]);
    v += w * l[j];
    dv += w * dl[j];
  }
  const float tgt = k3 == 0 ? t0 : (k3 == 1 ? t1 : t2);
  const float d = v - tgt;
  atomicAdd(loss, (double)fabsf(d));
  dq[i] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * dv;
}

__global__ void eb_forward_kernel(const float* __restrict__ z, int ld_z, const float* __restrict__ params, int C,
                                  float* __restrict__ zhat, int ld_zhat, float* __restrict__ lik, int ld_lik,
                                  int32_t* __restrict__ sym, int ld_sym, double* log2sum, int pix_per_item, long n_pix,
                                  const float* __restrict__ noise, int ld_noise) {
  // one thread per channel (blockDim.x >= C), pixels strided over blockIdx / y
  extern __shared__ float sh[];  // C * 62 floats of preprocessed params
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float* sp = sh + c * 62;
    const float* m0 = params;
    const float* b0 = m0 + C * 3;
    const float* f0 = b0 + C * 3;
    for (int k = 0; k < 3; ++k) {
      sp[k] = softplusf(m0[c * 3 + k]);
      sp[3 + k] = b0[c * 3 + k];
      sp[6 + k] = tanhf(f0[c * 3 + k]);
    }
    const float* base = f0 + C * 3;
    for (int layer = 0; layer < 3; ++layer) {
      const float* m = base;
      const float* b = m + C * 9;
      const float* f = b + C * 3;
      float* o = sp + 9 + layer * 15;
      for (int k = 0; k < 9; ++k) o[k] = softplusf(m[c * 9 + k]);
      for (int k = 0; k < 3; ++k) { o[9 + k] = b[c * 3 + k]; o[12 + k] = tanhf(f[c * 3 + k]); }
      base = f + C * 3;
    }
    const float* m4 = base;
    const float* b4 = m4 + C * 3;
    const float* qn = b4 + C;
    float* o = sp + 54;
    for (int k = 0; k < 3; ++k) o[k] = softplusf(m4[c * 3 + k]);
    o[3] = b4[c];
    sp[58] = qn[c * 3 + 1];  // median (entropy_models.py:354-356)
  }
  __syncthreads();
  int c = threadIdx.x;
  if (c >= C) return;
  const float* sp = sh + c * 62;
  const float med = sp[58];
  for (long p = blockIdx.x; p < n_pix; p += gridDim.x) {
    float v = z[p * ld_z + c];
    const float qz = rintf(v - med);
    float o = qz + med;                           // quantize "dequantize" with medians
    if (sym) sym[p * ld_sym + c] = (int)qz;       // quantize "symbols" (entropy_models.py:151-153)
    // training: the likelihood is evaluated at z + U(-.5,.5) (quantize "noise", entropy_models.py:132-138,471-473)
    const float at = noise ? v + noise[p * ld_noise + c] : o;
    float lower = eb_logits(sp, at - 0.5f);
    float upper = eb_logits(sp, at + 0.5f);
    float sum = lower + upper;
    float sign = sum > 0.f ? -1.f : (sum < 0.f ? 1.f : 0.f);   // -sign(lower+upper)
    float su = 1.0f / (1.0f + expf(-(sign * upper)));
    float sl = 1.0f / (1.0f + expf(-(sign * lower)));
    float lk = fmaxf(fabsf(su - sl), 1e-9f);
    if (zhat) zhat[p * ld_zhat + c] = o;
    if (lik) lik[p * ld_lik + c] = lk;
    if (log2sum) atomicAdd(log2sum + (int)(p / pix_per_item), log2((double)lk));
  }
}

__global__ void add_kernel(const float* __restrict__ a, int ld_a, const float* __restrict__ b, int ld_b,
                           float* __restrict__ out, int ld_out, long n_vec, int C4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p = i / C4;
    int c = (int)(i - p * C4) * 4;
    float4 x = *reinterpret_cast<const float4*>(a + p * ld_a + c);
    float4 y = *reinterpret_cast<const float4*>(b + p * ld_b + c);
    *reinterpret_cast<float4*>(out + p * ld_out + c) = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
  }
}

__global__ void dequantize_kernel(const int32_t* __restrict__ sym, int ld_sym, const float* __restrict__ mu, int ld_mu,
                                  float* __restrict__ out, int ld_out, long n_vec, int C4) {
  // EntropyModel.dequantize (entropy_models.py:161-168): float(symbols) + means
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p = i / C4;
    int c = (int)(i - p * C4) * 4;
    int4 q = *reinterpret_cast<const int4*>(sym + p * ld_sym + c);
    float4 m = mu ? *reinterpret_cast<const float4*>(mu + p * ld_mu + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(out + p * ld_out + c) = make_float4((float)q.x + m.x, (float)q.y + m.y, (float)q.z + m.z, (float)q.w + m.w);
  }
}

__global__ void sqdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, double* acc) {
  double s = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float d = a[i] - b[i];
    s += (double)d * (double)d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(acc, s);
}

static inline unsigned stream_grid(long n_items, int block) {
  long g = (n_items + block - 1) / block;
  return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

__global__ void zero_words_kernel(unsigned* __restrict__ p, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = 0u;
}

}  // namespace vam

using namespace vam;

extern "C" {

int vam_s2d_input(const float* x, float* out, int B, int H, int W, void* stream) {
  VAM_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "vam_s2d_input: need even H,W");
  long total = (long)B * (H / 2) * (W / 2) * 4;
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 4.0 * ((double)B * 3 * H * W + (double)total * 4));
  hipLaunchKernelGGL(s2d_input_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, B, H, W);
  return check_launch("s2d_input_kernel");
}

int vam_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int ld_dst, void* stream) {
  VAM_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && ld_dst >= C, "vam_nchw_to_nhwc: bad arguments");
  VAM_REQUIRE(B <= 65535 && cdiv(C, 32) <= 65535, "vam_nchw_to_nhwc: grid too large");
  dim3 grid(cdiv((long)H * W, 32), cdiv(C, 32), B);
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 8.0 * (double)B * C * H * W);
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, dst, B, C, H * W, ld_dst);
  return check_launch("nchw_to_nhwc_kernel");
}

int vam_nhwc_to_nchw(const float* src, int ld_src, float* dst, int B, int C, int H, int W, void* stream) {
  VAM_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && ld_src >= C, "vam_nhwc_to_nchw: bad arguments");
  VAM_REQUIRE(B <= 65535 && cdiv(C, 32) <= 65535, "vam_nhwc_to_nchw: grid too large");
  dim3 grid(cdiv((long)H * W, 32), cdiv(C, 32), B);
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 8.0 * (double)B * C * H * W);
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, ld_src, dst, B, C, H * W);
  return check_launch("nhwc_to_nchw_kernel");
}

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int vam_gauss_tail(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                   const float* sigma, int ld_sigma, const float* mask, int ld_mask, float* yhat, int ld_yhat,
                   float* lik, int ld_lik, int32_t* sym, int ld_sym, double* log2sum, int pix_per_item, long n_pix,
                   int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_tail: need y, mu, sigma and C %% 4 == 0");
  VAM_REQUIRE(!log2sum || pix_per_item > 0, "vam_gauss_tail: pix_per_item");
  VAM_REQUIRE(al16(y) && al16(mu) && al16(sigma) && al16(y2) && al16(mask) && al16(yhat) && al16(lik) && al16(sym), "vam_gauss_tail: 16-byte alignment");
  VAM_REQUIRE(ld_y % 4 == 0 && ld_mu % 4 == 0 && ld_sigma % 4 == 0 && (!y2 || ld_y2 % 4 == 0) && (!mask || ld_mask % 4 == 0) && (!yhat || ld_yhat % 4 == 0) && (!lik || ld_lik % 4 == 0) && (!sym || ld_sym % 4 == 0), "vam_gauss_tail: strides must be multiples of 4");
  TailArgs a;
  a.y = y; a.y2 = y2; a.mu = mu; a.sigma = sigma; a.mask = mask; a.yhat = yhat; a.lik = lik; a.sym = sym;
  a.log2sum = log2sum;
  a.ld_y = ld_y; a.ld_y2 = ld_y2; a.ld_mu = ld_mu; a.ld_sigma = ld_sigma; a.ld_mask = ld_mask;
  a.ld_yhat = ld_yhat; a.ld_lik = ld_lik; a.ld_sym = ld_sym;
  a.pix_per_item = pix_per_item; a.C4 = C / 4; a.n_vec = n_pix * (C / 4);
  int nin = 3 + (y2 ? 1 : 0) + (mask ? 1 : 0), nout = (yhat ? 1 : 0) + (lik ? 1 : 0) + (sym ? 1 : 0);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 4.0 * (double)n_pix * C * (nin + nout));
  hipLaunchKernelGGL(gauss_tail_kernel, dim3(stream_grid(a.n_vec, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_tail_kernel");
}

int vam_gauss_levels_eval(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                          const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls, float* yhat,
                          int ld_yhat, long yhat_ls, float* lik, int ld_lik, long lik_ls, int32_t* sym, int ld_sym,
                          long sym_ls, double* log2sum, int pix_per_item, int n_levels, long n_pix, int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && mask && n_levels > 0 && n_pix > 0 && C > 0 && C % 4 == 0,
              "vam_gauss_levels_eval: need y, mu, sigma, mask, n_levels > 0 and C %% 4 == 0");
  VAM_REQUIRE(!log2sum || (pix_per_item > 0 && n_pix % pix_per_item == 0), "vam_gauss_levels_eval: pix_per_item");
  VAM_REQUIRE(n_pix / (pix_per_item > 0 ? pix_per_item : 1) * (long)n_levels < (1L << 31), "vam_gauss_levels_eval: too many items");
  VAM_REQUIRE(al16(y) && al16(mu) && al16(sigma) && al16(y2) && al16(mask) && al16(yhat) && al16(lik) && al16(sym), "vam_gauss_levels_eval: 16-byte alignment");
  VAM_REQUIRE(ld_y % 4 == 0 && ld_mu % 4 == 0 && ld_sigma % 4 == 0 && ld_mask % 4 == 0 && mask_ls % 4 == 0 && (!y2 || ld_y2 % 4 == 0) &&
              (!yhat || (ld_yhat % 4 == 0 && yhat_ls % 4 == 0)) && (!lik || (ld_lik % 4 == 0 && lik_ls % 4 == 0)) &&
              (!sym || (ld_sym % 4 == 0 && sym_ls % 4 == 0)), "vam_gauss_levels_eval: strides must be multiples of 4");
  TailLevelsArgs a;
  a.y = y; a.y2 = y2; a.mu = mu; a.sigma = sigma; a.mask = mask; a.yhat = yhat; a.lik = lik; a.sym = sym;
  a.log2sum = log2sum;
  a.ld_y = ld_y; a.ld_y2 = ld_y2; a.ld_mu = ld_mu; a.ld_sigma = ld_sigma; a.ld_mask = ld_mask;
  a.ld_yhat = ld_yhat; a.ld_lik = ld_lik; a.ld_sym = ld_sym;
  a.ls_mask = mask_ls; a.ls_yhat = yhat_ls; a.ls_lik = lik_ls; a.ls_sym = sym_ls;
  a.pix_per_item = pix_per_item > 0 ? pix_per_item : 1;
  a.n_items = (int)(n_pix / a.pix_per_item);
  a.n_levels = n_levels; a.C4 = C / 4; a.n_vec = n_pix * (C / 4);
  int nin = 3 + (y2 ? 1 : 0) + n_levels, nout = n_levels * ((yhat ? 1 : 0) + (lik ? 1 : 0) + (sym ? 1 : 0));
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 4.0 * (double)n_pix * C * (nin + nout));
  hipLaunchKernelGGL(gauss_levels_eval_kernel, dim3(stream_grid(a.n_vec, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_levels_eval_kernel");
}

int vam_gauss_levels_decode(const int32_t* sym, int ld_sym, const uint8_t* layer, int ld_layer, const float* mu, int ld_mu,
                            const int* ks, int n_levels, float* yhat, int ld_yhat, long yhat_ls, long n_pix, int C,
                            void* stream) {
  VAM_REQUIRE(sym && layer && mu && ks && yhat && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_levels_decode: bad arguments");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_MASK_LEVELS, "vam_gauss_levels_decode: 1..%d levels, got %d",
              VAM_MAX_MASK_LEVELS, n_levels);
  VAM_REQUIRE(al16(sym) && al16(mu) && al16(yhat) && (((uintptr_t)layer) & 3) == 0, "vam_gauss_levels_decode: alignment");
  VAM_REQUIRE(ld_sym % 4 == 0 && ld_layer % 4 == 0 && ld_mu % 4 == 0 && ld_yhat % 4 == 0 && yhat_ls % 4 == 0,
              "vam_gauss_levels_decode: strides must be multiples of 4");
  DecodeLevelsArgs a;
  a.sym = sym; a.layer = layer; a.mu = mu; a.yhat = yhat;
  a.ld_sym = ld_sym; a.ld_layer = ld_layer; a.ld_mu = ld_mu; a.ld_yhat = ld_yhat; a.ls_yhat = yhat_ls;
  for (int l = 0; l < VAM_MAX_MASK_LEVELS; ++l) a.ks[l] = l < n_levels ? ks[l] : -1;
  a.n_levels = n_levels; a.C4 = C / 4; a.n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, (double)n_pix * C * (9.0 + 4.0 * n_levels));
  hipLaunchKernelGGL(gauss_levels_decode_kernel, dim3(stream_grid(a.n_vec, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_levels_decode_kernel");
}

int vam_gauss_layer_bits(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const uint8_t* layer, int ld_layer, int n_levels,
                         double* bits, long long* count, int pix_per_item, long n_pix, int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && layer && bits && count, "vam_gauss_layer_bits: y, mu, sigma, layer, bits and count must not be NULL");
  VAM_REQUIRE(n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_layer_bits: need n_pix > 0 and C %% 4 == 0");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "vam_gauss_layer_bits: 1..%d levels, got %d",
              VAM_MAX_LAYER_LEVELS, n_levels);
  VAM_REQUIRE(pix_per_item > 0 && n_pix % pix_per_item == 0, "vam_gauss_layer_bits: pix_per_item must divide n_pix");
  VAM_REQUIRE((long)pix_per_item * C < (1L << 31) && n_pix / pix_per_item < (1L << 24), "vam_gauss_layer_bits: item too large");
  VAM_REQUIRE(al16(y) && al16(mu) && al16(sigma) && al16(y2) && (((uintptr_t)layer) & 3) == 0 && (((uintptr_t)bits) & 7) == 0 &&
              (((uintptr_t)count) & 7) == 0, "vam_gauss_layer_bits: alignment");
  VAM_REQUIRE(ld_y % 4 == 0 && ld_mu % 4 == 0 && ld_sigma % 4 == 0 && ld_layer % 4 == 0 && (!y2 || ld_y2 % 4 == 0) &&
              ld_y >= C && ld_mu >= C && ld_sigma >= C && ld_layer >= C && (!y2 || ld_y2 >= C),
              "vam_gauss_layer_bits: pixel strides must be multiples of 4 and >= C");
  LayerBitsArgs a;
  a.y = y; a.y2 = y2; a.mu = mu; a.sigma = sigma; a.layer = layer; a.bits = bits; a.count = count;
  a.ld_y = ld_y; a.ld_y2 = ld_y2; a.ld_mu = ld_mu; a.ld_sigma = ld_sigma; a.ld_layer = ld_layer;
  a.n_levels = n_levels; a.C4 = C / 4;
  a.vec_per_item = (long)pix_per_item * (C / 4);
  const long n_items = n_pix / pix_per_item;
  // a workgroup stays inside one item; about two float4 per lane, and no more than ~2048 workgroups in all
  long per_item = cdiv(a.vec_per_item, 512L);
  const long room = n_items >= 2048 ? 1 : 2048 / n_items;
  if (per_item > room) per_item = room;
  if (per_item < 1) per_item = 1;
  a.blocks_per_item = (int)per_item;
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, (double)n_pix * C * (y2 ? 17.0 : 13.0));
  hipLaunchKernelGGL(gauss_layer_bits_kernel, dim3((unsigned)(n_items * per_item)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_layer_bits_kernel");
}

int vam_build_indexes(const float* sigma, int ld_sigma, const float* mask, int ld_mask, const float* table,
                      int n_table, int32_t* idx, int ld_idx, long n_pix, int C, void* stream) {
  VAM_REQUIRE(sigma && table && idx && n_pix > 0 && C > 0 && C % 4 == 0, "vam_build_indexes: bad arguments");
  VAM_REQUIRE(n_table >= 2 && n_table <= 256, "vam_build_indexes: table size %d", n_table);
  VAM_REQUIRE(al16(sigma) && al16(mask) && al16(idx) && ld_sigma % 4 == 0 && ld_idx % 4 == 0 && (!mask || ld_mask % 4 == 0), "vam_build_indexes: alignment");
  long n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 4.0 * (double)n_pix * C * (mask ? 3 : 2));
  hipLaunchKernelGGL(build_indexes_kernel, dim3(stream_grid(n_vec, 256)), dim3(256), 0, (hipStream_t)stream, sigma,
                     ld_sigma, mask, ld_mask, table, n_table, idx, ld_idx, n_vec, C / 4);
  return check_launch("build_indexes_kernel");
}

static int coded_bits_launch(CodedBitsArgs& a, const char* who, const vam_coder_tables* tables, const uint8_t* layer,
                             int ld_layer, int n_levels, int chans_per_stream, double* bits, long long* count,
                             int pix_per_item, long n_pix, int C, bool syms, double bytes_per_elem, void* stream) {
  VAM_REQUIRE(tables && tables->cost && tables->sizes && tables->offsets && bits && count, "%s: tables, bits and count must not be NULL", who);
  VAM_REQUIRE(tables->n_cdfs >= 1 && tables->stride >= 2, "%s: %d tables of stride %d", who, tables->n_cdfs, tables->stride);
  VAM_REQUIRE(n_pix > 0 && C > 0 && C % 4 == 0, "%s: need n_pix > 0 and C %% 4 == 0", who);
  VAM_REQUIRE(chans_per_stream > 0 && chans_per_stream % 4 == 0 && C % chans_per_stream == 0,
              "%s: chans_per_stream %d must be a multiple of 4 that divides C = %d", who, chans_per_stream, C);
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "%s: 1..%d levels, got %d", who, VAM_MAX_LAYER_LEVELS, n_levels);
  VAM_REQUIRE(pix_per_item > 0 && n_pix % pix_per_item == 0, "%s: pix_per_item must divide n_pix", who);
  VAM_REQUIRE((long)pix_per_item * C < (1L << 31) && n_pix / pix_per_item * (C / chans_per_stream) < (1L << 20), "%s: item too large", who);
  VAM_REQUIRE((((uintptr_t)layer) & 3) == 0 && (((uintptr_t)bits) & 7) == 0 && (((uintptr_t)count) & 7) == 0 &&
              (((uintptr_t)tables->cost) & 7) == 0 && (!layer || (ld_layer % 4 == 0 && ld_layer >= C)), "%s: alignment / layer stride", who);
  a.layer = layer; a.ld_layer = ld_layer; a.bits = bits; a.count = count;
  a.T.cost = tables->cost; a.T.sizes = tables->sizes; a.T.offsets = tables->offsets;
  a.T.n_cdfs = tables->n_cdfs; a.T.stride = tables->stride;
  a.n_levels = n_levels; a.S4 = chans_per_stream / 4; a.n_slices = C / chans_per_stream; a.pix_per_item = pix_per_item;
  a.vec_per_stream = (long)pix_per_item * a.S4;
  const long n_streams = n_pix / pix_per_item * a.n_slices;
  // a workgroup stays inside one stream; about two vectors per lane, and no more than ~2048 workgroups in all
  long per = cdiv(a.vec_per_stream, 512L);
  const long room = n_streams >= 2048 ? 1 : 2048 / n_streams;
  if (per > room) per = room;
  if (per < 1) per = 1;
  a.blocks_per_stream = (int)per;
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, (double)n_pix * C * bytes_per_elem);
  if (syms)
    hipLaunchKernelGGL(coded_bits_kernel<true>, dim3((unsigned)(n_streams * per)), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(coded_bits_kernel<false>, dim3((unsigned)(n_streams * per)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("coded_bits_kernel");
}

int vam_coded_layer_bits(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const uint8_t* layer, int ld_layer, int n_levels,
                         const float* scale_table, int n_table, const vam_coder_tables* tables, int chans_per_stream,
                         double* bits, long long* count, int pix_per_item, long n_pix, int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && scale_table, "vam_coded_layer_bits: y, mu, sigma and scale_table must not be NULL");
  VAM_REQUIRE(n_table >= 2 && n_table <= 256 && tables && n_table <= tables->n_cdfs,
              "vam_coded_layer_bits: scale table of %d entries (2..256, at most one per coder table)", n_table);
  VAM_REQUIRE(al16(y) && al16(mu) && al16(sigma) && al16(y2), "vam_coded_layer_bits: 16-byte alignment");
  VAM_REQUIRE(ld_y % 4 == 0 && ld_mu % 4 == 0 && ld_sigma % 4 == 0 && (!y2 || ld_y2 % 4 == 0) && ld_y >= C && ld_mu >= C &&
              ld_sigma >= C && (!y2 || ld_y2 >= C), "vam_coded_layer_bits: pixel strides must be multiples of 4 and >= C");
  CodedBitsArgs a = {};
  a.y = y; a.y2 = y2; a.mu = mu; a.sigma = sigma; a.scale_table = scale_table; a.n_table = n_table;
  a.ld_y = ld_y; a.ld_y2 = ld_y2; a.ld_mu = ld_mu; a.ld_sigma = ld_sigma;
  return coded_bits_launch(a, "vam_coded_layer_bits", tables, layer, ld_layer, n_levels, chans_per_stream, bits, count,
                           pix_per_item, n_pix, C, false, (y2 ? 16.0 : 12.0) + (layer ? 1.0 : 0.0), stream);
}

int vam_coded_symbol_bits(const int32_t* sym, int ld_sym, const int32_t* idx, int ld_idx, int idx_base,
                          const uint8_t* layer, int ld_layer, int n_levels, const vam_coder_tables* tables,
                          int chans_per_stream, double* bits, long long* count, int pix_per_item, long n_pix, int C,
                          void* stream) {
  VAM_REQUIRE(sym && al16(sym) && al16(idx), "vam_coded_symbol_bits: sym must not be NULL; 16-byte alignment");
  VAM_REQUIRE(ld_sym % 4 == 0 && ld_sym >= C && (!idx || (ld_idx % 4 == 0 && ld_idx >= C)),
              "vam_coded_symbol_bits: pixel strides must be multiples of 4 and >= C");
  VAM_REQUIRE(idx || (tables && idx_base >= 0 && (long)idx_base + C <= tables->n_cdfs),
              "vam_coded_symbol_bits: without idx the channels idx_base .. idx_base + C must name tables");
  CodedBitsArgs a = {};
  a.sym = sym; a.idx = idx; a.ld_sym = ld_sym; a.ld_idx = ld_idx; a.idx_base = idx_base;
  return coded_bits_launch(a, "vam_coded_symbol_bits", tables, layer, ld_layer, n_levels, chans_per_stream, bits, count,
                           pix_per_item, n_pix, C, true, (idx ? 8.0 : 4.0) + (layer ? 1.0 : 0.0), stream);
}

int vam_eb_forward(const float* z, int ld_z, const float* params, int C, float* zhat, int ld_zhat, float* lik,
                   int ld_lik, int32_t* sym, int ld_sym, double* log2sum, int pix_per_item, long n_pix, void* stream) {
  return vam_eb_forward_noise(z, ld_z, params, C, zhat, ld_zhat, lik, ld_lik, sym, ld_sym, log2sum, pix_per_item, n_pix,
                              nullptr, 0, stream);
}

int vam_eb_forward_noise(const float* z, int ld_z, const float* params, int C, float* zhat, int ld_zhat, float* lik,
                         int ld_lik, int32_t* sym, int ld_sym, double* log2sum, int pix_per_item, long n_pix,
                         const float* noise, int ld_noise, void* stream) {
  VAM_REQUIRE(!noise || ld_noise >= C, "vam_eb_forward_noise: noise stride");
  VAM_REQUIRE(z && params && C > 0 && C <= 1024 && n_pix > 0, "vam_eb_forward: bad arguments");
  VAM_REQUIRE(!log2sum || pix_per_item > 0, "vam_eb_forward: pix_per_item");
  int block = (C + 63) / 64 * 64;
  size_t smem = (size_t)C * 62 * sizeof(float);
  VAM_REQUIRE(smem <= 64 * 1024, "vam_eb_forward: C too large for LDS staging");
  unsigned grid = (unsigned)(n_pix < 1024 ? n_pix : 1024);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 12.0 * (double)n_pix * C);
  hipLaunchKernelGGL(eb_forward_kernel, dim3(grid), dim3(block), smem, (hipStream_t)stream, z, ld_z, params, C, zhat,
                     ld_zhat, lik, ld_lik, sym, ld_sym, log2sum, pix_per_item, n_pix, noise, ld_noise);
  return check_launch("eb_forward_kernel");
}

int vam_eb_aux_loss(const float* params, int C, const float* target3_host, double* loss, float* dquantiles, void* stream) {
  VAM_REQUIRE(params && target3_host && loss && dquantiles && C > 0, "vam_eb_aux_loss: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned*>(loss), 2L);   // (a kernel, see vam_memset_zero)
  hipLaunchKernelGGL(eb_aux_loss_kernel, dim3(cdiv(3L * C, 64)), dim3(64), 0, s, params, C, target3_host[0], target3_host[1],
                     target3_host[2], loss, dquantiles);
  return check_launch("eb_aux_loss_kernel");
}

int vam_add(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, long n_pix, int C,
            void* stream) {
  VAM_REQUIRE(a && b && out && n_pix > 0 && C > 0 && C % 4 == 0 && ld_a % 4 == 0 && ld_b % 4 == 0 && ld_out % 4 == 0, "vam_add: bad arguments");
  VAM_REQUIRE(al16(a) && al16(b) && al16(out), "vam_add: alignment");
  long n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 12.0 * (double)n_pix * C);
  hipLaunchKernelGGL(add_kernel, dim3(stream_grid(n_vec, 256)), dim3(256), 0, (hipStream_t)stream, a, ld_a, b, ld_b,
                     out, ld_out, n_vec, C / 4);
  return check_launch("add_kernel");
}

int vam_dequantize(const int32_t* sym, int ld_sym, const float* mu, int ld_mu, float* out, int ld_out, long n_pix, int C,
                   void* stream) {
  VAM_REQUIRE(sym && out && n_pix > 0 && C > 0 && C % 4 == 0 && ld_sym % 4 == 0 && ld_out % 4 == 0 && (!mu || ld_mu % 4 == 0), "vam_dequantize: bad arguments");
  VAM_REQUIRE(al16(sym) && al16(mu) && al16(out), "vam_dequantize: alignment");
  long n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 12.0 * (double)n_pix * C);
  hipLaunchKernelGGL(dequantize_kernel, dim3(stream_grid(n_vec, 256)), dim3(256), 0, (hipStream_t)stream, sym, ld_sym, mu,
                     ld_mu, out, ld_out, n_vec, C / 4);
  return check_launch("dequantize_kernel");
}

int vam_memset_zero(void* ptr, size_t bytes, void* stream) {
  // Always a KERNEL, never hipMemsetAsync: every node of a captured plan is then a kernel node, ordered like every other
  // launch of the plan (round 2 saw single elements of a 392-float table left un-cleared behind a memset NODE under
  // graph replay; scratch/probe/memset_graph.hip is the stand-alone probe of that pattern).
  VAM_REQUIRE(ptr && bytes > 0, "vam_memset_zero: bad arguments");
  VAM_REQUIRE((((uintptr_t)ptr) & 3) == 0 && (bytes & 3) == 0, "vam_memset_zero: pointer and size must be multiples of 4 bytes");
  const long n = (long)(bytes >> 2);
  hipLaunchKernelGGL(zero_words_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, (unsigned*)ptr, n);
  return check_launch("zero_words_kernel");
}

int vam_sqdiff_sum(const float* a, const float* b, long n, double* acc, void* stream) {
  VAM_REQUIRE(a && b && acc && n > 0, "vam_sqdiff_sum: bad arguments");
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 8.0 * (double)n);
  hipLaunchKernelGGL(sqdiff_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, n, acc);
  return check_launch("sqdiff_kernel");
}

}  // extern "C"
