// The device code of the two entropy models: the Gaussian conditional of the latent slices (inference tails, the
// progressive levels forms, the training likelihood and its backward, build_indexes, and the per-layer rate and coded-size
// bins) and the factorised prior of z (forward, aux loss, backward).  All Gaussian kernels are coalesced 16-byte-per-lane
// streams over NHWC channel windows (window.h), grid-stride with <= 2048 blocks.
//
// This file is compiled with -ffp-contract=off: the reference evaluates these chains as separate fp32 ops
// (entropy_models.py:140-149,620-652) and a contracted fma would change bits.
#include "common.h"
#include "window.h"

namespace vam {

constexpr int GRID_CAP = 2048;

// ------------------------------------------------------------------ Gaussian math
// entropy_models.py:573-576: 0.5 * erfc(-(2**-0.5) * t)
__device__ __forceinline__ float phi_cdf(float t) { return 0.5f * erfcf(-0.70710678118654752440f * t); }
__device__ __forceinline__ float phi_pdf(float t) { return 0.3989422804014327f * expf(-0.5f * t * t); }

// The likelihood of the unit bin around |v| under scale raw_s, before its lower bound: s = max(raw_s, 0.11)
// (LowerBound(0.11), entropy_models.py:628), lik_raw = Phi((.5 - |v|) / s) - Phi((-.5 - |v|) / s).
struct LikPoint {
  float u, l, s, lik_raw;
};
__device__ __forceinline__ LikPoint lik_point(float absv, float raw_s) {
  LikPoint q;
  q.s = fmaxf(raw_s, 0.11f);
  q.u = (0.5f - absv) / q.s;
  q.l = (-0.5f - absv) / q.s;
  q.lik_raw = phi_cdf(q.u) - phi_cdf(q.l);
  return q;
}

__device__ __forceinline__ float gauss_lik(float absv, float sigma) {
  return fmaxf(lik_point(absv, sigma).lik_raw, 1e-9f);            // likelihood_lower_bound, :650
}

// ---- training-mode Gaussian likelihood (additive-noise quantisation proxy)
//   v   = ((y - y2) - mu) * m + noise          (progressive: pic.py:437-442 / rem_pic.py:387-390; m, y2 optional)
//   s   = max(sigma * m, 0.11)                  LowerBound
//   lik = max(Phi((.5-|v|)/s) - Phi((-.5-|v|)/s), 1e-9)
// one element: d = (y - y2) - mu, m = mask (1 without one), n = noise
__device__ __forceinline__ float lik_train_fwd(float d, float sg, float m, float n, bool masked) {
  const float v = masked ? d * m + n : d + n;
  return fmaxf(lik_point(fabsf(v), masked ? sg * m : sg).lik_raw, 1e-9f);
}

// its backward: (dmu, dsigma) from the incoming gradient g of the bounded likelihood
__device__ __forceinline__ void lik_train_bwd(float d, float sg, float m, float n, float g, bool masked, float& dmu, float& dsg) {
  const float v = masked ? d * m + n : d + n;
  const float raw_s = masked ? sg * m : sg;
  const float av = fabsf(v);
  const LikPoint q = lik_point(av, raw_s);
  // LowerBound backward: pass where x >= bound or the incoming gradient is negative
  if (!(q.lik_raw >= 1e-9f || g < 0.f)) g = 0.f;
  const float pu = phi_pdf(q.u), pl = phi_pdf(q.l);
  const float dlik_dv = (av == 0.f ? 0.f : (v > 0.f ? 1.f : -1.f)) * (pl - pu) / q.s;    // d|v|/dv * dlik/d|v|
  float gs = g * (pl * q.l - pu * q.u) / q.s;                                           // dlik/ds = (-pu*u + pl*l)/s
  if (!(raw_s >= 0.11f || gs < 0.f)) gs = 0.f;                                          // LowerBound(0.11) rule
  dmu = -g * dlik_dv * m;              // d/dmu : v = (.. - mu) * m
  dsg = gs * m;                        // d/dsigma: s = sigma * m
}

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

// The residual window every Gaussian kernel starts from: d = (y - y2) - mu (pic.py:583-584; y2 optional), mu and sigma.
struct ResidualWin {
  const float *y, *y2, *mu, *sigma;
  int ld_y, ld_y2, ld_mu, ld_sigma;
};

__device__ __forceinline__ void load_residual(const ResidualWin& w, long p, int c, float* d, float* mu, float* sigma) {
  float y[4];
  ld4(w.y, p, w.ld_y, c, y);
  if (w.y2) {
    float t[4];
    ld4(w.y2, p, w.ld_y2, c, t);
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] -= t[k];
  }
  ld4(w.mu, p, w.ld_mu, c, mu);
  ld4(w.sigma, p, w.ld_sigma, c, sigma);
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = y[k] - mu[k];
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

// ------------------------------------------------------------------ Gaussian slice tail
struct TailArgs {
  ResidualWin r;
  const float* mask;
  float *yhat, *lik;
  int32_t* sym;
  double* log2sum;
  int ld_mask, ld_yhat, ld_lik, ld_sym;
  long ls_mask, ls_yhat, ls_lik, ls_sym;     // the levels form: level l's arrays sit at base + l * ls
  int pix_per_item, n_items, n_levels, C4;   // C4 = C/4
  long n_vec;                                // n_pix * C4
};

// level lv's outputs of one vector, shared by the two tail kernels (lv = 0 and level strides 0 in the one-level form)
__device__ __forceinline__ void store_tail(const TailArgs& a, int lv, long p, int c, const float* yh, const float* lk,
                                           const int* sy) {
  if (a.yhat) st4(a.yhat + lv * a.ls_yhat, p, a.ld_yhat, c, yh);
  if (a.lik) st4(a.lik + lv * a.ls_lik, p, a.ld_lik, c, lk);
  if (a.sym) sti4(a.sym + lv * a.ls_sym, p, a.ld_sym, c, sy);
}

__global__ void gauss_tail_kernel(const TailArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, a.C4, p, c);
    float dv[4], mv[4], sv[4];
    load_residual(a.r, p, c, dv, mv, sv);
    float mk[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.mask) ld4(a.mask, p, a.ld_mask, c, mk);
    float yh[4], lk[4];
    int sy[4];
    double lsum = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float q = rintf(dv[k]);                     // torch.round = half-to-even
      float absv, s;
      if (a.mask) {
        masked_tail(dv[k], q, mv[k], sv[k], mk[k], yh[k], absv, s, sy[k]);
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
    store_tail(a, 0, p, c, yh, lk, sy);
    if (a.log2sum) wave_accumulate(lsum, (int)(p / a.pix_per_item), a.log2sum);
  }
}

// The progressive tail of n_levels masks over one shared (y, y2, mu, sigma) window (vam_gauss_levels_eval): the shared
// operands are loaded once per element, level l's mask once; per level the element math of gauss_tail_kernel's masked
// branch, and level l's per-image log2 sum goes to log2sum[l * n_items + item].
__global__ void gauss_levels_eval_kernel(const TailArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, a.C4, p, c);
    float dv[4], mv[4], sv[4], qv[4];
    load_residual(a.r, p, c, dv, mv, sv);
#pragma unroll
    for (int k = 0; k < 4; ++k) qv[k] = rintf(dv[k]);                // torch.round = half-to-even
    const int item = (int)(p / a.pix_per_item);
    for (int lv = 0; lv < a.n_levels; ++lv) {
      float mk[4], yh[4], lk[4];
      ld4(a.mask + lv * a.ls_mask, p, a.ld_mask, c, mk);
      int sy[4];
      double lsum = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float absv, s;
        masked_tail(dv[k], qv[k], mv[k], sv[k], mk[k], yh[k], absv, s, sy[k]);
        lk[k] = gauss_lik(absv, s);
        lsum += log2((double)lk[k]);
      }
      store_tail(a, lv, p, c, yh, lk, sy);
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
    long p;
    int c;
    vec_at(i, a.C4, p, c);
    int sy[4];
    float mv[4];
    ldi4(a.sym, p, a.ld_sym, c, sy);
    const unsigned ly = ldb4(a.layer, p, a.ld_layer, c);
    ld4(a.mu, p, a.ld_mu, c, mv);
    for (int lv = 0; lv < a.n_levels; ++lv) {
      const int k = a.ks[lv];
      float yh[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m = layer_id(ly, e) <= k ? 1.f : 0.f;
        yh[e] = (float)sy[e] * m + mv[e];
      }
      st4(a.yhat + lv * a.ls_yhat, p, a.ld_yhat, c, yh);
    }
  }
}

// ------------------------------------------------------------------ training likelihood
struct LikArgs {
  ResidualWin r;
  const float *mask, *noise, *glik;
  float *lik, *dmu, *dsigma;
  int ld_mask, ld_noise, ld_glik, ld_lik, ld_dmu, ld_dsigma, C4;
  long n_vec;
};

template <bool BWD>
__global__ void gauss_train_kernel(const LikArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, a.C4, p, c);
    float dv[4], mv[4], sv[4], nv[4];
    load_residual(a.r, p, c, dv, mv, sv);
    ld4(a.noise, p, a.ld_noise, c, nv);
    float kv[4] = {1.f, 1.f, 1.f, 1.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.mask) ld4(a.mask, p, a.ld_mask, c, kv);
    if (BWD) ld4(a.glik, p, a.ld_glik, c, gv);
    float o0[4], o1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!BWD) o0[k] = lik_train_fwd(dv[k], sv[k], kv[k], nv[k], a.mask != nullptr);
      else lik_train_bwd(dv[k], sv[k], kv[k], nv[k], gv[k], a.mask != nullptr, o0[k], o1[k]);
    }
    if (!BWD) {
      st4(a.lik, p, a.ld_lik, c, o0);
    } else {
      st4(a.dmu, p, a.ld_dmu, c, o0);
      st4(a.dsigma, p, a.ld_dsigma, c, o1);
    }
  }
}

// ---- the progressive tail of several quality levels over one shared (y, y2, mu, sigma) window (vam_gauss_levels_*).
// Level l's arrays sit at base + l * <ls> floats.  Per element: the shared operands are read once, each level's mask /
// noise / gradient once; the arithmetic is that of gauss_tail_kernel (yhat), gauss_train_kernel and the EW_MASK_SPLIT /
// EW_AXPY launches, in the order the unfused sequence runs them (-ffp-contract=off: no contraction either way).
struct LevelsArgs {
  ResidualWin r;
  const float *mask, *noise, *glik, *drq;
  float *rq, *lik, *gmu, *dsigma, *dyt, *dys;
  int ld_mask, ld_noise, ld_glik, ld_drq, ld_rq, ld_lik, ld_gmu, ld_dsigma, ld_dyt, ld_dys, C4;
  long ls_mask, ls_noise, ls_glik, ls_drq, ls_rq, ls_lik;
  int n_levels;
  long n_vec;
};

template <bool BWD>
__global__ void gauss_levels_kernel(const LevelsArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, a.C4, p, c);
    float dv[4], mv[4], sv[4];
    load_residual(a.r, p, c, dv, mv, sv);
    float gacc[4] = {0.f, 0.f, 0.f, 0.f}, sacc[4] = {0.f, 0.f, 0.f, 0.f}, dyt[4], dys[4];
    if (BWD) {
      ld4(a.dyt, p, a.ld_dyt, c, dyt);
      if (a.dys) ld4(a.dys, p, a.ld_dys, c, dys);
    }
    for (int lv = 0; lv < a.n_levels; ++lv) {
      float kv[4], nv[4];
      ld4(a.mask + lv * a.ls_mask, p, a.ld_mask, c, kv);
      ld4(a.noise + lv * a.ls_noise, p, a.ld_noise, c, nv);
      if (!BWD) {
        float rq[4], lk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          rq[k] = rintf(dv[k]) * kv[k] + mv[k];                               // gauss_tail_kernel: yhat = round(r-mu)*m + mu
          lk[k] = lik_train_fwd(dv[k], sv[k], kv[k], nv[k], true);
        }
        st4(a.rq + lv * a.ls_rq, p, a.ld_rq, c, rq);
        st4(a.lik + lv * a.ls_lik, p, a.ld_lik, c, lk);
      } else {
        float gv[4], qv[4];
        ld4(a.glik + lv * a.ls_glik, p, a.ld_glik, c, gv);
        ld4(a.drq + lv * a.ls_drq, p, a.ld_drq, c, qv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float dmu, dsg;
          lik_train_bwd(dv[k], sv[k], kv[k], nv[k], gv[k], true, dmu, dsg);
          float dr = qv[k] * kv[k];                   // EW_MASK_SPLIT
          float g = qv[k] * (1.0f - kv[k]);
          g = g + 1.0f * dmu;                         // EW_AXPY (G_mu += dmu_lik)
          dr = dr + (-1.0f) * dmu;                    // EW_AXPY (d_r -= dmu_lik)
          dyt[k] = dyt[k] + 1.0f * dr;                // EW_AXPY into the two windows of D_y (delta_encode: r = y_top - y_sub)
          if (a.dys) dys[k] = dys[k] + (-1.0f) * dr;
          gacc[k] = gacc[k] + 1.0f * g;               // EW_AXPY: the levels' sum, level order
          sacc[k] = sacc[k] + 1.0f * dsg;
        }
      }
    }
    if (BWD) {
      st4(a.gmu, p, a.ld_gmu, c, gacc);
      st4(a.dsigma, p, a.ld_dsigma, c, sacc);
      st4(a.dyt, p, a.ld_dyt, c, dyt);
      if (a.dys) st4(a.dys, p, a.ld_dys, c, dys);
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
    long p;
    int c;
    vec_at(i, C4, p, c);
    float s[4];
    ld4(sigma, p, ld_sigma, c, s);
    if (mask) {
      float m[4];
      ld4(mask, p, ld_mask, c, m);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] *= m[k];
    }
    int r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = scale_index(s[k], tbl, n_table);
    sti4(idx, p, ld_idx, c, r);
  }
}

// ------------------------------------------------------------------ per-layer bins: rate and coded size
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

struct BinsArgs {
  ResidualWin r;
  const float* scale_table;
  const int32_t *sym, *idx;
  const uint8_t* layer;
  double* bits;
  long long* count;
  CoderTables T;
  int ld_sym, ld_idx, ld_layer, idx_base, n_table;
  int n_levels, S4, n_slices, blocks_per_stream, pix_per_item;
  long vec_per_stream;   // pix_per_item * S4
};

constexpr int LAYER_BINS = VAM_MAX_LAYER_LEVELS + 1;

// The two bins kernels bin every element of a stream (item, slice of 4 * S4 channels; vam_gauss_layer_bits has one stream
// per item) by its container layer; slot n_levels takes 0xFF and any id beyond the list.  One workgroup stays inside one
// stream; its four waves keep one row of n_levels + 1 fp64 bins (and counts) each in LDS, filled with LDS atomics, and the
// workgroup flushes one global fp64 atomic per non-empty bin.  The three pieces below are that, once.
__device__ __forceinline__ void bins_clear(double (*sh_bits)[LAYER_BINS], unsigned (*sh_cnt)[LAYER_BINS]) {
  for (int i = threadIdx.x; i < 4 * LAYER_BINS; i += 256) {
    (&sh_bits[0][0])[i] = 0.0;
    (&sh_cnt[0][0])[i] = 0u;
  }
}
__device__ __forceinline__ void bins_add(double (*sh_bits)[LAYER_BINS], unsigned (*sh_cnt)[LAYER_BINS], int l, int n_levels, double v) {
  const int wave = threadIdx.x >> 6;
  const int bin = l < n_levels ? l : n_levels;     // 0xFF (and any id beyond the list) -> the last slot
  __hip_atomic_fetch_add(&sh_bits[wave][bin], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(&sh_cnt[wave][bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// after a barrier: row `row` of bits / count [rows][nb]
__device__ __forceinline__ void bins_flush(double (*sh_bits)[LAYER_BINS], unsigned (*sh_cnt)[LAYER_BINS], int nb, long row,
                                           double* bits, long long* count) {
  const int t = threadIdx.x;
  if (t < nb) {
    const unsigned n = sh_cnt[0][t] + sh_cnt[1][t] + sh_cnt[2][t] + sh_cnt[3][t];
    if (n) {
      const double v = (sh_bits[0][t] + sh_bits[1][t]) + (sh_bits[2][t] + sh_bits[3][t]);
      atomicAdd(bits + row * nb + t, v);
      atomicAdd(reinterpret_cast<unsigned long long*>(count) + row * nb + t, (unsigned long long)n);
    }
  }
}

// The rate-only tail (vam_gauss_layer_bits): the in-mask likelihood of every element — masked_tail /
// gauss_lik with m = 1, the float gauss_levels_eval_kernel gets for an element inside a mask — binned by the element's
// container layer.
__global__ __launch_bounds__(256) void gauss_layer_bits_kernel(const BinsArgs a) {
  __shared__ double sh_bits[4][LAYER_BINS];
  __shared__ unsigned sh_cnt[4][LAYER_BINS];
  const int item = blockIdx.x / a.blocks_per_stream, blk = blockIdx.x - item * a.blocks_per_stream;
  bins_clear(sh_bits, sh_cnt);
  __syncthreads();
  const long v0 = (long)item * a.vec_per_stream;
  for (long j = (long)blk * 256 + threadIdx.x; j < a.vec_per_stream; j += (long)a.blocks_per_stream * 256) {
    long p;
    int c;
    vec_at(v0 + j, a.S4, p, c);
    float dv[4], mv[4], sv[4];
    load_residual(a.r, p, c, dv, mv, sv);
    const unsigned ly = ldb4(a.layer, p, a.ld_layer, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float yh, absv, s;
      int sy;
      masked_tail(dv[k], rintf(dv[k]), mv[k], sv[k], 1.f, yh, absv, s, sy);
      bins_add(sh_bits, sh_cnt, layer_id(ly, k), a.n_levels, log2((double)gauss_lik(absv, s)));
    }
  }
  __syncthreads();
  bins_flush(sh_bits, sh_cnt, a.n_levels + 1, item, a.bits, a.count);
}

// The coded-size tail.  SYMS: the (symbol, index) pair is read; else it is derived from (y, y2, mu,
// sigma) with masked_tail (m = 1) and scale_index.
template <bool SYMS>
__global__ __launch_bounds__(256) void coded_bits_kernel(const BinsArgs a) {
  __shared__ double sh_bits[4][LAYER_BINS];
  __shared__ unsigned sh_cnt[4][LAYER_BINS];
  __shared__ float tbl[256];
  const int stream = blockIdx.x / a.blocks_per_stream, blk = blockIdx.x - stream * a.blocks_per_stream;
  const int item = stream / a.n_slices, slice = stream - item * a.n_slices;
  bins_clear(sh_bits, sh_cnt);
  if (!SYMS)
    for (int i = threadIdx.x; i < a.n_table; i += 256) tbl[i] = a.scale_table[i];
  __syncthreads();
  const long p0 = (long)item * a.pix_per_item;
  const int c0 = slice * a.S4 * 4;
  for (long j = (long)blk * 256 + threadIdx.x; j < a.vec_per_stream; j += (long)a.blocks_per_stream * 256) {
    long pp;
    int cc;
    vec_at(j, a.S4, pp, cc);
    const long p = p0 + pp;
    const int c = c0 + cc;
    int sy[4], ix[4];
    if (SYMS) {
      ldi4(a.sym, p, a.ld_sym, c, sy);
      if (a.idx) {
        ldi4(a.idx, p, a.ld_idx, c, ix);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) ix[k] = a.idx_base + c + k;
      }
    } else {
      float dv[4], mv[4], sv[4];
      load_residual(a.r, p, c, dv, mv, sv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float yh, absv, s;
        masked_tail(dv[k], rintf(dv[k]), mv[k], sv[k], 1.f, yh, absv, s, sy[k]);
        ix[k] = scale_index(s, tbl, a.n_table);
      }
    }
    const unsigned ly = a.layer ? ldb4(a.layer, p, a.ld_layer, c) : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) bins_add(sh_bits, sh_cnt, layer_id(ly, k), a.n_levels, symbol_cost(sy[k], ix[k], a.T));
  }
  __syncthreads();
  bins_flush(sh_bits, sh_cnt, a.n_levels + 1, stream, a.bits, a.count);
}

// ------------------------------------------------------------------ factorised prior (z)
__device__ __forceinline__ float softplusf(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// Where the tensors of the 1-3-3-3-3-1 density network start in the parameter block, tensor-major and channel-major inside
// a tensor as in the state_dict:  m0[C*3] b0[C*3] f0[C*3] | 3 x (m[C*9] b[C*3] f[C*3]) | m4[C*3] b4[C] | quantiles[C*3]
struct EbOffsets {
  long C;
  __device__ __forceinline__ long m0() const { return 0; }
  __device__ __forceinline__ long b0() const { return 3 * C; }
  __device__ __forceinline__ long f0() const { return 6 * C; }
  __device__ __forceinline__ long m(int L) const { return (9 + 15 * L) * C; }      // layers 1..3: L = 0..2
  __device__ __forceinline__ long b(int L) const { return (18 + 15 * L) * C; }
  __device__ __forceinline__ long f(int L) const { return (21 + 15 * L) * C; }
  __device__ __forceinline__ long m4() const { return 54 * C; }
  __device__ __forceinline__ long b4() const { return 57 * C; }
  __device__ __forceinline__ long q() const { return 58 * C; }
};

// the network at x on a channel's preprocessed block (eb_forward_kernel's LDS layout): products first, bias last
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
// (channel, quantile): the scalar network is evaluated together with its derivative d logits / d x, each sum started from
// its bias (an order of its own, so an evaluator of its own).
__global__ void eb_aux_loss_kernel(const float* __restrict__ params, int C, float t0, float t1, float t2,
                                   double* __restrict__ loss, float* __restrict__ dq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * C) return;
  const int c = i / 3, k3 = i - 3 * c;
  const EbOffsets o = {C};
  const float *m0 = params + o.m0(), *b0 = params + o.b0(), *f0 = params + o.f0();
  const float x = params[o.q() + c * 3 + k3];
  float l[3], dl[3];
  for (int k = 0; k < 3; ++k) {
    const float a = softplusf(m0[c * 3 + k]);
    const float v = a * x + b0[c * 3 + k];
    const float f = tanhf(f0[c * 3 + k]), th = tanhf(v);
    l[k] = v + f * th;
    dl[k] = a * (1.0f + f * (1.0f - th * th));
  }
  for (int layer = 0; layer < 3; ++layer) {
    const float *m = params + o.m(layer), *b = params + o.b(layer), *f = params + o.f(layer);
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
  }
  const float *m4 = params + o.m4(), *b4 = params + o.b4();
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
  const EbOffsets o = {C};
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float* sp = sh + c * 62;
    const float *m0 = params + o.m0(), *b0 = params + o.b0(), *f0 = params + o.f0();
    for (int k = 0; k < 3; ++k) {
      sp[k] = softplusf(m0[c * 3 + k]);
      sp[3 + k] = b0[c * 3 + k];
      sp[6 + k] = tanhf(f0[c * 3 + k]);
    }
    for (int layer = 0; layer < 3; ++layer) {
      const float *m = params + o.m(layer), *b = params + o.b(layer), *f = params + o.f(layer);
      float* q = sp + 9 + layer * 15;
      for (int k = 0; k < 9; ++k) q[k] = softplusf(m[c * 9 + k]);
      for (int k = 0; k < 3; ++k) { q[9 + k] = b[c * 3 + k]; q[12 + k] = tanhf(f[c * 3 + k]); }
    }
    const float *m4 = params + o.m4(), *b4 = params + o.b4(), *qn = params + o.q();
    float* q = sp + 54;
    for (int k = 0; k < 3; ++k) q[k] = softplusf(m4[c * 3 + k]);
    q[3] = b4[c];
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
    float su = sigmoidf(sign * upper);
    float sl = sigmoidf(sign * lower);
    float lk = fmaxf(fabsf(su - sl), 1e-9f);
    if (zhat) zhat[p * ld_zhat + c] = o;
    if (lik) lik[p * ld_lik + c] = lk;
    if (log2sum) atomicAdd(log2sum + (int)(p / pix_per_item), log2((double)lk));
  }
}

// The noise likelihood's gradient w.r.t. z and the 14 density-network tensors (entropy_models.py:403-436,449-492; the
// LowerBound rule on the 1e-9 likelihood bound): the backward of first-stage training.  Fixed reduction order, no float atomics.
// Per-channel parameter block (58 values): layer 0: m[3] b[3] f[3]; layers 1..3: m[9] b[3] f[3]; layer 4: m[3] b[1].
// `raw` keeps the stored values (for softplus' = sigmoid(raw m), tanh' = 1 - tanh(raw f)^2), `sp` the transformed ones.
struct EbNet {
  float m0[3], b0[3], f0[3];
  float m[3][9], b[3][3], f[3][3];
  float m4[3], b4;
};

// forward of the 1-3-3-3-3-1 network at x keeping what the backward needs
struct EbTrace {
  float th0[3], l0[3];          // tanh(v) and output of layer 0
  float th[3][3], l[3][3];      // layers 1..3
};

__device__ __forceinline__ float eb_fwd(const EbNet& n, float x, EbTrace& t) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = n.m0[k] * x + n.b0[k];
    t.th0[k] = tanhf(v);
    t.l0[k] = v + n.f0[k] * t.th0[k];
  }
  const float* in = t.l0;
#pragma unroll
  for (int L = 0; L < 3; ++L) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = n.m[L][k * 3 + 0] * in[0];
      v = v + n.m[L][k * 3 + 1] * in[1];
      v = v + n.m[L][k * 3 + 2] * in[2];
      v = v + n.b[L][k];
      t.th[L][k] = tanhf(v);
      t.l[L][k] = v + n.f[L][k] * t.th[L][k];
    }
    in = t.l[L];
  }
  float v = n.m4[0] * in[0];
  v = v + n.m4[1] * in[1];
  v = v + n.m4[2] * in[2];
  return v + n.b4;
}

// backward of one evaluation: g = dL/dlogit; accumulates dL/d(transformed parameters) into `acc` (same struct layout,
// still w.r.t. softplus(m) / tanh(f): the chain to the stored values is applied once per channel at the end), returns dL/dx
__device__ __forceinline__ float eb_bwd(const EbNet& n, float x, const EbTrace& t, float g, EbNet& acc) {
  float gin[3];
  const float* in = t.l[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    acc.m4[j] += g * in[j];
    gin[j] = g * n.m4[j];
  }
  acc.b4 += g;
#pragma unroll
  for (int L = 2; L >= 0; --L) {
    const float* prev = L == 0 ? t.l0 : t.l[L - 1];
    float gp[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float th = t.th[L][k];
      acc.f[L][k] += gin[k] * th;
      const float gv = gin[k] * (1.0f + n.f[L][k] * (1.0f - th * th));
      acc.b[L][k] += gv;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        acc.m[L][k * 3 + j] += gv * prev[j];
        gp[j] += gv * n.m[L][k * 3 + j];
      }
    }
    gin[0] = gp[0]; gin[1] = gp[1]; gin[2] = gp[2];
  }
  float gx = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float th = t.th0[k];
    acc.f0[k] += gin[k] * th;
    const float gv = gin[k] * (1.0f + n.f0[k] * (1.0f - th * th));
    acc.b0[k] += gv;
    acc.m0[k] += gv * x;
    gx += gv * n.m0[k];
  }
  return gx;
}

constexpr int EB_NPAR = 58;
constexpr int EB_THREADS = 128;

// One block per channel.  params as for vam_eb_forward.
__global__ __launch_bounds__(EB_THREADS) void eb_train_bwd_kernel(const float* __restrict__ z, int ld_z,
                                                                  const float* __restrict__ noise, int ld_noise,
                                                                  const float* __restrict__ params, int C,
                                                                  const float* __restrict__ glik, int ld_g,
                                                                  float* __restrict__ dz, int ld_dz,
                                                                  float* __restrict__ dparams, long n_pix) {
  __shared__ float red[EB_NPAR][EB_THREADS + 1];
  const int c = blockIdx.x;
  const EbOffsets o = {C};
  EbNet n, raw;
  for (int k = 0; k < 3; ++k) {
    raw.m0[k] = params[o.m0() + c * 3 + k]; n.m0[k] = softplusf(raw.m0[k]);
    n.b0[k] = params[o.b0() + c * 3 + k];
    raw.f0[k] = params[o.f0() + c * 3 + k]; n.f0[k] = tanhf(raw.f0[k]);
    raw.m4[k] = params[o.m4() + c * 3 + k]; n.m4[k] = softplusf(raw.m4[k]);
  }
  n.b4 = params[o.b4() + c];
  for (int L = 0; L < 3; ++L) {
    for (int k = 0; k < 9; ++k) { raw.m[L][k] = params[o.m(L) + c * 9 + k]; n.m[L][k] = softplusf(raw.m[L][k]); }
    for (int k = 0; k < 3; ++k) {
      n.b[L][k] = params[o.b(L) + c * 3 + k];
      raw.f[L][k] = params[o.f(L) + c * 3 + k]; n.f[L][k] = tanhf(raw.f[L][k]);
    }
  }
  EbNet acc;
  {
    float* a = reinterpret_cast<float*>(&acc);
    for (int i = 0; i < EB_NPAR; ++i) a[i] = 0.f;
  }
  for (long p = threadIdx.x; p < n_pix; p += EB_THREADS) {
    const float x = z[p * ld_z + c] + noise[p * ld_noise + c];
    EbTrace tl, tu;
    const float lower = eb_fwd(n, x - 0.5f, tl);
    const float upper = eb_fwd(n, x + 0.5f, tu);
    const float sum = lower + upper;
    const float sign = sum > 0.f ? -1.f : (sum < 0.f ? 1.f : 0.f);          // detached (entropy_models.py:431-432)
    const float su = sigmoidf(sign * upper), sl = sigmoidf(sign * lower);
    const float diff = su - sl;
    const float lik_raw = fabsf(diff);
    float g = glik[p * ld_g + c];
    if (!(lik_raw >= 1e-9f || g < 0.f)) g = 0.f;                            // LowerBound(1e-9) gradient rule
    const float gd = g * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));     // torch.abs backward (0 at 0)
    const float gu = gd * su * (1.0f - su) * sign;
    const float gl = -gd * sl * (1.0f - sl) * sign;
    const float gx = eb_bwd(n, x + 0.5f, tu, gu, acc) + eb_bwd(n, x - 0.5f, tl, gl, acc);
    dz[p * ld_dz + c] = gx;
  }
  // chain to the stored values: d softplus(m)/dm = sigmoid(m); d tanh(f)/df = 1 - tanh(f)^2
  for (int k = 0; k < 3; ++k) {
    acc.m0[k] *= sigmoidf(raw.m0[k]);
    acc.f0[k] *= 1.0f - n.f0[k] * n.f0[k];
    acc.m4[k] *= sigmoidf(raw.m4[k]);
  }
  for (int L = 0; L < 3; ++L) {
    for (int k = 0; k < 9; ++k) acc.m[L][k] *= sigmoidf(raw.m[L][k]);
    for (int k = 0; k < 3; ++k) acc.f[L][k] *= 1.0f - n.f[L][k] * n.f[L][k];
  }
  {
    const float* a = reinterpret_cast<const float*>(&acc);
    for (int i = 0; i < EB_NPAR; ++i) red[i][threadIdx.x] = a[i];
  }
  __syncthreads();
  if (threadIdx.x < EB_NPAR) {
    float s = 0.f;
    for (int t = 0; t < EB_THREADS; ++t) s += red[threadIdx.x][t];         // fixed order
    // EbNet member order: m0[3] b0[3] f0[3] | m[3][9] b[3][3] f[3][3] | m4[3] b4
    const int i = threadIdx.x;
    long dst;
    if (i < 3) dst = o.m0() + c * 3 + i;
    else if (i < 6) dst = o.b0() + c * 3 + (i - 3);
    else if (i < 9) dst = o.f0() + c * 3 + (i - 6);
    else if (i < 36) { const int L = (i - 9) / 9, k = (i - 9) % 9; dst = o.m(L) + c * 9 + k; }
    else if (i < 45) { const int L = (i - 36) / 3, k = (i - 36) % 3; dst = o.b(L) + c * 3 + k; }
    else if (i < 54) { const int L = (i - 45) / 3, k = (i - 45) % 3; dst = o.f(L) + c * 3 + k; }
    else if (i < 57) dst = o.m4() + c * 3 + (i - 54);
    else dst = o.b4() + c;
    dparams[dst] = s;
  }
  if (threadIdx.x < 3) dparams[o.q() + c * 3 + threadIdx.x] = 0.f;            // the noise likelihood does not see the quantiles
}

}  // namespace vam

using namespace vam;

// ------------------------------------------------------------------ entry points
static const WinWords TAIL_WORDS = {"need y, mu, sigma", "16-byte alignment", "strides must be multiples of 4"};

// the four windows of a ResidualWin under one entry's rules
static int check_residual(const char* who, int C, const ResidualWin& r, bool at_least_C, const WinWords& w) {
  return check_windows(who, C,
                       {{"y", r.y, r.ld_y, 0, true, 16, at_least_C},
                        {"y2", r.y2, r.ld_y2, 0, false, 16, at_least_C},
                        {"mu", r.mu, r.ld_mu, 0, true, 16, at_least_C},
                        {"sigma", r.sigma, r.ld_sigma, 0, true, 16, at_least_C}},
                       w);
}

extern "C" {

// What the two tail entries share once their own rules have passed: the window rules, the byte count and the launch.  The
// one-level form has an optional mask, no level strides and n_levels = 1.
static int launch_tail(const char* who, bool levels, const TailArgs& a, long n_pix, int C, void* stream) {
  if (int rc = check_residual(who, C, a.r, false, TAIL_WORDS)) return rc;
  VAM_CHECK_WINDOWS(who, C,
                    {{"mask", a.mask, a.ld_mask, a.ls_mask, levels, 16, false},
                     {"yhat", a.yhat, a.ld_yhat, a.ls_yhat, false, 16, false},
                     {"lik", a.lik, a.ld_lik, a.ls_lik, false, 16, false},
                     {"sym", a.sym, a.ld_sym, a.ls_sym, false, 16, false}},
                    TAIL_WORDS);
  const int nin = 3 + (a.r.y2 ? 1 : 0) + (levels ? a.n_levels : (a.mask ? 1 : 0));
  const int nout = a.n_levels * ((a.yhat ? 1 : 0) + (a.lik ? 1 : 0) + (a.sym ? 1 : 0));
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 4.0 * (double)n_pix * C * (nin + nout));
  const dim3 grid(stream_grid(a.n_vec, 256, GRID_CAP));
  if (levels) hipLaunchKernelGGL(gauss_levels_eval_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(gauss_tail_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(levels ? "gauss_levels_eval_kernel" : "gauss_tail_kernel");
}

int vam_gauss_tail(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                   const float* sigma, int ld_sigma, const float* mask, int ld_mask, float* yhat, int ld_yhat,
                   float* lik, int ld_lik, int32_t* sym, int ld_sym, double* log2sum, int pix_per_item, long n_pix,
                   int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_tail: need y, mu, sigma and C %% 4 == 0");
  VAM_REQUIRE(!log2sum || pix_per_item > 0, "vam_gauss_tail: pix_per_item");
  const TailArgs a = {{y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma}, mask, yhat, lik, sym, log2sum, ld_mask, ld_yhat, ld_lik, ld_sym,
                      0, 0, 0, 0, pix_per_item, 0, 1, C / 4, n_pix * (C / 4)};
  return launch_tail("vam_gauss_tail", false, a, n_pix, C, stream);
}

int vam_gauss_levels_eval(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                          const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls, float* yhat,
                          int ld_yhat, long yhat_ls, float* lik, int ld_lik, long lik_ls, int32_t* sym, int ld_sym,
                          long sym_ls, double* log2sum, int pix_per_item, int n_levels, long n_pix, int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && mask && n_levels > 0 && n_pix > 0 && C > 0 && C % 4 == 0,
              "vam_gauss_levels_eval: need y, mu, sigma, mask, n_levels > 0 and C %% 4 == 0");
  VAM_REQUIRE(!log2sum || (pix_per_item > 0 && n_pix % pix_per_item == 0), "vam_gauss_levels_eval: pix_per_item");
  const int ppi = pix_per_item > 0 ? pix_per_item : 1;
  VAM_REQUIRE(n_pix / ppi * (long)n_levels < (1L << 31), "vam_gauss_levels_eval: too many items");
  const TailArgs a = {{y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma}, mask, yhat, lik, sym, log2sum, ld_mask, ld_yhat, ld_lik, ld_sym,
                      mask_ls, yhat_ls, lik_ls, sym_ls, ppi, (int)(n_pix / ppi), n_levels, C / 4, n_pix * (C / 4)};
  return launch_tail("vam_gauss_levels_eval", true, a, n_pix, C, stream);
}

int vam_gauss_levels_decode(const int32_t* sym, int ld_sym, const uint8_t* layer, int ld_layer, const float* mu, int ld_mu,
                            const int* ks, int n_levels, float* yhat, int ld_yhat, long yhat_ls, long n_pix, int C,
                            void* stream) {
  VAM_REQUIRE(ks && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_levels_decode: bad arguments");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_MASK_LEVELS, "vam_gauss_levels_decode: 1..%d levels, got %d",
              VAM_MAX_MASK_LEVELS, n_levels);
  VAM_CHECK_WINDOWS("vam_gauss_levels_decode", C,
                    {{"sym", sym, ld_sym, 0, true, 16, false},
                     {"layer", layer, ld_layer, 0, true, 4, false},
                     {"mu", mu, ld_mu, 0, true, 16, false},
                     {"yhat", yhat, ld_yhat, yhat_ls, true, 16, false}},
                    {"bad arguments", "alignment", "strides must be multiples of 4"});
  DecodeLevelsArgs a = {sym, layer, mu, yhat, ld_sym, ld_layer, ld_mu, ld_yhat, yhat_ls, {}, n_levels, C / 4, n_pix * (C / 4)};
  for (int l = 0; l < VAM_MAX_MASK_LEVELS; ++l) a.ks[l] = l < n_levels ? ks[l] : -1;
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, (double)n_pix * C * (9.0 + 4.0 * n_levels));
  hipLaunchKernelGGL(gauss_levels_decode_kernel, dim3(stream_grid(a.n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_levels_decode_kernel");
}

int vam_build_indexes(const float* sigma, int ld_sigma, const float* mask, int ld_mask, const float* table,
                      int n_table, int32_t* idx, int ld_idx, long n_pix, int C, void* stream) {
  VAM_REQUIRE(table && n_pix > 0 && C > 0 && C % 4 == 0, "vam_build_indexes: bad arguments");
  VAM_REQUIRE(n_table >= 2 && n_table <= 256, "vam_build_indexes: table size %d", n_table);
  VAM_CHECK_WINDOWS("vam_build_indexes", C,
                    {{"sigma", sigma, ld_sigma, 0, true, 16, false},
                     {"mask", mask, ld_mask, 0, false, 16, false},
                     {"idx", idx, ld_idx, 0, true, 16, false}},
                    {"bad arguments", "alignment", "alignment"});
  long n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 4.0 * (double)n_pix * C * (mask ? 3 : 2));
  hipLaunchKernelGGL(build_indexes_kernel, dim3(stream_grid(n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, sigma,
                     ld_sigma, mask, ld_mask, table, n_table, idx, ld_idx, n_vec, C / 4);
  return check_launch("build_indexes_kernel");
}

enum { BINS_WINDOW_COST, BINS_SYMBOL_COST, BINS_LOG2_LIK };     // vam_coded_layer_bits, vam_coded_symbol_bits, vam_gauss_layer_bits

// Sizes and launches a bins kernel over n_streams streams of a.vec_per_stream vectors: a workgroup stays inside
// one stream; about two vectors per lane, and no more than ~2048 workgroups in all.
static int launch_bins(int kind, BinsArgs& a, long n_streams, double bytes, void* stream) {
  long per = cdiv(a.vec_per_stream, 512L);
  const long room = n_streams >= 2048 ? 1 : 2048 / n_streams;
  if (per > room) per = room;
  if (per < 1) per = 1;
  a.blocks_per_stream = (int)per;
  const dim3 grid((unsigned)(n_streams * per));
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, bytes);
  if (kind == BINS_SYMBOL_COST)
    hipLaunchKernelGGL(coded_bits_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (kind == BINS_WINDOW_COST)
    hipLaunchKernelGGL(coded_bits_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(gauss_layer_bits_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(kind == BINS_LOG2_LIK ? "gauss_layer_bits_kernel" : "coded_bits_kernel");
}

int vam_gauss_layer_bits(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const uint8_t* layer, int ld_layer, int n_levels,
                         double* bits, long long* count, int pix_per_item, long n_pix, int C, void* stream) {
  static const WinWords words = {"y, mu, sigma, layer, bits and count must not be NULL", "alignment",
                                 "pixel strides must be multiples of 4 and >= C"};
  VAM_REQUIRE(n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_layer_bits: need n_pix > 0 and C %% 4 == 0");
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "vam_gauss_layer_bits: 1..%d levels, got %d",
              VAM_MAX_LAYER_LEVELS, n_levels);
  VAM_REQUIRE(pix_per_item > 0 && n_pix % pix_per_item == 0, "vam_gauss_layer_bits: pix_per_item must divide n_pix");
  VAM_REQUIRE((long)pix_per_item * C < (1L << 31) && n_pix / pix_per_item < (1L << 24), "vam_gauss_layer_bits: item too large");
  BinsArgs a = {};
  a.r = {y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma};
  if (int rc = check_residual("vam_gauss_layer_bits", C, a.r, true, words)) return rc;
  VAM_CHECK_WINDOWS("vam_gauss_layer_bits", C,
                    {{"layer", layer, ld_layer, 0, true, 4, true},
                     {"bits", bits, 0, 0, true, 8, false},
                     {"count", count, 0, 0, true, 8, false}},
                    words);
  a.layer = layer; a.ld_layer = ld_layer; a.bits = bits; a.count = count;
  a.n_levels = n_levels; a.S4 = C / 4; a.n_slices = 1; a.pix_per_item = pix_per_item;
  a.vec_per_stream = (long)pix_per_item * (C / 4);
  return launch_bins(BINS_LOG2_LIK, a, n_pix / pix_per_item, (double)n_pix * C * (y2 ? 17.0 : 13.0), stream);
}

// what the two coded-size entries share: the coder tables, the streams and the bins
static int coded_bits_launch(int kind, BinsArgs& a, const char* who, const vam_coder_tables* tables, const uint8_t* layer,
                             int ld_layer, int n_levels, int chans_per_stream, double* bits, long long* count,
                             int pix_per_item, long n_pix, int C, double bytes_per_elem, void* stream) {
  VAM_REQUIRE(tables && tables->cost && tables->sizes && tables->offsets && bits && count, "%s: tables, bits and count must not be NULL", who);
  VAM_REQUIRE(tables->n_cdfs >= 1 && tables->stride >= 2, "%s: %d tables of stride %d", who, tables->n_cdfs, tables->stride);
  VAM_REQUIRE(n_pix > 0 && C > 0 && C % 4 == 0, "%s: need n_pix > 0 and C %% 4 == 0", who);
  VAM_REQUIRE(chans_per_stream > 0 && chans_per_stream % 4 == 0 && C % chans_per_stream == 0,
              "%s: chans_per_stream %d must be a multiple of 4 that divides C = %d", who, chans_per_stream, C);
  VAM_REQUIRE(n_levels >= 1 && n_levels <= VAM_MAX_LAYER_LEVELS, "%s: 1..%d levels, got %d", who, VAM_MAX_LAYER_LEVELS, n_levels);
  VAM_REQUIRE(pix_per_item > 0 && n_pix % pix_per_item == 0, "%s: pix_per_item must divide n_pix", who);
  VAM_REQUIRE((long)pix_per_item * C < (1L << 31) && n_pix / pix_per_item * (C / chans_per_stream) < (1L << 20), "%s: item too large", who);
  VAM_CHECK_WINDOWS(who, C,
                    {{"layer", layer, ld_layer, 0, false, 4, true},
                     {"bits", bits, 0, 0, true, 8, false},
                     {"count", count, 0, 0, true, 8, false},
                     {"tables->cost", tables->cost, 0, 0, true, 8, false}},
                    {"tables, bits and count must not be NULL", "alignment / layer stride", "alignment / layer stride"});
  a.layer = layer; a.ld_layer = ld_layer; a.bits = bits; a.count = count;
  a.T.cost = tables->cost; a.T.sizes = tables->sizes; a.T.offsets = tables->offsets;
  a.T.n_cdfs = tables->n_cdfs; a.T.stride = tables->stride;
  a.n_levels = n_levels; a.S4 = chans_per_stream / 4; a.n_slices = C / chans_per_stream; a.pix_per_item = pix_per_item;
  a.vec_per_stream = (long)pix_per_item * a.S4;
  return launch_bins(kind, a, n_pix / pix_per_item * a.n_slices, (double)n_pix * C * bytes_per_elem, stream);
}

int vam_coded_layer_bits(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const uint8_t* layer, int ld_layer, int n_levels,
                         const float* scale_table, int n_table, const vam_coder_tables* tables, int chans_per_stream,
                         double* bits, long long* count, int pix_per_item, long n_pix, int C, void* stream) {
  VAM_REQUIRE(scale_table, "vam_coded_layer_bits: y, mu, sigma and scale_table must not be NULL");
  VAM_REQUIRE(n_table >= 2 && n_table <= 256 && tables && n_table <= tables->n_cdfs,
              "vam_coded_layer_bits: scale table of %d entries (2..256, at most one per coder table)", n_table);
  BinsArgs a = {};
  a.r = {y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma};
  if (int rc = check_residual("vam_coded_layer_bits", C, a.r, true,
                              {"y, mu, sigma and scale_table must not be NULL", "16-byte alignment",
                               "pixel strides must be multiples of 4 and >= C"}))
    return rc;
  a.scale_table = scale_table; a.n_table = n_table;
  return coded_bits_launch(BINS_WINDOW_COST, a, "vam_coded_layer_bits", tables, layer, ld_layer, n_levels, chans_per_stream, bits,
                           count, pix_per_item, n_pix, C, (y2 ? 16.0 : 12.0) + (layer ? 1.0 : 0.0), stream);
}

int vam_coded_symbol_bits(const int32_t* sym, int ld_sym, const int32_t* idx, int ld_idx, int idx_base,
                          const uint8_t* layer, int ld_layer, int n_levels, const vam_coder_tables* tables,
                          int chans_per_stream, double* bits, long long* count, int pix_per_item, long n_pix, int C,
                          void* stream) {
  VAM_CHECK_WINDOWS("vam_coded_symbol_bits", C,
                    {{"sym", sym, ld_sym, 0, true, 16, true}, {"idx", idx, ld_idx, 0, false, 16, true}},
                    {"sym must not be NULL; 16-byte alignment", "sym must not be NULL; 16-byte alignment",
                     "pixel strides must be multiples of 4 and >= C"});
  VAM_REQUIRE(idx || (tables && idx_base >= 0 && (long)idx_base + C <= tables->n_cdfs),
              "vam_coded_symbol_bits: without idx the channels idx_base .. idx_base + C must name tables");
  BinsArgs a = {};
  a.sym = sym; a.idx = idx; a.ld_sym = ld_sym; a.ld_idx = ld_idx; a.idx_base = idx_base;
  return coded_bits_launch(BINS_SYMBOL_COST, a, "vam_coded_symbol_bits", tables, layer, ld_layer, n_levels, chans_per_stream, bits,
                           count, pix_per_item, n_pix, C, (idx ? 8.0 : 4.0) + (layer ? 1.0 : 0.0), stream);
}

int vam_gauss_train(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu, const float* sigma,
                    int ld_sigma, const float* mask, int ld_mask, const float* noise, int ld_noise, const float* grad_lik,
                    int ld_glik, float* lik, int ld_lik, float* dmu, int ld_dmu, float* dsigma, int ld_dsigma, long n_pix,
                    int C, void* stream) {
  VAM_REQUIRE(y && mu && sigma && noise && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_train: bad arguments");
  const bool bwd = grad_lik != nullptr;
  VAM_REQUIRE(bwd ? (dmu && dsigma) : (lik != nullptr), "vam_gauss_train: forward needs lik, backward needs dmu and dsigma");
  const LikArgs a = {{y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma}, mask, noise, grad_lik, lik, dmu, dsigma,
                     ld_mask, ld_noise, ld_glik, ld_lik, ld_dmu, ld_dsigma, C / 4, n_pix * (C / 4)};
  if (int rc = check_residual("vam_gauss_train", C, a.r, false, WinWords())) return rc;
  // the strides of the direction that does not run are not looked at
  VAM_CHECK_WINDOWS("vam_gauss_train", C,
                    {{"mask", mask, ld_mask, 0, false, 16, false},
                     {"noise", noise, ld_noise, 0, true, 16, false},
                     {"grad_lik", grad_lik, ld_glik, 0, false, 16, false},
                     {"lik", lik, bwd ? 0 : ld_lik, 0, false, 16, false},
                     {"dmu", dmu, bwd ? ld_dmu : 0, 0, false, 16, false},
                     {"dsigma", dsigma, bwd ? ld_dsigma : 0, 0, false, 16, false}});
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 4.0 * (double)n_pix * C * 8);
  const dim3 grid(stream_grid(a.n_vec, 256, GRID_CAP));
  if (bwd) hipLaunchKernelGGL((gauss_train_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((gauss_train_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_train_kernel");
}

int vam_gauss_levels_fwd(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls,
                         const float* noise, int ld_noise, long noise_ls, float* rq, int ld_rq, long rq_ls,
                         float* lik, int ld_lik, long lik_ls, int n_levels, long n_pix, int C, void* stream) {
  VAM_REQUIRE(n_levels > 0 && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_levels_fwd: bad arguments");
  LevelsArgs a{};
  a.r = {y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma};
  if (int rc = check_residual("vam_gauss_levels_fwd", C, a.r, false, WinWords())) return rc;
  VAM_CHECK_WINDOWS("vam_gauss_levels_fwd", C,
                    {{"mask", mask, ld_mask, mask_ls, true, 16, false},
                     {"noise", noise, ld_noise, noise_ls, true, 16, false},
                     {"rq", rq, ld_rq, rq_ls, true, 16, false},
                     {"lik", lik, ld_lik, lik_ls, true, 16, false}});
  a.mask = mask; a.noise = noise; a.rq = rq; a.lik = lik;
  a.ld_mask = ld_mask; a.ld_noise = ld_noise; a.ld_rq = ld_rq; a.ld_lik = ld_lik;
  a.ls_mask = mask_ls; a.ls_noise = noise_ls; a.ls_rq = rq_ls; a.ls_lik = lik_ls;
  a.n_levels = n_levels; a.C4 = C / 4; a.n_vec = n_pix * (C / 4);
  hipLaunchKernelGGL((gauss_levels_kernel<false>), dim3(stream_grid(a.n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_levels_kernel");
}

int vam_gauss_levels_bwd(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls,
                         const float* noise, int ld_noise, long noise_ls, const float* grad_lik, int ld_glik, long glik_ls,
                         const float* d_rq, int ld_drq, long drq_ls, float* gmu, int ld_gmu, float* dsigma, int ld_dsigma,
                         float* dy_top, int ld_dyt, float* dy_sub, int ld_dys, int n_levels, long n_pix, int C, void* stream) {
  VAM_REQUIRE(n_levels > 0 && n_pix > 0 && C > 0 && C % 4 == 0, "vam_gauss_levels_bwd: bad arguments");
  LevelsArgs a{};
  a.r = {y, y2, mu, sigma, ld_y, ld_y2, ld_mu, ld_sigma};
  if (int rc = check_residual("vam_gauss_levels_bwd", C, a.r, false, WinWords())) return rc;
  VAM_CHECK_WINDOWS("vam_gauss_levels_bwd", C,
                    {{"mask", mask, ld_mask, mask_ls, true, 16, false},
                     {"noise", noise, ld_noise, noise_ls, true, 16, false},
                     {"grad_lik", grad_lik, ld_glik, glik_ls, true, 16, false},
                     {"d_rq", d_rq, ld_drq, drq_ls, true, 16, false},
                     {"gmu", gmu, ld_gmu, 0, true, 16, false},
                     {"dsigma", dsigma, ld_dsigma, 0, true, 16, false},
                     {"dy_top", dy_top, ld_dyt, 0, true, 16, false},
                     {"dy_sub", dy_sub, ld_dys, 0, false, 16, false}});
  a.mask = mask; a.noise = noise; a.glik = grad_lik; a.drq = d_rq;
  a.gmu = gmu; a.dsigma = dsigma; a.dyt = dy_top; a.dys = dy_sub;
  a.ld_mask = ld_mask; a.ld_noise = ld_noise; a.ld_glik = ld_glik; a.ld_drq = ld_drq; a.ld_gmu = ld_gmu;
  a.ld_dsigma = ld_dsigma; a.ld_dyt = ld_dyt; a.ld_dys = ld_dys;
  a.ls_mask = mask_ls; a.ls_noise = noise_ls; a.ls_glik = glik_ls; a.ls_drq = drq_ls;
  a.n_levels = n_levels; a.C4 = C / 4; a.n_vec = n_pix * (C / 4);
  hipLaunchKernelGGL((gauss_levels_kernel<true>), dim3(stream_grid(a.n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("gauss_levels_kernel");
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
  if (int rc = vam_memset_zero(loss, sizeof(double), stream)) return rc;
  hipLaunchKernelGGL(eb_aux_loss_kernel, dim3(cdiv(3L * C, 64)), dim3(64), 0, s, params, C, target3_host[0], target3_host[1],
                     target3_host[2], loss, dquantiles);
  return check_launch("eb_aux_loss_kernel");
}

int vam_eb_train_bwd(const float* z, int ld_z, const float* noise, int ld_noise, const float* params, int C,
                     const float* grad_lik, int ld_glik, float* dz, int ld_dz, float* dparams, long n_pix, void* stream) {
  VAM_REQUIRE(z && noise && params && grad_lik && dz && dparams && C > 0 && n_pix > 0, "vam_eb_train_bwd: bad arguments");
  VAM_REQUIRE(ld_z >= C && ld_noise >= C && ld_glik >= C && ld_dz >= C, "vam_eb_train_bwd: pixel strides");
  hipLaunchKernelGGL(eb_train_bwd_kernel, dim3(C), dim3(EB_THREADS), 0, (hipStream_t)stream, z, ld_z, noise, ld_noise, params, C,
                     grad_lik, ld_glik, dz, ld_dz, dparams, n_pix);
  return check_launch("eb_train_bwd_kernel");
}

}  // extern "C"
