// Weight, bias and scale packing for the convolution kernel (conv_igemm.hip), and max |x| of a tensor for its fp16x2 mode.
#include "conv_host.h"

namespace vam {

// ---------------------------------------------------------------- weight packing
__device__ __forceinline__ float pack_value(const float* __restrict__ src, int mode, int phase, int kh, int kw, int cin,
                                            int n, int nn, int cc, int ty, int tx) {
  float v = 0.f;
  if (nn < n && cc < cin) {
    if (mode == VAM_PACK_CONV) {
      v = src[(((size_t)nn * cin + cc) * kh + ty) * kw + tx];
    } else if (mode == VAM_PACK_PS2) {
      int cq = n / 4;
      int ph = nn / cq, c = nn - ph * cq;
      v = src[(((size_t)(c * 4 + ph) * cin + cc) * kh + ty) * kw + tx];
    } else if (mode == VAM_PACK_CONV_DGRAD) {
      // data gradient of a stride-1 conv = correlation of dY with the taps flipped and the channel roles
      // swapped: here `cin` = forward Cout (channels of dY), `n` = forward Cin; src is the forward OIHW tensor
      v = src[(((size_t)cc * n + nn) * kh + (kh - 1 - ty)) * kw + (kw - 1 - tx)];
    } else if (mode == VAM_PACK_GDN || mode == VAM_PACK_GDN_T) {
      float g = mode == VAM_PACK_GDN ? src[(size_t)nn * cin + cc] : src[(size_t)cc * n + nn];   // _T: gamma transposed
      const float bound = 3.814697265625e-06f;       // 2^-18 = sqrt(0 + 2^-36)
      const float ped = 1.4551915228366852e-11f;     // 2^-36
      g = fmaxf(g, bound);
      v = g * g - ped;
    } else if (mode == VAM_PACK_DECONV5S2) {
      if (phase >= 0) {
        int py = phase >> 1, px = phase & 1;
        int dy = ty - (py ? 0 : 1), dx = tx - (px ? 0 : 1);
        int ky = py + 2 - 2 * dy, kx = px + 2 - 2 * dx;
        if (ky >= 0 && ky < 5 && kx >= 0 && kx < 5)
          v = src[(((size_t)cc * n + nn) * 5 + ky) * 5 + kx];
      } else {
        int cout = n / 4;
        int ph = nn / cout, c = nn - ph * cout;
        int py = ph >> 1, px = ph & 1;
        int dy = ty - 1, dx = tx - 1;
        int ky = py + 2 - 2 * dy, kx = px + 2 - 2 * dx;
        if (ky >= 0 && ky < 5 && kx >= 0 && kx < 5)
          v = src[(((size_t)cc * cout + c) * 5 + ky) * 5 + kx];
      }
    }
  }
  return v;
}

__global__ void pack_weights_kernel(const float* __restrict__ src, float* __restrict__ dst, int mode,
                                    int phase, int kh, int kw, int cin, int n, int npad, int bk, int kc,
                                    long total) {
  long d = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= total) return;
  int kk = (int)(d % bk);
  long r = d / bk;
  int nn = (int)(r % npad);
  r /= npad;
  int c_chunk = (int)(r % kc);
  int tap = (int)(r / kc);
  int ty = tap / kw, tx = tap % kw;
  int cc = c_chunk * bk + kk;
  dst[d] = pack_value(src, mode, phase, kh, kw, cin, n, nn, cc, ty, tx);
}

// bf16x3 layout: [tap][32-channel chunk][Npad][12 chunks][8 bf16]; chunk (p*4 + g) holds plane p (hi/mid/lo) of
// channels 8g..8g+7 of the 32-channel chunk.  The three planes sum to the fp32 weight exactly.
__device__ __forceinline__ void pack_bf3_element(long d, const float* __restrict__ src, unsigned short* __restrict__ dst, int mode,
                                                 int phase, int kh, int kw, int cin, int n, int npad, int kc32, int dual) {
  int kk = (int)(d % 32);
  long r = d / 32;
  int nn = (int)(r % npad);
  r /= npad;
  int c_chunk = (int)(r % kc32);
  int tap = (int)(r / kc32);
  int cc = c_chunk * 32 + kk;
  if (dual) {                                    // 16 input channels: chunk = tap pair, [tap 2c: 16 ch | tap 2c+1: 16 ch]
    tap = 2 * tap + (kk >> 4);
    cc = kk & 15;
  }
  int ty = tap / kw, tx = tap % kw;
  const float v = (tap < kh * kw) ? pack_value(src, mode, phase, kh, kw, cin, n, nn, cc, ty, tx) : 0.f;
  // exact split by truncation (same as the activations' in the kernel): hi + mid + lo == v
  const unsigned hb = __float_as_uint(v);
  const float r1 = v - __uint_as_float(hb & 0xFFFF0000u);
  const unsigned mb = __float_as_uint(r1);
  const unsigned lb = __float_as_uint(r1 - __uint_as_float(mb & 0xFFFF0000u));
  const size_t row = (size_t)(d / 32) * 96;                                  // 96 bf16 = 192 B per (chunk, n) row
  const int g = kk >> 3, e = kk & 7;
  dst[row + (0 * 4 + g) * 8 + e] = (unsigned short)(hb >> 16);
  dst[row + (1 * 4 + g) * 8 + e] = (unsigned short)(mb >> 16);
  dst[row + (2 * 4 + g) * 8 + e] = (unsigned short)(lb >> 16);
}

__global__ void pack_weights_bf3_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int mode,
                                        int phase, int kh, int kw, int cin, int n, int npad, int kc32, long total, int dual) {
  long d = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= total) return;
  pack_bf3_element(d, src, dst, mode, phase, kh, kw, cin, n, npad, kc32, dual);
}

// fp16x2 (MODE 3): per output channel n the power of two 2^s_n that maps max |w[n, :]| into [2^14, 2^15); out[n] = 2^-s_n
// (1 for an all-zero channel).  One block per channel.
__global__ void wscale_f16x2_kernel(const float* __restrict__ src, float* __restrict__ out, int mode, int phase, int kh, int kw,
                                    int cin, int n, int npad) {
  const int nn = blockIdx.x;
  float m = 0.f;
  for (int i = threadIdx.x; i < kh * kw * cin; i += blockDim.x) {
    const int tap = i / cin, cc = i - tap * cin;
    m = fmaxf(m, fabsf(pack_value(src, mode, phase, kh, kw, cin, n, nn, cc, tap / kw, tap % kw)));
  }
  __shared__ float red[256];
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    m = red[0];
    const int e = (int)((__float_as_uint(m) >> 23) & 0xFFu) - 127;
    int sh = (m > 0.f && e > -127 && e < 128) ? 14 - e : 0;
    sh = sh > 126 ? 126 : (sh < -126 ? -126 : sh);
    out[nn] = __uint_as_float((unsigned)(127 - sh) << 23);
  }
  (void)npad;
}

// fp16x2 layout: [tap][32-channel chunk][Npad][8 chunks][8 fp16]; chunk (p*4 + g) holds plane p (h / l) of channels
// 8g..8g+7; w 2^s_n = h + l up to 2^-22 |w|.  (dual: as in the bf16x3 layout)
__global__ void pack_weights_f16x2_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, const float* __restrict__ wsc,
                                          int mode, int phase, int kh, int kw, int cin, int n, int npad, int kc32, long total, int dual) {
  long d = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= total) return;
  int kk = (int)(d % 32);
  long r = d / 32;
  int nn = (int)(r % npad);
  r /= npad;
  int c_chunk = (int)(r % kc32);
  int tap = (int)(r / kc32);
  int cc = c_chunk * 32 + kk;
  if (dual) {
    tap = 2 * tap + (kk >> 4);
    cc = kk & 15;
  }
  int ty = tap / kw, tx = tap % kw;
  const float v = (tap < kh * kw) ? pack_value(src, mode, phase, kh, kw, cin, n, nn, cc, ty, tx) : 0.f;
  const float vs = v / wsc[nn];                      // 2^-s_n is a power of two: the division is exact
  const _Float16 h = (_Float16)vs;
  const _Float16 l = (_Float16)(vs - (float)h);
  const size_t row = (size_t)(d / 32) * 64;          // 64 fp16 = 128 B per (chunk, n) row
  const int g = kk >> 3, e = kk & 7;
  dst[row + (0 * 4 + g) * 8 + e] = __builtin_bit_cast(unsigned short, h);
  dst[row + (1 * 4 + g) * 8 + e] = __builtin_bit_cast(unsigned short, l);
}

// max |x| over an NHWC window, folded into *cell (the float's bits; integer atomicMax).  float4 loads, grid-stride.
struct AbsmaxArgs { const float* ptr[VAM_MAX_SEG]; int C[VAM_MAX_SEG]; int ld[VAM_MAX_SEG]; int n_seg; long n_pix; int* cell; };
__global__ __launch_bounds__(256) void absmax_kernel(const AbsmaxArgs a) {
  float m = 0.f;
  for (int s = 0; s < a.n_seg; ++s) {
    const int c4 = a.C[s] >> 2;
    const long total = a.n_pix * c4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
      const long pix = i / c4;
      const int c = (int)(i - pix * c4);
      const float4 v = *reinterpret_cast<const float4*>(a.ptr[s] + pix * a.ld[s] + 4 * c);
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0.f && __float_as_int(m) > __hip_atomic_load(a.cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(a.cell, __float_as_int(m));
}

// bf16 storage mode: [tap][32-channel chunk][Npad][32 bf16] = 64 B per row, each weight rounded to nearest-even bf16
__global__ void pack_weights_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int mode,
                                         int phase, int kh, int kw, int cin, int n, int npad, int kc32, long total) {
  long d = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= total) return;
  int kk = (int)(d % 32);
  long r = d / 32;
  int nn = (int)(r % npad);
  r /= npad;
  int c_chunk = (int)(r % kc32);
  int tap = (int)(r / kc32);
  int ty = tap / kw, tx = tap % kw;
  const float v = pack_value(src, mode, phase, kh, kw, cin, n, nn, c_chunk * 32 + kk, ty, tx);
  const __bf16 h = (__bf16)v;
  dst[d] = __builtin_bit_cast(unsigned short, h);
}

__device__ __forceinline__ void pack_bias_element(int i, const float* __restrict__ src, float* __restrict__ dst, int mode, int n) {
  float v;
  if (mode == VAM_PACK_PS2) {
    int cq = n / 4;
    int ph = i / cq, c = i - ph * cq;
    v = src[c * 4 + ph];
  } else if (mode == VAM_PACK_DECONV5S2) {
    int cout = n / 4;
    v = src[i % cout];
  } else if (mode == VAM_PACK_GDN) {
    // beta: NonNegativeParametrizer(minimum=1e-6): bound = sqrt(1e-6 + 2^-36) rounded to fp32
    const float bound = (float)1.0000072759311445e-03;
    const float ped = 1.4551915228366852e-11f;
    float b = fmaxf(src[i], bound);
    v = b * b - ped;
  } else {
    v = src[i];
  }
  dst[i] = v;
}

__global__ void pack_bias_kernel(const float* __restrict__ src, float* __restrict__ dst, int mode, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pack_bias_element(i, src, dst, mode, n);
}

// Many small repacks as one launch (training: every trained layer is repacked after every optimiser step — 1,250 launches
// of ~4.5 us per first_train step when issued one by one).  blockIdx.y = job; a job's blocks stride over its elements.
struct PackJobD {
  const float* src;
  void* dst;
  long total;
  int kind, mode, phase, kh, kw, cin, n, npad, kc32, dual;
};
struct PackGroupArgs {
  PackJobD j[VAM_MAX_PACK_GROUP];
};
__global__ __launch_bounds__(256) void pack_group_kernel(const PackGroupArgs a) {
  const PackJobD& j = a.j[blockIdx.y];
  for (long d = (long)blockIdx.x * 256 + threadIdx.x; d < j.total; d += (long)gridDim.x * 256) {
    if (j.kind == 0) pack_bf3_element(d, j.src, reinterpret_cast<unsigned short*>(j.dst), j.mode, j.phase, j.kh, j.kw, j.cin, j.n, j.npad, j.kc32, j.dual);
    else pack_bias_element((int)d, j.src, reinterpret_cast<float*>(j.dst), j.mode, j.n);
  }
}

// The argument rules every weight-pack entry point shares; `who` prefixes the two generic messages (vam_pack_group has
// checked those two already, under its job-numbered texts).  gdn_rules: the bf16-storage pack does not apply the GDN rule.
static int check_pack_args(const char* who, int mode, int phase, int kh, int kw, int cin, int n, bool gdn_rules) {
  VAM_REQUIRE(kh > 0 && kw > 0 && cin > 0 && n > 0, "%s: bad arguments", who);
  VAM_REQUIRE(mode >= VAM_PACK_CONV && mode <= VAM_PACK_GDN_T, "%s: bad mode %d", who, mode);
  if (mode == VAM_PACK_PS2) VAM_REQUIRE(n % 4 == 0, "PS2 pack needs N %% 4 == 0");
  if (mode == VAM_PACK_DECONV5S2 && phase < 0) VAM_REQUIRE(n % 4 == 0 && kh == 3 && kw == 3, "merged deconv pack needs 3x3, N=4*Cout");
  if (mode == VAM_PACK_DECONV5S2 && phase >= 0)
    VAM_REQUIRE(phase < 4 && kh == ((phase >> 1) ? 2 : 3) && kw == ((phase & 1) ? 2 : 3), "deconv phase %d needs kh/kw = 3|2", phase);
  if (gdn_rules && (mode == VAM_PACK_GDN || mode == VAM_PACK_GDN_T)) VAM_REQUIRE(kh == 1 && kw == 1 && cin == n, "GDN pack is 1x1 and square");
  return VAM_OK;
}

}  // namespace vam

using namespace vam;

extern "C" {

size_t vam_conv_wpack_floats(int kh, int kw, int cin, int n) {
  const PackGeom g = pack_geom(kh, kw, cin, n);
  if (conv_mode() == 1) return (size_t)kh * kw * g.kc32 * g.npad * 48;   // 96 bf16 per (n, 32-channel chunk)
  if (conv_mode() == 3) return (size_t)kh * kw * g.kc32 * g.npad * 32 + g.npad;   // 64 fp16 per row, then 2^-s_n per channel
  int bk = PK;
  int kc = (cin + bk - 1) / bk;
  return (size_t)kh * kw * kc * g.npad * bk;
}

int vam_pack_conv_weights(const float* src, float* dst, int mode, int phase, int kh, int kw, int cin, int n,
                          void* stream) {
  VAM_REQUIRE(src && dst, "vam_pack_conv_weights: bad arguments");
  if (int rc = check_pack_args("vam_pack_conv_weights", mode, phase, kh, kw, cin, n, true)) return rc;
  const PackGeom g = pack_geom(kh, kw, cin, n);
  if (conv_mode() == 3) {
    float* wsc = dst + (size_t)kh * kw * g.kc32 * g.npad * 32;
    hipLaunchKernelGGL(wscale_f16x2_kernel, dim3(g.npad), dim3(256), 0, (hipStream_t)stream, src, wsc, mode, phase, kh, kw, cin, n, g.npad);
    hipLaunchKernelGGL(pack_weights_f16x2_kernel, dim3(cdiv(g.total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       reinterpret_cast<unsigned short*>(dst), wsc, mode, phase, kh, kw, cin, n, g.npad, g.kc32, g.total, g.dual);
    return check_launch("pack_weights_f16x2_kernel");
  }
  if (conv_mode() == 1) {      // 16-channel inputs: two taps per 32-channel chunk (g.dual; kernel: VAM_CONVI_DUAL)
    hipLaunchKernelGGL(pack_weights_bf3_kernel, dim3(cdiv(g.total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       reinterpret_cast<unsigned short*>(dst), mode, phase, kh, kw, cin, n, g.npad, g.kc32, g.total, g.dual);
    return check_launch("pack_weights_bf3_kernel");
  }
  int bk = PK;
  int kc = (cin + bk - 1) / bk;
  long total = (long)kh * kw * kc * g.npad * bk;
  hipLaunchKernelGGL(pack_weights_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, mode,
                     phase, kh, kw, cin, n, g.npad, bk, kc, total);
  return check_launch("pack_weights_kernel");
}

size_t vam_conv_wpack_bf16_bytes(int kh, int kw, int cin, int n) {
  return (size_t)kh * kw * ((cin + 31) / 32) * ((n + 31) / 32 * 32) * 64;
}

int vam_pack_conv_weights_bf16(const float* src, void* dst, int mode, int phase, int kh, int kw, int cin, int n, void* stream) {
  VAM_REQUIRE(src && dst, "vam_pack_conv_weights_bf16: bad arguments");
  if (int rc = check_pack_args("vam_pack_conv_weights_bf16", mode, phase, kh, kw, cin, n, false)) return rc;
  const int npad = (n + 31) / 32 * 32, kc32 = (cin + 31) / 32;
  const long total = (long)kh * kw * kc32 * npad * 32;
  hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     reinterpret_cast<unsigned short*>(dst), mode, phase, kh, kw, cin, n, npad, kc32, total);
  return check_launch("pack_weights_bf16_kernel");
}

int vam_pack_bias(const float* src, float* dst, int mode, int n, void* stream) {
  VAM_REQUIRE(src && dst && n > 0, "vam_pack_bias: bad arguments");
  hipLaunchKernelGGL(pack_bias_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, mode, n);
  return check_launch("pack_bias_kernel");
}

int vam_pack_group(const vam_pack_job* jobs, int n_jobs, void* stream) {
  VAM_REQUIRE(jobs && n_jobs >= 1, "vam_pack_group: no jobs");
  if (conv_mode() != 1) {                      // other arithmetic modes: one by one through the ordinary entry points
    for (int i = 0; i < n_jobs; ++i) {
      const vam_pack_job& q = jobs[i];
      int rc = q.bias ? vam_pack_bias(q.src, (float*)q.dst, q.mode, q.n, stream)
                      : vam_pack_conv_weights(q.src, (float*)q.dst, q.mode, q.phase, q.kh, q.kw, q.cin, q.n, stream);
      if (rc != VAM_OK) return rc;
    }
    return VAM_OK;
  }
  for (int i0 = 0; i0 < n_jobs; i0 += VAM_MAX_PACK_GROUP) {
    const int cnt = n_jobs - i0 < VAM_MAX_PACK_GROUP ? n_jobs - i0 : VAM_MAX_PACK_GROUP;
    PackGroupArgs a;
    long max_total = 0;
    for (int i = 0; i < cnt; ++i) {
      const vam_pack_job& q = jobs[i0 + i];
      PackJobD& j = a.j[i];
      VAM_REQUIRE(q.src && q.dst && q.n > 0, "vam_pack_group: job %d: bad arguments", i0 + i);
      j.src = q.src; j.dst = q.dst; j.mode = q.mode; j.phase = q.phase; j.kh = q.kh; j.kw = q.kw; j.cin = q.cin; j.n = q.n;
      if (q.bias) {
        j.kind = 1; j.total = q.n; j.npad = j.kc32 = j.dual = 0;
      } else {
        VAM_REQUIRE(q.kh > 0 && q.kw > 0 && q.cin > 0 && q.mode >= VAM_PACK_CONV && q.mode <= VAM_PACK_GDN_T, "vam_pack_group: job %d: bad geometry / mode", i0 + i);
        if (int rc = check_pack_args("vam_pack_group", q.mode, q.phase, q.kh, q.kw, q.cin, q.n, true)) return rc;
        const PackGeom g = pack_geom(q.kh, q.kw, q.cin, q.n);
        j.kind = 0; j.npad = g.npad; j.kc32 = g.kc32; j.dual = g.dual; j.total = g.total;
      }
      if (j.total > max_total) max_total = j.total;
    }
    long bx = cdiv(max_total, 256 * 4);          // ~4 elements per thread of the largest job
    if (bx > 512) bx = 512;
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(pack_group_kernel, dim3((unsigned)bx, (unsigned)cnt), dim3(256), 0, (hipStream_t)stream, a);
    if (int rc = check_launch("pack_group_kernel")) return rc;
  }
  return VAM_OK;
}

int vam_absmax(const vam_seg* segs, int n_seg, long n_pix, int32_t* cell, void* stream) {
  VAM_REQUIRE(segs && n_seg >= 1 && n_seg <= VAM_MAX_SEG && n_pix > 0 && cell, "vam_absmax: bad arguments");
  AbsmaxArgs a;
  double work = 0;
  for (int s = 0; s < n_seg; ++s) {
    VAM_REQUIRE(segs[s].ptr && segs[s].C > 0 && segs[s].C % 4 == 0 && segs[s].ld % 4 == 0 && (((uintptr_t)segs[s].ptr) & 15) == 0,
                "vam_absmax: segment %d needs C, ld multiples of 4 and a 16-byte aligned pointer", s);
    a.ptr[s] = segs[s].ptr; a.C[s] = segs[s].C; a.ld[s] = segs[s].ld;
    work += (double)n_pix * segs[s].C / 4;
  }
  a.n_seg = n_seg; a.n_pix = n_pix; a.cell = cell;
  long blocks = (long)(work / 256 / 8) + 1;            // ~8 float4 per thread
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("absmax_kernel");
}

}  // extern "C"
