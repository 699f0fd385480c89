// HBM-bound element-wise kernels outside the entropy models (csrc/entropy.hip): model-edge layout changes, the
// pixel-shuffle / zero-insertion layouts of the training backward, and a few tiny helpers.  The channel-window ones are
// coalesced 16-byte-per-lane streams over NHWC windows (window.h), grid-stride.
//
// This file is compiled with -ffp-contract=off, like every file of the library.
#include "common.h"
#include "window.h"

namespace vam {

constexpr int GRID_CAP = 2048;
constexpr int GRID_CAP_LAYOUT = 4096;     // ps2_unshuffle, upsample2_zero

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

// dst[b, y, x, c*4 + i*2 + j] = src[b, 2y+i, 2x+j, c]      (gradient of PixelShuffle(2), layers/layers.py:82-86: pixel
// un-shuffle of the output gradient into the conv's channel order; H, W = extent of dst)
__global__ void ps2_unshuffle_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst, int B, int H,
                                     int W, int Cq) {
  const long total = (long)B * H * W * Cq * 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i % (4 * Cq));
    long p = i / (4 * Cq);
    const int x = (int)(p % W);
    p /= W;
    const int y = (int)(p % H);
    const int b = (int)(p / H);
    const int c = n >> 2, ph = n & 3;
    const long sp = ((long)b * 2 * H + 2 * y + (ph >> 1)) * (2 * W) + 2 * x + (ph & 1);
    dst[(((long)b * H + y) * W + x) * ld_dst + n] = src[sp * ld_src + c];
  }
}

// dst[b, 2y, 2x, :] = src[b, y, x, :], zero elsewhere      (H, W = extent of src; C % 4 == 0).  The data gradient of a 3x3
// stride-2 convolution (h_a, models/builder.py:72-82) is the stride-1 data-gradient convolution (VAM_PACK_CONV_DGRAD) of
// the output gradient with zeros between its samples.
__global__ void upsample2_zero_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst, int B, int H,
                                      int W, int C4) {
  const long total = (long)B * 2 * H * 2 * W * C4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, C4, p, c);
    const long pix = p;
    const int x = (int)(p % (2 * W));
    p /= 2 * W;
    const int y = (int)(p % (2 * H));
    const int b = (int)(p / (2 * H));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(x & 1) && !(y & 1)) v = ld4(src, ((long)b * H + (y >> 1)) * W + (x >> 1), ld_src, c);
    *reinterpret_cast<float4*>(dst + pix * ld_dst + c) = v;
  }
}

// ------------------------------------------------------------------ two-operand streams
__global__ void add_kernel(const float* __restrict__ a, int ld_a, const float* __restrict__ b, int ld_b,
                           float* __restrict__ out, int ld_out, long n_vec, int C4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, C4, p, c);
    float x[4], y[4], o[4];
    ld4(a, p, ld_a, c, x);
    ld4(b, p, ld_b, c, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = x[k] + y[k];
    st4(out, p, ld_out, c, o);
  }
}

__global__ void mul_kernel(const float* __restrict__ a, int ld_a, const float* __restrict__ b, int ld_b,
                           float* __restrict__ out, int ld_out, long n_vec, int C4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, C4, p, c);
    float x[4], y[4], o[4];
    ld4(a, p, ld_a, c, x);
    ld4(b, p, ld_b, c, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = x[k] * y[k];
    st4(out, p, ld_out, c, o);
  }
}

__global__ void leaky_bwd_kernel(const float* __restrict__ act, int ld_a, const float* __restrict__ dy, int ld_dy,
                                 float* __restrict__ dx, int ld_dx, long n_vec, int C4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, C4, p, c);
    float a[4], g[4], o[4];
    ld4(act, p, ld_a, c, a);
    ld4(dy, p, ld_dy, c, g);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = g[k] * (a[k] > 0.f ? 1.f : 0.01f);
    st4(dx, p, ld_dx, c, o);
  }
}

__global__ void dequantize_kernel(const int32_t* __restrict__ sym, int ld_sym, const float* __restrict__ mu, int ld_mu,
                                  float* __restrict__ out, int ld_out, long n_vec, int C4) {
  // EntropyModel.dequantize (entropy_models.py:161-168): float(symbols) + means
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (long)gridDim.x * blockDim.x) {
    long p;
    int c;
    vec_at(i, C4, p, c);
    int q[4];
    float m[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    ldi4(sym, p, ld_sym, c, q);
    if (mu) ld4(mu, p, ld_mu, c, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (float)q[k] + m[k];
    st4(out, p, ld_out, c, o);
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
  hipLaunchKernelGGL(s2d_input_kernel, dim3(stream_grid(total, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, x, out, B, H, W);
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

int vam_ps2_unshuffle(const float* src, int ld_src, float* dst, int ld_dst, int B, int H, int W, int Cq, void* stream) {
  VAM_REQUIRE(src && dst && B > 0 && H > 0 && W > 0 && Cq > 0 && ld_src >= Cq && ld_dst >= 4 * Cq, "vam_ps2_unshuffle: bad arguments");
  const long total = (long)B * H * W * Cq * 4;
  hipLaunchKernelGGL(ps2_unshuffle_kernel, dim3(stream_grid(total, 256, GRID_CAP_LAYOUT)), dim3(256), 0, (hipStream_t)stream, src,
                     ld_src, dst, ld_dst, B, H, W, Cq);
  return check_launch("ps2_unshuffle_kernel");
}

int vam_upsample2_zero(const float* src, int ld_src, float* dst, int ld_dst, int B, int H, int W, int C, void* stream) {
  VAM_REQUIRE(src && dst && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ld_src >= C && ld_dst >= C, "vam_upsample2_zero: bad arguments");
  VAM_CHECK_WINDOWS("vam_upsample2_zero", C, {{"src", src, ld_src, 0, true, 16, false}, {"dst", dst, ld_dst, 0, true, 16, false}},
                    {"bad arguments", "alignment", "alignment"});
  const long total = (long)B * 2 * H * 2 * W * (C / 4);
  hipLaunchKernelGGL(upsample2_zero_kernel, dim3(stream_grid(total, 256, GRID_CAP_LAYOUT)), dim3(256), 0, (hipStream_t)stream, src,
                     ld_src, dst, ld_dst, B, H, W, C / 4);
  return check_launch("upsample2_zero_kernel");
}

// out = a (op) b over one window each: the argument rules of vam_add, vam_mul and vam_leaky_bwd
static int check_binary(const char* who, const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, long n_pix,
                        int C, const char* align_words) {
  VAM_REQUIRE(n_pix > 0 && C > 0 && C % 4 == 0, "%s: bad arguments", who);
  return check_windows(who, C, {{"a", a, ld_a, 0, true, 16, false}, {"b", b, ld_b, 0, true, 16, false}, {"out", out, ld_out, 0, true, 16, false}},
                       {"bad arguments", align_words, "bad arguments"});
}

int vam_add(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, long n_pix, int C,
            void* stream) {
  if (int rc = check_binary("vam_add", a, ld_a, b, ld_b, out, ld_out, n_pix, C, "alignment")) return rc;
  long n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 12.0 * (double)n_pix * C);
  hipLaunchKernelGGL(add_kernel, dim3(stream_grid(n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, a, ld_a, b, ld_b,
                     out, ld_out, n_vec, C / 4);
  return check_launch("add_kernel");
}

int vam_mul(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, long n_pix, int C, void* stream) {
  if (int rc = check_binary("vam_mul", a, ld_a, b, ld_b, out, ld_out, n_pix, C, "bad arguments")) return rc;
  long n_vec = n_pix * (C / 4);
  hipLaunchKernelGGL(mul_kernel, dim3(stream_grid(n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, a, ld_a, b, ld_b, out,
                     ld_out, n_vec, C / 4);
  return check_launch("mul_kernel");
}

int vam_leaky_bwd(const float* act, int ld_a, const float* dy, int ld_dy, float* dx, int ld_dx, long n_pix, int C,
                  void* stream) {
  if (int rc = check_binary("vam_leaky_bwd", act, ld_a, dy, ld_dy, dx, ld_dx, n_pix, C, "bad arguments")) return rc;
  long n_vec = n_pix * (C / 4);
  hipLaunchKernelGGL(leaky_bwd_kernel, dim3(stream_grid(n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, act, ld_a, dy,
                     ld_dy, dx, ld_dx, n_vec, C / 4);
  return check_launch("leaky_bwd_kernel");
}

int vam_dequantize(const int32_t* sym, int ld_sym, const float* mu, int ld_mu, float* out, int ld_out, long n_pix, int C,
                   void* stream) {
  VAM_REQUIRE(n_pix > 0 && C > 0 && C % 4 == 0, "vam_dequantize: bad arguments");
  VAM_CHECK_WINDOWS("vam_dequantize", C,
                    {{"sym", sym, ld_sym, 0, true, 16, false}, {"mu", mu, ld_mu, 0, false, 16, false}, {"out", out, ld_out, 0, true, 16, false}},
                    {"bad arguments", "alignment", "bad arguments"});
  long n_vec = n_pix * (C / 4);
  ProfScope ps(VAM_FAM_TAIL, (hipStream_t)stream, 0, 12.0 * (double)n_pix * C);
  hipLaunchKernelGGL(dequantize_kernel, dim3(stream_grid(n_vec, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, sym, ld_sym, mu,
                     ld_mu, out, ld_out, n_vec, C / 4);
  return check_launch("dequantize_kernel");
}

int vam_memset_zero(void* ptr, size_t bytes, void* stream) {
  // Always a KERNEL, never hipMemsetAsync: every node of a captured plan is then a kernel node, ordered like every other
  // launch of the plan (round 2 saw single elements of a 392-float table left un-cleared behind a memset NODE under
  // graph replay; scratch/probe/memset_graph.hip is the stand-alone probe of that pattern).
  VAM_REQUIRE(ptr && bytes > 0, "vam_memset_zero: bad arguments");
  VAM_REQUIRE(aligned(ptr, 4) && (bytes & 3) == 0, "vam_memset_zero: pointer and size must be multiples of 4 bytes");
  const long n = (long)(bytes >> 2);
  hipLaunchKernelGGL(zero_words_kernel, dim3(stream_grid(n, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, (unsigned*)ptr, n);
  return check_launch("zero_words_kernel");
}

int vam_sqdiff_sum(const float* a, const float* b, long n, double* acc, void* stream) {
  VAM_REQUIRE(a && b && acc && n > 0, "vam_sqdiff_sum: bad arguments");
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 8.0 * (double)n);
  hipLaunchKernelGGL(sqdiff_kernel, dim3(stream_grid(n, 256, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, a, b, n, acc);
  return check_launch("sqdiff_kernel");
}

}  // extern "C"
