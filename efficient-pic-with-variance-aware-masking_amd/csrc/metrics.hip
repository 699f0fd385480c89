// MS-SSIM building blocks (reference utility/functions.py:176-177 -> pytorch_msssim.ms_ssim, used by the real-codec
// evaluation training/step.py:323-326): one SSIM level (11x11 Gaussian window, "valid" positions) and the 2x2 average
// pooling between levels.  A metric, not the hot path: a direct 121-tap window per output position out of L2 is
// ~0.1 ms for a Kodak image; sums are accumulated in double (wave-aggregated atomics, like the rate sums).
#include "common.h"

namespace vam {

__global__ __launch_bounds__(256) void ssim_level_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                         int W, const float* __restrict__ win, float c1, float c2,
                                                         double* __restrict__ ssim_sum, double* __restrict__ cs_sum) {
  __shared__ float g[11];
  __shared__ double red[2][4];
  if (threadIdx.x < 11) g[threadIdx.x] = win[threadIdx.x];
  __syncthreads();
  const int plane = blockIdx.y;
  const int Ho = H - 10, Wo = W - 10;
  const float* xp = x + (size_t)plane * H * W;
  const float* yp = y + (size_t)plane * H * W;
  double s_ssim = 0.0, s_cs = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)Ho * Wo; i += (long)gridDim.x * blockDim.x) {
    const int oy = (int)(i / Wo), ox = (int)(i - (long)oy * Wo);
    // separable order of the reference implementation: filter along H first, then along W
    float mx = 0.f, my = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
    for (int dx = 0; dx < 11; ++dx) {
      float cx = 0.f, cy = 0.f, cxx = 0.f, cyy = 0.f, cxy = 0.f;
      for (int dy = 0; dy < 11; ++dy) {
        const float a = xp[(size_t)(oy + dy) * W + ox + dx], b = yp[(size_t)(oy + dy) * W + ox + dx];
        const float w = g[dy];
        cx += w * a; cy += w * b; cxx += w * (a * a); cyy += w * (b * b); cxy += w * (a * b);
      }
      const float w = g[dx];
      mx += w * cx; my += w * cy; sxx += w * cxx; syy += w * cyy; sxy += w * cxy;
    }
    const float vx = sxx - mx * mx, vy = syy - my * my, cov = sxy - mx * my;
    const float cs = (2.f * cov + c2) / (vx + vy + c2);
    const float ss = (2.f * mx * my + c1) / (mx * mx + my * my + c1) * cs;
    s_ssim += (double)ss;
    s_cs += (double)cs;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s_ssim += __shfl_down(s_ssim, o);
    s_cs += __shfl_down(s_cs, o);
  }
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wid] = s_ssim; red[1][wid] = s_cs; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&ssim_sum[plane], red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    atomicAdd(&cs_sum[plane], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

// F.avg_pool2d(kernel 2, stride 2, padding (ph, pw), zeros counted in the mean)
__global__ void avgpool2_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int Ho, int Wo, int ph,
                                int pw, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % Wo);
    long r = i / Wo;
    const int oy = (int)(r % Ho);
    const long plane = r / Ho;
    const float* xp = x + plane * H * W;
    float s = 0.f;
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int iy = 2 * oy - ph + dy, ix = 2 * ox - pw + dx;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) s += xp[(size_t)iy * W + ix];
      }
    out[i] = s * 0.25f;
  }
}

// Per (level, image) sums of squared differences of a rate sweep's reconstructions (vam_sqdiff_sum_levels): x is
// [B, n] (n = 3 H W floats per image), xhat holds the levels as consecutive image blocks [L * B, n].  Block row
// blockIdx.y = image b; each thread reads its x elements once and keeps one fp64 partial per level in registers, then
// one wave-reduced atomic per (wave, level) into out[l * B + b].  Same per-element arithmetic as vam_sqdiff_sum
// (fp32 difference, fp64 square and sum).
constexpr int SQD_MAX_LEVELS = 16;

__global__ __launch_bounds__(256) void sqdiff_levels_kernel(const float* __restrict__ x, const float* __restrict__ xhat, long n,
                                                            int B, int n_levels, double* __restrict__ out) {
  const int b = blockIdx.y;
  const float* xb = x + (long)b * n;
  double acc[SQD_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < SQD_MAX_LEVELS; ++l) acc[l] = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xv = xb[i];
#pragma unroll
    for (int l = 0; l < SQD_MAX_LEVELS; ++l) {
      if (l < n_levels) {
        float d = xv - xhat[((long)l * B + b) * n + i];
        acc[l] += (double)d * (double)d;
      }
    }
  }
#pragma unroll
  for (int l = 0; l < SQD_MAX_LEVELS; ++l) {
    if (l < n_levels) {
      double s = acc[l];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
      if ((threadIdx.x & 63) == 0) atomicAdd(out + (long)l * B + b, s);
    }
  }
}

}  // namespace vam

using namespace vam;

extern "C" {

int vam_ssim_level(const float* x, const float* y, int planes, int H, int W, const float* win11, float c1, float c2,
                   double* ssim_sum, double* cs_sum, void* stream) {
  VAM_REQUIRE(x && y && win11 && ssim_sum && cs_sum && planes > 0, "vam_ssim_level: bad arguments");
  VAM_REQUIRE(H > 10 && W > 10, "vam_ssim_level: plane %dx%d smaller than the 11x11 window", H, W);
  const long n = (long)(H - 10) * (W - 10);
  unsigned gx = (unsigned)((n + 255) / 256);
  if (gx > 512) gx = 512;
  hipLaunchKernelGGL(ssim_level_kernel, dim3(gx, planes), dim3(256), 0, (hipStream_t)stream, x, y, H, W, win11, c1, c2,
                     ssim_sum, cs_sum);
  return check_launch("ssim_level_kernel");
}

int vam_avgpool2(const float* x, float* out, int planes, int H, int W, int pad_h, int pad_w, void* stream) {
  VAM_REQUIRE(x && out && planes > 0 && H > 0 && W > 0 && pad_h >= 0 && pad_h <= 1 && pad_w >= 0 && pad_w <= 1, "vam_avgpool2: bad arguments");
  const int Ho = (H + 2 * pad_h - 2) / 2 + 1, Wo = (W + 2 * pad_w - 2) / 2 + 1;
  const long total = (long)planes * Ho * Wo;
  unsigned g = (unsigned)((total + 255) / 256);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(avgpool2_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, x, out, H, W, Ho, Wo, pad_h, pad_w, total);
  return check_launch("avgpool2_kernel");
}

int vam_sqdiff_sum_levels(const float* x, const float* xhat, int B, long n, int n_levels, double* out, void* stream) {
  // out[l * B + b] += sum_i (x[b, i] - xhat[l * B + b, i])^2 ; groups of SQD_MAX_LEVELS levels per launch
  VAM_REQUIRE(x && xhat && out && B > 0 && B <= 65535 && n > 0 && n_levels > 0, "vam_sqdiff_sum_levels: bad arguments");
  long per_img = (n + 255) / 256;
  unsigned gx = (unsigned)(per_img < 1 ? 1 : per_img);
  long cap = (2048 + B - 1) / B;                           // about 2048 blocks in all
  if (gx > (unsigned)(cap < 1 ? 1 : cap)) gx = (unsigned)(cap < 1 ? 1 : cap);
  for (int l0 = 0; l0 < n_levels; l0 += SQD_MAX_LEVELS) {
    int nl = n_levels - l0 < SQD_MAX_LEVELS ? n_levels - l0 : SQD_MAX_LEVELS;
    ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 4.0 * (double)B * n * (1 + nl));
    hipLaunchKernelGGL(sqdiff_levels_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, xhat + (long)l0 * B * n, n, B,
                       nl, out + (long)l0 * B);
    int rc = check_launch("sqdiff_levels_kernel");
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
