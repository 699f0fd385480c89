// Differentiable MS-SSIM distortion: the training loss beside the evaluation metric of metrics.hip.
// Function: oracle/msssim_oracle.py (pytorch_msssim 0.2.1's published algorithm) per plane = (image, channel):
//   11-tap Gaussian (sigma 1.5) applied separably at the "valid" positions, 5 levels, avg_pool2d(2, padding = size % 2,
//   zeros counted) between levels, V = prod_l relu(m_l)^w_l with m_l the mean cs map (levels 0-3) / ssim map (level 4).
//
//   forward   one launch per level: a workgroup stages a 42x42 tile of x and y in LDS (32x32 valid positions + the
//             10-pixel halo), filters along H, then along W (the oracle's order), forms cs / ssim, reduces in fp64 and
//             writes ONE partial per workgroup to a scratch buffer — no floating-point atomics.
//   combine   one launch: sums the partials in a fixed order, forms V per plane, the mean over channels per image and
//             the upstream factors dV/dm_l = w_l V / m_l.  A plane with any m_l <= 0 has V = 0 and factors exactly 0.
//   backward  one launch per level, coarse to fine, gradient with respect to y only: a workgroup owns 22x22 input
//             pixels, recomputes the moments at the 32x32 window positions that touch them from a 42x42 tile (20-pixel
//             halo), forms the three coefficient maps, correlates them with the transposed Gaussian (rows, then columns)
//             and adds the pooled gradient of the coarser level by gather (each pixel has exactly one parent).
//
// LDS: every pass maps consecutive lanes to consecutive columns of one tile row, so a half-wave's ds_read_b32 / ds_write_b32
// touches 32 consecutive dwords both in the pass along H (fixed column offset, row k) and in the pass along W (column
// c + k): neither pass is bank-conflicted, and no row padding is needed (the H pass walks the 42-wide tile linearly, so
// padding the stride would only introduce a gap).  53 KB (backward) and 42 KB (forward) per workgroup: three workgroups
// fit a CU's 160 KB.
#include "common.h"

namespace vam {

constexpr int MS_TAPS = 11;
constexpr int MS_HALO = MS_TAPS - 1;       // 10
constexpr int MS_P = 32;                   // window positions per tile side (forward outputs, backward coefficients)
constexpr int MS_I = MS_P + MS_HALO;       // 42: input tile side
constexpr int MS_Q = MS_P - MS_HALO;       // 22: input pixels whose gradient a backward tile owns, per side
constexpr int MS_THREADS = 256;
constexpr int MS_LEVELS = 5;

struct MsLevels {
  int H[MS_LEVELS], W[MS_LEVELS], tiles[MS_LEVELS];
  long off[MS_LEVELS];                     // first partial of the level, in doubles, for `planes` planes
};

static inline int ms_tiles(int H, int W) { return (int)(cdiv(H - MS_HALO, MS_P) * cdiv(W - MS_HALO, MS_P)); }

static inline void ms_levels(int planes, int H, int W, MsLevels& lv) {
  long off = 0;
  for (int l = 0; l < MS_LEVELS; ++l) {
    lv.H[l] = H; lv.W[l] = W; lv.tiles[l] = ms_tiles(H, W); lv.off[l] = off;
    off += (long)planes * lv.tiles[l];
    H = (H + 2 * (H % 2) - 2) / 2 + 1;
    W = (W + 2 * (W % 2) - 2) / 2 + 1;
  }
}

// Stage the 42x42 tile of x and y whose first pixel is (y0, x0); pixels outside the plane read as 0 (the window
// positions that would use them are outside the valid range and are masked by the caller).
__device__ __forceinline__ void ms_stage(const float* __restrict__ xp, const float* __restrict__ yp, int H, int W, int y0, int x0,
                                         float* __restrict__ sx, float* __restrict__ sy) {
  for (int i = threadIdx.x; i < MS_I * MS_I; i += MS_THREADS) {
    const int r = i / MS_I, c = i - r * MS_I;
    const int iy = y0 + r, ix = x0 + c;
    float a = 0.f, b = 0.f;
    if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
      a = xp[(size_t)iy * W + ix];
      b = yp[(size_t)iy * W + ix];
    }
    sx[i] = a;
    sy[i] = b;
  }
}

// Pass along H of the five moments x, y, x^2, y^2, xy: sm[m][r][c] = sum_k g[k] * v_m[r + k][c], 32 rows x 42 columns.
__device__ __forceinline__ void ms_moments_h(const float* __restrict__ sx, const float* __restrict__ sy, const float* g,
                                             float* __restrict__ sm) {
  for (int i = threadIdx.x; i < MS_P * MS_I; i += MS_THREADS) {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < MS_TAPS; ++k) {
      const float a = sx[i + k * MS_I], b = sy[i + k * MS_I], w = g[k];
      m0 = fmaf(w, a, m0); m1 = fmaf(w, b, m1); m2 = fmaf(w, a * a, m2); m3 = fmaf(w, b * b, m3); m4 = fmaf(w, a * b, m4);
    }
    sm[i] = m0; sm[MS_P * MS_I + i] = m1; sm[2 * MS_P * MS_I + i] = m2; sm[3 * MS_P * MS_I + i] = m3; sm[4 * MS_P * MS_I + i] = m4;
  }
}

// Pass along W at window position (r, c) of the tile: the five filtered moments.
__device__ __forceinline__ void ms_moments_w(const float* __restrict__ sm, const float* g, int r, int c, float& mx, float& my,
                                             float& sxx, float& syy, float& sxy) {
  mx = my = sxx = syy = sxy = 0.f;
  const float* p = sm + r * MS_I + c;
#pragma unroll
  for (int k = 0; k < MS_TAPS; ++k) {
    const float w = g[k];
    mx = fmaf(w, p[k], mx); my = fmaf(w, p[MS_P * MS_I + k], my); sxx = fmaf(w, p[2 * MS_P * MS_I + k], sxx);
    syy = fmaf(w, p[3 * MS_P * MS_I + k], syy); sxy = fmaf(w, p[4 * MS_P * MS_I + k], sxy);
  }
}

__global__ __launch_bounds__(MS_THREADS) void msssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                                int W, const float* __restrict__ win, float c1, float c2,
                                                                int last, double* __restrict__ partial) {
  __shared__ float sx[MS_I * MS_I], sy[MS_I * MS_I];
  __shared__ float sm[5 * MS_P * MS_I];
  __shared__ double red[MS_THREADS / 64];
  float g[MS_TAPS];
#pragma unroll
  for (int k = 0; k < MS_TAPS; ++k) g[k] = win[k];
  const int plane = blockIdx.z;
  const int oy0 = blockIdx.y * MS_P, ox0 = blockIdx.x * MS_P;
  const int Ho = H - MS_HALO, Wo = W - MS_HALO;
  ms_stage(x + (size_t)plane * H * W, y + (size_t)plane * H * W, H, W, oy0, ox0, sx, sy);
  __syncthreads();
  ms_moments_h(sx, sy, g, sm);
  __syncthreads();
  double acc = 0.0;
  for (int i = threadIdx.x; i < MS_P * MS_P; i += MS_THREADS) {
    const int r = i / MS_P, c = i - r * MS_P;
    float mx, my, sxx, syy, sxy;
    ms_moments_w(sm, g, r, c, mx, my, sxx, syy, sxy);
    const float vx = sxx - mx * mx, vy = syy - my * my, cov = sxy - mx * my;
    float v = (2.f * cov + c2) / (vx + vy + c2);
    if (last) v = (2.f * mx * my + c1) / (mx * mx + my * my + c1) * v;
    if (oy0 + r < Ho && ox0 + c < Wo) acc += (double)v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)plane * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One wave per image: lane-strided, fixed-order sums of the workgroup partials, then V, the mean over channels and the
// upstream factors.  means / dvdm are [5][planes].
__global__ __launch_bounds__(64) void msssim_combine_kernel(const double* __restrict__ partial, MsLevels lv, int planes, int C,
                                                            double* __restrict__ means, double* __restrict__ dvdm,
                                                            double* __restrict__ val, float* __restrict__ val32) {
  const double wts[MS_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  const int b = blockIdx.x;
  double img = 0.0;
  for (int ch = 0; ch < C; ++ch) {
    const int plane = b * C + ch;
    double m[MS_LEVELS];
    bool pos = true;
#pragma unroll
    for (int l = 0; l < MS_LEVELS; ++l) {
      const double* p = partial + lv.off[l] + (size_t)plane * lv.tiles[l];
      double s = 0.0;
      for (int t = threadIdx.x; t < lv.tiles[l]; t += 64) s += p[t];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
      s = __shfl(s, 0, 64);
      m[l] = s / ((double)(lv.H[l] - MS_HALO) * (double)(lv.W[l] - MS_HALO));
      pos = pos && m[l] > 0.0;
    }
    double V = 0.0;
    if (pos) {
      V = 1.0;
#pragma unroll
      for (int l = 0; l < MS_LEVELS; ++l) V *= pow(m[l], wts[l]);
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int l = 0; l < MS_LEVELS; ++l) {
        means[(size_t)l * planes + plane] = m[l];
        dvdm[(size_t)l * planes + plane] = pos ? wts[l] * V / m[l] : 0.0;
      }
    }
    img += V;
  }
  if (threadIdx.x == 0) {
    img /= (double)C;
    val[b] = img;
    val32[b] = (float)img;
  }
}

__global__ __launch_bounds__(MS_THREADS) void msssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int C,
                                                                int H, int W, const float* __restrict__ win, float c1, float c2,
                                                                int last, const double* __restrict__ dvdm,
                                                                const float* __restrict__ gout, const float* __restrict__ gc,
                                                                int Hc, int Wc, float* __restrict__ gy) {
  __shared__ float sx[MS_I * MS_I], sy[MS_I * MS_I];
  __shared__ float sm[5 * MS_P * MS_I];                 // the moments after the H pass; later the row-correlated maps
  __shared__ float sg[3 * MS_P * MS_P];                 // G_my, G_syy, G_sxy at the tile's 32x32 window positions
  float g[MS_TAPS];
#pragma unroll
  for (int k = 0; k < MS_TAPS; ++k) g[k] = win[k];
  const int plane = blockIdx.z;
  const int qy0 = blockIdx.y * MS_Q, qx0 = blockIdx.x * MS_Q;       // first owned pixel
  const int py0 = qy0 - MS_HALO, px0 = qx0 - MS_HALO;               // first window position = first staged pixel
  const int Ho = H - MS_HALO, Wo = W - MS_HALO;
  const float* xp = x + (size_t)plane * H * W;
  const float* yp = y + (size_t)plane * H * W;
  // a = upstream * dV/dm_l / N_l, one scalar per plane (the image's upstream gradient is shared by its C channels)
  const float a = (float)((double)gout[plane / C] / (double)C * dvdm[plane] / ((double)Ho * (double)Wo));
  ms_stage(xp, yp, H, W, py0, px0, sx, sy);
  __syncthreads();
  ms_moments_h(sx, sy, g, sm);
  __syncthreads();
  for (int i = threadIdx.x; i < MS_P * MS_P; i += MS_THREADS) {
    const int r = i / MS_P, c = i - r * MS_P;
    float gmy = 0.f, gsyy = 0.f, gsxy = 0.f;
    if (a != 0.f && (unsigned)(py0 + r) < (unsigned)Ho && (unsigned)(px0 + c) < (unsigned)Wo) {
      float mx, my, sxx, syy, sxy;
      ms_moments_w(sm, g, r, c, mx, my, sxx, syy, sxy);
      const float vx = sxx - mx * mx, vy = syy - my * my, cov = sxy - mx * my;
      const float A2 = 2.f * cov + c2, B2 = vx + vy + c2;
      float s = a, direct = 0.f;
      if (last) {
        const float A1 = 2.f * mx * my + c1, B1 = mx * mx + my * my + c1;
        s = a * (A1 / B1);
        direct = a * (A2 / B2) * (2.f * mx * B1 - 2.f * my * A1) / (B1 * B1);
      }
      gsxy = s * 2.f / B2;
      gsyy = -s * A2 / (B2 * B2);
      gmy = direct - 2.f * my * gsyy - mx * gsxy;
    }
    sg[i] = gmy; sg[MS_P * MS_P + i] = gsyy; sg[2 * MS_P * MS_P + i] = gsxy;
  }
  __syncthreads();
  // transposed Gaussian along H: st[m][qr][c] = sum_j sg[m][qr + j][c] * g[10 - j], 22 rows x 32 columns (sm is free now)
  float* st = sm;
  for (int i = threadIdx.x; i < MS_Q * MS_P; i += MS_THREADS) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int j = 0; j < MS_TAPS; ++j) {
      const float w = g[MS_HALO - j];
      t0 = fmaf(w, sg[i + j * MS_P], t0); t1 = fmaf(w, sg[MS_P * MS_P + i + j * MS_P], t1);
      t2 = fmaf(w, sg[2 * MS_P * MS_P + i + j * MS_P], t2);
    }
    st[i] = t0; st[MS_Q * MS_P + i] = t1; st[2 * MS_Q * MS_P + i] = t2;
  }
  __syncthreads();
  // along W, then g_y = F[G_my] + 2 y F[G_syy] + x F[G_sxy] + the pooled gradient of the coarser level
  const int ph = H & 1, pw = W & 1;
  for (int i = threadIdx.x; i < MS_Q * MS_P; i += MS_THREADS) {
    const int qr = i / MS_P, qc = i - qr * MS_P;
    const int iy = qy0 + qr, ix = qx0 + qc;
    if (qc >= MS_Q || iy >= H || ix >= W) continue;
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
#pragma unroll
    for (int j = 0; j < MS_TAPS; ++j) {
      const float w = g[MS_HALO - j];
      f0 = fmaf(w, st[i + j], f0); f1 = fmaf(w, st[MS_Q * MS_P + i + j], f1); f2 = fmaf(w, st[2 * MS_Q * MS_P + i + j], f2);
    }
    const float xv = sx[(qr + MS_HALO) * MS_I + qc + MS_HALO], yv = sy[(qr + MS_HALO) * MS_I + qc + MS_HALO];
    float out = f0 + 2.f * yv * f1 + xv * f2;
    if (gc) out += 0.25f * gc[((size_t)plane * Hc + ((iy + ph) >> 1)) * Wc + ((ix + pw) >> 1)];
    gy[(size_t)plane * H * W + (size_t)iy * W + ix] = out;
  }
}

// avg_pool2d(kernel 2, padding = size % 2, zeros counted) of x and y in one launch
__global__ __launch_bounds__(MS_THREADS) void msssim_pool2_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  float* __restrict__ xo, float* __restrict__ yo, int H, int W,
                                                                  int Ho, int Wo, long total) {
  const int ph = H & 1, pw = W & 1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % Wo);
    const long r = i / Wo;
    const int oy = (int)(r % Ho);
    const size_t base = (size_t)(r / Ho) * H * W;
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int iy = 2 * oy - ph + dy, ix = 2 * ox - pw + dx;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
          sa += x[base + (size_t)iy * W + ix];
          sb += y[base + (size_t)iy * W + ix];
        }
      }
    xo[i] = sa * 0.25f;
    yo[i] = sb * 0.25f;
  }
}

}  // namespace vam

using namespace vam;

extern "C" {

long vam_msssim_partial_doubles(int planes, int H, int W) {
  if (planes <= 0 || H <= MS_HALO * 16 || W <= MS_HALO * 16) return 0;
  MsLevels lv;
  ms_levels(planes, H, W, lv);
  return lv.off[MS_LEVELS - 1] + (long)planes * lv.tiles[MS_LEVELS - 1];
}

long vam_msssim_partial_offset(int planes, int H, int W, int level) {
  if (planes <= 0 || H <= MS_HALO * 16 || W <= MS_HALO * 16 || level < 0 || level >= MS_LEVELS) return -1;
  MsLevels lv;
  ms_levels(planes, H, W, lv);
  return lv.off[level];
}

int vam_msssim_fwd_level(const float* x, const float* y, int planes, int H, int W, const float* win11, float c1, float c2,
                         int last, double* partial, void* stream) {
  VAM_REQUIRE(x && y && win11 && partial && planes > 0 && planes <= 65535, "vam_msssim_fwd_level: bad arguments");
  VAM_REQUIRE(H > MS_HALO && W > MS_HALO, "vam_msssim_fwd_level: plane %dx%d smaller than the 11x11 window", H, W);
  const dim3 grid(cdiv(W - MS_HALO, MS_P), cdiv(H - MS_HALO, MS_P), planes);
  VAM_REQUIRE(grid.y <= 65535, "vam_msssim_fwd_level: plane too tall");
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 8.0 * (double)planes * H * W);
  hipLaunchKernelGGL(msssim_fwd_kernel, grid, dim3(MS_THREADS), 0, (hipStream_t)stream, x, y, H, W, win11, c1, c2, last, partial);
  return check_launch("msssim_fwd_kernel");
}

int vam_msssim_pool2(const float* x, const float* y, float* x_out, float* y_out, int planes, int H, int W, void* stream) {
  VAM_REQUIRE(x && y && x_out && y_out && planes > 0 && H > 0 && W > 0, "vam_msssim_pool2: bad arguments");
  const int Ho = (H + 2 * (H % 2) - 2) / 2 + 1, Wo = (W + 2 * (W % 2) - 2) / 2 + 1;
  const long total = (long)planes * Ho * Wo;
  unsigned g = cdiv(total, MS_THREADS);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(msssim_pool2_kernel, dim3(g), dim3(MS_THREADS), 0, (hipStream_t)stream, x, y, x_out, y_out, H, W, Ho, Wo, total);
  return check_launch("msssim_pool2_kernel");
}

int vam_msssim_combine(const double* partial, int B, int C, int H, int W, double* means, double* dvdm, double* val, float* val32,
                       void* stream) {
  VAM_REQUIRE(partial && means && dvdm && val && val32 && B > 0 && C > 0, "vam_msssim_combine: bad arguments");
  VAM_REQUIRE(H > MS_HALO * 16 && W > MS_HALO * 16, "vam_msssim_combine: %dx%d too small for 5 scales (smaller side must exceed 160)", H, W);
  MsLevels lv;
  ms_levels(B * C, H, W, lv);
  hipLaunchKernelGGL(msssim_combine_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, partial, lv, B * C, C, means, dvdm, val, val32);
  return check_launch("msssim_combine_kernel");
}

int vam_msssim_bwd_level(const float* x, const float* y, int B, int C, int H, int W, const float* win11, float c1, float c2, int last,
                         const double* dvdm, const float* gout, const float* g_coarse, float* g, void* stream) {
  VAM_REQUIRE(x && y && win11 && dvdm && gout && g && B > 0 && C > 0 && (long)B * C <= 65535, "vam_msssim_bwd_level: bad arguments");
  VAM_REQUIRE(H > MS_HALO && W > MS_HALO, "vam_msssim_bwd_level: plane %dx%d smaller than the 11x11 window", H, W);
  VAM_REQUIRE(!last || !g_coarse, "vam_msssim_bwd_level: the last level has no coarser gradient");
  const int Hc = (H + 2 * (H % 2) - 2) / 2 + 1, Wc = (W + 2 * (W % 2) - 2) / 2 + 1;
  const dim3 grid(cdiv(W, MS_Q), cdiv(H, MS_Q), B * C);
  VAM_REQUIRE(grid.y <= 65535, "vam_msssim_bwd_level: plane too tall");
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 12.0 * (double)B * C * H * W);
  hipLaunchKernelGGL(msssim_bwd_kernel, grid, dim3(MS_THREADS), 0, (hipStream_t)stream, x, y, C, H, W, win11, c1, c2, last, dvdm,
                     gout, g_coarse, Hc, Wc, g);
  return check_launch("msssim_bwd_kernel");
}

}  // extern "C"
