// Tiled pictures (vampic.tiled): cutting overlapping tiles out of a picture of any size and blending
// decoded tiles back into a window of it.
//
// Geometry (one definition for the host, these kernels and tests/tiled_ref.py): tiles of th x tw, overlap V with
// 2 V <= min(th, tw), strides Sy = th - V and Sx = tw - V, grid R = max(1, ceil((H - V) / Sy)) by C likewise; tile (r, c)
// covers rows [r Sy, r Sy + th) and columns [c Sx, c Sx + tw).  At most two tiles overlap along an axis.
//
//   tile_extract_kernel   tile pixel (y, x) = image[:, clamp(r Sy + y, 0, H - 1), clamp(c Sx + x, 0, W - 1)]: the edge is
//                         replicated.  One launch serves a list of (r, c); a thread moves four pixels of a row.
//   tile_blend_kernel     output-centric: a thread owns four consecutive pixels of one row of the window and all three
//                         channels.  Along an axis the pixel P lies in tile t1 = min(n - 1, P / S) at l1 = P - t1 S and, when
//                         t1 > 0 and l1 < V, in tile t1 - 1 too (the band): there t1 takes w_hi[l1] and t1 - 1 takes w_lo[l1]
//                         from the host's tables, elsewhere the one tile has weight 1.  The pixel is the sum, over its tiles in
//                         ascending r and within that ascending c, of (wy * wx) * v, every product and add one fp32
//                         operation (__fmul_rn / __fadd_rn never contract), starting from the first term: outside the bands
//                         it is the tile's value bit for bit.  No atomics, no division of floats, a fixed order.  This
//                         kernel, tile_refresh_kernel and tile_compose_kernel are the three modes of ONE skeleton,
//                         window_pixels<Mode>: thread layout, run decision, blend_run and store_pixels are written once.
//   tile_schedule_kernel  a picture-wide schedule, fp32 [L, H, W] at pixel resolution, brought down onto the latent grids of a
//                         list of tiles: out[i, k, a, b] = max over y, x in [0, 16) of
//                         maps[k, min(r Sy + 16 a + y, H - 1), min(c Sx + 16 b + x, W - 1)], the block maximum of
//                         evaluate.latent_quality_map composed with the extract kernel's edge replication.  One wave per
//                         output cell: lane l reads the four pixels 4 (l & 3) .. of row l >> 2 and the 64 partial results are
//                         reduced with wave-64 shuffles.  A NaN anywhere in the block gives NaN (fmaxf alone would drop it).
//   tile_refresh_kernel   the skeleton over a box of a persistent canvas: a pixel is computed and stored
//                         only when one of its tiles is marked in `dirty` [R][C]; the value is tile_blend_kernel's.  A pixel
//                         without a dirty tile is not written and its slots are not read.  The output has the canvas's
//                         pitch; wide stores need all four pixels written.
//   picture_halve_kernel  the next level of a resolution pyramid: fp32 [C, Hs, Ws] to [C, ceil(Hs / 2),
//                         ceil(Ws / 2)], out[c][y][x] = ((s[2y][2x] + s[2y][x1]) + (s[y1][2x] + s[y1][x1])) * 0.25f with
//                         y1 = min(2y + 1, Hs - 1), x1 = min(2x + 1, Ws - 1), every add and the multiply one fp32 operation;
//                         mode 1 takes the maximum of the four instead (schedules), a NaN among them giving NaN.
//   tile_compose_kernel   the skeleton over a window of pyramid level k whose tiles have not all arrived (DESIGN section
//                         9za): a pixel all of whose 1, 2 or 4 tiles have a slot >= 0 is sharp and gets
//                         tile_blend_kernel's value; any other pixel reads none of its tiles and is the bilinear upsample
//                         by 2^d of `below`, a window of level j = k + d.  Along an axis, output coordinate P has
//                         n = 2 P + 1 - 2^d, a = n >> (d + 1) (the floor, also for n < 0), f = (n - a 2^(d+1)) / 2^(d+1), exact
//                         and never 0, and the sources clamp(a) and clamp(a + 1) in 0 .. N_j - 1; with lerp(p, q, f) =
//                         p + f * (q - p), three fp32 operations that nothing contracts, the value is
//                         lerp(lerp(s[r0][c0], s[r0][c1], fx), lerp(s[r1][c0], s[r1][c1], fx), fy).  The switch is hard.
//   picture_resample_kernel  a viewport: the rect (y0, x0, h, w) / unit of the picture, read from level k,
//                         shown in oh x ow pixels at any zoom.  Along an axis, output coordinate P has its centre at n / D of
//                         level k (pixel i centred at i + 1/2): D = 2^(k+1) oh unit, n = 2 oh y0 + (2 P + 1) h - 2^k oh unit,
//                         T = max(D, 2 h); the taps are the i with |D i - n| < T, of integer weight u_i = T - |D i - n| and
//                         fp32 weight float(u_i) / float(sum u), the source clamp(i, 0, N_k - 1).  The value is the sum over
//                         the row taps of wy * (sum over the column taps of wx * s), ascending, each sum from its first term,
//                         every operation one fp32 operation.  All of it comes from the viewport's integers in the thread.
//                         Three kernels, one value: up to 4 taps per axis unrolled with cached reads, the same with the block's
//                         source box staged in LDS where the column scale is 1.9 .. 2, and a bounded loop up to 32 taps.
// All move data only: 16-byte loads and stores where the four pixels share their tiles and the addresses are aligned,
// scalar ones otherwise (a window may start at any column).  They allocate nothing and can be captured.
#include "common.h"
#include <cstdint>
#include <type_traits>

namespace vam {
namespace {

constexpr int kTileMaxSide = 1 << 24;       // picture sides: every pixel index stays far inside a long

struct TileGeom {
  int H, W, th, tw, V, Sy, Sx, R, C;
};

int tile_geometry(const char* who, int H, int W, int th, int tw, int V, TileGeom* g) {
  VAM_REQUIRE(H >= 1 && W >= 1 && H <= kTileMaxSide && W <= kTileMaxSide, "%s: a picture of %d x %d: sides are 1 .. %d", who, H, W,
              kTileMaxSide);
  VAM_REQUIRE(th >= 1 && tw >= 1 && th <= 65536 && tw <= 65536, "%s: tiles of %d x %d: sides are 1 .. 65536", who, th, tw);
  VAM_REQUIRE(V >= 0 && 2 * (long)V <= (th < tw ? th : tw), "%s: overlap %d: need 0 <= 2 * overlap <= min(%d, %d)", who, V, th, tw);
  g->H = H; g->W = W; g->th = th; g->tw = tw; g->V = V;
  g->Sy = th - V; g->Sx = tw - V;
  g->R = H - V > 0 ? (int)cdiv(H - V, g->Sy) : 1;
  g->C = W - V > 0 ? (int)cdiv(W - V, g->Sx) : 1;
  return VAM_OK;
}

struct ExtractArgs {
  const float* image;
  const int32_t* coords;
  float* out;
  TileGeom g;
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(256) void tile_extract_kernel(const ExtractArgs a) {
  const TileGeom& g = a.g;
  const int x = 4 * (blockIdx.x * 64 + threadIdx.x), y = blockIdx.y * 4 + threadIdx.y;
  if (x >= g.tw || y >= g.th) return;
  const int i = blockIdx.z;
  const int r = a.coords[2 * i], c = a.coords[2 * i + 1];
  if ((unsigned)r >= (unsigned)g.R || (unsigned)c >= (unsigned)g.C) return;      // not a tile of this grid: write nothing
  const int nv = min(4, g.tw - x);
  const int Y = min(r * g.Sy + y, g.H - 1), X = c * g.Sx + x;
  const long plane = (long)g.H * g.W;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* src = a.image + ch * plane + (long)Y * g.W;
    float* dst = a.out + (((long)i * 3 + ch) * g.th + y) * g.tw + x;
    float v[4];
    if (X + 3 < g.W && aligned16(src + X)) {
      const float4 q = *reinterpret_cast<const float4*>(src + X);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = src[min(X + k, g.W - 1)];
    }
    if (nv == 4 && aligned16(dst)) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) dst[k] = v[k];
    }
  }
}

struct ScheduleArgs {
  const float* maps;
  const int32_t* coords;
  float* out;
  TileGeom g;
  int L, ch, cw;                            // stages, latent rows and columns of a tile (th / 16, tw / 16)
};

// Block (64, 4): wave threadIdx.y owns cell (a, b) = (blockIdx.y, 4 blockIdx.x + threadIdx.y) of tile i at stage k, where
// blockIdx.z = i L + k.  Everything that decides a return is uniform over the wave, so the shuffles run with all 64 lanes.
__global__ __launch_bounds__(256) void tile_schedule_kernel(const ScheduleArgs s) {
  const TileGeom& g = s.g;
  const int a = blockIdx.y, b = 4 * blockIdx.x + threadIdx.y;
  if (b >= s.cw) return;
  const int i = blockIdx.z / s.L, k = blockIdx.z - i * s.L;
  const int r = s.coords[2 * i], c = s.coords[2 * i + 1];
  if ((unsigned)r >= (unsigned)g.R || (unsigned)c >= (unsigned)g.C) return;      // not a tile of this grid: write nothing
  const int lane = threadIdx.x;
  const int Y = min(r * g.Sy + 16 * a + (lane >> 2), g.H - 1), X = c * g.Sx + 16 * b + 4 * (lane & 3);
  const float* src = s.maps + ((long)k * g.H + Y) * g.W;
  float v[4];
  if (X + 3 < g.W && aligned16(src + X)) {
    const float4 q = *reinterpret_cast<const float4*>(src + X);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[min(X + j, g.W - 1)];
  }
  float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
  int bad = (v[0] != v[0]) | (v[1] != v[1]) | (v[2] != v[2]) | (v[3] != v[3]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m = fmaxf(m, __shfl_xor(m, d, 64));
    bad |= __shfl_xor(bad, d, 64);
  }
  if (lane == 0) s.out[(((long)i * s.L + k) * s.ch + a) * s.cw + b] = bad ? __int_as_float(0x7FC00000) : m;
}

struct BlendArgs {
  const float* tiles;
  const int32_t* slot;
  const float* w_lo;
  const float* w_hi;
  float* out_f;
  uint8_t* out_u8;
  int32_t* status;
  TileGeom g;
  int n, y0, x0, h, w;                      // the tile buffer's size; the window (refresh: the box) to visit
};

struct RefreshArgs {
  BlendArgs b;
  const int32_t* dirty;                     // int32 [R][C]
  int cy0, cx0, ch, cw;                     // the canvas's window in the picture: out has its pitch
};

struct ComposeArgs {
  BlendArgs b;                              // slot == nullptr: no tiles, and then the geometry is not looked at
  const float* below;                       // fp32 [3, hb, wb]: the window (by0, bx0, hb, wb) of the level-j picture
  int by0, bx0, hb, wb, Hj, Wj, d;
  float inv;                                // 2^-(d + 1)
};

// Where pixel P lies along an axis of n tiles with stride S: in tile t1 at l1, and when `two` in tile t1 - 1 at l1 + S.
struct Axis {
  int t1, l1;
  bool two;
};

__device__ __forceinline__ Axis tile_axis(int P, int S, int V, int n) {
  Axis a;
  a.t1 = min(n - 1, P / S);
  a.l1 = P - a.t1 * S;
  a.two = a.t1 > 0 && a.l1 < V;
  return a;
}

// NW pixels from column X on that share their column tiles (NW = 1: any pixel): acc[ch][k] by the rule above.
template <int NW>
__device__ __forceinline__ void blend_run(const BlendArgs& a, const Axis ay, const Axis ax, float (&acc)[3][4], int k0) {
  const TileGeom& g = a.g;
  bool started = false;
#pragma unroll
  for (int ry = 0; ry < 2; ++ry) {
    if (!ry && !ay.two) continue;
    const float wy = !ay.two ? 1.0f : ry ? a.w_hi[ay.l1] : a.w_lo[ay.l1];
    const int r = ay.t1 - 1 + ry, ly = ay.l1 + (ry ? 0 : g.Sy);
#pragma unroll
    for (int cx = 0; cx < 2; ++cx) {
      if (!cx && !ax.two) continue;
      const int c = ax.t1 - 1 + cx, lx = ax.l1 + (cx ? 0 : g.Sx);
      const int s = a.slot[r * g.C + c];
      if ((unsigned)s >= (unsigned)a.n) {                  // the host checks beforehand: a guard, every writer stores the same 1
        *a.status = 1;
        continue;
      }
      float w[NW];
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const float wx = !ax.two ? 1.0f : cx ? a.w_hi[ax.l1 + k] : a.w_lo[ax.l1 + k];
        w[k] = __fmul_rn(wy, wx);
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float* p = a.tiles + (((long)s * 3 + ch) * g.th + ly) * g.tw + lx;
        float v[4];
        if (NW == 4 && aligned16(p)) {
          const float4 q = *reinterpret_cast<const float4*>(p);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < NW; ++k) v[k] = p[k];
        }
#pragma unroll
        for (int k = 0; k < NW; ++k) {
          const float t = __fmul_rn(w[k], v[k]);
          acc[ch][k0 + k] = started ? __fadd_rn(acc[ch][k0 + k], t) : t;
        }
      }
      started = true;
    }
  }
  if (!started) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int k = 0; k < NW; ++k) acc[ch][k0 + k] = 0.0f;
  }
}

__device__ __forceinline__ unsigned tile_u8(float v) { return (unsigned)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }

// A thread's four pixels into element `at` on of a row of out, fp32 planes `plane` elements apart or uint8 triples.  Pixel k
// is written where k < nv (PREFIX: a thread that writes its first nv pixels; the compiler folds these compares) or where bit
// k of `mask` is set; wide where all four are written and the address is aligned (4 bytes for the uint8 triple).
template <bool PREFIX>
__device__ __forceinline__ void store_pixels(const BlendArgs& a, long at, long plane, int nv, unsigned mask, const float (&acc)[3][4]) {
  auto on = [&](int k) { return PREFIX ? k < nv : ((mask >> k) & 1u) != 0; };
  const bool all = PREFIX ? nv == 4 : mask == 15u;
  if (a.out_u8) {
    uint8_t* dst = a.out_u8 + 3 * at;
    unsigned b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[3 * k + ch] = on(k) ? tile_u8(acc[ch][k]) : 0u;
    if (all && ((uintptr_t)dst & 3) == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        reinterpret_cast<uint32_t*>(dst)[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (on(j / 3)) dst[j] = (uint8_t)b[j];
    }
    return;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* dst = a.out_f + ch * plane + at;
    if (all && aligned16(dst)) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (on(k)) dst[k] = acc[ch][k];
    }
  }
}

// Whether one of the 1, 2 or 4 entries of `table` [R][C] that belong to the tiles of a pixel at (ay, ax) passes `test`.
template <class Test>
__device__ __forceinline__ bool any_tile(const int32_t* table, int C, const Axis ay, const Axis ax, Test test) {
  const int32_t* row = table + ay.t1 * C + ax.t1;
  bool t = test(row[0]);
  if (ax.two) t |= test(row[-1]);
  if (ay.two) {
    t |= test(row[-C]);
    if (ax.two) t |= test(row[-C - 1]);
  }
  return t;
}

enum class Mode { Blend, Refresh, Compose };

// Whether a pixel at (ay, ax) gets blend_run's value.  Blend: always.  Refresh: when one of its tiles is dirty; this reads
// `dirty` only, never a slot.  Compose: when all of its tiles have a slot >= 0.
template <Mode M, class Args>
__device__ __forceinline__ bool blended(const BlendArgs& a, const Args& e, const Axis ay, const Axis ax) {
  if constexpr (M == Mode::Refresh) return any_tile(e.dirty, a.g.C, ay, ax, [](int32_t d) { return d != 0; });
  if constexpr (M == Mode::Compose) return !any_tile(a.slot, a.g.C, ay, ax, [](int32_t s) { return s < 0; });
  return true;
}

// Where coordinate P of level k reads level j = k + d along an axis of N source pixels: the two sources, as offsets into a
// window that begins at o, and the weight of the second.
struct Up {
  int i0, i1;
  float f;
};

__device__ __forceinline__ Up up_axis(int P, int d, float inv, int N, int o) {
  const int n = 2 * P + 1 - (1 << d);
  const int a = n >> (d + 1);                              // arithmetic: the floor for n < 0 as well
  Up u;
  u.f = (float)(n - a * (2 << d)) * inv;                   // an odd integer below 2^16 times a power of two: exact
  u.i0 = min(max(a, 0), N - 1) - o;
  u.i1 = min(max(a + 1, 0), N - 1) - o;
  return u;
}

__device__ __forceinline__ float lerp_rn(float p, float q, float f) { return __fadd_rn(p, __fmul_rn(f, __fsub_rn(q, p))); }

// The three window kernels.  A thread owns four consecutive pixels of one row of the window (refresh: the box) and all three
// channels.  Where the four share one tile set, one decision (blended) and blend_run<4> serve them; otherwise a decision and
// blend_run<1> per pixel.  Bit k of `sharp` says that pixel k holds blend_run's value.  A pixel that does not: refresh
// neither computes nor stores it, and its slots are not read; compose (also all pixels when slot == nullptr: no tiles, the
// geometry is not looked at) reads none of its tiles and takes the bilinear upsample of `below`, a quarter of the output's
// size or less, one value at a time: neighbouring lanes share them.
// `a`: what the three share; `e`: the mode's own arguments (blend: `a` again).
template <Mode M, class Args>
__device__ __forceinline__ void window_pixels(const BlendArgs& a, const Args& e) {
  const TileGeom& g = a.g;
  const int x = 4 * (blockIdx.x * 64 + threadIdx.x), y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.w || y >= a.h) return;
  const int nv = min(4, a.w - x);
  const int X = a.x0 + x, Y = a.y0 + y;
  float acc[3][4];
  unsigned sharp = 0;
  if (M != Mode::Compose || a.slot) {
    const Axis ay = tile_axis(Y, g.Sy, g.V, g.R);
    const Axis ax0 = tile_axis(X, g.Sx, g.V, g.C);
    bool run = false;
    if (nv == 4) {
      const Axis ax3 = tile_axis(X + 3, g.Sx, g.V, g.C);
      run = ax3.t1 == ax0.t1 && ax3.two == ax0.two;       // t1 never decreases and `two` only ends within a tile
    }
    if (run) {
      if (blended<M>(a, e, ay, ax0)) {
        blend_run<4>(a, ay, ax0, acc, 0);
        sharp = 15u;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= nv) continue;
        const Axis ax = tile_axis(X + k, g.Sx, g.V, g.C);
        if (!blended<M>(a, e, ay, ax)) continue;
        blend_run<1>(a, ay, ax, acc, k);
        sharp |= 1u << k;
      }
    }
  }
  if constexpr (M == Mode::Refresh) {
    if (sharp) store_pixels<false>(a, (long)(Y - e.cy0) * e.cw + (X - e.cx0), (long)e.ch * e.cw, nv, sharp, acc);
    return;
  }
  if constexpr (M == Mode::Compose) {
    if (sharp != 15u) {
      const Up uy = up_axis(Y, e.d, e.inv, e.Hj, e.by0);
      const long plane = (long)e.hb * e.wb;
      const float* r0 = e.below + (long)uy.i0 * e.wb;
      const float* r1 = e.below + (long)uy.i1 * e.wb;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= nv || ((sharp >> k) & 1u)) continue;
        const Up ux = up_axis(X + k, e.d, e.inv, e.Wj, e.bx0);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float* s0 = r0 + ch * plane;
          const float* s1 = r1 + ch * plane;
          acc[ch][k] = lerp_rn(lerp_rn(s0[ux.i0], s0[ux.i1], ux.f), lerp_rn(s1[ux.i0], s1[ux.i1], ux.f), uy.f);
        }
      }
    }
  }
  store_pixels<true>(a, (long)y * a.w + x, (long)a.h * a.w, nv, 0u, acc);
}

__global__ __launch_bounds__(256) void tile_blend_kernel(const BlendArgs a) { window_pixels<Mode::Blend>(a, a); }
__global__ __launch_bounds__(256) void tile_refresh_kernel(const RefreshArgs a) { window_pixels<Mode::Refresh>(a.b, a); }
__global__ __launch_bounds__(256) void tile_compose_kernel(const ComposeArgs a) { window_pixels<Mode::Compose>(a.b, a); }

struct HalveArgs {
  const float* src;
  float* dst;
  int C, Hs, Ws, Hd, Wd, mode, gy;          // gy: row blocks along grid.y; grid.z = C * (splits of the row blocks)
};

// One 2 x 2 block of the level below: rows a b over c d.  The mean is three adds and one multiply that
// nothing can contract; the maximum keeps the first of two equal operands.  Which NaN comes out is pinned: the quiet one.
__device__ __forceinline__ float halve_one(float a, float b, float c, float d, int mode) {
  float r;
  if (mode) {
    const float m0 = a >= b ? a : b, m1 = c >= d ? c : d;
    r = m0 >= m1 ? m0 : m1;
    if ((a != a) | (b != b) | (c != c) | (d != d)) r = __int_as_float(0x7FC00000);
  } else {
    r = __fmul_rn(__fadd_rn(__fadd_rn(a, b), __fadd_rn(c, d)), 0.25f);
    if (r != r) r = __int_as_float(0x7FC00000);
  }
  return r;
}

// Block (64, 4): a thread owns four consecutive pixels of one row of the level above, a wave 256 of them: it reads 2 KiB of
// each of the two source rows in 16-byte loads and stores 1 KiB.  The wide path needs all eight source columns inside the row
// and both addresses 16-byte aligned (an odd Ws or a base 4 bytes off puts rows off the boundary); otherwise the pixels are
// read one by one with the clamped column.  A clamped last ROW is the same row twice on either path.
__global__ __launch_bounds__(256) void picture_halve_kernel(const HalveArgs a) {
  const int ch = blockIdx.z % a.C;
  const long yb = (long)(blockIdx.z / a.C) * a.gy + blockIdx.y;
  const long y = yb * 4 + threadIdx.y;
  const int x = 4 * (blockIdx.x * 64 + threadIdx.x);
  if (x >= a.Wd || y >= a.Hd) return;
  const int nv = min(4, a.Wd - x);
  const long Y0 = 2 * y, Y1 = min(2 * y + 1, (long)a.Hs - 1);
  const float* r0 = a.src + ((long)ch * a.Hs + Y0) * a.Ws;
  const float* r1 = a.src + ((long)ch * a.Hs + Y1) * a.Ws;
  float* dst = a.dst + ((long)ch * a.Hd + y) * a.Wd + x;
  const int X = 2 * x;
  float v[4];
  if (X + 7 < a.Ws && aligned16(r0 + X) && aligned16(r1 + X)) {
    const float4 t0 = *reinterpret_cast<const float4*>(r0 + X), t1 = *reinterpret_cast<const float4*>(r0 + X + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(r1 + X), b1 = *reinterpret_cast<const float4*>(r1 + X + 4);
    v[0] = halve_one(t0.x, t0.y, b0.x, b0.y, a.mode);
    v[1] = halve_one(t0.z, t0.w, b0.z, b0.w, a.mode);
    v[2] = halve_one(t1.x, t1.y, b1.x, b1.y, a.mode);
    v[3] = halve_one(t1.z, t1.w, b1.z, b1.w, a.mode);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xa = min(X + 2 * k, a.Ws - 1), xb = min(X + 2 * k + 1, a.Ws - 1);      // k >= nv: clamped reads, never stored
      v[k] = halve_one(r0[xa], r0[xb], r1[xa], r1[xb], a.mode);
    }
  }
  if (nv == 4 && aligned16(dst)) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nv) dst[k] = v[k];
  }
}

// One axis of a viewport at level k, in units of 1 / D of a level-k pixel: output coordinate P has its
// centre at n(P) / D with n(P) = n0 + P dn, the tent reaches T = max(D, 2 extent) to either side, the level has N pixels
// along the axis and src's window begins at o.  Everything is below 2^53: exact in a long and in a double.
struct ResampleAxis {
  long D, T, n0, dn;
  int N, o;
};

struct ResampleArgs {
  const float* src;
  float* out_f;
  uint8_t* out_u8;
  ResampleAxis y, x;
  int C, hs, ws, oh, ow;
};

// floor(n / D) for D > 0.  The fp64 quotient of two exact operands is within 2^-27 of the true one here (it is below 2^26),
// so its floor is the true floor or one above it; the remainder, in integers, says which.
__device__ __forceinline__ long floor_div(long n, long D) {
  long q = (long)floor((double)n / (double)D);
  const long r = n - q * D;
  if (r < 0) --q;
  else if (r >= D) ++q;
  return q;
}

__device__ __forceinline__ long abs_l(long v) { return v < 0 ? -v : v; }

// Level coordinate i, clamped to the level (the edge is replicated), as an offset into a window that begins at o.
__device__ __forceinline__ int window_index(long i, int N, int o) { return (int)(i < 0 ? 0 : i > N - 1 ? N - 1 : i) - o; }

// The taps of coordinate P where the scale is at most 2 (T <= 2 D): a - 1 .. a + 2 with a = floor(n / D), r = n - a D, at the
// distances D + r, r, D - r, 2 D - r.  A weight u / S is never 0 (u >= 1, S < 2^46), so w == 0 marks a slot without a tap; such
// a slot carries the index of tap a, which always is one, so that it may be read all the same: reads need no branch.
struct Taps4 {
  int i[4];
  float w[4];
};

__device__ __forceinline__ Taps4 taps4(const ResampleAxis& ax, int P) {
  const long n = ax.n0 + P * ax.dn;
  const long a = floor_div(n, ax.D), r = n - a * ax.D;
  const long u[4] = {ax.T - ax.D - r, ax.T - r, ax.T - ax.D + r, ax.T - 2 * ax.D + r};
  long S = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) S += u[j] > 0 ? u[j] : 0;
  const float fS = (float)S;
  Taps4 t;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t.w[j] = u[j] > 0 ? (float)u[j] / fS : 0.0f;           // two round-to-nearest conversions, one correctly rounded division
    t.i[j] = window_index(u[j] > 0 ? a - 1 + j : a, ax.N, ax.o);
  }
  return t;
}

// The taps of coordinate P at any scale up to 16: lo .. lo + cnt - 1 (cnt <= 32), tap lo + j at the signed distance e0 + j D.
struct TapsN {
  long e0, lo;
  int cnt;
  float fS;
};

__device__ __forceinline__ TapsN tapsN(const ResampleAxis& ax, int P) {
  const long n = ax.n0 + P * ax.dn;
  TapsN t;
  t.lo = floor_div(n - ax.T, ax.D) + 1;                    // the first i with D i - n > -T
  const long cnt = floor_div(n + ax.T - 1, ax.D) - t.lo + 1;      // up to the last i with D i - n < T
  t.cnt = (int)(cnt < 32 ? cnt : 32);                      // the bound; the host refuses a scale above 16, which has no more
  t.e0 = ax.D * t.lo - n;
  long S = 0;
  for (int j = 0; j < t.cnt; ++j) S += ax.T - abs_l(t.e0 + j * ax.D);
  t.fS = (float)S;
  return t;
}

__device__ __forceinline__ float tapN_weight(const ResampleAxis& ax, const TapsN& t, int j) {
  return (float)(ax.T - abs_l(t.e0 + j * ax.D)) / t.fS;
}

// One plane's four pixels: v[k] = sum over the row taps r of wy_r * (sum over pixel k's column taps c of wx_c * s[r][c]),
// taps ascending, every sum from its first term, every product and add one fp32 operation.  Pixels past the row's end were
// given the last column's taps: their reads stay inside and they are never stored.  A wave shares its output row, so the row
// slots are in scalar registers and an empty one is skipped by the whole wave.  Along the columns the outer slots a - 1 and
// a + 2 are skipped by the whole launch when the scale is at most 1 (`wide` false: T = D leaves a and a + 1); a slot that is
// read is read without a branch, so that a row's loads are in flight together, and a select leaves an empty slot out of the
// sum: the operations performed are those of the taps alone.
__device__ __forceinline__ void resample_plane(const float* s, int pitch, const Taps4& ty, const Taps4 (&tx)[4], bool wide, float (&v)[4]) {
  bool started = false;
#pragma unroll
  for (int jr = 0; jr < 4; ++jr) {
    if (ty.w[jr] == 0.0f) continue;
    const float* row = s + (long)ty.i[jr] * pitch;
    float q[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[k][1] = row[tx[k].i[1]];
      q[k][2] = row[tx[k].i[2]];
      if (wide) {
        q[k][0] = row[tx[k].i[0]];
        q[k][3] = row[tx[k].i[3]];
      } else {
        q[k][0] = q[k][3] = 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float in = __fmul_rn(tx[k].w[1], q[k][1]);                                // tap a: always there
      in = tx[k].w[0] != 0.0f ? __fadd_rn(__fmul_rn(tx[k].w[0], q[k][0]), in) : in;
      in = tx[k].w[2] != 0.0f ? __fadd_rn(in, __fmul_rn(tx[k].w[2], q[k][2])) : in;
      in = tx[k].w[3] != 0.0f ? __fadd_rn(in, __fmul_rn(tx[k].w[3], q[k][3])) : in;
      const float t = __fmul_rn(ty.w[jr], in);
      v[k] = started ? __fadd_rn(v[k], t) : t;
    }
    started = true;
  }
}

__device__ __forceinline__ void resample_plane(const ResampleArgs& a, const float* s, const TapsN& ty, const TapsN (&tx)[4], float (&v)[4]) {
  for (int jr = 0; jr < ty.cnt; ++jr) {
    const float wy = tapN_weight(a.y, ty, jr);
    const float* row = s + (long)window_index(ty.lo + jr, a.y.N, a.y.o) * a.ws;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float in = 0.0f;
      for (int jc = 0; jc < tx[k].cnt; ++jc) {
        const float t = __fmul_rn(tapN_weight(a.x, tx[k], jc), row[window_index(tx[k].lo + jc, a.x.N, a.x.o)]);
        in = jc ? __fadd_rn(in, t) : t;
      }
      const float t = __fmul_rn(wy, in);
      v[k] = jr ? __fadd_rn(v[k], t) : t;
    }
  }
}

// Block (64, 4): a thread owns four consecutive pixels of one output row and every plane.  It works out the row's taps once
// and each pixel's column taps once, from the viewport's integers alone (no table comes from the host), then reads src, a
// window of the level that the host has checked to hold every tap, one value at a time: neighbouring lanes share them.
// LOOP = false: at most four taps along both axes, held in registers; true: up to 32, their weights recomputed where used.
// picture_resample_staged_kernel below is LOOP = false with src staged in LDS; the host picks it by the column scale.
template <bool LOOP>
__global__ __launch_bounds__(256) void picture_resample_kernel(const ResampleArgs a) {
  using Taps = typename std::conditional<LOOP, TapsN, Taps4>::type;
  const int x = 4 * (blockIdx.x * 64 + threadIdx.x), y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.ow || y >= a.oh) return;
  const int nv = min(4, a.ow - x);
  Taps ty, tx[4];
  if constexpr (LOOP) {
    ty = tapsN(a.y, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) tx[k] = tapsN(a.x, min(x + k, a.ow - 1));
  } else {
    ty = taps4(a.y, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                          // blockDim.x is the wave: its lanes share y
      ty.w[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ty.w[j])));
      ty.i[j] = __builtin_amdgcn_readfirstlane(ty.i[j]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tx[k] = taps4(a.x, min(x + k, a.ow - 1));
  }
  const bool wide = a.x.T > a.x.D;
  const long plane = (long)a.hs * a.ws, at = (long)y * a.ow + x;
  auto one = [&](int ch, float (&v)[4]) {
    if constexpr (LOOP) resample_plane(a, a.src + ch * plane, ty, tx, v);
    else resample_plane(a.src + ch * plane, a.ws, ty, tx, wide, v);
  };
  if (a.out_u8) {                                          // C = 3: the triples need all three planes
    float acc[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) one(ch, acc[ch]);
    BlendArgs b = {};
    b.out_u8 = a.out_u8;
    store_pixels<true>(b, at, 0, nv, 0u, acc);
    return;
  }
  for (int ch = 0; ch < a.C; ++ch) {
    float v[4];
    one(ch, v);
    float* dst = a.out_f + (long)ch * a.oh * a.ow + at;
    if (nv == 4 && aligned16(dst)) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) dst[k] = v[k];
    }
  }
}

// The unrolled kernel with the source staged in LDS, for column scales from 1.9 to 2, where a wave's reads of src lie 30 bytes
// and more apart and the cached reads above cost up to half as much again (below 1.9 staging loses).  The
// block's 4 x 256 pixels read a box of src of at most 3 * 2 + 4 rows and 255 * 2 + 4 columns: rows floor(n / D) - 1 of its first
// row .. floor(n / D) + 2 of its last, columns likewise, clamped to the level and cut to the window of src (a slot outside
// it is empty and carries the index of tap a).  Plane by plane the block copies the box with coalesced reads, waits, and
// every thread takes its taps from LDS with resample_plane: the same operations on the same values as the kernel above.  A
// thread past the output's edge takes the edge's taps, keeps to the barriers and stores nothing.
constexpr int kStageRows = 11, kStagePitch = 520;

__global__ __launch_bounds__(256) void picture_resample_staged_kernel(const ResampleArgs a) {
  __shared__ float tile[kStageRows * kStagePitch];
  const int bx = 256 * blockIdx.x, by = 4 * blockIdx.y;
  const int x = bx + 4 * threadIdx.x, y = by + threadIdx.y;
  const bool live = x < a.ow && y < a.oh;
  const int nv = min(4, a.ow - x);
  auto box = [&](const ResampleAxis& ax, int P0, int P1, int n_win, int* lo, int* hi) {
    const int l = window_index(floor_div(ax.n0 + P0 * ax.dn, ax.D) - 1, ax.N, ax.o);
    const int h = window_index(floor_div(ax.n0 + P1 * ax.dn, ax.D) + 2, ax.N, ax.o);
    *lo = min(max(l, 0), n_win - 1);
    *hi = min(max(h, 0), n_win - 1);
  };
  int rlo, rhi, clo, chi;
  box(a.y, by, min(by + 3, a.oh - 1), a.hs, &rlo, &rhi);
  box(a.x, bx, min(bx + 255, a.ow - 1), a.ws, &clo, &chi);
  const int nr = min(rhi - rlo + 1, kStageRows), nc = min(chi - clo + 1, kStagePitch);
  Taps4 ty = taps4(a.y, min(y, a.oh - 1)), tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ty.w[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ty.w[j])));
    ty.i[j] = __builtin_amdgcn_readfirstlane(ty.i[j]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) tx[k] = taps4(a.x, min(x + k, a.ow - 1));
  const bool wide = a.x.T > a.x.D;
  const long plane = (long)a.hs * a.ws, at = (long)y * a.ow + x;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  auto one = [&](int ch, float (&v)[4]) {
    __syncthreads();
    const float* s = a.src + ch * plane + (long)rlo * a.ws + clo;
    for (int r = 0; r < nr; ++r)
      for (int c = tid; c < nc; c += 256) tile[r * kStagePitch + c] = s[(long)r * a.ws + c];
    __syncthreads();
    resample_plane(tile - rlo * kStagePitch - clo, kStagePitch, ty, tx, wide, v);
  };
  if (a.out_u8) {
    float acc[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) one(ch, acc[ch]);
    BlendArgs b = {};
    b.out_u8 = a.out_u8;
    if (live) store_pixels<true>(b, at, 0, nv, 0u, acc);
    return;
  }
  for (int ch = 0; ch < a.C; ++ch) {
    float v[4];
    one(ch, v);
    if (!live) continue;
    float* dst = a.out_f + (long)ch * a.oh * a.ow + at;
    if (nv == 4 && aligned16(dst)) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) dst[k] = v[k];
    }
  }
}

// The checks and the arguments that vam_tile_blend, vam_tile_refresh and vam_tile_compose share, in three steps that an entry
// point puts its own checks between.  First the tiles: the geometry, the pointers (`have`: whether the entry point's are
// there, `need`: their names), the ramps and n; `none`: compose without tiles, where th, tw and V are not looked at.
int window_tiles(const char* who, BlendArgs* a, bool none, bool have, const char* need, const float* tiles, int n, const int32_t* slot,
                 const float* w_lo, const float* w_hi, int32_t* status, int H, int W, int th, int tw, int V) {
  if (none) {
    VAM_REQUIRE(H >= 1 && W >= 1 && H <= kTileMaxSide && W <= kTileMaxSide, "%s: a picture of %d x %d: sides are 1 .. %d", who, H, W,
                kTileMaxSide);
  } else {
    if (int rc = tile_geometry(who, H, W, th, tw, V, &a->g)) return rc;
    VAM_REQUIRE(have, "%s: need %s", who, need);
    VAM_REQUIRE(V == 0 || (w_lo && w_hi), "%s: an overlap of %d needs the two ramp tables", who, V);
    VAM_REQUIRE(n >= 1, "%s: a buffer of %d tiles", who, n);
  }
  a->tiles = tiles; a->slot = slot; a->w_lo = w_lo; a->w_hi = w_hi; a->status = status; a->n = n;
  return VAM_OK;
}

// Then the window of the picture that out holds (`noun`: what the entry point calls it), which is also the one to visit
// until the entry point says otherwise.
int window_inside(const char* who, const char* noun, BlendArgs* a, int y0, int x0, int h, int w, int H, int W) {
  VAM_REQUIRE(y0 >= 0 && x0 >= 0 && h >= 1 && w >= 1 && h <= H - y0 && w <= W - x0,
              "%s: the %s (y0 %d, x0 %d, h %d, w %d) does not lie inside the %d x %d picture", who, noun, y0, x0, h, w, H, W);
  a->y0 = y0; a->x0 = x0; a->h = h; a->w = w;
  return VAM_OK;
}

// Last the output and the a->h rows to visit (`noun`: what the entry point calls the pixels to visit).
int window_out(const char* who, const char* noun, BlendArgs* a, void* out, int out_u8) {
  VAM_REQUIRE(out_u8 == 0 || out_u8 == 1, "%s: out_u8 is 0 (fp32 [3, h, w]) or 1 (uint8 [h, w, 3]), got %d", who, out_u8);
  VAM_REQUIRE(cdiv(a->h, 4) <= 65535u, "%s: a %s of %d rows exceeds one launch", who, noun, a->h);
  a->out_f = out_u8 ? nullptr : (float*)out;
  a->out_u8 = out_u8 ? (uint8_t*)out : nullptr;
  return VAM_OK;
}

// The launch of a window kernel over the a.h x a.w pixels to visit; `more`: the bytes it moves beside its output.
template <class Args>
int window_launch(void (*kernel)(Args), const char* name, const Args& args, const BlendArgs& a, double more, void* stream) {
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, (double)a.h * a.w * (a.out_u8 ? 15.0 : 24.0) + more);
  hipLaunchKernelGGL(kernel, dim3(cdiv(cdiv(a.w, 4), 64), cdiv(a.h, 4)), dim3(64, 4), 0, (hipStream_t)stream, args);
  return check_launch(name);
}

}  // namespace
}  // namespace vam

using namespace vam;

extern "C" {

int vam_tile_extract(const float* image, int H, int W, int th, int tw, int V, const int32_t* coords, int n, float* out,
                     void* stream) {
  ExtractArgs a;
  if (int rc = tile_geometry("vam_tile_extract", H, W, th, tw, V, &a.g)) return rc;
  VAM_REQUIRE(image && coords && out, "vam_tile_extract: need image, coords and out");
  VAM_REQUIRE(n >= 1 && n <= 65535, "vam_tile_extract: 1 .. 65535 tiles per launch, got %d", n);
  VAM_REQUIRE(cdiv(th, 4) <= 65535u, "vam_tile_extract: tiles of %d rows exceed one launch", th);
  a.image = image; a.coords = coords; a.out = out;
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, (double)n * th * tw * 24.0);
  hipLaunchKernelGGL(tile_extract_kernel, dim3(cdiv(cdiv(tw, 4), 64), cdiv(th, 4), n), dim3(64, 4), 0, (hipStream_t)stream, a);
  return check_launch("tile_extract_kernel");
}

int vam_tile_schedule(const float* maps, int L, int H, int W, int th, int tw, int V, const int32_t* coords, int n, float* out,
                      void* stream) {
  ScheduleArgs a;
  if (int rc = tile_geometry("vam_tile_schedule", H, W, th, tw, V, &a.g)) return rc;
  VAM_REQUIRE(th % 16 == 0 && tw % 16 == 0, "vam_tile_schedule: tiles of %d x %d: a latent cell is 16 x 16 pixels, sides are multiples of 16",
              th, tw);
  VAM_REQUIRE(L >= 1 && L <= VAM_MAX_LAYER_LEVELS, "vam_tile_schedule: 1 .. %d stages, got %d", VAM_MAX_LAYER_LEVELS, L);
  VAM_REQUIRE(maps && coords && out, "vam_tile_schedule: need maps, coords and out");
  VAM_REQUIRE(n >= 1 && (long)n * L <= 65535, "vam_tile_schedule: 1 .. %d tiles per launch at %d stages, got %d", 65535 / L, L, n);
  a.maps = maps; a.coords = coords; a.out = out;
  a.L = L; a.ch = th / 16; a.cw = tw / 16;
  const dim3 grid(cdiv(a.cw, 4), a.ch, n * L);
  VAM_REQUIRE((double)grid.x * grid.y * grid.z * 256.0 < 4294967296.0, "vam_tile_schedule: %d tiles of %d x %d at %d stages exceed one launch",
              n, th, tw, L);
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, (double)n * L * th * tw * 4.0 * (1.0 + 1.0 / 256.0));
  hipLaunchKernelGGL(tile_schedule_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, a);
  return check_launch("tile_schedule_kernel");
}

int vam_tile_blend(const float* tiles, int n, const int32_t* slot, const float* w_lo, const float* w_hi, int H, int W, int th,
                   int tw, int V, int y0, int x0, int h, int w, void* out, int out_u8, int32_t* status, void* stream) {
  const char* who = "vam_tile_blend";
  BlendArgs a = {};
  if (int rc = window_tiles(who, &a, false, tiles && slot && out && status, "tiles, slot, out and status", tiles, n, slot, w_lo, w_hi,
                            status, H, W, th, tw, V))
    return rc;
  if (int rc = window_inside(who, "window", &a, y0, x0, h, w, H, W)) return rc;
  if (int rc = window_out(who, "window", &a, out, out_u8)) return rc;
  return window_launch(tile_blend_kernel, "tile_blend_kernel", a, a, 0.0, stream);
}

int vam_tile_compose(const float* tiles, int n, const int32_t* slot, const float* w_lo, const float* w_hi, int H, int W, int th,
                     int tw, int V, int y0, int x0, int h, int w, const float* below, int by0, int bx0, int hb, int wb, int Hj, int Wj,
                     int d, void* out, int out_u8, int32_t* status, void* stream) {
  const char* who = "vam_tile_compose";
  ComposeArgs a = {};
  BlendArgs& b = a.b;
  const bool none = !slot && n == 0;                                            // no tiles: th, tw and V are not looked at
  if (int rc = window_tiles(who, &b, none, tiles && slot && status, "tiles, slot and status (or slot = NULL and n = 0: no tiles)", tiles, n,
                            slot, w_lo, w_hi, status, H, W, th, tw, V))
    return rc;
  VAM_REQUIRE(below && out, "vam_tile_compose: need below and out");
  if (int rc = window_inside(who, "window", &b, y0, x0, h, w, H, W)) return rc;
  if (int rc = window_out(who, "window", &b, out, out_u8)) return rc;
  VAM_REQUIRE(d >= 1 && d <= 15, "vam_tile_compose: d is 1 .. 15 (the level below is 2^d times coarser), got %d", d);
  const int scale = 1 << d;
  VAM_REQUIRE(Hj == (H + scale - 1) / scale && Wj == (W + scale - 1) / scale,
              "vam_tile_compose: a level of %d x %d below a %d x %d picture at d = %d: it is ceil(H / 2^d) x ceil(W / 2^d) = %d x %d", Hj, Wj,
              H, W, d, (H + scale - 1) / scale, (W + scale - 1) / scale);
  VAM_REQUIRE(by0 >= 0 && bx0 >= 0 && hb >= 1 && wb >= 1 && hb <= Hj - by0 && wb <= Wj - bx0,
              "vam_tile_compose: the window of below (y0 %d, x0 %d, h %d, w %d) does not lie inside the %d x %d level", by0, bx0, hb, wb,
              Hj, Wj);
  // the sources of the window: clamp(a(first)) .. clamp(a(last) + 1) along each axis, a(P) = floor((2 P + 1 - 2^d) / 2^(d+1))
  auto lo = [&](int P, int N) { const int v = (2 * P + 1 - scale) >> (d + 1); return v < 0 ? 0 : v > N - 1 ? N - 1 : v; };
  auto hi = [&](int P, int N) { const int v = ((2 * P + 1 - scale) >> (d + 1)) + 1; return v < 0 ? 0 : v > N - 1 ? N - 1 : v; };
  const int sy0 = lo(y0, Hj), sy1 = hi(y0 + h - 1, Hj), sx0 = lo(x0, Wj), sx1 = hi(x0 + w - 1, Wj);
  VAM_REQUIRE(by0 <= sy0 && sy1 < by0 + hb && bx0 <= sx0 && sx1 < bx0 + wb,
              "vam_tile_compose: the window of below (y0 %d, x0 %d, h %d, w %d) does not cover the source window (y0 %d, x0 %d, h %d, w %d) "
              "of the window (y0 %d, x0 %d, h %d, w %d) at d = %d",
              by0, bx0, hb, wb, sy0, sx0, sy1 - sy0 + 1, sx1 - sx0 + 1, y0, x0, h, w, d);
  a.below = below; a.by0 = by0; a.bx0 = bx0; a.hb = hb; a.wb = wb; a.Hj = Hj; a.Wj = Wj; a.d = d;
  a.inv = 1.0f / (float)(2 << d);
  return window_launch(tile_compose_kernel, "tile_compose_kernel", a, b, 12.0 * hb * wb, stream);
}

int vam_tile_refresh(const float* tiles, int n, const int32_t* slot, const int32_t* dirty, const float* w_lo, const float* w_hi,
                     int H, int W, int th, int tw, int V, int cy0, int cx0, int ch, int cw, int y0, int x0, int h, int w, void* out,
                     int out_u8, int32_t* status, void* stream) {
  const char* who = "vam_tile_refresh";
  RefreshArgs a = {};
  BlendArgs& b = a.b;
  if (int rc = window_tiles(who, &b, false, tiles && slot && dirty && out && status, "tiles, slot, dirty, out and status", tiles, n, slot, w_lo,
                            w_hi, status, H, W, th, tw, V))
    return rc;
  if (int rc = window_inside(who, "canvas window", &b, cy0, cx0, ch, cw, H, W)) return rc;
  VAM_REQUIRE(y0 >= cy0 && x0 >= cx0 && h >= 1 && w >= 1 && h <= cy0 + ch - y0 && w <= cx0 + cw - x0,
              "vam_tile_refresh: the box (y0 %d, x0 %d, h %d, w %d) does not lie inside the canvas window (y0 %d, x0 %d, h %d, w %d)",
              y0, x0, h, w, cy0, cx0, ch, cw);
  a.dirty = dirty; a.cy0 = cy0; a.cx0 = cx0; a.ch = ch; a.cw = cw;
  b.y0 = y0; b.x0 = x0; b.h = h; b.w = w;
  if (int rc = window_out(who, "box", &b, out, out_u8)) return rc;
  return window_launch(tile_refresh_kernel, "tile_refresh_kernel", a, b, 0.0, stream);
}

int vam_picture_halve(const float* src, int C, int Hs, int Ws, float* dst, int mode, void* stream) {
  VAM_REQUIRE(src && dst, "vam_picture_halve: need src and dst");
  VAM_REQUIRE(C >= 1 && C <= VAM_MAX_LAYER_LEVELS, "vam_picture_halve: 1 .. %d planes, got %d", VAM_MAX_LAYER_LEVELS, C);
  VAM_REQUIRE(Hs >= 1 && Ws >= 1 && Hs <= kTileMaxSide && Ws <= kTileMaxSide, "vam_picture_halve: a picture of %d x %d: sides are 1 .. %d",
              Hs, Ws, kTileMaxSide);
  VAM_REQUIRE(mode == 0 || mode == 1, "vam_picture_halve: mode is 0 (mean) or 1 (max), got %d", mode);
  HalveArgs a;
  a.src = src; a.dst = dst; a.C = C; a.Hs = Hs; a.Ws = Ws; a.mode = mode;
  a.Hd = (Hs + 1) / 2; a.Wd = (Ws + 1) / 2;
  const unsigned row_blocks = cdiv(a.Hd, 4), kMaxY = 32768;                     // up to 2^21: over grid.y and grid.z
  a.gy = (int)(row_blocks < kMaxY ? row_blocks : kMaxY);
  const dim3 grid(cdiv(cdiv(a.Wd, 4), 64), a.gy, C * cdiv(row_blocks, a.gy));
  VAM_REQUIRE((double)grid.x * grid.y * grid.z * 256.0 < 4294967296.0, "vam_picture_halve: %d planes of %d x %d exceed one launch", C,
              Hs, Ws);
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0, 4.0 * C * ((double)Hs * Ws + (double)a.Hd * a.Wd));
  hipLaunchKernelGGL(picture_halve_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, a);
  return check_launch("picture_halve_kernel");
}

int vam_picture_resample(const float* src, int C, int sy0, int sx0, int hs, int ws, int Hk, int Wk, int shift, int64_t y0, int64_t x0,
                         int64_t h, int64_t w, int unit, int oh, int ow, void* out, int out_u8, void* stream) {
  VAM_REQUIRE(src && out, "vam_picture_resample: need src and out");
  VAM_REQUIRE(C >= 1 && C <= VAM_MAX_LAYER_LEVELS, "vam_picture_resample: 1 .. %d planes, got %d", VAM_MAX_LAYER_LEVELS, C);
  VAM_REQUIRE(out_u8 == 0 || out_u8 == 1, "vam_picture_resample: out_u8 is 0 (fp32 [C, oh, ow]) or 1 (uint8 [oh, ow, 3]), got %d", out_u8);
  VAM_REQUIRE(!out_u8 || C == 3, "vam_picture_resample: a uint8 output is [oh, ow, 3]: it takes 3 planes, got %d", C);
  VAM_REQUIRE(unit >= 1 && unit <= 256, "vam_picture_resample: unit is 1 .. 256, got %d", unit);
  VAM_REQUIRE(oh >= 1 && ow >= 1 && oh <= 65536 && ow <= 65536, "vam_picture_resample: an output of %d x %d: sides are 1 .. 65536", oh, ow);
  VAM_REQUIRE(shift >= 0 && shift <= 15, "vam_picture_resample: shift is 0 .. 15 (the level), got %d", shift);
  // the pictures that have this level: sides (N_k - 1) 2^shift + 1 .. N_k 2^shift, and 2^24 at the most
  VAM_REQUIRE(Hk >= 1 && Wk >= 1 && ((long)(Hk - 1) << shift) < kTileMaxSide && ((long)(Wk - 1) << shift) < kTileMaxSide,
              "vam_picture_resample: a level of %d x %d at shift %d is ceil(. / 2^shift) of no picture with sides 1 .. %d", Hk, Wk, shift,
              kTileMaxSide);
  const long Hmax = ((long)Hk << shift) < kTileMaxSide ? ((long)Hk << shift) : kTileMaxSide;
  const long Wmax = ((long)Wk << shift) < kTileMaxSide ? ((long)Wk << shift) : kTileMaxSide;
  VAM_REQUIRE(y0 >= 0 && x0 >= 0 && h >= 1 && w >= 1 && y0 <= unit * Hmax && h <= unit * Hmax - y0 && x0 <= unit * Wmax && w <= unit * Wmax - x0,
              "vam_picture_resample: the rect (y0 %lld, x0 %lld, h %lld, w %lld) / %d does not lie inside the %ld x %ld picture of this %d x %d "
              "level at shift %d", (long long)y0, (long long)x0, (long long)h, (long long)w, unit, Hmax, Wmax, Hk, Wk, shift);
  VAM_REQUIRE(sy0 >= 0 && sx0 >= 0 && hs >= 1 && ws >= 1 && hs <= Hk - sy0 && ws <= Wk - sx0,
              "vam_picture_resample: the window of src (y0 %d, x0 %d, h %d, w %d) does not lie inside the %d x %d level", sy0, sx0, hs, ws,
              Hk, Wk);
  ResampleArgs a;
  auto axis = [&](ResampleAxis* ax, long origin, long extent, int o_n, int N, int o) {
    const long half = ((long)o_n * unit) << shift;          // D / 2: an output pixel's share of the axis at scale 1
    ax->D = 2 * half;
    ax->T = ax->D > 2 * extent ? ax->D : 2 * extent;
    ax->n0 = 2 * o_n * origin + extent - half;
    ax->dn = 2 * extent;
    ax->N = N; ax->o = o;
  };
  axis(&a.y, y0, h, oh, Hk, sy0);
  axis(&a.x, x0, w, ow, Wk, sx0);
  if (a.y.T > 16 * a.y.D || a.x.T > 16 * a.x.D) {           // more than 32 taps: how many levels bring both scales to 16
    int need = shift;
    while ((h > 16 * (((long)oh * unit) << need) || w > 16 * (((long)ow * unit) << need)) && need < 40) ++need;
    set_error("vam_picture_resample: the rect (h %lld, w %lld) / %d into %d x %d at shift %d has a scale of %.4g x %.4g: above 16; a "
              "pyramid of %d levels has a level (shift %d) that brings it to 16 or below", (long long)h, (long long)w, unit, oh, ow, shift,
              (double)h / (double)(a.y.D / 2), (double)w / (double)(a.x.D / 2), need + 1, need);
    return VAM_EINVAL;
  }
  // the support window: clamp(first tap of the first output coordinate) .. clamp(last tap of the last one), per axis
  auto fdiv = [](long n, long D) { return n >= 0 ? n / D : -((-n + D - 1) / D); };
  auto clampN = [](long v, int N) { return (int)(v < 0 ? 0 : v > N - 1 ? N - 1 : v); };
  auto first = [&](const ResampleAxis& ax) { return clampN(fdiv(ax.n0 - ax.T, ax.D) + 1, ax.N); };
  auto last = [&](const ResampleAxis& ax, int o_n) { return clampN(fdiv(ax.n0 + (o_n - 1) * ax.dn + ax.T - 1, ax.D), ax.N); };
  const int ry0 = first(a.y), ry1 = last(a.y, oh), rx0 = first(a.x), rx1 = last(a.x, ow);
  VAM_REQUIRE(sy0 <= ry0 && ry1 < sy0 + hs && sx0 <= rx0 && rx1 < sx0 + ws,
              "vam_picture_resample: the window of src (y0 %d, x0 %d, h %d, w %d) does not cover the support window (y0 %d, x0 %d, h %d, w %d) "
              "of the rect (y0 %lld, x0 %lld, h %lld, w %lld) / %d into %d x %d at shift %d",
              sy0, sx0, hs, ws, ry0, rx0, ry1 - ry0 + 1, rx1 - rx0 + 1, (long long)y0, (long long)x0, (long long)h, (long long)w, unit, oh, ow,
              shift);
  a.src = src; a.C = C; a.hs = hs; a.ws = ws; a.oh = oh; a.ow = ow;
  a.out_f = out_u8 ? nullptr : (float*)out;
  a.out_u8 = out_u8 ? (uint8_t*)out : nullptr;
  const bool loop = a.y.T > 2 * a.y.D || a.x.T > 2 * a.x.D;  // a scale above 2 has more than four taps
  const dim3 grid(cdiv(cdiv(ow, 4), 64), cdiv(oh, 4));
  ProfScope ps(VAM_FAM_MISC, (hipStream_t)stream, 0,
               (double)C * ((double)oh * ow * (out_u8 ? 1.0 : 4.0) + 4.0 * (ry1 - ry0 + 1) * (double)(rx1 - rx0 + 1)));
  const bool staged = !loop && 10 * a.x.T >= 19 * a.x.D;     // a column scale of 1.9 .. 2: measured, DESIGN section 9zc
  if (staged) hipLaunchKernelGGL(picture_resample_staged_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, a);
  else if (loop) hipLaunchKernelGGL(picture_resample_kernel<true>, grid, dim3(64, 4), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(picture_resample_kernel<false>, grid, dim3(64, 4), 0, (hipStream_t)stream, a);
  return check_launch("picture_resample_kernel");
}

}  // extern "C"
