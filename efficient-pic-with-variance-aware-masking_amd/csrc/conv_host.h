// What the convolution kernel (conv_igemm.hip) and the weight packing (conv_pack.hip) share: the kernel's argument
// structs, the packing granularity, the arithmetic mode and the geometry of a packed weight buffer.
#pragma once
#include "common.h"
#include <cstdlib>

namespace vam {

struct ConvP {
  const float* seg_ptr[VAM_MAX_SEG];
  int seg_ld[VAM_MAX_SEG];
  int seg_end[VAM_MAX_SEG];  // cumulative channel end of each segment
  int n_seg;
  int H, W, HW;
  int kh, kw, stride, pad_y, pad_x;
  int Ho, Wo, HoWo;
  int P;        // B*Ho*Wo
  int N, Npad;  // output channels, padded to 32
  int Cin, Kc, Kc16;  // total input channels, K chunks (of the kernel's BK) per tap, 16-channel packing chunks per tap
  const float* wpack;
  const float* bias;
  float* out;
  int ldo, Hf, Wf, osy, osx, ooy, oox, Cq, act, flags;
  const float* pre;
  const float* mul;
  const float* post;
  const float* post2;
  int ld_pre, ld_mul, ld_post, ld_post2;
  float* preact;        // optional second output: the value the activation is applied to (bias + pre + conv), fp32, indexed like the output
  int ld_preact;
  int tiles_n;
  const int* in_amax[VAM_MAX_SEG];   // MODE 3: per input segment, a device cell holding the bits of an upper bound of max |x| (nullptr: unused)
  int* out_amax;        // any mode: if set, the epilogue folds max |stored value| into this cell (integer atomicMax on the float's bits)
};

constexpr int VAM_CONVI_DUAL = 1 << 29;     // internal ConvP flag: 16-channel input, two taps share one 32-channel K chunk (split-operand mode)
constexpr int VAM_CONVI_STAGED = 1 << 30;   // internal ConvP flag: tensor extents beyond the direct epilogue's 32-bit window

struct GroupArgs {
  int nprob;
  int staged_epilogue;   // 1: every problem takes the LDS-staged epilogue (VAMPIC_EPILOGUE=staged: A/B measurements, bit-identity tests)
  int tile_start[VAM_MAX_GROUP + 1];
  ConvP p[VAM_MAX_GROUP];
};

constexpr int PK = 16;  // packing granularity of the weight buffer along K

int conv_mode();        // 0 = fp32 MFMA, 1 = bf16x3 MFMA, 3 = fp16x2 MFMA (VAMPIC_CONV / vam_conv_set_mode; conv_igemm.hip)

static inline bool dual_tap(int cin, int taps) { return cin == 16 && taps > 1; }   // split-operand mode: see VAM_CONVI_DUAL

// A weight buffer of the split-operand layouts ([tap][32-channel chunk][npad][...]): padded output channels, chunks per
// tap, whether two taps share a chunk (dual_tap), and the elements (32 per chunk row) the pack kernels write.  The buffer
// itself is sized for the plain layout (kh * kw * kc32 chunk slabs), which the dual one never exceeds.
struct PackGeom {
  int npad, kc32, dual;
  long total;
};
static inline PackGeom pack_geom(int kh, int kw, int cin, int n) {
  PackGeom g;
  g.npad = (n + 31) / 32 * 32;
  g.kc32 = (cin + 31) / 32;
  g.dual = dual_tap(cin, kh * kw) ? 1 : 0;
  g.total = g.dual ? (long)((kh * kw + 1) / 2) * g.npad * 32 : (long)kh * kw * g.kc32 * g.npad * 32;
  return g;
}

}  // namespace vam
