// The last two layers of a slice stack — conv3x3(128 -> 64) + GELU, conv3x3(64 -> 32) [+ the LRP tail's epilogue] — as ONE launch
// (reference: the Sequential tails of cc_mean_transforms / cc_scale_transforms / lrp_transforms, models/pic.py:86-121; DESIGN
// section 10, profiles/r04_stack_tail_prototype.txt, profiles/r06_stack_tail_ab.txt).
//
//   * input: the 128-channel activation as bf16x3 planes (ops.View3: [pixel][8-channel group][plane][8 bf16]); weights and bias as
//     conv_igemm_kernel reads them ([tap][32-channel chunk][n][plane 3][group 4][8 bf16], 192 B per (n, chunk)); output fp32 NHWC;
//   * a workgroup (6 waves) owns 4 output rows x 16 columns of one image: layer 4 on the 6 x 16 pixels those need (rows outside
//     the image are zero = the next layer's padding), kept in LDS as planes after bias + GELU + the exact three-term split (what
//     the two-launch path writes with VAM_CONV_OUT_BF3); layer 5 from LDS;
//   * conv_igemm_kernel's canonical K order (32-channel chunk outer, tap, two 16-channel steps) and six-product order, MFMA with
//     A = weights, B = pixels (resunit.hip's orientation): the results are the two launches' bit for bit
//     (tests/test_gpu_ops.py::test_fused_stack_tail_is_bit_identical, tests/test_gpu_stack_tail_pipeline.py);
//   * 18 barrier-separated steps (12 of layer 4, 6 of layer 5), one weight slab each = the three taps of one kernel row of one
//     chunk (36 KB; layer 5: 18 KB).  Everything that enters LDS from memory comes by LDS-DMA (buffer_load ... lds), no staging
//     registers and no ds_write: the slabs into a ring of three slots, requested two steps ahead, six (three) 1 KB pieces per wave;
//     the input chunk (8 rows x 16 pixels x 192 B plus zero columns) into two buffers, requested three steps ahead, its zero
//     columns and out-of-image rows from out-of-range buffer offsets.  A packed weight row is [plane][group] already, so the LDS
//     image is what unit_off() defines, with the XOR swizzle applied to each lane's SOURCE address.  A step opens with a counted
//     s_waitcnt vmcnt(N) and a raw s_barrier (never __syncthreads(): hipcc drains vmcnt(0) there), so the younger requests stay
//     in flight across it;
//   * inside a step a wave reads the six fragments of the next (tap, half) group before it issues the six MFMAs of the current
//     one: what bounded the register-staged kernel was the exposed ds_read latency in front of every group of six MFMAs (its
//     layer-5 waves, alone on their SIMDs, ran at half the matrix rate), not the staging and not LDS bandwidth.  The DMA
//     requests of a step are spread through it in the same way, one piece behind an MFMA of each group.  Measured on 2 x 32
//     images: 31.4 -> 23.45 us per launch, 79 k -> 55 k cycles per workgroup against a matrix floor of 34.6 k; what is left is
//     the start of a workgroup (9.7 k cycles until its first step is done) and the VALU-bound layer-4 epilogue (4.1 k);
//   * LDS: [input buffer 0 | input buffer 1 | ring of 3 slabs] = 163,200 B; the layer-4 image (41 KB) lies over the two input
//     buffers, which are dead by then.  Input rows have a pitch of 17 pixels: the zero column right of a row is the zero column
//     left of the next.
// Latents 16 columns wide only (256-pixel-wide images); everything else takes the two launches.
#include "common.h"
#include <atomic>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace vam {

constexpr int C_IN = 128, C_MID = 64, C_OUT = 32, WW = 16, TR = 4;
constexpr int HALO_W = WW + 2;                      // layer-4 image: zero column left and right
constexpr int IN_W = WW + 1;                        // input chunk: one zero column per row, shared by neighbouring rows
constexpr int IN_ROWS = TR + 4, MID_ROWS = TR + 2;  // input rows r0-2 .. r0+TR+1, layer-4 rows r0-1 .. r0+TR
constexpr int IN_PIX = IN_ROWS * IN_W + 1;          // 137 (pixel ry * 17 + cx, cx = 0 .. 17; cx = 0 and cx = 17 are zero)
constexpr int MID_PIX = MID_ROWS * HALO_W;          // 108 (columns 0 and 17 stay zero)
constexpr int NPB4 = (TR + 2) / 2, NPB5 = TR / 2;   // 32-pixel blocks (two image rows) of layer 4 / layer 5
constexpr int NW = NPB4 * 2, NT = 64 * NW;          // one wave per (pixel block, 32-channel block) of layer 4
constexpr int IN_UNITS = IN_PIX * 12;               // 16-byte units of an input chunk: 1,644
constexpr int IN_PIECES = (IN_UNITS + 63) / 64;     // 1 KB DMA pieces: 26 (the last one 44 lanes)
constexpr int NIN = (IN_PIECES + NW - 1) / NW;      // per wave: 5 (pieces 26 .. 29 repeat 0 .. 3: same bytes to the same place)
constexpr int S_IN = IN_PIX * 192;                  // one 32-channel chunk of the input tile: 26,304 B
constexpr int S_MID = MID_PIX * 2 * 192;            // layer-4 output, 2 chunks: 41,472 B, over the input buffers
constexpr int S_TAP = C_MID * 192;                  // one tap of one chunk: 12,288 B (layer 5: the first half)
constexpr int S_SLAB = 3 * S_TAP;                   // a slab = the three taps of one kernel row
constexpr int NW4 = S_SLAB / 1024 / NW, NW5 = NW4 / 2;   // DMA pieces per wave and slab: 6 (layer 5: 3)
constexpr int TAIL_LDS = 2 * S_IN + 3 * S_SLAB;     // 163,200 B
static_assert(S_MID <= 2 * S_IN && TAIL_LDS <= 160 * 1024 && NW == 6, "stack tail: LDS plan");

struct TailProb {
  const unsigned char* x;                           // [pixel][16 groups][3 planes][8 bf16]: the whole 128-channel tensor
  const unsigned char* w4;
  const float* b4;
  const unsigned char* w5;
  const float* b5;
  float* out;
  const float* post;
  const float* post2;
  int ld_out, ld_post, ld_post2, act;
};
struct TailArgs {
  TailProb p[VAM_MAX_TAIL_GROUP];
  int B, H;
};

__device__ __forceinline__ void split4(const float (&v)[4], uint2& h, uint2& m, uint2& l) {
  unsigned hb[4], mb[4], lb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hb[k] = __float_as_uint(v[k]);
    const float r1 = v[k] - __uint_as_float(hb[k] & 0xFFFF0000u);
    mb[k] = __float_as_uint(r1);
    lb[k] = __float_as_uint(r1 - __uint_as_float(mb[k] & 0xFFFF0000u));
  }
  h = make_uint2(__builtin_amdgcn_perm(hb[1], hb[0], 0x07060302u), __builtin_amdgcn_perm(hb[3], hb[2], 0x07060302u));
  m = make_uint2(__builtin_amdgcn_perm(mb[1], mb[0], 0x07060302u), __builtin_amdgcn_perm(mb[3], mb[2], 0x07060302u));
  l = make_uint2(__builtin_amdgcn_perm(lb[1], lb[0], 0x07060302u), __builtin_amdgcn_perm(lb[3], lb[2], 0x07060302u));
}

#define MFMA6(acc, w, p)                                                              \
  do {                                                                                \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], p[0], acc, 0, 0, 0);          \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], p[2], acc, 0, 0, 0);          \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], p[1], acc, 0, 0, 0);          \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], p[0], acc, 0, 0, 0);          \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], p[1], acc, 0, 0, 0);          \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], p[0], acc, 0, 0, 0);          \
  } while (0)

// LDS row of 192 B = [plane 3][4 groups x 16 B], the 16-byte unit of group g stored at g ^ ((row >> 1) & 3): the 32 lanes of a
// half-wave read rows r .. r+15 (one image row) of one group — distinct banks for 8 consecutive rows x 2 halves
__device__ __forceinline__ int unit_off(int row, int plane, int g) { return row * 192 + plane * 64 + ((g ^ ((row >> 1) & 3)) << 4); }

// A step's opening: this wave's DMA pieces, all but the youngest n, have landed; then every wave's have, and every wave has
// finished the step before (its reads retired by lgkmcnt(0)).  n is a literal of the s_waitcnt.
#define TAIL_BAR(n) asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)\n\ts_barrier" ::: "memory")
// A step's 36 reads and 36 MFMAs in the order they are written: the six fragments of a (tap, half) group are read one behind
// each MFMA of the group before, in the order the MFMAs take them, so that the reads issue in the MFMAs' shadow and have a
// group of MFMAs (192 cycles) to return.  HOOK(group, MFMA) places the step's DMA requests in the same way: a piece costs its
// wave 60 - 185 cycles of issue, and six to eleven of them at the top of the step were exposed.  Left alone, the compiler's
// scheduler sinks every read to just in front of its MFMA and waits lgkmcnt(0) there; the sched_barrier behind every pair
// keeps it from that, and the waits become counted ones.
//   fragment f of a group: 0 = w[2], 1 = p[0], 2 = w[0], 3 = p[2], 4 = w[1], 5 = p[1]  (MFMA6's order of first use)
#define TAIL_MFMA(acc, fr, i)                                                                                                  \
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[i == 0 ? 0 : i == 1 || i >= 4 ? 2 : 4], fr[i == 0 || i == 3 || i == 5 ? 1 : i == 1 ? 3 : 5], \
                                                acc, 0, 0, 0)
#define TAIL_STEP(acc, FRAG, HOOK)                                               \
  do {                                                                           \
    bf16x8 fr_[2][6];                                                            \
    __builtin_amdgcn_sched_barrier(0);                                           \
    _Pragma("unroll") for (int f_ = 0; f_ < 6; ++f_) fr_[0][f_] = FRAG(0, f_);   \
    __builtin_amdgcn_sched_barrier(0);                                           \
    _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                           \
      _Pragma("unroll") for (int i_ = 0; i_ < 6; ++i_) {                         \
        TAIL_MFMA(acc, fr_[q_ & 1], i_);                                         \
        if (q_ + 1 < 6) fr_[(q_ + 1) & 1][i_] = FRAG(q_ + 1, i_);                \
        HOOK(q_, i_);                                                            \
        __builtin_amdgcn_sched_barrier(0);                                       \
      }                                                                          \
    }                                                                            \
  } while (0)
__device__ __forceinline__ void tail_bar(int n) {
  switch (n) {
    case 11: TAIL_BAR(11); break;
    case 6: TAIL_BAR(6); break;
    case 3: TAIL_BAR(3); break;
    default: TAIL_BAR(0); break;
  }
}

__global__ __launch_bounds__(NT) void stack_tail_kernel(const TailArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const sMid = smem;                 // over the input buffers, from the layer-4 epilogue on
  unsigned char* const sW = smem + 2 * S_IN;
  const int HH = __builtin_amdgcn_readfirstlane(a.H);
  const int tiles = HH / TR;
  int bid = blockIdx.x;
  const int pi = bid / (a.B * tiles);
  bid -= pi * a.B * tiles;
  const int img = bid / tiles, r0 = (bid - img * tiles) * TR;
  const TailProb& P = a.p[pi];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;

  auto desc = [&](const void* q, int bytes = 0x7FFFFFFF) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(q);
    return __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) |
                                (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)v)), 0, bytes, 0x00020000);
  };
  // the input descriptor starts at the tile's first image row, so that a lane's offset stays small whatever the tensor's size
  const int rb = r0 >= 2 ? r0 - 2 : 0;
  const __amdgpu_buffer_rsrc_t r_x = desc(P.x + (size_t)((img * HH + rb) * WW) * (C_IN / 8 * 48));
  const __amdgpu_buffer_rsrc_t r_w4 = desc(P.w4), r_w5 = desc(P.w5);

  // the layer-4 bias, ahead of every DMA request (an ordinary load behind them would wait for them all)
  const int pb4 = wid % NPB4, nb4 = wid / NPB4;     // pixel block (32 of the 96), channel block
  float4 bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias4[j] = *reinterpret_cast<const float4*>(P.b4 + nb4 * 32 + 8 * j + 4 * lh);
  // and what the final epilogue adds, for the same reason and to keep its latency off the end of the workgroup
  const int p5 = (wid % NPB5) * 32 + l31;                      // layer-5 pixel: waves 0 .. NPB5-1 compute it
  const int oy = p5 >> 4, ox = p5 & 15;
  // (no branch around the loads of an absent operand, which would put their wait here: its descriptor has no records)
  const bool has_post = P.post != nullptr, has_post2 = P.post2 != nullptr;
  const size_t tpix = (size_t)(img * HH + r0) * WW;            // the tile's first output pixel: a lane's offset stays small
  const __amdgpu_buffer_rsrc_t r_po = desc(has_post ? P.post + tpix * P.ld_post : nullptr, has_post ? 0x7FFFFFFF : 0);
  const __amdgpu_buffer_rsrc_t r_po2 = desc(has_post2 ? P.post2 + tpix * P.ld_post2 : nullptr, has_post2 ? 0x7FFFFFFF : 0);
  float4 bias5[4];
  u32x4 po[4], po2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bias5[j] = *reinterpret_cast<const float4*>(P.b5 + 8 * j + 4 * lh);
    po[j] = __builtin_amdgcn_raw_buffer_load_b128(r_po, (p5 * P.ld_post + 8 * j + 4 * lh) * 4, 0, 0);
    po2[j] = __builtin_amdgcn_raw_buffer_load_b128(r_po2, (p5 * P.ld_post2 + 8 * j + 4 * lh) * 4, 0, 0);
  }

  // ---- DMA roles.  A piece = one wave instruction = 64 lanes x 16 B, contiguous in LDS; lane `lane` of piece j fills the LDS
  // unit j * 64 + lane = (row, physical unit c'), whose content is the logical group c' ^ ((row >> 1) & 3) of its plane.
  // input chunk: pieces wid, wid + 6, ...; unit u -> halo pixel u / 12 = (ry, cx); offset 2^31 is out of range and loads zeros
  unsigned xgo[NIN];
  int xlo[NIN];
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    int j = wid + NW * i;
    j = j >= IN_PIECES ? j - IN_PIECES : j;
    const int u = j * 64 + lane;
    const int px = u / 12, cp = u - px * 12, pl = cp >> 2, g = (cp & 3) ^ ((px >> 1) & 3);
    const int ry = px / IN_W, cx = px - ry * IN_W;
    const int iy = r0 - 2 + ry;
    const bool ok = u < IN_UNITS && cx >= 1 && (unsigned)iy < (unsigned)HH;
    xgo[i] = ok ? (unsigned)(((iy - rb) * WW + cx - 1) * (C_IN / 8 * 48) + g * 48 + pl * 16) : 0x80000000u;
    xlo[i] = j * 1024;
  }
  auto dma_in = [&](int chunk, int i) {
    if (xlo[i] + lane * 16 < S_IN)                  // the last piece ends with the buffer: 44 lanes
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r_x, (__attribute__((address_space(3))) void*)(smem + (chunk & 1) * S_IN + xlo[i]), 16,
                                               (int)xgo[i], chunk * 192, 0, 0);
  };
  // weight slab: this wave stages half a tap: tap wid / 2 of the kernel row, pieces (wid & 1) * 6 + i of its 12 (layer 5: * 3, of 6)
  const int wtx = wid >> 1;
  unsigned wgo4[NW4], wgo5[NW5];
#pragma unroll
  for (int i = 0; i < NW4; ++i) {
    const int u = ((wid & 1) * NW4 + i) * 64 + lane;
    const int row = u / 12, cp = u - row * 12;
    wgo4[i] = (unsigned)((row * 12 + ((cp & ~3) | ((cp & 3) ^ ((row >> 1) & 3)))) * 16);
  }
#pragma unroll
  for (int i = 0; i < NW5; ++i) {
    const int u = ((wid & 1) * NW5 + i) * 64 + lane;
    const int row = u / 12, cp = u - row * 12;
    wgo5[i] = (unsigned)((row * 12 + ((cp & ~3) | ((cp & 3) ^ ((row >> 1) & 3)))) * 16);
  }
  // slab s = 0 .. 11: layer 4, (chunk s / 3, kernel row s % 3); s = 12 .. 17: layer 5; ring slot s % 3
  auto dma_w = [&](int s, int i) {                 // piece i of this wave's six (layer 5: three; the others are none)
    unsigned char* const d = sW + (s % 3) * S_SLAB + wtx * S_TAP;
    if (s < 12) {
      const int nc = s / 3, ty = s - nc * 3;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r_w4, (__attribute__((address_space(3))) void*)(d + ((wid & 1) * NW4 + i) * 1024), 16, (int)wgo4[i],
                                               ((ty * 3 + wtx) * 4 + nc) * (C_MID * 192), 0, 0);
    } else if (i < NW5) {
      const int nc = (s - 12) / 3, ty = s - 12 - nc * 3;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r_w5, (__attribute__((address_space(3))) void*)(d + ((wid & 1) * NW5 + i) * 1024), 16, (int)wgo5[i],
                                               ((ty * 3 + wtx) * 2 + nc) * (C_OUT * 192), 0, 0);
    }
  };
#pragma unroll
  for (int i = 0; i < NIN; ++i) dma_in(0, i);
#pragma unroll
  for (int i = 0; i < NW4; ++i) dma_w(0, i);
#pragma unroll
  for (int i = 0; i < NW4; ++i) dma_w(1, i);
  // (the wait for those ordinary loads belongs here, at the head of the request queue: left to the compiler it is a vmcnt(0)
  // at their first use, in the layer-4 epilogue, which drains layer 5's first slabs)
#pragma unroll
  for (int j = 0; j < 4; ++j)
    asm volatile("" : "+v"(bias4[j].x), "+v"(bias4[j].y), "+v"(bias4[j].z), "+v"(bias4[j].w), "+v"(bias5[j].x), "+v"(bias5[j].y), "+v"(bias5[j].z),
                 "+v"(bias5[j].w), "+v"(po[j][0]), "+v"(po[j][1]), "+v"(po[j][2]), "+v"(po[j][3]), "+v"(po2[j][0]), "+v"(po2[j][1]),
                 "+v"(po2[j][2]), "+v"(po2[j][3]));

  // =============================================================== layer 4: 96 pixels x 64 channels, K = 4 chunks x 9 taps x 2
  const int p4 = pb4 * 32 + l31;                               // layer-4 pixel: row p4 / 16 of MID_ROWS, column p4 % 16
  const int my = p4 >> 4, mx = p4 & 15;
  f32x16 acc4;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc4[r] = 0.f;
  // step st = (chunk, kernel row).  Requests in issue order, per wave: in0 w0 w1 | step 0: w2 with in1 among it (its last piece
  // is a slab's) | w3 | w4 | step 3: w5 with in2 | ... | step 9: w11 | step 10: w12 | step 11: w13 — so behind slab st there are,
  // at the top of step st, the 6 pieces of the next slab, and on a chunk's second row the 5 of the next input chunk as well
#pragma unroll
  for (int st = 0; st < 12; ++st) {
    const int chunk = st / 3, ty = st - chunk * 3;
    tail_bar(st == 11 ? NW5 : (ty == 1 && chunk + 1 < 4) ? NW4 + NIN : NW4);   // slab st (and, at row 0, the input chunk) is in LDS
    auto hook = [&](int q, int i) {
      if (i == 2) dma_w(st + 2, q);                            // into the slot step st - 1 read
      if (i == 4 && ty == 0 && chunk + 1 < 4 && q < NIN) dma_in(chunk + 1, q);   // into the buffer chunk - 1 lay in
    };
    const unsigned char* const in = smem + (chunk & 1) * S_IN;
    const unsigned char* const sl = sW + (st % 3) * S_SLAB;
    // fragment f of group q = (tap column q / 2, 16-channel half q % 2); the pixel = this lane's layer-4 pixel under the tap
    auto frag = [&](int q, int f) {
      const int tx = q >> 1, g = 2 * (q & 1) + lh, pl = f == 0 || f == 3 ? 2 : f >= 4 ? 1 : 0;
      return *reinterpret_cast<const bf16x8*>((f & 1) ? in + unit_off((my + ty) * IN_W + mx + tx, pl, g)
                                                      : sl + tx * S_TAP + unit_off(nb4 * 32 + l31, pl, g));
    };
    TAIL_STEP(acc4, frag, hook);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // every read of the input buffers and of slab 11 is done
#pragma unroll
  for (int i = 0; i < NW5; ++i) dma_w(14, i);
  // layer-4 epilogue: lane = pixel p4, registers 4j .. 4j+3 = channels nb4*32 + 8j + 4lh + {0..3}; GELU; planes into sMid
  {
    const int gy = r0 - 1 + my;                                // image row of this layer-4 pixel
    const bool in = (unsigned)gy < (unsigned)HH;
    const int row = my * HALO_W + mx + 1;                      // sMid pixel (column shifted by the zero column)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 bb = bias4[j];
      float v[4] = {acc4[4 * j] + bb.x, acc4[4 * j + 1] + bb.y, acc4[4 * j + 2] + bb.z, acc4[4 * j + 3] + bb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = in ? vam_gelu(v[i]) : 0.f;
      uint2 h, m, l;
      split4(v, h, m, l);
      unsigned char* d = sMid + nb4 * (MID_PIX * 192) + lh * 8;    // chunk nb4 of the 64 channels; group j of the chunk
      *reinterpret_cast<uint2*>(d + unit_off(row, 0, j)) = h;
      *reinterpret_cast<uint2*>(d + unit_off(row, 1, j)) = m;
      *reinterpret_cast<uint2*>(d + unit_off(row, 2, j)) = l;
    }
    // the zero columns 0 and 17 of the six rows of both chunks (the padding of layer 5): 24 pixels x 12 units
    if (tid < 2 * MID_ROWS * 2 * 12) {
      const int q = tid / 12, e = tid - q * 12;
      const int ch = q / (2 * MID_ROWS), rr = (q - ch * 2 * MID_ROWS) >> 1, side = q & 1;
      *reinterpret_cast<uint4*>(sMid + ch * (MID_PIX * 192) + (rr * HALO_W + side * (HALO_W - 1)) * 192 + e * 16) = make_uint4(0, 0, 0, 0);
    }
  }
  // =============================================================== layer 5: 64 pixels x 32 channels, K = 2 chunks x 9 taps x 2
  f32x16 acc5;                                                 // waves 0 .. NPB5-1 compute; all six stage slabs
#pragma unroll
  for (int r = 0; r < 16; ++r) acc5[r] = 0.f;
  // requests behind slab 12 + s at the top of step s: w13 w14 | w14 | w15 | w16 | w17 | none
#pragma unroll
  for (int st = 0; st < 6; ++st) {
    const int chunk = st / 3, ty = st - chunk * 3;
    tail_bar(st == 0 ? 2 * NW5 : st < 5 ? NW5 : 0);            // slab 12 + st is in LDS; at step 0, sMid is complete
    const bool more = st >= 1 && st + 2 < 6;                   // slab 12 + st + 2 into the slot step st - 1 read
    auto hook = [&](int q, int i) {
      if (more && i == 2) dma_w(12 + st + 2, q);
    };
    if (wid >= NPB5) {
#pragma unroll
      for (int q = 0; q < NW5; ++q) hook(q, 2);
    } else {
      const unsigned char* const md = sMid + chunk * (MID_PIX * 192);
      const unsigned char* const sl = sW + (st % 3) * S_SLAB;
      auto frag = [&](int q, int f) {                           // the pixel: a layer-4 halo pixel (rows r0-1.., zero border columns)
        const int tx = q >> 1, g = 2 * (q & 1) + lh, pl = f == 0 || f == 3 ? 2 : f >= 4 ? 1 : 0;
        return *reinterpret_cast<const bf16x8*>((f & 1) ? md + unit_off((oy + ty) * HALO_W + ox + tx, pl, g)
                                                        : sl + tx * S_TAP + unit_off(l31, pl, g));
      };
      TAIL_STEP(acc5, frag, hook);
    }
  }
  if (wid < NPB5) {
    // conv_igemm_kernel's epilogue order: (acc + bias) -> act -> + post -> + post2
    float* o = P.out + ((size_t)(img * HH + r0) * WW + p5) * P.ld_out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 8 * j + 4 * lh;
      const float4 bb = bias5[j];
      float v[4] = {acc5[4 * j] + bb.x, acc5[4 * j + 1] + bb.y, acc5[4 * j + 2] + bb.z, acc5[4 * j + 3] + bb.w};
      if (P.act == VAM_ACT_HALF_TANH) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = 0.5f * tanhf(v[i]);
      }
      if (has_post) {
        const u32x4 t = po[j];
        v[0] += __uint_as_float(t[0]); v[1] += __uint_as_float(t[1]); v[2] += __uint_as_float(t[2]); v[3] += __uint_as_float(t[3]);
      }
      if (has_post2) {
        const u32x4 t = po2[j];
        v[0] += __uint_as_float(t[0]); v[1] += __uint_as_float(t[1]); v[2] += __uint_as_float(t[2]); v[3] += __uint_as_float(t[3]);
      }
      *reinterpret_cast<float4*>(o + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // namespace vam

using namespace vam;

extern "C" int vam_stack_tail_group(const vam_stack_tail* probs, int n, void* stream) {
  VAM_REQUIRE(probs && n >= 1, "vam_stack_tail_group: no problems");
  const int B = probs[0].B, H = probs[0].H, W = probs[0].W;
  VAM_REQUIRE(B >= 1 && W == WW && H >= TR && H % TR == 0, "vam_stack_tail_group: built for latents 16 columns wide, rows a multiple of 4 (got %d x %d)", H, W);
  VAM_REQUIRE((long)B * H * W < (1L << 24), "vam_stack_tail_group: too many pixels");
  static std::atomic<unsigned long long> attr_set{0};
  if (int rc = set_dynamic_lds(reinterpret_cast<const void*>(stack_tail_kernel), TAIL_LDS, attr_set)) return rc;
  for (int i0 = 0; i0 < n; i0 += VAM_MAX_TAIL_GROUP) {
    const int m = n - i0 < VAM_MAX_TAIL_GROUP ? n - i0 : VAM_MAX_TAIL_GROUP;
    TailArgs a;
    a.B = B;
    a.H = H;
    for (int i = 0; i < VAM_MAX_TAIL_GROUP; ++i) {
      const vam_stack_tail& q = probs[i0 + (i < m ? i : 0)];
      if (i < m) {
        VAM_REQUIRE(q.B == B && q.H == H && q.W == W, "vam_stack_tail_group: problem %d has another extent", i0 + i);
        VAM_REQUIRE(q.x && q.w4 && q.b4 && q.w5 && q.b5 && q.out, "vam_stack_tail_group: problem %d: null operand", i0 + i);
        VAM_REQUIRE(q.x_groups == C_IN / 8 && q.ld_out >= C_OUT && q.ld_out % 4 == 0 && ((uintptr_t)q.out & 15) == 0 && ((uintptr_t)q.x & 15) == 0,
                    "vam_stack_tail_group: problem %d: pitches / alignment", i0 + i);
        VAM_REQUIRE(q.act == VAM_ACT_NONE || q.act == VAM_ACT_HALF_TANH, "vam_stack_tail_group: problem %d: activation %d", i0 + i, q.act);
        VAM_REQUIRE((!q.post.ptr || (q.post.ld >= C_OUT && q.post.ld % 4 == 0 && ((uintptr_t)q.post.ptr & 15) == 0)) &&
                    (!q.post2.ptr || (q.post2.ld >= C_OUT && q.post2.ld % 4 == 0 && ((uintptr_t)q.post2.ptr & 15) == 0)),
                    "vam_stack_tail_group: problem %d: epilogue operand", i0 + i);
      }
      TailProb& t = a.p[i];
      t.x = static_cast<const unsigned char*>(q.x);
      t.w4 = static_cast<const unsigned char*>(q.w4);
      t.b4 = q.b4;
      t.w5 = static_cast<const unsigned char*>(q.w5);
      t.b5 = q.b5;
      t.out = q.out;
      t.post = q.post.ptr;
      t.post2 = q.post2.ptr;
      t.ld_out = q.ld_out;
      t.ld_post = q.post.ld;
      t.ld_post2 = q.post2.ld;
      t.act = q.act;
    }
    const double px = (double)m * B * H * W;
    ProfScope ps(VAM_FAM_CONV, (hipStream_t)stream, 2.0 * px * 9.0 * (C_IN * C_MID + C_MID * C_OUT),
                 4.0 * (px * (C_IN + C_OUT) + 9.0 * m * (C_IN * C_MID + C_MID * C_OUT)));     // (the 64-channel intermediate never leaves LDS)
    hipLaunchKernelGGL(stack_tail_kernel, dim3((unsigned)(m * B * (H / TR))), dim3(NT), TAIL_LDS, (hipStream_t)stream, a);
    if (int rc = check_launch("stack_tail_kernel")) return rc;
  }
  return 0;
}
