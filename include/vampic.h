/*
 * libvampic — C ABI of the MI355X-native hot path of the variance-aware-masking
 * progressive image codec (reference: das-ankur/Efficient-PIC-with-Variance-Aware-Masking).
 *
 * The reference has no FFI: its boundary is the Python model object
 * (src/models/pic.py, src/models/rem_pic.py).  Each entry point below replaces the
 * torch operator pattern cited next to it; the Python package
 * `efficient-pic-with-variance-aware-masking_amd` binds them with ctypes and keeps the
 * reference's module/attribute surface on top.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - activations are NHWC fp32: element (b,y,x,c) of a tensor with pixel stride
 *     `ld` lives at ptr[((b*H + y)*W + x)*ld + c]  (ld >= C lets a tensor be a channel
 *     window of a wider buffer, which is how torch.cat is avoided);
 *   - the caller owns every buffer; kernels are enqueued on `stream` (a hipStream_t
 *     passed as void*), never allocate, never synchronise;
 *   - return value 0 = ok, negative = VAM_E*; vam_last_error() gives the message of
 *     the last failure on the calling thread.
 */
#ifndef VAMPIC_H
#define VAMPIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAM_OK 0
#define VAM_EINVAL (-1)   /* bad argument / unsupported shape */
#define VAM_EHIP (-2)     /* a HIP runtime call failed        */
#define VAM_ENOGPU (-3)   /* no gfx950 device visible          */

const char* vam_last_error(void);
int vam_version(void);
/* 0 if a HIP device is usable; fills name (<=128 bytes) and CU count. */
int vam_device_info(char* name128, int* cu_count);

/* ------------------------------------------------------------------ convolution */

/* activation applied to (acc + bias [+ pre]) */
enum vam_act {
  VAM_ACT_NONE = 0,
  VAM_ACT_GELU = 1,      /* exact erf GELU, nn.GELU() default  (pic.py:86)          */
  VAM_ACT_LEAKY = 2,     /* LeakyReLU(0.01)                    (layers/rem.py:41)   */
  VAM_ACT_HALF_TANH = 3, /* 0.5*tanh(v)                        (pic.py:550,637)     */
  VAM_ACT_SIGMOID = 4,   /*                                    (layers/layers.py:72)*/
  VAM_ACT_CLAMP01 = 5,   /* clamp_(0,1)                        (pic.py:558,651)     */
  VAM_ACT_RSQRT = 6,     /* GDN   (layers/gdn.py:72)                                */
  VAM_ACT_SQRT = 7,      /* IGDN  (layers/gdn.py:70)                                */
  VAM_ACT_DOUBLE = 8     /* 2 v: GDN backward, dx = dy dy/dx|norm + x * 2 (gamma'^T dL/dnorm) in one launch
                            (autograd of layers/gdn.py:62-75; exact: a power-of-two factor)  */
};

enum vam_conv_flags {
  VAM_CONV_SQUARE_IN = 1,   /* operand is x*x (GDN norm pool, gdn.py:68)                 */
  VAM_CONV_PS2 = 2,         /* phase-major output channels scattered like PixelShuffle(2):
                               n = phase*Cq + c -> pixel (2y+phase/2, 2x+phase%2), chan c  */
  VAM_CONV_OUT_NCHW = 4,    /* store the result NCHW (model edge, x_hat)                  */
  VAM_CONV_IN_BF3 = 8,      /* every input segment holds bf16x3 planes ("P3": [pixel][8-channel group][plane 3][8 bf16],
                               48 bytes per group; seg.ld counts GROUPS per pixel, seg.C channels) written by a launch
                               with VAM_CONV_OUT_BF3 — the split-operand kernel then stages them by plain copies     */
  VAM_CONV_OUT_BF3 = 16,    /* write the result as P3 planes (ldo counts groups per pixel) instead of fp32 NHWC; for
                               tensors whose only consumer is another convolution (inside conv stacks)               */
  /* bf16-storage mode (BASELINE configs[2] "bf16": activations of the large feature maps stored as bf16, fp32
   * accumulation; never used by the fp32 configurations) */
  VAM_CONV_W_BF16 = 32,     /* wpack comes from vam_pack_conv_weights_bf16: bf16 x bf16 products, one MFMA per block    */
  VAM_CONV_IN_BF16 = 64,    /* every input segment is a bf16 NHWC tensor (seg.ld counts bf16 elements, multiple of 8)   */
  VAM_CONV_OUT_BF16 = 128,  /* store the result as bf16 NHWC (ldo counts bf16 elements)                                 */
  VAM_CONV_AUX_BF16 = 256,  /* pre / mul / post / post2 are bf16 NHWC tensors (their ld counts bf16 elements)           */
  /* training (taped forward / backward plans): activations fused into the producing launch */
  VAM_CONV_MUL_GELU_GRAD = 512 /* the mul operand holds the PRE-ACTIVATION z of a GELU and the result is multiplied by
                               gelu'(z) instead: out = ... + gelu'(mul) * act(...).  A data-gradient launch then delivers
                               dL/dz of the GELU in front of the layer directly (autograd of nn.GELU, pic.py:86)     */
};

#define VAM_MAX_SEG 4

typedef struct vam_seg {
  const float* ptr; /* first channel of this segment at pixel (0,0,0) */
  int32_t C;        /* channels taken from it                          */
  int32_t ld;       /* pixel stride of the underlying buffer (floats)  */
} vam_seg;

typedef struct vam_aux {
  const float* ptr; /* NULL = unused; indexed like the output (pixel*ld + channel) */
  int32_t ld;
  int32_t pad_;
} vam_aux;

/*
 * One convolution problem:  out = post2 + post + mul * act(conv(cat(seg...)) + bias + pre)
 * (and, when preact is set, preact = conv(cat(seg...)) + bias + pre: the taped training forward keeps a GELU's input)
 * Replaces nn.Conv2d / nn.ConvTranspose2d (one sub-pixel phase per problem) /
 * nn.Linear and the element-wise ops the reference applies around them
 * (layers/layers.py:5-86, layers/gdn.py:62-75, layers/rem.py:52-66,130-141,
 *  models/pic.py:528-551,598-641).
 */
typedef struct vam_conv {
  vam_seg seg[VAM_MAX_SEG];
  int32_t n_seg;
  int32_t B, H, W;          /* input extent                                           */
  int32_t kh, kw;           /* taps                                                   */
  int32_t stride;           /* 1 or 2                                                 */
  int32_t pad_y, pad_x;     /* input y = oy*stride - pad_y + ty                       */
  int32_t Ho, Wo;           /* extent of the grid of output positions of THIS problem */
  int32_t N;                /* output channels (packed order)                         */
  const float* wpack;       /* from vam_pack_conv_weights (same kh,kw,Cin,N,BK)       */
  const float* bias;        /* N floats (packed order) or NULL                        */
  float* out;
  int32_t ldo;              /* output pixel stride (floats)                           */
  int32_t Hf, Wf;           /* full output extent                                     */
  int32_t osy, osx, ooy, oox; /* output pixel = (oy*osy+ooy, ox*osx+oox) (ignored w/ PS2) */
  int32_t Cq;               /* PS2: channels per phase (N == 4*Cq)                    */
  int32_t act;              /* enum vam_act                                           */
  int32_t flags;            /* enum vam_conv_flags                                    */
  vam_aux pre, mul, post, post2;
  const int32_t* in_amax[VAM_MAX_SEG]; /* fp16x2 mode (vam_conv_set_mode(3)): per input segment a device cell holding the bits
                               of an upper bound of max |x| of that segment (vam_absmax, or the out_amax cell of the launches
                               that wrote it); the launch scales by the largest.  Ignored in the other modes.            */
  int32_t* out_amax;        /* any mode, optional: the epilogue folds max |stored value| into this device cell (integer
                               atomicMax on the float's bits; zero the cell before the first producer of a step)     */
  vam_aux preact;           /* optional SECOND output (ptr is written): the value the activation is applied to, fp32 NHWC,
                               indexed like the output (pixel*ld + channel)                                           */
} vam_conv;

/* sizeof(vam_conv) as compiled into the library (binding layout guard). */
size_t vam_conv_struct_size(void);
/* Size in floats of the packed weight buffer for (kh,kw,Cin,N). */
size_t vam_conv_wpack_floats(int kh, int kw, int cin, int n);

enum vam_pack_mode {
  VAM_PACK_CONV = 0,     /* src OIHW [N][Cin][kh][kw]   (nn.Conv2d, nn.Linear with kh=kw=1) */
  VAM_PACK_DECONV5S2 = 1,/* src IOHW [Cin][Cout][5][5] (layers/layers.py:14-22); builds the
                            sub-pixel phase `phase` (0..3 = py*2+px) as a (kh,kw) in
                            {3,2}x{3,2} correlation, or with phase = -1 the merged
                            3x3 / N = 4*Cout phase-major form used with VAM_CONV_PS2   */
  VAM_PACK_PS2 = 2,      /* src OIHW with O = Cq*4 in PixelShuffle order (c*4+i*2+j) ->
                            packed n = (i*2+j)*Cq + c   (layers/layers.py:82-86)          */
  VAM_PACK_GDN = 3,      /* src gamma [N][Cin] in reparametrised storage -> max(g,2^-18)^2-2^-36
                            (layers/gdn.py:52-66, compressai NonNegativeParametrizer)     */
  VAM_PACK_CONV_DGRAD = 4,/* weights of the DATA-GRADIENT conv of a stride-1 nn.Conv2d: src is the forward
                            OIHW tensor [Cout][Cin][kh][kw]; call with cin = Cout, n = Cin (taps flipped,
                            channel roles swapped) — what autograd's conv backward-data computes          */
  VAM_PACK_GDN_T = 5     /* VAM_PACK_GDN with the reparametrised gamma TRANSPOSED: the 1x1 problem that carries
                            dL/dnorm back to the squared inputs (GDN / IGDN backward)                       */
};
/* Device-side repack of a weight tensor into the kernel's [tap][k-chunk][n][k] layout. */
int vam_pack_conv_weights(const float* src, float* dst, int mode, int phase,
                          int kh, int kw, int cin, int n, void* stream);
/* bf16-storage mode: weights rounded to nearest-even bf16, [tap][32-channel chunk][N up to 32][32 bf16]. */
size_t vam_conv_wpack_bf16_bytes(int kh, int kw, int cin, int n);
int vam_pack_conv_weights_bf16(const float* src, void* dst, int mode, int phase, int kh, int kw, int cin, int n,
                               void* stream);
/* Many repacks as ONE launch (training refreshes every trained layer's packed weights after every optimiser step).
 * bias != 0: a vam_pack_bias job (kh, kw, cin, phase ignored); else a vam_pack_conv_weights job. */
#define VAM_MAX_PACK_GROUP 32
typedef struct vam_pack_job {
  const float* src;
  void* dst;
  int32_t bias;
  int32_t mode, phase, kh, kw, cin, n;
  int32_t pad_;
} vam_pack_job;
int vam_pack_group(const vam_pack_job* jobs, int n_jobs, void* stream);
/* bias helpers: PS2 permutation / GDN beta reparam (max(b, sqrt(1e-6+2^-36))^2 - 2^-36) /
 * merged-deconv replication (4x). mode as above. */
int vam_pack_bias(const float* src, float* dst, int mode, int n, void* stream);

/* max |x| over up to VAM_MAX_SEG NHWC windows of n_pix pixels each, folded into *cell like vam_conv.out_amax. */
int vam_absmax(const vam_seg* segs, int n_seg, long n_pix, int32_t* cell, void* stream);

/* Launch up to VAM_MAX_GROUP independent problems as ONE grid (grouped launch:
 * e.g. the mean and scale stacks of one slice, or the four phases of a deconv). */
#define VAM_MAX_GROUP 8
int vam_conv_group(const vam_conv* problems, int n_problems, void* stream);
/* Tuning hook: force the tile (BM in {64,128}, BN in {32,...,224}, BK in {16,32}); 0 = automatic. */
int vam_conv_force_tile(int bm, int bn, int bk);
/* Test / measurement hook.  fp32 NHWC outputs normally leave the kernel straight from the accumulator registers
 * ("direct" epilogue); 1 sends every problem through the LDS-staged epilogue instead (the one bf16 / plane / NCHW
 * outputs always take), 0 = automatic, -1 = follow the environment variable VAMPIC_EPILOGUE=staged.  Both epilogues
 * perform the same operations per element: results are bit-identical. */
int vam_conv_force_epilogue(int staged);
/* Arithmetic of the convolution kernel.  1 (default): every fp32 operand is split exactly into three bf16 terms and
 * the product is formed from six exact bf16 x bf16 partial products on the bf16 matrix pipe, fp32 accumulation
 * (error vs float64 no larger than the fp32 fma chain's); 0: fp32 operands on the fp32 matrix pipe;
 * 3 (opt-in, round 3 prototype): every fp32 operand scaled by a power of two (one per launch input, from vam_conv.in_amax;
 * one per output channel of the weights, made at pack time) and split into two fp16 terms, three products on the fp16
 * matrix pipe, fp32 accumulation — 22 of 24 significand bits per operand, below fp32 accumulation noise.
 * The mode fixes the packed-weight layout: choose it (or the environment variable VAMPIC_CONV=f32|bf16x3|f16x2) before
 * the first vam_conv_wpack_floats / vam_pack_conv_weights call and do not change it while packed weights exist. */
int vam_conv_set_mode(int mode);
int vam_conv_get_mode(void);
/* Diagnostics: the (BM, BN, BK) the tile heuristic picked for the most recent vam_conv_group launch. */
int vam_conv_last_tile(int* bm, int* bn, int* bk);
/* What vam_conv_group would do with these problems, without launching: the contract checks and the tile heuristic only.
 * Host arithmetic (no GPU needed): pointers are checked for null and alignment, never dereferenced.  Return codes and
 * vam_last_error texts are vam_conv_group's.  (A forced tile that no kernel is built for is refused at the launch.) */
typedef struct vam_conv_choice {
  int32_t bm, bn, bk, spec;            /* the tile vam_conv_group would launch these problems with   */
  int32_t blocks;                      /* its grid size (8 x the largest per-XCD share)              */
  int32_t dual[VAM_MAX_GROUP];         /* per problem: two taps per 32-channel chunk                 */
  int32_t staged[VAM_MAX_GROUP];       /* per problem: forced onto the LDS-staged epilogue           */
} vam_conv_choice;
int vam_conv_plan(const vam_conv* problems, int n_problems, vam_conv_choice* out);

/* ------------------------------------------------------------------ fused residual unit */
/*
 * One ResidualUnit (reference layers/layers.py:30-48) as ONE launch:
 *   out = GELU( x + conv1x1(GELU(conv3x3(GELU(conv1x1(x))))) )
 * with both C/2-channel intermediates kept in LDS (csrc/resunit.hip).  The weights are the three convolutions'
 * ordinary packed weights (vam_pack_conv_weights, VAM_PACK_CONV, split-operand mode) and biases; results are
 * bit-identical to three vam_conv_group launches.  Built for C = 192 (the 64x64-position attention blocks of
 * g_a / g_s); vam_resunit_supported says whether a shape has a fused kernel — callers fall back to three
 * vam_conv_group launches (the same arithmetic) where it does not.
 */
typedef struct vam_resunit {
  const float* x;           /* input and identity, NHWC fp32 */
  float* out;               /* NHWC fp32, must not alias x   */
  int32_t ldx, ldo;         /* pixel strides (floats)        */
  int32_t B, H, W, C;
  const float* w1; const float* b1;   /* conv[0]: 1x1 C   -> C/2 */
  const float* w2; const float* b2;   /* conv[2]: 3x3 C/2 -> C/2 */
  const float* w3; const float* b3;   /* conv[4]: 1x1 C/2 -> C   */
  int32_t flags;            /* 0, or VAM_RESUNIT_BF16: bf16-storage mode (BASELINE configs[2]) — x / out are bf16 NHWC
                               tensors (ldx / ldo count bf16 elements, multiples of 8), w1..w3 come from
                               vam_pack_conv_weights_bf16, biases stay fp32; bit-identical to three vam_conv_group launches
                               with VAM_CONV_W_BF16 | IN_BF16 | OUT_BF16 [| AUX_BF16] */
  int32_t pad_;
} vam_resunit;
#define VAM_RESUNIT_BF16 1
size_t vam_resunit_struct_size(void);
int vam_resunit_supported(int C, int H, int W);
int vam_resunit_group(const vam_resunit* problems, int n_problems, void* stream);
/* Measurement hook: 1 (default) = weight slabs by LDS-DMA through a three-slot ring, 0 = register-staged (the A/B
 * arm), -1 = follow the environment variable VAMPIC_RU_DMA.  Both are bit-identical. */
int vam_resunit_set_dma(int mode);
/* Measurement hook: device buffer receiving 8 cycle-counter stamps per workgroup at the kernel's phase boundaries
 * (scratch/ru_phases.py); NULL (default) = off. */
int vam_resunit_set_debug(void* stamps);

/* ------------------------------------------------------------------ model edges */
/* x NCHW [B,3,H,W] -> space-to-depth NHWC [B,H/2,W/2,16] (12 real channels (py,px,c), 4 zero)
 * so that conv5x5 s2 (3->N) becomes a 3x3 s1 MFMA problem (layers/layers.py:5-12, builder.py:44). */
int vam_s2d_input(const float* x_nchw, float* out, int B, int H, int W, void* stream);
int vam_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int ld_dst, void* stream);
int vam_nhwc_to_nchw(const float* src, int ld_src, float* dst, int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------ window attention */
/* Swin block core (layers/win_attention.py:84-115,153-207): qkv is [B,H,W,3C] (q|k|v,
 * heads contiguous inside each), out[b,y,x,:] = softmax(q*scale k^T + bias + shiftmask) v
 * written at the un-shifted position; roll/partition/reverse are folded into addressing.
 * table: relative_position_bias_table [(2ws-1)^2][heads].  ws in {4,8}. */
int vam_win_attention(const float* qkv, int ld_qkv, float* out, int ld_out, const float* table,
                      int B, int H, int W, int C, int heads, int ws, int shift, void* stream);
/* 8 x 8 windows run on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: exact fp32 products), forward and backward;
 * vam_attn_set_mfma(0) selects the FMA kernels instead (A/B measurements, equivalence test), -1 = follow the
 * environment variable VAMPIC_ATTN_MFMA.  vam_attn_mfma() returns the mode in force. */
int vam_attn_set_mfma(int mode);
int vam_attn_mfma(void);

/* ------------------------------------------------------------------ variance mask */
/* ChannelMask.forward "point-based-std" (layers/channel_mask.py:132-151) for n_seg
 * independent segments.  Segment s covers, for every pixel p < n_pix, the C channels at
 * sigma + s_b*batch_stride ... ; element (p,c) at sigma[seg_off(s) + p*ld + c].
 *   seg s = b*n_slice + j  ->  seg_off = b*batch_stride + j*slice_stride
 * thr_out[s] receives the fp32 threshold (NaN if the segment holds a NaN, +inf/-inf
 * conventions for pr==0 / pr>=10: mask all 0 / all 1).  mask_out has the layout of sigma
 * (its own ld / strides) and receives 0.0f / 1.0f. pr is the reference's `pr` (0..10+). */
int vam_variance_mask(const float* sigma, int ld, long batch_stride, long slice_stride,
                      int n_batch, int n_slice, int n_pix, int C, double pr,
                      float* mask_out, int ld_mask, long mask_batch_stride, long mask_slice_stride,
                      float* thr_out, void* stream);
/* The masks of n_levels qualities prs[0..n_levels-1] in ONE launch (training forward with quality lists
 * [0, q1, ..., qL], pic.py:425-430 once per level): each segment is loaded once and both order statistics are selected
 * per level.  Level l's mask is written at mask_out + l*mask_level_stride (float 0/1, the layout of vam_variance_mask),
 * its thresholds at thr_out[l*n_batch*n_slice + s].  Bit-identical to n_levels vam_variance_mask calls. */
#define VAM_MAX_MASK_LEVELS 8
int vam_variance_mask_levels(const float* sigma, int ld, long batch_stride, long slice_stride,
                             int n_batch, int n_slice, int n_pix, int C, const double* prs, int n_levels,
                             float* mask_out, int ld_mask, long mask_batch_stride, long mask_slice_stride,
                             long mask_level_stride, float* thr_out, void* stream);
/* Progressive container layers (progressive.encode_batch / ProgressiveDecoder): for a non-decreasing list of
 * n_levels <= VAM_MAX_LAYER_LEVELS qualities, layer_out[e] = the first k with vam_variance_mask(sigma, prs[k])[e] == 1,
 * 0xFF when there is none, so that  layer[e] <= k  <=>  mask_k[e] == 1  (the masks are nested in q).  One uint8 per
 * element in the layout of vam_variance_mask's mask (pixel stride ld_layer, strides in elements); level k's thresholds
 * at thr_out[k*n_batch*n_slice + s] as vam_variance_mask_levels writes them.  One launch: each segment is loaded once,
 * the thresholds are selected level by level with vam_variance_mask_levels' code, and the layer ids are assigned in one
 * pass over the segment. */
#define VAM_MAX_LAYER_LEVELS 32
int vam_variance_layers(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                        int n_pix, int C, const double* prs, int n_levels, uint8_t* layer_out, int ld_layer,
                        long layer_batch_stride, long layer_slice_stride, float* thr_out, void* stream);
/* vam_variance_layers with a quality list PER IMAGE (the later passes of VarianceMaskingPIC.qualities_for_bytes, DESIGN
 * section 9i: every image refines its own bracket).  vam_variance_layer_params is the host arithmetic of one segment size:
 * for image b it turns the non-decreasing list prs[b * levels_stride .. + n_levels[b]) (1 <= n_levels[b] <=
 * VAM_MAX_LAYER_LEVELS) into the rank / weight / mode of every level, what vam_variance_layers computes for its one list,
 * and writes n_batch records of vam_layer_params to table_host.  The caller copies the table to the device (outside any
 * graph capture) and hands it to vam_variance_layers_per_image, which runs the same kernel code with image b's record:
 * the layer ids of image b equal vam_variance_layers on image b alone with prs[b], byte for byte, and its thresholds
 * land at thr_out[k * n_batch * n_slice + b * n_slice + j] for k < n_levels[b] (rows beyond are left alone).  A record
 * whose n_levels is outside 1..VAM_MAX_LAYER_LEVELS makes the kernel skip that image (ids 0xFF). */
typedef struct vam_layer_params {
  int32_t n_levels, any_select;
  int32_t k_lo[VAM_MAX_LAYER_LEVELS], k_hi[VAM_MAX_LAYER_LEVELS];
  float w[VAM_MAX_LAYER_LEVELS];
  int32_t mode[VAM_MAX_LAYER_LEVELS];
} vam_layer_params;
size_t vam_layer_params_size(void);
int vam_variance_layer_params(const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix, int C,
                              vam_layer_params* table_host);
int vam_variance_layers_per_image(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                  int n_slice, int n_pix, int C, const vam_layer_params* table_dev, uint8_t* layer_out,
                                  int ld_layer, long layer_batch_stride, long layer_slice_stride, float* thr_out,
                                  void* stream);
/* vam_variance_mask_levels with a quality list PER IMAGE, read from a device table (one captured graph then serves every
 * quality vector: the qualities are graph inputs).  vam_variance_mask_params is vam_variance_layer_params
 * for these lists: 1 <= n_levels[b] <= VAM_MAX_MASK_LEVELS qualities per image, in any order, repeats allowed.  The kernel
 * writes level l of image b at mask_out + l*mask_level_stride + b*mask_batch_stride + j*mask_slice_stride (float 0/1) and
 * its threshold at thr_out[l*n_batch*n_slice + b*n_slice + j], for l < n_levels[b]; rows beyond an image's count are left
 * alone.  max_levels = the levels mask_out and thr_out hold (1..VAM_MAX_MASK_LEVELS): a record with more writes nothing.
 * Mask and threshold of every (b, l) equal vam_variance_mask on image b alone with that quality, bit for bit. */
int vam_variance_mask_params(const double* prs, const int* n_levels, int n_batch, int levels_stride, int n_pix, int C,
                             vam_layer_params* table_host);
int vam_variance_masks_per_image(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch,
                                 int n_slice, int n_pix, int C, const vam_layer_params* table_dev, int max_levels,
                                 float* mask_out, int ld_mask, long mask_batch_stride, long mask_slice_stride,
                                 long mask_level_stride, float* thr_out, void* stream);
/* Quality maps (VarianceMaskingPIC.forward_quality_map): ONE float mask in which every latent pixel
 * takes its own quality.  table_dev: the records of vam_variance_layer_params (image b's non-decreasing list of
 * 1..VAM_MAX_LAYER_LEVELS qualities); level_map[b * map_batch_stride + p] (uint8, p < n_pix): the index of pixel p's
 * quality in image b's list.  The kernel of vam_variance_layers_per_image selects every level's threshold once per
 * segment, then writes, for every slice j, pixel p and channel c,
 *   mask_out[b, j, p, c] = vam_variance_mask(sigma of image b alone, prs[b][level_map[b, p]])[j, p, c]
 * bit for bit (float 0/1, the layout and strides of vam_variance_mask): all zero where the quality is 0, all one where
 * it is >= 10 (even in a segment that holds a NaN), zero in a NaN segment wherever the level needs the threshold.  A map
 * entry >= the image's n_levels writes 0 at that pixel; a record whose n_levels is outside 1..VAM_MAX_LAYER_LEVELS makes
 * the kernel write 0 for the whole image.  Level k's thresholds land at thr_out[k * n_batch * n_slice + b * n_slice + j]
 * for k < n_levels[b], as vam_variance_layers_per_image writes them.  Table and map are device buffers: the call can be
 * captured, and the captured graph serves every map. */
int vam_variance_mask_map(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice,
                          int n_pix, int C, const vam_layer_params* table_dev, const uint8_t* level_map,
                          long map_batch_stride, float* mask_out, int ld_mask, long mask_batch_stride,
                          long mask_slice_stride, float* thr_out, void* stream);

/* ------------------------------------------------------------------ rank order (embedded streams) */
/* Embedded streams (vampic.embedded).  A segment is one (image, slice) of the NHWC window that
 * vam_variance_layers reads (segment s = b*n_slice + j at sigma + b*batch_stride + j*slice_stride, n = n_pix * C elements,
 * element (p, c) at p*ld + c); its elements carry the canonical index e = c * n_pix + p, the [C, h, w] order of a stream.
 * vam_variance_rank writes perm_out[s][0 .. n) (int32), the permutation that sorts the segment by descending sigma:
 *   perm[s] == numpy.argsort(-sigma_s, kind="stable")   with sigma_s flattened in canonical order,
 * i.e. equal values by ascending e, -0.0 == +0.0, +inf first, NaN last (the NaNs again by e).  The variance mask of every
 * quality is a prefix of this order.  Segments of up to 8192 elements are sorted in LDS in one launch; larger ones (up to
 * 2^18 elements, anything above is VAM_EINVAL and launches nothing) in several passes through `workspace`, whose size
 * vam_variance_rank_workspace gives (0 when none is needed).  No allocation, no atomics: the call can be captured. */
size_t vam_variance_rank_workspace(int n_batch, int n_slice, int n_pix, int C);
int vam_variance_rank(const float* sigma, int ld, long batch_stride, long slice_stride, int n_batch, int n_slice, int n_pix,
                      int C, int32_t* perm_out, void* workspace, size_t workspace_bytes, void* stream);
/* out[s][r] = in[b, p, j*C + c] for e = c * n_pix + p = perm[s][r]: one or two contiguous int32 NHWC views (pixel strides
 * ld0 / ld1 >= n_slice * C, n_batch * n_pix pixels; in1 / out1 may be NULL) into rank order in one launch. */
int vam_rank_gather(const int32_t* in0, int ld0, const int32_t* in1, int ld1, const int32_t* perm, int n_batch, int n_slice,
                    int n_pix, int C, int32_t* out0, int32_t* out1, void* stream);
/* count_out[g][s] = #(layer id <= g) of segment s for the uint8 ids of vam_variance_layers (pixel stride ld_layer) and
 * g < n_levels <= VAM_MAX_LAYER_LEVELS: the length of the prefix of perm[s] that quality g's mask keeps.  The ids never
 * decrease along the rank order, so this is one binary search per (segment, level). */
int vam_rank_counts(const uint8_t* layer, int ld_layer, const int32_t* perm, int n_batch, int n_slice, int n_pix, int C,
                    int n_levels, int32_t* count_out, void* stream);
/* The decoder's inverse: ranked[s][r] int32, perm, and a device table count[g][s] (int32, non-decreasing in g,
 * 1 <= n_levels <= VAM_MAX_MASK_LEVELS).  For e = perm[s][r]:  sym_out[e] = ranked[r] if r < count[n_levels-1][s] else 0,
 * id_out[e] (uint8) = the smallest g with r < count[g][s], 0xFF if there is none, both in the NHWC layout of the views
 * above: what vam_gauss_levels_decode reads with ks = 0 .. n_levels-1.  The table is read on the device, so one captured
 * launch serves every cut. */
int vam_rank_scatter(const int32_t* ranked, const int32_t* perm, const int32_t* count, int n_levels, int n_batch, int n_slice,
                     int n_pix, int C, int32_t* sym_out, int ld_sym, uint8_t* id_out, int ld_id, void* stream);
/* Scheduled embedded streams.  A schedule is 1..VAM_MAX_LAYER_LEVELS quality maps per image that never
 * decrease from stage to stage at any pixel; image b's sorted distinct values are the list of its vam_layer_params record
 * and stage_map[b][k][p] (uint8, [n_batch][VAM_MAX_LAYER_LEVELS][n_pix]) is the index of stage k's quality at pixel p in
 * that list.  For the layer ids of vam_variance_layers_per_image on that table (uint8, n_batch * n_pix pixels of C_total
 * channels, pixel stride ld_layer) vam_stage_ids writes, in the same layout (pixel stride ld_out),
 *   stage_out[e] = min{k < n_stages[b] : stage_map[b][k][p] >= layer[e]},  0xFF when there is none,
 * so that  stage[e] <= k  <=>  vam_variance_mask_map of stage k's map holds e.  n_stages (int32 [n_batch]) and the maps
 * are read on the device: one captured launch serves every schedule.  An image whose n_stages is outside
 * 1..VAM_MAX_LAYER_LEVELS gets 0xFF everywhere.
 * vam_variance_rank_staged is vam_variance_rank with that id (slice j's channels at j*C, pixel stride ld_stage) as the
 * major key: ascending stage, within a stage vam_variance_rank's order,
 *   o = numpy.argsort(-sigma_s, kind="stable");  perm[s] == o[numpy.argsort(stage_s[o], kind="stable")].
 * Same network, chunks, workspace (vam_variance_rank_workspace) and passes.  The ids never decrease along this order, so
 * vam_rank_counts on them gives #(stage <= k), and vam_rank_gather / vam_rank_scatter take the permutation as it is. */
int vam_stage_ids(const uint8_t* layer, int ld_layer, const uint8_t* stage_map, const int32_t* n_stages, int n_batch, int n_pix,
                  int C_total, uint8_t* stage_out, int ld_out, void* stream);
int vam_variance_rank_staged(const float* sigma, int ld, long batch_stride, long slice_stride, const uint8_t* stage,
                             int ld_stage, int n_batch, int n_slice, int n_pix, int C, int32_t* perm_out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ pooled selection (picture-wide marks) */
/* Picture-wide quality marks of tiled pictures (vampic.tiled).  The pool of slice j is the multiset of
 * the T * n sigmas of slice j of all T tiles of a picture; quality q's threshold is torch.quantile(pool_j, float32(1 - 0.1 q))
 * with vam_variance_mask's arithmetic at N = T * n, bit for bit.  keys is uint32 [T][n_slice][n] on the device.
 * vam_pool_keys: for the n_batch tiles of the window vam_variance_rank read (same sigma, strides and perm), row
 *   (t0 + b, j) gets the segment's sigmas in rank order as keys that ascend as sigma descends, with vam_variance_rank's
 *   canonicalisation: -0.0 == +0.0, every NaN the key 0xFFFFFFFF, last.  An entry of perm outside [0, n) writes that key.
 * vam_pooled_select: thr_out[k][j] (fp32 [n_levels][n_slice]) for the non-decreasing qualities prs[k] > 0, 1 <= n_levels <=
 *   VAM_MAX_LAYER_LEVELS.  Every row of keys must be sorted (vam_pool_keys of a rank order is).  q >= 10 stores -inf; a NaN
 *   anywhere in pool_j stores NaN.  One workgroup per (slice, level) descends the 32 key bits; nothing waits across
 *   workgroups.  A pool above 16 000 000 elements is VAM_EINVAL, as torch.quantile refuses it.
 * vam_threshold_counts: count_out[k][t][j] (int32 [n_levels][T][n_slice]) = #{r : sigma(keys[t][j][r]) >= thr[k][j]}, compared
 *   as floats (a NaN threshold counts 0); a threshold of -inf counts n.  thr is read on the device.
 * No allocation, no atomics: all three can be captured.  Bad arguments are VAM_EINVAL and launch nothing. */
int vam_pool_keys(const float* sigma, int ld, long batch_stride, long slice_stride, const int32_t* perm, int n_batch,
                  int n_slice, int n_pix, int C, uint32_t* keys, int t0, int T, void* stream);
int vam_pooled_select(const uint32_t* keys, int T, int n_slice, int n, const double* prs, int n_levels, float* thr_out,
                      void* stream);
int vam_threshold_counts(const uint32_t* keys, int T, int n_slice, int n, const float* thr, int n_levels, int32_t* count_out,
                         void* stream);

/* ------------------------------------------------------------------ tiled pictures */
/* Tiled pictures (vampic.tiled).  A picture of H x W (any sizes >= 1) is covered by tiles of th x tw with
 * overlap V, 0 <= 2 V <= min(th, tw): strides Sy = th - V and Sx = tw - V, grid R = max(1, ceil((H - V) / Sy)) by
 * C = max(1, ceil((W - V) / Sx)), tile (r, c) over rows [r Sy, r Sy + th) and columns [c Sx, c Sx + tw).  Both calls derive
 * R and C from (H, W, th, tw, V); a geometry outside these bounds is VAM_EINVAL and launches nothing.
 * vam_tile_extract: image fp32 [3, H, W], coords int32 [n][2] = (r, c) on the device, out fp32 [n, 3, th, tw] with
 *   out[i, :, y, x] = image[:, min(r Sy + y, H - 1), min(c Sx + x, W - 1)]      (the edge is replicated);
 * an (r, c) outside the grid leaves its tile unwritten.  One launch for the whole list.
 * vam_tile_blend: tiles fp32 [n, 3, th, tw], slot int32 [R][C] (index into tiles, -1: absent), the ramps w_lo / w_hi fp32 [V]
 * (NULL allowed for V = 0), a window y0, x0, h, w inside the picture.  Along an axis pixel P lies in tile
 * t1 = min(n_tiles - 1, P / S) at l1 = P - t1 S with weight 1, or, when t1 > 0 and l1 < V, in t1 with w_hi[l1] and in t1 - 1
 * with w_lo[l1].  out = sum over the pixel's tiles, ascending r and within that ascending c, of (wy * wx) * v, every product
 * and add one fp32 operation, the sum starting from its first term: fp32 [3, h, w] (out_u8 = 0) or uint8 [h, w, 3]
 * (out_u8 = 1) as rintf(clamp(v, 0, 1) * 255).  A pixel that needs an absent tile (a slot outside 0 .. n - 1) sets
 * *status = 1 and skips that term; the caller clears status.  No atomics, no allocation: both calls can be captured.
 * vam_tile_schedule: maps fp32 [L, H, W], a picture-wide schedule of 1 <= L <= VAM_MAX_LAYER_LEVELS quality
 * maps at pixel resolution, the coords of vam_tile_extract, th and tw multiples of 16, out fp32 [n, L, th / 16, tw / 16] with
 *   out[i, k, a, b] = max over y, x in [0, 16) of maps[k, min(r Sy + 16 a + y, H - 1), min(c Sx + 16 b + x, W - 1)]:
 * the block maximum of a latent cell over the tile's replicated pixels; a NaN anywhere in the block gives NaN.  An (r, c)
 * outside the grid leaves its rows unwritten.  n L <= 65535 per launch.  No atomics, no allocation, capturable.
 * vam_tile_refresh: vam_tile_blend restricted to what changed.  out is a persistent canvas of the window
 * cy0, cx0, ch, cw of the picture: fp32 [3, ch, cw] (out_u8 = 0) or uint8 [ch, cw, 3] (out_u8 = 1).  dirty int32 [R][C] on the
 * device marks tiles (non-zero: dirty); y0, x0, h, w, in picture coordinates, is the box to visit inside the canvas window.  Per
 * pixel of the box: when none of its 1, 2 or 4 tiles is dirty it is not written and its tiles' slots are not read (they may
 * be absent); otherwise all of its tiles must be present (else *status = 1, as vam_tile_blend) and it gets vam_tile_blend's
 * value, bit for bit.  Pixels outside the box are never touched.  A canvas window outside the picture, a box outside the
 * canvas window and a box of more than 4 * 65535 rows are VAM_EINVAL and launch nothing.  No atomics, no allocation,
 * capturable.
 * vam_tile_compose: vam_tile_blend of a window of pyramid level k whose tiles have not all arrived.  A
 * tile is available when its slot is >= 0; a pixel is sharp exactly when every tile vam_tile_blend would sum there (1, 2 or 4)
 * is available, and it gets vam_tile_blend's value, bit for bit (an available slot >= n sets *status = 1 and skips the term,
 * as there).  Any other pixel reads none of its tiles and is the upsample of `below`, fp32 [3, hb, wb]: the window by0, bx0, hb,
 * wb of the picture of level j = k + d, Hj x Wj with Hj = ceil(H / 2^d), Wj = ceil(W / 2^d), 1 <= d <= 15.  For row Y:
 * n = 2 Y + 1 - 2^d, a = floor(n / 2^(d+1)), fy = float(n - a 2^(d+1)) / 2^(d+1) (exact, never 0 or 1), the source rows
 * r0 = clamp(a, 0, Hj - 1) and r1 = clamp(a + 1, 0, Hj - 1); columns likewise; with lerp(p, q, f) = p + f * (q - p), a subtract,
 * a multiply and an add in fp32 that nothing contracts,
 *   out = lerp(lerp(s[r0][c0], s[r0][c1], fx), lerp(s[r1][c0], s[r1][c1], fx), fy):
 * a constant stays constant bit for bit, the replicated edge is exact.  Only finite inputs are specified.  The switch between
 * sharp and filled pixels is hard.  slot = NULL with n = 0 means no tiles: every pixel comes from below; tiles, the ramps, th,
 * tw, V and status are then not looked at.  The value does not depend on the path a lane takes.  VAM_EINVAL, nothing launched:
 * a null below or out, d outside 1 .. 15, an Hj or Wj that is not ceil(. / 2^d), a window of below that does not lie inside
 * the level or does not cover the window's sources (rows clamp(a(y0)) .. clamp(a(y0 + h - 1) + 1), columns likewise), and
 * everything vam_tile_blend refuses.  No atomics, no allocation, capturable. */
int vam_tile_compose(const float* tiles, int n, const int32_t* slot, const float* w_lo, const float* w_hi, int H, int W, int th,
                     int tw, int V, int y0, int x0, int h, int w, const float* below, int by0, int bx0, int hb, int wb, int Hj, int Wj,
                     int d, void* out, int out_u8, int32_t* status, void* stream);
int vam_tile_extract(const float* image, int H, int W, int th, int tw, int V, const int32_t* coords, int n, float* out,
                     void* stream);
int vam_tile_blend(const float* tiles, int n, const int32_t* slot, const float* w_lo, const float* w_hi, int H, int W, int th,
                   int tw, int V, int y0, int x0, int h, int w, void* out, int out_u8, int32_t* status, void* stream);
int vam_tile_schedule(const float* maps, int L, int H, int W, int th, int tw, int V, const int32_t* coords, int n, float* out,
                      void* stream);
int vam_tile_refresh(const float* tiles, int n, const int32_t* slot, const int32_t* dirty, const float* w_lo, const float* w_hi,
                     int H, int W, int th, int tw, int V, int cy0, int cx0, int ch, int cw, int y0, int x0, int h, int w, void* out,
                     int out_u8, int32_t* status, void* stream);

/* Resolution pyramids (vampic.pyramid).  Level 0 is the picture; level k >= 1 has
 * H_k = ceil(H_{k-1} / 2) rows and W_k = ceil(W_{k-1} / 2) columns.  vam_picture_halve makes one level from the one below:
 * src fp32 [C, Hs, Ws] contiguous, dst fp32 [C, ceil(Hs / 2), ceil(Ws / 2)], 1 <= C <= VAM_MAX_LAYER_LEVELS (3 for a picture,
 * L for a schedule), 1 <= Hs, Ws <= 2^24.  With y1 = min(2y + 1, Hs - 1) and x1 = min(2x + 1, Ws - 1) (the edge is replicated)
 *   mode 0 (mean): dst[c][y][x] = ((src[c][2y][2x] + src[c][2y][x1]) + (src[c][y1][2x] + src[c][y1][x1])) * 0.25f,
 *                  every add and the multiply one fp32 operation, in exactly this order; nothing is contracted;
 *   mode 1 (max):  dst[c][y][x] = max(max(src[c][2y][2x], src[c][2y][x1]), max(src[c][y1][2x], src[c][y1][x1])), where
 *                  max(p, q) is p when p >= q and q otherwise (of +0 and -0 the first), and a NaN among the four gives NaN,
 *                  as vam_tile_schedule's block maximum does.
 * NaN and +-inf propagate as the arithmetic gives them; a NaN result is stored as the quiet NaN 0x7FC00000 (which NaN
 * inf - inf makes differs between processors, so its bits are pinned).  The value does not depend on the path a lane takes
 * (16-byte loads where all eight source columns lie inside the row and both row addresses are 16-byte aligned, single loads
 * with the clamped column otherwise).  One launch per level, rows split over two grid dimensions; no atomics, no allocation:
 * it can be captured.  Null pointers, C outside 1 .. VAM_MAX_LAYER_LEVELS, a side outside 1 .. 2^24, a mode other than 0
 * or 1 and a problem of 2^32 threads or more are VAM_EINVAL and launch nothing. */
int vam_picture_halve(const float* src, int C, int Hs, int Ws, float* dst, int mode, void* stream);

/* Pyramid viewports (vampic.pyramid): the rect (y0, x0, h, w) / unit of the picture, in level-0 pixels
 * divided by the integer unit (1 .. 256), resampled from level k = shift (0 .. 15) into oh x ow pixels (1 .. 65536 each), at any
 * zoom and pan, with a tent filter of half-width max(1, scale) level-k pixels.  src is fp32 [C, hs, ws], the window sy0, sx0, hs,
 * ws of the level's picture of Hk x Wk; out is fp32 [C, oh, ow] (out_u8 = 0) or, for C = 3, uint8 [oh, ow, 3] by vam_tile_blend's
 * rule (out_u8 = 1).  Along the rows (the columns likewise, with x0, w, ow, Wk), output row Y has its centre at n / D of level k,
 * pixel i being centred at i + 1/2 on both sides:
 *   D = 2^(k+1) oh unit,  n = 2 oh y0 + (2 Y + 1) h - 2^k oh unit,  T = max(D, 2 h);
 * its taps are the integers i with |D i - n| < T, of integer weight u_i = T - |D i - n| > 0 and fp32 weight
 * float(u_i) / float(S), S = sum u_i (two round-to-nearest conversions, one correctly rounded division), read at
 * clamp(i, 0, Hk - 1): the edge is replicated.  The scale is h / (oh unit 2^k); up to 2 there are at most 4 taps, within
 * floor(n / D) - 1 .. floor(n / D) + 2; up to 16, the limit, at most 32.  The value is
 *   sum over the row taps r of wy_r * (sum over the column taps c of wx_c * src[r][c]),
 * taps ascending, each sum starting from its first term, every multiply and add one fp32 operation that nothing contracts.
 * Only finite inputs are specified.  The kernel derives taps and weights from these integers in the thread: nothing is uploaded
 * per call.  The value does not depend on the path a lane takes (16-byte stores where aligned, scalar otherwise; at most 4 taps
 * per axis unrolled, with cached reads or, at column scales of 1.9 .. 2, the source staged in LDS; more in a bounded loop).  The picture is known here through its level: the rect / unit must lie inside
 * min(Hk 2^k, 2^24) x min(Wk 2^k, 2^24).  src must cover the support window, rows clamp(first tap of Y = 0) ..
 * clamp(last tap of Y = oh - 1) and columns likewise, so that every index formed lies inside it.  VAM_EINVAL, nothing launched:
 * a null src or out, C outside 1 .. VAM_MAX_LAYER_LEVELS, out_u8 other than 0 or 1 or 1 with C != 3, unit, oh, ow or shift out
 * of range, an Hk x Wk that is the level of no picture with sides 1 .. 2^24, a rect outside the picture, a window of src
 * outside the level or not covering the support window, and a scale above 16 on either axis (the message names the level
 * that would do).  No atomics, no allocation, capturable. */
int vam_picture_resample(const float* src, int C, int sy0, int sx0, int hs, int ws, int Hk, int Wk, int shift, int64_t y0, int64_t x0,
                         int64_t h, int64_t w, int unit, int oh, int ow, void* out, int out_u8, void* stream);

/* ------------------------------------------------------------------ Gaussian conditional */
/* Fused slice tail (models/pic.py:545-546,625-629; entropy_models.py:620-652).
 *  base  (mask == NULL):  v = round(y-mu);           lik = L(|(v+mu)-mu|, sigma);        yhat = v+mu
 *  prog  (mask != NULL):  r = y - ybase_raw; v = round(r-mu); in = (r-mu)*m;
 *                         lik = L(|round(in)|, sigma*m);   yhat = v*m + mu
 * Each tensor is a [n_pix, C] channel window with its own pixel stride. y2 (may be NULL)
 * is subtracted from y first (delta_encode, pic.py:583-584).
 * log2sum (may be NULL): per-batch-item sum of log2(lik) accumulated atomically
 * (pix_per_item pixels per item) — cleared by the caller.
 * sym (may be NULL): int32 quantised symbols (v, or v*m) for the entropy coder. */
int vam_gauss_tail(const float* y, int ld_y, const float* y2, int ld_y2,
                   const float* mu, int ld_mu, const float* sigma, int ld_sigma,
                   const float* mask, int ld_mask,
                   float* yhat, int ld_yhat, float* lik, int ld_lik,
                   int32_t* sym, int ld_sym, double* log2sum, int pix_per_item,
                   long n_pix, int C, void* stream);
/* Rate sweep (VarianceMaskingPIC.forward_qualities): the evaluation tail of n_levels masks over ONE
 * shared (y, y2, mu, sigma) window.  With all_scalable every quality shares the progressive (mu, sigma) chain, so only
 * the mask differs between levels.  y, y2, mu and sigma are loaded once per element; level l's mask, yhat, lik and sym
 * live at their base pointer + l * <name>_ls floats (ints), each with its own pixel stride.  Per level the prog branch
 * of vam_gauss_tail: yhat_l = round(r-mu)*m_l + mu, lik_l = L(|round((r-mu)*m_l)|, sigma*m_l), sym_l = round((r-mu)*m_l)
 * — bit-identical to vam_gauss_tail called once per level.  log2sum (may be NULL): level l's per-item sum of log2(lik_l)
 * is accumulated at log2sum[l * (n_pix / pix_per_item) + item] (fp64 atomics, cleared by the caller).  yhat, lik and sym
 * may be NULL. */
int vam_gauss_levels_eval(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                          const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls,
                          float* yhat, int ld_yhat, long yhat_ls, float* lik, int ld_lik, long lik_ls,
                          int32_t* sym, int ld_sym, long sym_ls, double* log2sum, int pix_per_item, int n_levels,
                          long n_pix, int C, void* stream);
/* The decoder's counterpart (ProgressiveDecoder): from the int32 symbols decoded so far and the layer ids of
 * vam_variance_layers, level l's quantised latents yhat_l = float(sym) * m_l + mu with m_l = (layer <= k_l), through
 * masked_tail's expression; k_l = ks[l] (n_levels <= VAM_MAX_MASK_LEVELS cut-offs).  yhat_l lives at yhat + l * yhat_ls,
 * the eval kernel's layout.  Fed the q = 10 symbols round(r - mu), bit-identical to vam_gauss_levels_eval's yhat. */
int vam_gauss_levels_decode(const int32_t* sym, int ld_sym, const uint8_t* layer, int ld_layer, const float* mu, int ld_mu,
                            const int* ks, int n_levels, float* yhat, int ld_yhat, long yhat_ls, long n_pix, int C,
                            void* stream);

/* Rate control (VarianceMaskingPIC.rate_curve / qualities_for_bpp): the rate of up to
 * VAM_MAX_LAYER_LEVELS qualities from ONE pass over the progressive windows vam_gauss_levels_eval reads, with the layer
 * ids of vam_variance_layers in place of masks.  Per element lk = L(|round(r-mu)|, sigma), r = y - y2: masked_tail /
 * gauss_lik with m = 1, the float vam_gauss_levels_eval gets for an element INSIDE a mask, bit for bit.  Per item
 * (pix_per_item consecutive pixels; it must divide n_pix):
 *   bits [item * (n_levels+1) + k] += sum of log2((double)lk) over the item's elements with layer == k   (fp64)
 *   count[item * (n_levels+1) + k] += the number of such elements
 * for k < n_levels; slot n_levels takes layer == 0xFF (and any id >= n_levels).  Both ACCUMULATE (fp64 / 64-bit atomics)
 * and are cleared by the caller, as log2sum is.  An element outside a mask contributes the constant log2 L(0, 0) at
 * every quality, so the list's level k sums to  sum_{j<=k} bits_j + (n - sum_{j<=k} count_j) * log2 L(0, 0);  the
 * constant is what this call writes to bits[0] for one element with y = mu = sigma = 0 and layer 0.  Each tensor is
 * read once, nothing else is written; no float32 accumulation.  layer: one uint8 per element, pixel stride ld_layer
 * (a multiple of 4, 4-byte aligned); y, y2 (may be NULL), mu, sigma as in vam_gauss_levels_eval. */
int vam_gauss_layer_bits(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const uint8_t* layer, int ld_layer, int n_levels,
                         double* bits, long long* count, int pix_per_item, long n_pix, int C, void* stream);

/* Coded-size control (VarianceMaskingPIC.coded_size_curve / qualities_for_bytes, progressive.container_sizes; DESIGN
 * section 9i): what the range coder of csrc/rans.cpp charges for every element, binned like vam_gauss_layer_bits but per
 * STREAM.  The coder's tables on the device: cost[t * stride + v] = 16 - log2(cdf[t][v+1] - cdf[t][v]) in float64 for
 * v <= sizes[t] - 2 (entry sizes[t] - 2 is the escape), built once on the host from the int32 CDFs (bitstream.py). */
typedef struct vam_coder_tables {
  const double* cost;       /* device [n_cdfs][stride] */
  const int32_t* sizes;     /* device [n_cdfs]: cdf lengths, as the coder takes them */
  const int32_t* offsets;   /* device [n_cdfs] */
  int32_t n_cdfs, stride;
} vam_coder_tables;
/* Per element of the windows vam_gauss_layer_bits reads: the symbol round(r - mu) (masked_tail with m = 1) and the table
 * index of sigma (the arithmetic of vam_build_indexes on scale_table[n_table], n_table <= n_cdfs) — bit for bit the pair
 * compress / encode_batch hand to the coder for an element inside the mask — and that pair's exact price in bits:
 * cost[index][v] for v = symbol - offset inside the table, else the escape entry plus 4 * (1 + n_bypass) with n_bypass
 * <= 8 raw nibbles (enc_put_bits).  A stream is chans_per_stream consecutive channels of one item (it divides C):
 *   bits [(item * (C / chans_per_stream) + slice) * (n_levels+1) + k] += the prices of the elements with layer == k (fp64)
 *   count[ same ] += their number
 * slot n_levels takes 0xFF (and any id >= n_levels); layer == NULL: every element is layer 0.  Both ACCUMULATE and are
 * cleared by the caller.  No float32 accumulation.  An index outside [0, n_cdfs) prices as NaN. */
int vam_coded_layer_bits(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const uint8_t* layer, int ld_layer, int n_levels,
                         const float* scale_table, int n_table, const vam_coder_tables* tables, int chans_per_stream,
                         double* bits, long long* count, int pix_per_item, long n_pix, int C, void* stream);
/* The symbol-input form: int32 symbols with int32 table indexes (idx == NULL: index = idx_base + channel, the entropy
 * bottleneck's per-channel tables), same bins.  Prices z, and the slices of a symbols-mode plan. */
int vam_coded_symbol_bits(const int32_t* sym, int ld_sym, const int32_t* idx, int ld_idx, int idx_base,
                          const uint8_t* layer, int ld_layer, int n_levels, const vam_coder_tables* tables,
                          int chans_per_stream, double* bits, long long* count, int pix_per_item, long n_pix, int C,
                          void* stream);

/* GaussianConditional.build_indexes (entropy_models.py:654-659): idx = 63 - #{i<63: max(s,.11) <= T_i}
 * table: 64 floats (device). mask (may be NULL) multiplies sigma first (pic.py:809). */
int vam_build_indexes(const float* sigma, int ld_sigma, const float* mask, int ld_mask,
                      const float* table, int n_table, int32_t* idx, int ld_idx,
                      long n_pix, int C, void* stream);

/* EntropyBottleneck eval forward (entropy_models.py:403-436,449-492) on z NHWC [n_pix, C]:
 * zhat = round(z-med)+med ; sym (may be NULL) = round(z-med) ; lik = |sigmoid(s*upper)-sigmoid(s*lower)| clamped at 1e-9.
 * params: the 15 tensors _matrix0.._4,_bias0.._4,_factor0.._3 and quantiles as stored in the
 * state_dict, concatenated per tensor (see INTEGRATION.md for the order), C channels. */
int vam_eb_forward(const float* z, int ld_z, const float* params, int C,
                   float* zhat, int ld_zhat, float* lik, int ld_lik, int32_t* sym, int ld_sym,
                   double* log2sum, int pix_per_item, long n_pix, void* stream);
/* Training variant: z_hat is still round(z-med)+med (pic.py:282-284) but the likelihood is evaluated at
 * z + noise (additive-uniform proxy, entropy_models.py:132-138,471-473).  noise == NULL: identical to
 * vam_eb_forward. */
int vam_eb_forward_noise(const float* z, int ld_z, const float* params, int C, float* zhat, int ld_zhat,
                         float* lik, int ld_lik, int32_t* sym, int ld_sym, double* log2sum, int pix_per_item,
                         long n_pix, const float* noise, int ld_noise, void* stream);
/* EntropyBottleneck.loss (entropy_models.py:398-401; models/base.py:22-29 aux_loss): loss[0] (device double) =
 * sum_{c,k} |logits_cumulative(quantiles[c,k]) - target[k]| with the density network held constant (stop_gradient),
 * dquantiles[c*3+k] = d loss / d quantiles[c,k].  params as for vam_eb_forward; target3_host: 3 HOST floats. */
int vam_eb_aux_loss(const float* params, int C, const float* target3_host, double* loss, float* dquantiles, void* stream);
/* EntropyModel.dequantize (entropy_models.py:161-168): out = float(sym) + mu (mu may be NULL). */
int vam_dequantize(const int32_t* sym, int ld_sym, const float* mu, int ld_mu, float* out, int ld_out,
                   long n_pix, int C, void* stream);

/* out[p, c] = a[p, c] + b[p, c]   (channel windows) — mu_total = mu + yhat_base (pic.py:603) */
int vam_add(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out,
            long n_pix, int C, void* stream);
/* Zero-fill KERNEL on the stream (ptr and bytes multiples of 4): accumulators are cleared inside the captured graph, where
 * every node is a kernel node */
int vam_memset_zero(void* ptr, size_t bytes, void* stream);
/* sum((a-b)^2) accumulated in double into acc[0] (PSNR, utility/functions.py:172-174) */
int vam_sqdiff_sum(const float* a, const float* b, long n, double* acc, void* stream);
/* Rate sweep distortion: x [B, n] and xhat [n_levels * B, n] (level l = images l*B .. l*B+B-1, n = 3*H*W floats per image);
 * out[l * B + b] += sum_i (x[b, i] - xhat[l*B + b, i])^2 in double (the arithmetic of vam_sqdiff_sum).  x is read once per
 * element for up to 16 levels (one launch per 16 levels).  out is cleared by the caller. */
int vam_sqdiff_sum_levels(const float* x, const float* xhat, int B, long n, int n_levels, double* out, void* stream);

/* ------------------------------------------------------------------ MS-SSIM pieces (utility/functions.py:176-177) */
/* One SSIM level over `planes` contiguous HxW planes (NCHW): 11-tap Gaussian window `win11` applied to x, y, x^2, y^2, xy
 * at the (H-10)x(W-10) valid positions; ADDS the per-plane sums of the ssim map and of the cs map to ssim_sum / cs_sum
 * (device doubles, one per plane; zero them first).  c1 = (0.01 L)^2, c2 = (0.03 L)^2. */
int vam_ssim_level(const float* x, const float* y, int planes, int H, int W, const float* win11, float c1, float c2,
                   double* ssim_sum, double* cs_sum, void* stream);
/* F.avg_pool2d(kernel 2, stride 2, padding (pad_h, pad_w) in {0,1}, padded zeros counted): out is
 * [planes][(H+2ph-2)/2+1][(W+2pw-2)/2+1]. */
int vam_avgpool2(const float* x, float* out, int planes, int H, int W, int pad_h, int pad_w, void* stream);

/* ------------------------------------------------------------------ differentiable MS-SSIM distortion */
/* The training loss 1 - MS-SSIM: the function of oracle/msssim_oracle.py per plane = (image, channel), V = prod_l
 * relu(m_l)^w_l, with the gradient with respect to y (the reconstruction).  Planes are contiguous HxW fp32 (NCHW); the
 * smaller side must exceed 160.  Every launch goes to `stream`, nothing synchronises, and no reduction uses atomics: a
 * replay gives the same bits.  A plane with any m_l <= 0 has V = 0 and gradient exactly 0 (pytorch_msssim's expression can give NaN there).
 *
 * Scratch: one double per forward workgroup, levels concatenated, [plane][tile] within a level.
 * vam_msssim_partial_doubles: size of the scratch for `planes` HxW planes (0: too small an image);
 * vam_msssim_partial_offset: first double of `level` (0..4) in it (-1: bad arguments). */
long vam_msssim_partial_doubles(int planes, int H, int W);
long vam_msssim_partial_offset(int planes, int H, int W, int level);
/* One level's forward on its HxW planes: 11-tap window `win11` (device), cs map (last = 0) or ssim map (last = 1) summed
 * per workgroup in double into partial[plane * tiles + tile] (partial = scratch + vam_msssim_partial_offset(level)). */
int vam_msssim_fwd_level(const float* x, const float* y, int planes, int H, int W, const float* win11, float c1, float c2,
                         int last, double* partial, void* stream);
/* avg_pool2d(kernel 2, padding = size % 2, zeros counted) of x and y in one launch: outputs [planes][Ho][Wo] with
 * Ho = (H + 2 (H % 2) - 2) / 2 + 1. */
int vam_msssim_pool2(const float* x, const float* y, float* x_out, float* y_out, int planes, int H, int W, void* stream);
/* From the scratch of the five levels of B images x C channels of H x W (level 0): means[l * B*C + plane] = m_l,
 * dvdm[l * B*C + plane] = w_l V / m_l (0 for a plane with any m_l <= 0), val[b] = mean_c V (double), val32[b] the same
 * in float.  Partials are summed in a fixed order. */
int vam_msssim_combine(const double* partial, int B, int C, int H, int W, double* means, double* dvdm, double* val, float* val32,
                       void* stream);
/* One level's backward, coarse to fine: g[plane][H][W] = d(sum_b gout[b] * val[b]) / dy at this level's HxW planes,
 * x and y this level's (pooled) planes, dvdm this level's row of vam_msssim_combine's output, gout [B] floats, g_coarse
 * the gradient already computed at the next coarser level ([planes][Hc][Wc], NULL at the last level; gathered through
 * the pool as g += g_coarse((iy + H % 2) / 2, (ix + W % 2) / 2) / 4). */
int vam_msssim_bwd_level(const float* x, const float* y, int B, int C, int H, int W, const float* win11, float c1, float c2, int last,
                         const double* dvdm, const float* gout, const float* g_coarse, float* g, void* stream);

/* ------------------------------------------------------------------ REM fine-tune backward (configs[4]) */
/* Weight (and bias) gradient of a stride-1, pad k/2 convolution (autograd's conv backward-weight for
 * layers/rem.py:40-49):  dw[n][c_off + c][ty][tx] = sum_p dy[p][n] * x[pix(p)+(ty-k/2, tx-k/2)][c]  in OIHW with
 * `cin_total` input channels; x is a C-channel window (one segment of a concatenated input lands at c_off).
 * db (may be NULL; honoured by the problem with c_off == 0) = sum_p dy[p][n].  Fixed summation order.
 * Up to VAM_MAX_WGRAD_GROUP independent problems run in one launch (the ten slices' REM blocks in lockstep). */
#define VAM_MAX_WGRAD_GROUP 16
typedef struct vam_wgrad {
  const float* x;
  const float* dy;
  float* dw;
  float* db;
  int ld_x, ld_dy;
  int B, H, W;        /* extent of dy (the convolution's output grid)                                          */
  int kh, kw;
  int C, N;
  int cin_total, c_off;
  int stride;         /* 0 or 1: stride 1, pad k/2, x has the extent of dy.  2: a stride-2, pad k/2 convolution (k5: g_a,  */
  int Hx, Wx;         /* k3: h_a) — x is [B, Hx, Wx] (Hx = 2H, Wx = 2W): input pixel = 2*o - k/2 + tap.  Also the   */
                      /* transposed convolutions of g_s: their weight gradient is this with x and dy exchanged      */
  int splits;         /* 0 / 1: one block per weight tile walks all pixels.  > 1 (from vam_conv_wgrad_plan): the      */
  float* workspace;   /* pixels are cut into `splits` ranges whose partial tiles go to this caller-owned buffer and   */
                      /* are added in range order by a second launch (layers with few weight tiles and many pixels)  */
  float slot_share;   /* planning hint (vam_conv_wgrad_plan only): the fraction of the chip this problem can count on  */
                      /* when it shares a grouped launch with others (its share of the group's FLOPs); 0 = alone       */
  int32_t flags;      /* VAM_WGRAD_X_P3: x is a bf16x3 plane tensor (VAM_CONV_OUT_BF3 layout; ld_x counts 8-channel     */
                      /* groups per pixel) — k3 stride-1 problems on grids vam_conv_wgrad_lds_grid() accepts only      */
} vam_wgrad;
#define VAM_WGRAD_X_P3 1
/* 1 when weight gradients on an H x W output grid take the LDS-tiled kernel (which alone reads plane tensors). */
int vam_conv_wgrad_lds_grid(int H, int W);
/* Suggested number of pixel splits for a problem (>= 1) and the workspace it needs (0 bytes when 1). */
int vam_conv_wgrad_plan(const vam_wgrad* problem, size_t* workspace_bytes);
/* Which kernel instantiation a problem launched alone takes (host arithmetic, no GPU needed; returns 0, or 1 on bad
 * arguments): out = {kernel (0 register-gather, 1 LDS-tiled), pipe (0 fp32, 1 bf16x3), waves wn, wc (0, 0: gather kernel),
 * 32x32 blocks tn, tc, pixels per step kp, plane input}. */
int vam_conv_wgrad_route(const vam_wgrad* problem, int out[8]);
int vam_conv_wgrad_group(const vam_wgrad* problems, int n_problems, void* stream);
int vam_conv_wgrad(const float* x, int ld_x, const float* dy, int ld_dy, int B, int H, int W, int kh, int kw,
                   int C, int N, float* dw_oihw, float* db, int cin_total, int c_off, void* stream);
/* out[n] = sum_p dy[p][n]  (bias gradient): pixel ranges in parallel into `workspace` (vam_colsum_workspace bytes,
 * caller-owned), then added in range order — deterministic. */
size_t vam_colsum_workspace(long n_pix, int N);
int vam_colsum(const float* dy, int ld, long n_pix, int N, float* out, float* workspace, void* stream);
/* dx = dy * (act > 0 ? 1 : 0.01): LeakyReLU(0.01) backward from its OUTPUT (same sign as its input) */
int vam_leaky_bwd(const float* act, int ld_a, const float* dy, int ld_dy, float* dx, int ld_dx, long n_pix, int C, void* stream);
int vam_mul(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, long n_pix, int C, void* stream);
/* Training-mode Gaussian likelihood (entropy_models.py:132-138,620-652; pic.py:437-442): v = ((y-y2)-mu)*m + noise,
 * s = max(sigma*m, .11), lik = max(Phi((.5-|v|)/s) - Phi((-.5-|v|)/s), 1e-9).  grad_lik == NULL: forward (writes lik).
 * grad_lik != NULL: backward (writes dmu, dsigma = grad_lik * dlik/d{mu,sigma}, with compressai's LowerBound
 * gradient rule on both bounds).  y2 / mask may be NULL. */
int vam_gauss_train(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                    const float* sigma, int ld_sigma, const float* mask, int ld_mask, const float* noise, int ld_noise,
                    const float* grad_lik, int ld_glik, float* lik, int ld_lik, float* dmu, int ld_dmu,
                    float* dsigma, int ld_dsigma, long n_pix, int C, void* stream);
/* The progressive tail of n_levels quality levels over ONE (y, y2, mu, sigma) window (training forward with quality lists
 * [0, q1, ..., qL]: every level shares the progressive (mu, sigma) chain, pic.py:380-478).  Level l's mask, noise, lik and
 * rq live at their base pointer + l * <name>_ls floats, with their own pixel stride.
 *   forward:  rq_l = round(r - mu) * m_l + mu (r = y - y2) and lik_l = vam_gauss_train's forward with m_l, noise_l —
 *             bit-identical to vam_gauss_tail (yhat) + vam_gauss_train (lik) per level.
 *   backward: for l = 0 .. n_levels-1 in order, vam_gauss_train's backward (grad_lik_l) -> (dmu_l, dsg_l) and the
 *             straight-through rounding under m_l of d_rq_l: d_r = d_rq*m + (-1)*dmu_l, g = d_rq*(1-m) + dmu_l;
 *             gmu = (0 + g_0) + g_1 ..., dsigma = (0 + dsg_0) + dsg_1 ..., dy_top += d_r (in place) and, when dy_sub is
 *             not NULL, dy_sub += (-1)*d_r — bit-identical to that sequence of vam_gauss_train, VAM_EW_MASK_SPLIT and
 *             VAM_EW_AXPY launches. */
int vam_gauss_levels_fwd(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls,
                         const float* noise, int ld_noise, long noise_ls, float* rq, int ld_rq, long rq_ls,
                         float* lik, int ld_lik, long lik_ls, int n_levels, long n_pix, int C, void* stream);
int vam_gauss_levels_bwd(const float* y, int ld_y, const float* y2, int ld_y2, const float* mu, int ld_mu,
                         const float* sigma, int ld_sigma, const float* mask, int ld_mask, long mask_ls,
                         const float* noise, int ld_noise, long noise_ls, const float* grad_lik, int ld_glik, long glik_ls,
                         const float* d_rq, int ld_drq, long drq_ls, float* gmu, int ld_gmu, float* dsigma, int ld_dsigma,
                         float* dy_top, int ld_dyt, float* dy_sub, int ld_dys, int n_levels, long n_pix, int C, void* stream);

/* ------------------------------------------------------------------ transform backward (refine_gs) */
/* Element-wise derivatives of the synthesis / analysis transforms (csrc/train_gs.hip).  Every tensor is a channel
 * window [n_pix, C] with its own pixel stride. */
enum vam_ew_op {
  VAM_EW_GELU_FWD = 0,      /* out0 = gelu(in0)                                          (layers/layers.py:36-40) */
  VAM_EW_GELU_BWD = 1,      /* in0 = pre-activation, in1 = dy: out0 = dy * gelu'(in0)                                 */
  VAM_EW_GATE_BWD = 2,      /* a*sigmoid(b)+x (layers.py:72-74): in0 = a, in1 = b, in2 = dout: out0 = da, out1 = db    */
  VAM_EW_GDN_APPLY = 3,     /* in0 = x, in1 = norm: out0 = x*sqrt(norm) (flag 1, IGDN) or x*rsqrt(norm) (gdn.py:70-72) */
  VAM_EW_GDN_BWD_PREP = 4,  /* in0 = x, in1 = norm, in2 = dy: out0 = dL/dnorm, out1 = dy * dy/dx at fixed norm, out2 = x^2 */
  VAM_EW_GDN_BWD_FIN = 5,   /* in0 = out1 above, in1 = x, in2 = gamma^T dL/dnorm: out0 = in0 + 2 x in2                  */
  VAM_EW_CLAMP_BWD = 6,     /* in0 = clamp_(v,0,1), in1 = dL/dout: out0 = dL/dv                      (pic.py:558,651) */
  VAM_EW_AXPY = 7,          /* out0 = in0 + coef * in1                                                                 */
  VAM_EW_GATE_FWD = 8,      /* in0 = a, in1 = b, in2 = x: out0 = a*sigmoid(b) + x                                      */
  VAM_EW_REPARAM_BWD = 9,   /* NonNegativeParametrizer backward: in0 = stored parameter, in1 = dL/dvalue, coef = bound */
  VAM_EW_HTANH_FWD = 10,    /* LRP tail (pic.py:635-641): in0 = z, in1 = quantised residual, in2 = base: (0.5 tanh z + in1) + in2 */
  VAM_EW_HTANH_BWD = 11,    /* in0 = z, in1 = dy: out0 = dy * 0.5 (1 - tanh(z)^2)                                         */
  VAM_EW_MASK_SPLIT = 12    /* straight-through rounding under the variance mask (pic.py:443: ste_round(r - mu) * m + mu):
                               in0 = dL/d(result), in1 = m: out0 = in0 * m (to r), out1 = in0 * (1 - m) (to mu)           */
};
typedef struct vam_ew {
  vam_aux in[4];
  vam_aux out[3];
  long n_pix;
  int32_t C;
  int32_t flag;
  float coef;
  int32_t pad_;
} vam_ew;
/* The last two layers of a slice stack — conv3x3(128 -> 64) + GELU, conv3x3(64 -> 32) with the epilogue
 * out = post2 + post + act(conv + bias), act = VAM_ACT_NONE or VAM_ACT_HALF_TANH — as ONE launch per VAM_MAX_TAIL_GROUP stacks
 * (reference: the tails of the Sequentials cc_mean_transforms[_prog] / cc_scale_transforms[_prog] / lrp_transforms[_prog],
 * models/pic.py:86-121, 550, 635-641).  x = the 128-channel input as bf16x3 planes (what a conv launch with VAM_CONV_OUT_BF3
 * writes; x_groups = 8-channel groups per pixel of that buffer: 16, the tensor is not a window of a wider one), w4 / b4 / w5 / b5 = the packed weights and bias of the two layers
 * as vam_conv takes them; out fp32 NHWC with row pitch ld_out.  Same bits as the two vam_conv_group launches.  Built for latents
 * 16 columns wide (W == 16, H a multiple of 4): the caller falls back to vam_conv_group otherwise. */
#define VAM_MAX_TAIL_GROUP 8
typedef struct vam_stack_tail {
  const void* x;
  const void* w4;
  const float* b4;
  const void* w5;
  const float* b5;
  float* out;
  vam_aux post, post2;
  int32_t B, H, W;
  int32_t x_groups;
  int32_t ld_out;
  int32_t act;
} vam_stack_tail;
int vam_stack_tail_group(const vam_stack_tail* probs, int n, void* stream);
int vam_train_elementwise(int op, const vam_ew* e, void* stream);
/* n <= VAM_MAX_EW_GROUP independent VAM_EW_AXPY updates (out0 = in0 + coef * in1, each job with its own windows, extent and
 * coefficient) in ONE launch: the backward of `torch.cat` in front of a slice stack (pic.py:407-408, 452-453: the first layer's
 * input gradient is added, channel range by channel range, into the accumulators of the concatenated tensors).  Windows WRITTEN
 * by different jobs of one call must not overlap. */
#define VAM_MAX_EW_GROUP 8
int vam_train_axpy_group(const vam_ew* jobs, int n, void* stream);
/* Backward of vam_win_attention: dqkv [B,H,W,3C] (dq | dk | dv, same layout as qkv) from dout = dL/d(attention output),
 * and the relative-position-bias gradient WRITTEN to dtable [(2ws-1)^2][heads].  Deterministic: every (window, head group)
 * block writes its partial table into `workspace` (vam_win_attention_bwd_workspace bytes, caller-owned) and a second
 * launch adds the rows in a fixed order — no float atomics in global memory. */
size_t vam_win_attention_bwd_workspace(int B, int H, int W, int heads, int ws);
int vam_win_attention_bwd(const float* qkv, int ld_qkv, const float* dout, int ld_do, float* dqkv, int ld_dq,
                          const float* table, float* dtable, float* workspace, int B, int H, int W, int C, int heads, int ws,
                          int shift, void* stream);

/* ------------------------------------------------------------------ first-stage training (configs[3]) */
/* Backward of the training-mode entropy bottleneck (entropy_models.py:403-436,449-492 with quantize "noise"): for
 * lik = max(|sigmoid(s u) - sigmoid(s l)|, 1e-9), u / l = logits_cumulative(z + noise +/- 0.5), s = -sign(l + u) detached:
 * dz = grad_lik * dlik/dz (written, not accumulated) and dparams (layout of `params`, see vam_eb_forward; the quantiles'
 * entries are zero: the noise likelihood does not read them) = sum over pixels, fixed order.  LowerBound rule on 1e-9. */
int vam_eb_train_bwd(const float* z, int ld_z, const float* noise, int ld_noise, const float* params, int C,
                     const float* grad_lik, int ld_glik, float* dz, int ld_dz, float* dparams, long n_pix, void* stream);
/* Gradient of PixelShuffle(2) (layers/layers.py:82-86): dst[b,y,x,c*4+i*2+j] = src[b,2y+i,2x+j,c]; H, W = extent of dst. */
int vam_ps2_unshuffle(const float* src, int ld_src, float* dst, int ld_dst, int B, int H, int W, int Cq, void* stream);
/* dst[b,2y,2x,:] = src[b,y,x,:], zeros elsewhere (H, W = extent of src): with the VAM_PACK_CONV_DGRAD problem on dst this is
 * the data gradient of a k3 / stride-2 / pad-1 convolution (h_a, models/builder.py:72-82). */
int vam_upsample2_zero(const float* src, int ld_src, float* dst, int ld_dst, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------ bitstream (HOST pointers) */
/* compressai `_CXX.pmf_to_quantized_cdf` (reference entropy_models.py:61-64): n probabilities ->
 * n+1 cumulative counts at `precision` bits, every symbol given a non-zero frequency. */
int vam_pmf_to_quantized_cdf(const float* pmf_host, int n, int precision, int32_t* cdf_out_host);
/* compressai `ans.RansEncoder.encode_with_indexes` / `RansDecoder.decode_with_indexes`
 * (reference entropy_models.py:231-239,280-290): symbols[i] coded with table indexes[i];
 * cdfs is [n_cdfs][cdf_stride], cdf_sizes[k] = valid entries of table k (pmf length + 2), offsets[k]
 * = symbol value of entry 0; out-of-range symbols use 4-bit bypass chunks.  16-bit precision.
 * encode returns the stream length in bytes (<0 on error). */
long vam_rans_encode(const int32_t* symbols_host, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                     int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                     uint8_t* out_host, long out_capacity);
int vam_rans_decode(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n,
                    const int32_t* cdfs_host, int cdf_stride, const int32_t* cdf_sizes_host,
                    const int32_t* offsets_host, int n_cdfs, int32_t* symbols_out_host);
/* Many independent streams in one call (progressive containers: z, the base slices and every layer of a batch of
 * images), coded on min(n_threads, VAM_RANS_MAX_THREADS, n_streams) host threads.  Each stream's bytes equal
 * vam_rans_encode's on the same inputs, whatever the thread count.  layer != NULL selects one container layer: element i
 * is coded as symbol 0 with table 0 unless layer[i] == sel (the reference's r_sym * delta, idx * delta), and decoding
 * writes symbols_out[i] only where layer[i] == sel, so the layers of a container fill one symbol array.  On error the
 * first failing stream (lowest index) is reported. */
#define VAM_RANS_MAX_THREADS 16
typedef struct vam_rans_stream {
  const int32_t* symbols;     /* encode: n symbols */
  int32_t* symbols_out;       /* decode: n symbols */
  const int32_t* indexes;     /* n table indexes */
  const uint8_t* layer;       /* NULL, or n layer ids (0xFF = in no layer) */
  long n;
  int sel;                    /* the layer this stream carries */
  int pad_;
  uint8_t* bytes;             /* encode: output buffer of `capacity` bytes; decode: the stream */
  long capacity;
  long n_bytes;               /* encode: bytes written (set by the call); decode: stream length */
} vam_rans_stream;
int vam_rans_encode_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs_host, int cdf_stride,
                            const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int n_threads);
int vam_rans_decode_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs_host, int cdf_stride,
                            const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int n_threads);

/* Embedded streams (vampic.embedded): a stream is decodable from any byte prefix, because the decoder
 * reads its words front to back and symbol i depends only on the words consumed up to it.
 * vam_rans_decode_prefix_streams: per stream (bytes = the first n_bytes >= 0 bytes of a stream of n symbols, any length;
 * layer must be NULL) decode as many leading symbols as the floor(n_bytes / 4) whole words allow, write them to
 * symbols_out[0 .. count) (the rest is left untouched; symbols_out may be NULL) and the count to counts_out[i].  Fewer
 * than 8 bytes give 0; a symbol whose renormalisation word or bypass nibbles are incomplete is not counted.  Threaded as
 * vam_rans_decode_streams.
 * vam_rans_prefix_bytes: for n_counts sorted symbol counts, bytes_out[q] = the smallest byte length (a multiple of 4)
 * from which the tolerant decoder yields at least counts[q] symbols (0 for a count of 0): one decoding pass that notes
 * the read pointer.  A count the given bytes do not reach is VAM_EINVAL. */
int vam_rans_decode_prefix_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs_host, int cdf_stride,
                                   const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int n_threads,
                                   long* counts_out);
int vam_rans_prefix_bytes(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                          int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                          const long* counts, int n_counts, long* bytes_out);

/* ------------------------------------------------------------------ device rANS coder */
/* The coder above restated as one core for host and device (csrc/rans_core.h): the same wire format, so host-coded and
 * device-coded streams are interchangeable byte for byte.
 * vam_rans_core_encode / _decode (HOST pointers): vam_rans_encode / vam_rans_decode through the core, plus the layer
 * selection of vam_rans_stream.  encode returns the length in bytes (< 0 on error); decode returns 0, a positive
 * per-stream status (1 bitstream truncated, 2 index out of range, 3 cdf size invalid, 6 stream shorter than 8 bytes or
 * not in whole words) or VAM_EINVAL for bad arguments.  It never reads outside the stream; after a failure every
 * remaining selected symbol is written as 0.
 * The _nhwc variants code one image's channel window of an int32 buffer [.., h, w, ld] in place: stream element
 * (c * h + y) * w + x reads buf[((image * h + y) * w + x) * ld + c0 + c], the [C, h, w] order the flat calls get after a
 * transpose.  idx == NULL means "table index = channel c" (the z streams).  layer, when given, has the geometry of sym. */
long vam_rans_core_encode(const int32_t* symbols_host, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                          int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                          uint8_t* out_host, long out_capacity, const uint8_t* layer_host, int sel);
int vam_rans_core_decode(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                         int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                         int32_t* symbols_out_host, const uint8_t* layer_host, int sel);
long vam_rans_core_encode_nhwc(const int32_t* sym_host, const int32_t* idx_host, const uint8_t* layer_host, int sel, int image,
                               int h, int w, int ld, int c0, int C, const int32_t* cdfs_host, int cdf_stride,
                               const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, uint8_t* out_host,
                               long out_capacity);
int vam_rans_core_decode_nhwc(const uint8_t* in_host, long n_bytes, const int32_t* idx_host, const uint8_t* layer_host, int sel,
                              int image, int h, int w, int ld, int c0, int C, const int32_t* cdfs_host, int cdf_stride,
                              const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int32_t* sym_out_host);

/* The coder's tables on the device (bitstream.DeviceCoderTables).  packed (may be NULL): the tables ragged as 16-bit
 * values for the decoder's LDS copy — table k is its entries 0 .. sizes[k]-2 at packed_start[k], the terminal 65536
 * implied; packed_entries is the total, padded to a multiple of 8.  Only tables that start at 0, increase strictly and
 * end at 65536 may be packed.  Without it the decoder reads the int32 tables from global memory. */
typedef struct vam_rans_tables {
  const int32_t* cdf;          /* [n_cdfs][stride] */
  const int32_t* sizes;        /* [n_cdfs] */
  const int32_t* offsets;      /* [n_cdfs] */
  int32_t n_cdfs, stride;
  const uint16_t* packed;
  const int32_t* packed_start; /* [n_cdfs] */
  int32_t packed_entries, pad_;
} vam_rans_tables;
/* The LDS bytes a workgroup may use on the current device: packed tables above it do not fit. */
int vam_rans_lds_table_bytes(void);

/* DEVICE pointers from here.  A stream is an (image, slice) pair: slice s covers the channels [c0 + s*C, c0 + (s+1)*C)
 * of the int32 NHWC buffers [B, h, w, ld], element order as in the _nhwc calls above; stream id = s * B + image.
 * vam_rans_encode_device: one launch codes all B * n_slices streams.  Stream id's words are written backwards from the
 * end of its region out_words + id * out_cap_words (2 * C*h*w + 16 words is the host coder's budget); lengths[id] = its
 * length in words, the stream being the region's tail, and status[id] = 0 or a status as above (4 output region too
 * small, 5 zero-frequency symbol; the length is then 0).
 * vam_rans_pack_device: offsets[id] = lengths[0] + .. + lengths[id-1] (offsets[n_streams] = the total) and every stream's
 * words copied to packed + offsets[id], so the host fetches the lengths and the coded bytes only.
 * vam_rans_decode_device: stream id is the byte_lengths[id] bytes at bytes + byte_offsets[id] (offsets are multiples of
 * 4); its symbols go straight into the window of sym_out, status[id] as above.  No read leaves a stream's bytes. */
int vam_rans_encode_device(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int B, int h, int w, int ld,
                           int c0, int C, int n_slices, const vam_rans_tables* tables, uint32_t* out_words, long out_cap_words,
                           int32_t* lengths, int32_t* status, void* stream);
int vam_rans_pack_device(const uint32_t* regions, long cap_words, const int32_t* lengths, int n_streams, uint32_t* packed,
                         long packed_cap_words, int64_t* offsets, void* stream);
int vam_rans_decode_device(const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                           const uint8_t* layer, int sel, int B, int h, int w, int ld, int c0, int C, int n_slices,
                           const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream);

/* ------------------------------------------------------------------ lane-split streams */
/* A stream of n elements as `lanes` = K independent lanes, K a power of two in 1 .. VAM_RANS_MAX_LANES: lane j is the
 * stream above of the elements j, j + K, j + 2K, ... (an empty lane is the 8 bytes of the initial state).  K = 1 is the
 * existing wire format byte for byte, with no header.  For K > 1 the string is K little-endian uint32 lane lengths in
 * 32-bit words (each >= 2), then the lanes' words back to back: 4 K + 4 sum(L_j) bytes exactly.  K is not stored in the
 * string: both sides share it, like the quality and the shape.
 * vam_rans_lanes_encode / _decode[_nhwc] (HOST pointers) mirror vam_rans_core_encode / _decode[_nhwc] with `lanes` and
 * lane_status (NULL or K int32: the status of every lane).  A buffer of 4 K + K * (8 * ceil(n / K) + 64) bytes holds any
 * string.  decode returns the status of the lowest-numbered failing lane: a string shorter than 4 K bytes, an L_j < 2 or
 * lengths that do not add up to the string's length (64-bit sums) are status 6 for every lane, and every selected symbol
 * is written as 0; a lane that fails on its own zeroes its symbols from the failure on, the other lanes are decoded. */
#define VAM_RANS_MAX_LANES 64
long vam_rans_lanes_encode(const int32_t* symbols_host, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                           int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                           uint8_t* out_host, long out_capacity, const uint8_t* layer_host, int sel, int lanes,
                           int32_t* lane_status_host);
int vam_rans_lanes_decode(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                          int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                          int32_t* symbols_out_host, const uint8_t* layer_host, int sel, int lanes, int32_t* lane_status_host);
long vam_rans_lanes_encode_nhwc(const int32_t* sym_host, const int32_t* idx_host, const uint8_t* layer_host, int sel, int image,
                                int h, int w, int ld, int c0, int C, const int32_t* cdfs_host, int cdf_stride,
                                const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, uint8_t* out_host,
                                long out_capacity, int lanes, int32_t* lane_status_host);
int vam_rans_lanes_decode_nhwc(const uint8_t* in_host, long n_bytes, const int32_t* idx_host, const uint8_t* layer_host, int sel,
                               int image, int h, int w, int ld, int c0, int C, const int32_t* cdfs_host, int cdf_stride,
                               const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int32_t* sym_out_host,
                               int lanes, int32_t* lane_status_host);
/* DEVICE pointers.  One thread per (stream, lane); lane id = stream id * lanes + lane.
 * vam_rans_lanes_encode_device: lane id's words are written backwards from the end of its region out_words + id *
 * out_cap_words (2 * ceil(C*h*w / lanes) + 16 words is the budget); lengths[id] and status[id] are per lane, so
 * vam_rans_pack_device over the B * n_slices * lanes regions gives the streams' bodies back to back and lengths is the
 * headers.  vam_rans_lanes_decode_device: stream id is byte_lengths[id] bytes at bytes + byte_offsets[id] as above;
 * status has B * n_slices * lanes entries.  No read leaves a stream's bytes, no write the window. */
int vam_rans_lanes_encode_device(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int B, int h, int w, int ld,
                                 int c0, int C, int n_slices, int lanes, const vam_rans_tables* tables, uint32_t* out_words,
                                 long out_cap_words, int32_t* lengths, int32_t* status, void* stream);
int vam_rans_lanes_decode_device(const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                                 const uint8_t* layer, int sel, int B, int h, int w, int ld, int c0, int C, int n_slices, int lanes,
                                 const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream);

/* ------------------------------------------------------------------ layered launches */
/* DEVICE pointers.  The device pairs above with a level dimension: one launch covers the n_sel consecutive layer selectors
 * sel0 .. sel0 + n_sel - 1 (layer ids are uint8: sel0 + n_sel <= 256; layer must not be NULL) over one window.  Stream id =
 * (k * n_slices + slice) * B + image, and stream (k, slice, image) is exactly what the single-selector call gives for
 * sel = sel0 + k: the elements with layer == sel0 + k, every other element as symbol 0 in table 0.  lanes = 1: one wave per
 * stream (vam_rans_encode_device / _decode_device's form); lanes = K > 1: one thread per (stream, lane), regions, lengths
 * and status per (stream, lane) as in the lanes calls.  n_sel * B * n_slices is at most 2^20.
 * vam_rans_layers_decode_device: all levels write into the same window, each only the elements of its own layer, so the
 * writes are disjoint; elements whose layer id is outside [sel0, sel0 + n_sel) are not touched.  With lanes = 1 eight
 * streams, one wave each, share a workgroup and its LDS copy of the packed tables. */
int vam_rans_layers_encode_device(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel0, int n_sel, int B, int h,
                                  int w, int ld, int c0, int C, int n_slices, int lanes, const vam_rans_tables* tables,
                                  uint32_t* out_words, long out_cap_words, int32_t* lengths, int32_t* status, void* stream);
int vam_rans_layers_decode_device(const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                                  const uint8_t* layer, int sel0, int n_sel, int B, int h, int w, int ld, int c0, int C,
                                  int n_slices, int lanes, const vam_rans_tables* tables, int32_t* sym_out, int32_t* status,
                                  void* stream);

/* ------------------------------------------------------------------ interleaved lanes */
/* A stream of n elements on `lanes` = K interleaved lanes, K as above: element i belongs to lane i % K and group i / K, and
 * the K coder states share ONE word stream.  The string is the K final states in lane order (two little-endian words each,
 * low then high; a lane without elements holds 2^31), then the renormalisation words in the order the decoder reads them:
 * groups ascending, inside a group rounds t = 0, 1, ..: every lane that still has a get t (0 the table symbol, then the
 * count and raw nibbles of an escape) updates its state, then the lanes whose state fell below 2^31 take one word each in
 * ascending lane order.  A byte prefix therefore decodes a rank prefix, and K = 1 is the existing wire format byte for
 * byte.  A buffer of 8 n + 8 K + 64 bytes holds any string.  K is not stored in the string.
 * HOST pointers.  vam_rans_interleaved_encode[_streams]: vam_rans_encode[_streams] for this format (layer must be NULL).
 * vam_rans_interleaved_decode_prefix[_streams]: the tolerant decode of the first n_bytes >= 0 bytes (floor(n_bytes / 4)
 * words; fewer than 2 K decode nothing).  A lane that needs a word the prefix does not hold fails, as does every later
 * request; the other lanes of that group finish the gets that need no word and decoding ends with that group: the count
 * is g K + the lowest failed lane.  symbols_out[0 .. count) is written, the rest left untouched.  The single-stream call
 * returns the count and, in status_out, 0 or the status (2 index out of range, 3 cdf size invalid) that ended the stream;
 * with status_out NULL, and in the _streams call, such a status is VAM_EINVAL.
 * vam_rans_interleaved_prefix_bytes: bytes_out[q] = 4 * the read position after the last word that any of the elements
 * 0 .. counts[q] - 1 reads (8 K when they read none, 0 for a count of 0): the smallest prefix that decodes counts[q]. */
long vam_rans_interleaved_encode(const int32_t* symbols_host, const int32_t* indexes_host, long n, const int32_t* cdfs_host,
                                 int cdf_stride, const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs,
                                 uint8_t* out_host, long out_capacity, int lanes);
int vam_rans_interleaved_encode_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs_host, int cdf_stride,
                                        const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int lanes,
                                        int n_threads);
long vam_rans_interleaved_decode_prefix(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n,
                                        const int32_t* cdfs_host, int cdf_stride, const int32_t* cdf_sizes_host,
                                        const int32_t* offsets_host, int n_cdfs, int lanes, int32_t* symbols_out_host,
                                        int32_t* status_out);
int vam_rans_interleaved_decode_prefix_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs_host, int cdf_stride,
                                               const int32_t* cdf_sizes_host, const int32_t* offsets_host, int n_cdfs, int lanes,
                                               int n_threads, long* counts_out);
int vam_rans_interleaved_prefix_bytes(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n,
                                      const int32_t* cdfs_host, int cdf_stride, const int32_t* cdf_sizes_host,
                                      const int32_t* offsets_host, int n_cdfs, int lanes, const long* counts, int n_counts,
                                      long* bytes_out);
/* DEVICE pointers.  n_streams streams of n elements each, flat: stream s reads sym / idx [s * n, (s + 1) * n) (the ranked
 * buffers of vam_rank_gather).  One thread per (stream, lane); 64 / K streams share a wave, a lane finds its word by a
 * prefix popcount of the wave's ballot.
 * vam_rans_interleaved_encode_device: regions, lengths and status as in vam_rans_encode_device (2 n + 2 K + 16 words hold
 * any string); vam_rans_pack_device packs them.  counts (may be NULL with n_marks = 0): int32 [n_marks][n_streams], for
 * every stream non-decreasing in the mark; mark_bytes [n_marks][n_streams] receives vam_rans_interleaved_prefix_bytes of
 * each count, taken from the encoder's own word positions (0 for a stream that failed).
 * vam_rans_interleaved_decode_device: stream s is the first byte_lengths[s] >= 0 bytes of a string at bytes +
 * byte_offsets[s] (a multiple of 4, inside [0, bytes_total)), decoded tolerantly: sym_out[s * n + i] for i < available[s],
 * 0 for every other element; status[s] = 0, 2, 3 or 6 (a refused offset or length: nothing is read).  No read leaves a
 * stream's bytes, no write the n_streams * n elements. */
int vam_rans_interleaved_encode_device(const int32_t* sym, const int32_t* idx, int n_streams, long n, int lanes,
                                       const vam_rans_tables* tables, uint32_t* out_words, long out_cap_words, int32_t* lengths,
                                       int32_t* status, const int32_t* counts, int n_marks, int32_t* mark_bytes, void* stream);
int vam_rans_interleaved_decode_device(const uint8_t* bytes, long bytes_total, const int64_t* byte_offsets,
                                       const int32_t* byte_lengths, const int32_t* idx, int n_streams, long n, int lanes,
                                       const vam_rans_tables* tables, int32_t* sym_out, int32_t* available, int32_t* status,
                                       void* stream);
/* The cut table.  vam_rans_interleaved_cut_table_device: for the streams vam_rans_interleaved_encode_device
 * reads (same sym / idx, n_streams, n >= 1, lanes, tables), cut [n_streams][n + 1] receives, for EVERY count 0 <= c <= n,
 * cut[s][c] = vam_rans_interleaved_prefix_bytes of count c on the string that launch writes for stream s (K = 1:
 * vam_rans_prefix_bytes): 0 for c = 0, 8 K while none of the elements 0 .. c - 1 reads a word, else 4 * the read position
 * after the last word any of them reads.  A row never decreases and cut[s][n] is at most the string's length.  It is a dry
 * walk of the encoder in the encode launch's thread geometry: no word is written, so there is no region, no lengths and no
 * status 4.  status[s] = 0, or 2 / 3 / 5 as the encode launch gives them, and then row s is all zeros.  No atomics, no
 * allocation; capturable.  Null pointers, n < 1, n > 2^28 (so that n + 1 and every entry fit an int32) and an invalid
 * lanes are VAM_EINVAL with a message, and nothing is launched or written. */
int vam_rans_interleaved_cut_table_device(const int32_t* sym, const int32_t* idx, int n_streams, long n, int lanes,
                                          const vam_rans_tables* tables, int32_t* cut, int32_t* status, void* stream);
/* The same strings over the stream geometry of vam_rans_encode_device / vam_rans_decode_device: a stream
 * is an (image, slice) pair over the channels [c0 + s C, c0 + (s + 1) C) of int32 NHWC buffers [B, h, w, ld], stream id =
 * s * B + image, n = C h w, element i = channel i / (h w) at pixel i % (h w); idx NULL: the table index is the channel.
 * Thread geometry as above: one thread per (stream, lane).  These code z and the base slices of an "embedded-4" container.
 * vam_rans_interleaved_encode_nhwc_device: regions (2 n + 2 K + 16 words hold any string), lengths and status as in
 * vam_rans_interleaved_encode_device, no marks; the strings equal vam_rans_interleaved_encode of the same elements, and at
 * K = 1 vam_rans_encode_device's.
 * vam_rans_interleaved_decode_nhwc_device: STRICT, the whole stream is needed.  status[s] = 0 and every element written;
 * 1 the words end early, 2 / 3 a bad index / table: the elements from the failing group on are written as 0; 6 a refused
 * offset or length: nothing is read or written.  No read leaves a stream's bytes, no write its own channel window. */
int vam_rans_interleaved_encode_nhwc_device(const int32_t* sym, const int32_t* idx, int B, int h, int w, int ld, int c0, int C,
                                            int n_slices, int lanes, const vam_rans_tables* tables, uint32_t* out_words,
                                            long out_cap_words, int32_t* lengths, int32_t* status, void* stream);
int vam_rans_interleaved_decode_nhwc_device(const uint8_t* bytes, long bytes_total, const int64_t* byte_offsets,
                                            const int32_t* byte_lengths, const int32_t* idx, int B, int h, int w, int ld, int c0,
                                            int C, int n_slices, int lanes, const vam_rans_tables* tables, int32_t* sym_out,
                                            int32_t* status, void* stream);

/* ------------------------------------------------------------------ resumable embedded decode */
/* The format above, unchanged, decoded in steps as the bytes arrive.  The CHECKPOINT of a stream is the decoder at the
 * start of a group: `done` elements lie before that group (a multiple of K, or n once the stream is finished), `pos` is the
 * index, in the whole string, of the next word to read, and states holds the K lane states (uint64) there.  The fresh
 * checkpoint is done = 0, pos = 0: its states are read from the string's first 2 K words (with fewer nothing decodes and it
 * stays fresh).
 * A resume call is handed the bytes of the string FROM BYTE 4 * pos ON and nothing before; the whole words among them extend
 * to an absolute word count W.  It decodes exactly as the tolerant decode does from group done / K, writes
 * symbols_out[i] for done_in <= i < count and no other element, and returns the count and the status.  If a lane of group g
 * failed, for want of a word or with a status, the checkpoint becomes the start of that group (done = g K, pos and states as
 * they were when it began); a complete stream gets done = n and later calls read and write nothing.  For successive
 * prefixes L1 <= L2 <= .. of one string, count, symbols and status after the call for Lk equal
 * vam_rans_interleaved_decode_prefix on the first Lk bytes; the status is recomputed on every call.  The Lk mod 4 trailing
 * bytes belong to no word yet: the caller keeps them and sends them again.
 * HOST pointers.  vam_rans_interleaved_resume: one stream; status_out as in vam_rans_interleaved_decode_prefix.
 * vam_rans_interleaved_resume_streams: streams[i] as vam_rans_interleaved_decode_prefix_streams reads it, bytes / n_bytes
 * being the string from byte 4 * checkpoints[i].pos on; counts_out and status_out receive one entry per stream, and a
 * status of 2 or 3 is VAM_EINVAL.  Refused by message, with nothing written: invalid lanes, n < 0, a negative length,
 * misaligned states, or an impossible checkpoint (done neither a multiple of K nor n, done > n, pos < 2 K while done > 0). */
typedef struct vam_rans_checkpoint {
  long done;                  /* elements before the checkpointed group */
  long pos;                   /* next word of the whole string */
  uint64_t* states;           /* K lane states */
} vam_rans_checkpoint;
long vam_rans_interleaved_resume(const uint8_t* in_host, long n_bytes, const int32_t* indexes_host, long n,
                                 const int32_t* cdfs_host, int cdf_stride, const int32_t* cdf_sizes_host,
                                 const int32_t* offsets_host, int n_cdfs, int lanes, int32_t* symbols_out_host,
                                 vam_rans_checkpoint* checkpoint, int32_t* status_out);
int vam_rans_interleaved_resume_streams(vam_rans_stream* streams, vam_rans_checkpoint* checkpoints, int n_streams,
                                        const int32_t* cdfs_host, int cdf_stride, const int32_t* cdf_sizes_host,
                                        const int32_t* offsets_host, int n_cdfs, int lanes, int n_threads, long* counts_out,
                                        int32_t* status_out);
/* DEVICE pointers.  vam_rans_interleaved_resume_device: the geometry of vam_rans_interleaved_decode_device, one thread per
 * (stream, lane).  The checkpoints are states [n_streams][lanes] (uint64), done [n_streams] and pos [n_streams] (int32), all
 * in and out; the uploaded bytes of stream s (byte_lengths[s] at bytes + byte_offsets[s]) begin at the string's word pos[s].
 * sym_out[s * n + i] is written for done_in <= i < available[s] only; status[s] = 0, 2, 3, or 6 for a refused offset, length
 * or checkpoint, and a refused stream is neither read nor written.  A wave leaves as soon as none of its streams is still
 * decoding.  No read leaves a stream's uploaded bytes, no write its n elements or its K states. */
int vam_rans_interleaved_resume_device(const uint8_t* bytes, long bytes_total, const int64_t* byte_offsets,
                                       const int32_t* byte_lengths, const int32_t* idx, int n_streams, long n, int lanes,
                                       const vam_rans_tables* tables, int32_t* sym_out, uint64_t* states, int32_t* done,
                                       int32_t* pos, int32_t* available, int32_t* status, void* stream);

/* ------------------------------------------------------------------ graphs / timing */
int vam_graph_begin(void* stream);
int vam_graph_end(void* stream, void** graph_exec_out);
int vam_graph_launch(void* graph_exec, void* stream);
/* The caller guarantees that no launch of graph_exec is in flight and that the calling thread is not capturing. */
int vam_graph_destroy(void* graph_exec);

/* Per-kernel-family timing with HIP events on the launch stream (bench.py roofline leg).
 * While enabled every launch is bracketed by an event pair; vam_prof_read synchronises the
 * events and returns accumulated milliseconds / launch count / algorithmic flops & bytes. */
enum vam_family { VAM_FAM_CONV = 0, VAM_FAM_ATTN = 1, VAM_FAM_MASK = 2, VAM_FAM_TAIL = 3,
                  VAM_FAM_MISC = 4, VAM_FAM_COUNT = 5 };
int vam_prof_enable(int on);
int vam_prof_reset(void);
int vam_prof_read(int family, double* ms, long* launches, double* flops, double* bytes);
/* Convolution launches are also summed per caller-defined class (which part of the model the launch belongs to:
 * g_a, g_s, hyperprior, stack heads, slice chain ... — the host plan sets the class before each launch while the
 * profiler is on), so that bench.py can report the roofline of the g_a/g_s conv stack on its own. */
#define VAM_PROF_CLASSES 16
int vam_prof_set_class(int cls);
int vam_prof_read_class(int cls, double* ms, long* launches, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* VAMPIC_H */
