"""ctypes binding of libvampic.so (C ABI declared in ``include/vampic.h``).

There is no CPU fallback: if the shared library is missing, or an op is called
without a usable gfx950 device, this module raises — loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VAMPIC_LIB", os.path.join(_HERE, "libvampic.so"))      # override: A/B kernel experiments

VAM_MAX_SEG = 4
VAM_MAX_GROUP = 8

# enum vam_act
ACT_NONE, ACT_GELU, ACT_LEAKY, ACT_HALF_TANH, ACT_SIGMOID, ACT_CLAMP01, ACT_RSQRT, ACT_SQRT, ACT_DOUBLE = range(9)
# enum vam_conv_flags
CONV_SQUARE_IN, CONV_PS2, CONV_OUT_NCHW, CONV_IN_BF3, CONV_OUT_BF3 = 1, 2, 4, 8, 16
CONV_W_BF16, CONV_IN_BF16, CONV_OUT_BF16, CONV_AUX_BF16 = 32, 64, 128, 256      # bf16-storage mode (BASELINE configs[2])
CONV_MUL_GELU_GRAD = 512         # training: the mul operand is a GELU's pre-activation z, the result is multiplied by gelu'(z)
# enum vam_pack_mode
PACK_CONV, PACK_DECONV5S2, PACK_PS2, PACK_GDN, PACK_CONV_DGRAD, PACK_GDN_T = range(6)
# enum vam_ew_op
(EW_GELU_FWD, EW_GELU_BWD, EW_GATE_BWD, EW_GDN_APPLY, EW_GDN_BWD_PREP, EW_GDN_BWD_FIN, EW_CLAMP_BWD, EW_AXPY, EW_GATE_FWD,
 EW_REPARAM_BWD, EW_HTANH_FWD, EW_HTANH_BWD, EW_MASK_SPLIT) = range(13)
# enum vam_family
FAM_CONV, FAM_ATTN, FAM_MASK, FAM_TAIL, FAM_MISC = range(5)
FAMILY_NAMES = ("conv_igemm", "win_attn", "variance_mask", "gauss_tail", "misc")
# launch classes of the event profiler (vam_prof_set_class): which part of the path a conv launch belongs to
PROF_CLASSES = ("other", "g_a", "g_s", "hyperprior", "stack_heads", "slice_chain", "lrp_prog", "rem")


class VamSeg(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int32), ("ld", C.c_int32)]


VAM_MAX_WGRAD_GROUP = 16
VAM_MAX_EW_GROUP = 8
VAM_MAX_MASK_LEVELS = 8         # include/vampic.h: levels of one vam_variance_mask_levels launch
VAM_MAX_TAIL_GROUP = 8
VAM_MAX_LAYER_LEVELS = 32       # include/vampic.h: qualities of one vam_variance_layers launch
VAM_RANS_MAX_THREADS = 16       # include/vampic.h: host threads of one vam_rans_*_streams call
VAM_RANS_MAX_LANES = 64         # include/vampic.h: lanes of a lane-split stream (a power of two in 1 .. 64)
LAYER_NONE = 0xFF               # vam_variance_layers: the element is in no layer
VAM_MAX_RANK_ELEMENTS = 1 << 18  # include/vampic.h: the largest segment vam_variance_rank sorts


class VamRansStream(C.Structure):
    _fields_ = [("symbols", C.c_void_p), ("symbols_out", C.c_void_p), ("indexes", C.c_void_p), ("layer", C.c_void_p),
                ("n", C.c_long), ("sel", C.c_int), ("pad_", C.c_int), ("bytes", C.c_void_p), ("capacity", C.c_long),
                ("n_bytes", C.c_long)]


class VamRansCheckpoint(C.Structure):
    """vam_rans_checkpoint: a resumable stream's decoder at the start of a group."""
    _fields_ = [("done", C.c_long), ("pos", C.c_long), ("states", C.c_void_p)]


class VamLayerParams(C.Structure):
    """vam_layer_params: one image's record of the device table of vam_variance_layers_per_image."""
    _fields_ = [("n_levels", C.c_int32), ("any_select", C.c_int32), ("k_lo", C.c_int32 * VAM_MAX_LAYER_LEVELS),
                ("k_hi", C.c_int32 * VAM_MAX_LAYER_LEVELS), ("w", C.c_float * VAM_MAX_LAYER_LEVELS),
                ("mode", C.c_int32 * VAM_MAX_LAYER_LEVELS)]


class VamCoderTables(C.Structure):
    """vam_coder_tables: the coder's tables on the device (bitstream.DeviceTables)."""
    _fields_ = [("cost", C.c_void_p), ("sizes", C.c_void_p), ("offsets", C.c_void_p), ("n_cdfs", C.c_int32), ("stride", C.c_int32)]


class VamRansTables(C.Structure):
    """vam_rans_tables: the coder's tables on the device for the device coder (bitstream.DeviceCoderTables)."""
    _fields_ = [("cdf", C.c_void_p), ("sizes", C.c_void_p), ("offsets", C.c_void_p), ("n_cdfs", C.c_int32), ("stride", C.c_int32),
                ("packed", C.c_void_p), ("packed_start", C.c_void_p), ("packed_entries", C.c_int32), ("pad_", C.c_int32)]


class VamWgrad(C.Structure):
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p),
                ("ld_x", C.c_int), ("ld_dy", C.c_int), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("kh", C.c_int), ("kw", C.c_int), ("C", C.c_int), ("N", C.c_int),
                ("cin_total", C.c_int), ("c_off", C.c_int), ("stride", C.c_int), ("Hx", C.c_int), ("Wx", C.c_int),
                ("splits", C.c_int), ("workspace", C.c_void_p), ("slot_share", C.c_float), ("flags", C.c_int32)]


WGRAD_X_P3 = 1


class VamAux(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("ld", C.c_int32), ("pad_", C.c_int32)]


class VamEw(C.Structure):
    _fields_ = [("inp", VamAux * 4), ("out", VamAux * 3), ("n_pix", C.c_long), ("C", C.c_int32), ("flag", C.c_int32),
                ("coef", C.c_float), ("pad_", C.c_int32)]


class VamStackTail(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w4", C.c_void_p), ("b4", C.c_void_p), ("w5", C.c_void_p), ("b5", C.c_void_p), ("out", C.c_void_p),
                ("post", VamAux), ("post2", VamAux), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("x_groups", C.c_int32),
                ("ld_out", C.c_int32), ("act", C.c_int32)]


class VamConv(C.Structure):
    _fields_ = [
        ("seg", VamSeg * VAM_MAX_SEG),
        ("n_seg", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32),
        ("stride", C.c_int32),
        ("pad_y", C.c_int32), ("pad_x", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("N", C.c_int32),
        ("wpack", C.c_void_p),
        ("bias", C.c_void_p),
        ("out", C.c_void_p),
        ("ldo", C.c_int32),
        ("Hf", C.c_int32), ("Wf", C.c_int32),
        ("osy", C.c_int32), ("osx", C.c_int32), ("ooy", C.c_int32), ("oox", C.c_int32),
        ("Cq", C.c_int32),
        ("act", C.c_int32),
        ("flags", C.c_int32),
        ("pre", VamAux), ("mul", VamAux), ("post", VamAux), ("post2", VamAux),
        ("in_amax", C.c_void_p * VAM_MAX_SEG), ("out_amax", C.c_void_p),
        ("preact", VamAux),
    ]


class VamConvChoice(C.Structure):
    """vam_conv_choice: what vam_conv_plan says vam_conv_group would launch a group of problems with."""
    _fields_ = [("bm", C.c_int32), ("bn", C.c_int32), ("bk", C.c_int32), ("spec", C.c_int32), ("blocks", C.c_int32),
                ("dual", C.c_int32 * VAM_MAX_GROUP), ("staged", C.c_int32 * VAM_MAX_GROUP)]


class VamPackJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("bias", C.c_int32), ("mode", C.c_int32), ("phase", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("cin", C.c_int32), ("n", C.c_int32), ("pad_", C.c_int32)]


class VamResunit(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("ldx", C.c_int32), ("ldo", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p), ("flags", C.c_int32), ("pad_", C.c_int32)]


RESUNIT_BF16 = 1


_SIGNATURES = {
    # name: (restype, argtypes)
    "vam_last_error": (C.c_char_p, []),
    "vam_version": (C.c_int, []),
    "vam_device_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "vam_conv_struct_size": (C.c_size_t, []),
    "vam_conv_wpack_floats": (C.c_size_t, [C.c_int] * 4),
    "vam_pack_conv_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_conv_wpack_bf16_bytes": (C.c_size_t, [C.c_int] * 4),
    "vam_pack_conv_weights_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_pack_bias": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vam_conv_force_tile": (C.c_int, [C.c_int] * 3),
    "vam_conv_force_epilogue": (C.c_int, [C.c_int]),
    "vam_conv_last_tile": (C.c_int, [C.c_void_p] * 3),
    "vam_conv_set_mode": (C.c_int, [C.c_int]),
    "vam_conv_get_mode": (C.c_int, []),
    "vam_conv_group": (C.c_int, [C.POINTER(VamConv), C.c_int, C.c_void_p]),
    "vam_conv_plan": (C.c_int, [C.POINTER(VamConv), C.c_int, C.POINTER(VamConvChoice)]),
    "vam_resunit_struct_size": (C.c_size_t, []),
    "vam_resunit_supported": (C.c_int, [C.c_int] * 3),
    "vam_resunit_group": (C.c_int, [C.POINTER(VamResunit), C.c_int, C.c_void_p]),
    "vam_resunit_set_dma": (C.c_int, [C.c_int]),
    "vam_resunit_set_debug": (C.c_int, [C.c_void_p]),
    "vam_s2d_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_nchw_to_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_nhwc_to_nchw": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_win_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]),
    "vam_attn_set_mfma": (C.c_int, [C.c_int]),
    "vam_attn_mfma": (C.c_int, []),
    "vam_variance_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                    C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_variance_mask_levels": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_variance_layers": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_layer_params_size": (C.c_size_t, []),
    "vam_variance_layer_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_variance_layers_per_image": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_variance_mask_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_variance_masks_per_image": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_variance_mask_map": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_coded_layer_bits": (C.c_int, [C.c_void_p, C.c_int] * 5 + [C.c_int, C.c_void_p, C.c_int, C.POINTER(VamCoderTables), C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_coded_symbol_bits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.POINTER(VamCoderTables), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int,
                                        C.c_void_p]),
    "vam_gauss_levels_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_void_p]),
    "vam_gauss_tail": (C.c_int, [C.c_void_p, C.c_int] * 5 + [C.c_void_p, C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_gauss_levels_eval": (C.c_int, [C.c_void_p, C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_long] * 4
                              + [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_gauss_layer_bits": (C.c_int, [C.c_void_p, C.c_int] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_build_indexes": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_eb_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_void_p]),
    "vam_eb_aux_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_dequantize": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_add": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_memset_zero": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "vam_pack_group": (C.c_int, [C.POINTER(VamPackJob), C.c_int, C.c_void_p]),
    "vam_absmax": (C.c_int, [C.POINTER(VamSeg), C.c_int, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_sqdiff_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_sqdiff_sum_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_eb_forward_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_ssim_level": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_avgpool2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_msssim_partial_doubles": (C.c_long, [C.c_int] * 3),
    "vam_msssim_partial_offset": (C.c_long, [C.c_int] * 4),
    "vam_msssim_fwd_level": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "vam_msssim_pool2": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]),
    "vam_msssim_combine": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 5),
    "vam_msssim_bwd_level": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_float, C.c_float, C.c_int]
                             + [C.c_void_p] * 5),
    "vam_conv_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vam_conv_wgrad_group": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vam_conv_wgrad_plan": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vam_conv_wgrad_route": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vam_conv_wgrad_lds_grid": (C.c_int, [C.c_int, C.c_int]),
    "vam_colsum_workspace": (C.c_size_t, [C.c_long, C.c_int]),
    "vam_colsum": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_leaky_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_mul": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_gauss_train": (C.c_int, [C.c_void_p, C.c_int] * 10 + [C.c_long, C.c_int, C.c_void_p]),
    "vam_gauss_levels_fwd": (C.c_int, [C.c_void_p, C.c_int] * 5 + [C.c_long, C.c_void_p, C.c_int, C.c_long] + [C.c_void_p, C.c_int, C.c_long] * 2
                             + [C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_gauss_levels_bwd": (C.c_int, [C.c_void_p, C.c_int] * 5 + [C.c_long] + [C.c_void_p, C.c_int, C.c_long] * 3 + [C.c_void_p, C.c_int] * 4
                             + [C.c_int, C.c_long, C.c_int, C.c_void_p]),
    "vam_train_elementwise": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "vam_train_axpy_group": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vam_stack_tail_group": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vam_win_attention_bwd_workspace": (C.c_size_t, [C.c_int] * 5),
    "vam_win_attention_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
                              + [C.c_int] * 7 + [C.c_void_p]),
    "vam_eb_train_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_long, C.c_void_p]),
    "vam_ps2_unshuffle": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_upsample2_zero": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_pmf_to_quantized_cdf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vam_rans_encode": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_long]),
    "vam_rans_decode": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_rans_encode_streams": (C.c_int, [C.POINTER(VamRansStream), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int]),
    "vam_rans_decode_streams": (C.c_int, [C.POINTER(VamRansStream), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int]),
    "vam_rans_decode_prefix_streams": (C.c_int, [C.POINTER(VamRansStream), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_void_p]),
    "vam_rans_prefix_bytes": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_rans_core_encode": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_long, C.c_void_p, C.c_int]),
    "vam_rans_core_decode": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int]),
    "vam_rans_core_encode_nhwc": (C.c_long, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_long]),
    "vam_rans_core_decode_nhwc": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p]),
    "vam_rans_lds_table_bytes": (C.c_int, []),
    "vam_rans_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.POINTER(VamRansTables), C.c_void_p,
                                         C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_pack_device": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]),
    "vam_rans_decode_device": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 8 + [C.POINTER(VamRansTables), C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_lanes_encode": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vam_rans_lanes_decode": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vam_rans_lanes_encode_nhwc": (C.c_long, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p]),
    "vam_rans_lanes_decode_nhwc": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_rans_lanes_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.POINTER(VamRansTables), C.c_void_p,
                                               C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_lanes_decode_device": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 9 + [C.POINTER(VamRansTables), C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "vam_rans_layers_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 10 + [C.POINTER(VamRansTables), C.c_void_p,
                                                C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_layers_decode_device": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 10 + [C.POINTER(VamRansTables), C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "vam_rans_interleaved_encode": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_long, C.c_int]),
    "vam_rans_interleaved_encode_streams": (C.c_int, [C.POINTER(VamRansStream), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_int, C.c_int]),
    "vam_rans_interleaved_decode_prefix": (C.c_long, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_rans_interleaved_decode_prefix_streams": (C.c_int, [C.POINTER(VamRansStream), C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vam_rans_interleaved_prefix_bytes": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_rans_interleaved_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.POINTER(VamRansTables),
                                                     C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_void_p]),
    "vam_rans_interleaved_decode_device": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long,
                                                     C.c_int, C.POINTER(VamRansTables), C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "vam_rans_interleaved_cut_table_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.POINTER(VamRansTables),
                                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_interleaved_encode_nhwc_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.POINTER(VamRansTables),
                                                          C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_interleaved_decode_nhwc_device": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8
                                                + [C.POINTER(VamRansTables), C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rans_interleaved_resume": (C.c_long, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(VamRansCheckpoint), C.c_void_p]),
    "vam_rans_interleaved_resume_streams": (C.c_int, [C.POINTER(VamRansStream), C.POINTER(VamRansCheckpoint), C.c_int, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_void_p]),
    "vam_rans_interleaved_resume_device": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long,
                                                     C.c_int, C.POINTER(VamRansTables)] + [C.c_void_p] * 7),
    "vam_variance_rank_workspace": (C.c_size_t, [C.c_int] * 4),
    "vam_variance_rank": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "vam_variance_rank_staged": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "vam_stage_ids": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                C.c_void_p]),
    "vam_rank_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "vam_rank_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "vam_rank_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_pool_keys": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                C.c_int, C.c_int, C.c_void_p]),
    "vam_pooled_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_threshold_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_tile_extract": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "vam_tile_blend": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_tile_schedule": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "vam_tile_refresh": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 13
                         + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_tile_compose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] + [C.c_int] * 7
                         + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vam_picture_halve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vam_picture_resample": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_int64] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p]),
    "vam_graph_begin": (C.c_int, [C.c_void_p]),
    "vam_graph_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "vam_graph_launch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vam_graph_destroy": (C.c_int, [C.c_void_p]),
    "vam_prof_enable": (C.c_int, [C.c_int]),
    "vam_prof_reset": (C.c_int, []),
    "vam_prof_read": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vam_prof_set_class": (C.c_int, [C.c_int]),
    "vam_prof_read_class": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class VamError(RuntimeError):
    pass


_lib = None


def load():
    """Load libvampic.so and bind every symbol of include/vampic.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VamError(
            f"libvampic.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.vam_conv_struct_size() != C.sizeof(VamConv):
        raise VamError(f"ABI mismatch: sizeof(vam_conv) is {lib.vam_conv_struct_size()} in libvampic.so, {C.sizeof(VamConv)} in the binding")
    if lib.vam_layer_params_size() != C.sizeof(VamLayerParams):
        raise VamError(f"ABI mismatch: sizeof(vam_layer_params) is {lib.vam_layer_params_size()} in libvampic.so, {C.sizeof(VamLayerParams)} in the binding")
    if lib.vam_resunit_struct_size() != C.sizeof(VamResunit):
        raise VamError(f"ABI mismatch: sizeof(vam_resunit) is {lib.vam_resunit_struct_size()} in libvampic.so, {C.sizeof(VamResunit)} in the binding")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().vam_last_error().decode(errors="replace")
        raise VamError(f"{what or 'libvampic'} failed ({rc}): {msg}")


def require_gpu():
    lib = load()
    name = C.create_string_buffer(128)
    cus = C.c_int(0)
    rc = lib.vam_device_info(name, C.byref(cus))
    if rc != 0:
        raise VamError("no HIP device: the variance-aware-masking hot path runs only on gfx950 (MI355X); "
                       + lib.vam_last_error().decode(errors="replace"))
    return name.value.decode(), cus.value
