"""Thin host-side wrappers over the C ABI.

``View`` is a channel window of an NHWC fp32 device buffer (``[B,H,W,ld]`` with
``C <= ld`` channels starting at ``c0``).  torch only owns the memory and the stream;
every arithmetic op below is a libvampic call.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


@dataclass
class View:
    buf: torch.Tensor   # [B, H, W, ld] fp32 contiguous, cuda
    c0: int
    C: int

    @property
    def B(self): return self.buf.shape[0]
    @property
    def H(self): return self.buf.shape[1]
    @property
    def W(self): return self.buf.shape[2]
    @property
    def ld(self): return self.buf.shape[3]
    @property
    def ptr(self): return self.buf.data_ptr() + 4 * self.c0
    @property
    def n_pix(self): return self.B * self.H * self.W

    def window(self, c0: int, C_: int) -> "View":
        assert 0 <= c0 and c0 + C_ <= self.C, (c0, C_, self.C)
        return View(self.buf, self.c0 + c0, C_)

    def torch_nchw(self) -> torch.Tensor:
        """Logical NCHW tensor sharing this window's memory (channels_last strides)."""
        return self.buf[..., self.c0:self.c0 + self.C].permute(0, 3, 1, 2)


@dataclass
class View3:
    """A channel window of a bf16x3-plane ("P3") tensor: [B, H, W, groups][plane 3][8 bf16], 48 bytes per 8-channel
    group (stored in an fp32 tensor of 12 floats per group).  Written by a conv launch with VAM_CONV_OUT_BF3 and read
    only by convolutions (VAM_CONV_IN_BF3): the exact hi/mid/lo split of each fp32 value, made once by the producer."""
    buf: torch.Tensor   # [B, H, W, 12 * groups] fp32 storage
    g0: int
    C: int

    @property
    def B(self): return self.buf.shape[0]
    @property
    def H(self): return self.buf.shape[1]
    @property
    def W(self): return self.buf.shape[2]
    @property
    def ld(self): return self.buf.shape[3] // 12      # groups per pixel
    @property
    def ptr(self): return self.buf.data_ptr() + 48 * self.g0
    @property
    def n_pix(self): return self.B * self.H * self.W

    def window(self, c0: int, C_: int) -> "View3":
        assert c0 % 8 == 0 and C_ % 8 == 0 and 0 <= c0 and c0 + C_ <= self.C
        return View3(self.buf, self.g0 + c0 // 8, C_)

    def to_float(self) -> torch.Tensor:
        """Decode to a [B,H,W,C] fp32 tensor (hi + mid + lo; test / debug helper)."""
        B, H, W = self.B, self.H, self.W
        raw = self.buf.view(torch.int16).view(B, H, W, self.ld, 3, 8)[..., self.g0:self.g0 + self.C // 8, :, :]
        planes = (raw.to(torch.int32) << 16).view(torch.float32)
        return (planes[..., 0, :] + planes[..., 1, :] + planes[..., 2, :]).reshape(B, H, W, self.C)


@dataclass
class View16:
    """A channel window of a bf16 NHWC tensor (bf16-storage mode, BASELINE configs[2]): activations of the large feature
    maps of g_a / g_s are kept in bf16; ``ld`` counts bf16 elements."""
    buf: torch.Tensor   # [B, H, W, ld] torch.bfloat16, cuda
    c0: int
    C: int

    @property
    def B(self): return self.buf.shape[0]
    @property
    def H(self): return self.buf.shape[1]
    @property
    def W(self): return self.buf.shape[2]
    @property
    def ld(self): return self.buf.shape[3]
    @property
    def ptr(self): return self.buf.data_ptr() + 2 * self.c0
    @property
    def n_pix(self): return self.B * self.H * self.W

    def window(self, c0: int, C_: int) -> "View16":
        assert c0 % 8 == 0 and C_ % 8 == 0 and 0 <= c0 and c0 + C_ <= self.C
        return View16(self.buf, self.c0 + c0, C_)

    def torch_nchw(self) -> torch.Tensor:
        return self.buf[..., self.c0:self.c0 + self.C].permute(0, 3, 1, 2).float()


def new_view16(B: int, H: int, W: int, C_: int, device="cuda") -> View16:
    assert C_ % 8 == 0
    return View16(torch.empty((B, H, W, C_), dtype=torch.bfloat16, device=device), 0, C_)


def new_view3(B: int, H: int, W: int, C_: int, device="cuda") -> View3:
    assert C_ % 8 == 0
    return View3(torch.zeros((B, H, W, (C_ // 8) * 12), dtype=torch.float32, device=device), 0, C_)


def split_mode() -> bool:
    """True when the convolution kernel runs on split bf16x3 operands (the default)."""
    return L.load().vam_conv_get_mode() == 1


def f16x2_mode() -> bool:
    """True when the convolution kernel runs on fp16x2 operands (opt-in: VAMPIC_CONV=f16x2 / vam_conv_set_mode(3))."""
    return L.load().vam_conv_get_mode() == 3


def amax_prepare(chunk: Sequence["L.VamConv"]):
    """fp16x2 mode, eager launches (``conv_group``): give every input segment of every problem of one grouped launch a
    max-|x| cell and return (cells, fn) where ``fn()`` zeroes the cells and reduces each segment into its cell on the
    current stream.  Plans avoid the re-read where the producer was a convolution (engine.Plan: ``out_amax`` cells)."""
    lib = L.load()
    cells = torch.zeros(len(chunk) * L.VAM_MAX_SEG, dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
    base = cells.data_ptr()
    todo = []
    for i, c in enumerate(chunk):
        c._amax_cells = cells            # the structs point into ``cells``: it lives as long as they do
        if c.flags & (L.CONV_W_BF16 | L.CONV_IN_BF3):
            continue
        for k in range(c.n_seg):
            cell = base + 4 * (i * L.VAM_MAX_SEG + k)
            c.in_amax[k] = cell
            todo.append((c, k, cell))

    def fill():
        if not todo:
            return
        s = stream_ptr()
        L.check(lib.vam_memset_zero(base, 4 * cells.numel(), s), "vam_memset_zero")
        for c, k, cell in todo:
            L.check(lib.vam_absmax(C.byref(c.seg[k]), 1, c.B * c.H * c.W, cell, s), "vam_absmax")
    return cells, fill


def new_view(B: int, H: int, W: int, C_: int, device="cuda", zero: bool = False) -> View:
    f = torch.zeros if zero else torch.empty
    return View(f((B, H, W, C_), dtype=torch.float32, device=device), 0, C_)


def from_nchw(x: torch.Tensor) -> View:
    """NCHW (any strides) -> NHWC view.  Uses the layout kernel for plain-contiguous inputs;
    a channels_last tensor is already NHWC in memory and is wrapped without a copy."""
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_cuda, "expected a cuda fp32 NCHW tensor"
    B, C_, H, W = x.shape
    xp = x.permute(0, 2, 3, 1)
    if xp.is_contiguous():
        return View(xp, 0, C_)
    x = x.contiguous()
    out = new_view(B, H, W, C_)
    L.check(L.load().vam_nchw_to_nhwc(x.data_ptr(), out.ptr, B, C_, H, W, out.ld, stream_ptr()), "vam_nchw_to_nhwc")
    return out


def to_nchw(v: View) -> torch.Tensor:
    out = torch.empty((v.B, v.C, v.H, v.W), dtype=torch.float32, device=v.buf.device)
    L.check(L.load().vam_nhwc_to_nchw(v.ptr, v.ld, out.data_ptr(), v.B, v.C, v.H, v.W, stream_ptr()), "vam_nhwc_to_nchw")
    return out


# --------------------------------------------------------------------------- weights
@dataclass
class Packed:
    """A conv problem's constant part: packed weights + bias and its geometry."""
    w: torch.Tensor
    b: Optional[torch.Tensor]
    kh: int
    kw: int
    cin: int
    n: int
    stride: int = 1
    pad_y: int = 0
    pad_x: int = 0
    ps2_cq: int = 0          # >0: PixelShuffle-style phase scatter with Cq channels per phase
    osy: int = 1
    osx: int = 1
    ooy: int = 0
    oox: int = 0
    w16: bool = False        # weights rounded to bf16 (vam_pack_conv_weights_bf16): the bf16-storage kernel


def pack_weights(src: torch.Tensor, mode: int, phase: int, kh: int, kw: int, cin: int, n: int, bf16: bool = False) -> torch.Tensor:
    lib = L.load()
    src = src.detach().to(dtype=torch.float32).contiguous()
    assert src.is_cuda
    if bf16:
        dst = torch.empty(lib.vam_conv_wpack_bf16_bytes(kh, kw, cin, n) // 4, dtype=torch.float32, device=src.device)
        L.check(lib.vam_pack_conv_weights_bf16(src.data_ptr(), dst.data_ptr(), mode, phase, kh, kw, cin, n, stream_ptr()),
                "vam_pack_conv_weights_bf16")
        return dst
    dst = torch.empty(lib.vam_conv_wpack_floats(kh, kw, cin, n), dtype=torch.float32, device=src.device)
    L.check(lib.vam_pack_conv_weights(src.data_ptr(), dst.data_ptr(), mode, phase, kh, kw, cin, n, stream_ptr()),
            "vam_pack_conv_weights")
    return dst


_PACK_JOBS: Optional[list] = None      # inside ``pack_batch()``: deferred (job, keep-alive) pairs


class pack_batch:
    """``with ops.pack_batch(): ...`` — the repack calls inside are collected and issued as grouped launches
    (``vam_pack_group``) when the block ends, on the stream that is current then.  Nothing may read the packed buffers
    inside the block."""

    def __enter__(self):
        global _PACK_JOBS
        self.prev, _PACK_JOBS = _PACK_JOBS, []
        return self

    def __exit__(self, *exc):
        global _PACK_JOBS
        jobs, _PACK_JOBS = _PACK_JOBS, self.prev
        if exc[0] is None and jobs:
            arr = (L.VamPackJob * len(jobs))(*[j for j, _ in jobs])
            L.check(L.load().vam_pack_group(arr, len(jobs), stream_ptr()), "vam_pack_group")
        return False


def _pack_job(src: torch.Tensor, dst: torch.Tensor, bias: bool, mode: int, phase: int, kh: int, kw: int, cin: int, n: int) -> bool:
    if _PACK_JOBS is None:
        return False
    j = L.VamPackJob()
    j.src, j.dst, j.bias, j.mode, j.phase, j.kh, j.kw, j.cin, j.n = src.data_ptr(), dst.data_ptr(), int(bias), mode, phase, kh, kw, cin, n
    _PACK_JOBS.append((j, (src, dst)))
    return True


def pack_bias(src: torch.Tensor, mode: int, n: int) -> torch.Tensor:
    lib = L.load()
    src = src.detach().to(dtype=torch.float32).contiguous()
    dst = torch.empty(n, dtype=torch.float32, device=src.device)
    L.check(lib.vam_pack_bias(src.data_ptr(), dst.data_ptr(), mode, n, stream_ptr()), "vam_pack_bias")
    return dst


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, bf16: bool = False) -> Packed:
    """nn.Conv2d(k, stride, padding=k//2)  (reference layers/layers.py:5-12,24-26,77-79)."""
    n, cin, kh, kw = weight.shape
    return Packed(pack_weights(weight, L.PACK_CONV, 0, kh, kw, cin, n, bf16),
                  None if bias is None else pack_bias(bias, L.PACK_CONV, n),
                  kh, kw, cin, n, stride, kh // 2, kw // 2, w16=bf16)


def pack_linear(weight: torch.Tensor, bias: Optional[torch.Tensor], bf16: bool = False) -> Packed:
    n, cin = weight.shape
    return Packed(pack_weights(weight, L.PACK_CONV, 0, 1, 1, cin, n, bf16),
                  None if bias is None else pack_bias(bias, L.PACK_CONV, n), 1, 1, cin, n, w16=bf16)


def pack_subpel(weight: torch.Tensor, bias: torch.Tensor) -> Packed:
    """conv3x3(Cin -> 4*Cq) + PixelShuffle(2)  (layers/layers.py:82-86)."""
    n, cin, kh, kw = weight.shape
    return Packed(pack_weights(weight, L.PACK_PS2, 0, kh, kw, cin, n), pack_bias(bias, L.PACK_PS2, n),
                  kh, kw, cin, n, 1, kh // 2, kw // 2, ps2_cq=n // 4)


def pack_conv5s2_rgb(weight: torch.Tensor, bias: torch.Tensor, bf16: bool = False) -> Packed:
    """conv5x5 s2 pad2 on 3 input channels as a 3x3 s1 problem over the space-to-depth
    input of vam_s2d_input (16 channels = (py,px,c) + 4 zeros).  Pure re-indexing of the
    weights (a gather of existing values and zeros): w'[n,(py,px,c),ty,tx] = w[n,c,2ty+py,2tx+px]."""
    n, cin, kh, kw = weight.shape
    assert cin == 3 and kh == 5 and kw == 5
    w6 = torch.zeros((n, 3, 6, 6), dtype=torch.float32, device=weight.device)
    w6[:, :, :5, :5] = weight.detach()
    w = w6.reshape(n, 3, 3, 2, 3, 2).permute(0, 3, 5, 1, 2, 4).reshape(n, 12, 3, 3)   # [n,(py,px,c),ty,tx]
    w16 = torch.zeros((n, 16, 3, 3), dtype=torch.float32, device=weight.device)
    w16[:, :12] = w
    return Packed(pack_weights(w16, L.PACK_CONV, 0, 3, 3, 16, n, bf16), pack_bias(bias, L.PACK_CONV, n),
                  3, 3, 16, n, 1, 1, 1, w16=bf16)


def pack_deconv(weight: torch.Tensor, bias: torch.Tensor, bf16: bool = False) -> List[Packed]:
    """ConvTranspose2d(k5,s2,p2,op1) (layers/layers.py:14-22) as sub-pixel phase problems.
    Cout % 4 == 0: four problems (taps 3x3,3x2,2x3,2x2) writing interleaved output pixels.
    Otherwise (Cout = 3): one merged 3x3 problem with phase-major channels + PS2 scatter."""
    cin, cout, kh, kw = weight.shape
    assert kh == 5 and kw == 5
    if cout % 4 == 0:
        b = pack_bias(bias, L.PACK_CONV, cout)
        out = []
        for ph in range(4):
            py, px = ph >> 1, ph & 1
            k_h, k_w = (2 if py else 3), (2 if px else 3)
            out.append(Packed(pack_weights(weight, L.PACK_DECONV5S2, ph, k_h, k_w, cin, cout, bf16), b, k_h, k_w, cin, cout,
                              1, 0 if py else 1, 0 if px else 1, osy=2, osx=2, ooy=py, oox=px, w16=bf16))
        return out
    n = 4 * cout
    return [Packed(pack_weights(weight, L.PACK_DECONV5S2, -1, 3, 3, cin, n, bf16), pack_bias(bias, L.PACK_DECONV5S2, n),
                   3, 3, cin, n, 1, 1, 1, ps2_cq=cout, w16=bf16)]


def pack_gdn(beta: torch.Tensor, gamma: torch.Tensor, bf16: bool = False) -> Packed:
    """GDN norm pool as a 1x1 problem on x^2 with the reparametrised gamma/beta (layers/gdn.py:62-69)."""
    c = beta.shape[0]
    return Packed(pack_weights(gamma, L.PACK_GDN, 0, 1, 1, c, c, bf16), pack_bias(beta, L.PACK_GDN, c), 1, 1, c, c, w16=bf16)


# --------------------------------------------------------------------------- conv problems
def _aux(v: Optional[View]) -> L.VamAux:
    a = L.VamAux()
    if v is not None:
        a.ptr = v.ptr
        a.ld = v.ld
    return a


def conv_problem(pk: Packed, inputs: Sequence[View], out: View, act: int = L.ACT_NONE, *,
                 pre: Optional[View] = None, mul: Optional[View] = None, post: Optional[View] = None,
                 post2: Optional[View] = None, flags: int = 0, out_nchw: Optional[torch.Tensor] = None,
                 preact: Optional[View] = None, gelu_z: Optional[View] = None) -> L.VamConv:
    """Describe one problem.  ``inputs`` are concatenated along channels (virtually).  Training plans: ``preact`` = a second
    output holding the value the activation is applied to (the taped input of a GELU); ``gelu_z`` = the pre-activation of
    the GELU in FRONT of this (data-gradient) layer — the result is multiplied by gelu'(z): (conv + bias + pre) * gelu'(z)."""
    if gelu_z is not None:
        assert mul is None and act == L.ACT_NONE and type(gelu_z) is View
        mul, flags = gelu_z, flags | L.CONV_MUL_GELU_GRAD
    c = L.VamConv()
    assert 1 <= len(inputs) <= L.VAM_MAX_SEG
    in3 = isinstance(inputs[0], View3)
    assert all(isinstance(v, View3) == in3 for v in inputs), "a conv problem reads either fp32 or bf16x3-plane segments"
    in16 = isinstance(inputs[0], View16)
    assert all(isinstance(v, View16) == in16 for v in inputs), "a conv problem reads either fp32 or bf16 segments"
    if in3:
        flags |= L.CONV_IN_BF3
    if isinstance(out, View3):
        assert out_nchw is None
        flags |= L.CONV_OUT_BF3
    auxs = [a for a in (pre, mul, post, post2) if a is not None]
    aux16 = bool(auxs) and isinstance(auxs[0], View16)
    assert all(isinstance(a, View16) == aux16 for a in auxs), "epilogue operands of one problem share a storage type"
    if in16 or isinstance(out, View16) or aux16 or pk.w16:
        assert pk.w16, "bf16-stored tensors are read / written by the bf16-weight kernel: pack the layer with bf16=True"
        flags |= L.CONV_W_BF16 | (L.CONV_IN_BF16 if in16 else 0) | (L.CONV_OUT_BF16 if isinstance(out, View16) else 0) | \
            (L.CONV_AUX_BF16 if aux16 else 0)
    B, H, W = inputs[0].B, inputs[0].H, inputs[0].W
    cin = 0
    for i, v in enumerate(inputs):
        assert (v.B, v.H, v.W) == (B, H, W), "all input segments must share the spatial extent"
        c.seg[i].ptr = v.ptr
        c.seg[i].C = v.C
        c.seg[i].ld = v.ld
        cin += v.C
    assert cin == pk.cin, f"conv expects {pk.cin} input channels, got {cin}"
    c.n_seg = len(inputs)
    c.B, c.H, c.W = B, H, W
    c.kh, c.kw, c.stride, c.pad_y, c.pad_x = pk.kh, pk.kw, pk.stride, pk.pad_y, pk.pad_x
    if pk.stride == 1:
        Ho, Wo = H, W
    else:
        Ho = (H + 2 * pk.pad_y - pk.kh) // pk.stride + 1
        Wo = (W + 2 * pk.pad_x - pk.kw) // pk.stride + 1
    c.Ho, c.Wo = Ho, Wo
    c.N = pk.n
    c.wpack = pk.w.data_ptr()
    c.bias = pk.b.data_ptr() if pk.b is not None else None
    c.osy, c.osx, c.ooy, c.oox = pk.osy, pk.osx, pk.ooy, pk.oox
    c.Cq = pk.ps2_cq
    c.act = act
    c.flags = flags | (L.CONV_PS2 if pk.ps2_cq else 0)
    if out_nchw is not None:
        assert out_nchw.is_contiguous()
        c.flags |= L.CONV_OUT_NCHW
        c.out = out_nchw.data_ptr()
        c.Hf, c.Wf = out_nchw.shape[2], out_nchw.shape[3]
        c.ldo = 0
        cexp = pk.ps2_cq if pk.ps2_cq else pk.n
        assert out_nchw.shape[0] == B and out_nchw.shape[1] == cexp
    else:
        c.out = out.ptr
        c.ldo = out.ld
        c.Hf, c.Wf = out.H, out.W
        cexp = pk.ps2_cq if pk.ps2_cq else pk.n
        assert out.B == B and out.C == cexp, f"output window has {out.C} channels, problem writes {cexp}"
    if pk.ps2_cq:
        assert (c.Hf, c.Wf) == (2 * Ho, 2 * Wo)
    else:
        assert (Ho - 1) * pk.osy + pk.ooy < c.Hf and (Wo - 1) * pk.osx + pk.oox < c.Wf
    c.pre, c.mul, c.post, c.post2 = _aux(pre), _aux(mul), _aux(post), _aux(post2)
    if preact is not None:
        assert type(preact) is View and out_nchw is None and preact.B == B and (preact.H, preact.W) == (c.Hf, c.Wf) and \
            preact.C == (pk.ps2_cq if pk.ps2_cq else pk.n), "preact is an fp32 NHWC tensor of the output's shape"
        c.preact = _aux(preact)
    return c


def conv_group(problems: Sequence[L.VamConv]):
    lib = L.load()
    s = stream_ptr()
    for i in range(0, len(problems), L.VAM_MAX_GROUP):
        chunk = problems[i:i + L.VAM_MAX_GROUP]
        if f16x2_mode():
            cells, fill = amax_prepare(chunk)
            fill()
        arr = (L.VamConv * len(chunk))(*chunk)
        L.check(lib.vam_conv_group(arr, len(chunk), s), "vam_conv_group")


# --------------------------------------------------------------------------- fused residual unit
def resunit_supported(x) -> bool:
    """A fused kernel exists for this unit's shape (csrc/resunit.hip: C = 192; fp32 tensors in the split-operand mode, or
    bf16-stored tensors of the bf16-storage mode)."""
    if os.environ.get("VAMPIC_FUSED_RU", "1") == "0":
        return False
    if type(x) is View:
        if not split_mode():
            return False
    elif type(x) is not View16:
        return False
    return bool(L.load().vam_resunit_supported(x.C, x.H, x.W))


def resunit_problem(p1: Packed, p2: Packed, p3: Packed, x, out) -> "L.VamResunit":
    """One ResidualUnit (layers/layers.py:30-48) as a single launch; p1 / p2 / p3 are the ordinary packed weights of
    its 1x1 (C -> C/2), 3x3 (C/2 -> C/2) and 1x1 (C/2 -> C) convolutions — bf16-packed ones (``m.packed(True)``) when
    x / out are bf16-stored tensors."""
    b16 = type(x) is View16
    assert type(out) is type(x) and type(x) in (View, View16), "the fused residual unit reads and writes fp32 or bf16 NHWC tensors"
    assert (out.B, out.H, out.W, out.C) == (x.B, x.H, x.W, x.C)
    C_ = x.C
    assert (p1.kh, p1.cin, p1.n) == (1, C_, C_ // 2) and (p2.kh, p2.kw, p2.cin, p2.n, p2.stride) == (3, 3, C_ // 2, C_ // 2, 1) and \
        (p3.kh, p3.cin, p3.n) == (1, C_ // 2, C_), "residual unit: conv1x1(C, C/2), conv3x3(C/2, C/2), conv1x1(C/2, C)"
    assert p1.w16 == p2.w16 == p3.w16 == b16 and p1.b is not None and p2.b is not None and p3.b is not None
    c = L.VamResunit()
    c.x, c.out, c.ldx, c.ldo = x.ptr, out.ptr, x.ld, out.ld
    c.B, c.H, c.W, c.C = x.B, x.H, x.W, C_
    c.w1, c.b1 = p1.w.data_ptr(), p1.b.data_ptr()
    c.w2, c.b2 = p2.w.data_ptr(), p2.b.data_ptr()
    c.w3, c.b3 = p3.w.data_ptr(), p3.b.data_ptr()
    c.flags = L.RESUNIT_BF16 if b16 else 0
    return c


def resunit_group(problems: Sequence["L.VamResunit"]):
    lib = L.load()
    s = stream_ptr()
    for i in range(0, len(problems), L.VAM_MAX_GROUP):
        chunk = problems[i:i + L.VAM_MAX_GROUP]
        arr = (L.VamResunit * len(chunk))(*chunk)
        L.check(lib.vam_resunit_group(arr, len(chunk), s), "vam_resunit_group")


# --------------------------------------------------------------------------- other ops
def s2d_input(x: torch.Tensor) -> View:
    B, C_, H, W = x.shape
    assert C_ == 3 and x.is_cuda and x.dtype == torch.float32
    x = x.contiguous()
    out = new_view(B, H // 2, W // 2, 16)
    L.check(L.load().vam_s2d_input(x.data_ptr(), out.ptr, B, H, W, stream_ptr()), "vam_s2d_input")
    return out


def win_attention(qkv: View, out: View, table: torch.Tensor, C_: int, heads: int, ws: int, shift: int):
    L.check(L.load().vam_win_attention(qkv.ptr, qkv.ld, out.ptr, out.ld, table.data_ptr(), qkv.B, qkv.H, qkv.W, C_, heads,
                                       ws, shift, stream_ptr()), "vam_win_attention")


def _segments(sigma: View, n_slice: int, slice_C: Optional[int] = None):
    """(the eight leading arguments of every variance-mask entry point, slice_C, H * W): ``sigma``'s window as ``n_slice``
    consecutive slices of ``slice_C`` channels per image, one segment per (image, slice)."""
    slice_C = slice_C or sigma.C // n_slice
    assert slice_C * n_slice == sigma.C
    hw = sigma.H * sigma.W
    return (sigma.ptr, sigma.ld, hw * sigma.ld, slice_C, sigma.B, n_slice, hw, slice_C), slice_C, hw


def _thr_ptr(thr: Optional[torch.Tensor], rows: int, sigma: View, n_slice: int, any_dtype: bool = False):
    """The pointer of ``thr`` (optional): ``rows`` levels of one fp32 threshold per segment."""
    assert thr is None or ((any_dtype or thr.dtype == torch.float32) and thr.numel() >= rows * sigma.B * n_slice)
    return thr.data_ptr() if thr is not None else None


def _assert_table(table_dev: torch.Tensor, sigma: View):
    """``table_dev``: one L.VamLayerParams record per image of ``sigma``, as bytes on its device."""
    assert table_dev.dtype == torch.uint8 and table_dev.is_contiguous() and table_dev.device == sigma.buf.device and \
        table_dev.numel() >= sigma.B * C.sizeof(L.VamLayerParams)


def _quality_table(params: str, prs_per_image: Sequence[Sequence[float]], n_pix: int, C_: int):
    """(host bytes of one L.VamLayerParams record per image, the longest list's length) from the library's host
    arithmetic ``params`` (vam_variance_layer_params / vam_variance_mask_params)."""
    lists = [[float(p_) for p_ in row] for row in prs_per_image]
    B = len(lists)
    width = max([len(r) for r in lists] + [1])
    flat = (C.c_double * (width * max(B, 1)))(*[v for r in lists for v in r + [0.0] * (width - len(r))])
    nl = (C.c_int * max(B, 1))(*[len(r) for r in lists])
    table = np.zeros(B * C.sizeof(L.VamLayerParams), dtype=np.uint8)
    L.check(getattr(L.load(), params)(flat, nl, B, width, n_pix, C_, table.ctypes.data), params)
    return table, width


def variance_mask(sigma: View, pr: float, mask: View, n_slice: int = 1, slice_C: Optional[int] = None,
                  thr: Optional[torch.Tensor] = None):
    """sigma/mask windows hold n_slice consecutive slices of slice_C channels each; one
    quantile per (batch item, slice)."""
    seg, slice_C, hw = _segments(sigma, n_slice, slice_C)
    assert sigma.C == mask.C
    L.check(L.load().vam_variance_mask(*seg, float(pr), mask.ptr, mask.ld, hw * mask.ld, slice_C,
                                       thr.data_ptr() if thr is not None else None, stream_ptr()), "vam_variance_mask")


def variance_mask_levels(sigma: View, prs: Sequence[float], mask: View, n_slice: int = 1, level_stride: Optional[int] = None,
                         thr: Optional[torch.Tensor] = None):
    """The masks of several qualities in one launch: level l's mask is ``mask`` shifted by l * ``level_stride`` floats
    (default: the next ``sigma.B`` images, i.e. ``mask`` holds [L * B, H, W, ld]); ``thr`` [L, B * n_slice].  Bit-identical
    to one :func:`variance_mask` per level."""
    seg, slice_C, hw = _segments(sigma, n_slice)
    assert sigma.C == mask.C and sigma.H == mask.H and sigma.W == mask.W
    prs = [float(p_) for p_ in prs]
    nl = len(prs)
    if level_stride is None:
        assert mask.B == nl * sigma.B, (mask.B, nl, sigma.B)
        level_stride = sigma.B * hw * mask.ld
    arr = (C.c_double * max(nl, 1))(*prs)
    L.check(L.load().vam_variance_mask_levels(*seg, arr, nl, mask.ptr, mask.ld, hw * mask.ld, slice_C, level_stride,
                                              _thr_ptr(thr, nl, sigma, n_slice, any_dtype=True), stream_ptr()),
            "vam_variance_mask_levels")


def variance_layers(sigma: View, prs: Sequence[float], layer: torch.Tensor, n_slice: int = 1,
                    thr: Optional[torch.Tensor] = None):
    """Container layer of every element for the non-decreasing quality list ``prs`` (up to L.VAM_MAX_LAYER_LEVELS, one
    launch): ``layer`` uint8 [B, H, W, sigma.C] gets the first k with ``variance_mask(sigma, prs[k])`` == 1 (L.LAYER_NONE if
    none); ``thr`` [L, B * n_slice] the thresholds as :func:`variance_mask_levels` writes them."""
    seg, slice_C, hw = _segments(sigma, n_slice)
    assert layer.dtype == torch.uint8 and layer.is_contiguous() and tuple(layer.shape) == (sigma.B, sigma.H, sigma.W, sigma.C)
    prs = [float(p_) for p_ in prs]
    nl = len(prs)
    arr = (C.c_double * max(nl, 1))(*prs)
    L.check(L.load().vam_variance_layers(*seg, arr, nl, layer.data_ptr(), sigma.C, hw * sigma.C, slice_C,
                                         _thr_ptr(thr, nl, sigma, n_slice), stream_ptr()), "vam_variance_layers")


def variance_layers_per_image(sigma: View, prs: Sequence[Sequence[float]], layer: torch.Tensor, n_slice: int = 1,
                              thr: Optional[torch.Tensor] = None):
    """:func:`variance_layers` with one non-decreasing quality list per image (``prs[b]``, 1..L.VAM_MAX_LAYER_LEVELS entries,
    the lengths may differ) in ONE launch: image b's layer ids equal ``variance_layers`` on image b alone with ``prs[b]``,
    byte for byte; ``thr`` [max length, B * n_slice] gets level k of image b at [k, b * n_slice + j] for k < len(prs[b]).
    The per-image ranks and weights are host arithmetic (vam_variance_layer_params); their table is copied to the device
    here, so this call cannot be captured into a graph."""
    seg, slice_C, hw = _segments(sigma, n_slice)
    assert len(prs) == sigma.B
    assert layer.dtype == torch.uint8 and layer.is_contiguous() and tuple(layer.shape) == (sigma.B, sigma.H, sigma.W, sigma.C)
    table, width = _quality_table("vam_variance_layer_params", prs, hw, slice_C)
    variance_layers_table(sigma, torch.from_numpy(table).to(sigma.buf.device), layer, n_slice=n_slice, thr=thr, thr_levels=width)
    # the device copy of the table returns to the allocator of this same stream


def mask_table(prs_per_image: Sequence[Sequence[float]], n_pix: int, C_: int) -> np.ndarray:
    """The host bytes (uint8, one L.VamLayerParams record per image) of the table :func:`variance_masks_per_image` reads:
    image b's qualities ``prs_per_image[b]`` (1..L.VAM_MAX_MASK_LEVELS, any order, repeats allowed) for segments of
    ``n_pix`` pixels x ``C_`` channels.  Host arithmetic only (vam_variance_mask_params)."""
    return _quality_table("vam_variance_mask_params", prs_per_image, n_pix, C_)[0]


def variance_masks_per_image(sigma: View, table_dev: torch.Tensor, mask: View, n_slice: int = 1,
                             level_stride: Optional[int] = None, thr: Optional[torch.Tensor] = None,
                             max_levels: Optional[int] = None):
    """:func:`variance_mask_levels` with image b's quality list read from record b of ``table_dev`` (the bytes of
    :func:`mask_table` on the device), so the call can be captured and the captured graph serves every table content.
    Level l's mask is ``mask`` shifted by l * ``level_stride`` floats (default: ``mask`` holds [L * B, H, W, ld] and the
    table may hold up to L = mask.B // sigma.B levels per image; with an explicit stride ``max_levels`` says how many
    the buffers hold); ``thr`` [L, B * n_slice].  Bit-identical per (image, level) to :func:`variance_mask` on that image."""
    seg, slice_C, hw = _segments(sigma, n_slice)
    assert sigma.C == mask.C and sigma.H == mask.H and sigma.W == mask.W
    if level_stride is None:
        assert mask.B % sigma.B == 0 and mask.B >= sigma.B, (mask.B, sigma.B)
        max_levels = mask.B // sigma.B if max_levels is None else max_levels
        assert max_levels * sigma.B <= mask.B
        level_stride = sigma.B * hw * mask.ld
    assert max_levels is not None and 1 <= max_levels <= L.VAM_MAX_MASK_LEVELS, max_levels
    # the last element the kernel may write lies inside the mask's buffer
    assert level_stride >= 0 and mask.c0 + (max_levels - 1) * level_stride + (sigma.B * hw - 1) * mask.ld + mask.C <= mask.buf.numel()
    _assert_table(table_dev, sigma)
    L.check(L.load().vam_variance_masks_per_image(*seg, table_dev.data_ptr(), max_levels, mask.ptr, mask.ld, hw * mask.ld, slice_C,
                                                  level_stride, _thr_ptr(thr, max_levels, sigma, n_slice), stream_ptr()),
            "vam_variance_masks_per_image")


def layer_table(prs_per_image: Sequence[Sequence[float]], n_pix: int, C_: int) -> np.ndarray:
    """The host bytes (uint8, one L.VamLayerParams record per image) of the table :func:`variance_mask_map` (and
    vam_variance_layers_per_image) reads: image b's non-decreasing qualities ``prs_per_image[b]`` (1..L.VAM_MAX_LAYER_LEVELS)
    for segments of ``n_pix`` pixels x ``C_`` channels.  Host arithmetic only (vam_variance_layer_params)."""
    return _quality_table("vam_variance_layer_params", prs_per_image, n_pix, C_)[0]


def variance_mask_map(sigma: View, table_dev: torch.Tensor, level_map: torch.Tensor, mask: View, n_slice: int = 1,
                      thr: Optional[torch.Tensor] = None):
    """ONE mask in which every latent pixel takes its own quality: image b's sorted quality list is
    record b of ``table_dev`` (the bytes of :func:`layer_table` on the device), ``level_map`` uint8 [B, H * W] (or
    [B, H, W]) the index of each pixel's quality in it.  At the pixels of level k the mask is bit-identical to
    :func:`variance_mask` on that image alone at that quality; an index beyond the image's list writes 0.  ``thr``
    [L.VAM_MAX_LAYER_LEVELS, B * n_slice]: level k of image b at [k, b * n_slice + j] for k < the image's count.  Table and
    map are device buffers, so the call can be captured and the captured graph serves every map."""
    seg, slice_C, hw = _segments(sigma, n_slice)
    assert sigma.C == mask.C and (sigma.B, sigma.H, sigma.W) == (mask.B, mask.H, mask.W)
    _assert_table(table_dev, sigma)
    assert level_map.dtype == torch.uint8 and level_map.is_contiguous() and level_map.device == sigma.buf.device and \
        level_map.numel() == sigma.B * hw, (level_map.dtype, tuple(level_map.shape), sigma.B, hw)
    L.check(L.load().vam_variance_mask_map(*seg, table_dev.data_ptr(), level_map.data_ptr(), hw, mask.ptr, mask.ld, hw * mask.ld,
                                           slice_C, _thr_ptr(thr, L.VAM_MAX_LAYER_LEVELS, sigma, n_slice), stream_ptr()),
            "vam_variance_mask_map")


# --------------------------------------------------------------------------- rank order (embedded streams)
def rank_workspace(sigma: View, n_slice: int, device=None) -> Optional[torch.Tensor]:
    """The workspace :func:`variance_rank` needs for the segments of ``sigma`` (None when they fit LDS).  Raises for
    segments above L.VAM_MAX_RANK_ELEMENTS elements."""
    slice_C = sigma.C // n_slice
    n = L.load().vam_variance_rank_workspace(sigma.B, n_slice, sigma.H * sigma.W, slice_C)
    if sigma.H * sigma.W * slice_C > L.VAM_MAX_RANK_ELEMENTS:
        raise ValueError(f"rank order: segments of {sigma.H * sigma.W * slice_C} elements exceed {L.VAM_MAX_RANK_ELEMENTS}")
    return torch.empty((n // 8,), dtype=torch.int64, device=device or sigma.buf.device) if n else None


def variance_rank(sigma: View, perm: torch.Tensor, n_slice: int = 1, workspace: Optional[torch.Tensor] = None):
    """``perm`` int32 [B, n_slice, n] (n = slice_C * H * W) gets, per (image, slice) segment of ``sigma``, the permutation
    that sorts it by descending sigma: numpy.argsort(-s, kind="stable") with s flattened in the canonical [C, H, W] order
    of a stream.  ``workspace``: :func:`rank_workspace` (segments above 8192 elements).  No allocation: capturable."""
    slice_C = sigma.C // n_slice
    hw = sigma.H * sigma.W
    assert slice_C * n_slice == sigma.C
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == sigma.B * n_slice * hw * slice_C
    assert workspace is None or (workspace.dtype == torch.int64 and workspace.is_contiguous())
    L.check(L.load().vam_variance_rank(sigma.ptr, sigma.ld, hw * sigma.ld, slice_C, sigma.B, n_slice, hw, slice_C, perm.data_ptr(),
                                       workspace.data_ptr() if workspace is not None else None,
                                       8 * workspace.numel() if workspace is not None else 0, stream_ptr()), "vam_variance_rank")


def variance_layers_table(sigma: View, table_dev: torch.Tensor, layer: torch.Tensor, n_slice: int = 1,
                          thr: Optional[torch.Tensor] = None, thr_levels: int = L.VAM_MAX_LAYER_LEVELS):
    """:func:`variance_layers_per_image` with image b's list read from record b of ``table_dev`` (the bytes of
    :func:`layer_table` on the device): no host arithmetic and no copy, so the call can be captured and the captured
    launch serves every table content.  ``thr`` holds ``thr_levels`` rows, at least the longest list of the table."""
    seg, slice_C, hw = _segments(sigma, n_slice)
    assert layer.dtype == torch.uint8 and layer.is_contiguous() and tuple(layer.shape) == (sigma.B, sigma.H, sigma.W, sigma.C)
    _assert_table(table_dev, sigma)
    L.check(L.load().vam_variance_layers_per_image(*seg, table_dev.data_ptr(), layer.data_ptr(), sigma.C,
                                                   hw * sigma.C, slice_C,
                                                   _thr_ptr(thr, thr_levels, sigma, n_slice), stream_ptr()),
            "vam_variance_layers_per_image")


def stage_ids(layer: torch.Tensor, stage_map: torch.Tensor, n_stages: torch.Tensor, stage: torch.Tensor):
    """Scheduled embedded streams: ``stage`` uint8 [B, H, W, Ct] gets, for the layer ids ``layer`` of
    :func:`variance_layers_per_image` (same shape), the first stage k < n_stages[b] whose index map reaches the id,
    ``stage_map[b, k, p] >= layer[e]``, L.LAYER_NONE when none does or when n_stages[b] is outside
    1..L.VAM_MAX_LAYER_LEVELS.  ``stage_map`` uint8 [B, L.VAM_MAX_LAYER_LEVELS, H * W] and ``n_stages`` int32 [B] are device
    buffers, so the call can be captured and the captured launch serves every schedule."""
    B, H, W, Ct = layer.shape
    dev = layer.device
    assert layer.dtype == torch.uint8 and layer.is_contiguous() and layer.is_cuda
    assert stage.dtype == torch.uint8 and stage.is_contiguous() and stage.shape == layer.shape and stage.device == dev
    assert stage_map.dtype == torch.uint8 and stage_map.is_contiguous() and stage_map.device == dev and \
        stage_map.numel() == B * L.VAM_MAX_LAYER_LEVELS * H * W, (tuple(stage_map.shape), B, H, W)
    assert n_stages.dtype == torch.int32 and n_stages.is_contiguous() and n_stages.device == dev and n_stages.numel() == B
    L.check(L.load().vam_stage_ids(layer.data_ptr(), Ct, stage_map.data_ptr(), n_stages.data_ptr(), B, H * W, Ct,
                                   stage.data_ptr(), Ct, stream_ptr()), "vam_stage_ids")


def variance_rank_staged(sigma: View, stage: torch.Tensor, perm: torch.Tensor, n_slice: int = 1,
                         workspace: Optional[torch.Tensor] = None):
    """:func:`variance_rank` with the ids of :func:`stage_ids` (uint8 [B, H, W, sigma.C]) as the major key: ascending
    stage, within a stage descending sigma with :func:`variance_rank`'s ties.  With o = numpy.argsort(-s, kind="stable"),
    ``perm`` = o[numpy.argsort(stage[o], kind="stable")].  Same workspace (:func:`rank_workspace`); capturable."""
    slice_C = sigma.C // n_slice
    hw = sigma.H * sigma.W
    assert slice_C * n_slice == sigma.C
    assert stage.dtype == torch.uint8 and stage.is_contiguous() and tuple(stage.shape) == (sigma.B, sigma.H, sigma.W, sigma.C) \
        and stage.device == sigma.buf.device
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == sigma.B * n_slice * hw * slice_C
    assert workspace is None or (workspace.dtype == torch.int64 and workspace.is_contiguous())
    L.check(L.load().vam_variance_rank_staged(sigma.ptr, sigma.ld, hw * sigma.ld, slice_C, stage.data_ptr(), sigma.C, sigma.B,
                                              n_slice, hw, slice_C, perm.data_ptr(),
                                              workspace.data_ptr() if workspace is not None else None,
                                              8 * workspace.numel() if workspace is not None else 0, stream_ptr()),
            "vam_variance_rank_staged")


def _rank_view(v: "IView", n_slice: int, slice_C: int):
    assert v.buf.dtype == torch.int32 and v.buf.is_contiguous() and v.C == n_slice * slice_C, (v.C, n_slice, slice_C)
    return v.ptr, v.ld


def rank_gather(perm: torch.Tensor, n_slice: int, a: "IView", out_a: torch.Tensor, b: Optional["IView"] = None,
                out_b: Optional[torch.Tensor] = None):
    """out[b, j, r] = view[b, y, x, j * C + c] for the element perm[b, j, r] = c * H * W + y * W + x: one or two int32 views
    (symbols and table indexes) into rank order in one launch."""
    B, H, W = a.buf.shape[:3]
    slice_C = a.C // n_slice
    n = H * W * slice_C
    for o in (out_a, out_b):
        assert o is None or (o.dtype == torch.int32 and o.is_contiguous() and o.numel() == B * n_slice * n)
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == B * n_slice * n
    assert (b is None) == (out_b is None) and (b is None or tuple(b.buf.shape[:3]) == (B, H, W))
    pa, la = _rank_view(a, n_slice, slice_C)
    pb, lb = _rank_view(b, n_slice, slice_C) if b is not None else (None, 0)
    L.check(L.load().vam_rank_gather(pa, la, pb, lb, perm.data_ptr(), B, n_slice, H * W, slice_C, out_a.data_ptr(),
                                     out_b.data_ptr() if out_b is not None else None, stream_ptr()), "vam_rank_gather")


def rank_counts(layer: torch.Tensor, perm: torch.Tensor, n_slice: int, n_levels: int, count: torch.Tensor):
    """count int32 [n_levels, B, n_slice] = #(layer id <= g) per segment, for the uint8 ids of :func:`variance_layers`
    ([B, H, W, n_slice * C]): how long a prefix of the rank order quality g keeps."""
    B, H, W, Ct = layer.shape
    assert layer.dtype == torch.uint8 and layer.is_contiguous() and Ct % n_slice == 0
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == B * H * W * Ct
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() >= n_levels * B * n_slice
    L.check(L.load().vam_rank_counts(layer.data_ptr(), Ct, perm.data_ptr(), B, n_slice, H * W, Ct // n_slice, n_levels,
                                     count.data_ptr(), stream_ptr()), "vam_rank_counts")


def rank_scatter(ranked: torch.Tensor, perm: torch.Tensor, count: torch.Tensor, n_levels: int, n_slice: int, sym: "IView",
                 level_id: torch.Tensor):
    """The inverse of :func:`rank_gather` for a decoder: ``sym`` gets ranked[r] at the element perm[r] where
    r < count[n_levels - 1] (0 elsewhere), ``level_id`` uint8 [B, H, W, n_slice * C] the smallest g with r < count[g]
    (L.LAYER_NONE if none).  ``count`` int32 [n_levels, B, n_slice] on the device, non-decreasing in g."""
    B, H, W = sym.buf.shape[:3]
    slice_C = sym.C // n_slice
    n = H * W * slice_C
    ps, ls = _rank_view(sym, n_slice, slice_C)
    assert ranked.dtype == torch.int32 and ranked.is_contiguous() and ranked.numel() == B * n_slice * n
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == B * n_slice * n
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == n_levels * B * n_slice and count.is_cuda
    assert level_id.dtype == torch.uint8 and level_id.is_contiguous() and tuple(level_id.shape) == (B, H, W, sym.C)
    L.check(L.load().vam_rank_scatter(ranked.data_ptr(), perm.data_ptr(), count.data_ptr(), n_levels, B, n_slice, H * W, slice_C,
                                      ps, ls, level_id.data_ptr(), sym.C, stream_ptr()), "vam_rank_scatter")


# ------------------------------------------------------------- pooled selection (picture-wide marks)
def _pool_keys_shape(keys: torch.Tensor):
    assert keys.dtype == torch.int32 and keys.is_contiguous() and keys.dim() == 3 and keys.is_cuda, (keys.dtype, tuple(keys.shape))
    return tuple(int(v) for v in keys.shape)


def pool_keys(sigma: View, perm: torch.Tensor, keys: torch.Tensor, t0: int = 0, n_slice: int = 1):
    """Rows ``[t0, t0 + sigma.B)`` of ``keys`` (the bits of uint32 in an int32 tensor [T, n_slice, n]) get every (tile, slice)
    segment of ``sigma`` in the rank order ``perm`` (:func:`variance_rank` on the same view) as order-preserving keys that
    ascend as sigma descends; -0.0 == +0.0 and every NaN is the key 0xFFFFFFFF, last.  One launch; capturable."""
    T, ns, n = _pool_keys_shape(keys)
    slice_C = sigma.C // n_slice
    hw = sigma.H * sigma.W
    assert slice_C * n_slice == sigma.C and ns == n_slice and n == hw * slice_C, (sigma.C, n_slice, ns, n, hw)
    assert 0 <= t0 and t0 + sigma.B <= T, (t0, sigma.B, T)
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == sigma.B * n_slice * n
    assert keys.device == sigma.buf.device == perm.device
    L.check(L.load().vam_pool_keys(sigma.ptr, sigma.ld, hw * sigma.ld, slice_C, perm.data_ptr(), sigma.B, n_slice, hw, slice_C,
                                   keys.data_ptr(), int(t0), T, stream_ptr()), "vam_pool_keys")


def pooled_select(keys: torch.Tensor, prs: Sequence[float], thr: torch.Tensor):
    """``thr`` fp32 [len(prs), n_slice] gets, per slice j, ``torch.quantile(pool_j, float32(1 - 0.1 q))`` of the pool of all
    T * n sigmas behind ``keys[:, j]`` (:func:`pool_keys`; every row sorted) for the non-decreasing qualities ``prs`` > 0 (up
    to L.VAM_MAX_LAYER_LEVELS), bit for bit; -inf for q >= 10, NaN when the pool holds one.  One launch; capturable."""
    T, ns, n = _pool_keys_shape(keys)
    prs = [float(p_) for p_ in prs]
    assert thr.dtype == torch.float32 and thr.is_contiguous() and tuple(thr.shape) == (len(prs), ns) and thr.device == keys.device
    arr = (C.c_double * max(len(prs), 1))(*prs)
    L.check(L.load().vam_pooled_select(keys.data_ptr(), T, ns, n, arr, len(prs), thr.data_ptr(), stream_ptr()), "vam_pooled_select")


def threshold_counts(keys: torch.Tensor, thr: torch.Tensor, count: torch.Tensor):
    """``count`` int32 [L, T, n_slice] = how many keys of row (t, j) of ``keys`` hold a sigma >= ``thr[k, j]`` (fp32
    [L, n_slice] on the device), compared as floats; a threshold of -inf counts the whole row.  One launch; capturable."""
    T, ns, n = _pool_keys_shape(keys)
    assert thr.dtype == torch.float32 and thr.is_contiguous() and thr.dim() == 2 and thr.shape[1] == ns and thr.device == keys.device
    nl = int(thr.shape[0])
    assert count.dtype == torch.int32 and count.is_contiguous() and tuple(count.shape) == (nl, T, ns) and count.device == keys.device
    L.check(L.load().vam_threshold_counts(keys.data_ptr(), T, ns, n, thr.data_ptr(), nl, count.data_ptr(), stream_ptr()),
            "vam_threshold_counts")


def tile_extract(image: torch.Tensor, coords: torch.Tensor, out: torch.Tensor, overlap: int):
    """out[i, :, y, x] = image[:, min(r * Sy + y, H - 1), min(c * Sx + x, W - 1)] for (r, c) = coords[i]: the tiles of a
    picture ``image`` fp32 [3, H, W], edge replicated, ``coords`` int32 [n, 2] on the device, ``out`` fp32
    [n, 3, th, tw], strides Sy = th - overlap and Sx = tw - overlap.  One launch; capturable."""
    assert image.dtype == torch.float32 and image.is_contiguous() and image.dim() == 3 and image.shape[0] == 3 and image.is_cuda
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[1] == 3 and out.device == image.device
    n, _, th, tw = out.shape
    assert coords.dtype == torch.int32 and coords.is_contiguous() and tuple(coords.shape) == (n, 2) and coords.device == image.device
    L.check(L.load().vam_tile_extract(image.data_ptr(), image.shape[1], image.shape[2], th, tw, int(overlap), coords.data_ptr(), n,
                                      out.data_ptr(), stream_ptr()), "vam_tile_extract")


def tile_schedule(maps: torch.Tensor, coords: torch.Tensor, out: torch.Tensor, th: int, tw: int, overlap: int):
    """out[i, k, a, b] = the maximum over the 16 x 16 pixels of latent cell (a, b) of tile (r, c) = coords[i] of
    ``maps[k, min(r * Sy + y, H - 1), min(c * Sx + x, W - 1)]``: a picture-wide schedule ``maps`` fp32 [L, H, W] at pixel
    resolution brought down onto the tiles' latent grids, the block maximum of
    evaluate.latent_quality_map over :func:`tile_extract`'s replicated edge; a NaN in a block gives NaN.  ``coords`` int32
    [n, 2] on the device, ``out`` fp32 [n, L, th / 16, tw / 16].  One launch; capturable."""
    assert maps.dtype == torch.float32 and maps.is_contiguous() and maps.dim() == 3 and maps.is_cuda
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.device == maps.device
    n, nl = int(out.shape[0]), int(maps.shape[0])
    assert tuple(out.shape) == (n, nl, th // 16, tw // 16), (tuple(out.shape), (n, nl, th // 16, tw // 16))
    assert coords.dtype == torch.int32 and coords.is_contiguous() and tuple(coords.shape) == (n, 2) and coords.device == maps.device
    L.check(L.load().vam_tile_schedule(maps.data_ptr(), nl, maps.shape[1], maps.shape[2], int(th), int(tw), int(overlap),
                                       coords.data_ptr(), n, out.data_ptr(), stream_ptr()), "vam_tile_schedule")


def _check_tiles(tiles, slot, w_lo, w_hi, H, W, overlap, hw, out, status, device=None):
    """The asserts that :func:`tile_blend`, :func:`tile_refresh` and :func:`tile_compose` share: ``tiles``, ``slot`` (against
    the grid the library derives), the ramps and ``status`` (all on ``device``, by default wherever ``tiles`` lies) and ``out``,
    which holds a window of ``hw`` = (h, w).  ``tiles`` None (compose without tiles): ``out`` alone.  Returns (n, th, tw)."""
    n = th = tw = 0
    if tiles is not None:
        assert tiles.dtype == torch.float32 and tiles.is_contiguous() and tiles.dim() == 4 and tiles.shape[1] == 3
        assert tiles.is_cuda if device is None else tiles.device == device
        device = tiles.device
        n, _, th, tw = tiles.shape
        assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.dim() == 2 and slot.device == device
        if H >= 1 and W >= 1 and 0 <= 2 * overlap <= min(th, tw):   # the grid the library derives; anything else it refuses
            grid = tuple(max(1, -(-(n_ - overlap) // (t_ - overlap))) for n_, t_ in ((H, th), (W, tw)))
            assert tuple(slot.shape) == grid, (tuple(slot.shape), grid)
        for t in (w_lo, w_hi):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == overlap and t.device == device)
        assert status is not None and status.dtype == torch.int32 and status.numel() == 1 and status.device == device
    assert out.is_contiguous() and out.device == device
    assert (out.dtype == torch.float32 and tuple(out.shape) == (3,) + hw) or (out.dtype == torch.uint8 and tuple(out.shape) == hw + (3,)), \
        (out.dtype, tuple(out.shape), hw)
    return n, th, tw


def tile_blend(tiles: torch.Tensor, slot: torch.Tensor, w_lo: Optional[torch.Tensor], w_hi: Optional[torch.Tensor], H: int, W: int,
               overlap: int, window: Sequence[int], out: torch.Tensor, status: torch.Tensor):
    """The window (y0, x0, h, w) of a picture of H x W blended from decoded tiles: ``tiles`` fp32
    [n, 3, th, tw], ``slot`` int32 [R, C] (index into ``tiles``, -1: absent), the ramps ``w_lo`` / ``w_hi`` fp32 [overlap]
    (None for overlap 0).  ``out``: fp32 [3, h, w], or uint8 [h, w, 3] as rint(clamp(v, 0, 1) * 255).  ``status`` int32 [1],
    cleared by the caller, becomes 1 when a pixel needs an absent tile.  One launch; capturable."""
    y0, x0, h, w = (int(v) for v in window)
    n, th, tw = _check_tiles(tiles, slot, w_lo, w_hi, H, W, overlap, (h, w), out, status)
    rc = L.load().vam_tile_blend(tiles.data_ptr(), n, slot.data_ptr(), w_lo.data_ptr() if w_lo is not None else None,
                                 w_hi.data_ptr() if w_hi is not None else None, int(H), int(W), th, tw, int(overlap), y0, x0, h, w,
                                 out.data_ptr(), int(out.dtype == torch.uint8), status.data_ptr(), stream_ptr())
    L.check(rc, "vam_tile_blend")


def tile_refresh(tiles: torch.Tensor, slot: torch.Tensor, dirty: torch.Tensor, w_lo: Optional[torch.Tensor], w_hi: Optional[torch.Tensor],
                 H: int, W: int, overlap: int, window: Sequence[int], box: Sequence[int], out: torch.Tensor, status: torch.Tensor):
    """:func:`tile_blend` restricted to what changed: ``out`` is a persistent canvas of ``window`` =
    (cy0, cx0, ch, cw), fp32 [3, ch, cw] or uint8 [ch, cw, 3]; ``dirty`` int32 [R, C] marks tiles, ``box`` = (y0, x0, h, w) in
    picture coordinates is the part of the window to visit.  A pixel of the box with a dirty tile gets tile_blend's value, bit
    for bit (all its tiles must be present, else ``status`` becomes 1); any other pixel is not written, and the slots of its
    tiles are not read.  One launch; capturable."""
    cy0, cx0, ch, cw = (int(v) for v in window)
    y0, x0, h, w = (int(v) for v in box)
    n, th, tw = _check_tiles(tiles, slot, w_lo, w_hi, H, W, overlap, (ch, cw), out, status)
    assert dirty.dtype == torch.int32 and dirty.is_contiguous() and dirty.shape == slot.shape and dirty.device == tiles.device
    rc = L.load().vam_tile_refresh(tiles.data_ptr(), n, slot.data_ptr(), dirty.data_ptr(), w_lo.data_ptr() if w_lo is not None else None,
                                   w_hi.data_ptr() if w_hi is not None else None, int(H), int(W), th, tw, int(overlap), cy0, cx0, ch, cw,
                                   y0, x0, h, w, out.data_ptr(), int(out.dtype == torch.uint8), status.data_ptr(), stream_ptr())
    L.check(rc, "vam_tile_refresh")


def tile_compose(tiles: Optional[torch.Tensor], slot: Optional[torch.Tensor], w_lo: Optional[torch.Tensor], w_hi: Optional[torch.Tensor],
                 H: int, W: int, overlap: int, window: Sequence[int], below: torch.Tensor, below_window: Sequence[int], shift: int,
                 out: torch.Tensor, status: Optional[torch.Tensor]):
    """:func:`tile_blend` of a window of a pyramid level whose tiles have not all arrived: a tile is
    available when its ``slot`` is >= 0; a pixel all of whose tiles are available gets tile_blend's value, bit for bit; any
    other pixel reads none of its tiles and is the bilinear upsample by 2^``shift`` (1 .. 15) of ``below``, fp32 [3, hb, wb]:
    the window ``below_window`` = (by0, bx0, hb, wb) of the level ``shift`` levels coarser, ceil(H / 2^shift) x
    ceil(W / 2^shift), which must cover ``pyramid.source_window(window, shift, ...)``.  ``tiles`` and ``slot`` None: no tiles,
    every pixel comes from ``below`` (``overlap``, the ramps and ``status`` are then ignored).  One launch; capturable."""
    y0, x0, h, w = (int(v) for v in window)
    by0, bx0, hb, wb = (int(v) for v in below_window)
    d = int(shift)
    assert below.dtype == torch.float32 and below.is_contiguous() and tuple(below.shape) == (3, hb, wb) and below.is_cuda, \
        (below.dtype, tuple(below.shape), (hb, wb))
    assert (tiles is None) == (slot is None)
    n, th, tw = _check_tiles(tiles, slot, w_lo, w_hi, H, W, overlap, (h, w), out, status, below.device)
    Hj, Wj = (-(-int(v) // (1 << d)) for v in (H, W)) if 1 <= d <= 15 else (0, 0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = L.load().vam_tile_compose(ptr(tiles), n, ptr(slot), ptr(w_lo), ptr(w_hi), int(H), int(W), th, tw, int(overlap), y0, x0, h, w,
                                   below.data_ptr(), by0, bx0, hb, wb, Hj, Wj, d, out.data_ptr(), int(out.dtype == torch.uint8),
                                   ptr(status), stream_ptr())
    L.check(rc, "vam_tile_compose")


HALVE_MODES = ("mean", "max")


def picture_halve(src: torch.Tensor, mode: str = "mean", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The next level of a resolution pyramid: ``src`` fp32 [C, Hs, Ws], contiguous, 1 <= C <= 32, to fp32
    [C, ceil(Hs / 2), ceil(Ws / 2)].  ``mode`` = "mean": ``((s[2y][2x] + s[2y][x1]) + (s[y1][2x] + s[y1][x1])) * 0.25`` with
    ``y1 = min(2y + 1, Hs - 1)``, ``x1 = min(2x + 1, Ws - 1)``, every operation one fp32 operation in this order; "max": the
    maximum of the four (schedules), a NaN among them giving NaN.  ``out``: where to write it (allocated when None).  One
    launch (vam_picture_halve); capturable when ``out`` is given."""
    if mode not in HALVE_MODES:
        raise ValueError(f"picture_halve: mode is one of {HALVE_MODES}, got {mode!r}")
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3 and src.is_cuda
    C_, Hs, Ws = (int(v) for v in src.shape)
    shape = (C_, (Hs + 1) // 2, (Ws + 1) // 2)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape and out.device == src.device, \
        (out.dtype, tuple(out.shape), shape)
    L.check(L.load().vam_picture_halve(src.data_ptr(), C_, Hs, Ws, out.data_ptr(), HALVE_MODES.index(mode), stream_ptr()),
            "vam_picture_halve")
    return out


def picture_resample(src: torch.Tensor, src_window: Sequence[int], level_hw: Sequence[int], shift: int, rect: Sequence[int], unit: int,
                     out_hw: Sequence[int], out: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """A viewport of a picture at any zoom and pan: the rect (y0, x0, h, w) / ``unit`` of the picture, in
    level-0 pixels divided by the integer ``unit`` (1 .. 256), resampled from pyramid level ``shift`` (0 .. 15) into ``out_hw``
    = (oh, ow) pixels with a tent of half-width max(1, scale) level pixels, scale = h / (oh unit 2^shift) at most 16.  ``src``
    fp32 [C, hs, ws], contiguous, 1 <= C <= 32, is the window ``src_window`` = (sy0, sx0, hs, ws) of the level's picture of
    ``level_hw`` = (Hk, Wk) and must cover ``pyramid.viewport_window(rect, out_hw, shift, ...)``.  Taps and weights are exact
    integer arithmetic in the kernel (``pyramid.viewport_taps`` restates them); the value is the sum over the row taps of
    wy * (the sum over the column taps of wx * s), ascending, every operation one fp32 operation.  ``out``: fp32 [C, oh, ow] or,
    for C = 3, uint8 [oh, ow, 3] as rint(clamp(v, 0, 1) * 255); allocated in ``dtype`` (torch.float32 when None) when None.
    One launch (vam_picture_resample), no table is uploaded; capturable when ``out`` is given."""
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3 and src.is_cuda
    sy0, sx0, hs, ws = (int(v) for v in src_window)
    assert tuple(src.shape[1:]) == (hs, ws), (tuple(src.shape), (hs, ws))
    Hk, Wk = (int(v) for v in level_hw)
    y0, x0, h, w = (int(v) for v in rect)
    oh, ow = (int(v) for v in out_hw)
    C_ = int(src.shape[0])
    if out is None:
        if dtype not in (None, torch.float32, torch.uint8):
            raise ValueError(f"picture_resample: dtype is torch.float32 or torch.uint8, got {dtype}")
        if not (1 <= oh <= 65536 and 1 <= ow <= 65536):
            raise ValueError(f"picture_resample: an output of {oh} x {ow}: sides are 1 .. 65536")
        out = torch.empty((oh, ow, C_), dtype=torch.uint8, device=src.device) if dtype == torch.uint8 \
            else torch.empty((C_, oh, ow), dtype=torch.float32, device=src.device)
    assert out.is_contiguous() and out.device == src.device
    assert (out.dtype == torch.float32 and tuple(out.shape) == (C_, oh, ow)) or (out.dtype == torch.uint8 and tuple(out.shape) == (oh, ow, C_)), \
        (out.dtype, tuple(out.shape), (C_, oh, ow))
    within = lambda v: v if -2 ** 63 <= v < 2 ** 63 else -1                    # what no int64 holds is outside every picture
    L.check(L.load().vam_picture_resample(src.data_ptr(), C_, sy0, sx0, hs, ws, Hk, Wk, int(shift), within(y0), within(x0), within(h),
                                          within(w), int(unit), oh, ow, out.data_ptr(), int(out.dtype == torch.uint8), stream_ptr()),
            "vam_picture_resample")
    return out


@dataclass
class IView:
    """int32 NHWC channel window (symbols / table indexes)."""
    buf: torch.Tensor   # [B,H,W,ld] int32
    c0: int
    C: int

    @property
    def ptr(self): return self.buf.data_ptr() + 4 * self.c0
    @property
    def ld(self): return self.buf.shape[3]

    def window(self, c0, C_): return IView(self.buf, self.c0 + c0, C_)


def new_iview(B, H, W, C_, device="cuda") -> IView:
    return IView(torch.empty((B, H, W, C_), dtype=torch.int32, device=device), 0, C_)


def _win(v):
    """(ptr, pixel stride) of a window, or (None, 0) for an absent one."""
    return (v.ptr, v.ld) if v is not None else (None, 0)


def _levels_win(v, n: int, ref: View, ls: Optional[int] = None):
    """(ptr, pixel stride, level stride in elements) of a per-level operand of ``n`` levels over ``ref``'s window, or
    (None, 0, 0): by default the levels are consecutive blocks of ``ref.B`` images of ``v``'s buffer; with ``ls`` they are
    windows of one [B, ...] buffer ``ls`` elements apart."""
    if v is None:
        return None, 0, 0
    nb, ld = v.buf.shape[0], v.buf.shape[3]
    assert v.C == ref.C and tuple(v.buf.shape[1:3]) == (ref.H, ref.W), (v.C, ref.C, tuple(v.buf.shape))
    if ls is None:
        assert nb == n * ref.B, (nb, n, ref.B)
        ls = ref.B * ref.H * ref.W * ld
    else:
        assert nb == ref.B
    return v.ptr, ld, ls


def gauss_tail(y: View, mu: View, sigma: View, *, y2: Optional[View] = None, mask: Optional[View] = None,
               yhat: Optional[View] = None, lik: Optional[View] = None, sym=None,
               log2sum: Optional[torch.Tensor] = None):
    n_pix = y.n_pix
    if sym is None:
        sym_ptr, sym_ld = None, 0
    elif isinstance(sym, IView):
        sym_ptr, sym_ld = sym.ptr, sym.ld
    else:
        sym_ptr, sym_ld = sym.data_ptr(), sym.shape[-1]
    L.check(L.load().vam_gauss_tail(*_win(y), *_win(y2), *_win(mu), *_win(sigma), *_win(mask), *_win(yhat), *_win(lik), sym_ptr, sym_ld,
                                    log2sum.data_ptr() if log2sum is not None else None, y.H * y.W, n_pix, y.C,
                                    stream_ptr()), "vam_gauss_tail")


def gauss_levels_eval(y: View, mu: View, sigma: View, mask: View, n_levels: int, *, y2: Optional[View] = None,
                      yhat: Optional[View] = None, lik: Optional[View] = None, sym: Optional[IView] = None,
                      log2sum: Optional[torch.Tensor] = None):
    """Evaluation tail of ``n_levels`` masks over one (y, y2, mu, sigma) window (rate sweep): per level the masked branch
    of :func:`gauss_tail`, bit for bit.  ``mask`` / ``yhat`` / ``lik`` / ``sym`` hold the levels as consecutive image
    blocks ([L * B, H, W, ld], level l = images l*B ..); ``log2sum`` [L, B] float64 receives level l's per-image sums."""
    B = y.B
    assert log2sum is None or (log2sum.dtype == torch.float64 and log2sum.is_contiguous() and log2sum.numel() == n_levels * B)
    L.check(L.load().vam_gauss_levels_eval(*_win(y), *_win(y2), *_win(mu), *_win(sigma), *_levels_win(mask, n_levels, y), *_levels_win(yhat, n_levels, y),
                                           *_levels_win(lik, n_levels, y), *_levels_win(sym, n_levels, y),
                                           log2sum.data_ptr() if log2sum is not None else None, y.H * y.W, n_levels,
                                           y.n_pix, y.C, stream_ptr()), "vam_gauss_levels_eval")


def gauss_levels_decode(sym: "IView", layer: torch.Tensor, mu: View, ks: Sequence[int], yhat: View):
    """Decoder side of :func:`gauss_levels_eval`: level l's quantised latents float(sym) * (layer <= ks[l]) + mu, written as
    ``yhat``'s consecutive image blocks ([L * B, H, W, ld], level l = images l*B ..).  ``layer`` uint8 [B, H, W, mu.C]."""
    B, nl = mu.B, len(ks)
    assert yhat.buf.shape[0] == nl * B and tuple(yhat.buf.shape[1:3]) == (mu.H, mu.W) and yhat.C == mu.C == sym.C
    assert layer.dtype == torch.uint8 and layer.is_contiguous() and tuple(layer.shape) == (B, mu.H, mu.W, mu.C)
    arr = (C.c_int * max(nl, 1))(*[int(k) for k in ks])
    L.check(L.load().vam_gauss_levels_decode(sym.ptr, sym.ld, layer.data_ptr(), mu.C, mu.ptr, mu.ld, arr, nl, yhat.ptr, yhat.ld,
                                             B * mu.H * mu.W * yhat.ld, mu.n_pix, mu.C, stream_ptr()), "vam_gauss_levels_decode")


def gauss_layer_bits(y: View, mu: View, sigma: View, layer: torch.Tensor, n_levels: int, bits: torch.Tensor,
                     count: torch.Tensor, *, y2: Optional[View] = None, ld_layer: Optional[int] = None,
                     pix_per_item: Optional[int] = None):
    """Rate-only tail (rate control): per image the fp64 sum of log2 of the IN-mask likelihood — the float
    :func:`gauss_levels_eval` gets for an element inside a mask — and the element count, binned by the layer ids of
    :func:`variance_layers`: ``bits`` float64 / ``count`` int64 [B, n_levels + 1], slot ``n_levels`` for L.LAYER_NONE.
    Both accumulate: clear them first (:func:`memset_zero`); one image may use the head of a longer row.  ``layer`` uint8 with pixel stride ``ld_layer`` (default:
    contiguous [B, H, W, y.C]).  ``pix_per_item`` (default: a whole image): the bins are kept per ``pix_per_item``
    consecutive pixels instead, [B * H * W / pix_per_item, n_levels + 1] (1: per latent pixel, the quality-map rate)."""
    B = y.B
    if pix_per_item is not None and pix_per_item != y.H * y.W:
        assert pix_per_item >= 1 and y.n_pix % pix_per_item == 0, (pix_per_item, y.n_pix)
        B = y.n_pix // pix_per_item                                  # items
    pix_per_item = y.H * y.W if pix_per_item is None else pix_per_item
    if ld_layer is None:
        assert layer.is_contiguous() and tuple(layer.shape) == (y.B, y.H, y.W, y.C)
        ld_layer = y.C
    assert layer.dtype == torch.uint8 and mu.C == sigma.C == y.C and (y2 is None or y2.C == y.C)
    for t, dt in ((bits, torch.float64), (count, torch.int64)):
        assert t.dtype == dt and t.is_contiguous(), (t.dtype, tuple(t.shape))
        assert t.numel() == B * (n_levels + 1) or (B == 1 and t.numel() > n_levels), (tuple(t.shape), B, n_levels)
    L.check(L.load().vam_gauss_layer_bits(*_win(y), *_win(y2), *_win(mu), *_win(sigma), layer.data_ptr(), ld_layer, n_levels,
                                          bits.data_ptr(), count.data_ptr(), pix_per_item, y.n_pix, y.C, stream_ptr()),
            "vam_gauss_layer_bits")


_LOG2_LIK_OUTSIDE: dict = {}


def log2_lik_outside(device) -> float:
    """log2 L(0, 0): what an element outside the variance mask contributes to the log2-likelihood sum at every quality
    (masked_tail with m = 0 gives |v| = 0 and sigma = 0; the 0.11 bound applies).  Taken once per process and device from
    :func:`gauss_layer_bits` itself on one such element, so it is the device's own double."""
    device = torch.device(device)
    key = (device.type, device.index)
    if key not in _LOG2_LIK_OUTSIDE:
        z = new_view(1, 1, 1, 4, device, zero=True)
        layer = torch.tensor([0, L.LAYER_NONE, L.LAYER_NONE, L.LAYER_NONE], dtype=torch.uint8, device=device).view(1, 1, 1, 4)
        bits = torch.zeros((1, 2), dtype=torch.float64, device=device)
        count = torch.zeros((1, 2), dtype=torch.int64, device=device)
        gauss_layer_bits(z, z, z, layer, 1, bits, count)
        assert count.tolist() == [[1, 3]]
        _LOG2_LIK_OUTSIDE[key] = float(bits[0, 0])
    return _LOG2_LIK_OUTSIDE[key]


def _coded_bins(bits: torch.Tensor, count: torch.Tensor, n_streams: int, n_levels: int):
    for t, dt in ((bits, torch.float64), (count, torch.int64)):
        assert t.dtype == dt and t.is_contiguous() and t.numel() == n_streams * (n_levels + 1), (t.dtype, tuple(t.shape), n_streams, n_levels)


def coded_layer_bits(y: View, mu: View, sigma: View, layer: Optional[torch.Tensor], n_levels: int, scale_table: torch.Tensor,
                     tables, chans_per_stream: int, bits: torch.Tensor, count: torch.Tensor, *, y2: Optional[View] = None):
    """Coded-size tail: per stream (image, slice of ``chans_per_stream`` channels) the exact price in bits
    the range coder charges for the pair (round(r - mu), build_indexes(sigma)) of every element, and the element count,
    binned by the layer ids of :func:`variance_layers` (``layer`` None: all in layer 0): ``bits`` float64 / ``count`` int64
    [B, y.C // chans_per_stream, n_levels + 1], slot ``n_levels`` for L.LAYER_NONE.  Both accumulate: clear them first.
    ``tables``: a bitstream.DeviceTables of the gaussian conditional."""
    B = y.B
    assert mu.C == sigma.C == y.C and (y2 is None or y2.C == y.C)
    assert layer is None or (layer.dtype == torch.uint8 and layer.is_contiguous() and tuple(layer.shape) == (B, y.H, y.W, y.C))
    assert scale_table.dtype == torch.float32 and scale_table.is_contiguous() and scale_table.device == y.buf.device
    _coded_bins(bits, count, B * (y.C // max(chans_per_stream, 1)), n_levels)
    L.check(L.load().vam_coded_layer_bits(*_win(y), *_win(y2), *_win(mu), *_win(sigma), layer.data_ptr() if layer is not None else None, y.C,
                                          n_levels, scale_table.data_ptr(), scale_table.numel(), C.byref(tables.struct),
                                          chans_per_stream, bits.data_ptr(), count.data_ptr(), y.H * y.W, y.n_pix, y.C,
                                          stream_ptr()), "vam_coded_layer_bits")


def coded_symbol_bits(sym: IView, idx: Optional[IView], layer: Optional[torch.Tensor], n_levels: int, tables,
                      chans_per_stream: int, bits: torch.Tensor, count: torch.Tensor, *, idx_base: int = 0):
    """The symbol-input form of :func:`coded_layer_bits`: int32 symbols with int32 table indexes (``idx`` None: index =
    ``idx_base`` + channel, the entropy bottleneck's per-channel tables)."""
    B, H, W = sym.buf.shape[:3]
    assert idx is None or (idx.C == sym.C and tuple(idx.buf.shape[:3]) == (B, H, W))
    assert layer is None or (layer.dtype == torch.uint8 and layer.is_contiguous() and tuple(layer.shape) == (B, H, W, sym.C))
    _coded_bins(bits, count, B * (sym.C // max(chans_per_stream, 1)), n_levels)
    L.check(L.load().vam_coded_symbol_bits(sym.ptr, sym.ld, idx.ptr if idx is not None else None, idx.ld if idx is not None else 0,
                                           idx_base, layer.data_ptr() if layer is not None else None, sym.C, n_levels,
                                           C.byref(tables.struct), chans_per_stream, bits.data_ptr(), count.data_ptr(), H * W,
                                           B * H * W, sym.C, stream_ptr()), "vam_coded_symbol_bits")


def build_indexes(sigma: View, table: torch.Tensor, mask: Optional[View] = None, out: Optional[IView] = None) -> torch.Tensor:
    if out is None:
        out = new_iview(sigma.B, sigma.H, sigma.W, sigma.C, sigma.buf.device)
    L.check(L.load().vam_build_indexes(sigma.ptr, sigma.ld, mask.ptr if mask is not None else None,
                                       mask.ld if mask is not None else 0, table.data_ptr(), table.numel(),
                                       out.ptr, out.ld, sigma.n_pix, sigma.C, stream_ptr()), "vam_build_indexes")
    return out.buf


def dequantize(sym: IView, mu: Optional[View], out: View):
    L.check(L.load().vam_dequantize(sym.ptr, sym.ld, mu.ptr if mu is not None else None, mu.ld if mu is not None else 0,
                                    out.ptr, out.ld, out.n_pix, out.C, stream_ptr()), "vam_dequantize")


def eb_forward(z: View, params: torch.Tensor, zhat: Optional[View], lik: Optional[View],
               log2sum: Optional[torch.Tensor] = None, sym: Optional[IView] = None, noise: Optional[View] = None):
    L.check(L.load().vam_eb_forward_noise(z.ptr, z.ld, params.data_ptr(), z.C, *_win(zhat), *_win(lik), *_win(sym),
                                          log2sum.data_ptr() if log2sum is not None else None, z.H * z.W, z.n_pix,
                                          *_win(noise), stream_ptr()), "vam_eb_forward")


def add(a: View, b: View, out: View):
    L.check(L.load().vam_add(a.ptr, a.ld, b.ptr, b.ld, out.ptr, out.ld, a.n_pix, a.C, stream_ptr()), "vam_add")


# ---- REM fine-tune backward pieces (csrc/train.hip, csrc/elementwise.hip, csrc/entropy.hip)
def pack_conv_dgrad(weight: torch.Tensor) -> Packed:
    """Weights of the data-gradient conv of a stride-1 ``nn.Conv2d`` (taps flipped, channel roles swapped)."""
    n_out, c_in, kh, kw = weight.shape
    w = pack_weights(weight, L.PACK_CONV_DGRAD, 0, kh, kw, n_out, c_in)
    return Packed(w, None, kh, kw, n_out, c_in, 1, kh // 2, kw // 2)


def wgrad_problems(x_segs: Sequence[View], dy: View, dw: torch.Tensor, db: Optional[torch.Tensor],
                   stride: int = 1) -> List[L.VamWgrad]:
    """dw (OIHW) / db of a conv (stride 1 pad k/2, or the k5/s2/p2 one) whose input was the channel concat of
    ``x_segs``: one problem per segment.  dw may be a 2-D [N, C] tensor (a 1x1 layer / nn.Linear)."""
    if dw.dim() == 2:
        n, cin_total, kh, kw = dw.shape[0], dw.shape[1], 1, 1
    else:
        n, cin_total, kh, kw = dw.shape
    assert dy.C == n and sum(v.C for v in x_segs) == cin_total and dw.is_contiguous() and kh == kw
    out, off = [], 0
    for v in x_segs:
        assert v.B == dy.B and (v.H, v.W) == (stride * dy.H, stride * dy.W)
        p = L.VamWgrad()
        p.x, p.dy, p.dw = v.ptr, dy.ptr, dw.data_ptr()
        p.db = db.data_ptr() if (db is not None and off == 0) else None
        p.ld_x, p.ld_dy, p.B, p.H, p.W, p.kh, p.kw, p.C, p.N = v.ld, dy.ld, dy.B, dy.H, dy.W, kh, kw, v.C, n
        if isinstance(v, View3):          # taped activation stored as bf16x3 planes: the LDS-tiled kernel copies instead of splitting
            assert kh == 3 and stride == 1 and wgrad_reads_planes(dy.H, dy.W), "plane inputs: k3 stride-1 layers on an LDS-kernel grid"
            p.flags = L.WGRAD_X_P3
        p.cin_total, p.c_off = cin_total, off
        p.stride, p.Hx, p.Wx = stride, v.H, v.W
        p._dev = dy.buf.device
        p._keep = (v, dy, dw, db)         # the struct holds raw pointers: the tensors live at least as long as it does
        out.append(p)
        off += v.C
    wgrad_plan(out)                       # alone; a grouped launch re-plans with each problem's share of the group
    return out


def wgrad_reads_planes(H: int, W: int) -> bool:
    """True when the weight gradient of a k3 stride-1 layer on an H x W grid takes the LDS-tiled kernel, which can read its
    input as bf16x3 planes (``View3``)."""
    return split_mode() and bool(L.load().vam_conv_wgrad_lds_grid(int(H), int(W)))


def train_tape_planes(H: int, W: int) -> bool:
    """Policy: write the taped activations of the training slice stacks as bf16x3 planes where forward convolution and
    weight gradient can both read them.  OFF by default — built, bit-identical (tests/test_gpu_wgrad_lds.py), and measured
    no faster on the first_train step (interleaved on one box: 140.2 / 140.3 ms with, 140.1 / 139.9 without,
    profiles/r04_first_train_ab.txt: the forward gains what the 1.5x bytes of the plane stores cost the backward).
    ``VAMPIC_TRAIN_P3=1`` switches it on."""
    return os.environ.get("VAMPIC_TRAIN_P3", "0") == "1" and wgrad_reads_planes(H, W)


def wgrad_plan(problems: Sequence[L.VamWgrad]):
    """Pixel splits (vam_conv_wgrad_plan) and the caller-owned scratch of the problems of ONE launch.  A problem that
    shares the launch with others plans against its share of the chip (its fraction of the group's FLOPs)."""
    lib = L.load()
    work = [float(p.B) * p.H * p.W * p.C * p.N * p.kh * p.kw for p in problems]
    tot = sum(work) or 1.0
    # VAMPIC_WGRAD_SHARE (experiment): the fraction of the chip a weight-gradient launch is planned against.  On a branch of
    # its own (engine.Plan.wgrad_branch) a launch shares the chip with the data-gradient chain.
    chip = float(os.environ.get("VAMPIC_WGRAD_SHARE", "1.0"))
    for p, w in zip(problems, work):
        share = 1.0 if len(problems) == 1 else max(w / tot, 1e-3)
        share *= chip
        p.slot_share = 0.0 if share == 1.0 else max(share, 1e-3)
        nbytes = C.c_size_t(0)
        p.splits = lib.vam_conv_wgrad_plan(C.byref(p), C.byref(nbytes))
        if p.splits > 1:                  # caller-owned scratch for the pixel-split partial tiles; lives with the problem
            if getattr(p, "_ws", None) is None or p._ws.numel() * 4 < nbytes.value:
                p._ws = torch.empty(nbytes.value // 4, dtype=torch.float32, device=p._dev)
            p.workspace = p._ws.data_ptr()
        else:
            p._ws, p.workspace = None, None


def wgrad_group(problems: Sequence[L.VamWgrad]):
    lib = L.load()
    for i in range(0, len(problems), L.VAM_MAX_WGRAD_GROUP):
        chunk = list(problems[i:i + L.VAM_MAX_WGRAD_GROUP])
        if len(chunk) > 1:
            wgrad_plan(chunk)
        arr = (L.VamWgrad * len(chunk))(*chunk)
        L.check(lib.vam_conv_wgrad_group(arr, len(chunk), stream_ptr()), "vam_conv_wgrad_group")


def conv_wgrad(x_segs: Sequence[View], dy: View, dw: torch.Tensor, db: Optional[torch.Tensor]):
    wgrad_group(wgrad_problems(x_segs, dy, dw, db))


def leaky_bwd(act: View, dy: View, dx: View):
    L.check(L.load().vam_leaky_bwd(act.ptr, act.ld, dy.ptr, dy.ld, dx.ptr, dx.ld, dx.n_pix, dx.C, stream_ptr()), "vam_leaky_bwd")


def mul(a: View, b: View, out: View):
    L.check(L.load().vam_mul(a.ptr, a.ld, b.ptr, b.ld, out.ptr, out.ld, out.n_pix, out.C, stream_ptr()), "vam_mul")


def gauss_train(y: View, mu: View, sigma: View, noise: View, *, y2: Optional[View] = None, mask: Optional[View] = None,
                lik: Optional[View] = None, grad_lik: Optional[View] = None, dmu: Optional[View] = None,
                dsigma: Optional[View] = None):
    """Noisy-likelihood forward (``lik``) or backward (``grad_lik`` -> ``dmu``, ``dsigma``)."""
    L.check(L.load().vam_gauss_train(*_win(y), *_win(y2), *_win(mu), *_win(sigma), *_win(mask), *_win(noise), *_win(grad_lik), *_win(lik),
                                     *_win(dmu), *_win(dsigma), y.n_pix, y.C, stream_ptr()), "vam_gauss_train")



def gauss_levels_fwd(y: View, mu: View, sigma: View, mask: View, noise: View, rq: View, lik: View, n_levels: int, *,
                     y2: Optional[View] = None, noise_ls: Optional[int] = None, lik_ls: Optional[int] = None):
    """Progressive tail of ``n_levels`` quality levels over one (y, y2, mu, sigma) window (csrc/entropy.hip): per level
    rq = round(r - mu) * m + mu and the noisy likelihood.  ``mask`` / ``rq`` hold the levels as consecutive image blocks
    ([L * B, H, W, ld]); ``noise`` / ``lik`` likewise, or — with ``noise_ls`` / ``lik_ls`` — windows of one [B, ...]
    buffer whose level l starts ``l * ls`` floats further (e.g. consecutive channel blocks)."""
    L.check(L.load().vam_gauss_levels_fwd(*_win(y), *_win(y2), *_win(mu), *_win(sigma), *_levels_win(mask, n_levels, y, None),
                                          *_levels_win(noise, n_levels, y, noise_ls), *_levels_win(rq, n_levels, y, None),
                                          *_levels_win(lik, n_levels, y, lik_ls), n_levels, y.n_pix, y.C, stream_ptr()),
            "vam_gauss_levels_fwd")


def gauss_levels_bwd(y: View, mu: View, sigma: View, mask: View, noise: View, grad_lik: View, d_rq: View, gmu: View,
                     dsigma: View, dy_top: View, n_levels: int, *, y2: Optional[View] = None, dy_sub: Optional[View] = None,
                     noise_ls: Optional[int] = None, glik_ls: Optional[int] = None):
    """Backward of :func:`gauss_levels_fwd` with the straight-through rounding under each level's mask: writes
    gmu = sum_l (d_rq_l * (1 - m_l) + dmu_l) and dsigma = sum_l dsigma_l, and adds sum_l d_r_l into ``dy_top`` (and its
    negative into ``dy_sub``) in place — level by level, as the unfused launches would."""
    L.check(L.load().vam_gauss_levels_bwd(*_win(y), *_win(y2), *_win(mu), *_win(sigma), *_levels_win(mask, n_levels, y, None),
                                          *_levels_win(noise, n_levels, y, noise_ls), *_levels_win(grad_lik, n_levels, y, glik_ls),
                                          *_levels_win(d_rq, n_levels, y, None), *_win(gmu), *_win(dsigma), *_win(dy_top), *_win(dy_sub),
                                          n_levels, y.n_pix, y.C, stream_ptr()), "vam_gauss_levels_bwd")


# ---- transform backward pieces (csrc/train_gs.hip)
def ew(op: int, ins: Sequence[View], outs: Sequence[View], coef: float = 0.0, flag: int = 0):
    """One element-wise derivative kernel (enum vam_ew_op) over channel windows of equal extent."""
    e = L.VamEw()
    v0 = ins[0]
    for k, v in enumerate(ins):
        assert v.n_pix == v0.n_pix and v.C == v0.C
        e.inp[k].ptr, e.inp[k].ld = v.ptr, v.ld
    for k, v in enumerate(outs):
        assert v.n_pix == v0.n_pix and v.C == v0.C
        e.out[k].ptr, e.out[k].ld = v.ptr, v.ld
    e.n_pix, e.C, e.flag, e.coef = v0.n_pix, v0.C, int(flag), float(coef)
    L.check(L.load().vam_train_elementwise(op, C.byref(e), stream_ptr()), "vam_train_elementwise")


def stack_tail_ok(x, m4, m5, out: Optional[View], kw: dict) -> bool:
    """``out`` None = a fresh buffer.  Can the last two layers (m4: 128 -> 64 + GELU, m5: 64 -> 32) of a slice stack run as ONE launch (csrc/stack_tail.hip)?"""
    if os.environ.get("VAMPIC_STACK_TAIL", "1") != "1" or not split_mode():
        return False
    if not (isinstance(x, View3) and x.C == 128 and x.g0 == 0 and x.ld == 16 and x.W == 16 and x.H % 4 == 0):
        return False
    if (out is not None and (type(out) is not View or out.C != 32)) or any(kw.get(k) is not None for k in ("pre", "mul")) or kw.get("flags"):
        return False
    if kw.get("act", L.ACT_NONE) not in (L.ACT_NONE, L.ACT_HALF_TANH) or any(v is not None and type(v) is not View for v in (kw.get("post"), kw.get("post2"))):
        return False
    ok = lambda m, ci, co: (type(m).__name__ == "Conv2d" and m.in_channels == ci and m.out_channels == co and m.kernel_size == 3 and m.stride == 1)
    return ok(m4, 128, 64) and ok(m5, 64, 32)


def stack_tail_problem(x: "View3", pk4: Packed, pk5: Packed, out: View, act: int = L.ACT_NONE, post: Optional[View] = None,
                       post2: Optional[View] = None) -> "L.VamStackTail":
    t = L.VamStackTail()
    assert pk4.b is not None and pk5.b is not None and not pk4.w16 and not pk5.w16
    t.x, t.w4, t.b4, t.w5, t.b5, t.out = x.ptr, pk4.w.data_ptr(), pk4.b.data_ptr(), pk5.w.data_ptr(), pk5.b.data_ptr(), out.ptr
    t.B, t.H, t.W, t.x_groups, t.ld_out, t.act = x.B, x.H, x.W, x.ld, out.ld, int(act)
    for name, v in (("post", post), ("post2", post2)):
        if v is not None:
            assert v.n_pix == out.n_pix and v.C == out.C
            a = getattr(t, name)
            a.ptr, a.ld = v.ptr, v.ld
    t._keep = (x, pk4, pk5, out, post, post2)
    return t


def stack_tail_group(problems: Sequence["L.VamStackTail"]):
    arr = (L.VamStackTail * len(problems))(*problems)
    L.check(L.load().vam_stack_tail_group(arr, len(problems), stream_ptr()), "vam_stack_tail_group")


def axpy_jobs(updates: Sequence[tuple]):
    """Pre-marshalled jobs of :func:`axpy_group`: updates = [(dst, src, coef)] means dst += coef * src on channel windows of
    equal extent.  Returns the ctypes array (keep it alive as long as a plan step refers to it)."""
    assert 1 <= len(updates) <= L.VAM_MAX_EW_GROUP
    arr = (L.VamEw * len(updates))()
    for e, (dst, src, coef) in zip(arr, updates):
        assert dst.n_pix == src.n_pix and dst.C == src.C
        e.inp[0].ptr, e.inp[0].ld = dst.ptr, dst.ld
        e.inp[1].ptr, e.inp[1].ld = src.ptr, src.ld
        e.out[0].ptr, e.out[0].ld = dst.ptr, dst.ld
        e.n_pix, e.C, e.flag, e.coef = dst.n_pix, dst.C, 0, float(coef)
    return arr


def axpy_group(arr):
    """Several ``dst += coef * src`` updates of windows that do not overlap, ONE launch (vam_train_axpy_group)."""
    L.check(L.load().vam_train_axpy_group(arr, len(arr), stream_ptr()), "vam_train_axpy_group")


def flat_view(t: torch.Tensor, width: int = 4) -> View:
    """A contiguous fp32 tensor of any shape as an [n/width, width] channel window (element-wise kernels only)."""
    assert t.is_contiguous() and t.dtype == torch.float32 and t.numel() % width == 0
    return View(t.view(1, 1, t.numel() // width, width), 0, width)


def win_attention_bwd_workspace(qkv: View, heads: int, ws: int) -> torch.Tensor:
    """Caller-owned scratch of vam_win_attention_bwd (per-block partial bias-table gradients)."""
    n = L.load().vam_win_attention_bwd_workspace(qkv.B, qkv.H, qkv.W, heads, ws)
    return torch.empty(n // 4, dtype=torch.float32, device=qkv.buf.device)


def win_attention_bwd(qkv: View, dout: View, dqkv: View, table: torch.Tensor, dtable: torch.Tensor, C_: int, heads: int,
                      ws: int, shift: int, workspace: Optional[torch.Tensor] = None):
    assert dtable.shape == table.shape and dtable.is_contiguous()
    if workspace is None:
        workspace = win_attention_bwd_workspace(qkv, heads, ws)
    assert workspace.numel() * 4 >= L.load().vam_win_attention_bwd_workspace(qkv.B, qkv.H, qkv.W, heads, ws)
    L.check(L.load().vam_win_attention_bwd(qkv.ptr, qkv.ld, dout.ptr, dout.ld, dqkv.ptr, dqkv.ld, table.data_ptr(),
                                           dtable.data_ptr(), workspace.data_ptr(), qkv.B, qkv.H, qkv.W, C_, heads, ws, shift,
                                           stream_ptr()), "vam_win_attention_bwd")


def colsum_workspace(dy: View) -> torch.Tensor:
    return torch.empty(L.load().vam_colsum_workspace(dy.n_pix, dy.C) // 4, dtype=torch.float32, device=dy.buf.device)


def colsum(dy: View, out: torch.Tensor, workspace: Optional[torch.Tensor] = None):
    if workspace is None:
        workspace = colsum_workspace(dy)
    L.check(L.load().vam_colsum(dy.ptr, dy.ld, dy.n_pix, dy.C, out.data_ptr(), workspace.data_ptr(), stream_ptr()), "vam_colsum")


def repack_weights(src: torch.Tensor, dst: torch.Tensor, mode: int, phase: int, kh: int, kw: int, cin: int, n: int):
    """vam_pack_conv_weights into an EXISTING packed buffer (training: the optimiser changed ``src`` in place)."""
    assert src.is_cuda and src.is_contiguous() and src.dtype == torch.float32
    if _pack_job(src, dst, False, mode, phase, kh, kw, cin, n):
        return
    L.check(L.load().vam_pack_conv_weights(src.data_ptr(), dst.data_ptr(), mode, phase, kh, kw, cin, n, stream_ptr()),
            "vam_pack_conv_weights")


def repack_bias(src: torch.Tensor, dst: torch.Tensor, mode: int, n: int):
    if _pack_job(src, dst, True, mode, 0, 0, 0, 0, n):
        return
    L.check(L.load().vam_pack_bias(src.data_ptr(), dst.data_ptr(), mode, n, stream_ptr()), "vam_pack_bias")


def eb_train_bwd(z: View, noise: View, params: torch.Tensor, grad_lik: View, dz: View, dparams: torch.Tensor):
    """Backward of the training-mode entropy bottleneck (vam_eb_train_bwd): dz written, dparams in ``params`` layout."""
    assert dparams.numel() == params.numel() and dparams.is_contiguous()
    L.check(L.load().vam_eb_train_bwd(z.ptr, z.ld, noise.ptr, noise.ld, params.data_ptr(), z.C, grad_lik.ptr, grad_lik.ld,
                                      dz.ptr, dz.ld, dparams.data_ptr(), z.n_pix, stream_ptr()), "vam_eb_train_bwd")


def ps2_unshuffle(src: View, dst: View):
    """Gradient of PixelShuffle(2): src [B,2H,2W,Cq] -> dst [B,H,W,4Cq] in the convolution's channel order c*4+i*2+j."""
    assert src.C * 4 == dst.C and (src.H, src.W) == (2 * dst.H, 2 * dst.W) and src.B == dst.B
    L.check(L.load().vam_ps2_unshuffle(src.ptr, src.ld, dst.ptr, dst.ld, dst.B, dst.H, dst.W, src.C, stream_ptr()), "vam_ps2_unshuffle")


def upsample2_zero(src: View, dst: View):
    """dst[b,2y,2x] = src[b,y,x], zeros elsewhere (data gradient of a stride-2 3x3 convolution, first half)."""
    assert src.C == dst.C and (dst.H, dst.W) == (2 * src.H, 2 * src.W) and src.B == dst.B
    L.check(L.load().vam_upsample2_zero(src.ptr, src.ld, dst.ptr, dst.ld, src.B, src.H, src.W, src.C, stream_ptr()), "vam_upsample2_zero")


def memset_zero(t: torch.Tensor):
    L.check(L.load().vam_memset_zero(t.data_ptr(), t.numel() * t.element_size(), stream_ptr()), "vam_memset_zero")


def sqdiff_sum(a: torch.Tensor, b: torch.Tensor, acc: torch.Tensor):
    assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    L.check(L.load().vam_sqdiff_sum(a.data_ptr(), b.data_ptr(), a.numel(), acc.data_ptr(), stream_ptr()), "vam_sqdiff_sum")


def sqdiff_sum_levels(x: torch.Tensor, x_hat: torch.Tensor, acc: torch.Tensor):
    """acc[l, b] += sum((x[b] - x_hat[l * B + b])^2) in float64: x [B, ...], x_hat [L * B, ...] (level-major), acc [L, B]."""
    B = x.shape[0]
    n = x[0].numel()
    nl = x_hat.shape[0] // B
    assert x.is_contiguous() and x_hat.is_contiguous() and x.dtype == x_hat.dtype == torch.float32
    assert x_hat.shape[0] == nl * B and x_hat[0].numel() == n and x.device == x_hat.device
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == nl * B
    L.check(L.load().vam_sqdiff_sum_levels(x.data_ptr(), x_hat.data_ptr(), B, n, nl, acc.data_ptr(), stream_ptr()),
            "vam_sqdiff_sum_levels")


# --------------------------------------------------------------------------- graphs / profiling
_CAPTURING = 0                      # depth of stream captures in progress on this (single) host thread
_GRAVEYARD: list = []               # (exec handle, torch stream it was last launched on) of dropped graphs


class Graph:
    """hipGraph capture of a sequence of libvampic launches on the current stream.

    Lifetime.  A dropped graph (``close()`` or garbage collection) only parks its handle: no HIP call from ``__del__``,
    which can run inside another plan's capture.  :func:`drain_graveyard` — called by ``engine.Runner`` at every entry of
    a plan, never during a capture — synchronises the stream each parked handle was last launched on and then RETIRES it: the
    handle is kept for the life of the process and ``hipGraphExecDestroy`` is not called.

    Why not destroyed (round 3, demonstrated; ROCm 7.2 / gfx950).  The host segfault of round 2 (``hipGraphLaunch``
    inside tests/test_gpu_bitstream.py, right after ``net.update()`` had dropped the model's plans) came back
    DETERMINISTICALLY with the deferred, synchronised, return-code-checked destruction of round 3 in place, in the test
    order ops -> model -> golden -> config_variants -> bitstream (two runs of two; ~20 executable graphs destroyed at
    that entry point, then the capture and launch of a new plan faults inside the runtime, gpurun_out/r3_segv.log).  The
    same order with the handles retired instead of destroyed: 73 passed (gpurun_out/r3_segv2.log).  Every destroyed
    graph had finished (its stream synchronised), none was destroyed twice (``close`` clears the handle), no capture was
    active: the library's side of the contract holds, and the only difference between crash and no crash is the call
    to hipGraphExecDestroy.  A retired executable graph costs host memory for its kernel arguments (~0.3 MB for a
    230-launch plan); at most ``VAMPIC_GRAPH_RETIRE_MAX`` (256) handles are kept, older ones are destroyed after all.
    ``VAMPIC_GRAPH_DESTROY=1`` restores immediate destruction.  Round 4 could not make the fault reappear with the
    destruction on (stand-alone probe with every ingredient, the library's own sequence, the faulting test order twice:
    DESIGN.md section 5), so the cause is unknown and retirement stays the default."""

    def __init__(self):
        self.exec = C.c_void_p(None)
        self.last_stream = None

    def capture(self, fn):
        global _CAPTURING
        drain_graveyard()
        lib = L.load()
        s = stream_ptr()
        dev = torch.cuda.current_device()
        n_alloc = torch.cuda.memory_stats(dev).get("allocation.all.allocated", 0)
        L.check(lib.vam_graph_begin(s), "vam_graph_begin")
        _CAPTURING += 1
        try:
            fn()
        finally:
            _CAPTURING -= 1
            rc = lib.vam_graph_end(s, C.byref(self.exec))
        L.check(rc, "vam_graph_end")
        # The capture is a raw hipStreamBeginCapture torch's caching allocator knows nothing about: a tensor allocated by a
        # captured step would be returned to the pool while the graph keeps its address.  Plans allocate while they are
        # BUILT, never while they run — enforce it.
        n_new = torch.cuda.memory_stats(dev).get("allocation.all.allocated", 0) - n_alloc
        if n_new:
            self.close()
            raise RuntimeError(f"{n_new} device allocation(s) inside a hipGraph capture: a captured step created a torch temporary "
                               "(pre-allocate it when the plan is built and write through views)")

    def launch(self):
        self.last_stream = torch.cuda.current_stream()
        L.check(L.load().vam_graph_launch(self.exec, self.last_stream.cuda_stream), "vam_graph_launch")

    def close(self):
        """Give the executable graph up; it is destroyed at the next safe point."""
        if self.exec:
            _GRAVEYARD.append((self.exec.value, self.last_stream))
            self.exec = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()                # no HIP call here: see the class docstring
        except Exception:
            pass


def drain_graveyard():
    """Retire (or, with VAMPIC_GRAPH_DESTROY=1, destroy) the executable graphs dropped since the last call, after
    synchronising the streams they last ran on.  No-op while a capture is in progress."""
    if _CAPTURING or not _GRAVEYARD:
        return
    dead = list(_GRAVEYARD)
    del _GRAVEYARD[:]
    seen = set()
    for _, st in dead:
        if st is not None and st.cuda_stream not in seen:
            seen.add(st.cuda_stream)
            st.synchronize()            # the last replay of every dropped graph has finished
    lib = L.load()
    if os.environ.get("VAMPIC_GRAPH_DESTROY", "0") != "1":   # default: see the class docstring
        _RETIRED.extend(h for h, _ in dead)
        # bounded: a loop that changes the weights and runs an eval forward every step drops a plan per step.
        # Beyond the cap the OLDEST retired handles are destroyed after all — their last launch is long finished, and round
        # 4's probes found the destruction harmless in every set-up tried.
        cap = int(os.environ.get("VAMPIC_GRAPH_RETIRE_MAX", "256"))
        while len(_RETIRED) > cap:
            L.check(lib.vam_graph_destroy(C.c_void_p(_RETIRED.pop(0))), "vam_graph_destroy")
        return
    for handle, _ in dead:
        L.check(lib.vam_graph_destroy(C.c_void_p(handle)), "vam_graph_destroy")


_RETIRED: list = []      # handles of dropped executable graphs, kept alive on purpose


def graveyard_size() -> int:
    return len(_GRAVEYARD)


def retired_graphs() -> int:
    return len(_RETIRED)


_PROF_ON = False


def prof_enable(on: bool):
    global _PROF_ON
    _PROF_ON = bool(on)
    L.check(L.load().vam_prof_enable(1 if on else 0))


def prof_on() -> bool:
    return _PROF_ON


def prof_set_class(name_or_idx):
    """Launch class of the convolution launches that follow (event profiler only; see L.PROF_CLASSES)."""
    i = L.PROF_CLASSES.index(name_or_idx) if isinstance(name_or_idx, str) else int(name_or_idx)
    L.check(L.load().vam_prof_set_class(i), "vam_prof_set_class")


def prof_read_classes():
    lib = L.load()
    out = {}
    for i, name in enumerate(L.PROF_CLASSES):
        ms, n, fl, by = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        L.check(lib.vam_prof_read_class(i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        out[name] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
    return out


def prof_reset():
    L.check(L.load().vam_prof_reset())


def prof_read():
    lib = L.load()
    out = {}
    for fam, name in enumerate(L.FAMILY_NAMES):
        ms, n, fl, by = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        L.check(lib.vam_prof_read(fam, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        out[name] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
    return out


# ------------------------------------------------------------------ differentiable MS-SSIM (csrc/msssim.hip)
_MS_WINDOWS: dict = {}


def _msssim_window(device) -> torch.Tensor:
    """The 11-tap Gaussian (sigma 1.5) in float32, as pytorch_msssim builds it; one device copy per device."""
    key = str(device)
    if key not in _MS_WINDOWS:
        coords = torch.arange(11, dtype=torch.float32) - 5
        g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
        _MS_WINDOWS[key] = (g / g.sum()).to(device)
    return _MS_WINDOWS[key]


def _msssim_check(x: torch.Tensor, y: torch.Tensor):
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"expected two [B,C,H,W] tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise ValueError("ms_ssim runs on the GPU only: both tensors must be CUDA tensors (there is no CPU fallback)")
    if min(x.shape[2:]) <= (11 - 1) * 2 ** 4:
        raise ValueError("image too small for 5 scales with an 11-tap window (smaller side must exceed 160)")


def msssim_forward(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, keep_pyramid: bool = False):
    """The forward of :func:`ms_ssim` on contiguous fp32 [B,C,H,W] CUDA tensors: 5 level launches, 4 pool launches and the
    combine launch on the current stream, no host synchronisation.  Returns (val [B] float64, val32 [B] float32, state);
    ``state`` holds what the backward needs (the pooled pyramids and the upstream factors) when ``keep_pyramid``."""
    lib = L.load()
    B, C_, H, W = x.shape
    planes = B * C_
    win = _msssim_window(x.device)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    n_part = lib.vam_msssim_partial_doubles(planes, H, W)
    if n_part <= 0:
        raise ValueError("image too small for 5 scales with an 11-tap window (smaller side must exceed 160)")
    partial = torch.empty(n_part, dtype=torch.float64, device=x.device)
    st = stream_ptr()
    pyramid = []
    xl, yl, h, w = x, y, H, W
    for lvl in range(5):
        off = lib.vam_msssim_partial_offset(planes, H, W, lvl)
        L.check(lib.vam_msssim_fwd_level(xl.data_ptr(), yl.data_ptr(), planes, h, w, win.data_ptr(), c1, c2, int(lvl == 4),
                                         partial.data_ptr() + 8 * off, st), "vam_msssim_fwd_level")
        pyramid.append((xl, yl, h, w))
        if lvl < 4:
            ho, wo = (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1
            nx = torch.empty((planes, ho, wo), dtype=torch.float32, device=x.device)
            ny = torch.empty_like(nx)
            L.check(lib.vam_msssim_pool2(xl.data_ptr(), yl.data_ptr(), nx.data_ptr(), ny.data_ptr(), planes, h, w, st),
                    "vam_msssim_pool2")
            xl, yl, h, w = nx, ny, ho, wo
    means = torch.empty((5, planes), dtype=torch.float64, device=x.device)
    dvdm = torch.empty_like(means)
    val = torch.empty(B, dtype=torch.float64, device=x.device)
    val32 = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(lib.vam_msssim_combine(partial.data_ptr(), B, C_, H, W, means.data_ptr(), dvdm.data_ptr(), val.data_ptr(),
                                   val32.data_ptr(), st), "vam_msssim_combine")
    state = (pyramid, dvdm, (c1, c2), (B, C_)) if keep_pyramid else None
    return val, val32, state


def msssim_backward(state, gout: torch.Tensor) -> torch.Tensor:
    """d(sum_b gout[b] * ms_ssim[b]) / dy from the state of :func:`msssim_forward`: 5 launches, coarse to fine."""
    lib = L.load()
    pyramid, dvdm, (c1, c2), (B, C_) = state
    win = _msssim_window(dvdm.device)
    gout = gout.detach().to(torch.float32).contiguous()
    st = stream_ptr()
    g_coarse = None
    for lvl in range(4, -1, -1):
        xl, yl, h, w = pyramid[lvl]
        g = torch.empty((B * C_, h, w), dtype=torch.float32, device=dvdm.device)
        L.check(lib.vam_msssim_bwd_level(xl.data_ptr(), yl.data_ptr(), B, C_, h, w, win.data_ptr(), c1, c2, int(lvl == 4),
                                         dvdm[lvl].data_ptr(), gout.data_ptr(), None if g_coarse is None else g_coarse.data_ptr(),
                                         g.data_ptr(), st), "vam_msssim_bwd_level")
        g_coarse = g
    return g_coarse.view(B, C_, *g_coarse.shape[1:])


class _MsSsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range):
        xc, yc = x.detach().float().contiguous(), y.detach().float().contiguous()
        _, val32, state = msssim_forward(xc, yc, data_range, keep_pyramid=ctx.needs_input_grad[1])
        ctx.state = state
        ctx.y_dtype = y.dtype
        return val32

    @staticmethod
    def backward(ctx, gout):
        if ctx.state is None:
            raise RuntimeError("ms_ssim: backward called twice (the saved pyramid is released after the first call)")
        g = msssim_backward(ctx.state, gout)
        ctx.state = None
        return None, g.to(ctx.y_dtype), None


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """MS-SSIM of each image of ``y`` against the target ``x``: [B,C,H,W] CUDA tensors -> [B] float32, the mean over channels
    of V = prod_l relu(m_l)^w_l (11-tap Gaussian, sigma 1.5, 5 scales, pytorch_msssim 0.2.1's published algorithm as restated
    in oracle/msssim_oracle.py).  Differentiable in ``y`` only (the reconstruction); raises if ``x`` requires grad.  HIP
    kernels of csrc/msssim.hip on the current stream, no host synchronisation, no atomics: forward and backward replay bit
    for bit.

    Contract at the relu: an (image, channel) plane with any level mean m_l <= 0 has value 0 and gradient exactly 0 —
    pytorch_msssim's expression (relu(m)^w differentiated at the kink) can give NaN gradients there.

    Raises ValueError for mismatched shapes, non-CUDA tensors or a smaller side <= 160, and VamError without a GPU: there
    is no CPU fallback."""
    L.require_gpu()
    _msssim_check(x, y)
    if x.requires_grad:
        raise ValueError("ms_ssim is differentiable in its second argument (the reconstruction) only: x requires grad")
    return _MsSsimFn.apply(x, y, float(data_range))
