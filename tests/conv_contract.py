"""The convolution problem contract of include/vampic.h, stated as a float64 reference and a table of small cases.

    out = post2 + post + mul * act(conv(cat(seg...)) + bias + pre)            (struct vam_conv)

``reference(case)`` evaluates that line in float64 on the CPU from the fp32 inputs, with nothing of the library in it:
F.pad + F.conv2d for the core, index arithmetic for the placement, the nine activations written out.  ``build(case, device)``
makes the same problem for ``vam_conv_group`` straight from the OIHW weights (no ``layers`` module in between), every tensor
a channel window of its own wider buffer.  ``check_z`` / ``check_rms`` / ``check_out`` are the bounds the GPU test asserts;
tests/test_conv_contract_cpu.py shows that an fp32 ATen evaluation of the same formula meets them.

Helper module (not collected), in the manner of tests/levels_oracle.py."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

import vampic.synth

U = 2.0 ** -24                    # unit roundoff of fp32
SENTINEL = -777.25                # what every output buffer holds before a launch (exact in fp32)
EPI_ULPS = 16                     # the epilogue constant of check_out (see test_conv_contract_cpu for what may move it)
ACTS = ("NONE", "GELU", "LEAKY", "HALF_TANH", "SIGMOID", "CLAMP01", "RSQRT", "SQRT", "DOUBLE")     # enum vam_act, in order
OPERANDS = ("pre", "mul", "post", "post2")


@dataclass(frozen=True)
class Case:
    id: str
    segs: Tuple[int, ...]         # channels of each input segment (virtually concatenated)
    n: int                        # output channels of the problem (4 * Cq under PS2)
    kh: int
    kw: int
    B: int
    H: int
    W: int
    stride: int = 1
    pad_y: Optional[int] = None   # None: k // 2
    pad_x: Optional[int] = None
    full: Optional[Tuple[int, int]] = None      # Hf, Wf of a strided / offset placement
    osy: int = 1
    osx: int = 1
    ooy: int = 0
    oox: int = 0
    ps2: bool = False
    nchw: bool = False
    act: str = "NONE"
    operands: Tuple[str, ...] = ()
    square_in: bool = False       # VAM_CONV_SQUARE_IN
    gelu_grad: bool = False       # VAM_CONV_MUL_GELU_GRAD (conv_problem's gelu_z=)
    preact: bool = False          # the second output
    gdn: bool = False             # positive weights and bias, mul = the input itself, pre >= 0 (keeps z >= 0.5)

    def __post_init__(self):
        if self.pad_y is None:
            object.__setattr__(self, "pad_y", self.kh // 2)
        if self.pad_x is None:
            object.__setattr__(self, "pad_x", self.kw // 2)
        # the written limits of the interface
        assert self.cin % 16 == 0 and self.n % 4 == 0
        assert all(sum(self.segs[:i + 1]) % 32 == 0 for i in range(len(self.segs) - 1))
        assert not (self.cin == 16 and self.kh * self.kw > 1) or len(self.segs) == 1
        assert 1 <= len(self.segs) <= 4 and self.stride in (1, 2)

    @property
    def cin(self): return sum(self.segs)
    @property
    def K(self): return self.cin * self.kh * self.kw
    @property
    def Ho(self): return self.H if self.stride == 1 else (self.H + 2 * self.pad_y - self.kh) // self.stride + 1
    @property
    def Wo(self): return self.W if self.stride == 1 else (self.W + 2 * self.pad_x - self.kw) // self.stride + 1
    @property
    def Hf(self): return 2 * self.Ho if self.ps2 else (self.full[0] if self.full else self.Ho)
    @property
    def Wf(self): return 2 * self.Wo if self.ps2 else (self.full[1] if self.full else self.Wo)
    @property
    def cout(self): return self.n // 4 if self.ps2 else self.n       # channels of the stored tensor


def _table():
    c = [
        Case("g1", (16,), 4, 3, 3, 1, 1, 1),
        Case("g2", (16,), 36, 5, 5, 3, 5, 3),
        Case("g3", (32, 16), 68, 3, 3, 3, 7, 5),
        Case("g4", (32, 64, 16), 228, 3, 3, 2, 9, 7),
        Case("g5", (64,), 32, 5, 5, 2, 7, 9, stride=2),
        Case("g6", (32,), 12, 3, 3, 2, 5, 6, stride=2),
        Case("g7a", (64,), 20, 3, 2, 2, 4, 5, pad_y=1, pad_x=0, full=(8, 10), osy=2, osx=2, ooy=0, oox=1),
        Case("g7b", (64,), 20, 2, 3, 2, 4, 5, pad_y=0, pad_x=1, full=(8, 10), osy=2, osx=2, ooy=1, oox=0),
        Case("g7c", (64,), 20, 2, 2, 2, 4, 5, pad_y=0, pad_x=0, full=(8, 10), osy=2, osx=2, ooy=1, oox=1),
        Case("g8", (32, 32, 32, 32), 64, 1, 1, 5, 3, 3),
        Case("g9a", (32,), 16, 3, 3, 2, 3, 5, ps2=True),
        Case("g9b", (32,), 12, 3, 3, 2, 3, 5, ps2=True),
        Case("g10", (32,), 12, 3, 3, 2, 5, 7, nchw=True),
        Case("g11", (32,), 96, 3, 3, 1, 13, 21),
    ]
    by = {k.id: k for k in c}
    for a in ("NONE", "GELU", "LEAKY", "HALF_TANH", "SIGMOID", "CLAMP01", "DOUBLE"):
        c.append(Case("e-" + a, (32, 16), 36, 3, 3, 3, 5, 3, act=a, operands=OPERANDS))
    c.append(replace(by["g9a"], id="e-ps2", act="GELU", operands=OPERANDS))
    c.append(replace(by["g7a"], id="e-phase", act="LEAKY", operands=OPERANDS))
    for a in ("RSQRT", "SQRT"):
        c.append(Case("e-gdn-" + a, (32,), 32, 1, 1, 2, 4, 4, act=a, operands=OPERANDS, square_in=True, gdn=True))
    c.append(Case("e-preact", (32, 16), 36, 3, 3, 3, 5, 3, act="GELU", operands=OPERANDS, preact=True))
    c.append(Case("e-gelugrad", (32, 16), 36, 3, 3, 3, 5, 3, operands=("pre", "mul"), gelu_grad=True))
    return {k.id: k for k in c}


CASES: Dict[str, Case] = _table()
Z_CASES = [k for k, v in CASES.items() if v.act == "NONE" and not set(v.operands) & {"mul", "post", "post2"}]   # out == z
RMS_CASES = ("g4", "g11", "e-preact")          # thousands of outputs: the statistical bound means something
OUT_CASES = [k for k in CASES if k.startswith("e-")]


# ------------------------------------------------------------------------------------------------ inputs
def tensors(case: Case) -> dict:
    """The fp32 CPU inputs of a case, NCHW: ``segs`` (list), ``w`` (OIHW; under PS2 O is in PixelShuffle order c*4+i*2+j),
    ``b`` and the epilogue operands at the stored tensor's shape [B, cout, Hf, Wf].  Fixed seeds, host-independent."""
    seed = 1000 * (1 + list(CASES).index(case.id) if case.id in CASES else 77)
    nrm = vampic.synth.normal
    t = {"segs": [nrm((case.B, c, case.H, case.W), seed + i) for i, c in enumerate(case.segs)]}
    wshape = (case.n, case.cin, case.kh, case.kw)
    if case.gdn:
        t["w"] = nrm(wshape, seed + 10).abs() / 32.0
        t["b"] = 0.5 + nrm((case.n,), seed + 11).abs()
    else:
        t["w"] = nrm(wshape, seed + 10, 1.0 / math.sqrt(case.K))
        t["b"] = nrm((case.n,), seed + 11, 0.5)
    oshape = (case.B, case.cout, case.Hf, case.Wf)
    for i, name in enumerate(OPERANDS):
        if name in case.operands:
            t[name] = nrm(oshape, seed + 20 + i)
    if case.gdn:
        t["pre"] = t["pre"].abs()
        t["mul"] = t["segs"][0]                 # GDN: x * rsqrt(beta + gamma x^2); 1x1 stride 1, so the shapes agree
    return t


# ------------------------------------------------------------------------------------------------ the formula
def _act(name: str, z: torch.Tensor) -> torch.Tensor:
    if name == "NONE": return z
    if name == "GELU": return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if name == "LEAKY": return torch.where(z > 0, z, 0.01 * z)
    if name == "HALF_TANH": return 0.5 * torch.tanh(z)
    if name == "SIGMOID": return 1.0 / (1.0 + torch.exp(-z))
    if name == "CLAMP01": return z.clamp(0.0, 1.0)
    if name == "RSQRT": return 1.0 / torch.sqrt(z)
    if name == "SQRT": return torch.sqrt(z)
    if name == "DOUBLE": return 2.0 * z
    raise ValueError(name)


def _gelu_grad(m: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(m / math.sqrt(2.0))) + m * torch.exp(-0.5 * m * m) / math.sqrt(2.0 * math.pi)


def _core(case: Case, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """core[b,n,oy,ox] = sum w[n,c,ty,tx] x[b,c, oy*stride - pad_y + ty, ox*stride - pad_x + tx], zeros outside the image."""
    s, Ho, Wo = case.stride, case.Ho, case.Wo
    right = max((Wo - 1) * s - case.pad_x + case.kw - case.W, 0)
    below = max((Ho - 1) * s - case.pad_y + case.kh - case.H, 0)
    y = F.conv2d(F.pad(x, (case.pad_x, right, case.pad_y, below)), w, stride=s)
    return y[:, :, :Ho, :Wo]


def _place(case: Case, v: torch.Tensor) -> torch.Tensor:
    """[B, n, Ho, Wo] -> the stored tensor [B, cout, Hf, Wf] (zeros where the problem does not write)."""
    if case.ps2:
        return F.pixel_shuffle(v, 2)
    full = torch.zeros((case.B, case.n, case.Hf, case.Wf), dtype=v.dtype)
    ys = case.ooy + case.osy * torch.arange(case.Ho)
    xs = case.oox + case.osx * torch.arange(case.Wo)
    full[:, :, ys[:, None], xs[None, :]] = v
    return full


def evaluate(case: Case, t: Optional[dict] = None, dtype=torch.float64) -> SimpleNamespace:
    """The contract in ``dtype``.  Returns out, z (what preact must hold), written (bool map of the owned elements),
    abs_sum (the same core on |x|, |w| plus |bias| + |pre|: the scale of check_z), and the pieces check_out weighs
    (act_z, mul = the effective multiplier, post, post2).  All at the stored tensor's shape [B, cout, Hf, Wf]."""
    t = t or tensors(case)
    x = torch.cat([s.to(dtype) for s in t["segs"]], 1)
    if case.square_in:
        x = x * x
    w, b = t["w"].to(dtype), t["b"].to(dtype).reshape(1, -1, 1, 1)
    zero = torch.zeros((case.B, case.cout, case.Hf, case.Wf), dtype=dtype)
    op = {k: (t[k].to(dtype) if k in t else None) for k in OPERANDS}
    written = _place(case, torch.ones((case.B, case.n, case.Ho, case.Wo))) > 0
    z = _place(case, _core(case, x, w) + b)
    abs_sum = _place(case, _core(case, x.abs(), w.abs()) + b.abs())
    if op["pre"] is not None:
        z = z + op["pre"]
        abs_sum = abs_sum + op["pre"].abs()
    z = torch.where(written, z, torch.ones_like(z))          # unowned elements: any value every activation accepts
    act_z = _act(case.act, z)
    out, mul = act_z, None
    if op["mul"] is not None:
        mul = _gelu_grad(op["mul"]) if case.gelu_grad else op["mul"]
        out = out * mul
    if op["post"] is not None:
        out = out + op["post"]
    if op["post2"] is not None:
        out = out + op["post2"]
    return SimpleNamespace(out=out, z=z, written=written, abs_sum=abs_sum, act_z=act_z, mul=mul if mul is not None else zero + 1.0,
                           post=op["post"] if op["post"] is not None else zero, post2=op["post2"] if op["post2"] is not None else zero)


def reference(case: Case, t: Optional[dict] = None) -> SimpleNamespace:
    return evaluate(case, t, torch.float64)


# ------------------------------------------------------------------------------------------------ bounds
def _ratio(err: torch.Tensor, bound: torch.Tensor, written: torch.Tensor) -> float:
    """max err / bound over the owned elements; inf when an owned element is not finite."""
    e, bnd = err[written], bound[written]
    if not bool(torch.isfinite(e).all()):
        return float("inf")
    return float((e / bnd).max())


def z_bound(case: Case, ref) -> torch.Tensor:
    """Worst case of an fp32 accumulation of K exact products, in any order, plus bias and pre: (K + 4) u abs_sum."""
    return (case.K + 4) * U * ref.abs_sum


def check_z(case: Case, ref, z_got: torch.Tensor, what="") -> float:
    r = _ratio((z_got.double() - ref.z).abs(), z_bound(case, ref), ref.written)
    assert r <= 1.0, f"{case.id} {what}: |z - z64| reaches {r:.3g} x the bound (K + 4) 2^-24 abs_sum"
    return r


def check_rms(case: Case, ref, z_got: torch.Tensor, what="") -> float:
    """rms(z - z64) <= (0.5 sqrt(K) + 2) 2^-24 rms(z64): the bound of test_conv_accuracy_against_float64, unchanged."""
    w = ref.written
    e = (z_got.double() - ref.z)[w].pow(2).mean().sqrt().item()
    bound = (0.5 * math.sqrt(case.K) + 2.0) * U * ref.z[w].pow(2).mean().sqrt().item()
    assert e <= bound, f"{case.id} {what}: rms error {e:.3e} above (0.5 sqrt(K) + 2) 2^-24 rms(z64) = {bound:.3e}"
    return e / bound


def out_bound(case: Case, ref, ulps: float = EPI_ULPS) -> torch.Tensor:
    ez = z_bound(case, ref)
    lip = {"NONE": 1.0, "LEAKY": 1.0, "CLAMP01": 1.0, "GELU": 1.13, "HALF_TANH": 0.5, "SIGMOID": 0.25, "DOUBLE": 2.0}.get(case.act)
    if lip is None:
        lo = ref.z - ez
        assert bool((lo[ref.written] > 0).all()), f"{case.id}: z - E_z must stay positive under {case.act}"
        lo = torch.where(ref.written, lo, torch.ones_like(lo))
        lip = 0.5 * lo.pow(-1.5 if case.act == "RSQRT" else -0.5)
    return lip * ref.mul.abs() * ez + ulps * U * (1.0 + (ref.act_z * ref.mul).abs() + ref.post.abs() + ref.post2.abs())


def check_out(case: Case, ref, out_got: torch.Tensor, what="", ulps: float = EPI_ULPS) -> float:
    r = _ratio((out_got.double() - ref.out).abs(), out_bound(case, ref, ulps), ref.written)
    assert r <= 1.0, f"{case.id} {what}: |out - out64| reaches {r:.3g} x the bound Lip |mul| E_z + {ulps} 2^-24 (1 + |act mul| + |post| + |post2|)"
    return r


# ------------------------------------------------------------------------------------------------ the GPU side
def _round4(v: int) -> int:
    return (v + 3) // 4 * 4


class Built:
    """A case on the device: packed weights, the input and operand windows (each inside its own NaN-filled buffer, no two
    with the same pixel stride), and ``problem()`` = a fresh sentinel-filled output (and preact) buffer with the vam_conv
    that writes into it."""

    def __init__(self, case: Case, device, t: Optional[dict] = None):
        from vampic import ops, _lib as L
        self.case, self.device, self.t = case, device, t or tensors(case)
        self._lds = set()
        mode = L.PACK_PS2 if case.ps2 else L.PACK_CONV
        self.pk = ops.Packed(ops.pack_weights(self.t["w"].to(device), mode, 0, case.kh, case.kw, case.cin, case.n),
                             ops.pack_bias(self.t["b"].to(device), mode, case.n), case.kh, case.kw, case.cin, case.n,
                             case.stride, case.pad_y, case.pad_x, ps2_cq=case.cout if case.ps2 else 0,
                             osy=case.osy, osx=case.osx, ooy=case.ooy, oox=case.oox)
        self.segs = [self._window(s, 4 if i % 2 == 0 else 8) for i, s in enumerate(self.t["segs"])]
        self.aux = {}
        for i, k in enumerate(OPERANDS):
            if k in case.operands:
                self.aux[k] = self.segs[0] if case.gdn and k == "mul" else self._window(self.t[k], 8 if i % 2 == 0 else 4)
        self.ld_out, self.ld_preact = self._ld(case.cout + 8), self._ld(case.cout + 8)

    def _ld(self, least: int) -> int:
        ld = _round4(least)
        while ld in self._lds:
            ld += 4
        self._lds.add(ld)
        return ld

    def _window(self, nchw: torch.Tensor, off: int):
        from vampic import ops
        B, C, H, W = nchw.shape
        buf = torch.full((B, H, W, self._ld(C + off + 4)), float("nan"), dtype=torch.float32, device=self.device)
        buf[..., off:off + C] = nchw.permute(0, 2, 3, 1).to(self.device)
        return ops.View(buf, off, C)

    def _nhwc_out(self, ld: int):
        from vampic import ops
        c = self.case
        buf = torch.full((c.B + 1, c.Hf, c.Wf, ld), SENTINEL, dtype=torch.float32, device=self.device)
        return buf, ops.View(buf[:c.B], 4, c.cout)

    def problem(self, concat: bool = False):
        """(vam_conv, whole output buffer, whole preact buffer or None).  ``concat``: the input as ONE contiguous tensor
        holding the concatenation of the segments."""
        from vampic import ops, _lib as L
        c = self.case
        inputs = self.segs
        if concat:
            inputs = [ops.View(torch.cat([s.permute(0, 2, 3, 1) for s in self.t["segs"]], 3).contiguous().to(self.device), 0, c.cin)]
        kw = {k: v for k, v in self.aux.items() if not (c.gelu_grad and k == "mul")}
        pbuf = None
        if c.preact:
            pbuf, kw["preact"] = self._nhwc_out(self.ld_preact)
        if c.gelu_grad:
            kw["gelu_z"] = self.aux["mul"]
        flags = L.CONV_SQUARE_IN if c.square_in else 0
        act = ACTS.index(c.act)
        if c.nchw:
            obuf = torch.full((c.B + 1, c.cout, c.Hf, c.Wf), SENTINEL, dtype=torch.float32, device=self.device)
            prob = ops.conv_problem(self.pk, inputs, None, act, flags=flags, out_nchw=obuf[:c.B], **kw)
        else:
            obuf, oview = self._nhwc_out(self.ld_out)
            prob = ops.conv_problem(self.pk, inputs, oview, act, flags=flags, **kw)
        prob._keep = (inputs, obuf, pbuf, kw)
        return prob, obuf, pbuf

    def read(self, buf: torch.Tensor, written: torch.Tensor, nchw: bool = False):
        """From a whole output buffer (any device): the stored tensor [B, cout, Hf, Wf] on the CPU, and how many elements
        outside ``written`` (guard channels, the spare image, unowned positions) no longer hold the sentinel's bits."""
        c = self.case
        buf = buf.cpu()
        owned = torch.zeros(buf.shape, dtype=torch.bool)
        if nchw:
            owned[:c.B] = written
            val = buf[:c.B].clone()
        else:
            owned[:c.B, :, :, 4:4 + c.cout] = written.permute(0, 2, 3, 1)
            val = buf[:c.B, :, :, 4:4 + c.cout].permute(0, 3, 1, 2).contiguous()
        sent = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
        stray = int((buf.view(torch.int32)[~owned] != sent).sum())
        return val, stray


def build(case: Case, device, t: Optional[dict] = None) -> Built:
    return Built(case, device, t)
