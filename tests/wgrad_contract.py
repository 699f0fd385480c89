"""The weight-gradient contract of include/vampic.h (struct vam_wgrad), stated as a float64 reference and a table of small
cases.

    dW[n, c_off + c, ty, tx] = sum_{b,oy,ox} dY[b,oy,ox,n] * X[b, s*oy + ty - k/2, s*ox + tx - k/2, c]   (zero outside the image)
    db[n]                    = sum_{b,oy,ox} dY[b,oy,ox,n]

``reference(case)`` evaluates these two lines in float64 on the CPU from the fp32 inputs with nothing of the library and
no ``F.conv2d`` in it: a loop over the k x k taps, each a pixel GEMM of dY with a shifted window of the zero-padded input.
The same pass gives ``abs_sum`` = sum |dY| |X|, the scale of the elementwise bound.  ``build(case, device)`` makes the
problem for ``vam_conv_wgrad_group``: every input a channel window of its own wider NaN-filled buffer with a spare NaN
image behind the last, ``dw`` / ``db`` contiguous slices of flat sentinel-filled buffers with guard elements on both sides,
the workspace of a pixel-split problem NaN-filled.  ``check_dw`` / ``check_db`` / ``check_rms`` are the bounds the GPU test
asserts (the forms of tests/conv_contract.py with the reduction length K = B H W); tests/test_wgrad_contract_cpu.py
shows that fp32 ATen autograd meets them and that seven wrong formulas do not.

Helper module (not collected), in the manner of tests/conv_contract.py."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

import vampic.synth

U = 2.0 ** -24                    # unit roundoff of fp32
SENTINEL = -777.25                # what dw / db hold before a launch (exact in fp32)
GUARD = 8                         # sentinel elements before and after dw, db and behind a workspace
KERNELS = ("gather", "lds")       # out[0] of vam_conv_wgrad_route


@dataclass(frozen=True)
class Case:
    id: str
    segs: Tuple[int, ...]         # channels of each input segment (virtually concatenated; one problem per segment)
    n: int                        # output channels
    k: int
    B: int
    H: int                        # the OUTPUT grid (the extent of dy); x is stride times as large
    W: int
    stride: int = 1
    splits: Optional[int] = None  # None: what vam_conv_wgrad_plan says for the problem alone; else forced
    db: bool = True               # hand a db pointer to every segment's problem (only c_off == 0 may write it)
    plane: bool = False           # x as bf16x3 planes (View3)
    dw2d: bool = False            # ops.wgrad_problems gets dw as a 2-D [N, cin] tensor

    @property
    def cin(self): return sum(self.segs)
    @property
    def taps(self): return self.k * self.k
    @property
    def K(self): return self.B * self.H * self.W      # the reduction length
    @property
    def Hx(self): return self.stride * self.H
    @property
    def Wx(self): return self.stride * self.W
    @property
    def c_offs(self): return [sum(self.segs[:i]) for i in range(len(self.segs))]


# (N, C) that sit ragged inside each tile of the LDS kernel (wgrad2_tile): C <= 32 -> 4 x 1 waves (128 x 32), N = 96 -> 3 x 2
# (96 x 64), else 2 x 2 (64 x 64; two tiles each way at 132 x 68).  k5 stride 2 below 65536 pixels: 4 x 2 with 64-pixel chunks.
_A, _B, _C = (36, 20), (132, 68), (96, 64)


def _table():
    c = [
        # ---- register-gather kernel (grids the LDS kernel declines), one case per tile (TN, TC) of wgrad_tile
        Case("w11", (20,), 24, 3, 2, 5, 7),                    # K = 70: the `pin` edge of the last 16-pixel step; N < 32
        Case("w21", (6,), 60, 3, 2, 5, 7),                     # C % 4 != 0
        Case("w12", (60,), 24, 3, 3, 5, 7),
        Case("w22", (60,), 60, 3, 2, 8, 8),
        Case("w31", (20,), 96, 3, 2, 7, 5),
        Case("w32", (60,), 96, 3, 2, 5, 7),
        Case("wk1seg", (20, 8, 36), 36, 1, 2, 5, 7, dw2d=True),
        Case("wk5s2", (20,), 24, 5, 2, 4, 6, stride=2),        # x is 8 x 12
        Case("wk3s2", (36,), 40, 3, 3, 4, 6, stride=2),
        # ---- LDS kernel, k3 stride 1
        Case("l3a16", (_A[1],), _A[0], 3, 3, 4, 16),           # W = 16: 6 chunks of 32 (prefetch branch), chunks start at images
        Case("l3b16", (_B[1],), _B[0], 3, 3, 4, 16),
        Case("l3c16", (_C[1],), _C[0], 3, 3, 4, 16),
        Case("l3b32", (_B[1],), _B[0], 3, 2, 2, 32),
        Case("l3a64", (_A[1],), _A[0], 3, 2, 1, 64),           # H = 1
        Case("l3b64", (_B[1],), _B[0], 3, 2, 1, 64),
        Case("l3c64", (_C[1],), _C[0], 3, 2, 1, 64),
        Case("l3b128", (_B[1],), _B[0], 3, 1, 1, 128),         # later chunks of a row: the halo crosses the chunk edge
        # ---- k5 stride 1, k3 stride 2
        Case("l5a16", (_A[1],), _A[0], 5, 3, 4, 16),
        Case("l5b64", (_B[1],), _B[0], 5, 2, 1, 64),
        Case("l5c16", (_C[1],), _C[0], 5, 3, 4, 16),
        Case("l5c64", (_C[1],), _C[0], 5, 2, 2, 64),
        Case("l3s2a16", (_A[1],), _A[0], 3, 3, 4, 16, stride=2),
        Case("l3s2b16", (_B[1],), _B[0], 3, 3, 4, 16, stride=2),
        Case("l3s2b64", (_B[1],), _B[0], 3, 2, 1, 64, stride=2),
        Case("l3s2c64", (_C[1],), _C[0], 3, 2, 1, 64, stride=2),
        # ---- k5 stride 2: 4 x 1 / 32-pixel chunks at C <= 32, else 4 x 2 / 64-pixel chunks
        Case("l5s2a16", (_A[1],), _A[0], 5, 3, 4, 16, stride=2),
        Case("l5s2b16", (_B[1],), _B[0], 5, 3, 4, 16, stride=2),     # R = 4 image rows per chunk
        Case("l5s2c64", (_C[1],), _C[0], 5, 2, 1, 64, stride=2),     # one row of one image per chunk
        Case("l5s2b128", (_B[1],), _B[0], 5, 1, 1, 128, stride=2),   # a row made of two chunks
        Case("l5s2a64", (_A[1],), _A[0], 5, 2, 1, 64, stride=2),
        # ... and its 64 x 64 / 96 x 64 tiles, taken from 65536 output pixels on
        Case("l5s2big22", (64,), 36, 5, 1, 512, 128, stride=2),
        Case("l5s2big32", (64,), 96, 5, 4, 256, 64, stride=2),
        # ---- 1x1 layers: waves own 2 x 1 / 1 x 2 / 2 x 2 blocks
        Case("lk1a", (36,), 132, 1, 3, 4, 16),
        Case("lk1b", (100,), 68, 1, 2, 1, 64),
        Case("lk1c", (100,), 100, 1, 2, 2, 32),
        # ---- three segments whose tiles differ
        Case("lseg", (20, 68, 32), 132, 3, 3, 4, 16),
        # ---- plane input on its three tiles
        Case("lpa", (24,), 36, 3, 3, 4, 16, plane=True),
        Case("lpb", (80,), 132, 3, 3, 4, 16, plane=True),
        Case("lpc", (64,), 96, 3, 3, 4, 16, plane=True),
        # ---- pixel splits.  LDS kernel: 18 chunks of 32
        Case("ls2", (_B[1],), _B[0], 3, 9, 4, 16, splits=2),
        Case("ls4", (_B[1],), _B[0], 3, 9, 4, 16, splits=4),         # 5, 5, 5, 3 chunks
        Case("ls7", (_B[1],), _B[0], 3, 9, 4, 16, splits=7),         # 3 chunks each, the last split empty
        Case("lsplan", (_B[1],), _B[0], 3, 9, 4, 16),                # the planner's own S > 1
        Case("ls2n", (_B[1],), _B[0], 3, 9, 4, 16, splits=2, db=False),
        Case("ls2seg", (20, 68), 132, 3, 9, 4, 16, splits=2),        # c_off > 0 with splits, db requested
        # gather kernel: 4096 pixels
        Case("gs2", (32,), 32, 1, 64, 8, 8, splits=2),
        Case("gs3", (32,), 32, 1, 64, 8, 8, splits=3),               # 1376, 1376, 1344 pixels
        Case("gsplan", (20,), 24, 3, 64, 8, 8),
        Case("gs2n", (32,), 32, 1, 64, 8, 8, splits=2, db=False),
        Case("gs2seg", (32, 32), 32, 1, 64, 8, 8, splits=2),
        # db = None at c_off > 0 on a split problem, both kernels
        Case("ls2segn", (20, 68), 132, 3, 9, 4, 16, splits=2, db=False),
        Case("gs2segn", (32, 32), 32, 1, 64, 8, 8, splits=2, db=False),
    ]
    return {k.id: k for k in c}


CASES: Dict[str, Case] = _table()
RMS_CASES = ("w32", "l3b16", "l5s2big32")       # thousands of outputs: the statistical bound means something
BIG_CASES = ("l5s2big22", "l5s2big32")
PLANE_CASES = ("lpa", "lpb", "lpc")
PROBE = "l3b16"                                  # a case the LDS kernel must take in the default mode
PLAN_CASES = ("lsplan", "gsplan", "l5s2big22", "l5s2big32")   # vam_conv_wgrad_plan itself returns more than 1

# Every (kernel, pipe, wn, wc, tn, tc, kp, plane) the dispatchers can launch in the default mode without the measurement
# switches VAMPIC_WGRAD_TILE / VAMPIC_WGRAD_KP, with the template arguments that vam_conv_wgrad_route does not report:
# (kernel size, stride) for the LDS kernel's k3 / k5 instantiations.
def reachable_default():
    want = set()
    for tn, tc in ((1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (3, 2)):
        want.add(("gather", 1, 0, 0, tn, tc, 16, 0, None, None))
    for k, s in ((3, 1), (5, 1), (3, 2), (5, 2)):
        for wn, wc in ((4, 1), (3, 2), (2, 2)):
            want.add(("lds", 1, wn, wc, 1, 1, 32, 0, k, s))
    want.add(("lds", 1, 4, 2, 1, 1, 64, 0, 5, 2))
    for wn, wc in ((4, 1), (3, 2), (2, 2)):
        want.add(("lds", 1, wn, wc, 1, 1, 32, 1, 3, 1))
    for wn, wc, tn, tc in ((3, 2, 2, 1), (3, 2, 1, 2), (2, 2, 2, 2)):
        want.add(("lds", 1, wn, wc, tn, tc, 32, 0, 1, 1))
    return want


# ------------------------------------------------------------------------------------------------ inputs
def tensors(case: Case) -> dict:
    """The fp32 CPU inputs of a case, NCHW: ``segs`` (list, [B, C, Hx, Wx]) and ``dy`` [B, n, H, W].  Fixed seeds."""
    seed = 1000 * (101 + list(CASES).index(case.id) if case.id in CASES else 77)
    nrm = vampic.synth.normal
    return {"segs": [nrm((case.B, c, case.Hx, case.Wx), seed + i) for i, c in enumerate(case.segs)],
            "dy": nrm((case.B, case.n, case.H, case.W), seed + 9)}


def one_hot(case: Case, pixels) -> dict:
    """The inputs of ``case`` with dy = 0 except 1.0 at (pixel_i, channel n_i = 3 i + 1)."""
    t = dict(tensors(case))
    dy = torch.zeros((case.B * case.H * case.W, case.n))
    for i, p in enumerate(pixels):
        dy[p, 3 * i + 1] = 1.0
    t["dy"] = dy.reshape(case.B, case.H, case.W, case.n).permute(0, 3, 1, 2).contiguous()
    return t


# ------------------------------------------------------------------------------------------------ the formula
def evaluate(case: Case, t: Optional[dict] = None, dtype=torch.float64, shift=(0, 0)) -> SimpleNamespace:
    """The contract in ``dtype`` as a loop over taps of pixel GEMMs.  ``shift`` is added to the input position (dy, dx) and
    is (0, 0) for the contract; the CPU test uses it to state wrong formulas.  Returns dw [n, cin, k, k], db [n], abs_sum
    (dw's shape: sum |dY| |X|) and abs_db (sum |dY|)."""
    t = t or tensors(case)
    s, k, pad, H, W = case.stride, case.k, case.k // 2, case.H, case.W
    x = torch.cat([v.to(dtype) for v in t["segs"]], 1)
    dy = t["dy"].to(dtype).permute(1, 0, 2, 3).reshape(case.n, -1)                # [n, pixels]
    m = pad + 2                                                                    # room for the shifts of the wrong formulas
    xp = F.pad(x, (m, m + 2, m, m + 2))                                            # zeros outside the image
    dw = torch.zeros((case.n, case.cin, k, k), dtype=dtype)
    ab = torch.zeros_like(dw)
    for ty in range(k):
        for tx in range(k):
            y0, x0 = ty - pad + shift[0] + m, tx - pad + shift[1] + m             # input row of output row 0, in xp
            win = xp[:, :, y0:y0 + s * (H - 1) + 1:s, x0:x0 + s * (W - 1) + 1:s]   # X[b, c, s oy + ty - pad, s ox + tx - pad]
            win = win.permute(1, 0, 2, 3).reshape(case.cin, -1)                    # [cin, pixels]
            dw[:, :, ty, tx] = dy @ win.t()
            ab[:, :, ty, tx] = dy.abs() @ win.abs().t()
    return SimpleNamespace(dw=dw, db=dy.sum(1), abs_sum=ab, abs_db=dy.abs().sum(1))


def reference(case: Case, t: Optional[dict] = None) -> SimpleNamespace:
    return evaluate(case, t, torch.float64)


# ------------------------------------------------------------------------------------------------ bounds
def _ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err / bound; inf when an element is not finite; 0 / 0 (an all-zero input column) counts as 0."""
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(r.max())


def check_dw(case: Case, ref, dw: torch.Tensor, what="") -> float:
    """Worst case of an fp32 accumulation of K exact products in any order: |dw - dw64| <= (K + 4) 2^-24 abs_sum."""
    r = _ratio((dw.double().reshape(ref.dw.shape) - ref.dw).abs(), (case.K + 4) * U * ref.abs_sum)
    assert r <= 1.0, f"{case.id} {what}: |dw - dw64| reaches {r:.3g} x the bound (K + 4) 2^-24 abs_sum"
    return r


def check_db(case: Case, ref, db: torch.Tensor, what="") -> float:
    r = _ratio((db.double() - ref.db).abs(), (case.K + 4) * U * ref.abs_db)
    assert r <= 1.0, f"{case.id} {what}: |db - db64| reaches {r:.3g} x the bound (K + 4) 2^-24 sum |dY|"
    return r


def check_rms(case: Case, ref, dw: torch.Tensor, what="") -> float:
    """rms(dw - dw64) <= (0.5 sqrt(K) + 2) 2^-24 rms(dw64): the statistical bound of tests/conv_contract.py, K = B H W."""
    e = (dw.double().reshape(ref.dw.shape) - ref.dw).pow(2).mean().sqrt().item()
    bound = (0.5 * math.sqrt(case.K) + 2.0) * U * ref.dw.pow(2).mean().sqrt().item()
    assert e <= bound, f"{case.id} {what}: rms error {e:.3e} above (0.5 sqrt(K) + 2) 2^-24 rms(dw64) = {bound:.3e}"
    return e / bound


# ------------------------------------------------------------------------------------------------ the device side
def _round4(v: int) -> int:
    return (v + 3) // 4 * 4


def to_planes(x: torch.Tensor) -> torch.Tensor:
    """[..., C] fp32 (C % 8 == 0) -> the bf16x3 plane layout [..., C / 8, 3, 8] as int16: the exact truncation split
    hi + mid + lo of every value (hi = the upper 16 bits, mid = the upper 16 bits of x - hi, lo likewise)."""
    def top(f):
        return (f.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = top(x)
    r1 = x - hi
    mid = top(r1)
    lo = top(r1 - mid)
    g = [(v.contiguous().view(torch.int32) >> 16).to(torch.int16).reshape(*x.shape[:-1], x.shape[-1] // 8, 8) for v in (hi, mid, lo)]
    return torch.stack(g, -2)


class Built:
    """A case on a device: ``x`` (one ops.View per segment; ops.View3 under ``plane``) and ``dy``, each a window at a
    channel offset that is a multiple of 4 of its own NaN-filled buffer (no two with the same pixel stride) with a spare
    NaN image behind the last; ``outputs()`` = fresh flat dw / db buffers; ``problem()`` = the vam_wgrad of one segment.
    Works on the CPU as well (for vam_conv_wgrad_plan / vam_conv_wgrad_route, which only do arithmetic)."""

    def __init__(self, case: Case, device, t: Optional[dict] = None):
        self.case, self.device, self.t = case, device, t or tensors(case)
        self._lds = set()
        self.x = [self._window(v, 4 if i % 2 == 0 else 8) for i, v in enumerate(self.t["segs"])]
        self.dy = self._window(self.t["dy"], 8)
        self.x3 = [self._planes(v) for v in self.t["segs"]] if case.plane else None     # (the fp32 windows exist as well)

    def _ld(self, least: int) -> int:
        ld = _round4(least)
        while ld in self._lds:
            ld += 4
        self._lds.add(ld)
        return ld

    def _window(self, nchw: torch.Tensor, off: int):
        from vampic import ops
        B, C, H, W = nchw.shape
        buf = torch.full((B + 1, H, W, self._ld(C + off + 4)), float("nan"), dtype=torch.float32, device=self.device)
        buf[:B, :, :, off:off + C] = nchw.permute(0, 2, 3, 1).to(self.device)
        return ops.View(buf[:B], off, C)

    def _planes(self, nchw: torch.Tensor):
        from vampic import ops
        B, C, H, W = nchw.shape
        G = C // 8
        raw = torch.full((B + 1, H, W, G + 2, 3, 8), 0x7FC0, dtype=torch.int16)               # bf16 NaN in every plane
        raw[:B, :, :, 1:1 + G] = to_planes(nchw.permute(0, 2, 3, 1).contiguous())
        buf = raw.reshape(B + 1, H, W, (G + 2) * 24).view(torch.float32).to(self.device)       # 12 floats per group
        return ops.View3(buf[:B], 1, C)

    def outputs(self, fill: float = SENTINEL):
        c = self.case
        dwbuf = torch.full((GUARD + c.n * c.cin * c.taps + GUARD,), fill, dtype=torch.float32, device=self.device)
        dbbuf = torch.full((GUARD + c.n + GUARD,), fill, dtype=torch.float32, device=self.device)
        return dwbuf, dbbuf

    def dw_view(self, dwbuf: torch.Tensor) -> torch.Tensor:
        c = self.case
        flat = dwbuf[GUARD:GUARD + c.n * c.cin * c.taps]
        return flat.view(c.n, c.cin) if c.dw2d else flat.view(c.n, c.cin, c.k, c.k)

    def problem(self, seg: int, dwbuf: torch.Tensor, dbbuf: Optional[torch.Tensor], splits: Optional[int] = None,
                plane: Optional[bool] = None):
        """The vam_wgrad of segment ``seg`` writing into the flat buffers (``dbbuf`` None: no db pointer).  ``splits``
        None: the case's forced value, or vam_conv_wgrad_plan's for the problem alone.  ``plane`` False: a plane case's
        problem on the fp32 windows of the same values.  A split problem gets a NaN-filled
        workspace of S (N C taps + N) floats with GUARD sentinel elements behind it (``p._ws``)."""
        from vampic import _lib as L
        c = self.case
        plane = c.plane if plane is None else plane
        v = (self.x3 if plane else self.x)[seg]
        p = L.VamWgrad()
        p.x, p.dy, p.dw = v.ptr, self.dy.ptr, dwbuf.data_ptr() + 4 * GUARD
        p.db = dbbuf.data_ptr() + 4 * GUARD if dbbuf is not None else None
        p.ld_x, p.ld_dy, p.B, p.H, p.W, p.kh, p.kw, p.C, p.N = v.ld, self.dy.ld, c.B, c.H, c.W, c.k, c.k, v.C, c.n
        p.cin_total, p.c_off = c.cin, c.c_offs[seg]
        p.stride, p.Hx, p.Wx = c.stride, c.Hx, c.Wx
        p.flags = L.WGRAD_X_P3 if plane else 0
        p.slot_share = 0.0
        if splits is None:
            splits = c.splits
        if splits is None:
            splits = L.load().vam_conv_wgrad_plan(ctypes.byref(p), None)
        p.splits = splits
        p._ws = None
        if splits > 1:
            n_ws = splits * (c.n * v.C * c.taps + c.n)
            p._ws = torch.full((n_ws + GUARD,), float("nan"), dtype=torch.float32, device=self.device)
            p._ws[n_ws:] = SENTINEL
            p.workspace = p._ws.data_ptr()
        p._dev = self.device
        p._keep = (v, self.dy, dwbuf, dbbuf)
        return p

    def route(self, seg: int = 0) -> tuple:
        """vam_conv_wgrad_route of one segment's problem: (kernel name, pipe, wn, wc, tn, tc, kp, plane)."""
        from vampic import _lib as L
        dwbuf, dbbuf = self.outputs()
        out = (ctypes.c_int * 8)()
        p = self.problem(seg, dwbuf, dbbuf, splits=1)
        assert L.load().vam_conv_wgrad_route(ctypes.byref(p), out) == 0
        return (KERNELS[out[0]],) + tuple(out[1:])

    def read(self, dwbuf: torch.Tensor, dbbuf: torch.Tensor, segs, db_owned: bool):
        """From the flat buffers (any device): dw [n, cin, k, k] and db [n] on the CPU, and how many elements outside the
        columns [c_off, c_off + C) of the segments ``segs`` (guards and foreign columns; all of db's buffer unless
        ``db_owned``, else its guards) no longer hold the sentinel's bits."""
        c = self.case
        dwbuf, dbbuf = dwbuf.cpu(), dbbuf.cpu()
        sent = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
        owned = torch.zeros((c.n, c.cin, c.taps), dtype=torch.bool)
        for s in segs:
            owned[:, c.c_offs[s]:c.c_offs[s] + c.segs[s]] = True
        own = torch.zeros(dwbuf.shape, dtype=torch.bool)
        own[GUARD:GUARD + owned.numel()] = owned.reshape(-1)
        stray = int((dwbuf.view(torch.int32)[~own] != sent).sum())
        ownb = torch.zeros(dbbuf.shape, dtype=torch.bool)
        if db_owned:
            ownb[GUARD:GUARD + c.n] = True
        stray += int((dbbuf.view(torch.int32)[~ownb] != sent).sum())
        dw = dwbuf[GUARD:GUARD + owned.numel()].reshape(c.n, c.cin, c.k, c.k).clone()
        return dw, dbbuf[GUARD:GUARD + c.n].clone(), stray


def ws_stray(p) -> int:
    """Elements of the sentinel guard behind a problem's workspace that were overwritten."""
    if p._ws is None:
        return 0
    sent = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
    return int((p._ws[-GUARD:].cpu().view(torch.int32) != sent).sum())


def build(case: Case, device, t: Optional[dict] = None) -> Built:
    return Built(case, device, t)
