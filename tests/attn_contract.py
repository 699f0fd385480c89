"""The window-attention contract of include/vampic.h (vam_win_attention, vam_win_attention_bwd), stated as a float64
reference, a table of small cases and the bounds an fp32 implementation has to meet.

    S = (q hd^-0.5) k^T + bias + mask ;  P = softmax(S) ;  O = P v        per (image, window, head), written back at the
                                                                          pixel the token came from
    dP = dO v^T ;  r = sum_u P dP ;  dS = P (dP - r)
    dq = scale dS k ;  dk = dS^T (q scale) ;  dv = P^T dO ;  dtable[ridx(i, u)][head] = sum over images, windows, pairs of dS

``reference(case)`` evaluates these lines in float64 on the CPU from the fp32 inputs, with nothing of the library in it and
in the reference model's own formulation: torch.roll, reshape / permute for the window partition, the relative-position
index from a meshgrid of coordinates, the 0 / -100 mask from a region image cut into windows.  The kernels fold all of that
into index arithmetic; a shared mistake there cannot agree with this file.  The backward is closed-form (no autograd), so
that every intermediate is at hand for the bounds.  ``build(case, device)`` puts the same problem on the device, every
tensor a channel window of its own wider buffer: NaN around what may be read, a sentinel around what may be written.

Helper module (not collected), in the manner of tests/conv_contract.py."""
from __future__ import annotations

from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Dict, Optional

import torch

import vampic.synth

U = 2.0 ** -24                    # unit roundoff of fp32
ETA = 2.0 ** -120                 # floor for probabilities of masked keys that an fp32 exp flushes to zero
SENTINEL = -777.25                # what every output buffer holds before a launch (exact in fp32)
GUARD = 4                         # guard channels either side of a window, guard rows either side of dtable
WRONG = ("roll+1", "ridx^T", "region-1", "hard mask", "no scale", "table[head][ridx]", "dk<->dq")


@dataclass(frozen=True)
class Case:
    id: str
    ws: int
    hd: int
    H: int
    W: int
    shift: int
    B: int = 2
    heads: int = 8
    qk: float = 1.0               # q and k are multiplied by this (strong logits: a masked key still carries weight)
    backward: bool = True         # False: the library has a forward kernel only for this (ws, hd)

    def __post_init__(self):
        assert self.ws in (4, 8) and self.H % self.ws == 0 and self.W % self.ws == 0 and 0 <= self.shift < self.ws
        assert self.heads % (64 // self.N) == 0 and self.hd % 4 == 0

    @property
    def C(self): return self.heads * self.hd
    @property
    def N(self): return self.ws * self.ws
    @property
    def NT(self): return (2 * self.ws - 1) ** 2
    @property
    def nW(self): return (self.H // self.ws) * (self.W // self.ws)
    @property
    def scale(self): return self.hd ** -0.5


def _table():
    c = [
        Case("a", 8, 24, 16, 24, 4),
        Case("b", 8, 24, 8, 16, 4, qk=6.0),
        Case("c", 8, 24, 16, 16, 0),
        Case("d", 8, 24, 16, 8, 7, qk=6.0),
        Case("e", 8, 24, 8, 8, 1, B=3, heads=4),
        Case("f", 8, 24, 8, 8, 4, qk=30.0),
        Case("g", 4, 40, 8, 12, 2),
        Case("h", 4, 40, 4, 4, 0, B=1),
        Case("i", 4, 40, 8, 8, 2, heads=4),
        Case("j", 4, 80, 4, 8, 2, qk=3.0),
        Case("k", 8, 40, 8, 8, 1, backward=False),
        Case("l", 4, 24, 8, 8, 3, heads=12, backward=False),
    ]
    return {k.id: k for k in c}


CASES: Dict[str, Case] = _table()
FORWARD_PAIRS = ((8, 24), (4, 40), (8, 40), (4, 24), (4, 80))     # (ws, hd) the forward dispatcher names
BACKWARD_PAIRS = ((8, 24), (4, 40), (4, 80))                      # ... and the backward dispatcher
QUANTITIES = ("out", "dq", "dk", "dv", "dtable")


# ------------------------------------------------------------------------------------------------ inputs
def tensors(case: Case) -> dict:
    """The fp32 CPU inputs of a case: ``qkv`` [B, H, W, 3C] (q | k | v, heads contiguous inside each), ``dout`` [B, H, W, C]
    and ``table`` [(2ws-1)^2, heads].  Fixed seeds, host-independent."""
    seed = 100 * (1 + list(CASES).index(case.id) if case.id in CASES else 77)
    nrm = vampic.synth.normal
    qkv = nrm((case.B, case.H, case.W, 3 * case.C), seed).clone()
    qkv[..., :2 * case.C] *= case.qk
    return {"qkv": qkv, "dout": nrm((case.B, case.H, case.W, case.C), seed + 1), "table": nrm((case.NT, case.heads), seed + 2, 0.5)}


# ------------------------------------------------------------------------------------------------ the formula
def partition(t: torch.Tensor, ws: int, shift: int) -> torch.Tensor:
    """[B, H, W, X] -> [B, windows, ws*ws, X]: cyclic shift by -shift, then cut into windows."""
    if shift > 0:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    B, H, W, X = t.shape
    return t.reshape(B, H // ws, ws, W // ws, ws, X).permute(0, 1, 3, 2, 4, 5).reshape(B, -1, ws * ws, X)


def reverse(w: torch.Tensor, H: int, W: int, ws: int, shift: int) -> torch.Tensor:
    """The inverse of ``partition``."""
    B, X = w.shape[0], w.shape[-1]
    t = w.reshape(B, H // ws, W // ws, ws, ws, X).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, X)
    if shift > 0:
        t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
    return t


def relative_position_index(ws: int) -> torch.Tensor:
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij"))      # [2, ws, ws]
    flat = coords.flatten(1)                                                                      # [2, N]
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()                     # [N, N, 2]
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)                                                                            # [N, N]


def shift_mask(H: int, W: int, ws: int, shift: int, hard: bool = False, moved: int = 0) -> torch.Tensor:
    """[windows, N, N] float64: 0 where query and key lie in the same region of the shifted image, -100 elsewhere.
    ``hard`` / ``moved`` are the wrong variants of the CPU test (-inf; the last row boundary one row early)."""
    img = torch.zeros((1, H, W, 1), dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift - moved), slice(-shift - moved, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = partition(img, ws, 0)[0, :, :, 0]                                                        # [windows, N]
    diff = mw[:, None, :] - mw[:, :, None]
    return torch.zeros_like(diff).masked_fill(diff != 0, float("-inf") if hard else -100.0)


def _heads(w: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, windows, N, heads*hd] -> [B, windows, heads, N, hd]"""
    B, nW, N, C = w.shape
    return w.reshape(B, nW, N, heads, C // heads).permute(0, 1, 3, 2, 4)


def _merge(w: torch.Tensor) -> torch.Tensor:
    B, nW, heads, N, hd = w.shape
    return w.permute(0, 1, 3, 2, 4).reshape(B, nW, N, heads * hd)


def _gather_bias(case: Case, table: torch.Tensor, idx: torch.Tensor, by_head: bool) -> torch.Tensor:
    N = case.N
    if by_head:                                       # wrong variant: the table read as [heads][NT]
        return table.reshape(-1).reshape(case.heads, case.NT)[:, idx.reshape(-1)].reshape(case.heads, N, N)
    return table[idx.reshape(-1)].reshape(N, N, case.heads).permute(2, 0, 1)


def _scatter_bias(case: Case, per_pair: torch.Tensor, idx: torch.Tensor, by_head: bool) -> torch.Tensor:
    """[heads, N, N] -> [NT, heads]: the sum of the pairs of every table entry."""
    flat = per_pair.reshape(case.heads, case.N * case.N)
    g = torch.zeros((case.heads, case.NT), dtype=per_pair.dtype).index_add_(1, idx.reshape(-1), flat)
    return g.reshape(-1).reshape(case.NT, case.heads) if by_head else g.t().contiguous()


def evaluate(case: Case, t: Optional[dict] = None, dtype=torch.float64, wrong: Optional[str] = None, backward: bool = True,
             qkv: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None) -> SimpleNamespace:
    """The contract in ``dtype``.  Returns out [B, H, W, C], dqkv [B, H, W, 3C], dtable [NT, heads] and every intermediate
    in window layout [B, windows, heads, N, ...].  ``wrong`` names one of WRONG: a deliberately wrong formula for the CPU
    test.  ``qkv`` / ``table`` replace the case's inputs (tensors that require grad: the forward is differentiable)."""
    assert wrong is None or wrong in WRONG
    t = t or tensors(case)
    ws, N, C, H, W = case.ws, case.N, case.C, case.H, case.W
    qkv = t["qkv"].to(dtype) if qkv is None else qkv
    table = t["table"].to(dtype) if table is None else table
    roll = case.shift + 1 if wrong == "roll+1" else case.shift
    scale = 1.0 if wrong == "no scale" else case.scale
    by_head = wrong == "table[head][ridx]"
    idx = relative_position_index(ws)
    if wrong == "ridx^T":
        idx = idx.t().contiguous()

    win = partition(qkv, ws, roll)
    q, k, v = (_heads(win[..., i * C:(i + 1) * C], case.heads) for i in range(3))
    qs = q * scale
    bias = _gather_bias(case, table, idx, by_head)                                # [heads, N, N]
    mask = torch.zeros((case.nW, N, N), dtype=dtype)
    if case.shift > 0:
        mask = shift_mask(H, W, ws, case.shift, hard=wrong == "hard mask", moved=1 if wrong == "region-1" else 0).to(dtype)
    s = qs @ k.transpose(-2, -1) + bias[None, None] + mask[None, :, None]
    p = torch.softmax(s, dim=-1)
    o = p @ v
    r = SimpleNamespace(case=case, qs=qs, k=k, v=v, bias=bias, mask=mask, s=s, p=p, o=o, idx=idx, scale=scale,
                        out=reverse(_merge(o), H, W, ws, roll), dqkv=None, dtable=None)
    if not backward:
        return r
    dO = _heads(partition(t["dout"].to(dtype), ws, roll), case.heads)
    dP = dO @ v.transpose(-2, -1)
    rs = (p * dP).sum(-1, keepdim=True)
    dS = p * (dP - rs)
    dq = scale * (dS @ k)
    dk = dS.transpose(-2, -1) @ qs
    dv = p.transpose(-2, -1) @ dO
    if wrong == "dk<->dq":
        dq, dk = dk, dq
    r.dO, r.dP, r.rs, r.dS = dO, dP, rs, dS
    r.dqkv = reverse(torch.cat([_merge(dq), _merge(dk), _merge(dv)], -1), H, W, ws, roll)
    r.dtable = _scatter_bias(case, dS.sum((0, 1)), idx, by_head)
    return r


def reference(case: Case, t: Optional[dict] = None) -> SimpleNamespace:
    return evaluate(case, t, torch.float64, backward=case.backward)


# ------------------------------------------------------------------------------------------------ bounds
def bounds(case: Case, ref) -> Dict[str, torch.Tensor]:
    """Elementwise error bounds of an fp32 evaluation, from the float64 intermediates (U = 2^-24, N = ws^2):

        A   = |q scale| |k|^T + |bias| + |mask|                   magnitude of a logit's terms
        ds  = (hd + 3) U A                                        a logit: hd products and the two additions
        w   = ds + sum_u p ds + (8 + 2 |s - max_u s|) U + (N + 4) U        relative error of P: the logit's error in and out
                                                                  of the normaliser, exp and its argument, the sum, the divide
        out : (p w) |v|
        dPa = |dO| |v|^T ;  edP = (hd + 2) U dPa ;  ra = sum_u p dPa
        er  = sum_u p (w dPa + edP) + (N + 2) U ra
        dSa = p (dPa + ra)
        eS  = p (w (dPa + ra) + edP + er) + 2 U dSa + ETA (dPa + ra)
        dq  : scale (eS |k| + (N + 3) U dSa |k|)
        dk  : eS^T |q scale| + (N + 3) U dSa^T |q scale|
        dv  : (p w + ETA)^T |dO| + (N + 2) U p^T |dO|
        dtable : scatter-sum(eS) + (n_terms + 2) U scatter-sum(dSa),  n_terms = windows * images * N

    out, dq, dk, dv come back at [B, H, W, C], dtable at [NT, heads]."""
    N, hd, H, W, ws, sh = case.N, case.hd, case.H, case.W, case.ws, case.shift
    p, s = ref.p, ref.s
    ka, va, qa = ref.k.abs(), ref.v.abs(), ref.qs.abs()
    A = qa @ ka.transpose(-2, -1) + ref.bias.abs()[None, None] + ref.mask.abs()[None, :, None]
    ds = (hd + 3) * U * A
    w = ds + (p * ds).sum(-1, keepdim=True) + (8 + 2 * (s - s.max(-1, keepdim=True).values).abs()) * U + (N + 4) * U
    back = lambda x: reverse(_merge(x), H, W, ws, sh)
    b = {"out": back((p * w) @ va)}
    if ref.dqkv is None:
        return b
    dOa = ref.dO.abs()
    dPa = dOa @ va.transpose(-2, -1)
    edP = (hd + 2) * U * dPa
    ra = (p * dPa).sum(-1, keepdim=True)
    er = (p * (w * dPa + edP)).sum(-1, keepdim=True) + (N + 2) * U * ra
    dSa = p * (dPa + ra)
    eS = p * (w * (dPa + ra) + edP + er) + 2 * U * dSa + ETA * (dPa + ra)
    b["dq"] = back(case.scale * (eS @ ka + (N + 3) * U * (dSa @ ka)))
    b["dk"] = back(eS.transpose(-2, -1) @ qa + (N + 3) * U * (dSa.transpose(-2, -1) @ qa))
    b["dv"] = back((p * w + ETA).transpose(-2, -1) @ dOa + (N + 2) * U * (p.transpose(-2, -1) @ dOa))
    n_terms = case.nW * case.B * N
    b["dtable"] = _scatter_bias(case, eS.sum((0, 1)), ref.idx, False) + (n_terms + 2) * U * _scatter_bias(case, dSa.sum((0, 1)), ref.idx, False)
    return b


def split(case: Case, out=None, dqkv=None, dtable=None) -> Dict[str, torch.Tensor]:
    """The five quantities by name, from what a launch (or ``evaluate``) returns."""
    C, d = case.C, {}
    if out is not None:
        d["out"] = out
    if dqkv is not None:
        d.update(dq=dqkv[..., :C], dk=dqkv[..., C:2 * C], dv=dqkv[..., 2 * C:3 * C])
    if dtable is not None:
        d["dtable"] = dtable
    return d


def _ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want| / bound; inf when an element is not finite, or differs where the bound is zero."""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got.double() - want).abs()
    inf = torch.full_like(err, float("inf"))
    return float(torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), inf)).max())


def ratios(case: Case, ref, got: Dict[str, torch.Tensor], bnd: Optional[dict] = None) -> Dict[str, float]:
    """error / bound of every quantity in ``got`` (see ``split``), largest element."""
    bnd = bnd or bounds(case, ref)
    want = split(case, ref.out, ref.dqkv, ref.dtable)
    return {k: _ratio(v, want[k], bnd[k]) for k, v in got.items()}


def check(case: Case, ref, got: Dict[str, torch.Tensor], what: str = "", bnd: Optional[dict] = None) -> Dict[str, float]:
    r = ratios(case, ref, got, bnd)
    for k, v in r.items():
        assert v <= 1.0, f"{case.id} {what}: |{k} - {k}64| reaches {v:.3g} x its bound"
    return r


# ------------------------------------------------------------------------------------------------ the GPU side
_SENT_BITS = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)


def stray(buf: torch.Tensor, owned: torch.Tensor) -> int:
    """How many elements of a (CPU) buffer outside ``owned`` no longer hold the sentinel's bits."""
    return int((buf.view(torch.int32)[~owned] != _SENT_BITS).sum())


class Built:
    """A case on the device.  Inputs: ``qkv`` and ``dout`` are channel windows at offset 4 of NaN-filled buffers with
    ld = 3C + 8 / C + 8, ``table`` the middle rows of a NaN-filled buffer.  ``forward()`` / ``backward()`` make fresh
    sentinel-filled outputs (guard channels either side, one spare image, guard rows around dtable, a sentinel tail on the
    NaN-filled workspace), launch through ``ops`` and return what was written with the count of stray writes."""

    def __init__(self, case: Case, device, t: Optional[dict] = None):
        from vampic import ops
        self.case, self.device, self.t = case, device, t or tensors(case)
        self.qkv = self._in(self.t["qkv"])
        self.dout = self._in(self.t["dout"])
        tb = torch.full((case.NT + 2 * GUARD, case.heads), float("nan"), dtype=torch.float32, device=device)
        tb[GUARD:GUARD + case.NT] = self.t["table"].to(device)
        self._table_buf, self.table = tb, tb[GUARD:GUARD + case.NT]
        self._ops = ops

    def _in(self, nhwc: torch.Tensor):
        from vampic import ops
        B, H, W, C = nhwc.shape
        buf = torch.full((B, H, W, C + 2 * GUARD), float("nan"), dtype=torch.float32, device=self.device)
        buf[..., GUARD:GUARD + C] = nhwc.to(self.device)
        return ops.View(buf, GUARD, C)

    def _out(self, C: int):
        c = self.case
        buf = torch.full((c.B + 1, c.H, c.W, C + 2 * GUARD), SENTINEL, dtype=torch.float32, device=self.device)
        return buf, self._ops.View(buf[:c.B], GUARD, C)

    def _read(self, buf: torch.Tensor, C: int):
        c = self.case
        buf = buf.cpu()
        owned = torch.zeros(buf.shape, dtype=torch.bool)
        owned[:c.B, :, :, GUARD:GUARD + C] = True
        return buf[:c.B, :, :, GUARD:GUARD + C].contiguous(), stray(buf, owned)

    def forward(self):
        """(out [B, H, W, C] on the CPU, stray elements of its buffer)"""
        c = self.case
        buf, view = self._out(c.C)
        self._ops.win_attention(self.qkv, view, self.table, c.C, c.heads, c.ws, c.shift)
        torch.cuda.synchronize()
        return self._read(buf, c.C)

    def backward(self, dtable_fill: float = SENTINEL):
        """(dqkv [B, H, W, 3C], dtable [NT, heads], stray elements of the dqkv buffer, of the rows around dtable, of the
        workspace tail).  ``dtable_fill``: what dtable's own rows hold before the launch."""
        from vampic import _lib as L
        c = self.case
        buf, view = self._out(3 * c.C)
        dtb = torch.full((c.NT + 2 * GUARD, c.heads), SENTINEL, dtype=torch.float32, device=self.device)
        dtable = dtb[GUARD:GUARD + c.NT]
        dtable.fill_(dtable_fill)
        n = L.load().vam_win_attention_bwd_workspace(c.B, c.H, c.W, c.heads, c.ws) // 4
        wsp = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=self.device)
        wsp[n:] = SENTINEL
        self._ops.win_attention_bwd(self.qkv, self.dout, view, self.table, dtable, c.C, c.heads, c.ws, c.shift, workspace=wsp)
        torch.cuda.synchronize()
        dqkv, s_dq = self._read(buf, 3 * c.C)
        dtb = dtb.cpu()
        rows = torch.zeros(dtb.shape, dtype=torch.bool)
        rows[GUARD:GUARD + c.NT] = True
        return dqkv, dtb[GUARD:GUARD + c.NT].contiguous(), s_dq, stray(dtb, rows), stray(wsp[n:].cpu(), torch.zeros(64, dtype=torch.bool))


def build(case: Case, device, t: Optional[dict] = None) -> Built:
    return Built(case, device, t)


def image0(case: Case, t: dict):
    """The case and inputs of image 0 alone."""
    return replace(case, id=case.id + "[0]", B=1), {"qkv": t["qkv"][:1].clone(), "dout": t["dout"][:1].clone(), "table": t["table"]}


def window_pixels(case: Case, window: int) -> torch.Tensor:
    """The (y, x) pixels of one window, by the roll arithmetic of the reference: an image of pixel numbers, partitioned."""
    ids = torch.arange(case.H * case.W).reshape(1, case.H, case.W, 1)
    flat = partition(ids, case.ws, case.shift)[0, window, :, 0]
    return torch.stack([flat // case.W, flat % case.W], 1)
