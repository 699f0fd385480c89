"""The contract of the inference likelihood and rate kernels in float64.  TEST HELPER (torch and numpy on the CPU).

Kernels (csrc/entropy.hip): ``gauss_tail_kernel``, ``gauss_levels_eval_kernel``, ``gauss_levels_decode_kernel``,
``gauss_layer_bits_kernel``, ``build_indexes_kernel`` and the evaluation path of ``eb_forward_kernel``.

The machinery is the training contract's (tests/train_ew_contract.py): every chain is ONE body in the kernel's order of
operations over a ``Tape`` (the library is built with -ffp-contract=off), run as float64 (the reference), as float32,
as emulated float32 ("f32e": every + - * / correctly rounded) and as a rounding budget A delivered by autograd.  What is
different here is what the training chains do not have: rounding instead of noise, integer symbols, the unmasked
branch's own |v|, and float64 sums.

EXACT outputs — yhat, zhat, the symbols, the table indexes, the decoded yhat — are made of + - *, rint, comparisons and
int conversions only: they must equal the emulated float32 chain in bits.  The float64 body takes every decision (rint,
``<=`` against the scale table, ``layer <= k``) from those same fp32 values, because fp32 computes them exactly; so does
|v| of the unmasked branch, |fl(fl(q + mu) - mu)|, a value of two exact operations that need not be an integer — that is
what keeps the masked and the unmasked branch two different statements in float64, where q + mu - mu is just q.

BUDGETED outputs — the likelihoods — must meet |got - ref64| <= K 2^-24 A + 2^-126, K = max(4 K_cpu, 8), K_cpu measured
on this contract's inputs with the float32 body against the float64 one, never from a GPU.  A counts every rounded
operation of the chain; the inputs are fp32 numbers as they stand and carry no rounding of their own.  Whenever a
likelihood is judged, the same statement is judged in the unit the codec uses:
|log2 got - log2 ref64| <= (K 2^-24 A + 2^-126) / (ref64 ln 2) (1 + 2^-10).  The 1e-9 decision splits the elements as in
the training contract: clear-above (float64 value > 2e-9), clear-below (< 0.5e-9: exactly 1e-9f) and in-band ones, which
may take either branch and are judged against the nearer one.

Float64 SUMS (log2sum, bits) are held twice: to the float64 sum of log2 of the launch's own fp32 likelihoods within
1e-12 of sum |term| (the figure of tests/test_gpu_rate_control.py), and to the sum of log2 of the float64 likelihoods
within the sum of the per-element bounds in bits.  Counts are exact.

Inputs: y, y2 and mu normal (scales 4, 2, 2), sigma log-uniform in [0.03, 64], binary masks, and the placed points of
``_draw_tail`` / ``_draw_eb``.  At those scales a third of the plain draws would lie below the likelihood bound; so that
the either-or rule of the band stays the exception (at most 1 % of a case in or below the band), an unplaced element in or
below the band is pulled towards the mode — |d| halved until it is clear above — which leaves tail elements of every
size above 2e-9 in place.  In-band points are placed in the cases marked ``band`` only; the others check their sums
against float64 and hold none.

Domain: finite inputs with |y - y2 - mu| < 2^24.  NaN scales and saturating int conversions are outside this contract.
(For the record: the kernels' ``fmaxf`` sends a NaN scale to the 0.11 bound and to index 0, the oracle's ``clamp_min``
keeps the NaN and ends at the last index.  Nothing here tests that.)"""
import dataclasses
import functools
import math

import numpy as np
import torch

import train_ew_contract as TC
from train_ew_contract import (Tape, Ref, _phi_cdf, _solve_av, eb_split, _eb_net, _eb_fwd, bits, BOUND_S, BOUND_L, BAND,  # noqa: F401
                               K_FLOOR, K_FACTOR, FLOOR, SENTINEL_BITS)

F32 = np.float32
U24 = TC.U24
LN2 = math.log(2.0)
SUM_RTOL = 1e-12                         # float64 sums against the sum of their own terms (tests/test_gpu_rate_control.py)
BITS_SLACK = 1.0 + 2.0 ** -10            # |ln(1 + x)| <= |x| (1 + 2^-10) for |x| <= 2^-9
MAX_MASK_LEVELS = 8                      # include/vampic.h (asserted against the library by the GPU test)
MAX_LAYER_LEVELS = 32
LAYER_NONE = 0xFF
GRID = 1024.0                            # placed points live on a 2^-10 grid: both subtractions of d are exact


# ====================================================================================================== bodies
def _const(T, a):
    """an input: the fp32 numbers as they stand (no rounding mark)"""
    t = torch.tensor(np.ascontiguousarray(a), dtype=T.dtype)
    return TC.V(t) if T.mode == "run" else t


def _rint(t, mut):
    if "half_away" in mut:
        return torch.sign(t) * torch.floor(t.abs() + 0.5)
    return torch.round(t)                                          # half to even, as rintf


def _phi(T, t, mut):
    if "erfc_const" in mut:
        return 0.5 * T.r(torch.erfc(T.r(-0.7071 * t, 2)))
    return _phi_cdf(T, t)


def _gauss_lik(T, absv, s, mut=()):
    """gauss_lik(): (bounded, raw) of max(Phi((.5 - |v|) / max(s, .11f)) - Phi((-.5 - |v|) / max(s, .11f)), 1e-9f)"""
    r = T.r
    sb = s if "no_scale_bound" in mut or "scale_bound_before_mask" in mut else torch.clamp_min(s, BOUND_S)
    u, l = r(r(0.5 - absv) / sb), r(r(-0.5 - absv) / sb)
    raw = r(_phi(T, u, mut) - _phi(T, l, mut))
    if "bits_scale" in mut:                                        # (before the bound: 1e-9f itself stays what it is)
        raw = torch.where(raw < 1e-4, raw * (1.0 + 3e-5), raw)
    lik = torch.clamp_min(raw, 1e-8 if "lik_bound_1e-8" in mut else BOUND_L)
    return lik, raw


def _tail(T, I, masked, mut, dec):
    r = T.r
    J = {k: _const(T, v) for k, v in I.items() if k in ("y", "y2", "mu", "sigma") or (masked and k == "mask")}
    d = r(J["y"] - J["y2"]) if "y2" in J else J["y"]
    d = r(d - J["mu"])
    q = _rint(d, mut) if dec is None else dec["q"]
    mu, sg = J["mu"], J["sigma"]
    if masked:
        m = J["mask"]
        rq = _rint(r(d * m), mut) if dec is None else dec["rq"]
        absv = q.abs().expand_as(rq) if "absv_before_mask" in mut else rq.abs()
        if "scale_bound_before_mask" in mut:
            s = r(torch.clamp_min(sg, BOUND_S) * m)
        else:
            s = sg.expand_as(rq) if "s_sigma" in mut else r(sg * m)
        yhat, sym = r(r(q * m) + mu), rq
    else:
        o = r(q + mu)
        if "absq" in mut:
            absv = q.abs()
        else:
            absv = r(o - mu).abs() if dec is None else dec["absv"]
        s, yhat, sym = sg, o, q
    lik, raw = _gauss_lik(T, absv, s, mut)
    return {"yhat": yhat, "sym": sym, "lik": lik, "lik_raw": raw, "q": q, "rq": sym, "absv": absv, "d": d, "s": s}


def tail_body(T, I, masked, mut=()):
    """``gauss_tail``, each level of ``gauss_levels_eval`` (mask [L, Q]: outputs [L, Q]) and — mask of ones —
    ``gauss_layer_bits``.  I: fp32 arrays y, mu, sigma[, y2][, mask]."""
    dec = None
    if T.mode not in ("f32", "f32e"):
        o = _tail(Tape("f32e"), I, masked, mut, None)
        dec = {k: o[k].detach() for k in ("q", "rq", "absv")}
    return _tail(T, I, masked, mut, dec)


def decode_body(T, sym, layer, mu, ks):
    """``gauss_levels_decode``: yhat_l = float(sym) * (layer <= k_l) + mu, [L, Q]"""
    r = T.r
    q, mu = _const(T, np.asarray(sym, dtype=np.float64)), _const(T, mu)
    ly = torch.tensor(np.asarray(layer, dtype=np.int64))
    return torch.stack([r(r(q * (ly <= int(k)).to(T.dtype)) + mu) for k in ks])


def scale_table():
    import vampic_oracle as O
    return O.scale_table().numpy().astype(F32)


def index_body(T, sigma, mask, table, mut=()):
    """``build_indexes``: n_table - 1 - #{t < n_table - 1: max(sigma m, .11f) <= table[t]}"""
    s = _const(T, sigma)
    if mask is not None:
        s = T.r(s * _const(T, mask))
    v = torch.clamp_min(s, BOUND_S)
    tb = _const(T, table)
    cnt = torch.zeros(v.shape, dtype=torch.int64)
    for t in range(len(table) - 1):
        cnt += ((v < tb[t]) if "index_lt" in mut else (v <= tb[t])).to(torch.int64)
    return len(table) - 1 - cnt


def _eb(T, P, z, mut, dec):
    r = T.r
    C, N = z.shape
    net = _eb_net(T, P, N)
    med = _const(T, np.broadcast_to(P[14][:, (0 if "median_q0" in mut else 1):][:, :1], (C, N)))
    zz = _const(T, z)
    if dec is None:
        qz = _rint(r(zz - med), mut)
    else:
        qz = TC.V(dec["qz"]) if T.mode == "run" else dec["qz"]
    o = r(qz + med)
    lower = _eb_fwd(T, net, r(o - 0.5))[0]
    upper = _eb_fwd(T, net, r(o + 0.5))[0]
    s = r(lower + upper)
    if "no_sign_rule" in mut:
        sign = torch.ones((C, N), dtype=torch.float64 if T.mode == "run" else T.dtype)
    else:
        sign = TC._sel(s > 0.0, -1.0, TC._sel(s < 0.0, 1.0, 0.0, s), s)
        sign = sign.v if isinstance(sign, TC.V) else sign
    su, sl = TC._sigmoid_t(T, sign * upper), TC._sigmoid_t(T, sign * lower)
    raw = r(su - sl).abs()
    rv = raw.v if isinstance(raw, TC.V) else raw
    lik = TC._sel(rv >= BOUND_L, raw, BOUND_L, raw)
    return {"zhat": o, "sym": qz, "lik": lik, "lik_raw": raw, "qz": qz, "sum": s, "lower": lower, "upper": upper}


def eb_eval_body(T, P, z, mut=()):
    """the evaluation path of ``eb_forward_kernel``: P = eb_split(params, C), z [C, N] (channel-major).  ``eb_body`` of the
    training contract evaluates at z + noise; the evaluation point here is fl(rint(fl(z - med)) + med)."""
    dec = None
    if T.mode not in ("f32", "f32e"):
        o = _eb(Tape("f32e"), P, z, mut, None)
        dec = {"qz": o["qz"].detach()}
    return _eb(T, P, z, mut, dec)


# ====================================================================================================== cases
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    fam: str                 # tail | eb
    shape: tuple             # (B, H, W)
    C: int
    opt: tuple = ()

    def o(self, key, default=None):
        return dict(self.opt).get(key, default)

    @property
    def n_pix(self):
        return self.shape[0] * self.shape[1] * self.shape[2]


PATTERN = 4099
CASES = {c.id: c for c in (
    Case("t-min", "tail", (1, 1, 1), 4),
    Case("t-mixed", "tail", (5, 1, 3), 4),
    Case("t-ragged", "tail", (2, 5, 7), 36, (("band", True),)),
    Case("t-blocks", "tail", (3, 10, 7), 32),
    Case("t-levels", "tail", (2, 4, 6), 32, (("band", True),)),
    Case("t-stride", "tail", (1, 4099, 1), 512, (("tile", True),)),
    Case("t-opt", "tail", (2, 5, 7), 36),
    Case("e-small", "eb", (1, 1, 7), 5),
    Case("e-odd", "eb", (2, 1, 3), 130),
    Case("e-wide", "eb", (2, 1, 515), 192),
)}
LEVELS_OF = {"t-min": (1,), "t-mixed": (1,), "t-ragged": (2,), "t-blocks": (2,), "t-levels": (1, 3, MAX_MASK_LEVELS)}
LAYER_LEVELS_OF = {"t-min": (1,), "t-mixed": (2,), "t-ragged": (3,), "t-blocks": (3,), "t-levels": (1, 3, MAX_LAYER_LEVELS)}


def layout(case, k):
    """(ld, c0) of operand k: every operand its own pitch, windows off the buffer's start (multiples of 4); the bottleneck
    kernel reads scalars, any pitch"""
    if case.fam == "eb":
        return case.C + 3 + k, 0
    return case.C + 12 + 4 * k, 4 + 4 * (k % 2)


def n_unique(case):
    return PATTERN if case.o("tile") else case.n_pix * case.C


def expand(case, a):
    return TC.expand(case, a)


def _g(a):
    return F32(np.round(np.float64(a) * GRID) / GRID)


def _lik_at(av, s):
    s = max(s, BOUND_S)
    return 0.5 * (math.erfc(-TC.INV_SQRT2 * (0.5 - av) / s) - math.erfc(-TC.INV_SQRT2 * (-0.5 - av) / s))


def _sigma_for(av, target, lo=0.12, hi=60.0):
    """sigma with lik(|v| = av, sigma) = target on the tail side (the likelihood of a tail symbol grows with sigma there)"""
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if _lik_at(av, mid) < target else (lo, mid)
    return math.sqrt(lo * hi)


def _raw64(I, L):
    """float64 raw likelihoods [L + 1, Q]: the masked chain per level and the mask of ones / unmasked chain (the same value up
    to the unmasked |v|)"""
    T = Tape("f64")
    a = _tail(T, I, True, (), None)["lik_raw"].numpy()
    b = _tail(T, {**I, "mask": np.ones_like(I["sigma"])}, True, (), None)["lik_raw"].numpy()
    c = _tail(T, I, False, (), None)["lik_raw"].numpy()
    e = _tail(T, {k: v for k, v in I.items() if k != "y2"}, False, (), None)["lik_raw"].numpy()       # the launches without y2
    return np.concatenate([a.reshape(L, -1), b.reshape(1, -1), c.reshape(1, -1), e.reshape(1, -1)])


def _draw_tail(case):
    rng = np.random.RandomState(TC.hash_id("entropy " + case.id) % (2 ** 31))
    q, L = n_unique(case), MAX_MASK_LEVELS
    I = {"y": TC._normal(rng, q, 4.0), "y2": TC._normal(rng, q, 2.0), "mu": TC._normal(rng, q, 2.0),
         "sigma": np.exp(rng.uniform(math.log(0.03), math.log(64.0), q)).astype(F32),
         "mask": (rng.uniform(size=(L, q)) > 0.4).astype(F32)}
    # layer ids of the container: 0 .. 33 and 0xFF — whatever n_levels a launch names, ids 0, n_levels - 1, n_levels
    # (beyond the list) and 0xFF are all present once q is a few hundred (asserted by the CPU test for the cases that bin)
    layer = rng.randint(0, MAX_LAYER_LEVELS + 2, q).astype(np.uint8)
    small = rng.uniform(size=q) < 0.5
    layer[small] = rng.randint(0, 4, int(small.sum())).astype(np.uint8)
    layer[rng.uniform(size=q) < 0.15] = LAYER_NONE
    placed, todo = {}, []

    def point(name, fn):
        todo.append((name, fn))

    def setd(i, d, m=1.0, zero=False, y2=False):
        """y - y2 - mu == d exactly (d on the grid, or y2 = mu = 0).  y2 is 0 at a placed point, so that the launches without
        y2 meet the same d — but for the ties, which keep a small y2 on the grid (without it they are ordinary elements)"""
        if zero:
            I["y2"][i], I["mu"][i] = 0.0, 0.0
        else:
            I["y2"][i], I["mu"][i] = (_g(np.clip(I["y2"][i], -0.45, 0.45)) if y2 else 0.0), _g(np.clip(I["mu"][i], -8, 8))
        I["y"][i] = F32(np.float64(d) + np.float64(I["y2"][i]) + np.float64(I["mu"][i])) if not zero else F32(d)
        I["mask"][:, i] = m

    def sig(i, s):
        I["sigma"][i] = F32(s)

    for k in (0, 1, 2, 7, 1022):
        for sgn in (1.0, -1.0):
            point("tie", lambda i, k=k, sgn=sgn: (setd(i, sgn * (k + 0.5), y2=True), sig(i, max(0.3, 0.4 * k))))
    for sgn in (1.0, -1.0):
        for side in (np.inf, -np.inf):
            point("tie_ulp", lambda i, sgn=sgn, side=side: (setd(i, np.nextafter(F32(sgn * 2.5), F32(side)), zero=True), sig(i, 1.0)))
    for dd in (5.0, -5.0, 3.0, -3.0):
        point("half_mask", lambda i, dd=dd: (setd(i, dd, m=0.5), sig(i, 0.8)))
    for sgn in (1.0, -1.0):
        point("m0", lambda i, sgn=sgn: (setd(i, sgn * 3.25, m=0.0), sig(i, 0.7)))
    point("neg_zero", lambda i: (setd(i, -0.0, zero=True), sig(i, 0.5)))
    point("neg_zero", lambda i: (setd(i, 0.0, zero=True), I["mu"].__setitem__(i, F32(-0.0)), I["y"].__setitem__(i, F32(-0.0)), sig(i, 0.5)))
    b = F32(0.11)
    for dd in (0.25, -1.25):
        point("s_at", lambda i, dd=dd: (setd(i, dd), sig(i, b)))
        point("s_below", lambda i, dd=dd: (setd(i, dd), sig(i, np.nextafter(b, F32(0)))))
        point("s_half", lambda i, dd=dd: (setd(i, 2 * dd if dd > 0 else dd, m=0.5), sig(i, 0.15)))   # 0.5 (a tie) and -1.25: |q| <= 1
    point("s_m0", lambda i: (setd(i, 0.25, m=0.0), sig(i, 0.7)))
    for sgn in (1.0, -1.0):                                        # the unmasked branch: fl(fl(q + mu) - mu) != q
        def big_mu(i, sgn=sgn):
            m = F32(sgn * 1023.3)                                  # q + mu crosses into the next binade: odd last bits are rounded away
            while F32(F32(F32(sgn) + m) - m) == F32(sgn):
                m = np.nextafter(m, F32(0))
            I["y2"][i], I["mu"][i] = 0.0, m
            I["y"][i] = F32(np.float64(I["mu"][i]) + sgn * 1.2)
            I["mask"][:, i] = 1.0
            sig(i, 0.3)
        point("big_mu", big_mu)
    tb = scale_table()
    for t in (0, 1, 31, 62):
        for side in (0, 1, -1):
            point("table", lambda i, t=t, side=side: (I["mask"].__setitem__((slice(None), i), 1.0),
                                                        sig(i, tb[t] if side == 0 else np.nextafter(tb[t], F32(side * np.inf)))))
    point("table_edge", lambda i: (I["mask"].__setitem__((slice(None), i), 1.0), sig(i, np.nextafter(tb[-1], F32(np.inf)))))
    point("table_edge", lambda i: (I["mask"].__setitem__((slice(None), i), 1.0), sig(i, 0.05)))

    def aim(i, target, sgn, s0):
        av = float(round(_solve_av(s0, target)))
        setd(i, sgn * max(av, 2.0))
        sig(i, _sigma_for(max(av, 2.0), target))

    if q >= 1000:                                                  # (1 % of a smaller case is no element at all)
        if case.o("band"):
            for j, t in enumerate((0.6e-9, 0.9e-9, 1.0e-9, 1.1e-9, 1.8e-9)):
                point("band", lambda i, t=t, j=j: aim(i, t, 1.0 if j % 2 else -1.0, 0.4 + 0.25 * j))
        for j, t in enumerate((1e-10, 1e-10, 3e-10, 3e-10)):
            point("below", lambda i, t=t, j=j: aim(i, t, 1.0 if j % 2 else -1.0, 0.5 + 0.3 * j))
        for sgn in (1.0, -1.0):
            point("far_below", lambda i, sgn=sgn: (setd(i, sgn * 80.0), sig(i, 0.2)))
        # a likelihood just under 1e-4 with nothing but the tail in it: where a relative error of 3e-5 is 4e-5 bits
        for sgn in (1.0, -1.0):
            point("bits", lambda i, sgn=sgn: aim(i, 0.97e-4, sgn, 1.0))
    pos = rng.permutation(q).tolist()
    for name, fn in todo:
        if not pos:
            break
        i = pos.pop()
        fn(i)
        placed.setdefault(name, []).append(i)
    fixed = np.zeros(q, dtype=bool)
    fixed[[i for k, v in placed.items() if not k.startswith("table") for i in v]] = True       # (the table points place sigma only)
    # every unplaced element clear above the band: one in or below it is pulled towards the mode, |d| halved until it is clear
    for _ in range(40):
        lr = _raw64(I, L)
        stray = (lr <= BAND[1]).any(0) & ~fixed
        if not stray.any():
            break
        d = I["y"].astype(np.float64) - I["y2"] - I["mu"]
        I["y2"][stray] = (0.5 * I["y2"])[stray]                     # (y2 too: the launches without it see y - mu)
        I["y"][stray] = (I["mu"].astype(np.float64) + I["y2"] + 0.5 * d)[stray].astype(F32)
    lr = _raw64(I, L)
    for i in list(placed.get("band", [])):                          # a placed point must sit where it claims, on every chain that runs it
        assert ((lr[:, i] >= BAND[0]) & (lr[:, i] <= BAND[1])).all(), (case.id, i, lr[:, i])
    I["layer"] = layer
    return I, placed


def _draw_eb(case):
    rng = np.random.RandomState(TC.hash_id("entropy " + case.id) % (2 ** 31))
    C, N = case.C, case.n_pix
    P = []
    for i, shp in enumerate(TC.EB_SHAPES):
        n = shp[0] * shp[1]
        kind = i % 3 if i < 14 else 3
        if kind == 0:
            a = rng.standard_normal((C, n)) * 0.8 - 0.7           # a gain of about one: tails of a few units, as a trained prior's
        elif kind == 1:
            a = rng.uniform(-0.5, 0.5, (C, n))
        elif kind == 2:
            a = rng.standard_normal((C, n)) * 0.5
        else:
            a = np.stack([np.full(C, -10.0), np.round(rng.uniform(-2, 2, C) * GRID) / GRID, np.full(C, 10.0)], axis=1)
        P.append(a.astype(F32))
    params = np.concatenate([a.reshape(-1) for a in P])
    med = P[14][:, 1].astype(np.float64)
    z = TC._normal(rng, (C, N), 3.0)
    placed = {"tie": [], "saturated": [], "tail": [], "sign": []}
    probe = lambda zz: eb_eval_body(Tape("f64"), eb_split(params, C), zz)
    pix = list(range(N))
    # ties, both parities and both signs, on every channel of the first four pixels
    for p, k in zip(pix[:4], (0.5, 1.5, -0.5, -2.5)):
        z[:, p] = (med + k).astype(F32)
        placed["tie"].append(p)
    if N >= 7:
        c = min(1, C - 1)
        for p, sgn in ((4, 1.0), (5, -1.0)):                        # both sigmoids saturate: the likelihood at the bound
            for mag in (45.0, 70.0, 110.0, 170.0, 260.0):
                z[c, p] = F32(med[c] + sgn * mag)
                if probe(z)["lik_raw"].numpy()[c, p] < BAND[0]:
                    break
            placed["saturated"].append((c, p))
        c2 = min(2, C - 1)
        o = probe((med[:, None] + np.arange(-30, 31)[None, :]).astype(F32))       # the kernel evaluates at integers + median only
        s = o["sum"].numpy()[c2]
        scale = np.maximum(np.abs(o["lower"].numpy()[c2]), np.abs(o["upper"].numpy()[c2]))
        ok = np.abs(s) > 2.0 ** -14 * scale                          # a clear sign in fp32 (the rule has a third branch at exactly 0)
        k0 = int(np.arange(-30, 31)[ok][np.argmin(np.abs(s[ok]))])
        z[c2, 6] = F32(med[c2] + k0)
        placed["sign"] = [(c2, 6, k0)]
    if N >= 100:                                                     # tail pixels: likelihoods of 1e-8 .. 1e-3, where bits are expensive
        for j, p in enumerate(range(8, 8 + 12)):
            kk = (6, 9, 12, 15, 18, 22)[j % 6] * (1 if j < 6 else -1)
            z[:, p] = (med + kk).astype(F32)
            placed["tail"].append(p)
    fixed = np.zeros((C, N), dtype=bool)
    for c, p in placed["saturated"]:
        fixed[c, p] = True
    fixed[:, placed["tie"]] = True
    for _ in range(40):                                              # an unplaced pixel in or below the band is pulled towards the median
        lr = probe(z)["lik_raw"].numpy()
        stray = (lr <= BAND[1]) & ~fixed
        if not stray.any():
            break
        z[stray] = (med[:, None] + 0.5 * (z.astype(np.float64) - med[:, None]))[stray].astype(F32)
    lr = probe(z)["lik_raw"].numpy()                                 # a tie that a steep channel puts into the band becomes the tie at 0.5 there
    inband = (lr >= BAND[0]) & (lr <= BAND[1]) & fixed
    z[inband] = (med[:, None] + 0.5 + 0.0 * z)[inband].astype(F32)
    return {"params": params, "z": z}, placed


@functools.lru_cache(maxsize=None)
def inputs(cid):
    case = CASES[cid]
    I, placed = _draw_tail(case) if case.fam == "tail" else _draw_eb(case)
    for v in I.values():
        v.setflags(write=False)
    return I, placed


# ====================================================================================================== references
def _ref_lik(run, exp):
    """Ref of a likelihood from run(T) -> dict(lik, lik_raw); exp maps a pattern array to the output's logical shape"""
    o64, o32 = run(Tape("f64")), run(Tape("f32"))
    Tb = Tape("budget")
    ob = run(Tb)
    r64, raw64 = o64["lik"].numpy(), o64["lik_raw"].numpy()
    band = (raw64 >= BAND[0]) & (raw64 <= BAND[1])
    A = Tb.budget_of(ob["lik"])
    if band.any():
        A = np.where(band, np.maximum(A, Tb.budget_of(ob["lik_raw"])), A)
    alt = np.where(r64 == raw64, BOUND_L, raw64)
    return Ref(exp(r64), exp(o32["lik"].numpy()), exp(A), False, exp(alt), exp(band))


def _ref_exact(run, name, exp):
    o64, oe = run(Tape("f64")), run(Tape("f32e"))
    return Ref(exp(o64[name].numpy()), exp(oe[name].numpy().astype(F32)), None, True)


@functools.lru_cache(maxsize=None)
def tail_reference(cid, variant):
    """{yhat, sym, lik: Ref} of one chain over a case's inputs.  variant: "unmasked" | "unmasked-noy2" | "masked" (level 0's mask) |
    "masked-noy2" | "ones" (gauss_layer_bits) | "levels" (all MAX_MASK_LEVELS masks: arrays [L, n_pix, C])"""
    case = CASES[cid]
    I = dict(inputs(cid)[0])
    if variant.endswith("-noy2"):
        del I["y2"]
    kind = variant.split("-")[0]
    masked = kind != "unmasked"
    if kind == "masked":
        I["mask"] = I["mask"][0]
    elif kind == "ones":
        I["mask"] = np.ones_like(I["sigma"])
    exp = lambda a: expand(case, a)
    run = lambda T: tail_body(T, I, masked)
    out = {"lik": _ref_lik(run, exp), "yhat": _ref_exact(run, "yhat", exp)}
    sym = run(Tape("f32e"))["sym"].numpy()
    out["sym"] = expand(case, sym.astype(np.int32))
    return out


@functools.lru_cache(maxsize=None)
def index_reference(cid, masked):
    case = CASES[cid]
    I = inputs(cid)[0]
    return expand(case, index_body(Tape("f32e"), I["sigma"], I["mask"][0] if masked else None, scale_table()).numpy().astype(np.int32))


def decode_ks(n_levels):
    """container thresholds of a decode launch: increasing, the last one beyond every listed id but 0xFF"""
    return [0, 1, 2, 5, 9, 17, 33, 40][:n_levels - 1] + [40]


@functools.lru_cache(maxsize=None)
def decode_reference(cid, n_levels):
    case = CASES[cid]
    I = inputs(cid)[0]
    sym = tail_body(Tape("f32e"), I, False)["sym"].numpy().astype(np.int32)
    y = decode_body(Tape("f32e"), sym, I["layer"], I["mu"], decode_ks(n_levels)).numpy()
    return sym, expand(case, y.astype(F32))


@functools.lru_cache(maxsize=None)
def eb_reference(cid):
    """{zhat: Ref, sym: int32 [C, N], lik: Ref}, arrays [C, N]"""
    case = CASES[cid]
    I = inputs(cid)[0]
    P = eb_split(I["params"], case.C)
    run = lambda T: eb_eval_body(T, P, I["z"])
    o64, o32, oe, ob = run(Tape("f64")), run(Tape("f32")), run(Tape("f32e")), run(Tape("run"))
    r64, raw64 = o64["lik"].numpy(), o64["lik_raw"].numpy()
    band = (raw64 >= BAND[0]) & (raw64 <= BAND[1])
    A = np.where(band, np.maximum(ob["lik"].e.numpy(), ob["lik_raw"].e.numpy()), ob["lik"].e.numpy())
    alt = np.where(r64 == raw64, BOUND_L, raw64)
    return {"lik": Ref(r64, o32["lik"].numpy(), A, False, alt, band),
            "zhat": Ref(o64["zhat"].numpy(), oe["zhat"].numpy().astype(F32), None, True),
            "sym": oe["sym"].numpy().astype(np.int32)}


# ====================================================================================================== judgement
def bits_bound(ref, K):
    """per-element bound on |log2 got - log2 ref64| (for an in-band element: against the branch the float64 body took)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (K * U24 * ref.A + FLOOR) / (ref.ref64 * LN2) * BITS_SLACK


def judge_lik(what, got, ref, K):
    """The acceptance rule of a likelihood window, as a ratio and in bits.  Returns (worst ratio, worst bits error); raises
    AssertionError where either statement fails."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.ref64.shape)
    assert np.isfinite(got).all() and (got > 0).all(), (what, "a likelihood that is not finite and positive")
    rat, i = ref.ratio(got)
    assert rat <= K, (what, "ratio", rat, K, i, got.reshape(-1)[i], ref.ref64.reshape(-1)[i], ref.A.reshape(-1)[i])
    lg = np.log2(got)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(lg - np.log2(ref.ref64))
        bound = bits_bound(ref, K)
        over = np.where(err > 0, err / bound, 0.0)                  # an exact hit of a zero-budget element is 0 / 0
        if ref.band is not None and ref.band.any():
            e2 = np.abs(lg - np.log2(ref.alt64))
            b2 = (K * U24 * ref.A + FLOOR) / (ref.alt64 * LN2) * BITS_SLACK
            o2 = np.where(e2 > 0, e2 / b2, 0.0)
            take = ref.band & (o2 < over)
            over, err = np.where(take, o2, over), np.where(take, e2, err)
    over = np.where(np.isnan(over), np.inf, over)
    j = int(np.argmax(over))
    assert over.reshape(-1)[j] <= 1.0, (what, "bits", err.reshape(-1)[j], over.reshape(-1)[j], j, got.reshape(-1)[j], ref.ref64.reshape(-1)[j])
    return rat, float(err.max())


def judge_exact(what, got, want):
    """bit equality of an exact output: float32 against the emulated chain (signed zeros included), or integers"""
    got, want = np.asarray(got), np.asarray(want)
    got = got.reshape(want.shape)
    if want.dtype.kind == "f":
        assert np.isfinite(got).all(), (what, "not finite inside the window")
        diff = bits(got) != bits(want)
    else:
        diff = got.astype(np.int64) != want.astype(np.int64)
    assert not diff.any(), (what, int(diff.sum()), got[diff][:4], want[diff][:4])


def judge_sum(what, got, own_terms, ref=None, K=None, groups=None, n_groups=None):
    """A float64 sum output [n_groups] against the float64 sum of log2 of the launch's own fp32 likelihoods (1e-12 of sum |term|)
    and — ref given — against the sum of log2(ref64) within the summed per-element bounds.  groups: the group of each element."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    n_groups = got.size if n_groups is None else n_groups
    groups = np.asarray(groups).reshape(-1)
    t = np.log2(np.asarray(own_terms, dtype=np.float64)).reshape(-1)
    own = np.bincount(groups, weights=t, minlength=n_groups)
    mag = np.bincount(groups, weights=np.abs(t), minlength=n_groups)
    assert np.isfinite(got).all(), (what, got)
    bad = np.abs(got - own) > SUM_RTOL * mag
    assert not bad.any(), (what, "against its own terms", got[bad][:3], own[bad][:3], mag[bad][:3])
    worst = float(np.max(np.abs(got - own) / np.maximum(mag, 1e-300))) if got.size else 0.0
    if ref is not None:
        assert not ref.band.any(), (what, "a case that checks sums against float64 has no in-band element")
        want = np.bincount(groups, weights=np.log2(ref.ref64).reshape(-1), minlength=n_groups)
        tol = np.bincount(groups, weights=bits_bound(ref, K).reshape(-1), minlength=n_groups)
        bad = np.abs(got - want) > tol + SUM_RTOL * mag
        assert not bad.any(), (what, "against float64", got[bad][:3], want[bad][:3], tol[bad][:3])
    return worst


def outside_ref():
    """Ref of the likelihood of an element outside every mask: |v| = 0, s = 0 (the 0.11 bound applies)"""
    I = {"y": np.zeros(1, F32), "mu": np.zeros(1, F32), "sigma": np.zeros(1, F32), "mask": np.zeros(1, F32)}
    return _ref_lik(lambda T: tail_body(T, I, True), lambda a: a)


# ====================================================================================================== K
GAUSS_VARIANTS = {"t-min": ("unmasked", "masked", "levels", "ones"), "t-mixed": ("unmasked", "masked", "levels", "ones"),
                  "t-ragged": ("unmasked", "masked", "levels", "ones"), "t-blocks": ("levels", "ones"), "t-levels": ("levels", "ones"),
                  "t-stride": ("masked",), "t-opt": ("unmasked", "unmasked-noy2", "masked", "masked-noy2")}


@functools.lru_cache(maxsize=None)
def k_cpu(fam):
    """worst ratio of the float32 body against the float64 one over this contract's inputs: "gauss" or "eb" """
    worst = 0.0
    if fam == "gauss":
        for cid, vs in GAUSS_VARIANTS.items():
            for v in vs:
                ref = tail_reference(cid, v)["lik"]
                worst = max(worst, ref.ratio(ref.ref32)[0])
        ref = outside_ref()
        worst = max(worst, ref.ratio(ref.ref32)[0])
    else:
        for cid, case in CASES.items():
            if case.fam == "eb":
                ref = eb_reference(cid)["lik"]
                worst = max(worst, ref.ratio(ref.ref32)[0])
    return worst


def k_of(fam):
    return max(K_FACTOR * k_cpu(fam), K_FLOOR)
