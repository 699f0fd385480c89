"""The contract of the training element-wise and likelihood kernels in float64.  TEST HELPER (torch and numpy on the CPU).

Kernels: ``ew_kernel`` / ``axpy_group_kernel`` (csrc/train_gs.hip), ``leaky_bwd`` / ``mul`` / ``ps2_unshuffle`` /
``upsample2_zero`` (csrc/elementwise.hip), ``gauss_train`` / ``gauss_levels`` / ``eb_train_bwd`` and the
noisy likelihood of ``eb_forward_kernel`` (csrc/entropy.hip).

Every operation is ONE function body written in the kernel's order of operations over a ``Tape``:
  * ``ref64``  the body in float64 (inputs are the fp32 values converted exactly) — the reference;
  * ``ref32``  the same body in float32 on the CPU (the library is built with -ffp-contract=off: no fused multiply-adds);
  * ``budget`` A = sum over every fp32 intermediate t of the body (the inputs and their differences included) of
               |d out / d t| * |t|, per element.  It is computed, not transcribed: in budget mode every rounded
               intermediate t is replaced by t * (1 + e_t) with e_t = 0, and autograd of the float64 body delivers
               d out / d e_t = d out / d t * t.  A product with an fp32-rounded mathematical constant counts twice.
For the Gaussian likelihood this reproduces, term for term, e_v = |y| + |y2| + |y - y2| + |mu| + |d| + |d m| + |n| + |v|,
du = e_v / s + |0.5 - |v|| / s + 3 |u| and A_lik = Phi(u) + Phi(l) + |lik| + phi(u) du + phi(l) dl.

Acceptance of one element:  |got - ref64| <= K * 2^-24 * A + 2^-126  with K = max(4 * K_cpu, 8), K_cpu the worst
(|ref32 - ref64| - 2^-126) / (2^-24 A) of the operation over the contract's own inputs (``k_cpu``).
Operations made of + - * /, sqrt, max, comparisons and copies only are EXACT: bit-equal to ref32, which for them is the
emulated, correctly rounded chain (Tape mode "f32e") and not a host's ATen float32.

Decisions taken on a computed value (likelihood >= 1e-9) split the elements into clear-above (float64 value > 2e-9),
clear-below (< 0.5e-9) and in-band ones; an in-band element may take either branch (``alt`` holds the other one)."""
import dataclasses
import functools
import math

import numpy as np
import torch

U24 = 2.0 ** -24
FLOOR = 2.0 ** -126                      # one smallest normal fp32: whether a GPU flushes subnormals is not this contract's business
F32 = np.float32
BOUND_S = float(F32(0.11))               # the bounds are fp32 numbers in the kernels and in the oracle
BOUND_L = float(F32(1e-9))
BAND = (0.5e-9, 2e-9)
K_FLOOR, K_FACTOR = 8.0, 4.0
INV_SQRT2 = 0.70710678118654752440
INV_SQRT2PI = 0.3989422804014327
SENTINEL_BITS = -0x21524111              # 0xDEADBEEF as int32: a finite fp32 (-6.26e18) no kernel here produces

(EW_GELU_FWD, EW_GELU_BWD, EW_GATE_BWD, EW_GDN_APPLY, EW_GDN_BWD_PREP, EW_GDN_BWD_FIN, EW_CLAMP_BWD, EW_AXPY, EW_GATE_FWD,
 EW_REPARAM_BWD, EW_HTANH_FWD, EW_HTANH_BWD, EW_MASK_SPLIT) = range(13)


class Tape:
    """Runs a body in one of five modes: "f64", "f32", "budget" (float64 with a zero relative perturbation per rounding: the
    exact sum, by autograd), "run" (the bottleneck: float64 values carrying a running bound, see ``V``) and "f32e": float32
    EMULATED — every + - * / and sqrt is done in float64 on fp32 operands and rounded to fp32 once, which is the correctly
    rounded fp32 result (53 >= 2 * 24 + 2 bits: the double rounding is innocuous).  The exact operations take their float32
    statement from "f32e", so that it does not depend on how a host's ATen builds its float32 sqrt and division."""

    def __init__(self, mode):
        assert mode in ("f64", "f32", "f32e", "budget", "run")
        self.mode = mode
        self.dtype = torch.float32 if mode == "f32" else torch.float64
        self.eps = []

    def inp(self, a):
        t = torch.tensor(np.asarray(a), dtype=self.dtype)
        return self.r(V(t) if self.mode == "run" else t)

    def r(self, t, n=1):
        """``t`` is stored as an fp32 number in the kernel (n roundings of its size)."""
        if self.mode == "run":
            return V(t.v, t.e + n * t.v.abs())
        if self.mode == "f32e":
            return t.to(torch.float32).to(torch.float64)
        if self.mode != "budget":
            return t
        e = torch.zeros_like(t, requires_grad=True)
        self.eps.append((e, n))
        return t * (1.0 + e)

    def budget_of(self, out, reduce=None):
        """sum_t n_t |d sum(out) / d e_t|: per element for element-wise bodies; ``reduce`` maps a gradient to the output's shape."""
        if reduce is None and out.dim() == 2:                # [levels, Q]: level by level (shared operands have one row)
            return np.stack([self.budget_of(out[k]) for k in range(out.shape[0])])
        if reduce is None:
            reduce = lambda g: g.sum(0) if g.dim() == 2 else g
        if not out.requires_grad:
            return np.zeros(out.shape if reduce is None else reduce(torch.zeros_like(self.eps[0][0])).shape)
        gs = torch.autograd.grad(out.sum(), [e for e, _ in self.eps], retain_graph=True, allow_unused=True)
        acc = None
        for (e, n), g in zip(self.eps, gs):
            if g is None:
                continue
            g = g.abs() * n
            g = g if reduce is None else reduce(g)
            acc = g if acc is None else acc + g
        return acc.numpy()


def _where(c, a, b):
    return torch.where(c, a, b)


def _z(t):
    return torch.zeros_like(t)


# ====================================================================================================== element-wise bodies
def _erf_arg(T, v):
    return T.r(v * INV_SQRT2, 2)


def _sigmoid(T, b):
    e = T.r(torch.exp(-b))
    return T.r(1.0 / T.r(1.0 + e))


def ew_body(T, op, x, coef=0.0, flag=0):
    """``vam_train_elementwise``: x = list of inputs, returns the list of outputs (order of the kernel's out[])."""
    r = T.r
    if op == EW_GELU_FWD:                   # nn.GELU(): 0.5 v (1 + erf(v / sqrt 2))
        e = r(torch.erf(_erf_arg(T, x[0])))
        return [r((x[0] * 0.5) * r(1.0 + e))]
    if op == EW_GELU_BWD:                   # g * (Phi(v) + v phi(v))
        v, g = x
        a = r(0.5 * r(1.0 + r(torch.erf(_erf_arg(T, v)))))
        ex = r(torch.exp(r((-0.5 * v) * v)))
        b = r(r(v * INV_SQRT2PI, 2) * ex)
        return [r(g * r(a + b))]
    if op == EW_GATE_FWD:                   # a * sigmoid(b) + x
        a, b, xx = x
        return [r(r(a * _sigmoid(T, b)) + xx)]
    if op == EW_GATE_BWD:                   # in: a, b, dout -> d a = g s, d b = g a s (1 - s)
        a, b, g = x
        s = _sigmoid(T, b)
        return [r(g * s), r(r(g * a) * r(s * r(1.0 - s)))]
    if op == EW_GDN_APPLY:                  # x sqrt(norm) (flag) or x / sqrt(norm)
        xx, n = x
        rt = r(torch.sqrt(n))
        return [r(rt * xx) if flag else r(r(1.0 / rt) * xx)]
    if op == EW_GDN_BWD_PREP:               # in: x, norm, dy -> dL/dnorm, dy * dy/dx|norm, x^2
        xx, n, g = x
        rt = r(torch.sqrt(n))
        if flag:
            o0, o1 = r(r(g * xx) / (2.0 * rt)), r(g * rt)
        else:
            o0, o1 = r(r(-g * xx) / r((2.0 * n) * rt)), r(g / rt)
        return [o0, o1, r(xx * xx)]
    if op == EW_GDN_BWD_FIN:                # in0 + 2 x u
        a, xx, u = x
        return [r(a + r((2.0 * xx) * u))]
    if op == EW_CLAMP_BWD:                  # in0 = the clamped value: passes strictly inside (0, 1)
        v, g = x
        return [_where((v > 0.0) & (v < 1.0), g, _z(g))]
    if op == EW_AXPY:
        return [r(x[0] + r(coef * x[1]))]
    if op == EW_REPARAM_BWD:                # value = max(p, bound)^2 - pedestal with LowerBound's rule; coef = bound
        p, g = x
        go = r((g * 2.0) * torch.clamp_min(p, coef))
        return [_where((p >= coef) | (go < 0.0), go, _z(go))]
    if op == EW_HTANH_FWD:                  # (0.5 tanh(z) + p1) + p2
        z, p1, p2 = x
        return [r(r(0.5 * r(torch.tanh(z)) + p1) + p2)]
    if op == EW_HTANH_BWD:                  # g * 0.5 (1 - tanh(z)^2)
        z, g = x
        t = r(torch.tanh(z))
        return [r(g * (0.5 * r(1.0 - r(t * t))))]
    if op == EW_MASK_SPLIT:                 # g m, g (1 - m)
        g, m = x
        return [r(g * m), r(g * r(1.0 - m))]
    raise KeyError(op)


def leaky_body(T, x):                       # act = LeakyReLU OUTPUT (same sign as its input), slope 0.01
    act, g = x
    return [T.r(g * _where(act > 0.0, torch.ones_like(g), torch.full_like(g, 0.01 if T.mode in ("f64", "budget") else float(F32(0.01)))), 2)]


def mul_body(T, x):
    return [T.r(x[0] * x[1])]


# ====================================================================================================== the noisy Gaussian likelihood
def _phi_cdf(T, t):
    return 0.5 * T.r(torch.erfc(T.r(-INV_SQRT2 * t, 2)))


def _phi_pdf(T, t):
    return T.r(INV_SQRT2PI * T.r(torch.exp(T.r((-0.5 * t) * t))), 2)


def _lik_common(T, d, sg, m, n):
    r = T.r
    v = r(r(d * m) + n) if m is not None else r(d + n)
    raw_s = r(sg * m) if m is not None else sg
    s = torch.clamp_min(raw_s, BOUND_S)
    av = v.abs()
    u, l = r(r(0.5 - av) / s), r(r(-0.5 - av) / s)
    lik_raw = r(_phi_cdf(T, u) - _phi_cdf(T, l))
    return v, raw_s, s, av, u, l, lik_raw


def lik_fwd(T, d, sg, m, n, passes=None):
    """max(Phi((.5 - |v|) / s) - Phi((-.5 - |v|) / s), 1e-9), v = d m + n, s = max(sigma m, 0.11).  ``passes``: the decision
    lik_raw >= 1e-9 forced (in-band elements), None = taken on the body's own value."""
    lik_raw = _lik_common(T, d, sg, m, n)[-1]
    if passes is None:
        return torch.clamp_min(lik_raw, BOUND_L), lik_raw
    return (lik_raw if passes else torch.full_like(lik_raw, BOUND_L)), lik_raw


def lik_bwd(T, d, sg, m, n, g, passes=None, mut=()):
    """(dmu, dsigma) for the incoming gradient g of the bounded likelihood, both LowerBound rules included."""
    r = T.r
    v, raw_s, s, av, u, l, lik_raw = _lik_common(T, d, sg, m, n)
    keep = (lik_raw >= BOUND_L) if passes is None else torch.full_like(lik_raw, bool(passes), dtype=torch.bool)
    neg = (g <= 0.0) if "lb_le" in mut else (g < 0.0)
    g = _where(keep | neg, g, _z(g))
    pu, pl = _phi_pdf(T, u), _phi_pdf(T, l)
    sgn = _where(av == 0.0, _z(v), _where(v > 0.0, torch.ones_like(v), -torch.ones_like(v)))
    dlik_dv = sgn * r(r(pl - pu) / s)
    gs = r(r(g * r(r(pl * l) - r(pu * u))) / s)
    s_rule = sg if "scale_on_sigma" in mut else raw_s
    gs = _where((s_rule >= BOUND_S) | (gs < 0.0), gs, _z(gs))
    dmu = r(-g * dlik_dv)
    if m is not None:
        dmu = r(dmu * m)
        dsg = gs if "no_mask_dsigma" in mut else r(gs * m)
    else:
        dsg = gs
    return dmu, dsg


def gauss_body(T, I, bwd, passes=None, mut=()):
    """``vam_gauss_train``: I = dict(y, mu, sigma, noise[, y2][, mask][, g])."""
    d = T.r(I["y"] - I["y2"]) if "y2" in I else I["y"]
    d = T.r(d - I["mu"])
    if not bwd:
        return {"lik": lik_fwd(T, d, I["sigma"], I.get("mask"), I["noise"], passes)[0]}
    dmu, dsg = lik_bwd(T, d, I["sigma"], I.get("mask"), I["noise"], I["g"], passes, mut)
    return {"dmu": dmu, "dsigma": dsg}


def levels_body(T, I, bwd, passes=None):
    """``vam_gauss_levels_fwd`` / ``_bwd``: mask, noise, g (grad_lik), drq are [L, ...]; dyt / dys the in-place windows."""
    r = T.r
    d = T.r(I["y"] - I["y2"]) if "y2" in I else I["y"]
    d = r(d - I["mu"])
    nl = I["mask"].shape[0]
    if not bwd:
        rq, lik = [], []
        for k in range(nl):
            m = I["mask"][k]
            rq.append(r(r(torch.round(d) * m) + I["mu"]))
            lik.append(lik_fwd(T, d, I["sigma"], m, I["noise"][k], passes)[0])
        return {"rq": torch.stack(rq), "lik": torch.stack(lik)}
    gacc, sacc, dyt = _z(d), _z(d), I["dyt"]
    dys = I.get("dys")
    for k in range(nl):
        m, q = I["mask"][k], I["drq"][k]
        dmu, dsg = lik_bwd(T, d, I["sigma"], m, I["noise"][k], I["g"][k], passes)
        dr = r(q * m)
        g = r(q * r(1.0 - m))
        g = r(g + dmu)
        dr = r(dr - dmu)
        dyt = r(dyt + dr)
        if dys is not None:
            dys = r(dys - dr)
        gacc = r(gacc + g)
        sacc = r(sacc + dsg)
    out = {"gmu": gacc, "dsigma": sacc, "dyt": dyt}
    if dys is not None:
        out["dys"] = dys
    return out


# ====================================================================================================== entropy bottleneck
class V:
    """Forward-mode running error: a float64 value and the first-order bound e on its fp32 error in units of 2^-24, i.e. the
    running form of sum_t |d out / d t| |t| (the triangle inequality is taken at every step, so it is never below that sum).
    The bottleneck's 58 sums per channel over hundreds of intermediates are budgeted this way: one pass instead of 58
    reverse passes."""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(torch.as_tensor(o, dtype=torch.float64))

    shape = property(lambda self: self.v.shape)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.e)

    def __sub__(self, o):
        return self + (-V.of(o))

    def __rsub__(self, o):
        return V.of(o) + (-self)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e)
    __rmul__ = __mul__

    def __rtruediv__(self, o):
        o = V.of(o)
        return V(o.v / self.v, o.e / self.v.abs() + (o.v / (self.v * self.v)).abs() * self.e)

    def __gt__(self, o): return self.v > V.of(o).v
    def __lt__(self, o): return self.v < V.of(o).v
    def __ge__(self, o): return self.v >= V.of(o).v
    def abs(self): return V(self.v.abs(), self.e)
    def sum(self, dim): return V(self.v.sum(dim), self.e.sum(dim))
    def detach(self): return self
    def numpy(self): return self.v.numpy()


def _fn(x, f, df):
    return V(f(x.v), df(x.v).abs() * x.e) if isinstance(x, V) else f(x)


def _tanh(x): return _fn(x, torch.tanh, lambda v: 1.0 - torch.tanh(v) ** 2)
def _exp(x): return _fn(x, torch.exp, torch.exp)
def _log1p(x): return _fn(x, torch.log1p, lambda v: 1.0 / (1.0 + v))


def _sel(c, a, b, like):
    """where(c, a, b) with python floats allowed"""
    if isinstance(like, V) or isinstance(a, V) or isinstance(b, V):
        a, b = V.of(a), V.of(b)
        return V(torch.where(c, a.v, b.v), torch.where(c, a.e.expand_as(c) if a.e.dim() else a.e, b.e.expand_as(c) if b.e.dim() else b.e))
    a = a if torch.is_tensor(a) else torch.full_like(like, a)
    b = b if torch.is_tensor(b) else torch.full_like(like, b)
    return torch.where(c, a, b)


EB_NAMES = ["_matrix0", "_bias0", "_factor0", "_matrix1", "_bias1", "_factor1", "_matrix2", "_bias2", "_factor2",
            "_matrix3", "_bias3", "_factor3", "_matrix4", "_bias4", "quantiles"]
EB_SHAPES = [(3, 1), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (1, 3), (1, 1), (1, 3)]
EB_THREADS = 128


def eb_split(params, C):
    """flat [61 C] (tensor-major, channel-major inside a tensor) -> list of [C, n] arrays in EB_NAMES order."""
    out, o = [], 0
    for shp in EB_SHAPES:
        n = shp[0] * shp[1]
        out.append(params[o:o + C * n].reshape(C, n))
        o += C * n
    assert o == params.size
    return out


def _sigmoid_t(T, b):
    """1 / (1 + exp(-b)).  Running mode: the three roundings (exp, 1 + e, 1 / .) weigh s (1 - s), s and s, written out so
    that an overflowing exp(-b) (s = 0, as in fp32) does not become inf * 0."""
    if T.mode == "run":
        s = torch.sigmoid(b.v)
        return V(s, s * (1.0 - s) * (b.e + 1.0) + 2.0 * s)
    return T.r(1.0 / T.r(1.0 + T.r(_exp(-b))))


def _softplus(T, x):
    big = x > 20.0
    sp = T.r(_log1p(T.r(_exp(_sel(big, 0.0, x, x)))))
    return _sel(big, x, sp, x)


def _eb_net(T, P, N):
    """Transformed parameters, each a [C, N] tensor (expanded over the pixels BEFORE the rounding mark, so that a budget is per
    pixel): m[i][k][j] = softplus(matrix i)[k, j], b[i][k], f[i][k] = tanh(factor i)[k]; raw values for the chain rules."""
    def ex(a, col):
        return T.inp(np.broadcast_to(a[:, col:col + 1], (a.shape[0], N)))
    net = {"m": [], "b": [], "f": [], "rawm": [], "rawf": []}
    for i in range(5):
        rows, cols = EB_SHAPES[3 * i]
        net["rawm"].append([[ex(P[3 * i], k * cols + j) for j in range(cols)] for k in range(rows)])
        net["m"].append([[_softplus(T, v) for v in row] for row in net["rawm"][-1]])
        net["b"].append([ex(P[3 * i + 1], k) for k in range(rows)])
        if i < 4:
            net["rawf"].append([ex(P[3 * i + 2], k) for k in range(rows)])
            net["f"].append([T.r(_tanh(v)) for v in net["rawf"][-1]])
    return net


def _eb_fwd(T, net, x):
    """logits of the 1-3-3-3-3-1 network at x, keeping tanh(v) and the layer inputs."""
    r = T.r
    trace, inp = [], [x]
    for i in range(4):
        th, out = [], []
        for k in range(3):
            v = r(net["m"][i][k][0] * inp[0])
            for j in range(1, len(inp)):
                v = r(v + r(net["m"][i][k][j] * inp[j]))
            v = r(v + net["b"][i][k])
            t = r(_tanh(v))
            th.append(t)
            out.append(r(v + r(net["f"][i][k] * t)))
        trace.append((inp, th))
        inp = out
    v = r(net["m"][4][0][0] * inp[0])
    v = r(v + r(net["m"][4][0][1] * inp[1]))
    v = r(v + r(net["m"][4][0][2] * inp[2]))
    return r(v + net["b"][4][0]), trace, inp


def _eb_bwd(T, net, trace, last, g):
    """per-pixel contributions to dL/d(transformed parameters) for dL/dlogit = g, and dL/dx: the order of eb_bwd."""
    r = T.r
    terms = {("m", 4, 0, j): r(g * last[j]) for j in range(3)}
    terms[("b", 4, 0)] = g
    gin = [r(g * net["m"][4][0][j]) for j in range(3)]
    for i in range(3, -1, -1):
        inp, th = trace[i]
        gp = None
        for k in range(3):
            terms[("f", i, k)] = r(gin[k] * th[k])
            gv = r(gin[k] * r(1.0 + r(net["f"][i][k] * r(1.0 - r(th[k] * th[k])))))
            terms[("b", i, k)] = gv
            for j in range(len(inp)):
                terms[("m", i, k, j)] = r(gv * inp[j])
            c = [r(gv * net["m"][i][k][j]) for j in range(len(inp))]
            gp = c if gp is None else [r(a + b) for a, b in zip(gp, c)]
        gin = gp
    return terms, gin[0]


def eb_keys():
    """the 58 parameters of a channel in the order of the flat parameter block's tensors: (kind, layer, row[, col])."""
    keys = []
    for i in range(5):
        rows, cols = EB_SHAPES[3 * i]
        keys += [("m", i, k, j) for k in range(rows) for j in range(cols)]
        keys += [("b", i, k) for k in range(rows)]
        if i < 4:
            keys += [("f", i, k) for k in range(rows)]
    return keys


def eb_body(T, P, z, noise, g=None, passes=None, mut=()):
    """``vam_eb_forward_noise`` (lik) and ``vam_eb_train_bwd`` (dz [C, N], dparams {key: [C]}).  P = eb_split(params);
    z, noise, g are [C, N] (channel-major).  Returns dict(lik, lik_raw[, dz, dparams, terms])."""
    r = T.r
    C, N = z.shape
    net = _eb_net(T, P, N)
    x = r(T.inp(z) + T.inp(noise))
    lower, tl, ll = _eb_fwd(T, net, r(x - 0.5))
    upper, tu, lu = _eb_fwd(T, net, r(x + 0.5))
    s = r(lower + upper)
    sign = _sel(s > 0.0, -1.0, _sel(s < 0.0, 1.0, 0.0, s), s)
    sign = sign.v if isinstance(sign, V) else sign              # detached (entropy_models.py:431-432): an exact -1, 0 or 1
    su, sl = _sigmoid_t(T, sign * upper), _sigmoid_t(T, sign * lower)
    diff = r(su - sl)
    lik_raw = diff.abs()
    lr = lik_raw.v if isinstance(lik_raw, V) else lik_raw
    keep = (lr >= BOUND_L) if passes is None else torch.full_like(lr, bool(passes), dtype=torch.bool)
    out = {"lik_raw": lik_raw, "lik": _sel(keep, lik_raw, BOUND_L, lik_raw), "logits": (V.of(lower).v.abs(), V.of(upper).v.abs())}
    if g is None:
        return out
    g = T.inp(g)
    g = _sel(keep | (g < 0.0), g, 0.0, g)
    gd = g * _sel(diff > 0.0, 1.0, _sel(diff < 0.0, -1.0, 0.0, s), s)
    wu, wl = r(su * r(1.0 - su)), r(sl * r(1.0 - sl))
    gu = r(gd * wu) * sign
    gl = r(-gd * wl) * sign
    if "sign_attached" in mut:           # a straight-through sign -(lower + upper): its slope -1 leaks into both logits' gradients
        leak = -(r(r(gd * wu) * upper) - r(r(gd * wl) * lower))
        gu, gl = gu + leak, gl + leak
    t_u, gx_u = _eb_bwd(T, net, tu, lu, gu)
    t_l, gx_l = _eb_bwd(T, net, tl, ll, gl)
    out["dz"] = r(gx_u + gx_l)
    # chain to the stored values, applied once per thread after its pixels: d softplus = sigmoid(raw), d tanh = 1 - tanh^2
    chain = {}
    for key in eb_keys():
        if key[0] == "m":
            chain[key] = _sigmoid_t(T, net["rawm"][key[1]][key[2]][key[3]])
        elif key[0] == "f":
            f = net["rawf" if "tanh_raw" in mut else "f"][key[1]][key[2]]
            chain[key] = r(1.0 - r(f * f))
        else:
            chain[key] = None
    dpar, mag = {}, {}
    for key in eb_keys():
        a, b, ch = t_u[key], t_l[key], chain[key]
        if T.mode == "f32":                                  # the kernel's order: thread t takes pixels t, t + 128, ...; upper, then lower
            acc = torch.zeros((C, EB_THREADS), dtype=T.dtype)
            for j in range(0, N, EB_THREADS):
                w = min(EB_THREADS, N - j)
                acc[:, :w] = acc[:, :w] + a[:, j:j + w]
                acc[:, :w] = acc[:, :w] + b[:, j:j + w]
            if ch is not None:
                acc = acc * ch[:, :1]
            tot = torch.zeros(C, dtype=T.dtype)
            for t in range(EB_THREADS):                      # fixed order over the threads
                tot = tot + acc[:, t]
            dpar[key] = tot
        else:
            pa, pb = (r(a * ch), r(b * ch)) if ch is not None else (a, b)
            dpar[key] = (pa + pb).sum(1)
            mag[key] = (pa.abs() + pb.abs()).sum(1)
    out["dparams"], out["terms"] = dpar, mag
    return out


def eb_sum_terms(N):
    """Additions on the longest chain of one parameter's sum: two per pixel of a thread, then the 128 threads in order.  Each
    rounds a partial sum no larger than sum |term|, so the summation adds n * sum |term| to a budget (never more than the
    2 N + 128 additions that exist)."""
    return min(2 * N + EB_THREADS, 2 * -(-N // EB_THREADS) + EB_THREADS)


# ====================================================================================================== layout kernels
def ps2_unshuffle_ref(src, mut=()):
    """dst[b, y, x, c*4 + i*2 + j] = src[b, 2y+i, 2x+j, c]: src [B, 2H, 2W, Cq] -> [B, H, W, 4 Cq] (any dtype, a copy)."""
    B, H2, W2, Cq = src.shape
    t = src.reshape(B, H2 // 2, 2, W2 // 2, 2, Cq)           # b y i x j c
    order = (0, 1, 3, 5, 4, 2) if "ji" in mut else (0, 1, 3, 5, 2, 4)
    return np.ascontiguousarray(t.transpose(order)).reshape(B, H2 // 2, W2 // 2, 4 * Cq)


def upsample2_zero_ref(src, mut=()):
    """dst[b, 2y, 2x, :] = src[b, y, x, :], zero elsewhere."""
    B, H, W, C = src.shape
    dst = np.zeros((B, 2 * H, 2 * W, C), dtype=src.dtype)
    o = 1 if "odd" in mut else 0
    dst[:, o::2, o::2] = src
    return dst


# ====================================================================================================== cases
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    fam: str                 # ew | axpy | leaky | mul | gauss | levels | eb | ps2 | up2
    op: str                  # the operation K_cpu is kept for
    shape: tuple             # (B, H, W)
    C: int
    opt: tuple = ()          # (key, value) pairs

    def o(self, key, default=None):
        return dict(self.opt).get(key, default)

    @property
    def n_pix(self):
        return self.shape[0] * self.shape[1] * self.shape[2]


BASE = (2, 5, 7)
PATTERN = 4099               # over-cap cases repeat a pattern of this (prime) length: element-wise references are computed once per pattern element

EW_OPS = {"GELU_FWD": (EW_GELU_FWD, 1, 1), "GELU_BWD": (EW_GELU_BWD, 2, 1), "GATE_FWD": (EW_GATE_FWD, 3, 1),
          "GATE_BWD": (EW_GATE_BWD, 3, 2), "GDN_APPLY": (EW_GDN_APPLY, 2, 1), "GDN_BWD_PREP": (EW_GDN_BWD_PREP, 3, 3),
          "GDN_BWD_FIN": (EW_GDN_BWD_FIN, 3, 1), "CLAMP_BWD": (EW_CLAMP_BWD, 2, 1), "AXPY": (EW_AXPY, 2, 1),
          "REPARAM_BWD": (EW_REPARAM_BWD, 2, 1), "HTANH_FWD": (EW_HTANH_FWD, 3, 1), "HTANH_BWD": (EW_HTANH_BWD, 2, 1),
          "MASK_SPLIT": (EW_MASK_SPLIT, 2, 2)}
EXACT_EW = {"AXPY", "MASK_SPLIT", "CLAMP_BWD", "REPARAM_BWD", "GDN_APPLY", "GDN_BWD_PREP", "GDN_BWD_FIN"}
REPARAM_BOUND = float(F32(math.sqrt(1e-6 + 2.0 ** -36)))         # NonNegativeParametrizer(minimum = 1e-6): GDN's beta
AXPY_COEF = float(F32(-0.3))

CASES = {}


def _add(case):
    assert case.id not in CASES
    CASES[case.id] = case


for _name in EW_OPS:
    for _flag in ((0, 1) if _name.startswith("GDN") and _name != "GDN_BWD_FIN" else (0,)):
        for _C in (4, 8, 36):
            _add(Case(f"ew-{_name}-f{_flag}-C{_C}", "ew", _name, BASE, _C, (("flag", _flag),)))
    # GDN_BWD_FIN does not read the flag: both values must give the same bits
_add(Case("ew-GDN_BWD_FIN-f1-C8", "ew", "GDN_BWD_FIN", BASE, 8, (("flag", 1),)))
for _name in ("AXPY", "GATE_BWD", "GDN_BWD_PREP"):                # 16400 * 64 float4s: 1024 past the 4096 x 256 grid
    _add(Case(f"ew-{_name}-overcap", "ew", _name, (1, 16400, 1), 256, (("flag", 0), ("tile", True))))
for _n in (1, 2, 5, 8):
    _add(Case(f"axpy-{_n}jobs", "axpy", "axpy_group", BASE, 8, (("jobs", _n),)))
_add(Case("axpy-overcap", "axpy", "axpy_group", (1, 16400, 1), 256, (("jobs", 3), ("tile", True))))
for _C in (4, 8, 36):
    _add(Case(f"leaky-C{_C}", "leaky", "leaky_bwd", BASE, _C))
    _add(Case(f"mul-C{_C}", "mul", "mul", BASE, _C))
_add(Case("leaky-overcap", "leaky", "leaky_bwd", (1, 8208, 1), 256, (("tile", True),)))     # 8208 * 64: 1024 past 2048 x 256
_add(Case("mul-overcap", "mul", "mul", (1, 8208, 1), 256, (("tile", True),)))
for _y2 in (0, 1):
    for _m in (0, 1):
        for _C in (4, 8, 36):
            _add(Case(f"gauss-y2{_y2}-m{_m}-C{_C}", "gauss", "gauss_train", BASE, _C, (("y2", _y2), ("mask", _m))))
_add(Case("gauss-overcap", "gauss", "gauss_train", (1, 8208, 1), 256, (("y2", 1), ("mask", 1), ("tile", True))))
for _L in (1, 3):
    for _y2 in (0, 1):
        for _C in (4, 8, 36):
            _add(Case(f"levels-L{_L}-y2{_y2}-C{_C}", "levels", "gauss_levels", BASE, _C, (("levels", _L), ("y2", _y2))))
_add(Case("levels-overcap", "levels", "gauss_levels", (1, 8208, 1), 256, (("levels", 3), ("y2", 1), ("tile", True))))
for _C in (1, 5, 192):
    for _i, _N in enumerate((1, 100, 128, 129, 549)):
        _pad = 3 * ((_i + (_C == 5)) % 2)                          # both pitches for every C and every n_pix
        _add(Case(f"eb-C{_C}-N{_N}-ld{_C + _pad}", "eb", "eb_train_bwd", (1, 1, _N), _C, (("pad", _pad),)))
for _Cq in (1, 3, 48):
    _add(Case(f"ps2-Cq{_Cq}", "ps2", "ps2_unshuffle", (2, 3, 5), _Cq))
_add(Case("ps2-overcap", "ps2", "ps2_unshuffle", (1, 74, 75), 48))   # 74 * 75 * 192 elements: 66.5 blocks past the 4096 x 256 grid
for _C in (4, 8, 36):
    _add(Case(f"up2-C{_C}", "up2", "upsample2_zero", (2, 3, 5), _C))
_add(Case("up2-overcap", "up2", "upsample2_zero", (1, 129, 129), 64))  # 258 * 258 * 16 float4s: 64.25 blocks past the grid


def layout(case, k):
    """(ld, c0) of operand k of a case: every operand another pitch, windows off the buffer's start, all multiples of 4.  The
    bottleneck kernel reads scalars: its windows start at 0 (the wrapper has no channel offset to give) with pitch C + pad."""
    if case.fam == "eb":
        return case.C + case.o("pad") + (k if case.o("pad") else 0), 0
    c0 = 4 + 4 * (k % 2)
    return case.C + 12 + 4 * k, c0


def _rng(case, salt=0):
    return np.random.RandomState((hash_id(case.id) + salt) % (2 ** 31))


def hash_id(s):
    h = 2166136261
    for ch in s.encode():
        h = ((h ^ ch) * 16777619) % (2 ** 32)
    return h


def _n_unique(case):
    n = case.n_pix * case.C
    return PATTERN if case.o("tile") else n


def expand(case, a):
    """pattern [.., Q] -> [.., n_pix, C]"""
    a = np.asarray(a)
    lead = a.shape[:-1]
    n = case.n_pix * case.C
    flat = a.reshape(-1, a.shape[-1])
    if flat.shape[1] != n:
        flat = np.stack([np.resize(row, n) for row in flat])
    return flat.reshape(lead + (case.n_pix, case.C))


def _normal(rng, q, scale):
    return (rng.standard_normal(q) * scale).astype(F32)


def _away_from_zero(a, lo=1e-3):
    """no subnormal intermediate in a product of two such numbers"""
    return np.where(np.abs(a) < lo, np.copysign(F32(lo), a), a).astype(F32)


TINY = float(np.finfo(F32).tiny)


def _solve_av(s, target):
    """|v| with Phi((.5 - |v|) / s) - Phi((-.5 - |v|) / s) = target (float64 bisection)."""
    f = lambda av: 0.5 * (math.erfc(-INV_SQRT2 * (0.5 - av) / s) - math.erfc(-INV_SQRT2 * (-0.5 - av) / s))
    lo, hi = 0.0, 0.5 + 40.0 * s
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > target else (lo, mid)
    return 0.5 * (lo + hi)


def _lik_raw64(I):
    T = Tape("f64")
    J = {k: T.inp(v) for k, v in I.items()}
    d = J["y"] - J["y2"] if "y2" in J else J["y"]
    return _lik_common(T, d - J["mu"], J["sigma"], J.get("mask"), J["noise"])[-1].numpy()


def _draw_gauss(case, rng, q, levels=None):
    """Inputs of a likelihood case as patterns of length q, with the decision points placed.  Returns (I, placed) where placed
    names the pattern positions of each decision point.  Masks are binary (as the plans' are): d * m and sigma * m are exact."""
    L = levels or 1
    I = {"y": _normal(rng, q, 4.0), "mu": _normal(rng, q, 2.0),
         "sigma": np.exp(rng.uniform(math.log(0.03), math.log(8.0), q)).astype(F32)}
    if case.o("y2"):
        I["y2"] = _normal(rng, q, 2.0)
    masked = levels is not None or case.o("mask")
    lead = (L,) if levels is not None else ()
    if masked:
        I["mask"] = (rng.uniform(size=lead + (q,)) > 0.4).astype(F32)
    I["noise"] = (rng.uniform(size=lead + (q,)) - 0.5).astype(F32)
    I["g"] = _normal(rng, lead + (q,), 1.0)
    placed = {}
    pos = iter(rng.permutation(q)[:min(q, 64)].tolist())

    def put(name, n=1):
        placed.setdefault(name, [])
        idx = [next(pos) for _ in range(n)]
        placed[name] += idx
        return idx

    def setm(i, val):
        if masked:
            I["mask"][..., i] = val

    # the scale bound: sigma * m exactly 0.11f, one ulp below, m = 0
    for name, sig, mval in (("s_at", F32(0.11), 1.0), ("s_below", np.nextafter(F32(0.11), F32(0)), 1.0), ("s_m0", F32(0.7), 0.0)):
        if mval == 0.0 and not masked:
            continue
        for i in put(name, 2):
            I["sigma"][i] = sig
            setm(i, mval)
            I["y"][i] = I["mu"][i] + (I["y2"][i] if "y2" in I else 0) + F32(0.2)
            I["noise"][..., i] = F32(0.05)                          # |v| < 0.5: the likelihood falls as s grows, dlik/ds < 0
        I["g"][..., placed[name][0]] = np.abs(I["g"][..., placed[name][0]])       # both signs of the incoming gradient
        I["g"][..., placed[name][1]] = -np.abs(I["g"][..., placed[name][1]])
    # a fractional mask (the kernels take any m; 0.5 keeps d * m and sigma * m exact): sigma above the bound, sigma * m below it
    if masked:
        for j, i in enumerate(put("s_half", 2)):
            I["sigma"][i] = F32(0.15)
            setm(i, 0.5)
            I["y"][i] = I["mu"][i] + (I["y2"][i] if "y2" in I else 0) + F32(0.25)
            I["noise"][..., i] = F32(0.05)
            I["g"][..., i] = np.abs(I["g"][..., i]) * (1 if j else -1)
    # v == 0: d = -n on a grid where the differences are exact (m = 1), and m = 0 with n = 0
    for i in put("v0_m1", 2):
        I["y"][i], I["mu"][i], I["noise"][..., i] = F32(300 / 1024), F32(-52 / 1024), F32(0)
        if "y2" in I:
            I["y2"][i] = F32(96 / 1024)
        dd = F32(I["y"][i] - (I["y2"][i] if "y2" in I else 0) - I["mu"][i])
        I["noise"][..., i] = -dd
        setm(i, 1.0)
    if masked:
        for i in put("v0_m0", 2):
            I["mask"][..., i] = 0.0
            I["noise"][..., i] = 0.0
    # the likelihood bound: in-band targets, clear-below ones with both signs of g, one far below (erfc underflows)
    def aim(i, target, sign=1.0):
        s = max(float(I["sigma"][i]), BOUND_S)
        av = _solve_av(s, target)
        n0 = float(I["noise"].reshape(-1, q)[0, i])
        I["noise"][..., i] = F32(n0)
        setm(i, 1.0)
        I["y"][i] = F32(sign * av - n0 + float(I["mu"][i]) + (float(I["y2"][i]) if "y2" in I else 0.0))
    for t, i in zip((0.6e-9, 0.9e-9, 1.0e-9, 1.1e-9, 1.8e-9)[:max(1, min(5, q // 200))], put("band", max(1, min(5, q // 200)))):
        I["sigma"][i] = F32(min(max(float(I["sigma"][i]), 0.05), 1.5))      # |v| stays moderate: the band is wide in ulps of y
        aim(i, t, 1.0 if i % 2 else -1.0)
    for j, i in enumerate(put("below", 4)):
        I["sigma"][i] = F32(min(max(float(I["sigma"][i]), 0.05), 1.5))
        aim(i, 1e-10 if j < 2 else 3e-10, 1.0 if j % 2 else -1.0)
        I["g"][..., i] = (np.abs(I["g"][..., i]) + F32(0.1)) * (1 if j % 2 else -1)
    for j, i in enumerate(put("far_below", 2)):
        I["y"][i] += F32(80.0)
        setm(i, 1.0)
        I["g"][..., i] = np.abs(I["g"][..., i]) * (1 if j else -1)
    # every other element must be clear of the band: move the ones that landed in it to the mode
    band = set(placed["band"])
    for _ in range(3):
        J = dict(I)
        stray = np.zeros(q, dtype=bool)
        for k in range(L):
            Jk = {n: (v[k] if n in ("mask", "noise", "g") and levels is not None else v) for n, v in J.items() if n != "g"}
            lr = _lik_raw64(Jk)
            stray |= (lr >= BAND[0]) & (lr <= BAND[1])
        stray[list(band)] = False
        if not stray.any():
            break
        I["y"][stray] = I["mu"][stray]
        if "y2" in I:
            I["y2"][stray] = 0
    if levels is not None:
        I["drq"] = _normal(rng, (L, q), 1.0)
        I["dyt"] = _normal(rng, q, 1.0)
        if case.o("y2"):
            I["dys"] = _normal(rng, q, 1.0)
    return I, placed


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(I, placed): I maps operand names to fp32 pattern arrays [.., Q] (element-wise families; ``expand`` gives [.., n_pix, C]),
    or to the family's own arrays (eb, ps2, up2).  Nothing in it is modified by the tests."""
    case = CASES[cid]
    rng, q = _rng(case), _n_unique(case)
    placed = {}
    if case.fam == "ew":
        op, n_in = case.op, EW_OPS[case.op][1]
        I = {f"in{k}": _normal(rng, q, 1.5) for k in range(n_in)}
        if op.startswith("GDN"):
            I = {k: _away_from_zero(v * 2) for k, v in I.items()}
            if op != "GDN_BWD_FIN":
                I["in1"] = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), q)).astype(F32)
        elif op in ("GELU_FWD", "GELU_BWD", "GATE_FWD", "GATE_BWD", "HTANH_FWD", "HTANH_BWD"):
            k = "in1" if op.startswith("GATE") else "in0"          # the argument of the transcendental: body, tails, zero
            I[k] = _normal(rng, q, 2.5)
            I[k][:6] = np.array([0.0, -0.0, 12.0, -12.0, 1e-4, -5.5], dtype=F32)[:min(6, q)]
            placed["special"] = list(range(6))
        elif op == "CLAMP_BWD":
            I["in0"] = np.clip(_normal(rng, q, 0.7) + F32(0.5), 0, 1).astype(F32)
            I["in0"][:6] = np.array([0.0, 1.0, TINY, np.nextafter(F32(1), F32(0)), -0.0, 0.5], dtype=F32)
            placed["edges"] = list(range(6))
        elif op == "REPARAM_BWD":
            b = F32(REPARAM_BOUND)
            I["in0"] = (b * np.exp(rng.uniform(-1.5, 1.5, q))).astype(F32)
            I["in1"] = _away_from_zero(I["in1"])
            I["in0"][:4] = np.array([b, b, np.nextafter(b, F32(0)), np.nextafter(b, F32(0))], dtype=F32)
            I["in1"][:4] = np.array([0.75, -0.75, 0.75, -0.75], dtype=F32)
            placed["edges"] = list(range(4))
        elif op == "MASK_SPLIT":
            I["in0"] = _away_from_zero(I["in0"])
            m = (rng.uniform(size=q) > 0.4).astype(F32)
            frac = rng.uniform(size=q) < 0.2
            I["in1"] = np.where(frac, rng.uniform(0.01, 0.99, q), m).astype(F32)
        elif op == "AXPY":
            I = {k: _away_from_zero(v) for k, v in I.items()}
    elif case.fam == "axpy":
        n = case.o("jobs")
        I = {}
        for j in range(n):
            qj = q if j == 0 else BASE[0] * BASE[1] * BASE[2] * 8          # over-cap: the first job is the long one
            I[f"a{j}"], I[f"b{j}"] = _away_from_zero(_normal(rng, qj, 1.5)), _away_from_zero(_normal(rng, qj, 1.5))
    elif case.fam == "leaky":
        I = {"in0": _normal(rng, q, 1.0), "in1": _away_from_zero(_normal(rng, q, 1.5))}
        I["in0"][:4] = np.array([0.0, -0.0, TINY, -TINY], dtype=F32)
        placed["edges"] = list(range(4))
    elif case.fam == "mul":
        I = {"in0": _away_from_zero(_normal(rng, q, 1.5)), "in1": _away_from_zero(_normal(rng, q, 1.5))}
    elif case.fam == "gauss":
        I, placed = _draw_gauss(case, rng, q)
    elif case.fam == "levels":
        I, placed = _draw_gauss(case, rng, q, levels=case.o("levels"))
    elif case.fam == "eb":
        I, placed = _draw_eb(case, rng)
    elif case.fam == "ps2":
        B, H, W = case.shape
        I = {"src": _normal(rng, (B, 2 * H, 2 * W, case.C), 1.0)}
    elif case.fam == "up2":
        B, H, W = case.shape
        I = {"src": _away_from_zero(_normal(rng, (B, H, W, case.C), 1.0))}
    else:
        raise KeyError(case.fam)
    for v in I.values():
        v.setflags(write=False)
    return I, placed


# ---------------------------------------------------------------------------------------------------------------- eb inputs
EB_ODD_CHANNEL = 0           # the channel whose five biases are zero (C >= 5: channel 1 keeps its biases)
EB_ZERO_PIX = 3              # pixels with z + noise == 0 at the END of that channel (so that dropping them moves no other pixel)


def _draw_eb(case, rng):
    C, N = case.C, case.n_pix
    P = []
    for i, shp in enumerate(EB_SHAPES):
        n = shp[0] * shp[1]
        kind = i % 3 if i < 14 else 3
        if kind == 0:
            a = rng.standard_normal((C, n)) * 0.8
        elif kind == 1:
            a = rng.uniform(-0.5, 0.5, (C, n))
        elif kind == 2:
            a = rng.standard_normal((C, n)) * 0.5
        else:
            a = np.tile(np.array([-10.0, 0.0, 10.0]), (C, 1))
        P.append(a.astype(F32))
    oc = EB_ODD_CHANNEL if C > 1 else None
    if C == 1 and N >= 100:
        oc = 0                                                    # the single channel is the odd one at the larger sizes
    if oc is not None:
        for i in range(5):
            P[3 * i + 1][oc] = 0.0
    if C >= 5:
        P[3][C - 1, 4] = F32(21.0)                                # softplus above its threshold (x > 20: the identity)
    z = _normal(rng, (C, N), 3.0)
    noise = (rng.uniform(size=(C, N)) - 0.5).astype(F32)
    g = _normal(rng, (C, N), 1.0)
    placed = {"odd_channel": oc, "zero_pix": []}
    if oc is not None and N > EB_ZERO_PIX + 1:
        for p in range(N - EB_ZERO_PIX, N):
            noise[oc, p] = F32(0.25) * (1 if p % 2 else -1)
            z[oc, p] = -noise[oc, p]
            placed["zero_pix"].append(p)
        g[oc, N - 1] = -abs(g[oc, N - 1]) - F32(0.1)               # a negative gradient passes the bound and still meets sign = 0
    params = np.concatenate([a.reshape(-1) for a in P])
    # the likelihood bound: far tails are clear-below (both signs of g).  Strays in the band are moved to the mode, and so are
    # pixels with a logit of 80 ... 120: there exp() leaves the fp32 range and a sigmoid is subnormal, which the one-normal
    # floor of the bound (times the network's gain) does not cover — the inputs keep out of it, as the exact operations' do.
    def probe(zz):
        o = eb_body(Tape("f64"), eb_split(params, C), zz, noise)
        lr = o["lik_raw"].numpy()
        return lr, np.logical_or(*[(lg.numpy() > 80.0) & (lg.numpy() < 120.0) for lg in o["logits"]])
    if N >= 100:
        c = min(1, C - 1)
        for p, sgn in ((0, 1.0), (1, -1.0)):
            for mag in (45.0, 70.0, 110.0, 170.0, 260.0):
                z[c, p] = F32(sgn * mag)
                lr, sub = probe(z)
                if lr[c, p] < BAND[0] and not sub[c, p]:
                    break
        g[c, 0], g[c, 1] = F32(0.8), F32(-0.8)
        placed["far_below"] = [(c, 0), (c, 1)]
    for cand in (0.0, 0.3, -0.3, 1.0, -1.0, 0.1):                     # (the steep channel can sit in the band at its mode too)
        lr, sub = probe(z)
        stray = ((lr >= BAND[0]) & (lr <= BAND[1])) | sub
        if not stray.any():
            break
        z[stray] = (cand - noise[stray]).astype(F32)
    placed["band"] = []
    if N >= 100 and C >= 5:                                       # in-band: bisect z of a few pixels of channel 2 onto the bound
        c = 2
        for p, target in ((2, 0.7e-9), (3, 1.0e-9), (4, 1.6e-9)):
            f = lambda zz: float(eb_body(Tape("f64"), eb_split(params, C)[:0] + [a[c:c + 1] for a in eb_split(params, C)],
                                         np.array([[zz]], dtype=np.float64), np.zeros((1, 1)))["lik_raw"][0, 0])
            lo, hi = 0.0, 200.0
            if not f(hi) < target < f(lo):
                continue
            for _ in range(80):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if f(mid) > target else (lo, mid)
            noise[c, p] = 0.0
            z[c, p] = F32(lo)
            if BAND[0] <= f(float(z[c, p])) <= BAND[1]:
                placed["band"].append((c, p))
            else:
                z[c, p] = 0
    return {"params": params, "z": z, "noise": noise, "g": g}, placed


# ====================================================================================================== references
@dataclasses.dataclass
class Ref:
    ref64: np.ndarray
    ref32: np.ndarray
    A: np.ndarray = None          # budget (None for exact operations)
    exact: bool = False
    alt64: np.ndarray = None      # the other branch of the likelihood bound (in-band elements may take it)
    band: np.ndarray = None       # bool: in-band elements

    def ratio(self, got, k_floor=True):
        """worst (|got - ref64| - 2^-126) / (2^-24 A) and where; in-band elements against the nearer branch"""
        err = np.abs(np.asarray(got, dtype=np.float64) - self.ref64)
        if self.alt64 is not None and self.band is not None and self.band.any():
            err = np.where(self.band, np.minimum(err, np.abs(np.asarray(got, dtype=np.float64) - self.alt64)), err)
        over = np.maximum(err - FLOOR, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rat = np.where(over > 0, over / (U24 * self.A), 0.0)
        rat = np.where(np.isfinite(np.asarray(got, dtype=np.float64)), rat, np.inf)
        i = int(np.argmax(rat)) if rat.size else 0
        return (float(rat.reshape(-1)[i]) if rat.size else 0.0), i


def _run_modes(body, exact=False):
    """body(T, J) -> dict of tensors.  Returns {out: (ref64, ref32, A)} as numpy."""
    res = {}
    outs64 = body(Tape("f64"), None)
    outs32 = {k: v.to(torch.float32) for k, v in body(Tape("f32e" if exact else "f32"), None).items()}
    Tb = Tape("budget")
    outsb = body(Tb, None)
    for k in outs64:
        res[k] = (outs64[k].detach().numpy(), outs32[k].detach().numpy(), Tb.budget_of(outsb[k]))
    return res


def _ew_like_body(case, I, mut=()):
    """the body of an element-wise family over the pattern arrays, as a function of the tape"""
    fam = case.fam
    if fam == "ew":
        code, n_in, n_out = EW_OPS[case.op]
        coef = AXPY_COEF if case.op == "AXPY" else (REPARAM_BOUND if case.op == "REPARAM_BWD" else 0.0)
        return lambda T, _: {f"out{k}": v for k, v in enumerate(ew_body(T, code, [T.inp(I[f"in{j}"]) for j in range(n_in)], coef, case.o("flag")))}
    if fam == "leaky":
        return lambda T, _: {"out0": leaky_body(T, [T.inp(I["in0"]), T.inp(I["in1"])])[0]}
    if fam == "mul":
        return lambda T, _: {"out0": mul_body(T, [T.inp(I["in0"]), T.inp(I["in1"])])[0]}
    raise KeyError(fam)


def _gauss_in(T, I, names):
    return {k: T.inp(I[k]) for k in names if k in I}


@functools.lru_cache(maxsize=None)
def reference(cid):
    """{output name: Ref} of a case, arrays in the family's logical shape ([.., n_pix, C] for element-wise families).  Computed
    once and shared; nothing in it is modified by the tests."""
    case = CASES[cid]
    I, placed = inputs(cid)
    fam = case.fam
    out = {}
    if fam in ("ew", "leaky", "mul"):
        exact = fam != "ew" or case.op in EXACT_EW
        for k, (r64, r32, A) in _run_modes(_ew_like_body(case, I), exact).items():
            out[k] = Ref(expand(case, r64), expand(case, r32), None if exact else expand(case, A), exact)
    elif fam == "axpy":
        for j in range(case.o("jobs")):
            coef = float(F32(0.5 * (j + 1) * (-1) ** j))
            a, b = torch.tensor(I[f"a{j}"]), torch.tensor(I[f"b{j}"])
            r32 = (a.double() + (coef * b.double()).float().double()).float().numpy()
            sub = case if j == 0 else Case("-", "axpy", "axpy_group", BASE, 8)
            out[f"a{j}"] = Ref(expand(sub, (a.double() + coef * b.double()).numpy()), expand(sub, r32), None, True)
    elif fam in ("gauss", "levels"):
        names = ("y", "y2", "mu", "sigma", "mask", "noise", "g", "drq", "dyt", "dys")
        body = gauss_body if fam == "gauss" else levels_body
        band = np.zeros(_n_unique(case), dtype=bool)
        band[placed["band"]] = True
        for bwd in (False, True):
            use = [n for n in names if bwd or n not in ("g", "drq", "dyt", "dys")]
            res = _run_modes(lambda T, _: body(T, _gauss_in(T, I, use), bwd))
            alt = {k: (body(Tape("f64"), _gauss_in(Tape("f64"), I, use), bwd, passes=True)[k].numpy(),
                       body(Tape("f64"), _gauss_in(Tape("f64"), I, use), bwd, passes=False)[k].numpy()) for k in res}
            Tp = Tape("budget")                              # an in-band element is budgeted on the passing branch (the bound itself has none)
            outp = body(Tp, _gauss_in(Tp, I, use), bwd, passes=True)
            if not bwd and fam == "levels":                  # rq is exact: its float32 statement from the emulation
                Te = Tape("f32e")
                res["rq"] = (res["rq"][0], body(Te, _gauss_in(Te, I, use), bwd)["rq"].to(torch.float32).numpy(), res["rq"][2])
            for k, (r64, r32, A) in res.items():
                other = np.where(alt[k][0] == r64, alt[k][1], alt[k][0])
                bnd = np.broadcast_to(band, r64.shape)
                A = np.where(bnd, np.maximum(A, Tp.budget_of(outp[k])), A)
                out[k] = Ref(expand(case, r64), expand(case, r32), expand(case, A), k == "rq", expand(case, other), expand(case, bnd))
    elif fam == "eb":
        out = _eb_reference(case, I, placed)
    elif fam == "ps2":
        r = ps2_unshuffle_ref(I["src"])
        out["dst"] = Ref(r.astype(np.float64), r, None, True)
    elif fam == "up2":
        r = upsample2_zero_ref(I["src"])
        out["dst"] = Ref(r.astype(np.float64), r, None, True)
    return out


def eb_flat(dpar, C, dtype):
    """{key: [C]} -> the flat parameter block's layout (the three quantile gradients: zero)"""
    cols = {}
    for key in eb_keys():
        cols.setdefault((key[0], key[1]), []).append(np.asarray(dpar[key], dtype=dtype))
    parts = []
    for i in range(5):
        for kind in ("m", "b", "f"):
            if (kind, i) in cols:
                parts.append(np.stack(cols[(kind, i)], axis=1).reshape(-1))
    parts.append(np.zeros(3 * C, dtype=dtype))
    return np.concatenate(parts)


def _eb_reference(case, I, placed):
    C, N = case.C, case.n_pix
    P = eb_split(I["params"], C)
    run = lambda T, **kw: eb_body(T, P, I["z"], I["noise"], I["g"], **kw)
    o64, o32, ob = run(Tape("f64")), run(Tape("f32")), run(Tape("run"))
    band = np.zeros((C, N), dtype=bool)
    for c, p in placed["band"]:
        band[c, p] = True
    alt = (run(Tape("f64"), passes=True), run(Tape("f64"), passes=False))
    res = {}
    obp = run(Tape("run"), passes=True) if band.any() else ob     # an in-band pixel is budgeted on the passing branch
    for k in ("lik", "dz"):
        r64 = o64[k].numpy()
        other = np.where(alt[0][k].numpy() == r64, alt[1][k].numpy(), alt[0][k].numpy())
        res[k] = Ref(r64, o32[k].numpy(), np.maximum(ob[k].e.numpy(), obp[k].e.numpy()), False, other, band)
    n_sum = eb_sum_terms(N)
    A = {key: np.maximum(ob["dparams"][key].e.numpy(), obp["dparams"][key].e.numpy())
         + n_sum * np.maximum(alt[0]["terms"][key].numpy(), o64["terms"][key].numpy()) for key in eb_keys()}
    flat = lambda o, dt: eb_flat({k: v.numpy() for k, v in o["dparams"].items()}, C, dt)
    res["dparams"] = Ref(flat(o64, np.float64), flat(o32, F32), eb_flat(A, C, np.float64))
    if placed["band"]:                                            # an in-band pixel moves its channel's sums with its branch
        a0, a1 = flat(alt[0], np.float64), flat(alt[1], np.float64)
        res["dparams"].alt64 = np.where(a0 == res["dparams"].ref64, a1, a0)
        res["dparams"].band = (a0 != a1)
    return res


# ====================================================================================================== K
def ops_of_cases():
    seen = []
    for c in CASES.values():
        if c.op not in seen:
            seen.append(c.op)
    return seen


@functools.lru_cache(maxsize=None)
def k_cpu(op):
    """{output: worst ratio of ref32 against ref64} over the contract's cases of one operation (budget outputs only)."""
    worst = {}
    for cid, case in CASES.items():
        if case.op != op:
            continue
        for name, ref in reference(cid).items():
            if ref.exact:
                continue
            key = name if case.fam != "ew" or not case.op.startswith("GDN") else f"{name}/flag{case.o('flag')}"
            worst[key] = max(worst.get(key, 0.0), ref.ratio(ref.ref32)[0])
    return worst


def k_of(op, name):
    return max(K_FACTOR * k_cpu(op).get(name, 0.0), K_FLOOR)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)
