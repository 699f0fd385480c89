"""The contract of the differentiable MS-SSIM distortion (csrc/msssim.hip, vampic.ops.ms_ssim) in float64.  TEST HELPER.

(a) ``ms_ssim_planes`` / ``ms_ssim_images``: oracle/msssim_oracle.py restated so that the result stays a tensor — autograd
    of it is the reference gradient.  Per plane = (image, channel): V = prod_l relu(m_l)^w_l.  The one place where it
    departs from the oracle's expression is the relu contract: a plane with any m_l <= 0 has value 0 and gradient
    exactly 0 (pytorch_msssim's expression differentiates relu(m)^w at the kink and can give NaN there).
(b) ``closed_form_grad``: the kernel's closed-form backward (coefficient maps G_my, G_syy, G_sxy, correlation with the
    transposed Gaussian, gather through the pool), written out in float64 without autograd.
(c) input generators and the case table shared by the CPU and the GPU tests.

Bounds.  The fp32 error of sxx - mx^2 relative to c2 = 9e-4 cannot be derived in advance, so the GPU tests measure the
reference's OWN fp32 error instead: (a) with its autograd run in float32 on the CPU on the same inputs, against (a) in
float64.  The kernel is allowed 4 x that (its summation order differs: LDS separable passes against ATen's conv), with
a floor of 8 fp32 ulps of the quantity's scale (``bound``)."""
import functools

import torch
import torch.nn.functional as F

import msssim_oracle as MO

WEIGHTS = MO.WEIGHTS
ULP32 = 2.0 ** -23


def window(dtype=torch.float64) -> torch.Tensor:
    """The oracle's window: built in float32 (as pytorch_msssim does), then cast."""
    return MO.gaussian_window().to(dtype)


def _filter(x, win):
    C = x.shape[1]
    w = win.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1)
    return F.conv2d(F.conv2d(x, w.transpose(2, 3), groups=C), w, groups=C)          # along H, then along W


def _filter_t(gmap, win):
    """Correlation with the transposed Gaussian, "full" extent: the adjoint of ``_filter``."""
    C = gmap.shape[1]
    w = win.flip(0).reshape(1, 1, 1, -1).repeat(C, 1, 1, 1)
    return F.conv2d(F.conv2d(gmap, w.transpose(2, 3), groups=C, padding=(10, 0)), w, groups=C, padding=(0, 10))


def _pool(x):
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def _moments(x, y, win):
    mx, my = _filter(x, win), _filter(y, win)
    return mx, my, _filter(x * x, win), _filter(y * y, win), _filter(x * y, win)


def level_means(x, y, data_range=1.0):
    """[5, B, C]: the mean cs map of levels 0-3 and the mean ssim map of level 4, in the dtype of the inputs."""
    win = window(x.dtype)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    out = []
    for lvl in range(5):
        mx, my, sxx, syy, sxy = _moments(x, y, win)
        cs = (2 * (sxy - mx * my) + c2) / ((sxx - mx * mx) + (syy - my * my) + c2)
        if lvl == 4:
            cs = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
        out.append(cs.flatten(2).mean(-1))
        if lvl < 4:
            x, y = _pool(x), _pool(y)
    return torch.stack(out, 0)


def ms_ssim_planes(x, y, data_range=1.0):
    """(a): V per plane, [B, C], differentiable in y.  Zero value and zero gradient for a plane with any m_l <= 0."""
    m = level_means(x, y, data_range)
    pos = (m > 0).all(0)
    safe = torch.where(pos.unsqueeze(0), m, torch.ones_like(m))
    w = torch.tensor(WEIGHTS, dtype=m.dtype).reshape(-1, 1, 1)
    return torch.prod(safe ** w, dim=0) * pos.to(m.dtype)


def ms_ssim_images(x, y, data_range=1.0):
    """What vampic.ops.ms_ssim returns: the mean over channels, [B]."""
    return ms_ssim_planes(x, y, data_range).mean(1)


def value_and_grad(x, y, gout, dtype=torch.float64):
    """(a) and its autograd in ``dtype``: (ms_ssim [B], d sum_b gout[b] ms_ssim[b] / dy)."""
    xd, yd = x.to(dtype), y.to(dtype).clone().requires_grad_(True)
    val = ms_ssim_images(xd, yd)
    (val * gout.to(dtype)).sum().backward()
    return val.detach(), yd.grad


def closed_form_grad(x, y, gout, data_range=1.0):
    """(b): the kernel's backward in float64.  Returns (grad, scale) with ``scale`` [B,C,H,W] the same expression with every
    term replaced by its magnitude, i.e. what the result's rounding error is relative to where the terms cancel (y = x)."""
    x, y, gout = x.double(), y.double(), gout.double()
    B, C = x.shape[:2]
    win = window()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    m = level_means(x, y, data_range)
    pos = (m > 0).all(0)
    w = torch.tensor(WEIGHTS, dtype=torch.float64).reshape(-1, 1, 1)
    V = torch.where(pos, torch.prod(torch.where(pos.unsqueeze(0), m, torch.ones_like(m)) ** w, dim=0), torch.zeros_like(m[0]))
    dvdm = torch.where(pos.unsqueeze(0), w * V / torch.where(pos.unsqueeze(0), m, torch.ones_like(m)), torch.zeros_like(m))
    pyr = [(x, y)]
    for _ in range(4):
        pyr.append((_pool(pyr[-1][0]), _pool(pyr[-1][1])))
    g_coarse = s_coarse = None
    for lvl in range(4, -1, -1):
        xl, yl = pyr[lvl]
        H, W = xl.shape[2:]
        mx, my, sxx, syy, sxy = _moments(xl, yl, win)
        a = (gout.reshape(B, 1) / C * dvdm[lvl] / ((H - 10) * (W - 10))).reshape(B, C, 1, 1)
        A1, B1 = 2 * mx * my + c1, mx * mx + my * my + c1
        A2, B2 = 2 * (sxy - mx * my) + c2, (sxx - mx * mx) + (syy - my * my) + c2
        cs, lum = A2 / B2, A1 / B1
        if lvl < 4:
            G_sxy, G_syy, direct = a * 2 / B2, -a * A2 / B2 ** 2, torch.zeros_like(mx)
        else:
            G_sxy, G_syy = a * lum * 2 / B2, -a * lum * A2 / B2 ** 2
            direct = a * cs * (2 * mx * B1 - 2 * my * A1) / B1 ** 2
        G_my = direct - 2 * my * G_syy - mx * G_sxy
        g = _filter_t(G_my, win) + 2 * yl * _filter_t(G_syy, win) + xl * _filter_t(G_sxy, win)
        s = (_filter_t(direct.abs() + 2 * (my * G_syy).abs() + (mx * G_sxy).abs(), win) + 2 * yl.abs() * _filter_t(G_syy.abs(), win)
             + xl.abs() * _filter_t(G_sxy.abs(), win))
        if g_coarse is not None:
            iy = (torch.arange(H) + H % 2) // 2
            ix = (torch.arange(W) + W % 2) // 2
            g = g + 0.25 * g_coarse[:, :, iy][:, :, :, ix]
            s = s + 0.25 * s_coarse[:, :, iy][:, :, :, ix]
        g_coarse, s_coarse = g, s
    return g_coarse, s_coarse


def bound(ref_err: float, scale: float) -> float:
    """4 x the reference's own fp32 error, floor 8 fp32 ulps of the quantity's scale."""
    return max(4.0 * ref_err, 8.0 * ULP32 * scale)


# ---------------------------------------------------------------------------------------------------------- (c) inputs
def smooth_field(B, C, H, W, seed):
    """A smooth field (a few low-frequency waves) plus noise (sigma 0.05), clamped to [0, 1]."""
    gen = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, H, dtype=torch.float64).reshape(1, 1, H, 1)
    xx = torch.linspace(0, 1, W, dtype=torch.float64).reshape(1, 1, 1, W)
    f = torch.full((B, C, H, W), 0.5, dtype=torch.float64)
    for _ in range(4):
        fy, fx = (torch.rand((B, C, 1, 1), generator=gen, dtype=torch.float64) * 6 for _ in range(2))
        ph = torch.rand((B, C, 1, 1), generator=gen, dtype=torch.float64) * 6.283185307179586
        f = f + 0.09 * torch.sin(fy * yy * 6.283185307179586 + fx * xx * 6.283185307179586 + ph)
    f = f + 0.05 * torch.randn((B, C, H, W), generator=gen, dtype=torch.float64)
    return f.clamp(0, 1).float()


def noisy(x, sigma, seed):
    gen = torch.Generator().manual_seed(seed)
    return (x.double() + sigma * torch.randn(x.shape, generator=gen, dtype=torch.float64)).float()


def constant_patches(B, C, H, W, seed, patch=16):
    """x and y piecewise constant on the same 16x16 patches with different levels: vx = vy = cov = 0 inside a patch, where
    cs = c2 / c2 is decided by cancellation alone."""
    gen = torch.Generator().manual_seed(seed)
    hp, wp = -(-H // patch), -(-W // patch)

    def up(levels):
        return levels.repeat_interleave(patch, 2).repeat_interleave(patch, 3)[:, :, :H, :W].contiguous()
    lx = torch.rand((B, C, hp, wp), generator=gen)
    ly = (lx + 0.1 * (torch.rand((B, C, hp, wp), generator=gen) - 0.5)).clamp(0, 1)
    return up(lx), up(ly)


SHAPES = {"odd161": (1, 1, 161, 161), "even176x208": (2, 3, 176, 208), "patch256": (4, 3, 256, 256)}

# case id -> (shape id, kind)
CASES = {}
for _sid in SHAPES:
    CASES[f"{_sid}-noise0.02"] = (_sid, "noise0.02")
    CASES[f"{_sid}-noise0.1"] = (_sid, "noise0.1")
CASES["even176x208-constant"] = ("even176x208", "constant")
CASES["odd161-identical"] = ("odd161", "identical")
CASES["even176x208-identical"] = ("even176x208", "identical")
CASES["patch256-relu"] = ("patch256", "relu")
RELU_IMAGE = 1                      # the image of the "relu" batch with y = 1 - x


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(x, y, gout) of a case: fp32 CPU tensors and the per-image upstream gradient of the gradient checks."""
    sid, kind = CASES[cid]
    B, C, H, W = SHAPES[sid]
    seed = 1000 + sorted(CASES).index(cid)
    x = smooth_field(B, C, H, W, seed)
    if kind.startswith("noise"):
        y = noisy(x, float(kind[5:]), seed + 500)
    elif kind == "constant":
        x, y = constant_patches(B, C, H, W, seed)
    elif kind == "identical":
        y = x.clone()
    elif kind == "relu":
        y = noisy(x, 0.02, seed + 500)
        y[RELU_IMAGE] = 1.0 - x[RELU_IMAGE]
    else:
        raise KeyError(kind)
    gout = torch.linspace(1.0, 0.5, B) if B > 1 else torch.ones(1)
    return x, y, gout


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Computed once per case and shared: float64 value and gradient of (a), the same in float32 on the CPU, and the
    reference's own fp32 errors.  Returns a dict; nothing in it is modified by the tests."""
    x, y, gout = inputs(cid)
    val, grad = value_and_grad(x, y, gout, torch.float64)
    val32, grad32 = value_and_grad(x, y, gout, torch.float32)
    gmax = float(grad.abs().max())
    _, scale = closed_form_grad(x, y, gout)
    # the scale of the gradient: its largest element; at y = x, where the exact gradient is 0 and the comparison is absolute,
    # the size of the terms that cancel
    gscale = float(scale.max()) if CASES[cid][1] == "identical" else gmax
    return {"val": val, "grad": grad, "gmax": gmax, "gscale": gscale,
            "val_err32": float((val32.double() - val).abs().max()), "grad_err32": float((grad32.double() - grad).abs().max())}
