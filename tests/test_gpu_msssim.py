"""The differentiable MS-SSIM distortion on the GPU (csrc/msssim.hip, vampic.ops.ms_ssim, the ``metric="ms-ssim"`` losses)
against the float64 contract of tests/msssim_contract.py.

Bound (msssim_contract.bound): 4 x the error of the contract's own float32 CPU run against float64 on the same inputs,
with a floor of 8 fp32 ulps of the quantity's scale.  Nothing here compares with the reference implementation of the
codec, which has no MS-SSIM loss; MS-SSIM itself stays unpinned to the pytorch_msssim package (absent offline)."""
import argparse
import warnings

import pytest
import torch

import msssim_contract as MC
from conftest import README_ARGS, record_measurement

pytestmark = pytest.mark.gpu


def _run(x, y, gout):
    """ops.ms_ssim forward and backward: (value [B] float32, gradient [B,C,H,W] float32), both on the CPU."""
    from vampic import ops
    yd = y.cuda().requires_grad_(True)
    val = ops.ms_ssim(x.cuda(), yd)
    assert val.dtype == torch.float32 and tuple(val.shape) == (x.shape[0],)
    (val * gout.cuda()).sum().backward()
    return val.detach().cpu(), yd.grad.cpu()


@pytest.mark.parametrize("cid", list(MC.CASES))
def test_value_and_gradient_against_the_float64_contract(cid):
    x, y, gout = MC.inputs(cid)
    ref = MC.reference(cid)
    val, grad = _run(x, y, gout)
    assert torch.isfinite(val).all() and torch.isfinite(grad).all()
    verr = float((val.double() - ref["val"]).abs().max())
    gerr = float((grad.double() - ref["grad"]).abs().max())
    vb, gb = MC.bound(ref["val_err32"], 1.0), MC.bound(ref["grad_err32"], ref["gscale"])
    record_measurement(f"ms_ssim {cid}", value_err=f"{verr:.3e}", value_err_fp32_cpu=f"{ref['val_err32']:.3e}",
                       value_ratio=round(verr / vb, 4), grad_err=f"{gerr:.3e}", grad_err_fp32_cpu=f"{ref['grad_err32']:.3e}",
                       grad_scale=f"{ref['gscale']:.3e}", grad_ratio=round(gerr / gb, 4))
    print(f"{cid}: value err {verr:.3e} (fp32 CPU {ref['val_err32']:.3e}, bound {vb:.3e}); gradient err {gerr:.3e} "
          f"(fp32 CPU {ref['grad_err32']:.3e}, scale {ref['gscale']:.3e}, bound {gb:.3e})")
    assert verr <= vb, (verr, vb)
    assert gerr <= gb, (gerr, gb)
    if MC.CASES[cid][1] == "identical":
        assert float((val - 1.0).abs().max()) <= vb


def test_relu_image_is_zero_and_leaves_the_others_alone():
    """The image with y = 1 - x (cs < 0): value 0, gradient all-zero and finite; the other images of the batch are bit-equal
    to the same images run without it."""
    x, y, gout = MC.inputs("patch256-relu")
    val, grad = _run(x, y, gout)
    r = MC.RELU_IMAGE
    assert float(val[r]) == 0.0
    assert torch.isfinite(grad[r]).all() and float(grad[r].abs().max()) == 0.0
    keep = [b for b in range(x.shape[0]) if b != r]
    val2, grad2 = _run(x[keep], y[keep], gout[keep])
    assert torch.equal(val[keep], val2) and torch.equal(grad[keep], grad2)
    assert float(val2.min()) > 0.0 and float(grad2.abs().amax(dim=(1, 2, 3)).min()) > 0.0


@pytest.mark.parametrize("cid", ["patch256-noise0.1", "odd161-noise0.1"])
def test_forward_and_backward_are_deterministic(cid):
    """No float atomics: the partial sums are combined in a fixed order, the pooled gradient is gathered."""
    x, y, gout = MC.inputs(cid)
    a, b = _run(x, y, gout), _run(x, y, gout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_msssim_per_image_agrees_with_compute_msssim():
    """The new forward against the evaluation metric's direct 121-tap kernel on single images (no bit identity claimed:
    the old kernel sums in another order), and against the contract per image."""
    from vampic.evaluate import compute_msssim, msssim_per_image
    cid = "even176x208-noise0.1"
    x, y, _ = MC.inputs(cid)
    ref = MC.reference(cid)
    got = msssim_per_image(x.cuda(), y.cuda())
    assert got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],)
    vb = MC.bound(ref["val_err32"], 1.0)
    assert float((got.cpu() - ref["val"]).abs().max()) <= vb
    for b in range(x.shape[0]):
        old = compute_msssim(x[b:b + 1].cuda(), y[b:b + 1].cuda())
        assert abs(float(got[b]) - old) <= vb, (b, float(got[b]), old, vb)


@pytest.fixture(scope="module")
def loss_case():
    """x [2,3,192,192], x_hat [2,2,3,192,192] (two levels), likelihoods of ones and halves, and the contract's value and
    per-image gradient (upstream 1 per image) of the 4 (level, image) pairs."""
    x = MC.smooth_field(2, 3, 192, 192, 77)
    x_hat = torch.stack([MC.noisy(x, 0.1, 78), MC.noisy(x, 0.03, 79)], 0)
    lik = {"y": torch.full((1, 2, 8, 12, 12), 0.5), "z": torch.ones((2, 4, 3, 3))}
    xx, yy = x.repeat(2, 1, 1, 1), x_hat.reshape(4, 3, 192, 192)
    val, grad = MC.value_and_grad(xx, yy, torch.ones(4), torch.float64)
    val32, grad32 = MC.value_and_grad(xx, yy, torch.ones(4), torch.float32)
    return {"x": x, "x_hat": x_hat, "lik": lik, "val": val.view(2, 2), "grad": grad.view(2, 2, 3, 192, 192),
            "val_err32": float((val32.double() - val).abs().max()), "grad_err32": float((grad32.double() - grad).abs().max()),
            "bpp": 2 * 8 * 12 * 12 / (2 * 192 * 192)}


@pytest.mark.parametrize("name", ["ScalableRateDistortionLoss", "RateDistortionLoss", "DistortionLoss"])
def test_loss_classes_with_ms_ssim(name, loss_case):
    """loss = bpp_loss + msssim_weight * mean_l(lambda_l * (1 - msssim_l)) (DistortionLoss: the distortion term alone);
    d loss / d x_hat[l, b] = -msssim_weight * lambda_l / L / B * d ms_ssim(x_b, x_hat[l, b]) / d x_hat[l, b]."""
    from vampic import finetune as ft
    c = loss_case
    wgt, L_, B_ = 3.0, 2, 2
    x, lik = c["x"].cuda(), {k: v.cuda() for k, v in c["lik"].items()}
    x_hat = c["x_hat"].cuda().requires_grad_(True)
    if name == "ScalableRateDistortionLoss":
        lams = torch.tensor([0.2, 1.5], dtype=torch.float64)
        out = ft.ScalableRateDistortionLoss(lmbda_list=lams.tolist(), device="cuda", metric="ms-ssim", msssim_weight=wgt)(
            {"x_hat": x_hat, "likelihoods": lik}, x)
    else:
        lams = torch.tensor([0.7, 0.7], dtype=torch.float64)
        with warnings.catch_warnings():                 # DistortionLoss's reported MSE broadcasts the target over the levels
            warnings.simplefilter("ignore")
            out = getattr(ft, name)(device="cuda", metric="ms-ssim", msssim_weight=wgt)({"x_hat": x_hat, "likelihoods": lik}, x, lmbda=0.7)
    out["loss"].backward()
    ms = c["val"].mean(1)                                                   # per level
    vb = MC.bound(c["val_err32"], 1.0)
    assert tuple(out["ms_ssim_loss"].shape) == (2,)
    assert float((out["ms_ssim_loss"].detach().cpu().double() - ms).abs().max()) <= vb
    mse = ((c["x"].unsqueeze(0) - c["x_hat"]).double() ** 2).mean(dim=(1, 2, 3, 4))
    got_mse = out["mse_loss"].detach().cpu().double()
    assert not out["mse_loss"].requires_grad
    want_mse = mse.mean() if name == "DistortionLoss" else mse
    assert float((got_mse - want_mse).abs().max()) <= 1e-5 * float(mse.max())
    dist = wgt * float((lams * (1.0 - ms)).mean())
    want = dist if name == "DistortionLoss" else c["bpp"] + dist
    assert abs(float(out["bpp_loss"]) - c["bpp"]) <= 1e-6 * c["bpp"]
    # the loss is an fp32 number of size `want`; its MS-SSIM part carries the value bound times its factor
    got = float(out["loss"].detach())
    assert abs(got - want) <= wgt * float(lams.max()) * vb + 4 * MC.ULP32 * abs(want), (got, want)
    factor = (-wgt * lams / L_ / B_).reshape(2, 1, 1, 1, 1)
    want_g = c["grad"] * factor
    gerr = float((x_hat.grad.cpu().double() - want_g).abs().max())
    gb = float(factor.abs().max()) * MC.bound(c["grad_err32"], float(c["grad"].abs().max()))
    print(f"{name}: x_hat.grad err {gerr:.3e}, bound {gb:.3e}")
    assert gerr <= gb, (gerr, gb)


def _train_model():
    import vampic
    from vampic import synth
    net = vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu")
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
    return net.cuda().train()


def test_first_train_step_with_ms_ssim():
    """One real first_train step (README configuration, synthetic weights, 1x3x192x192, qualities (0, 10), fixed noise)
    with ``metric="ms-ssim"``: finite loss, a finite gradient on every parameter, the step repeated from the same state
    reproduces every gradient bit for bit, and the gradients are not the ``metric="mse"`` step's.  No comparison with the
    reference: it has no such loss."""
    from vampic import synth
    from vampic.finetune import ScalableRateDistortionLoss, first_train_setup, first_train_step
    net = _train_model()
    params = first_train_setup(net)
    start = [p.detach().clone() for p in params]
    x = synth.synth_image(1, 192, 192, seed=21).cuda()
    noise = {"y": synth.uniform((1, 640, 12, 12), 501) - 0.5, "z": synth.uniform((1, 192, 3, 3), 502) - 0.5}

    def step(metric):
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        opt = torch.optim.SGD(params, lr=1e-6)
        crit = ScalableRateDistortionLoss(lmbda_list=[0.0055, 0.04], device="cuda", metric=metric, msssim_weight=100.0)
        c = first_train_step(net, crit, x, opt, (0, 10), clip_max_norm=0.0, noise=noise)
        assert all(p.grad is not None for p in params)
        return c, torch.cat([p.grad.reshape(-1) for p in params]).clone()

    c1, g1 = step("ms-ssim")
    c2, g2 = step("ms-ssim")
    c3, g3 = step("mse")
    assert torch.isfinite(c1["loss"]).all() and torch.isfinite(g1).all()
    assert tuple(c1["ms_ssim_loss"].shape) == (2,) and tuple(c1["mse_loss"].shape) == (2,)
    record_measurement("first_train step with ms-ssim", ms_ssim=[round(float(v), 6) for v in c1["ms_ssim_loss"]],
                       loss=float(c1["loss"]), loss_mse=float(c3["loss"]))
    assert float(c1["loss"]) == float(c2["loss"]) and torch.equal(g1, g2)
    assert "ms_ssim_loss" not in c3 and not torch.equal(g1, g3)


def test_error_paths():
    from vampic import ops
    from vampic.evaluate import msssim_per_image
    a = torch.zeros((1, 3, 160, 300), device="cuda")
    with pytest.raises(ValueError):
        ops.ms_ssim(a, a)                                                         # smaller side <= 160
    with pytest.raises(ValueError):
        msssim_per_image(a, a)
    b = torch.zeros((1, 3, 176, 176), device="cuda")
    with pytest.raises(ValueError):
        ops.ms_ssim(b, torch.zeros((1, 3, 176, 177), device="cuda"))              # shape mismatch
    with pytest.raises(ValueError):
        ops.ms_ssim(b.cpu(), b.cpu())                                             # not CUDA tensors
    with pytest.raises(ValueError):
        ops.ms_ssim(b.clone().requires_grad_(True), b)                            # the target is not differentiated
