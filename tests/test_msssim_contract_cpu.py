"""The float64 contract of the MS-SSIM distortion (tests/msssim_contract.py) checked without a GPU: its value against
oracle/msssim_oracle.py, its closed-form backward against autograd, the relu contract, and the loss classes' ``metric``
argument."""
import math

import pytest
import torch

import msssim_contract as MC
import msssim_oracle as MO

@pytest.mark.parametrize("cid", [c for c in MC.CASES if MC.CASES[c][1] != "relu"])
def test_restatement_equals_the_oracle(cid):
    """(a) is oracle/msssim_oracle.py: the mean over planes equals ``ms_ssim`` to 1e-12 wherever no plane sits at the relu."""
    x, y, _ = MC.inputs(cid)
    got = float(MC.ms_ssim_planes(x.double(), y.double()).mean())
    want = MO.ms_ssim(x, y)
    assert abs(got - want) <= 1e-12, (got, want)
    if MC.CASES[cid][1] == "identical":
        assert abs(got - 1.0) <= 1e-12


def test_relu_batch_equals_the_oracle_value():
    """With one image at the relu the VALUE still equals the oracle's (relu(m)^w = 0 there); only the gradient differs."""
    x, y, _ = MC.inputs("patch256-relu")
    got = MC.ms_ssim_planes(x.double(), y.double())
    assert abs(float(got.mean()) - MO.ms_ssim(x, y)) <= 1e-12
    assert float(got[MC.RELU_IMAGE].abs().max()) == 0.0 and float(got.min(1).values.max()) > 0.0


@pytest.mark.parametrize("cid", list(MC.CASES))
def test_closed_form_backward_equals_autograd(cid):
    """(b) equals autograd of (a).  Both are float64 evaluations of the same derivative in different association orders:
    the difference is rounding, 2^-53 times the ~1e3 terms of size <= scale that make up an element — 1e-9 of max|g|
    (of the terms' scale where the exact gradient is 0) leaves four decades."""
    x, y, gout = MC.inputs(cid)
    _, want = MC.value_and_grad(x, y, gout)
    got, scale = MC.closed_form_grad(x, y, gout)
    ref = float(scale.max()) if MC.CASES[cid][1] == "identical" else float(want.abs().max())
    assert ref > 0
    assert float((got - want).abs().max()) <= 1e-9 * ref, (float((got - want).abs().max()), ref)
    assert bool((scale >= got.abs() * (1 - 1e-12)).all())


def test_relu_plane_has_finite_zero_value_and_gradient():
    x, y, gout = MC.inputs("patch256-relu")
    m = MC.level_means(x.double(), y.double())
    assert bool((m[:, MC.RELU_IMAGE] <= 0).any(0).all()), "the y = 1 - x image must reach the relu in every channel"
    val, grad = MC.value_and_grad(x, y, gout)
    assert torch.isfinite(grad).all() and torch.isfinite(val).all()
    assert float(val[MC.RELU_IMAGE]) == 0.0 and float(grad[MC.RELU_IMAGE].abs().max()) == 0.0
    others = [b for b in range(x.shape[0]) if b != MC.RELU_IMAGE]
    assert float(grad[others].abs().amax(dim=(1, 2, 3)).min()) > 0.0
    closed, _ = MC.closed_form_grad(x, y, gout)
    assert torch.isfinite(closed).all() and float(closed[MC.RELU_IMAGE].abs().max()) == 0.0


def test_fp32_reference_error_is_what_the_gpu_bound_uses():
    """The GPU bound is 4 x the fp32 CPU run's own error with a floor of 8 ulps: both parts are positive numbers and the
    fp32 run itself lies within it."""
    ref = MC.reference("odd161-noise0.1")
    assert ref["gmax"] > 0 and ref["grad_err32"] > 0
    assert MC.bound(ref["grad_err32"], ref["gscale"]) >= ref["grad_err32"]
    assert MC.bound(0.0, 1.0) == 8 * 2.0 ** -23


@pytest.mark.parametrize("name", ["ScalableRateDistortionLoss", "RateDistortionLoss", "DistortionLoss"])
def test_loss_classes_reject_an_unknown_metric(name):
    from vampic import finetune as ft
    cls = getattr(ft, name)
    with pytest.raises(ValueError):
        cls(device="cpu", metric="psnr")
    assert cls(device="cpu").metric == "mse" and cls(device="cpu", metric="ms-ssim", msssim_weight=2.0).msssim_weight == 2.0


def test_default_metric_is_the_mse_formula():
    """A hand-made output dict on the CPU: the default signature yields the reference's MSE losses, without an
    ``ms_ssim_loss`` key."""
    from vampic import finetune as ft
    gen = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 16, 16), generator=gen)
    x_hat = torch.rand((2, 2, 3, 16, 16), generator=gen)
    lik = {"y": torch.full((1, 2, 4, 2, 2), 0.5), "z": torch.ones((2, 4, 1, 1))}
    mse = ((x.unsqueeze(0) - x_hat) ** 2).mean(dim=(1, 2, 3, 4))
    bpp = 32 / (2 * 16 * 16)                                        # 32 likelihoods of 1/2: one bit each
    out = ft.ScalableRateDistortionLoss(lmbda_list=(0.005, 0.05), device="cpu")({"x_hat": x_hat, "likelihoods": lik}, x)
    assert "ms_ssim_loss" not in out and torch.equal(out["mse_loss"], mse)
    assert math.isclose(float(out["bpp_loss"]), bpp, rel_tol=1e-6)
    assert math.isclose(float(out["loss"]), bpp + 255 ** 2 * float((torch.tensor([0.005, 0.05]) * mse).mean()), rel_tol=1e-6)
    out = ft.RateDistortionLoss(device="cpu")({"x_hat": x_hat, "likelihoods": lik}, x, lmbda=0.01)
    assert math.isclose(float(out["loss"]), bpp + 255 ** 2 * 0.01 * float(mse.mean()), rel_tol=1e-6)
    out = ft.DistortionLoss(device="cpu")({"x_hat": x_hat[0], "likelihoods": lik}, x, lmbda=0.02)      # a single-quality output
    assert "ms_ssim_loss" not in out
    assert math.isclose(float(out["loss"]), 255 ** 2 * 0.02 * float(mse[0]), rel_tol=1e-6)


def test_ms_ssim_has_no_cpu_fallback():
    """Without a GPU the op raises (like every other op); with one, CPU tensors are a ValueError."""
    import vampic
    from vampic import _lib as L
    x = torch.zeros((1, 1, 161, 161))
    with pytest.raises((L.VamError, ValueError)):
        vampic.ops.ms_ssim(x, x)
