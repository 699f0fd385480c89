"""First-stage training over quality lists [0, q1, ..., qL] on the GPU: the level kernels against the launches they
replace (bit for bit), the complete step against the oracle's restatement of the reference (tests/levels_oracle.py, held
to the reference's own run by tests/test_oracle_levels.py), the shared front end against the [0, q_k] plans, refusals,
and a short training loop."""
import argparse
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                              # noqa: E402
import vampic.synth as synth               # noqa: E402
from vampic import _lib as L, ops          # noqa: E402
import levels_oracle as LO                 # noqa: E402
from test_gpu_first_train import _compare_grads, _model, _rel   # noqa: E402

QS = [0, 2.5, 10]
LMBDA = [0.0055, 0.015, 0.04]


def _v(t):
    """NCHW cpu tensor -> NHWC View on the GPU."""
    return ops.from_nchw(t.cuda())


def _levels_of(view, n, B):
    return [ops.View(view.buf[k * B:(k + 1) * B], view.c0, view.C) for k in range(n)]


# ----------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("hw", [(4, 4), (16, 16), (32, 64)])       # the three register paths of the selection kernel
def test_level_masks_equal_separate_calls(hw):
    h, w = hw
    B, ns, C = 3, 4, 32
    sig = synth.normal((B, ns * C, h, w), 11).abs()
    sig[1] = torch.round(sig[1] * 4) / 4                   # ties
    sig[2, C:2 * C, 0, 0] = float("nan")                   # one segment holds a NaN
    prs = [0.0, 2.5, 5.0, 7.3, 10.0, 12.0, 0.01, 9.99]
    s_v = _v(sig)
    nl = len(prs)
    got = ops.new_view(nl * B, h, w, ns * C)
    thr = torch.empty(nl, B * ns, device="cuda")
    ops.variance_mask_levels(s_v, prs, got, n_slice=ns, thr=thr)
    for k, pr in enumerate(prs):
        want = ops.new_view(B, h, w, ns * C)
        t1 = torch.empty(B * ns, device="cuda")
        ops.variance_mask(s_v, pr, want, n_slice=ns, thr=t1)
        torch.cuda.synchronize()
        assert torch.equal(got.buf[k * B:(k + 1) * B], want.buf), pr
        assert torch.equal(thr[k].view(torch.int32), t1.view(torch.int32)) or \
            (torch.isnan(thr[k]) == torch.isnan(t1)).all() and torch.equal(thr[k][~torch.isnan(t1)], t1[~torch.isnan(t1)]), pr
    assert float(got.buf[2 * B + 2, ..., C:2 * C].abs().sum()) == 0.0      # NaN segment: all zero below pr 10


def _tail_inputs(B=2, h=8, w=8, d=64, nl=3, seed=40):
    y = synth.normal((B, 2 * d, h, w), seed) * 4
    mu = synth.normal((B, d, h, w), seed + 1) * 2
    sg = synth.normal((B, d, h, w), seed + 2).abs() * 0.5
    sg[0, :5] = 0.05                                        # below the 0.11 bound
    noise = synth.uniform((B, (nl + 1) * d, h, w), seed + 3) - 0.5
    y_v = _v(y)
    masks = ops.new_view(nl * B, h, w, d)
    ops.variance_mask_levels(_v(sg), [2.5, 5.0, 10.0][:nl], masks, n_slice=d // 32)
    return y_v, _v(mu), _v(sg), masks, _v(noise)


def test_fused_forward_equals_tail_and_train_per_level():
    B, d, nl = 2, 64, 3
    y_v, mu, sg, masks, noise = _tail_inputs(B=B, d=d, nl=nl)
    y_top, y_sub = y_v.window(d, d), y_v.window(0, d)
    rq = ops.new_view(nl * B, 8, 8, d)
    lik = ops.new_view(B, 8, 8, (nl + 1) * d)
    ops.gauss_levels_fwd(y_top, mu, sg, masks, noise.window(d, d), rq, lik.window(d, d), nl, y2=y_sub, noise_ls=d, lik_ls=d)
    for k, m in enumerate(_levels_of(masks, nl, B)):
        yh, junk, lk = ops.new_view(B, 8, 8, d), ops.new_view(B, 8, 8, d), ops.new_view(B, 8, 8, d)
        ops.gauss_tail(y_top, mu, sg, y2=y_sub, mask=m, yhat=yh, lik=junk)
        ops.gauss_train(y_top, mu, sg, noise.window((k + 1) * d, d), y2=y_sub, mask=m, lik=lk)
        torch.cuda.synchronize()
        assert torch.equal(rq.buf[k * B:(k + 1) * B], yh.buf), k
        assert torch.equal(lik.buf[..., (k + 1) * d:(k + 2) * d], lk.buf), k


@pytest.mark.parametrize("delta", [True, False])
def test_fused_backward_equals_unfused_sequence(delta):
    B, d, nl, h, w = 2, 64, 3, 8, 8
    y_v, mu, sg, masks, noise = _tail_inputs(B=B, d=d, nl=nl, seed=60)
    y_top, y_sub = y_v.window(d, d), (y_v.window(0, d) if delta else None)
    glik = _v(synth.normal((B, (nl + 1) * d, h, w), 70) * 3)
    d_rq = _v(synth.normal((nl * B, d, h, w), 71))
    dy0 = synth.normal((B, 2 * d, h, w), 72)
    # fused
    D_y = _v(dy0)
    gmu, dsg = ops.new_view(B, h, w, d), ops.new_view(B, h, w, d)
    ops.gauss_levels_bwd(y_top, mu, sg, masks, noise.window(d, d), glik.window(d, d), d_rq, gmu, dsg, D_y.window(d, d), nl,
                         y2=y_sub, dy_sub=D_y.window(0, d) if delta else None, noise_ls=d, glik_ls=d)
    # unfused, level by level: likelihood backward, mask split, the four accumulations, the levels' sums
    D_u = _v(dy0)
    G_t, S_t = ops.new_view(B, h, w, d, zero=True), ops.new_view(B, h, w, d, zero=True)
    for k, m in enumerate(_levels_of(masks, nl, B)):
        dmu_l, dsg_l, d_r, G = (ops.new_view(B, h, w, d) for _ in range(4))
        ops.gauss_train(y_top, mu, sg, noise.window((k + 1) * d, d), y2=y_sub, mask=m, grad_lik=glik.window((k + 1) * d, d),
                        dmu=dmu_l, dsigma=dsg_l)
        ops.ew(L.EW_MASK_SPLIT, [_levels_of(d_rq, nl, B)[k], m], [d_r, G])
        ops.ew(L.EW_AXPY, [G, dmu_l], [G], coef=1.0)
        ops.ew(L.EW_AXPY, [d_r, dmu_l], [d_r], coef=-1.0)
        ops.ew(L.EW_AXPY, [D_u.window(d, d), d_r], [D_u.window(d, d)], coef=1.0)
        if delta:
            ops.ew(L.EW_AXPY, [D_u.window(0, d), d_r], [D_u.window(0, d)], coef=-1.0)
        ops.ew(L.EW_AXPY, [G_t, G], [G_t], coef=1.0)
        ops.ew(L.EW_AXPY, [S_t, dsg_l], [S_t], coef=1.0)
    torch.cuda.synchronize()
    assert float(gmu.buf.abs().max()) > 0 and float(dsg.buf.abs().max()) > 0
    assert torch.equal(gmu.buf, G_t.buf)
    assert torch.equal(dsg.buf, S_t.buf)
    assert torch.equal(D_y.buf, D_u.buf)


# ----------------------------------------------------------------------------------------------- the complete step
def _inputs():
    from test_oracle_levels import levels_fixture_inputs
    return levels_fixture_inputs()


def _levels_plan(net, n_lv):
    return next(p for k, p in net._plans.items() if k[0] == "full_train" and k[4] == "levels" and k[-1] == n_lv)


_ORACLE: dict = {}


def _forced_levels_step(net, sd, x, ny, nz, qs, lmbda):
    pl = _levels_plan(net, len(qs) - 1)
    B = x.shape[0]
    nchw = lambda v: v.torch_nchw().detach().cpu()
    med = sd["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    mu_p = nchw(pl.mu_p)
    force = {"base_sym": torch.round(nchw(pl.yq) - nchw(pl.mu_b)), "z_sym": torch.round(nchw(pl.z_hat) - med),
             "prog_sym": [torch.round(r - mu_p) for r in nchw(pl.rq).split(B, 0)], "mask": list(nchw(pl.mask).split(B, 0))}
    hit = _ORACLE.get("last")
    if hit is not None and all(torch.equal(hit[1][k], force[k]) for k in ("base_sym", "z_sym")) and \
            all(torch.equal(a, b) for k in ("prog_sym", "mask") for a, b in zip(hit[1][k], force[k])):
        return hit[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = LO.first_train_step_levels(sd, x, qs, ny, nz, lmbda, force=force)
    _ORACLE["last"] = (ref, force)
    return ref


@pytest.mark.parametrize("use_graph", [False, True])
def test_levels_step_matches_oracle(use_graph):
    """forward(x, [0, 2.5, 10], training=True) with per-level noise, the 3-lambda ScalableRateDistortionLoss and backward with
    every parameter trainable, against the oracle's step at equal decisions: the bars of test_first_train_step_matches_reference."""
    from vampic.finetune import ScalableRateDistortionLoss
    net, sd = _model()
    net.use_graph = use_graph
    x, ny, nz = _inputs()
    out = net(x.cuda(), quality=QS, training=True, noise={"y": ny, "z": nz})
    assert tuple(out["x_hat"].shape) == (3, 2, 3, 64, 64)
    assert tuple(out["likelihoods"]["y_prog"].shape) == (2, 2, 640, 4, 4) and len(out["y_hat"]) == 3
    crit = ScalableRateDistortionLoss(lmbda_list=LMBDA, device="cuda")(out, x.cuda())
    crit["loss"].backward()
    ref = _forced_levels_step(net, sd, x, ny, nz, QS, LMBDA)
    n_grads = sum(1 for g in ref["grads"].values() if g is not None)
    joint, fam, worst = _compare_grads(net, ref["grads"])
    lik = {k: _rel(out["likelihoods"][k], ref["out"]["likelihoods"][k]) for k in ("y", "y_prog", "z")}
    print(f"levels graph={use_graph} likelihoods", {k: f"{v:.2e}" for k, v in lik.items()}, "x_hat", f"{_rel(out['x_hat'], ref['out']['x_hat']):.2e}",
          "joint gradient error", joint, "worst tensor", worst, {k: f"{v:.2e}" for k, v in fam.items()})
    for k in ("loss", "bpp_loss", "bpp_base", "bpp_scalable", "bpp_hype"):
        a, b = float(crit[k].detach().mean()), float(ref["crit"][k].mean())
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (k, a, b)
    assert _rel(crit["mse_loss"], ref["crit"]["mse_loss"]) <= 1e-4
    assert _rel(out["x_hat"], ref["out"]["x_hat"]) <= 1e-4
    for a, b in zip(out["y_hat"], ref["out"]["y_hat"]):
        assert _rel(a, b) <= 1e-4
    assert lik["y"] <= 1e-4 and lik["z"] <= 1e-4, lik
    # the progressive likelihoods: each level's are bit-identical to the [0, q_k] plan's (next test), whose own distance to
    # the oracle on these inputs is the same 2e-4 (measured: DESIGN.md section 9e) — the argument (r - mu) * m + noise is a
    # difference of numbers up to ~46 whose fp32 summation noise is ~1e-4 of its O(1) value
    assert lik["y_prog"] <= 3e-4, lik
    assert n_grads == 1065
    assert joint <= 2e-4, (joint, fam)
    for f, v in fam.items():
        assert v <= 5e-4, (f, v, fam)


def test_levels_share_the_front_end_of_the_two_level_plans():
    """Level k of the levels plan is the [0, q_k] plan's progressive pass on the same inputs and that level's noise block:
    mask, quantised residual and likelihoods bit for bit (same front end, same kernels' arithmetic), reconstructions to
    1e-6 (the LRP stacks and g_s[1] run as one batch of L * B images)."""
    net, sd = _model()
    x, ny, nz = _inputs()
    B, d = 2, 320
    out = net(x.cuda(), quality=QS, training=True, noise={"y": ny, "z": nz})
    pl = _levels_plan(net, 2)
    lv = {"mask": pl.mask.buf.clone(), "rq": pl.rq.buf.clone(), "lik": pl.lik.buf.clone(), "x_hat": out["x_hat"].detach().clone()}
    for k, q in enumerate(QS[1:], start=1):
        o2 = net(x.cuda(), quality=[0, q], training=True, noise={"y": torch.cat([ny[:, :d], ny[:, k * d:(k + 1) * d]], 1), "z": nz})
        p2 = next(p for kk, p in net._plans.items() if kk[0] == "full_train" and kk[4] == "multi")
        torch.cuda.synchronize()
        sl = slice((k - 1) * B, k * B)
        assert torch.equal(lv["mask"][sl], p2.mask.buf), q
        assert torch.equal(lv["rq"][sl], p2.rq.buf), q
        assert torch.equal(lv["lik"][..., :d], p2.lik.buf[..., :d]), q
        assert torch.equal(lv["lik"][..., k * d:(k + 1) * d], p2.lik.buf[..., d:]), q
        assert torch.equal(lv["x_hat"][0], o2["x_hat"][0].detach()), q
        assert _rel(lv["x_hat"][k], o2["x_hat"][1]) <= 1e-6, (q, _rel(lv["x_hat"][k], o2["x_hat"][1]))


def test_shared_noise_block_serves_every_level():
    """noise["y"] of [B, 2d]: one progressive block for every level (the no-grad forward's convention)."""
    net, sd = _model()
    x, ny, nz = _inputs()
    d = 320
    net(x.cuda(), quality=QS, training=True, noise={"y": ny[:, :2 * d], "z": nz})
    pl = _levels_plan(net, 2)
    got = pl.noise_y.buf.clone()
    torch.cuda.synchronize()
    want = torch.cat([ny[:, :2 * d], ny[:, d:2 * d]], 1).permute(0, 2, 3, 1).cuda()
    assert torch.equal(got, want)


def test_two_levels_policy_gives_all_ones_masks():
    net, sd = _model()
    x, ny, nz = _inputs()
    net(x.cuda(), quality=QS, mask_pol="two-levels", training=True, noise={"y": ny, "z": nz})
    pl = _levels_plan(net, 2)
    assert float(pl.mask.buf.min()) == 1.0


def test_levels_refusals(monkeypatch):
    net, sd = _model()
    x = synth.synth_image(2, 64, 64, seed=5).cuda()
    for qs in ([0, 0, 10], [0, 2.5, -1.0], [0] + [float(k) for k in range(1, L.VAM_MAX_MASK_LEVELS + 2)]):
        with pytest.raises(NotImplementedError):
            net(x, quality=qs, training=True)
    import sys
    monkeypatch.setattr(sys.modules["vampic.models"], "MAX_PLAN_PIXELS", 3 * 64 * 64)           # three 64x64 images per plan
    with pytest.raises(NotImplementedError):
        net(x, quality=QS, training=True)                             # 2 levels x 2 images
    monkeypatch.undo()
    net.all_scalable = False
    try:
        with pytest.raises(NotImplementedError):
            net(x, quality=QS, training=True)
    finally:
        net.all_scalable = True
    assert not any(k[0] == "full_train" for k in net._plans)


def test_levels_training_loop():
    """Three first_train_step calls with [0, 2.5, 5, 10] and Adam lower the loss (finite throughout)."""
    from vampic.finetune import ScalableRateDistortionLoss, first_train_step
    from vampic.checkpoint import configure_optimizers
    net, sd = _model()
    args = argparse.Namespace(learning_rate=1e-4, aux_learning_rate=1e-3, training_type="first_train")
    opt, _ = configure_optimizers(net, args)
    crit = ScalableRateDistortionLoss(lmbda_list=[0.0055, 0.01, 0.02, 0.04], device="cuda")
    x = synth.synth_image(2, 64, 64, seed=8).cuda()
    noise = {"y": synth.uniform((2, 320 * 4, 4, 4), 301) - 0.5, "z": synth.uniform((2, 192, 1, 1), 302) - 0.5}
    losses = []
    for _ in range(3):
        c = first_train_step(net, crit, x, opt, [0, 2.5, 5, 10], clip_max_norm=1.0, noise=noise)
        losses.append(float(c["loss"]))
        assert np.isfinite(losses[-1])
    print("levels losses", losses)
    assert losses[-1] < losses[0]


def test_levels_graph_replay_is_bit_identical():
    from vampic.finetune import ScalableRateDistortionLoss
    net, sd = _model()
    net.use_graph = True
    x, ny, nz = _inputs()
    crit = ScalableRateDistortionLoss(lmbda_list=LMBDA, device="cuda")
    res = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        out = net(x.cuda(), quality=QS, training=True, noise={"y": ny, "z": nz})
        c = crit(out, x.cuda())
        c["loss"].backward()
        res.append((float(c["loss"]), [p.grad.detach().clone() for p in net.parameters()]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
