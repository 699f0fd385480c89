"""Rate sweep on the GPU (VarianceMaskingPIC.forward_qualities, evaluate.rd_sweep): the two level kernels
against the launches they replace, the sweep against one forward_single_quality per quality (bit for bit; the float64 rate
sums to 1e-12), level groups and image sub-batches, graph replay, the evaluation drivers and the configurations that keep
the per-quality loop."""
import argparse
import copy
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                              # noqa: E402
import vampic.synth as synth               # noqa: E402
from vampic import evaluate as EV, ops     # noqa: E402

M = sys.modules["vampic.models"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
QS7 = [0, 0.05, 0.5, 1, 2.5, 5, 10]
QS15 = [0, 0.05, 0.1, 0.25, 0.5, 0.6, 0.75, 1, 1.25, 2, 2.5, 3, 3.5, 5, 10]
_NETS = {}


def _net(kind="pic", **over):
    key = (kind,) + tuple(sorted(over.items()))
    if key not in _NETS:
        a = dict(README_ARGS, **over)
        if kind == "rem":
            a.update(check_levels=[0.01, 0.25, 1.75], mu_std=True, dimension="big")
        net = vampic.get_model(argparse.Namespace(model=kind, **a), "cpu").eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
        _NETS[key] = net.cuda()
    return _NETS[key]


def _x(B, H, W, seed=3):
    return synth.synth_image(B, H, W, seed=seed).cuda()


def _v(t):
    return ops.from_nchw(t.cuda())


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _same(got, want, what=""):
    """got / want: forward_single_quality result dicts.  Every tensor bit-identical, log2_likelihood_sum to 1e-12."""
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        g, w = got[k], want[k]
        if k == "likelihoods":
            assert list(g) == list(w)
            for kk in w:
                assert torch.equal(g[kk], w[kk]), (what, k, kk)
        elif k == "log2_likelihood_sum":
            assert g.shape == w.shape and _rel(g, w) < 1e-12, (what, k, _rel(g, w))
        elif torch.is_tensor(w):
            assert g.shape == w.shape and torch.equal(g, w), (what, k)
        else:
            assert g == w, (what, k)


def _loop(net, x, qs, mask_pol=None):
    mp = net.mask_policy if mask_pol is None else mask_pol
    return [net.forward_single_quality(x, q, mp, training=False) for q in qs]


# ----------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n_levels", [1, 3, 8])
@pytest.mark.parametrize("with_y2", [True, False])
def test_gauss_levels_eval_equals_gauss_tail_per_level(n_levels, with_y2):
    B, h, w, d = 2, 8, 12, 64
    y = synth.normal((B, 2 * d, h, w), 40) * 4
    musg = synth.normal((B, 3 * d, h, w), 41) * 2                       # mu and sigma: windows of one wider tensor
    musg[:, 2 * d:] = musg[:, 2 * d:].abs() * 0.5
    musg[0, 2 * d:2 * d + 5] = 0.05                                      # below the 0.11 bound
    y_v, ms_v = _v(y), _v(musg)
    y_top, y_sub = y_v.window(d, d), (y_v.window(0, d) if with_y2 else None)
    mu, sg = ms_v.window(0, d), ms_v.window(2 * d, d)                   # pixel stride 3d != C
    prs = [0.0, 10.0, 2.5, 5.0, 0.5, 7.3, 1.0, 9.99][:n_levels]
    masks = ops.new_view(n_levels * B, h, w, d)
    ops.variance_mask_levels(sg, prs, masks, n_slice=d // 32)
    if n_levels >= 2:                                                   # all-zero and all-one masks
        masks.buf[:B].zero_()
        masks.buf[B:2 * B].fill_(1.0)
    yhat = ops.View(torch.empty((n_levels * B, h, w, d + 32), device="cuda"), 32, d)   # output windows with their own stride
    lik = ops.new_view(n_levels * B, h, w, d)
    sym = ops.new_iview(n_levels * B, h, w, d)
    ls = torch.zeros((n_levels, B), dtype=torch.float64, device="cuda")
    ops.gauss_levels_eval(y_top, mu, sg, masks, n_levels, y2=y_sub, yhat=yhat, lik=lik, sym=sym, log2sum=ls)
    for k in range(n_levels):
        lv = lambda v: ops.View(v.buf[k * B:(k + 1) * B], v.c0, v.C)
        yh1, lk1, sy1 = ops.new_view(B, h, w, d), ops.new_view(B, h, w, d), ops.new_iview(B, h, w, d)
        ls1 = torch.zeros(B, dtype=torch.float64, device="cuda")
        ops.gauss_tail(y_top, mu, sg, y2=y_sub, mask=lv(masks), yhat=yh1, lik=lk1, sym=sy1, log2sum=ls1)
        torch.cuda.synchronize()
        assert torch.equal(lv(yhat).torch_nchw(), yh1.torch_nchw()), k
        assert torch.equal(lv(lik).torch_nchw(), lk1.torch_nchw()), k
        assert torch.equal(sym.buf[k * B:(k + 1) * B], sy1.buf), k
        assert _rel(ls[k], ls1) < 1e-12, (k, ls[k], ls1)


@pytest.mark.parametrize("n_levels", [1, 3, 17])
def test_sqdiff_sum_levels_equals_float64_and_per_level_sums(n_levels):
    B, H, W = 3, 64, 96
    x = synth.uniform((B, 3, H, W), 5).cuda()
    xh = synth.uniform((n_levels * B, 3, H, W), 6).cuda()
    acc = torch.zeros((n_levels, B), dtype=torch.float64, device="cuda")
    ops.sqdiff_sum_levels(x, xh, acc)
    diff = (x.unsqueeze(0) - xh.view(n_levels, B, 3, H, W)).double()
    ref = (diff * diff).sum(dim=(2, 3, 4))
    assert _rel(acc, ref) < 1e-12
    for k in range(n_levels):
        for b in range(B):
            one = torch.zeros(1, dtype=torch.float64, device="cuda")
            ops.sqdiff_sum(x[b].contiguous(), xh[k * B + b].contiguous(), one)
            assert abs(float(acc[k, b]) - float(one)) <= 1e-12 * float(one), (k, b)


# ----------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("use_graph", [False, True])
def test_forward_qualities_is_bit_identical_to_forward_single_quality(use_graph):
    net = _net()
    net.use_graph = use_graph
    try:
        x = _x(2, 128, 192)
        with torch.no_grad():
            got = net.forward_qualities(x, QS7)
            want = _loop(net, x, QS7)
        for q, g, w in zip(QS7, got, want):
            _same(g, w, q)
        assert "mask" in got[1] and "mask" not in got[0]
    finally:
        net.use_graph = True


def test_forward_qualities_full_batch_fifteen_levels():
    net = _net()
    x = _x(32, 256, 256, seed=7)
    with torch.no_grad():
        got = net.forward_qualities(x, QS15)
        for q, g in zip(QS15, got):
            _same(g, net.forward_single_quality(x, q, training=False), q)
    del got
    torch.cuda.empty_cache()


def test_level_groups_and_image_sub_batches(monkeypatch):
    net = _net()
    x = _x(3, 64, 64, seed=9)
    qs = [2.5, 0, 10, 0.5, 5, 1]
    with torch.no_grad():
        want = _loop(net, x, qs)
        monkeypatch.setattr(M, "MAX_PLAN_PIXELS", 2 * 64 * 64)          # sub-batches of 2 + 1 images, 1 and 2 levels a group
        assert M.sweep_groups(5, 3, 64, 64) == [(0, 2, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]), (2, 3, [(0, 2), (2, 4), (4, 5)])]
        got = net.forward_qualities(x, qs)
        again = net.forward_qualities(x, qs)                             # graph replay
    for q, g, a, w in zip(qs, got, again, want):
        _same(g, w, q)
        _same(a, w, q)


def test_twelve_levels_two_mask_launches_and_changed_lists():
    net = _net()
    x = _x(1, 64, 128, seed=11)
    qs12 = [0.05, 0.1, 0.25, 0.5, 0.6, 0.75, 1, 1.25, 2, 3, 5, 10]
    assert [len(g) for _, _, g in M.sweep_groups(12, 1, 64, 128)] == [2]
    with torch.no_grad():
        want = _loop(net, x, qs12)
        for _ in range(2):                                               # capture, then replay
            for q, g, w in zip(qs12, net.forward_qualities(x, qs12), want):
                _same(g, w, q)
        other = [10, 0, 0.3, 2.5]                                        # a changed list: new graphs, same bits
        for q, g, w in zip(other, net.forward_qualities(x, other), _loop(net, x, other)):
            _same(g, w, q)
        for q, g, w in zip(qs12, net.forward_qualities(x, qs12), want):
            _same(g, w, q)


def test_two_levels_mask_policy():
    net = _net()
    x = _x(2, 64, 64, seed=13)
    qs = [0, 0.5, 5]
    with torch.no_grad():
        for q, g, w in zip(qs, net.forward_qualities(x, qs, mask_pol="two-levels"), _loop(net, x, qs, "two-levels")):
            _same(g, w, q)


# ----------------------------------------------------------------------------------------------- drivers
def test_forward_eval_list_equals_stacked_results():
    net = _net()
    x = _x(2, 64, 128, seed=15)
    with torch.no_grad():
        got = net.forward(x, [0, 2.5, 10], training=False)
        outs = _loop(net, x, [0, 2.5, 10])
    assert torch.equal(got["x_hat"], torch.stack([o["x_hat"] for o in outs]))
    assert torch.equal(got["likelihoods"]["y"], outs[0]["likelihoods"]["y"])
    assert torch.equal(got["likelihoods"]["y_prog"], torch.stack([o["likelihoods"]["y"] for o in outs[1:]]))
    assert torch.equal(got["likelihoods"]["z"], outs[0]["likelihoods"]["z"])
    assert all(torch.equal(a, o["y_hat"]) for a, o in zip(got["y_hat"], outs))
    assert torch.equal(got["y_base"], outs[0]["y_hat"]) and torch.equal(got["y_prog"], outs[-1]["y_hat"])


def test_test_epoch_and_valid_epoch_equal_per_quality_loop():
    net = _net()
    batches = [_x(2, 64, 128, seed=s) for s in (21, 22)]
    qs = [0, 0.05, 1, 10]

    def crit(out, d):
        return {"loss": ((out["x_hat"] - d) ** 2).mean() - out["log2_likelihood_sum"].sum() * 1e-4,
                "bpp_loss": -out["log2_likelihood_sum"].sum() / (d.shape[0] * d.shape[2] * d.shape[3])}
    with torch.no_grad():
        bpp_l, psnr_l = [[] for _ in qs], [[] for _ in qs]
        tot = {"loss": 0.0, "bpp": 0.0, "mse": 0.0, "psnr": 0.0}
        for d in batches:
            n_pix = d.shape[0] * d.shape[2] * d.shape[3]
            for j, q in enumerate(qs):
                out = net.forward_single_quality(d, q, training=False)
                bpp_l[j].append(EV.estimated_bpp(out, n_pix))
                psnr_l[j].append(EV.compute_psnr(d, out["x_hat"]))
                c = crit(out, d)
                tot["loss"] += float(c["loss"])
                tot["bpp"] += float(c["bpp_loss"])
                tot["mse"] += 10.0 ** (-psnr_l[j][-1] / 10.0)
                tot["psnr"] += psnr_l[j][-1]
    n = len(batches) * len(qs)
    bpp, psnr = EV.test_epoch(batches, net, qs)
    for j in range(len(qs)):
        assert abs(bpp[j] - sum(bpp_l[j]) / 2) <= 1e-12 * abs(bpp[j]), qs[j]
        assert abs(psnr[j] - sum(psnr_l[j]) / 2) <= 1e-9, qs[j]
    loss, avg = EV.valid_epoch(0, batches, crit, net, qs)
    assert abs(loss - tot["loss"] / n) <= 1e-9 * abs(loss)
    assert abs(avg["bpp"] - tot["bpp"] / n) <= 1e-12 * abs(avg["bpp"])
    assert abs(avg["psnr"] - tot["psnr"] / n) <= 1e-9


def test_rd_sweep_per_image_values():
    net = _net()
    x = _x(3, 64, 64, seed=25)
    qs = [0, 0.25, 2.5, 10, 0]
    bpp, psnr = EV.rd_sweep(net, x, qs)
    assert bpp.shape == psnr.shape == (len(qs), 3) and bpp.dtype == psnr.dtype == torch.float64
    with torch.no_grad():
        for j, q in enumerate(qs):
            out = net.forward_single_quality(x, q, training=False)
            for b in range(3):
                one = {"log2_likelihood_sum": out["log2_likelihood_sum"][:, b:b + 1]}
                assert abs(float(bpp[j, b]) - EV.estimated_bpp(one, 64 * 64)) <= 1e-12 * float(bpp[j, b]), (q, b)
                assert abs(float(psnr[j, b]) - EV.compute_psnr(x[b:b + 1], out["x_hat"][b:b + 1])) <= 1e-9, (q, b)


# ----------------------------------------------------------------------------------------------- fallbacks
@pytest.mark.parametrize("variant", ["rem", "not_all_scalable", "bf16"])
def test_fallbacks_return_the_loop(variant):
    if variant == "bf16":
        # a copy of its own (no plans), run eagerly: dropping the shared model's plans would retire their graphs
        net = copy.deepcopy(_net())
        net.storage, net.use_graph = "bf16", False
    else:
        net = _net("rem") if variant == "rem" else _net(all_scalable=False)
    x = _x(2, 64, 64, seed=27)
    qs = [0, 0.5, 10]
    assert not net._sweep_eligible()
    with torch.no_grad():
        for q, g, w in zip(qs, net.forward_qualities(x, qs), _loop(net, x, qs)):
            _same(g, w, q)
        bpp, psnr = EV.rd_sweep(net, x, qs)
        assert torch.isfinite(bpp).all() and torch.isfinite(psnr).all()


_CHILD = r"""
import argparse, sys, torch
sys.path.insert(0, {root!r})
import vampic, vampic.synth as synth
from vampic import ops
a = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
         division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
         total_mu_rep=True, all_scalable=True)
net = vampic.get_model(argparse.Namespace(model="pic", **a), "cpu").eval()
net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
net = net.cuda()
x = synth.synth_image(2, 64, 128, seed=31).cuda()
qs = [0, 0.5, 2.5, 10]
assert net._sweep_eligible() == {eligible}, net._sweep_eligible()
with torch.no_grad():
    got = net.forward_qualities(x, qs)
    want = [net.forward_single_quality(x, q, training=False) for q in qs]
for q, g, w in zip(qs, got, want):
    for k in ("x_hat", "y_hat", "y_base", "mu", "std"):
        assert torch.equal(g[k], w[k]), (q, k)
    assert torch.equal(g["likelihoods"]["y"], w["likelihoods"]["y"]) and torch.equal(g["likelihoods"]["z"], w["likelihoods"]["z"])
    assert q == 0 or torch.equal(g["mask"], w["mask"])
    r = float(((g["log2_likelihood_sum"] - w["log2_likelihood_sum"]).abs().max() / w["log2_likelihood_sum"].abs().max()))
    assert r < 1e-12, r
print("CHILD-OK")
"""


@pytest.mark.parametrize("mode,eligible", [("f16x2", False), ("f32", True)])
def test_conv_modes_in_a_child_process(mode, eligible):
    """VAMPIC_CONV fixes the packed-weight layout for the life of a process: f16x2 keeps the per-quality loop, the fp32-pipe
    mode takes the sweep, both equal the loop."""
    env = dict(os.environ, VAMPIC_CONV=mode)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, eligible=eligible)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
