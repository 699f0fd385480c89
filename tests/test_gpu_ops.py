"""Operator-level parity of the HIP kernels (through the C ABI) against the CPU oracle /
plain fp32 ATen CPU ops on the same seeded inputs.  Integer/rank work is bit-exact;
float work is compared with the tolerance written next to each check."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vampic                                     # noqa: E402
from vampic import layers as Ly, ops, _lib as L  # noqa: E402
import vampic_oracle as O                         # noqa: E402


def _rand(shape, seed, scale=1.0):
    return vampic.synth.normal(shape, seed, scale)


def _close(a, b, rtol=2e-5, atol=2e-5, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max abs err {err:.3e} vs ref magnitude {ref:.3e}"


def _fill(m, seed):
    sd = vampic.synth.synth_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    return {k: v.clone() for k, v in sd.items()}


@pytest.mark.parametrize("cin,cout,k,s,hw", [(32, 32, 3, 1, (16, 16)), (352, 224, 3, 1, (16, 24)), (176, 128, 3, 1, (9, 7)),
                                              (192, 192, 5, 2, (32, 32)), (3, 192, 5, 2, (64, 96)), (96, 192, 1, 1, (16, 16)),
                                              (288, 256, 3, 2, (16, 16)), (192, 320, 5, 2, (32, 32))])
def test_conv2d(cin, cout, k, s, hw):
    m = Ly.Conv2d(cin, cout, k, s)
    sd = _fill(m, 1)
    x = _rand((2, cin) + hw, 2)
    ref = F.conv2d(x, sd["weight"], sd["bias"], stride=s, padding=k // 2)
    with torch.no_grad():
        out = m.cuda()(x.cuda())
    assert out.shape == ref.shape
    _close(out, ref, what=f"conv {cin}->{cout} k{k} s{s}")


@pytest.mark.parametrize("cin,cout,hw", [(320, 192, (4, 4)), (192, 192, (8, 12)), (192, 3, (16, 16))])
def test_deconv(cin, cout, hw):
    m = Ly.ConvTranspose2d(cin, cout)
    sd = _fill(m, 3)
    x = _rand((2, cin) + hw, 4)
    ref = F.conv_transpose2d(x, sd["weight"], sd["bias"], stride=2, padding=2, output_padding=1)
    with torch.no_grad():
        out = m.cuda()(x.cuda())
    _close(out, ref, what=f"deconv {cin}->{cout}")


def test_subpel_and_stack():
    from vampic.models import _hyper_synthesis
    m = _hyper_synthesis(192, 192, 320)
    sd = _fill(m, 5)
    x = _rand((2, 192, 2, 3), 6)
    ref = O.h_s({("p." + k): v for k, v in sd.items()}, "p.", x)
    with torch.no_grad():
        out = m.cuda()(x.cuda())
    _close(out, ref, what="hyper synthesis stack")


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn(inverse):
    m = Ly.GDN(192, inverse=inverse)
    sd = _fill(m, 7)
    x = _rand((2, 192, 8, 8), 8, 2.0)
    ref = O.gdn({("g." + k): v for k, v in sd.items()}, "g.", x, inverse)
    with torch.no_grad():
        out = m.cuda()(x.cuda())
    _close(out, ref, what="gdn")


@pytest.mark.parametrize("dim,ws,hw", [(192, 8, (16, 24)), (320, 4, (8, 8))])
def test_attention_block(dim, ws, hw):
    m = Ly.Win_noShift_Attention(dim=dim, num_heads=8, window_size=ws, shift_size=ws // 2)
    sd = _fill(m, 9)
    x = _rand((2, dim) + hw, 10)
    ref = O.attention_block({("a." + k): v for k, v in sd.items()}, "a.", x, ws)
    with torch.no_grad():
        out = m.cuda()(x.cuda())
    _close(out, ref, rtol=5e-5, atol=5e-5, what="attention block")


def test_rem_block():
    m = Ly.LatentRateReduction(32, True, "middle")
    sd = _fill(m, 11)
    yck, epb, epp = _rand((2, 32, 8, 8), 12, 3.0), _rand((2, 64, 8, 8), 13), _rand((2, 64, 8, 8), 14)
    att = (vampic.synth.uniform((2, 32, 8, 8), 15) > 0.5).float()
    att2 = torch.cat([att, att], 1)
    ref = O.rem_block({("r." + k): v for k, v in sd.items()}, "r.", yck, epb, epp, att2)
    with torch.no_grad():
        out = m.cuda()(yck.cuda(), epb.cuda(), epp.cuda(), att2.cuda())
    _close(out, ref, what="REM block")


# ---------------------------------------------------------------- variance mask: bit-exact
Q_LEVS = [0, 0.01, 0.05, 0.1, 0.25, 0.5, 0.6, 0.75, 1, 1.5, 2, 2.5, 3, 5, 7.7, 9.99, 10, 12]


@pytest.mark.parametrize("shape", [(3, 32, 16, 16), (2, 32, 32, 48), (2, 32, 5, 3), (1, 4, 1, 1)])
def test_variance_mask_bit_exact(shape):
    B, C, h, w = shape
    s = vampic.synth.synth_sigma(B, C * h * w, seed=3).reshape(B, C, h, w)
    cm = Ly.ChannelMask("point-based-std")
    for q in Q_LEVS:
        ref = O.variance_mask_np(s.numpy(), q)
        out = cm(s.cuda(), pr=q).cpu().numpy()
        assert out.shape == ref.shape
        assert np.array_equal(out, ref), f"mask XOR = {(out != ref).sum()} at q={q} shape={shape}"


def test_variance_mask_edge_cases():
    cm = Ly.ChannelMask("point-based-std")
    # all-equal segment: ties are all kept
    s = torch.full((1, 32, 4, 4), 1.25)
    assert cm(s.cuda(), pr=5).sum().item() == s.numel()
    # NaN in a segment -> threshold NaN -> all zero, other segments unaffected
    s = vampic.synth.synth_sigma(2, 32 * 16, seed=5).reshape(2, 32, 4, 4)
    s[0, 3, 1, 1] = float("nan")
    out = cm(s.cuda(), pr=3).cpu().numpy()
    ref = O.variance_mask_np(s.numpy(), 3)
    assert out[0].sum() == 0 and np.array_equal(out, ref)
    # +-0 and denormals and infinities
    s = torch.tensor([0.0, -0.0, 1e-42, -1e-42, float("inf"), -float("inf"), 3.0, 2.0] * 4).reshape(1, 4, 2, 4)
    for q in (1, 2.5, 5, 9):
        assert np.array_equal(cm(s.cuda(), pr=q).cpu().numpy(), O.variance_mask_np(s.numpy(), q))
    # nestedness in q
    s = vampic.synth.synth_sigma(1, 8192, seed=9).reshape(1, 32, 16, 16).cuda()
    prev = None
    for q in (0.5, 1, 2.5, 5, 7.5):
        mk = cm(s, pr=q)
        if prev is not None:
            assert bool((mk >= prev).all())
        prev = mk
    # two-levels policy and unknown policy
    assert cm(s, pr=0, mask_pol="two-levels").sum().item() == 0
    assert cm(s, pr=2, mask_pol="two-levels").mean().item() == 1
    with pytest.raises(NotImplementedError):
        cm(s, pr=2, mask_pol="nope")


def test_prog_mask_matches_oracle():
    cm = Ly.ChannelMask("point-based-std")
    blocks = [vampic.synth.synth_sigma(1, 32 * 64, seed=20 + i).reshape(1, 32, 8, 8) for i in range(10)]
    for q in (0, 0.5, 2.5, 10):
        ref = O.prog_mask_np([b.numpy() for b in blocks], q)
        out = cm.ProgMask([b.cuda() for b in blocks], q).cpu().numpy()
        assert np.array_equal(out, ref)


# ---------------------------------------------------------------- Gaussian conditional
def test_gauss_likelihood_and_indexes():
    gc = vampic.GaussianConditional(None).cuda()
    y, mu = _rand((2, 32, 16, 16), 30, 6.0), _rand((2, 32, 16, 16), 31, 4.0)
    sg = vampic.synth.synth_sigma(2, 32 * 256, seed=32).reshape(2, 32, 16, 16)
    out, lik = gc(y.cuda(), sg.cuda(), mu.cuda(), training=False)
    ref_out = torch.round(y - mu) + mu
    assert torch.equal(out.cpu(), ref_out), "quantised latent must be bit-exact"
    ref = O.gaussian_likelihood(y, sg, mu)
    # lik = Phi(a) - Phi(b): two erfc values of magnitude <= 1 whose implementations differ by a
    # few ulp (6e-8 each), so the tolerance is absolute
    err = (lik.cpu() - ref).abs().max().item()
    # (the bound in bits, the tails and the rounding edges: tests/test_gpu_entropy_contract.py)
    assert err < 3e-7, f"likelihood abs err {err}"
    out2, lik2 = gc(y.cuda(), sg.cuda(), None, training=False)
    assert torch.equal(out2.cpu(), torch.round(y))
    assert (lik2.cpu() - O.gaussian_likelihood(y, sg, None)).abs().max() < 3e-7
    gc.update_scale_table([float(v) for v in O.scale_table()])
    idx = gc.build_indexes(sg.cuda())
    assert torch.equal(idx.cpu(), O.build_indexes(sg)), "build_indexes must be bit-exact"
    sym = gc.quantize(y.cuda(), "symbols", mu.cuda())
    assert torch.equal(sym.cpu(), torch.round(y - mu).int())


def test_entropy_bottleneck():
    eb = vampic.EntropyBottleneck(192)
    sd = _fill(eb, 40)
    z = _rand((2, 192, 4, 6), 41, 5.0)
    zh_ref, lik_ref = O.eb_forward({("e." + k): v for k, v in sd.items()}, z, "e.")
    zh, lik = eb.cuda()(z.cuda(), training=False)
    assert torch.equal(zh.cpu(), zh_ref), "z_hat must be bit-exact"
    # The likelihood is a difference of two sigmoids of the 5-layer logit chain (entropy_models.py:373-383): its error
    # is absolute (the fp32 oracle itself sits 1.0e-7 abs / 8e-6 rel from a float64 evaluation of the same formula on
    # this input, smallest likelihood 7e-3).  Same 3e-7 abs bar as the Gaussian likelihood; the relative figure is
    # printed and bounded where it means something (it was round 1's only, loose, assertion).
    err = (lik.cpu() - lik_ref).abs()
    rel = (err / lik_ref).max().item()
    print(f"EB likelihood: abs err {err.max().item():.3g}, rel err {rel:.3g}, min lik {lik_ref.min().item():.3g}")
    # (the bound in bits against float64, ties and the 1e-9 decision: tests/test_gpu_entropy_contract.py)
    assert err.max().item() <= 3e-7, f"EB likelihood abs err {err.max().item()}"
    assert rel <= 2e-5, rel                            # measured 6.6e-6 (the fp32 oracle's own: 8e-6)


def test_errors_are_loud():
    m = Ly.Conv2d(8, 8, 3)
    x = torch.randn(1, 8, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        m.cuda()(x)                                  # no silent autograd fallback
    with pytest.raises(Exception):
        ops.conv_problem(m.cuda().packed(), [ops.from_nchw(torch.randn(1, 4, 4, 4, device="cuda"))],
                         ops.new_view(1, 4, 4, 8))   # channel mismatch


def test_conv_result_is_independent_of_tiling():
    """Encoder and decoder run the same layers under different groupings / tile shapes; the K
    order is canonical, so every (BM, BN, BK) must give bit-identical outputs."""
    lib = L.load()
    for cin, n, k, st, hw in ((192, 192, 3, 1, (16, 16)), (176, 128, 3, 1, (16, 16)), (512, 224, 3, 1, (16, 16)),
                              (192, 192, 5, 2, (32, 32)), (96, 192, 1, 1, (16, 16))):
        m = Ly.Conv2d(cin, n, k, st).cuda()
        _fill(m, 21)
        x = _rand((4, cin) + hw, 22).cuda()
        outs = []
        for bm, bn, bk in ((0, 0, 0), (64, 64, 16), (64, 64, 32), (128, 64, 16), (128, 192, 16), (64, 128, 32), (128, 32, 16), (128, 224, 32)):
            if bk == 32 and cin % 32:
                continue
            lib.vam_conv_force_tile(bm, bn, bk)
            try:
                with torch.no_grad():
                    outs.append(m(x).clone())
            finally:
                lib.vam_conv_force_tile(0, 0, 0)
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), (cin, n, k, st)


@pytest.mark.parametrize("hw,batch", [((16, 16), 2), ((24, 40), 2), ((13, 21), 1), ((64, 64), 2), ((8, 16), 3), ((64, 64), 40)])
def test_fused_residual_unit_is_bit_identical(hw, batch, monkeypatch):
    """csrc/resunit.hip runs a ResidualUnit (layers/layers.py:30-48) as ONE launch with both C/2-channel intermediates
    in LDS.  Same split-operand arithmetic in the same canonical K order as three conv launches: the results must agree
    bit for bit (image sizes that are not multiples of the 8 x 16 tile included), with the weight slabs staged by LDS-DMA
    and by registers alike; and they agree with ATen's fp32 unit."""
    lib = L.load()
    m = Ly.ResidualUnit(192)
    sd = _fill(m, 31)
    x = _rand((batch, 192) + hw, 32)
    m = m.cuda()
    xc = x.cuda()
    assert ops.resunit_supported(ops.from_nchw(xc)), "C = 192 has a fused kernel"
    outs = {}
    with torch.no_grad():
        for mode in (1, 0):           # weight slabs by LDS-DMA (default) / register-staged
            lib.vam_resunit_set_dma(mode)
            try:
                outs[f"fused mode={mode}"] = m(xc).clone()
            finally:
                lib.vam_resunit_set_dma(-1)
        monkeypatch.setenv("VAMPIC_FUSED_RU", "0")
        assert not ops.resunit_supported(ops.from_nchw(xc))
        outs["three launches"] = m(xc).clone()
        monkeypatch.delenv("VAMPIC_FUSED_RU")
    ref3 = outs["three launches"]
    for k, o in outs.items():
        assert torch.isfinite(o).all(), k
        assert torch.equal(o, ref3), f"{k}: {(o != ref3).sum().item()} of {o.numel()} elements differ, max {(o - ref3).abs().max().item():.3e}"
    t = F.gelu(F.conv2d(x, sd["conv.0.weight"], sd["conv.0.bias"]))
    t = F.gelu(F.conv2d(t, sd["conv.2.weight"], sd["conv.2.bias"], padding=1))
    ref = F.gelu(F.conv2d(t, sd["conv.4.weight"], sd["conv.4.bias"]) + x)
    _close(ref3, ref, what="residual unit vs ATen fp32")


def test_gelu_accuracy_against_float64():
    """Every GELU of the library is csrc/common.h vam_gelu: 0.5 v (1 + erf(v / sqrt 2)) with a branch-free erf
    (1 - 2^(-|x| P(|x|)), 18 instructions instead of ocml erff's ~45).  Against float64 on a dense grid: relative error
    <= 5e-7 for v > -1 (measured 3.5e-7; a correctly rounded fp32 erf in the same formula gives 2.1e-7), absolute error
    <= 6e-7 everywhere (measured 4.5e-7 = half an ulp at |v| ~ 8), and within 2e-6 of ATen's own fp32 gelu (whose
    vectorised erf is itself 1.4e-6 = 1.5 ulp from this kernel — and from float64 — at |v| ~ 8)."""
    from scipy.special import erf as erf64
    n = 1 << 20
    v = torch.linspace(-8.0, 8.0, n, dtype=torch.float32)
    v = torch.cat([v, torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 1e4, -1e4])])
    v = torch.cat([v, torch.zeros((-v.numel()) % 64)]).reshape(1, -1, 1, 64).permute(0, 3, 1, 2).contiguous()    # [1, 64, n/64, 1]
    x = ops.from_nchw(v.cuda())
    o = ops.new_view(x.B, x.H, x.W, x.C, "cuda")
    ops.ew(L.EW_GELU_FWD, [x], [o])
    got = o.torch_nchw().cpu().double().reshape(-1)
    vv = v.double().reshape(-1)
    truth = 0.5 * vv * (1.0 + torch.from_numpy(erf64(vv.numpy() / math.sqrt(2.0))))
    err = (got - truth).abs()
    assert torch.isfinite(got).all()
    assert err.max().item() <= 6e-7 * max(1.0, 1.0), err.max().item()            # |v| <= 8 on the grid; the far points below
    sel = (vv > -1) & (vv.abs() <= 8) & (vv.abs() > 1e-20)
    rel = (err[sel] / truth[sel].abs()).max().item()
    assert rel <= 5e-7, rel
    aten = F.gelu(v.reshape(-1)).double()
    grid = vv.abs() <= 8
    assert (got - aten).abs()[grid].max().item() <= 2e-6
    far = {20.0: 20.0, -20.0: 0.0, 1e4: 1e4, -1e4: 0.0}
    for k, want in far.items():
        assert abs(got[vv == k][0].item() - want) <= 1e-6 * max(1.0, abs(want)), (k, got[vv == k][0].item())
    print(f"GELU vs float64: max abs {err[grid].max().item():.2e}, max rel (v > -1) {rel:.2e}; vs ATen fp32: {(got - aten).abs()[grid].max().item():.2e}")


def test_direct_and_staged_epilogues_are_bit_identical():
    """On the 128x64 tile fp32 NHWC outputs leave the convolution kernel straight from the accumulator registers (direct
    epilogue); every other tile, bf16 / plane / NCHW outputs and tensors beyond its 32-bit window go through LDS
    (staged epilogue).  Same operations per
    element in the same order: every module must produce the same bits either way — dense outputs, the strided views
    of the four deconvolution phases, the pixel-shuffle scatter, bias / pre / mul / post operands (GDN, residual
    units, attention, REM), ragged channel counts and a ragged last row tile, every tile shape."""
    from vampic.models import _hyper_synthesis
    lib = L.load()
    cases = []
    m = Ly.Conv2d(176, 144, 3, 1); _fill(m, 51); cases.append(("conv ragged N", m, (_rand((3, 176, 9, 7), 52),)))
    m = Ly.Conv2d(192, 192, 5, 2); _fill(m, 53); cases.append(("conv 5x5 s2", m, (_rand((2, 192, 32, 32), 54),)))
    m = Ly.ConvTranspose2d(192, 192); _fill(m, 55); cases.append(("deconv phases", m, (_rand((2, 192, 8, 12), 56),)))
    m = _hyper_synthesis(192, 192, 320); _fill(m, 57); cases.append(("subpel stack", m, (_rand((2, 192, 2, 3), 58),)))
    m = Ly.GDN(192); _fill(m, 59); cases.append(("gdn", m, (_rand((2, 192, 16, 16), 60, 2.0),)))
    m = Ly.GDN(192, inverse=True); _fill(m, 61); cases.append(("igdn", m, (_rand((2, 192, 16, 16), 62, 2.0),)))
    m = Ly.Win_noShift_Attention(dim=192, num_heads=8, window_size=8, shift_size=4); _fill(m, 63)
    cases.append(("attention block", m, (_rand((2, 192, 16, 24), 64),)))
    m = Ly.LatentRateReduction(32, True, "middle"); _fill(m, 65)
    att = (vampic.synth.uniform((2, 32, 8, 8), 66) > 0.5).float()
    cases.append(("rem block", m, (_rand((2, 32, 8, 8), 67, 3.0), _rand((2, 64, 8, 8), 68), _rand((2, 64, 8, 8), 69), torch.cat([att, att], 1))))
    for what, m, xs in cases:
        m = m.cuda()
        xs = [x.cuda() for x in xs]
        outs = []
        for staged, tile in ((1, (0, 0)), (0, (0, 0)), (1, (128, 64)), (0, (128, 64)), (0, (64, 64)), (0, (128, 192))):
            lib.vam_conv_force_epilogue(staged)
            lib.vam_conv_force_tile(tile[0], tile[1], 0)
            try:
                with torch.no_grad():
                    outs.append(m(*xs).clone())
            finally:
                lib.vam_conv_force_epilogue(-1)
                lib.vam_conv_force_tile(0, 0, 0)
        assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0, what
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), what


def test_conv_accuracy_against_float64():
    """The convolution kernel against a float64 convolution of the same fp32 inputs.  The default kernel splits every
    fp32 operand exactly into three bf16 terms and sums six exact partial products in fp32, so
    what remains is the rounding of a length-K fp32 accumulation: rms error <= (0.5 sqrt(K) + 2) * 2^-24 * rms(out),
    the random-walk size of a sequential fp32 fma chain (what the fp32-operand kernel produces; ATen's blocked CPU
    summation, printed for context, is a few times tighter than any sequential chain)."""
    for cin, n, k, hw in ((512, 224, 3, (16, 16)), (192, 192, 5, (24, 24)), (96, 192, 1, (16, 16))):
        m = Ly.Conv2d(cin, n, k, 1)
        sd = _fill(m, 31)
        x = _rand((2, cin) + hw, 32, 2.0)
        truth = F.conv2d(x.double(), sd["weight"].double(), sd["bias"].double(), padding=k // 2)
        e32 = (F.conv2d(x, sd["weight"], sd["bias"], padding=k // 2).double() - truth).pow(2).mean().sqrt().item()
        with torch.no_grad():
            got = m.cuda()(x.cuda()).cpu().double()
        e_gpu = (got - truth).pow(2).mean().sqrt().item()
        print(f"conv {cin}->{n} k{k}: rms error vs float64: fp32 ATen {e32:.3e}, kernel {e_gpu:.3e} (output rms {truth.pow(2).mean().sqrt().item():.3e})")
        bound = (0.5 * math.sqrt(cin * k * k) + 2.0) * 2.0 ** -24 * truth.pow(2).mean().sqrt().item()
        assert e_gpu <= bound, (cin, n, k, e_gpu, bound)


def test_fp32_matrix_pipe_mode_in_a_child_process():
    """VAMPIC_CONV=f32 selects the fp32-operand kernel (v_mfma_f32_32x32x2_f32).  The mode fixes the packed-weight
    layout for the life of a process, so the fp32 arithmetic is exercised in a child: the convolution tests must
    pass there as well."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, VAMPIC_CONV="f32")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_ops.py"), "-q", "-x", "-m", "gpu",
                        "-k", "conv2d or deconv or gdn or tiling or float64 or rem_block"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "passed" in r.stdout


def test_bf16x3_plane_tensors_are_transparent():
    """Inside conv stacks the producer writes its output as bf16x3 planes (VAM_CONV_OUT_BF3) and the consumer stages them
    by plain copies (VAM_CONV_IN_BF3).  The split is exact, so (a) decoding the planes returns the fp32 output bit for
    bit and (b) a convolution fed with planes returns exactly what it returns on the fp32 tensor."""
    if not ops.split_mode():
        pytest.skip("bf16x3-plane tensors exist only in the split-operand mode")
    B, H, W = 2, 16, 24
    m1, m2 = Ly.Conv2d(96, 176, 3, 1).cuda(), Ly.Conv2d(176, 64, 3, 1).cuda()
    _fill(m1, 41), _fill(m2, 42)
    x = ops.from_nchw(_rand((B, 96, H, W), 43).cuda())
    mid32, mid3 = ops.new_view(B, H, W, 176), ops.new_view3(B, H, W, 176)
    ops.conv_group([ops.conv_problem(m1.packed(), [x], mid32, L.ACT_GELU)])
    ops.conv_group([ops.conv_problem(m1.packed(), [x], mid3, L.ACT_GELU)])
    assert torch.equal(mid3.to_float(), mid32.buf)                                     # (a)
    o32, o3 = ops.new_view(B, H, W, 64), ops.new_view(B, H, W, 64)
    ops.conv_group([ops.conv_problem(m2.packed(), [mid32], o32)])
    ops.conv_group([ops.conv_problem(m2.packed(), [mid3], o3)])
    assert torch.equal(o3.buf, o32.buf)                                                # (b)
    # channel windows of a plane tensor, and a stride-2 consumer
    m3 = Ly.Conv2d(64, 32, 3, 2).cuda()
    _fill(m3, 44)
    q32, q3 = ops.new_view(B, H // 2, W // 2, 32), ops.new_view(B, H // 2, W // 2, 32)
    ops.conv_group([ops.conv_problem(m3.packed(), [mid32.window(112, 64)], q32)])
    ops.conv_group([ops.conv_problem(m3.packed(), [mid3.window(112, 64)], q3)])
    assert torch.equal(q3.buf, q32.buf)
    with pytest.raises(Exception):                                                      # formats do not mix within a problem
        ops.conv_problem(m2.packed(), [mid3.window(0, 88), mid32.window(88, 88)], o3)


@pytest.mark.parametrize("H,K", [(16, 2), (16, 10), (4, 1), (32, 3)])
def test_fused_stack_tail_is_bit_identical(H, K):
    """csrc/stack_tail.hip: the last two layers of a slice stack (conv3x3 128 -> 64 + GELU, conv3x3 64 -> 32 with the stack's
    final epilogue) in ONE launch, the 64-channel intermediate kept in LDS as bf16x3 planes — against the two conv_igemm
    launches (planes between them) it replaces: the same bits, for plain outputs (mean / scale stacks, written into channel
    windows of wider tensors) and for the LRP tail (0.5 tanh + quantised residual + base slice); groups larger than one
    launch's eight stacks; what it is not built for is refused."""
    if not ops.split_mode():
        pytest.skip("the fused tail reads bf16x3 planes")
    B, W = 3, 16
    outs_a, outs_b = ops.new_view(B, H, W, 32 * K), ops.new_view(B, H, W, 32 * K)
    post, post2 = ops.from_nchw(_rand((B, 32 * K, H, W), 70).cuda()), ops.from_nchw(_rand((B, 32 * K, H, W), 71).cuda())
    two, fused = [[], []], []
    keep = []
    for k in range(K):
        m3, m4, m5 = Ly.Conv2d(32, 128, 3, 1).cuda(), Ly.Conv2d(128, 64, 3, 1).cuda(), Ly.Conv2d(64, 32, 3, 1).cuda()
        _fill(m3, 50 + 3 * k), _fill(m4, 51 + 3 * k), _fill(m5, 52 + 3 * k)
        x = ops.from_nchw(_rand((B, 32, H, W), 60 + k).cuda())
        x3 = ops.new_view3(B, H, W, 128)
        ops.conv_group([ops.conv_problem(m3.packed(), [x], x3, L.ACT_GELU)])            # the stack's third layer writes planes
        mid = ops.new_view3(B, H, W, 64)
        lrp = k % 2 == 1
        kw = dict(act=L.ACT_HALF_TANH, post=post.window(32 * k, 32), post2=post2.window(32 * k, 32) if k % 4 == 1 else None) if lrp else {}
        two[0].append(ops.conv_problem(m4.packed(), [x3], mid, L.ACT_GELU))
        two[1].append(ops.conv_problem(m5.packed(), [mid], outs_a.window(32 * k, 32), kw.get("act", L.ACT_NONE), post=kw.get("post"), post2=kw.get("post2")))
        assert ops.stack_tail_ok(x3, m4, m5, outs_b.window(32 * k, 32), kw)
        fused.append(ops.stack_tail_problem(x3, m4.packed(), m5.packed(), outs_b.window(32 * k, 32), kw.get("act", L.ACT_NONE), kw.get("post"), kw.get("post2")))
        keep += [m3, m4, m5, x, x3, mid]
    ops.conv_group(two[0])
    ops.conv_group(two[1])
    ops.stack_tail_group(fused)
    torch.cuda.synchronize()
    assert torch.isfinite(outs_a.buf).all() and float(outs_a.buf.abs().max()) > 1e-3
    assert torch.equal(outs_a.buf, outs_b.buf)
    # refused: another width, a window of a wider plane tensor, an epilogue operand it does not have
    wide = ops.new_view3(B, H, 32, 128)
    assert not ops.stack_tail_ok(wide, m4, m5, None, {})
    assert not ops.stack_tail_ok(ops.new_view3(B, H, W, 256).window(128, 128), m4, m5, None, {})
    assert not ops.stack_tail_ok(x3, m4, m5, None, {"pre": post.window(0, 32)})
    bad = ops.stack_tail_problem(x3, m4.packed(), m5.packed(), outs_b.window(0, 32))
    bad.W = 32
    with pytest.raises(L.VamError):
        ops.stack_tail_group([bad])


def test_entropy_bottleneck_aux_loss_and_gradient():
    """model.aux_loss() (models/base.py:22-29 -> EntropyBottleneck.loss, entropy_models.py:398-401): value and the
    gradient w.r.t. the quantiles from vam_eb_aux_loss against the REFERENCE's autograd (tests/golden/entropy_ops.npz),
    and one step of the aux optimiser moves the quantiles (utility/functions.py:27-59)."""
    import os
    from vampic.entropy_models import EntropyBottleneck
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "entropy_ops.npz"))
    eb = EntropyBottleneck(192)
    eb.load_state_dict(vampic.synth.synth_state_dict(eb.state_dict(), 40))
    eb = eb.cuda()
    loss = eb.loss()
    loss.backward()
    assert abs(float(loss) - gold["eb_aux_loss"][0]) <= 2e-5 * abs(gold["eb_aux_loss"][0]), (float(loss), gold["eb_aux_loss"][0])
    g = eb.quantiles.grad.cpu().numpy()
    assert np.abs(g - gold["eb_aux_dq"]).max() <= 2e-5 * np.abs(gold["eb_aux_dq"]).max()
    assert all(p.grad is None for n, p in eb.named_parameters() if n != "quantiles")       # stop_gradient on the network
    opt = torch.optim.Adam([eb.quantiles], lr=1e-2)
    before = float(loss)
    for _ in range(20):
        opt.zero_grad()
        l = eb.loss()
        l.backward()
        opt.step()
    assert float(eb.loss()) < before


def test_epilogues_publish_the_output_maximum():
    """``vam_conv.out_amax``: every epilogue path (direct from the accumulators, LDS-staged, wave-specialised blocks, the
    scalar NCHW / PixelShuffle tail) folds max |stored value| into a device cell — the scale source of the fp16x2 mode's
    consumers — and ``vam_absmax`` reduces a channel window of an NHWC tensor the same way."""
    import ctypes
    lib = L.load()
    for cin, n, k, st, B, H, W, act in [(192, 192, 1, 1, 2, 32, 32, L.ACT_GELU),      # 128x64 one-role tile: direct epilogue
                                        (192, 192, 3, 1, 2, 32, 32, L.ACT_NONE),      # wide tile, staged
                                        (224, 176, 3, 1, 4, 16, 16, L.ACT_GELU),      # wave-specialised 64x64
                                        (96, 44, 3, 2, 1, 24, 40, L.ACT_LEAKY)]:      # ragged N, stride 2
        m = Ly.Conv2d(cin, n, k, st).cuda()
        _fill(m, 90 + n)
        x = ops.from_nchw(_rand((B, cin, H, W), 91).cuda())
        wide = ops.new_view(B, H // st, W // st, n + 8, zero=True)                    # the output is a channel window
        out = wide.window(4, n)
        cell = torch.zeros(2, dtype=torch.int32, device="cuda")
        c = ops.conv_problem(m.packed(), [x], out, act)
        c.out_amax = cell.data_ptr()
        ops.conv_group([c])
        torch.cuda.synchronize()
        want = wide.buf[..., 4:4 + n].abs().max()
        assert cell[:1].view(torch.float32).item() == want.item(), (cin, n, k)
        assert cell[1].item() == 0
        seg = (L.VamSeg * 1)()
        seg[0].ptr, seg[0].C, seg[0].ld = out.ptr, n, out.ld
        L.check(lib.vam_absmax(seg, 1, out.n_pix, cell.data_ptr() + 4, ops.stream_ptr()), "vam_absmax")
        torch.cuda.synchronize()
        assert cell[1:].view(torch.float32).item() == want.item()


def test_fp16x2_mode_in_a_child_process():
    """VAMPIC_CONV=f16x2 (opt-in prototype): fp32 operands as two fp16 terms with power-of-two scales, three
    MFMA products.  Like the fp32-pipe mode it fixes the packed-weight layout for the life of a process, so it runs in a
    child: the convolution tests (F.conv2d tolerances, the float64 error bound, tiling invariance, direct vs staged
    epilogue) and the model-level flip-aware parity / graph-replay tests against the oracle must pass there unchanged."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, VAMPIC_CONV="f16x2")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_ops.py"), "-q", "-x", "-m", "gpu",
                        "-k", "conv2d or deconv or gdn or tiling or float64 or rem_block or epilogue"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "passed" in r.stdout
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_model.py"), "-q", "-x", "-m", "gpu",
                        "-k", "flip_aware or graph_replay"],      # (the 48-case parity sweep is the default arithmetic's test: 95 s)
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "passed" in r.stdout
