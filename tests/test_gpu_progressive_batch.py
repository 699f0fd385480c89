"""Batched progressive containers on the fused plans (progressive.encode_batch / ProgressiveDecoder):
the two kernels against the launches they stand for, the container against the eager harness and compress(), every
decoded level against forward_single_quality bit for bit, incremental decoding, batch invariance, graph replay,
corruption, the refusals and evaluate.progressive_rd."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                                         # noqa: E402
import vampic.synth as synth                          # noqa: E402
from vampic import _lib as L, bitstream as bs, evaluate as EV, ops, progressive as P   # noqa: E402

README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
DEMO_Q = [0.01, 0.05, 0.1, 0.25, 0.5, 0.6, 0.7, 0.8, 0.9, 1, 2, 3, 4, 4.5, 10]       # test/parser.py:20
_NETS = {}


def _net(kind="pic", **over):
    key = (kind,) + tuple(sorted(over.items()))
    if key not in _NETS:
        a = dict(README_ARGS, **over)
        if kind == "rem":
            a.update(check_levels=[0.01, 0.25, 1.75], mu_std=True, dimension="big")
        net = vampic.get_model(argparse.Namespace(model=kind, **a), "cpu").eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
        net = net.cuda()
        net.update()
        _NETS[key] = net
    return _NETS[key]


def _x(B, H, W, seed=3):
    return synth.synth_image(B, H, W, seed=seed).cuda()


def _sigma(B, h, w, seed=0):
    """Progressive-sigma-like input of 10 slices x 32 channels: slice 3 constant (ties), slice 7 of image 0 holds a NaN."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand((B, 320, h, w), generator=g) * 4 + 0.05
    s[:, 3 * 32:4 * 32] = 1.25
    s[0, 7 * 32 + 5, 1, 2] = float("nan")
    s[:, 9 * 32:10 * 32] = torch.round(s[:, 9 * 32:10 * 32] * 2) / 2            # many ties
    return ops.from_nchw(s.cuda())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("hw", [(16, 16), (32, 48)])
@pytest.mark.parametrize("qs", [[2.5], [0, 0.05, 0.5, 0.5, 1, 2.5, 10, 12], DEMO_Q,
                                sorted([0, 0, 0.01, 0.05, 0.1, 0.2, 0.25, 0.3, 0.5, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 1, 1.25, 1.5,
                                        2, 2.5, 3, 3.5, 4, 4.5, 5, 6, 6.6, 7, 8, 9, 10, 12])])
def test_variance_layers_kernel(hw, qs):
    assert len(qs) <= 32
    h, w = hw
    sg = _sigma(2, h, w)
    layer = torch.empty((2, h, w, 320), dtype=torch.uint8, device="cuda")
    thr = torch.empty((len(qs), 20), dtype=torch.float32, device="cuda")
    ops.variance_layers(sg, qs, layer, n_slice=10, thr=thr)
    mask = ops.new_view(2, h, w, 320, "cuda")
    t1 = torch.empty(20, dtype=torch.float32, device="cuda")
    for k, q in enumerate(qs):
        ops.variance_mask(sg, q, mask, n_slice=10, thr=t1)
        assert torch.equal(layer <= k, mask.buf == 1), (k, q)
        assert torch.equal(_bits(thr[k]), _bits(t1)), (k, q)
    assert (layer[0, :, :, 7 * 32:8 * 32] == (qs.index(10) if 10 in qs else 255)).all()    # NaN segment: only q >= 10


def test_variance_layers_refuses_unsorted_and_too_many():
    sg = _sigma(1, 16, 16)
    layer = torch.empty((1, 16, 16, 320), dtype=torch.uint8, device="cuda")
    with pytest.raises(L.VamError, match="non-decreasing"):
        ops.variance_layers(sg, [1, 0.5], layer, n_slice=10)
    with pytest.raises(L.VamError):
        ops.variance_layers(sg, [0.1] * 33, layer, n_slice=10)


@pytest.mark.parametrize("n", [1, 3, 8])
def test_gauss_levels_decode_equals_eval(n):
    B, h, w, d = 2, 16, 24, 320
    g = torch.Generator().manual_seed(n)
    mk = lambda s: ops.from_nchw((torch.randn((B, d, h, w), generator=g) * s).cuda())
    y, y2, mu = mk(3.0), mk(1.0), mk(2.0)
    sg = ops.from_nchw((torch.rand((B, d, h, w), generator=g) * 3 + 0.05).cuda())
    qs = [0, 0.05, 0.5, 0.5, 1, 2.5, 5, 10]
    layer = torch.empty((B, h, w, d), dtype=torch.uint8, device="cuda")
    ops.variance_layers(sg, qs, layer, n_slice=10)
    ones = ops.new_view(B, h, w, d, "cuda")
    ops.variance_mask_levels(sg, [10.0], ones, n_slice=10)
    sym = ops.new_iview(B, h, w, d, "cuda")
    ops.gauss_levels_eval(y, mu, sg, ones, 1, y2=y2, sym=sym)                    # the q = 10 symbols round(r - mu)
    for start in range(0, len(qs) - n + 1, max(1, n // 2)):
        ks = list(range(start, start + n))
        masks, want = ops.new_view(n * B, h, w, d, "cuda"), ops.new_view(n * B, h, w, d, "cuda")
        ops.variance_mask_levels(sg, [qs[k] for k in ks], masks, n_slice=10)
        ops.gauss_levels_eval(y, mu, sg, masks, n, y2=y2, yhat=want)
        got = ops.new_view(n * B, h, w, d, "cuda")
        ops.gauss_levels_decode(sym, layer, mu, ks, got)
        assert torch.equal(_bits(got.buf), _bits(want.buf)), ks


def _equal_levels(net, x, q_list, dec, ks=None):
    ks = list(range(len(q_list) + 1)) if ks is None else ks
    outs = dec.decode_levels(ks)
    with torch.no_grad():
        for k, o in zip(ks, outs):
            fw = net.forward_single_quality(x, 0 if k == 0 else q_list[k - 1])
            assert torch.equal(o["x_hat"], fw["x_hat"]), k
            assert torch.equal(o["y_hat"], fw["y_hat"]), k


def test_container_b1_matches_eager_and_compress():
    net = _net()
    x = _x(1, 128, 128, seed=5)
    q_list = [0.05, 0.5, 0.5, 1, 2.5, 5]
    cs, bits = P.encode_batch(net, x, q_list)
    c = cs[0]
    eager, ebits = P.encode(net, x, q_list=q_list)
    assert set(c) == set(eager) == {"q_list", "shape", "z", "base", "progressive"}
    assert c["q_list"] == eager["q_list"] and tuple(c["shape"]) == tuple(eager["shape"])
    assert len(c["progressive"]) == len(q_list) and all(len(l_) == net.ns0 for l_ in c["progressive"])
    assert bits[0] == P.container_bits(c)
    enc0 = net.compress(x, quality=0)
    assert c["z"] == enc0["strings"][1] and c["base"] == enc0["strings"][0]
    # each layer decodes to compress(x, 10)'s progressive symbols on that layer and 0 elsewhere
    with torch.no_grad():
        sym10 = net.compress(x, quality=10, real_compress=False)["strings"][0]
        fw10 = net.forward_single_quality(x, 10)
        gc = net.gaussian_conditional
        idx = gc.build_indexes(fw10["std"]).int().cpu().numpy()[0]          # [d, h, w]
        masks = [torch.zeros_like(fw10["std"])] + [net.forward_single_quality(x, q)["mask"] for q in q_list]
    sym_p = torch.cat(sym10[net.ns0:], 1).int().cpu().numpy()[0]
    tg = bs.Tables.of(gc)
    C = net.dim_chunk
    for k in range(len(q_list)):
        delta = (masks[k + 1] - masks[k]).int().cpu().numpy()[0]
        assert delta.min() >= 0
        for j in range(net.ns0):
            s_ = slice(j * C, (j + 1) * C)
            got = bs.decode(c["progressive"][k][j], idx[s_] * delta[s_], tg).reshape(delta[s_].shape)
            assert np.array_equal(got * delta[s_], sym_p[s_] * delta[s_]), (k, j)
            assert np.array_equal(got[delta[s_] == 0], np.zeros(int((delta[s_] == 0).sum()), np.int32)), (k, j)
    # the eager decoder reads the new container, the new decoder the eager one (today's tolerances)
    dec = P.ProgressiveDecoder(net, [eager])
    with torch.no_grad():
        for k in (0, 2, len(q_list)):
            fw = net.forward_single_quality(x, 0 if k == 0 else q_list[k - 1])
            e = P.decode(net, c, q_ind=k)
            assert (e["x_hat"].clamp(0, 1) - fw["x_hat"]).abs().max().item() <= 1e-5, k
            if k:
                assert (e["y_prog"] - fw["y_hat"]).abs().max().item() <= 1e-4, k
            n = dec.decode(k)
            assert (n["x_hat"] - fw["x_hat"]).abs().max().item() <= 1e-5, k
            assert (n["y_hat"] - fw["y_hat"]).abs().max().item() <= 1e-4, k


def test_exact_demo_levels_256():
    net = _net()
    x = _x(1, 256, 256, seed=0)
    cs, _ = P.encode_batch(net, x, DEMO_Q)
    _equal_levels(net, x, DEMO_Q, P.ProgressiveDecoder(net, cs))


def test_exact_q_list_batch_of_3():
    net = _net()
    x = _x(3, 128, 192, seed=1)
    cs, bits = P.encode_batch(net, x, P.Q_LIST)
    assert len(cs) == 3 and len(bits) == 3
    _equal_levels(net, x, P.Q_LIST, P.ProgressiveDecoder(net, cs))


def test_exact_single_decoder_and_hyperprior():
    net = _net(multiple_decoder=False, multiple_hyperprior=False, support_progressive_slices=2)
    x = _x(2, 64, 128, seed=2)
    q_list = [0.1, 0.5, 1, 3, 10]
    cs, _ = P.encode_batch(net, x, q_list)
    _equal_levels(net, x, q_list, P.ProgressiveDecoder(net, cs))


def test_incremental_decoding_and_levels():
    net = _net()
    x = _x(1, 128, 128, seed=4)
    cs, _ = P.encode_batch(net, x, DEMO_Q)
    d1 = P.ProgressiveDecoder(net, cs)
    d1.decode(3)
    assert d1.layers_decoded == 3
    a = d1.decode(9)
    assert d1.layers_decoded == 9
    d1.decode(2)
    assert d1.layers_decoded == 9
    b = P.ProgressiveDecoder(net, cs).decode(9)
    assert torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"])
    ks = [0, 3, 9, 14]
    many = P.ProgressiveDecoder(net, cs).decode_levels(ks)
    for k, o in zip(ks, many):
        s = P.ProgressiveDecoder(net, cs).decode(k)
        assert torch.equal(o["x_hat"], s["x_hat"]) and torch.equal(o["y_hat"], s["y_hat"]), k
    assert d1.bits(9) == [P.bits_up_to(cs[0], 9)] and d1.bits(0)[0] < d1.bits(9)[0]


def test_batch_invariance_and_graph_replay():
    net = _net()
    x = _x(4, 64, 128, seed=6)
    q_list = [0.05, 0.5, 1, 2.5, 5]
    cs, bits = P.encode_batch(net, x, q_list)
    for b in range(4):
        cb, bb = P.encode_batch(net, x[b:b + 1], q_list)
        assert cb[0] == cs[b] and bb[0] == bits[b], b
    d1 = P.ProgressiveDecoder(net, cs)
    r1 = d1.decode_levels([0, 2, 5])
    d2 = P.ProgressiveDecoder(net, cs)                     # same plans, graphs replayed
    r2 = d2.decode_levels([0, 2, 5])
    r1b = d1.decode_levels([0, 2, 5])                      # d1 again after d2 used the plans
    for a, b, c in zip(r1, r2, r1b):
        assert torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["x_hat"], c["x_hat"])
        assert torch.equal(a["y_hat"], b["y_hat"]) and torch.equal(a["y_hat"], c["y_hat"])


def test_truncated_layer_raises():
    net = _net()
    x = _x(1, 64, 64, seed=8)
    cs, _ = P.encode_batch(net, x, [0.5, 1, 2.5])
    bad = dict(cs[0])
    bad["progressive"] = [list(l_) for l_ in cs[0]["progressive"]]
    bad["progressive"][1][4] = bad["progressive"][1][4][:8]
    dec = P.ProgressiveDecoder(net, [bad])
    dec.decode(1)
    with pytest.raises(L.VamError):
        dec.decode(2)


def test_refusals(monkeypatch):
    x = _x(1, 64, 64)
    with pytest.raises(NotImplementedError, match="eager harness"):
        P.encode_batch(_net("rem"), x, [0.5, 1])
    for over in (dict(all_scalable=False), dict(delta_encode=False)):
        with pytest.raises(NotImplementedError):
            P.encode_batch(_net(**over), x, [0.5, 1])
    net = _net()
    with pytest.raises(ValueError, match="non-decreasing"):
        P.encode_batch(net, x, [1, 0.5])
    cs, _ = P.encode_batch(net, x, [0.5, 1])
    cs2, _ = P.encode_batch(net, x, [0.5, 2])
    cs3, _ = P.encode_batch(net, _x(1, 64, 128), [0.5, 1])
    with pytest.raises(ValueError, match="same shape and q_list"):
        P.ProgressiveDecoder(net, cs + cs2)
    with pytest.raises(ValueError, match="same shape and q_list"):
        P.ProgressiveDecoder(net, cs + cs3)
    monkeypatch.setattr(net, "storage", "bf16")
    with pytest.raises(NotImplementedError, match="eager harness"):
        P.encode_batch(net, x, [0.5, 1])
    with pytest.raises(NotImplementedError, match="eager harness"):
        P.ProgressiveDecoder(net, cs)
    monkeypatch.setattr(net, "storage", "fp32")
    monkeypatch.setattr(ops, "f16x2_mode", lambda: True)
    with pytest.raises(NotImplementedError, match="f16x2"):
        P.encode_batch(net, x, [0.5, 1])


def test_progressive_rd():
    net = _net()
    imgs = [synth.synth_image(1, 50, 100, seed=s).cuda() for s in (11, 12)]
    q_list = [0.05, 0.5, 2.5, 10]
    rows = EV.progressive_rd(net, imgs, q_list)
    assert len(rows) == len(q_list) + 1
    xp, unpad = EV.pad_image(torch.cat(imgs, 0))
    cs, _ = P.encode_batch(net, xp, q_list)
    dec = P.ProgressiveDecoder(net, cs)
    for k, r in enumerate(rows):
        out = torch.nn.functional.pad(dec.decode(k)["x_hat"], unpad)
        for i, x in enumerate(imgs):
            n_bytes = len(cs[i]["z"][0]) + sum(len(s[0]) for s in cs[i]["base"]) + \
                sum(len(s) for layer in cs[i]["progressive"][:k] for s in layer)
            assert r["bpp_all"][i] == 8.0 * n_bytes / (50 * 100)
            # compute_psnr's float64 sum is accumulated with atomics (order unspecified): equal to the last few ulps
            assert abs(r["psnr_all"][i] - EV.compute_psnr(x, out[i:i + 1])) <= 1e-9
        assert r["enc_s"] > 0 and r["dec_s"] > 0
    assert all(b["bpp"] > a["bpp"] for a, b in zip(rows, rows[1:]))
