"""Per-image qualities in one batch on the GPU: vam_variance_masks_per_image against vam_variance_mask per
(image, level) and the numpy oracle per segment, and forward_per_image / forward_qualities_per_image / compress_per_image /
decompress_per_image / compress_to_bytes / rd_at_qualities against the single-image functions they batch: bit for bit
(log2 sums to their float64 summation order, relative 1e-12: the bound of the sweep tests), with one graph per plan."""
import argparse
import copy
import ctypes
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                              # noqa: E402
import vampic.synth as synth               # noqa: E402
import vampic_oracle as O                  # noqa: E402
from vampic import _lib as L, evaluate as EV, ops     # noqa: E402

README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
_NETS = {}


def _net(kind="pic", **over):
    """Models live for the session, are updated once at birth and never drop a plan afterwards (tests/test_gpu_runtime.py
    counts on room below the retirement cap)."""
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


def _eager(kind="pic", **over):
    """The twin the single-image references run on, hipGraph off: a reference at a new quality captures nothing."""
    key = ("eager", kind) + tuple(sorted(over.items()))
    if key not in _NETS:
        net = copy.deepcopy(_net(kind, **over))
        net.use_graph = False
        _NETS[key] = net
    return _NETS[key]


def _x(B, H, W, seed=3):
    return synth.synth_image(B, H, W, seed=seed).cuda()


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_image(out, b, ref, what):
    """Image b of the batched dict ``out`` against the single-image dict ``ref``."""
    for k in ("x_hat", "y_hat", "mask"):
        assert torch.equal(out[k][b], ref[k][0]), (what, k)
    for k in ("y", "z"):
        assert torch.equal(out["likelihoods"][k][b], ref["likelihoods"][k][0]), (what, "likelihoods", k)
    rel = _rel(out["log2_likelihood_sum"][:, b], ref["log2_likelihood_sum"][:, 0])
    print(f"{what}: log2_likelihood_sum rel = {rel:.3e}")
    assert rel <= 1e-12, (what, rel)


# ----------------------------------------------------------------------------------------------- kernel
LISTS = [[5.0, 0.0, 12.0, 0.37, 5.0], [10.0, 0.3], [7.7, 0.05, 2.5, 0.0, 1.0, 9.99, 0.6, 3.0]]


@pytest.mark.parametrize("hw", [(16, 16), (32, 48), (64, 96)])          # the MAXV = 4, 16 and 0 instantiations
def test_masks_per_image_equal_single_image_masks_and_the_oracle(hw):
    h, w = hw
    B, ns, C = 3, 10, 32
    s = synth.synth_sigma(B, ns * C * h * w, seed=11).reshape(B, ns * C, h, w)
    s[0, 3 * C + 5, 1, 2] = float("nan")                                  # a NaN segment: (image 0, slice 3)
    s[1, 2 * C:3 * C] = torch.round(s[1, 2 * C:3 * C] * 2) / 2           # ties: (image 1, slice 2) holds a few distinct values
    s[2, 7 * C:8 * C] = 1.25                                              # ... and (image 2, slice 7) one value
    sg = ops.from_nchw(s.cuda())
    NL = L.VAM_MAX_MASK_LEVELS
    assert max(len(r) for r in LISTS) == NL
    mask = ops.new_view(NL * B, h, w, ns * C, zero=True)
    thr = torch.full((NL, B * ns), -7.0, dtype=torch.float32, device="cuda")
    table = torch.from_numpy(ops.mask_table(LISTS, h * w, C)).cuda()
    assert table.numel() == B * ctypes.sizeof(L.VamLayerParams)
    ops.variance_masks_per_image(sg, table, mask, n_slice=ns, thr=thr)
    torch.cuda.synchronize()
    s_np = s.numpy()
    for b, row in enumerate(LISTS):
        one = ops.View(sg.buf[b:b + 1], sg.c0, sg.C)
        for l, q in enumerate(row):
            m1 = ops.new_view(1, h, w, ns * C)
            t1 = torch.empty((ns,), dtype=torch.float32, device="cuda")
            ops.variance_mask(one, q, m1, n_slice=ns, thr=t1)
            got = mask.buf[l * B + b]
            assert torch.equal(got, m1.buf[0]), (b, l, q)
            assert _same_bits(thr[l, b * ns:(b + 1) * ns], t1), (b, l, q)
            got_nchw = got.permute(2, 0, 1).cpu().numpy()
            for j in range(ns):
                ref = O.variance_mask_np(s_np[b:b + 1, j * C:(j + 1) * C], q)[0]
                assert np.array_equal(got_nchw[j * C:(j + 1) * C], ref), (b, l, q, j)
        assert bool((thr[len(row):, b * ns:(b + 1) * ns] == -7.0).all()), b       # rows beyond the image's count: untouched
        assert float(mask.buf[len(row) * B + b:: B].abs().sum()) == 0.0 if len(row) < NL else True
    assert torch.isnan(thr[0, 3]) and float(mask.buf[0 * B + 0][..., 3 * C:4 * C].sum()) == 0.0   # NaN segment: all zero


# ----------------------------------------------------------------------------------------------- forward
def _forward_case(net, ref, x, qs, what):
    with torch.no_grad():
        out = net.forward_per_image(x, qs)
        for b, q in enumerate(qs):
            _check_image(out, b, ref.forward_single_quality(x[b:b + 1], q, training=False), f"{what} image {b} q {q}")
    return out


def test_forward_per_image_equals_single_images_and_keeps_one_graph():
    net, ref = _net(), _eager()
    x = _x(4, 128, 128)
    _forward_case(net, ref, x, [2.5, 10.0, 0.03, 0.7], "forward_per_image")
    plan = net._plan(x, base_only=False, per_image=True)
    assert plan.per_image and len(plan.runner.graphs) == 1
    gone = ops.retired_graphs() + ops.graveyard_size()
    with torch.no_grad():
        for qs in ([1.0, 1.0, 9.0, 0.2], [0.05, 3.0, 12.0, 6.5], [4.0, 0.5, 0.25, 0.01]):
            out = net.forward_per_image(x, qs)
            assert tuple(out["x_hat"].shape) == (4, 3, 128, 128)
    assert net._plan(x, base_only=False, per_image=True) is plan
    assert len(plan.runner.graphs) == 1
    assert ops.retired_graphs() + ops.graveyard_size() == gone
    # the last vector against the references too: the one graph really read the new table
    with torch.no_grad():
        _check_image(out, 2, ref.forward_single_quality(x[2:3], 0.25, training=False), "third vector, image 2")


def test_forward_per_image_all_scalable_false():
    net, ref = _net(all_scalable=False), _eager(all_scalable=False)
    _forward_case(net, ref, _x(3, 64, 128, seed=5), [0.08, 10.0, 3.3], "all_scalable=False")


def test_forward_qualities_per_image():
    net, ref = _net(), _eager()
    x = _x(2, 128, 128, seed=4)
    Q = [[0.5, 2.0], [0.0, 0.0], [10.0, 0.04]]
    with torch.no_grad():
        outs = net.forward_qualities_per_image(x, Q)
        assert len(outs) == 3
        for t, row in enumerate(Q):
            for b, q in enumerate(row):
                r = ref.forward_single_quality(x[b:b + 1], q, training=False)
                if q == 0:
                    assert "mask" not in outs[t]
                    for k in ("x_hat", "y_hat"):
                        assert torch.equal(outs[t][k][b], r[k][0]), (t, b, k)
                    for k in ("y", "z"):
                        assert torch.equal(outs[t]["likelihoods"][k][b], r["likelihoods"][k][0]), (t, b, k)
                    assert _rel(outs[t]["log2_likelihood_sum"][:, b], r["log2_likelihood_sum"][:, 0]) <= 1e-12
                else:
                    _check_image(outs[t], b, r, f"row {t} image {b} q {q}")
        one = net.forward_qualities_per_image(x, [0.5, 2.0])               # a [B] vector: T = 1
        assert len(one) == 1 and torch.equal(one[0]["x_hat"], outs[0]["x_hat"])
    sw = net._sweep_plan(x)
    assert all(len(t.runner.graphs) == 1 for t in sw.pi_tails.values()) and sw.pi_tails


# ----------------------------------------------------------------------------------------------- bitstream
def test_compress_and_decompress_per_image():
    net, ref = _net(), _eager()
    x = _x(3, 64, 128, seed=6)
    qs = [1.5, 0.0, 0.2]
    with torch.no_grad():
        items = net.compress_per_image(x, qs)
        assert len(items) == 3
        for b, q in enumerate(qs):
            want = ref.compress(x[b:b + 1], q)
            assert items[b]["strings"] == want["strings"], (b, q)
            assert tuple(items[b]["shape"]) == tuple(want["shape"]) and items[b]["quality"] == q
        dec = net.decompress_per_image(items)["x_hat"]
        assert tuple(dec.shape) == tuple(x.shape)
        for b, q in enumerate(qs):
            assert torch.equal(dec[b], ref.forward_single_quality(x[b:b + 1], q, training=False)["x_hat"][0]), (b, q)
        # other qualities through the same plans: still one graph on the symbols plan
        items2 = net.compress_per_image(x, [0.3, 4.0, 0.0])
        assert items2[1]["strings"] == ref.compress(x[1:2], 4.0)["strings"]
    plan = net._plan(x[:2], base_only=False, symbols=True, per_image=True)
    assert len(plan.runner.graphs) == 1
    with pytest.raises(ValueError, match="same shape"):
        net.decompress_per_image([items[0], dict(items[1], shape=(2, 2))])


def test_bitstream_pair_sub_batches_by_the_plan_size(monkeypatch):
    net = _net()
    x = _x(3, 128, 128)
    qs = [0, 2.5, 0.7]
    with torch.no_grad():
        items = net.compress_per_image(x, qs)
        dec = net.decompress_per_image(items)["x_hat"]
        monkeypatch.setattr(sys.modules["vampic.models"], "MAX_PLAN_PIXELS", 128 * 128)      # one image per plan
        items1 = net.compress_per_image(x, qs)
        dec1 = net.decompress_per_image(items1)["x_hat"]
    assert any(k[0] == 1 and k[-1] == "per_image" for k in net._dec_plans)   # the patched run decoded the positives one by one
    for a, b in zip(items, items1):
        assert a["strings"] == b["strings"] and tuple(a["shape"]) == tuple(b["shape"]) and a["quality"] == b["quality"]
    assert [it["quality"] for it in items1] == [0.0, 2.5, 0.7]
    assert tuple(dec.shape) == tuple(x.shape) and torch.equal(dec, dec1)


def _total(item):
    return sum(len(s) for part in item["strings"][0] for s in part) + sum(len(s) for s in item["strings"][1])


def test_compress_to_bytes_and_bpp():
    net, ref = _net(), _eager()
    x = torch.cat([_x(1, 128, 128, seed=3), _x(1, 128, 128, seed=4) * 0.5, _x(1, 128, 128, seed=7)])
    with torch.no_grad():
        ends = net.coded_size_curve(x, [0, 10])
        lo, hi = ends["bytes_hi"][0].double(), ends["bytes_lo"][1].double()
        assert bool((hi > lo).all())
        for f in (0.3, 0.7):                                             # two budgets per image, between the base and q = 10
            budget = lo + f * (hi - lo)
            res = net.compress_to_bytes(x, budget)
            assert res["reached"].all() and len(res["items"]) == 3
            for b in range(3):
                print(f"f = {f}, image {b}: budget {float(budget[b]):.0f}, coded {_total(res['items'][b])}, q {float(res['quality'][b]):.4f}")
                assert _total(res["items"][b]) <= float(budget[b])
                assert _total(res["items"][b]) <= float(res["bytes_hi"][b])
            sol = net.qualities_for_bytes(x, budget.unsqueeze(0))
            assert torch.equal(sol["quality"][0], res["quality"])
            again = net.compress_per_image(x, sol["quality"][0].tolist())
            assert [it["strings"] for it in again] == [it["strings"] for it in res["items"]]
        budget = torch.stack([lo[0] * 0.5, lo[1] + 0.5 * (hi[1] - lo[1]), lo[2] * 0.9])     # two below the base
        res = net.compress_to_bytes(x, budget)
        assert res["reached"].tolist() == [False, True, False] and res["quality"][0] == 0 and res["quality"][2] == 0
        for b in (0, 2):
            assert res["items"][b]["strings"] == ref.compress(x[b:b + 1], 0)["strings"]
        assert _total(res["items"][1]) <= float(budget[1])
        one = net.compress_to_bytes(x, float(hi.max()) * 2)              # a scalar: the same budget for every image
        assert one["reached"].all() and (one["quality"] == 10).all()
        rate = net.rate_curve(x, [0, 10])["bpp"]
        tb = rate[0] + 0.5 * (rate[1] - rate[0])
        rb = net.compress_to_bpp(x, tb)
        sol = net.qualities_for_bpp(x, tb.unsqueeze(0))
        assert rb["reached"].all() and torch.equal(rb["quality"], sol["quality"][0])
        assert _rel(rb["bpp"], sol["bpp"][0]) <= 1e-12                  # (two runs differ in their float64 summation order)
        assert rb["items"][1]["strings"] == ref.compress(x[1:2], float(rb["quality"][1]))["strings"]


# ----------------------------------------------------------------------------------------------- evaluation driver
def test_rd_at_qualities_equals_rd_sweep_per_image():
    net = _net()
    x = torch.cat([_x(1, 128, 128, seed=3), _x(1, 128, 128, seed=4) * 0.5])
    Q = torch.tensor([[0.5, 0.0], [2.0, 1.0], [0.0, 10.0]], dtype=torch.float64)
    bpp, psnr = EV.rd_at_qualities(net, x, Q)
    assert tuple(bpp.shape) == tuple(psnr.shape) == (3, 2) and bpp.dtype == psnr.dtype == torch.float64
    for b in range(2):
        r, p_ = EV.rd_sweep(net, x[b:b + 1], Q[:, b].tolist())
        print(f"image {b}: bpp rel = {_rel(bpp[:, b], r[:, 0]):.3e}, psnr rel = {_rel(psnr[:, b], p_[:, 0]):.3e}")
        assert _rel(bpp[:, b], r[:, 0]) <= 1e-12 and _rel(psnr[:, b], p_[:, 0]) <= 1e-12


# ----------------------------------------------------------------------------------------------- loops and refusals
def test_rem_model_loops():
    net = _net("rem")
    assert not net._batch_shareable()
    x = _x(2, 64, 64)
    qs = [0.5, 3.0]
    with torch.no_grad():
        out = net.forward_per_image(x, qs)
        for b, q in enumerate(qs):
            _check_image(out, b, net.forward_single_quality(x[b:b + 1], q, training=False), f"rem image {b}")
    assert not any(isinstance(k, tuple) and "per_image" in k for k in net._plans)


def test_bf16_storage_refuses_as_compress_does():
    if "bf16" not in _NETS:
        _NETS["bf16"] = copy.deepcopy(_eager())
        _NETS["bf16"].storage = "bf16"
    net = _NETS["bf16"]
    x = _x(2, 64, 64)
    with pytest.raises(NotImplementedError) as e1:
        net.compress(x[:1], 1.0)
    with pytest.raises(NotImplementedError) as e2:
        net.compress_per_image(x, [1.0, 2.0])
    assert str(e1.value) == str(e2.value)
    with torch.no_grad():                                                # the forward loops over single images
        out = net.forward_per_image(x, [1.0, 2.0])
        assert torch.equal(out["x_hat"][1], net.forward_single_quality(x[1:2], 2.0, training=False)["x_hat"][0])
