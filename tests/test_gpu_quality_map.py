"""Quality maps on the GPU: vam_variance_mask_map against vam_variance_mask per (image, level) and the numpy
oracle per segment, and forward_quality_map / compress_quality_map / decompress_quality_map / quality_map_rate /
quality_map_for_bpp against the single-quality functions they compose: bit for bit (log2 sums to their float64 summation
order, relative 1e-12: the bound of the per-image tests), with one graph per plan."""
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
    """The twin the single-quality references run on, hipGraph off: a reference at a new quality captures nothing."""
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


# ----------------------------------------------------------------------------------------------- kernel
LIST32 = [0.0] + [round(0.05 + 0.34 * i, 4) for i in range(29)] + [10.0, 12.0]
LISTS = [[0.0, 0.37, 5.0, 10.0, 12.0], [2.5], LIST32]                   # 5, 1 and 32 levels; image 0 holds the NaN segment


@pytest.mark.parametrize("hw", [(16, 16), (32, 48), (64, 96)])          # the MAXV = 4, 16 and 0 instantiations
def test_mask_map_equals_single_image_masks_and_the_oracle(hw):
    h, w = hw
    B, ns, C = 3, 10, 32
    assert [len(r) for r in LISTS] == [5, 1, L.VAM_MAX_LAYER_LEVELS] and all(r == sorted(r) for r in LISTS) and max(LIST32[:-2]) < 10
    s = synth.synth_sigma(B, ns * C * h * w, seed=11).reshape(B, ns * C, h, w)
    s[0, 3 * C + 5, 1, 2] = float("nan")                                  # a NaN segment: (image 0, slice 3)
    s[1, 2 * C:3 * C] = torch.round(s[1, 2 * C:3 * C] * 2) / 2           # ties: (image 1, slice 2) holds a few distinct values
    s[2, 7 * C:8 * C] = 1.25                                              # ... and (image 2, slice 7) one value
    sg = ops.from_nchw(s.cuda())
    g = torch.Generator().manual_seed(5)
    lmap = torch.stack([torch.randint(0, 5, (h, w), generator=g), torch.zeros(h, w, dtype=torch.int64),     # image 1: constant
                        torch.randint(0, 32, (h, w), generator=g)]).to(torch.uint8)
    lmap[0, 0, 0], lmap[0, 0, 1], lmap[0, h - 1, w - 1] = 0, 3, 4         # (every level of image 0 is used, whatever the draw)
    bad = [(0, 2, 3, 5), (0, h - 1, 0, 255), (2, 1, 1, 32), (2, h - 2, w - 1, 200)]      # entries beyond the image's list
    for b, y_, x_, v in bad:
        lmap[b, y_, x_] = v
    NL = L.VAM_MAX_LAYER_LEVELS
    mask = ops.new_view(B, h, w, ns * C)
    mask.buf.fill_(-3.0)                                                  # every element must be written
    thr = torch.full((NL, B * ns), -7.0, dtype=torch.float32, device="cuda")
    table = torch.from_numpy(ops.layer_table(LISTS, h * w, C)).cuda()
    assert table.numel() == B * ctypes.sizeof(L.VamLayerParams)
    ops.variance_mask_map(sg, table, lmap.cuda(), mask, n_slice=ns, thr=thr)
    torch.cuda.synchronize()
    got_all = mask.buf.cpu()                                              # [B, h, w, ns * C]
    assert bool(((got_all == 0) | (got_all == 1)).all())
    s_np = s.numpy()
    for b, row in enumerate(LISTS):
        one = ops.View(sg.buf[b:b + 1], sg.c0, sg.C)
        used = 0
        for k, q in enumerate(row):
            m1 = ops.new_view(1, h, w, ns * C)
            t1 = torch.empty((ns,), dtype=torch.float32, device="cuda")
            ops.variance_mask(one, q, m1, n_slice=ns, thr=t1)
            assert _same_bits(thr[k, b * ns:(b + 1) * ns], t1), (b, k, q)        # thresholds: those of the single launches
            pos = lmap[b] == k
            if not bool(pos.any()):
                continue
            used += 1
            assert torch.equal(got_all[b][pos], m1.buf[0].cpu()[pos]), (b, k, q)
            if (h, w) == (16, 16):                                        # ... and the oracle's, per segment
                got_nchw = got_all[b].permute(2, 0, 1).numpy()
                for j in range(ns):
                    ref = O.variance_mask_np(s_np[b:b + 1, j * C:(j + 1) * C], q)[0]
                    assert np.array_equal(got_nchw[j * C:(j + 1) * C][:, pos.numpy()], ref[:, pos.numpy()]), (b, k, q, j)
        assert used >= min(len(row), 5), (b, used)
        assert bool((thr[len(row):, b * ns:(b + 1) * ns] == -7.0).all()), b       # rows beyond the image's count: untouched
    for b, y_, x_, v in bad:
        assert float(got_all[b, y_, x_].abs().sum()) == 0.0, (b, y_, x_, v)       # an out-of-range entry writes 0
    nan_seg = got_all[0][..., 3 * C:4 * C]                                # the NaN segment of image 0, by the level of each position
    assert torch.isnan(thr[1, 3]) and torch.isnan(thr[2, 3])
    for k, want in ((0, 0.0), (1, 0.0), (2, 0.0), (3, 1.0), (4, 1.0)):   # q = 0: zero; needs the threshold: zero; q >= 10: one
        assert bool((nan_seg[lmap[0] == k] == want).all()), k


# ----------------------------------------------------------------------------------------------- forward
KEYS = ("x_hat", "y_hat", "y_base", "y_prog", "mu_base", "mu", "std_base", "std", "mask")


def _const_map(x, qs):
    h, w = x.shape[2] // 16, x.shape[3] // 16
    return torch.tensor(qs, dtype=torch.float64).view(-1, 1, 1).expand(len(qs), h, w).contiguous()


def test_constant_map_equals_single_quality_and_keeps_one_graph():
    net, ref = _net(), _eager()
    x = _x(4, 128, 128)
    qs = [0.08, 2.5, 10.0, 3.3]
    with torch.no_grad():
        out = net.forward_quality_map(x, _const_map(x, qs))
        for b, q in enumerate(qs):
            r = ref.forward_single_quality(x[b:b + 1], q, training=False)
            assert set(out) == set(r)
            for k in KEYS:
                assert torch.equal(out[k][b], r[k][0]), (b, q, k)
            for k in ("y", "z"):
                assert torch.equal(out["likelihoods"][k][b], r["likelihoods"][k][0]), (b, q, "likelihoods", k)
            rel = _rel(out["log2_likelihood_sum"][:, b], r["log2_likelihood_sum"][:, 0])
            print(f"constant map, image {b} q {q}: log2_likelihood_sum rel = {rel:.3e}")
            assert rel <= 1e-12, (b, q, rel)
    plan = net._plan(x, base_only=False, quality_map=True)
    assert plan.quality_map and len(plan.runner.graphs) == 1
    gone = ops.retired_graphs() + ops.graveyard_size()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for vals in ([0.0, 1.0, 9.0], [0.05, 3.0, 12.0, 6.5], [4.0]):
            qmap = torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (4, 8, 8), generator=g)]
            out = net.forward_quality_map(x, qmap)
            assert tuple(out["x_hat"].shape) == (4, 3, 128, 128)
    assert net._plan(x, base_only=False, quality_map=True) is plan
    assert len(plan.runner.graphs) == 1
    assert ops.retired_graphs() + ops.graveyard_size() == gone
    with torch.no_grad():                                                 # the one graph really read the last map
        r = ref.forward_single_quality(x[2:3], 4.0, training=False)
    assert torch.equal(out["x_hat"][2], r["x_hat"][0]) and torch.equal(out["mask"][2], r["mask"][0])


def _block_map():
    """[2, 4, 8] for images 64 x 128: three values in blocks, one 0 and one 10; image 1 holds two of them."""
    qmap = torch.zeros(2, 4, 8, dtype=torch.float64)
    qmap[0, :, 3:6] = 2.5
    qmap[0, 2:, 6:] = 10.0
    qmap[1, :2] = 10.0
    qmap[1, 2:] = 2.5
    return qmap


def test_map_composes_single_quality_results_per_position():
    net, ref = _net(), _eager()
    x = _x(2, 64, 128)
    qmap = _block_map()
    d = net.division_dimension[0]
    with torch.no_grad():
        out = net.forward_quality_map(x, qmap)
        out_of_mask = None
        for q in (2.5, 10.0, 0.0):
            r = ref.forward_single_quality(x, q, training=False)
            pos = (qmap == q).cuda()[:, None].expand(-1, d, -1, -1)
            assert bool(pos.any())
            if q == 0:                                                    # the base dict: no mask, the base half of the likelihoods
                assert float(out["mask"][pos].abs().sum()) == 0.0
                assert torch.equal(out["likelihoods"]["y"][:, :d][pos], r["likelihoods"]["y"][pos])
                assert bool((out["likelihoods"]["y"][:, d:][pos] == out_of_mask).all())    # every element at L(0, 0)
                continue
            assert torch.equal(out["mask"][pos], r["mask"][pos]), q
            for half in (slice(0, d), slice(d, 2 * d)):
                assert torch.equal(out["likelihoods"]["y"][:, half][pos], r["likelihoods"]["y"][:, half][pos]), q
            if q == 2.5:
                out_of_mask = r["likelihoods"]["y"][:, d:][r["mask"] == 0][0]
            for k in ("mu", "std", "y_base"):                             # all_scalable: independent of the quality
                assert torch.equal(out[k], r[k]), (q, k)
        one = net.forward_quality_map(x[:1], qmap[:1])                    # image 0 alone, at B = 1
        for k in KEYS:
            assert torch.equal(one[k][0], out[k][0]), k
        for k in ("y", "z"):
            assert torch.equal(one["likelihoods"][k][0], out["likelihoods"][k][0]), k
        assert _rel(one["log2_likelihood_sum"][:, 0], out["log2_likelihood_sum"][:, 0]) <= 1e-12
        # ---- the rate of the same map, without masks, LRP stacks or g_s
        rate = net.quality_map_rate(x, qmap)
        rel = _rel(rate["log2_likelihood_sum"], out["log2_likelihood_sum"])
        print(f"quality_map_rate vs forward_quality_map: rel = {rel:.3e}")
        assert rate["log2_likelihood_sum"].dtype == torch.float64 and tuple(rate["log2_likelihood_sum"].shape) == (2, 2)
        assert rel <= 1e-12
        assert _rel(rate["bpp"], -out["log2_likelihood_sum"].sum(0) / (64 * 128)) <= 1e-12
        res = EV.rd_quality_map(net, x, qmap, region=torch.ones(2, 64, 128, dtype=torch.bool))
        assert _rel(res["bpp"], rate["bpp"].cpu()) <= 1e-12 and _rel(res["psnr_in"], res["psnr"]) <= 1e-12
        assert abs(float(res["psnr"][0]) - EV.compute_psnr(x[:1], out["x_hat"][:1])) <= 1e-9
        assert bool(torch.isnan(res["psnr_out"]).all())


# ----------------------------------------------------------------------------------------------- bitstream
def _mixed_map(B):
    g = torch.Generator().manual_seed(9)
    vals = torch.tensor([0.0, 0.3, 1.5, 4.0, 10.0], dtype=torch.float64)
    qmap = vals[torch.randint(0, 5, (B, 4, 8), generator=g)]
    qmap[0, :, :4] = 1.5
    return qmap


@pytest.mark.parametrize("all_scalable", [True, False])
def test_compress_and_decompress_quality_map(all_scalable):
    over = {} if all_scalable else {"all_scalable": False}
    net = _net(**over)
    x = _x(3, 64, 128, seed=6)
    qmap = _mixed_map(3)
    with torch.no_grad():
        items = net.compress_quality_map(x, qmap)
        assert len(items) == 3
        for b, it in enumerate(items):
            lv = sorted(set(qmap[b].flatten().tolist()))
            assert it["quality_map"]["levels"] == lv and it["quality_map"]["index"].dtype == np.uint8
            assert np.array_equal(np.asarray(lv)[it["quality_map"]["index"].astype(np.int64)], qmap[b].numpy())
            assert it["side_bytes"] == 8 * len(lv) + 4 * 8 and tuple(it["shape"]) == (1, 2)
            assert len(it["strings"][0]) == net.ns1 and len(it["strings"][1]) == 1
        fwd = net.forward_quality_map(x, qmap)
        dec = net.decompress_quality_map(items)["x_hat"]
        assert tuple(dec.shape) == tuple(x.shape) and torch.equal(dec, fwd["x_hat"])
        qs = [1.5, 0.2, 4.0]                                              # constant maps: the strings of compress_per_image
        const = net.compress_quality_map(x, _const_map(x, qs))
        want = net.compress_per_image(x, qs)
        for b in range(3):
            assert const[b]["strings"] == want[b]["strings"] and tuple(const[b]["shape"]) == tuple(want[b]["shape"]), b
            assert const[b]["quality_map"]["levels"] == [qs[b]] and const[b]["side_bytes"] == 8 + 32
    plan = net._plan(x, base_only=False, symbols=True, quality_map=True)
    assert len(plan.runner.graphs) == 1
    with pytest.raises(ValueError, match="same shape"):
        net.decompress_quality_map([items[0], dict(items[1], shape=(2, 2))])


def test_map_functions_sub_batch_by_the_plan_size(monkeypatch):
    net = _net()
    x = _x(3, 64, 128, seed=6)
    qmap = _mixed_map(3)
    with torch.no_grad():
        fwd, items, rate = net.forward_quality_map(x, qmap), net.compress_quality_map(x, qmap), net.quality_map_rate(x, qmap)
        monkeypatch.setattr(sys.modules["vampic.models"], "MAX_PLAN_PIXELS", 64 * 128)       # one image per plan
        fwd1, items1, rate1 = net.forward_quality_map(x, qmap), net.compress_quality_map(x, qmap), net.quality_map_rate(x, qmap)
        dec1 = net.decompress_quality_map(items1)["x_hat"]
    assert any(k[0] == 1 and k[-1] == "quality_map" for k in net._dec_plans)
    for k in KEYS:
        assert torch.equal(fwd[k], fwd1[k]), k
    assert [it["strings"] for it in items] == [it["strings"] for it in items1]
    assert torch.equal(dec1, fwd["x_hat"])
    assert _rel(rate1["log2_likelihood_sum"], rate["log2_likelihood_sum"]) <= 1e-12
    assert _rel(fwd1["log2_likelihood_sum"], fwd["log2_likelihood_sum"]) <= 1e-12


# ----------------------------------------------------------------------------------------------- the budget solver
def test_quality_map_for_bpp_meets_its_contract():
    net = _net()
    x = torch.cat([_x(1, 128, 128, seed=3), _x(1, 128, 128, seed=4) * 0.5, _x(1, 128, 128, seed=7)])
    floor = EV.quality_map_from_boxes(3, 128, 128, 0.0, [(b, 32, 32, 96, 96, 8.0) for b in range(3)])     # a centre box at q = 8
    assert tuple(floor.shape) == (3, 8, 8) and float(floor.sum()) == 3 * 16 * 8.0
    q_tol = 1e-3
    with torch.no_grad():
        r_floor = net.quality_map_rate(x, floor)["bpp"].cpu()
        r_full = net.quality_map_rate(x, torch.full_like(floor, 10.0))["bpp"].cpu()
        assert bool((r_full > r_floor).all())
        targets = torch.stack([r_floor - 0.1 * (r_full - r_floor), 0.5 * (r_floor + r_full), r_full + 0.1 * (r_full - r_floor)])
        sol = net.quality_map_for_bpp(x, floor, targets, q_tol=q_tol)
        assert all(tuple(sol[k].shape) == (3, 3) for k in ("quality", "bpp", "reached")) and tuple(sol["quality_map"].shape) == (3, 3, 8, 8)
        q = sol["quality"]
        assert sol["reached"].tolist() == [[False] * 3, [True] * 3, [True] * 3]
        assert bool((q[0] == 0).all()) and bool((q[2] == 10).all()) and bool(((q[1] > 0) & (q[1] < 10)).all())
        for t in range(3):
            want_map = torch.maximum(floor, q[t].view(3, 1, 1))
            assert torch.equal(sol["quality_map"][t], want_map), t
            at = net.quality_map_rate(x, want_map)["bpp"].cpu()
            above = net.quality_map_rate(x, torch.maximum(floor, (q[t] + q_tol).clamp(max=10.0).view(3, 1, 1)))["bpp"].cpu()
            for b in range(3):
                print(f"target {t} image {b}: t = {float(targets[t, b]):.6f}, q* = {float(q[t, b]):.5f}, bpp(q*) = {float(at[b]):.6f}, "
                      f"bpp(q* + tol) = {float(above[b]):.6f}, reached {bool(sol['reached'][t, b])}")
                if not sol["reached"][t, b]:
                    assert q[t, b] == 0 and at[b] > targets[t, b]          # the floor map alone exceeds the budget
                    continue
                assert at[b] <= targets[t, b]
                assert q[t, b] == 10 or above[b] > targets[t, b]
            assert _rel(sol["bpp"][t], at) <= 1e-12
    assert _rel(sol["bpp"][0], r_floor) <= 1e-12 and _rel(sol["bpp"][2], r_full) <= 1e-12


# ----------------------------------------------------------------------------------------------- refusals
def _map_calls(net, x, qmap):
    return [lambda: net.forward_quality_map(x, qmap), lambda: net.compress_quality_map(x, qmap),
            lambda: net.quality_map_rate(x, qmap), lambda: net.quality_map_for_bpp(x, qmap, 1.0),
            lambda: net.decompress_quality_map([{"strings": [[], []], "shape": (1, 1),
                                                 "quality_map": {"levels": [1.0], "index": np.zeros((4, 4), dtype=np.uint8)}}])]


def test_rem_models_are_refused():
    net = _net("rem")
    x = _x(2, 64, 64)
    for call in _map_calls(net, x, torch.ones(2, 4, 4)):
        with pytest.raises(NotImplementedError, match="REM"):
            call()
    assert not any(isinstance(k, tuple) and "quality_map" in k for k in net._plans)


def test_bf16_storage_is_refused():
    if "bf16" not in _NETS:
        _NETS["bf16"] = copy.deepcopy(_eager())
        _NETS["bf16"].storage = "bf16"
    net = _NETS["bf16"]
    x = _x(2, 64, 64)
    for call in _map_calls(net, x, torch.ones(2, 4, 4)):
        with pytest.raises(NotImplementedError, match="bf16 storage"):
            call()


def test_solver_refuses_two_levels_and_all_scalable_false():
    x = _x(2, 64, 64)
    floor = torch.zeros(2, 4, 4)
    floor[:, 1:3, 1:3] = 8.0
    with pytest.raises(ValueError, match="point-based-std"):
        _net().quality_map_for_bpp(x, floor, 1.0, mask_pol="two-levels")
    with pytest.raises(NotImplementedError, match="all_scalable"):
        _net(all_scalable=False).quality_map_for_bpp(x, floor, 1.0)
    with pytest.raises(ValueError, match="9 distinct"):
        _net().quality_map_for_bpp(x, (torch.arange(32).reshape(2, 4, 4) % 9).double(), 1.0)
