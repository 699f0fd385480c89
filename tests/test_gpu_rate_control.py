"""Rate control on the GPU (VarianceMaskingPIC.rate_curve / qualities_for_bpp): vam_gauss_layer_bits against
vam_gauss_levels_eval fed the masks layer <= k, the rate curve against one forward_single_quality per quality (float64 sums to
1e-12), no transform work per level, the solver's contract against forward_single_quality itself, the drivers, and the
configurations that loop or refuse."""
import argparse
import copy
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                              # noqa: E402
import vampic.synth as synth               # noqa: E402
from vampic import _lib as L, evaluate as EV, ops, progressive as PR     # noqa: E402

M = sys.modules["vampic.models"]
README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
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


def _eager(kind="pic", **over):
    """The same model with hipGraph off: the reference loops run on it, so that a probe at a new quality captures nothing.
    Like :func:`_net` it lives for the session and never drops a plan: a dropped plan's graphs are retired, and
    tests/test_gpu_runtime.py counts on room below the retirement cap."""
    key = ("eager", kind) + tuple(sorted(over.items()))
    if key not in _NETS:
        net = copy.deepcopy(_net(kind, **over))
        net.use_graph = False
        _NETS[key] = net
    return _NETS[key]


def _x(B, H, W, seed=3):
    return synth.synth_image(B, H, W, seed=seed).cuda()


def _v(t):
    return ops.from_nchw(t.cuda())


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _loop_sums(ref, x, qs, mask_pol=None):
    mp = ref.mask_policy if mask_pol is None else mask_pol
    with torch.no_grad():
        return torch.stack([ref.forward_single_quality(x, q, mp, training=False)["log2_likelihood_sum"] for q in qs])


def _check_curve(net, x, qs, what="", mask_pol=None, ref=None):
    """rate_curve of ``net`` against one forward_single_quality per quality on ``ref`` (default: the eager twin)."""
    got = net.rate_curve(x, qs, mask_pol=mask_pol)
    want = _loop_sums(_eager() if ref is None else ref, x, qs, mask_pol)
    ls, bpp = got["log2_likelihood_sum"], got["bpp"]
    assert ls.dtype == bpp.dtype == torch.float64 and tuple(ls.shape) == (len(qs), 2, x.shape[0]) and tuple(bpp.shape) == (len(qs), x.shape[0])
    for k, q in enumerate(qs):
        for row in range(2):
            r = _rel(ls[k, row], want[k, row])
            print(f"rate_curve {what} q={q} row={row}: rel = {r:.3e}")
            assert r < 1e-12, (what, k, q, row, r)
    assert torch.equal(bpp, -ls.sum(1) / (x.shape[2] * x.shape[3]))
    return got


# ----------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("n_levels", [1, 5, 32])
@pytest.mark.parametrize("with_y2", [True, False])
def test_gauss_layer_bits_equals_levels_eval_on_layer_masks(n_levels, with_y2):
    B, h, w, d = 2, 8, 12, 128
    ns = d // 32
    y = synth.normal((B, 2 * d, h, w), 40) * 4
    musg = synth.normal((B, 3 * d, h, w), 41) * 2                       # mu and sigma: windows of one wider tensor
    musg[:, 2 * d:] = musg[:, 2 * d:].abs() * 0.5
    musg[0, 2 * d:2 * d + 5] = 0.05                                      # below the 0.11 bound
    musg[1, 2 * d + 32:2 * d + 64, 0, 0] = float("nan")                  # a NaN segment: in no layer unless the list holds q >= 10
    y_v, ms_v = _v(y), _v(musg)
    y_top, y_sub = y_v.window(d, d), (y_v.window(0, d) if with_y2 else None)
    mu, sg = ms_v.window(0, d), ms_v.window(2 * d, d)                   # pixel stride 3d != C
    qs32 = sorted([0.0, 0.0, 0.003, 0.05, 0.1, 0.25, 0.5, 0.5, 0.75, 1, 1.25, 1.5, 2, 2.5, 2.5, 3, 3.5, 4, 4.5, 5, 5.5, 6, 6.5, 7,
                   7.5, 8, 8.5, 9, 9.5, 9.9, 10, 10])
    prs = {1: [2.5], 5: [0.0, 0.5, 0.5, 5.0, 9.99], 32: qs32}[n_levels]  # q = 0, q = 10 and repeats in the lists
    layer = torch.empty((B, h, w, d), dtype=torch.uint8, device="cuda")
    ops.variance_layers(sg, prs, layer, n_slice=ns)
    nb = n_levels + 1
    bits = torch.zeros((B, nb), dtype=torch.float64, device="cuda")
    count = torch.zeros((B, nb), dtype=torch.int64, device="cuda")
    ops.gauss_layer_bits(y_top, mu, sg, layer, n_levels, bits, count, y2=y_sub)
    torch.cuda.synchronize()
    # counts: exact
    lay = layer.long()
    lay[lay == L.LAYER_NONE] = n_levels
    want_count = torch.stack([torch.bincount(lay[b].flatten(), minlength=nb) for b in range(B)])
    assert torch.equal(count, want_count), (count, want_count)
    assert int(count[1, n_levels]) >= (0 if max(prs) >= 10 else 32 * h * w)
    # sums: level k against vam_gauss_levels_eval fed the mask layer <= k
    outside = ops.log2_lik_outside("cuda")
    n = h * w * d
    got = bits[:, :n_levels].cumsum(1) + (n - count[:, :n_levels].cumsum(1)).double() * outside
    for k0 in range(0, n_levels, 8):
        ks = list(range(k0, min(k0 + 8, n_levels)))
        masks = ops.new_view(len(ks) * B, h, w, d)
        for i, k in enumerate(ks):
            masks.buf[i * B:(i + 1) * B] = (layer <= k).float()
        ls = torch.zeros((len(ks), B), dtype=torch.float64, device="cuda")
        ops.gauss_levels_eval(y_top, mu, sg, masks, len(ks), y2=y_sub, log2sum=ls)
        torch.cuda.synchronize()
        for i, k in enumerate(ks):
            good = torch.isfinite(ls[i])                                  # (a non-finite sum, if there is one, is non-finite in both)
            assert torch.equal(good, torch.isfinite(got[:, k]))
            r = _rel(got[good, k], ls[i][good])
            print(f"layer_bits n_levels={n_levels} y2={with_y2} level {k}: rel = {r:.3e}")
            assert good.any() and r < 1e-12, (k, r)
    # a second launch without clearing doubles the sums: the kernel accumulates
    b1, c1 = bits.clone(), count.clone()
    ops.gauss_layer_bits(y_top, mu, sg, layer, n_levels, bits, count, y2=y_sub)
    torch.cuda.synchronize()
    assert torch.equal(count, 2 * c1)
    fin = torch.isfinite(b1)
    assert _rel(bits[fin], 2 * b1[fin]) < 1e-12 and torch.equal(torch.isfinite(bits), fin)


def test_gauss_layer_bits_outside_constant_and_refusals():
    c = ops.log2_lik_outside("cuda")
    z = ops.new_view(1, 1, 1, 4, zero=True)
    m = ops.new_view(1, 1, 1, 4, zero=True)
    ls = torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    ops.gauss_levels_eval(z, z, z, m, 1, log2sum=ls)                    # four masked-out elements
    assert abs(float(ls) - 4 * c) <= 1e-15 * abs(4 * c) and c < 0
    y = ops.new_view(1, 4, 4, 32, zero=True)
    layer = torch.zeros((1, 4, 4, 32), dtype=torch.uint8, device="cuda")
    bits = torch.zeros((1, 34), dtype=torch.float64, device="cuda")
    count = torch.zeros((1, 34), dtype=torch.int64, device="cuda")
    lib = L.load()
    call = lambda **kw: lib.vam_gauss_layer_bits(*[{**dict(y=y.ptr, ld_y=32, y2=None, ld_y2=0, mu=y.ptr, ld_mu=32, sg=y.ptr, ld_sg=32,
                                                           layer=layer.data_ptr(), ld_layer=32, nl=1, bits=bits.data_ptr(),
                                                           count=count.data_ptr(), ppi=16, n_pix=16, C=32, stream=ops.stream_ptr()), **kw}[k]
                                                   for k in ("y", "ld_y", "y2", "ld_y2", "mu", "ld_mu", "sg", "ld_sg", "layer", "ld_layer",
                                                             "nl", "bits", "count", "ppi", "n_pix", "C", "stream")])
    assert call() == 0
    for bad in (dict(C=30), dict(nl=0), dict(nl=33), dict(ppi=0), dict(ppi=5), dict(y=None), dict(layer=None), dict(bits=None),
                dict(count=None), dict(ld_layer=30)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- curve against loop
@pytest.mark.parametrize("B,H,W", [(2, 256, 256), (1, 512, 768)])
@pytest.mark.parametrize("use_graph", [False, True])
def test_rate_curve_equals_loop(B, H, W, use_graph):
    net = _net() if use_graph else _eager()
    assert net.use_graph == use_graph
    x = _x(B, H, W)
    first = _check_curve(net, x, QS15, f"{B}x{H}x{W} graph={use_graph}")
    again = _check_curve(net, x, QS15, "replay")                         # twice in a row: replay
    assert _rel(again["log2_likelihood_sum"], first["log2_likelihood_sum"]) < 1e-12
    _check_curve(net, x, [9.0, 0.3, 0.3, 0, 7.7, 10, 12, 0.001], "another list on the same plan")
    _check_curve(net, _x(B, H, W, seed=8), QS15, "another input")


def test_rate_curve_groups_70_unsorted_qualities():
    net = _net()
    g = torch.Generator().manual_seed(5)
    qs = (torch.rand(66, generator=g) * 10).tolist() + [0, 10, 0, 2.5]
    assert len(qs) == 70
    x = _x(1, 128, 192)
    got = _check_curve(net, x, qs, "70 qualities")
    order = sorted(range(70), key=lambda k: qs[k])
    bpp = got["bpp"][order, 0]
    assert (bpp[1:] >= bpp[:-1] * (1 - 1e-12)).all()                     # the rate is non-decreasing in q
    sw = net._sweep_plan(x)
    assert sorted(sw.rate_tails) == [4, 32]                              # 68 distinct positive qualities: 32 + 32 + 4
    _check_curve(net, x, [2.5, 1.0, 0, 7.0], "two-levels", mask_pol="two-levels")


def test_rate_curve_splits_sub_batches(monkeypatch):
    net = _net()
    monkeypatch.setattr(M, "MAX_PLAN_PIXELS", 2 * 128 * 128)             # two images of 128x128 per plan
    x = _x(5, 128, 128)
    _check_curve(net, x, [0, 0.5, 5, 10], "sub-batches 2 + 2 + 1")


# ----------------------------------------------------------------------------------------------- no transform work per level
def _conv_launches(fn):
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        p = ops.prof_read()
    finally:
        ops.prof_enable(False)
    return {k: v["launches"] for k, v in p.items()}


def test_rate_calls_run_one_front_end_and_no_other_transform(monkeypatch):
    net = _eager()                                                       # the event profiler brackets eager launches
    x = _x(2, 128, 128)
    sw = net._sweep_plan(x)
    front = _conv_launches(lambda: sw.front(x, False))
    assert front["conv_igemm"] > 50 and front["win_attn"] > 0
    g = torch.Generator().manual_seed(6)
    qs = (torch.rand(62, generator=g) * 10).tolist() + [0, 10]
    curve = _conv_launches(lambda: net.rate_curve(x, qs))
    assert curve["conv_igemm"] == front["conv_igemm"] and curve["win_attn"] == front["win_attn"], (curve, front)
    assert curve["variance_mask"] == 2                                   # 63 distinct positive qualities: two layer launches
    base = net.rate_curve(x, [0, 10])["bpp"].cpu()
    tg = base[0] + torch.tensor([[0.3], [0.7]]) * (base[1] - base[0])
    solve = _conv_launches(lambda: net.qualities_for_bpp(x, tg))
    assert solve["conv_igemm"] == front["conv_igemm"] and solve["win_attn"] == front["win_attn"], (solve, front)
    monkeypatch.setattr(M, "MAX_PLAN_PIXELS", 128 * 128)                 # one image per plan: one front end per sub-batch
    solve2 = _conv_launches(lambda: net.qualities_for_bpp(x, tg))
    assert solve2["conv_igemm"] == 2 * _conv_launches(lambda: net._sweep_plan(x[:1]).front(x[:1], False))["conv_igemm"]


# ----------------------------------------------------------------------------------------------- solver contract
def _bpp_at(ref, xb, q):
    with torch.no_grad():
        out = ref.forward_single_quality(xb, float(q), training=False)
    return float(-out["log2_likelihood_sum"].sum() / (xb.shape[2] * xb.shape[3]))


def _check_contract(ref, x, sol, tg, q_tol):
    """The solver's contract in forward_single_quality's own rates (on ``ref``, an eager model: every probe is a new quality)."""
    net = ref
    T, B = tg.shape
    for t in range(T):
        for b in range(B):
            q, tt, ok = float(sol["quality"][t, b]), float(tg[t, b]), bool(sol["reached"][t, b])
            xb = x[b:b + 1]
            at = _bpp_at(net, xb, q)
            print(f"solver t={tt:.6f} image {b}: q* = {q:.6f}, bpp(q*) = {at:.6f}, reached = {ok}")
            if not ok:
                assert q == 0.0 and at > tt
                continue
            assert at <= tt * (1 + 1e-12), (t, b, q, at, tt)
            assert abs(float(sol["bpp"][t, b]) - at) <= 1e-12 * at
            if q < 10.0:
                above = _bpp_at(net, xb, min(10.0, q + 1.001 * q_tol))
                assert above > tt * (1 - 1e-12), (t, b, q, above, tt)


@pytest.mark.parametrize("use_graph", [True, False])
def test_qualities_for_bpp_contract(use_graph):
    net, ref = (_net() if use_graph else _eager()), _eager()
    assert net.use_graph == use_graph
    x = torch.cat([_x(1, 128, 128, seed=3), _x(1, 128, 128, seed=4) * 0.5, _x(1, 128, 128, seed=5).flip(3)])
    B = x.shape[0]
    lo = torch.tensor([_bpp_at(ref, x[b:b + 1], 0) for b in range(B)], dtype=torch.float64)
    hi = torch.tensor([_bpp_at(ref, x[b:b + 1], 10) for b in range(B)], dtype=torch.float64)
    assert (hi > lo).all()
    tg = torch.stack([lo + f * (hi - lo) for f in (0.1, 0.5, 0.9)])      # per-image budgets inside each image's reachable range
    sol = net.qualities_for_bpp(x, tg)
    for k in ("quality", "bpp", "reached"):
        assert tuple(sol[k].shape) == (3, B)
    assert sol["quality"].dtype == sol["bpp"].dtype == torch.float64 and sol["reached"].dtype == torch.bool
    assert sol["reached"].all() and (sol["quality"] > 0).all() and (sol["quality"] < 10).all()
    _check_contract(ref, x, sol, tg, 1e-3)
    # a coarser tolerance takes fewer passes and keeps the contract
    sol2 = net.qualities_for_bpp(x, tg[1:2], q_tol=0.05)
    _check_contract(ref, x, sol2, tg[1:2], 0.05)
    # one scalar target for the batch; under every base rate; above every full rate
    mid = float(tg[1].mean())
    s1 = net.qualities_for_bpp(x, mid)
    assert tuple(s1["quality"].shape) == (1, B)
    _check_contract(ref, x, s1, torch.full((1, B), mid, dtype=torch.float64), 1e-3)
    s2 = net.qualities_for_bpp(x, [float(lo.min()) * 0.5, float(hi.max()) * 2])
    assert not s2["reached"][0].any() and (s2["quality"][0] == 0).all()
    assert s2["reached"][1].all() and (s2["quality"][1] == 10).all()
    _check_contract(ref, x, s2, torch.tensor([[float(lo.min()) * 0.5] * B, [float(hi.max()) * 2] * B], dtype=torch.float64), 1e-3)
    with pytest.raises(ValueError):
        net.qualities_for_bpp(x, tg[:, :2])


# ----------------------------------------------------------------------------------------------- drivers
def test_rd_at_rates_equals_rd_sweep_at_the_resolved_qualities():
    net = _net()
    x = torch.cat([_x(1, 128, 128, seed=3), _x(1, 128, 128, seed=4) * 0.5])
    base = EV.rate_curve(net, x, [0, 10])
    assert _rel(base, net.rate_curve(x, [0, 10])["bpp"].cpu()) < 1e-12         # (two runs differ in their float64 summation order)
    tg = torch.stack([base[0] + f * (base[1] - base[0]) for f in (0.25, 0.75)])
    bpp, psnr, q, ok = EV.rd_at_rates(net, x, tg)
    assert tuple(bpp.shape) == tuple(psnr.shape) == tuple(q.shape) == (2, 2) and ok.all()
    assert (bpp <= tg * (1 + 1e-12)).all()
    for b in range(2):
        r, p_ = EV.rd_sweep(net, x[b:b + 1], q[:, b].tolist())
        assert _rel(r[:, 0], bpp[:, b]) < 1e-12 and _rel(p_[:, 0], psnr[:, b]) < 1e-12


def test_q_list_for_bpps_feeds_the_container():
    if "coder" not in _NETS:                                             # update() drops plans: a model of its own, updated once
        _NETS["coder"] = copy.deepcopy(_net())
        _NETS["coder"].update()
    net = _NETS["coder"]
    x = _x(1, 128, 192)
    base = EV.rate_curve(net, x, [0, 10])[:, 0]
    tg = [float(base[0]) * 0.5] + [float(base[0] + f * (base[1] - base[0])) for f in (0.6, 0.2, 0.2)]     # one unreachable, one repeated
    qs = PR.q_list_for_bpps(net, x, tg)
    assert len(qs) == 2 and qs == sorted(qs) and 0 < qs[0] < qs[1] < 10
    containers, bits = PR.encode_batch(net, x, qs)
    dec = PR.ProgressiveDecoder(net, containers)
    with torch.no_grad():
        for k, q in enumerate(qs, start=1):
            out = dec.decode(k)
            ref = _eager().forward_single_quality(x, q, training=False)
            assert torch.equal(out["x_hat"], ref["x_hat"]) and torch.equal(out["y_hat"], ref["y_hat"]), (k, q)
    with pytest.raises(ValueError):
        PR.q_list_for_bpps(net, torch.cat([x, x]), tg)
    with pytest.raises(ValueError):
        PR.q_list_for_bpps(net, x, [float(base[0]) * 0.5])


# ----------------------------------------------------------------------------------------------- fallbacks and refusals
def test_loop_fallbacks_keep_the_layout_and_the_contract():
    x = _x(2, 64, 64)
    qs = [5, 0, 0.5, 10]
    n1 = _eager(all_scalable=False)
    assert not n1._sweep_eligible()
    _check_curve(n1, x, qs, "all_scalable=False", ref=n1)
    lo, hi = (n1.rate_curve(x, [q])["bpp"][0].cpu() for q in (0, 10))
    tg = (lo + 0.5 * (hi - lo)).unsqueeze(0)
    sol = n1.qualities_for_bpp(x, tg, q_tol=0.05)
    assert tuple(sol["quality"].shape) == (1, 2) and sol["reached"].all()
    _check_contract(n1, x, sol, tg, 0.05)
    if "bf16" not in _NETS:
        _NETS["bf16"] = copy.deepcopy(_eager())
        _NETS["bf16"].storage = "bf16"
    n2 = _NETS["bf16"]
    assert not n2._sweep_eligible()
    _check_curve(n2, x, qs, "bf16 storage", ref=n2)


def test_refusals():
    x = _x(1, 64, 64)
    rem = _net("rem")
    with pytest.raises(NotImplementedError, match="checkpoint"):
        rem.rate_curve(x, [1.0])
    with pytest.raises(NotImplementedError, match="checkpoint"):
        rem.qualities_for_bpp(x, [1.0])
    net = _net()
    with pytest.raises(ValueError, match="two values"):
        net.qualities_for_bpp(x, [1.0], mask_pol="two-levels")
    with pytest.raises(ValueError):
        net.qualities_for_bpp(x, [1.0], q_tol=0)
