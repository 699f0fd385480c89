"""Coded-size control on the GPU: vam_coded_layer_bits / vam_coded_symbol_bits against the host pricing
of bitstream.py, vam_variance_layers_per_image against one vam_variance_layers per image, coded_size_curve and
container_sizes against the real compress / encode_batch, the byte-budget solvers' contracts, launch accounting, and the
configurations that loop or refuse."""
import argparse
import copy
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                              # noqa: E402
import vampic.synth as synth               # noqa: E402
from vampic import _lib as L, bitstream as bs, evaluate as EV, ops, progressive as PR     # noqa: E402

M = sys.modules["vampic.models"]
README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
QS5 = [0, 0.05, 0.5, 2.5, 10]
DEMO_Q = [0.01, 0.05, 0.1, 0.25, 0.5, 0.6, 0.7, 0.8, 0.9, 1, 2, 3, 4, 4.5, 10]
_NETS = {}
_ACTUAL = {}


def _net(kind="pic", updated=True, **over):
    """Models live for the session and never drop a plan (tests/test_gpu_runtime.py counts on room below the retirement cap)."""
    key = (kind, updated) + tuple(sorted(over.items()))
    if key not in _NETS:
        a = dict(README_ARGS, **over)
        if kind == "rem":
            a.update(check_levels=[0.01, 0.25, 1.75], mu_std=True, dimension="big")
        net = vampic.get_model(argparse.Namespace(model=kind, **a), "cpu").eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
        net = net.cuda()
        if updated:
            net.update()
        _NETS[key] = net
    return _NETS[key]


def _eager(kind="pic", **over):
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


def _close(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    rel = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    print(f"{what}: rel = {rel:.3e}")
    assert rel <= 1e-12, (what, rel)


def _actual(xb, q, tag):
    """(bytes, table cost) of the real compress of ONE image on the eager twin, the cost priced on the host from that plan's
    own symbol and index buffers; kept per (tag, q)."""
    key = (tag, float(q))
    if key not in _ACTUAL:
        ref = _eager()
        with torch.no_grad():
            out = ref.compress(xb, q)
        nbytes = sum(len(s) for part in out["strings"][0] for s in part) + sum(len(s) for s in out["strings"][1])
        plan = ref._plan(xb, base_only=q <= 0, symbols=True)
        tg, te = bs.Tables.of(ref.gaussian_conditional), bs.Tables.of(ref.entropy_bottleneck)
        bits = bs.price(plan.sym.buf.cpu().numpy(), plan.idx.buf.cpu().numpy(), tg).sum() + \
            bs.price(plan.z_sym.buf.cpu().numpy(), np.arange(ref.N)[None, None, None, :], te).sum()
        n_streams = len(out["strings"][1]) + sum(len(part) for part in out["strings"][0])
        _ACTUAL[key] = (nbytes, float(bits), n_streams)
    return _ACTUAL[key]


# ----------------------------------------------------------------------------------------------- pricing kernel
def _crafted(B, h, w, d):
    y = synth.normal((B, 2 * d, h, w), 40) * 4
    musg = synth.normal((B, 3 * d, h, w), 41) * 2                       # mu and sigma: windows of one wider tensor
    musg[:, 2 * d:] = musg[:, 2 * d:].abs() * 1.5
    musg[0, 2 * d:2 * d + 5] = 0.05                                      # below the 0.11 bound
    musg[1, 2 * d + 40:2 * d + 44] = 1000.0                              # above the largest table entry
    y[0, d:d + 5, 0, :] += 300.0                                         # far outside the narrowest tables: bypass, both signs
    y[0, d:d + 5, 1, :] -= 300.0
    y[1, d + 70, 2, :] = 3.0e6
    y[1, d + 70, 3, :] = -3.0e6
    return y, musg


def _host_pairs(y, musg, d, with_y2, table):
    """The (symbol, index) pairs in numpy float32: round-half-even of (y - y2) - mu, and build_indexes' count."""
    yt, mu, sg = y[:, d:].numpy(), musg[:, :d].numpy(), musg[:, 2 * d:].numpy()
    r = (yt - y[:, :d].numpy()).astype(np.float32) if with_y2 else yt
    sym = np.rint((r - mu).astype(np.float32)).astype(np.int64)
    v = np.maximum(sg, np.float32(0.11))
    tb = table.cpu().numpy().astype(np.float32)
    idx = tb.size - 1 - (v[..., None] <= tb[:-1]).sum(-1)
    return sym, idx                                                      # NCHW


def _host_bins(pr, lay, n_levels, cps):
    """[B, C // cps, n_levels + 1] sums and counts of the NCHW prices ``pr`` by (image, slice, layer id)."""
    B, C = pr.shape[:2]
    bits, count = np.zeros((B, C // cps, n_levels + 1)), np.zeros((B, C // cps, n_levels + 1), dtype=np.int64)
    slot = np.where(lay < n_levels, lay, n_levels)
    for b in range(B):
        for j in range(C // cps):
            p_, s_ = pr[b, j * cps:(j + 1) * cps].ravel(), slot[b, j * cps:(j + 1) * cps].ravel()
            bits[b, j] = np.bincount(s_, weights=p_, minlength=n_levels + 1)
            count[b, j] = np.bincount(s_, minlength=n_levels + 1)
    return bits, count


@pytest.mark.parametrize("n_levels", [1, 5, 32])
@pytest.mark.parametrize("with_y2", [True, False])
@pytest.mark.parametrize("with_layer", [True, False])
def test_coded_layer_bits_equals_host_pricing(n_levels, with_y2, with_layer):
    net = _net()
    B, h, w, d = 2, 8, 12, 128
    ns = d // 32
    y, musg = _crafted(B, h, w, d)
    y_v, ms_v = _v(y), _v(musg)
    y_top, y_sub = y_v.window(d, d), (y_v.window(0, d) if with_y2 else None)
    mu, sg = ms_v.window(0, d), ms_v.window(2 * d, d)                   # pixel stride 3d != C
    qs32 = sorted([0.0, 0.0, 0.003, 0.05, 0.1, 0.25, 0.5, 0.5, 0.75, 1, 1.25, 1.5, 2, 2.5, 2.5, 3, 3.5, 4, 4.5, 5, 5.5, 6, 6.5, 7,
                   7.5, 8, 8.5, 9, 9.5, 9.9, 9.95, 9.99])
    prs = {1: [2.5], 5: [0.0, 0.5, 0.5, 5.0, 9.99], 32: qs32}[n_levels]
    layer = None
    if with_layer:
        layer = torch.empty((B, h, w, d), dtype=torch.uint8, device="cuda")
        ops.variance_layers(sg, prs, layer, n_slice=ns)
    tg = bs.DeviceTables.of(net.gaussian_conditional, "cuda")
    table = net.gaussian_conditional.scale_table.float().contiguous()
    nb = n_levels + 1
    bits = torch.zeros((B, ns, nb), dtype=torch.float64, device="cuda")
    count = torch.zeros((B, ns, nb), dtype=torch.int64, device="cuda")
    ops.coded_layer_bits(y_top, mu, sg, layer, n_levels, table, tg, 32, bits, count, y2=y_sub)
    torch.cuda.synchronize()
    # the host pricing of the same tensors
    sym, idx = _host_pairs(y, musg, d, with_y2, table)
    t = tg.host
    v = sym - t.offsets[idx]
    outside = (v < 0) | (v >= t.sizes[idx] - 2)
    assert (outside & (v < 0)).any() and (outside & (v > 0)).any()      # bypass symbols of both signs
    assert (idx == 0).any() and (idx == table.numel() - 1).any()        # sigma under 0.11 and above the table
    lay = layer.permute(0, 3, 1, 2).cpu().numpy().astype(np.int64) if with_layer else np.zeros(sym.shape, dtype=np.int64)
    hb, hc = _host_bins(bs.price(sym, idx, t), lay, n_levels, 32)
    assert np.array_equal(count.cpu().numpy(), hc)
    assert with_layer or int(count[..., 1:].sum()) == 0
    for b in range(B):
        for j in range(ns):
            _close(bits[b, j].cpu().numpy(), hb[b, j], f"levels={n_levels} y2={with_y2} layer={with_layer} stream ({b}, {j})")
    # the priced pairs are the coder's: the symbols of vam_gauss_tail and the indexes of vam_build_indexes, priced on the host
    sym_d = ops.new_iview(B, h, w, d)
    ops.gauss_tail(y_top, mu, sg, y2=y_sub, sym=sym_d)
    idx_d = ops.new_iview(B, h, w, d)
    ops.build_indexes(sg, table, out=idx_d)
    nchw = lambda iv: iv.buf.permute(0, 3, 1, 2).cpu().numpy().astype(np.int64)
    assert np.array_equal(nchw(sym_d), sym) and np.array_equal(nchw(idx_d), idx)
    hb2, _ = _host_bins(bs.price(nchw(sym_d), nchw(idx_d), t), lay, n_levels, 32)
    _close(bits.cpu().numpy(), hb2, "against the coder's own pairs")
    # the symbol-input form prices the same pairs; a second launch without clearing doubles the bins
    bits2, count2 = torch.zeros_like(bits), torch.zeros_like(count)
    ops.coded_symbol_bits(sym_d, idx_d, layer, n_levels, tg, 32, bits2, count2)
    assert torch.equal(count2, count)
    _close(bits2.cpu().numpy(), hb, "symbol-input form")
    ops.coded_layer_bits(y_top, mu, sg, layer, n_levels, table, tg, 32, bits, count, y2=y_sub)
    assert torch.equal(count, 2 * count2)
    _close(bits.cpu().numpy(), 2 * hb, "second launch accumulates")


def test_coded_symbol_bits_per_channel_tables():
    net = _net()
    te = bs.DeviceTables.of(net.entropy_bottleneck, "cuda")
    B, h, w, N = 3, 4, 6, net.N
    g = torch.Generator().manual_seed(11)
    sym = torch.round(torch.randn((B, h, w, N), generator=g) * 6).int()
    sym[0, 0, 0, :7] = torch.tensor([2 ** 31 - 1, -2 ** 31 + 1, 4000, -4000, 70000, -70000, 0], dtype=torch.int32)
    iv = ops.IView(sym.cuda().contiguous(), 0, N)
    bits = torch.zeros((B, 1, 2), dtype=torch.float64, device="cuda")
    count = torch.zeros((B, 1, 2), dtype=torch.int64, device="cuda")
    ops.coded_symbol_bits(iv, None, None, 1, te, N, bits, count)
    pr = bs.price(sym.numpy(), np.arange(N)[None, None, None, :], te.host)
    assert count[:, 0, 0].tolist() == [h * w * N] * B and int(count[:, 0, 1].sum()) == 0
    _close(bits[:, 0, 0].cpu().numpy(), pr.reshape(B, -1).sum(1), "z symbols, index = channel")
    # two streams of N / 2 channels: the second one's tables start at channel N / 2
    bits2 = torch.zeros((B, 2, 2), dtype=torch.float64, device="cuda")
    count2 = torch.zeros((B, 2, 2), dtype=torch.int64, device="cuda")
    ops.coded_symbol_bits(iv, None, None, 1, te, N // 2, bits2, count2)
    _close(bits2[:, :, 0].cpu().numpy(), pr.reshape(B, h * w, 2, N // 2).sum((1, 3)), "two streams per image")


def test_coded_bits_refusals():
    net = _net()
    tg = bs.DeviceTables.of(net.gaussian_conditional, "cuda")
    te = bs.DeviceTables.of(net.entropy_bottleneck, "cuda")
    table = net.gaussian_conditional.scale_table.float().contiguous()
    v = ops.new_view(1, 4, 4, 64, zero=True)
    iv = ops.IView(torch.zeros((1, 4, 4, 64), dtype=torch.int32, device="cuda"), 0, 64)
    lib, sp = L.load(), ops.stream_ptr()
    buf = torch.zeros(2 * 40, dtype=torch.float64, device="cuda")
    b_, c_ = buf.data_ptr(), buf.data_ptr() + 8 * 40
    tgs, tes = ops.C.byref(tg.struct), ops.C.byref(te.struct)

    def layer_call(n_levels=1, cps=32, n_table=table.numel(), tables=tgs, bits=b_, y=v.ptr, scale=table.data_ptr()):
        return lib.vam_coded_layer_bits(y, v.ld, None, 0, v.ptr, v.ld, v.ptr, v.ld, None, 0, n_levels, scale, n_table, tables, cps,
                                        bits, c_, 16, 16, 64, sp)
    assert layer_call() == 0
    for kw in (dict(n_levels=0), dict(n_levels=33), dict(cps=24), dict(cps=48), dict(cps=0), dict(n_table=1),
               dict(n_table=tg.struct.n_cdfs + 1), dict(tables=None), dict(bits=None), dict(y=None), dict(scale=None)):
        assert layer_call(**kw) != 0, kw
    with pytest.raises(L.VamError):
        L.check(layer_call(n_levels=33), "vam_coded_layer_bits")

    def sym_call(n_levels=1, cps=32, idx=iv.ptr, base=0, tables=tgs, sym=iv.ptr, C_=64):
        return lib.vam_coded_symbol_bits(sym, iv.ld, idx, iv.ld, base, None, 0, n_levels, tables, cps, b_, c_, 16, 16, C_, sp)
    assert sym_call() == 0 and sym_call(idx=None, tables=tes) == 0
    for kw in (dict(n_levels=0), dict(n_levels=33), dict(cps=20), dict(sym=None), dict(tables=None), dict(C_=62),
               dict(idx=None, tables=tes, base=te.struct.n_cdfs - 63), dict(idx=None, tables=tes, base=-1)):
        assert sym_call(**kw) != 0, kw
    torch.cuda.synchronize()
    # an index outside the tables prices as NaN instead of reading past them
    iv.buf[0, 0, 0, 0] = 10 ** 6
    bits = torch.zeros((1, 2, 2), dtype=torch.float64, device="cuda")
    count = torch.zeros((1, 2, 2), dtype=torch.int64, device="cuda")
    ops.coded_symbol_bits(iv, iv, None, 1, tg, 32, bits, count)
    assert bool(torch.isnan(bits[0, 0, 0])) and not bool(torch.isnan(bits[0, 1, 0]))


# ----------------------------------------------------------------------------------------------- per-image layers
@pytest.mark.parametrize("hw", [(8, 12), (32, 48), (64, 48)])            # 4, 16 and 0 float4 per thread in registers
def test_variance_layers_per_image_equals_one_launch_per_image(hw):
    h, w = hw
    B, d, ns = 4, 64, 2
    sg = synth.normal((B, d, h, w), 50).abs()
    sg[1, :3] = 0.25                                                     # ties
    sg_v = _v(sg)
    qs32 = sorted(np.random.default_rng(1).uniform(0, 10, 30).tolist() + [0.0, 10.0])
    lists = [[0.0, 0.5, 0.5, 2.5, 10.0, 12.0], [3.3], qs32, [0.0]]
    width = max(len(r) for r in lists)
    layer = torch.full((B, h, w, d), 7, dtype=torch.uint8, device="cuda")
    thr = torch.full((width, B * ns), -7.0, dtype=torch.float32, device="cuda")
    ops.variance_layers_per_image(sg_v, lists, layer, n_slice=ns, thr=thr)
    for b, prs in enumerate(lists):
        one = ops.View(sg_v.buf[b:b + 1], sg_v.c0, sg_v.C)
        want = torch.empty((1, h, w, d), dtype=torch.uint8, device="cuda")
        wthr = torch.empty((len(prs), ns), dtype=torch.float32, device="cuda")
        ops.variance_layers(one, prs, want, n_slice=ns, thr=wthr)
        assert torch.equal(layer[b:b + 1], want), (hw, b)
        got = thr[:len(prs), b * ns:(b + 1) * ns]
        assert torch.equal(got.view(torch.int32), wthr.view(torch.int32)), (hw, b)
        assert bool((thr[len(prs):, b * ns:(b + 1) * ns] == -7.0).all())   # rows beyond the image's list are left alone
    with pytest.raises(L.VamError):
        ops.variance_layers_per_image(sg_v, [[1.0], [2.0, 1.0], [1.0], [1.0]], layer, n_slice=ns)
    with pytest.raises(L.VamError):
        ops.variance_layers_per_image(sg_v, [[1.0], [], [1.0], [1.0]], layer, n_slice=ns)
    with pytest.raises(L.VamError):
        ops.variance_layers_per_image(sg_v, [[1.0], [1.0] * 33, [1.0], [1.0]], layer, n_slice=ns)


# ----------------------------------------------------------------------------------------------- coded_size_curve
def _check_sizes(got, x, qs, tag):
    B = x.shape[0]
    lo, hi, bits = got["bytes_lo"], got["bytes_hi"], got["bits"]
    assert lo.dtype == hi.dtype == torch.int64 and bits.dtype == torch.float64
    assert tuple(lo.shape) == tuple(hi.shape) == tuple(bits.shape) == (len(qs), B)
    for k, q in enumerate(qs):
        for b in range(B):
            nbytes, cost, n_streams = _actual(x[b:b + 1], q, (tag, b))
            print(f"{tag} image {b} q={q}: [{int(lo[k, b])}, {int(hi[k, b])}] actual {nbytes}, {n_streams} streams")
            assert int(lo[k, b]) <= nbytes <= int(hi[k, b]), (tag, b, q, int(lo[k, b]), nbytes, int(hi[k, b]))
            assert int(hi[k, b]) - int(lo[k, b]) <= 4 * n_streams
            assert abs(float(bits[k, b]) - cost) <= 1e-12 * cost, (tag, b, q, float(bits[k, b]), cost)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("shape", [(2, 256, 256), (1, 512, 768)])
def test_coded_size_curve_brackets_the_real_compress(shape, use_graph):
    net = _net() if use_graph else _eager()
    assert net.use_graph == use_graph
    x = _x(*shape)
    tag = "x".join(map(str, shape))
    got = net.coded_size_curve(x, QS5)
    _check_sizes(got, x, QS5, tag)
    # grouping: 70 entries, unsorted, with repeats (68 distinct positive qualities: 32 + 32 + 4)
    g = torch.Generator().manual_seed(9)
    many = (torch.rand(64, generator=g) * 10).tolist() + [2.5, 0.0, 10.0, 0.5, 0.05, 2.5]
    big = net.coded_size_curve(x, many)
    assert tuple(big["bytes_hi"].shape) == (70, shape[0])
    for k, q in enumerate(many):
        if q in QS5:
            for key in ("bytes_lo", "bytes_hi"):
                assert torch.equal(big[key][k], got[key][QS5.index(q)]), (q, key)
            _close(big["bits"][k].numpy(), got["bits"][QS5.index(q)].numpy(), f"70-entry list, q={q}")
    assert bool((big["bytes_lo"] <= big["bytes_hi"]).all())
    assert {4, 32} <= set(net._sweep_plan(x).size_tail.tails)             # one plan per group size; 4: also QS5's positive ones


# ----------------------------------------------------------------------------------------------- container_sizes
@pytest.mark.parametrize("shape,q_list", [((2, 256, 256), PR.Q_LIST), ((1, 512, 768), DEMO_Q)])
def test_container_sizes_bracket_encode_batch(shape, q_list):
    net = _net()
    x = _x(*shape)
    sizes = PR.container_sizes(net, x, q_list)
    cs, _ = PR.encode_batch(net, x, q_list)
    assert len(sizes) == len(cs) == shape[0]
    ns = net.ns0
    for b, (s, c) in enumerate(zip(sizes, cs)):
        groups = [("z", s["z"], sum(len(v) for v in c["z"]), 1), ("base", s["base"], sum(len(v[0]) for v in c["base"]), ns)]
        groups += [(f"layer {k}", s["progressive"][k], sum(len(v) for v in c["progressive"][k]), ns) for k in range(len(q_list))]
        for name, (lo, hi), actual, n_streams in groups:
            print(f"{shape} image {b} {name}: [{lo}, {hi}] actual {actual}")
            assert lo <= actual <= hi and hi - lo <= 4 * n_streams, (b, name, lo, actual, hi)


# ----------------------------------------------------------------------------------------------- solvers
@pytest.mark.parametrize("use_graph", [True, False])
def test_qualities_for_bytes_contract(use_graph):
    net = _net() if use_graph else _eager()
    x = _x(2, 256, 256)
    q_tol = 1e-3
    ends = net.coded_size_curve(x, [0, 10])["bytes_hi"].double()
    tg = torch.cat([ends[0] + torch.tensor([[0.2], [0.4], [0.6], [0.8]], dtype=torch.float64) * (ends[1] - ends[0]),
                    (ends[0] - 100.0)[None]])
    sol = net.qualities_for_bytes(x, tg, q_tol=q_tol)
    assert tuple(sol["quality"].shape) == tuple(sol["bytes"].shape) == tuple(sol["reached"].shape) == (5, 2)
    for t in range(5):
        for b in range(2):
            q, tt, ok = float(sol["quality"][t, b]), float(tg[t, b]), bool(sol["reached"][t, b])
            if t == 4:
                assert not ok and q == 0.0
                continue
            assert ok
            nbytes = _actual(x[b:b + 1], q, ("solve", b))[0]
            at = net.coded_size_curve(x, [q, min(10.0, q + q_tol)])["bytes_hi"][:, b]
            print(f"target {tt:.0f} image {b}: q* = {q:.6f}, actual {nbytes}, bytes_hi {int(at[0])}, at q* + q_tol {int(at[1])}")
            assert nbytes <= tt, (t, b, q, nbytes, tt)
            assert float(sol["bytes"][t, b]) == float(at[0]) <= tt
            assert q == 10.0 or float(at[1]) > tt, (t, b, q, float(at[1]), tt)
    # the maximality clause assumes a bytes_hi that does not decrease in q: it does not on these images
    grid = [10.0 * (k + 1) / 32 for k in range(32)]
    hi = net.coded_size_curve(x, grid)["bytes_hi"]
    assert bool((hi.diff(dim=0) >= 0).all())
    by, psnr, q, reached = EV.rd_at_sizes(net, x[:1], tg[:2, :1])
    assert torch.equal(q, sol["quality"][:2, :1]) and bool(reached.all()) and bool(torch.isfinite(psnr).all())
    assert torch.equal(by, sol["bytes"][:2, :1])


def test_q_list_for_bytes_levels_fit_their_budgets():
    net = _net()
    x = _x(2, 256, 256)[:1]
    full = PR.container_sizes(net, x, [10.0])[0]
    base = full["z"][1] + full["base"][1]
    top = base + full["progressive"][0][1]
    targets = [base - 50.0] + [base + f * (top - base) for f in (0.2, 0.4, 0.6, 0.8)]
    qs, kept = PR.q_list_for_bytes(net, x, targets, return_targets=True)
    assert PR.check_q_list(qs) == qs and kept == targets[1:] and PR.q_list_for_bytes(net, x, targets) == qs
    cs, _ = PR.encode_batch(net, x, qs)
    for k, t in enumerate(kept, 1):
        got = PR.bits_up_to(cs[0], k) / 8
        print(f"level {k}: q = {qs[k - 1]:.5f}, {got:.0f} bytes of {t:.0f}")
        assert got <= t, (k, qs, got, t)
    assert qs[0] > 0 and qs == sorted(qs)
    with pytest.raises(ValueError):
        PR.q_list_for_bytes(net, x, [base - 50.0])


# ----------------------------------------------------------------------------------------------- launch accounting
def _launches(fn):
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        p = ops.prof_read()
    finally:
        ops.prof_enable(False)
    return {k: v["launches"] for k, v in p.items()}


def test_size_calls_run_one_front_end_and_one_layer_launch_per_pass(monkeypatch):
    net = _eager()                                                       # the event profiler brackets eager launches
    x = _x(2, 128, 128)
    sw = net._sweep_plan(x)
    front = _launches(lambda: sw.front(x, False))
    assert front["conv_igemm"] > 50 and front["win_attn"] > 0
    g = torch.Generator().manual_seed(6)
    qs = (torch.rand(62, generator=g) * 10).tolist() + [0, 10]
    curve = _launches(lambda: net.coded_size_curve(x, qs))
    assert curve["conv_igemm"] == front["conv_igemm"] and curve["win_attn"] == front["win_attn"], (curve, front)
    assert curve["variance_mask"] == 2                                   # 63 distinct positive qualities: two layer launches
    assert curve["gauss_tail"] == front["gauss_tail"] + 2 + 2            # z and base once, one pricing launch per group
    ends = net.coded_size_curve(x, [0, 10])["bytes_hi"].double()
    tg = (ends[0] + 0.45 * (ends[1] - ends[0]))[None]
    solve = _launches(lambda: net.qualities_for_bytes(x, tg))
    assert solve["conv_igemm"] == front["conv_igemm"] and solve["win_attn"] == front["win_attn"], (solve, front)
    passes = M.rate_search_passes(1e-3)
    assert solve["variance_mask"] == passes                              # every pass: ONE layer launch for the sub-batch
    assert solve["gauss_tail"] == front["gauss_tail"] + 2 + passes
    monkeypatch.setattr(M, "MAX_PLAN_PIXELS", 128 * 128)                 # one image per plan: one front end per sub-batch
    solve2 = _launches(lambda: net.qualities_for_bytes(x, tg))
    assert solve2["conv_igemm"] == 2 * _launches(lambda: net._sweep_plan(x[:1]).front(x[:1], False))["conv_igemm"]


# ----------------------------------------------------------------------------------------------- fallbacks and refusals
def test_not_all_scalable_loops_over_the_real_compress():
    net = _net(all_scalable=False)
    assert not net._sweep_eligible()
    x = _x(1, 64, 64)
    qs = [0, 2.5, 2.5]
    got = net.coded_size_curve(x, qs)
    for k, q in enumerate(qs):
        with torch.no_grad():
            out = net.compress(x, q)
        nbytes = sum(len(s) for part in out["strings"][0] for s in part) + sum(len(s) for s in out["strings"][1])
        assert int(got["bytes_lo"][k, 0]) == int(got["bytes_hi"][k, 0]) == nbytes
        assert 8 * (nbytes - 8 * 21) - 1 <= float(got["bits"][k, 0]) <= 8 * nbytes     # len - S / 8 in (4, 8] per stream
    ends = got["bytes_hi"].double()
    t = float(ends[0, 0] + 0.5 * (ends[1, 0] - ends[0, 0]))
    sol = net.qualities_for_bytes(x, [t], q_tol=0.5)
    q = float(sol["quality"][0, 0])
    assert bool(sol["reached"][0, 0]) and 0 <= q <= 10 and float(sol["bytes"][0, 0]) <= t


def test_refusals():
    x = _x(1, 64, 64)
    rem = _net("rem")
    with pytest.raises(NotImplementedError):
        rem.coded_size_curve(x, [1.0])
    with pytest.raises(NotImplementedError):
        rem.qualities_for_bytes(x, [1e5])
    with pytest.raises(NotImplementedError):
        PR.container_sizes(rem, x, [1.0])
    net = _net()
    with pytest.raises(ValueError):
        net.qualities_for_bytes(x, [1e5], mask_pol="two-levels")
    with pytest.raises(ValueError):
        net.qualities_for_bytes(x, [1e5], q_tol=0.0)
    with pytest.raises(ValueError):
        net.qualities_for_bytes(x, torch.zeros(2, 3))
    with pytest.raises(ValueError):
        PR.container_sizes(net, x, [2.0, 1.0])
    with pytest.raises(ValueError):
        PR.q_list_for_bytes(net, _x(2, 64, 64), [1e5])
    two = net.coded_size_curve(x, [0, 1.0, 10.0], mask_pol="two-levels")     # every q != 0 is the full mask
    assert torch.equal(two["bytes_hi"][1], two["bytes_hi"][2]) and int(two["bytes_hi"][0, 0]) < int(two["bytes_hi"][1, 0])
    raw = _net(updated=False)
    for call in (lambda: raw.coded_size_curve(x, [1.0]), lambda: raw.qualities_for_bytes(x, [1e5]),
                 lambda: PR.container_sizes(raw, x, [1.0]), lambda: PR.q_list_for_bytes(raw, x, [1e5])):
        with pytest.raises(ValueError):
            call()
