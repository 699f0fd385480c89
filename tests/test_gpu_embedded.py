"""Embedded streams on the GPU (embedded.encode_batch / truncate / EmbeddedDecoder): the rank, gather
and scatter kernels against the numpy contracts of tests/test_embedded_cpu.py, prefix = mask, and on models the round trip,
arbitrary qualities, cuts at any byte, batch invariance, the sizes, graph replay and the refusals.  Every equality is
bit-exact."""
import argparse
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_embedded_cpu as EC                        # noqa: E402  (the numpy contracts)
import vampic                                         # noqa: E402
import vampic.synth as synth                          # noqa: E402
from vampic import _lib as L, bitstream as bs, embedded as EB, evaluate as EV, ops, progressive as P   # noqa: E402

README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
NS, C = 10, 32
_NETS, _SIGMAS, _CODED = {}, {}, {}


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


def _sigma(h, w, B=2, seed=0):
    """(NCHW host tensor, NHWC device view) of a progressive-sigma-like input of 10 slices x 32 channels: slice 3 constant
    (ties), slice 7 of image 0 holds a NaN, slice 9 many ties (the recipe of test_gpu_progressive_batch._sigma), and slice 5
    holds +inf, -0.0 and +0.0.  Computed once per shape and left unchanged."""
    if (h, w) not in _SIGMAS:
        g = torch.Generator().manual_seed(seed)
        s = torch.rand((B, 320, h, w), generator=g) * 4 + 0.05
        s[:, 3 * 32:4 * 32] = 1.25
        s[0, 7 * 32 + 5, 1, 2] = float("nan")
        s[:, 9 * 32:10 * 32] = torch.round(s[:, 9 * 32:10 * 32] * 2) / 2
        s[1, 5 * 32 + 2, 0, 1] = float("inf")
        s[:, 5 * 32 + 3, 0, :3] = -0.0
        s[:, 5 * 32 + 1, 2, 1:4] = 0.0
        s[0, 5 * 32 + 30, 3, 3] = -0.0
        _SIGMAS[(h, w)] = (s, ops.from_nchw(s.cuda()))
    return _SIGMAS[(h, w)]


def _segments(t):
    """[B, NS * C, h, w] -> [B, NS, n] in the canonical [C, h, w] order of a stream."""
    B = t.shape[0]
    return t.reshape(B, NS, -1)


def _rank(sg):
    perm = torch.full((sg.B, NS, C * sg.H * sg.W), -7, dtype=torch.int32, device="cuda")
    ops.variance_rank(sg, perm, n_slice=NS, workspace=ops.rank_workspace(sg, NS))
    return perm


def _contract_perm(s):
    seg = _segments(s).numpy()
    return np.stack([np.stack([EC.rank_order(seg[b, j]) for j in range(NS)]) for b in range(seg.shape[0])])


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("hw", [(4, 8), (8, 12), (16, 16), (32, 48), (64, 128)])
def test_rank_kernel_equals_the_numpy_contract(hw):
    """n = 1024, 3072 (no power of two, LDS), 8192 (the LDS limit), 49152 (workspace, padded), 2^18 (the limit)."""
    s, sg = _sigma(*hw)
    n = C * hw[0] * hw[1]
    ws = ops.rank_workspace(sg, NS)
    assert (ws is None) == (n <= 8192)
    perm = _rank(sg).cpu().numpy()
    want = _contract_perm(s)
    assert perm.shape == want.shape == (2, NS, n)
    assert np.array_equal(perm, want)


def test_rank_kernel_refuses_segments_above_the_limit():
    h, w = 64, 132                                        # n = 2^18 + 8192
    sg = ops.new_view(1, h, w, 320, "cuda", zero=True)
    perm = torch.full((1, NS, C * h * w), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(L.VamError, match="exceeds"):
        ops.variance_rank(sg, perm, n_slice=NS)
    torch.cuda.synchronize()
    assert (perm == -7).all()                             # nothing was launched
    with pytest.raises(ValueError, match="exceed"):
        ops.rank_workspace(sg, NS)
    assert L.load().vam_variance_rank_workspace(1, NS, h * w, C) == 0
    s, sg = _sigma(32, 48)                                # a segment that needs the workspace and gets none
    with pytest.raises(L.VamError, match="workspace"):
        ops.variance_rank(sg, torch.empty((2, NS, C * 32 * 48), dtype=torch.int32, device="cuda"), n_slice=NS)


@pytest.mark.parametrize("hw", [(16, 16), (32, 48)])
def test_prefix_of_the_rank_order_is_the_variance_mask(hw):
    s, sg = _sigma(*hw)
    h, w = hw
    n = C * h * w
    perm = _rank(sg)
    qs = [0.05, 0.5, 2.5, 7, 9.99, 10]
    layer = torch.empty((2, h, w, 320), dtype=torch.uint8, device="cuda")
    ops.variance_layers(sg, qs, layer, n_slice=NS)
    count = torch.empty((len(qs), 2, NS), dtype=torch.int32, device="cuda")
    ops.rank_counts(layer, perm, NS, len(qs), count)
    mask = ops.new_view(2, h, w, 320, "cuda")
    r = torch.arange(n, device="cuda")
    for k, q in enumerate(qs):
        ops.variance_mask(sg, q, mask, n_slice=NS)
        m = _segments(mask.buf.permute(0, 3, 1, 2).contiguous())                    # [B, NS, n], canonical order
        assert torch.equal(count[k].long(), m.sum(-1).long()), q
        ranked = torch.gather(m, 2, perm.long())                                    # the mask along the rank order
        assert torch.equal(ranked == 1, r[None, None, :] < count[k][..., None]), q  # perm[:count] is the mask's support
    assert (count[-1] == n).all() and (count[:-1, 0, 7] == 0).all()                 # q = 10 keeps all; a NaN segment nothing below


@pytest.mark.parametrize("hw", [(8, 12), (32, 48)])
def test_gather_then_scatter(hw):
    s, sg = _sigma(*hw)
    h, w = hw
    n = C * h * w
    perm = _rank(sg)
    g = torch.Generator().manual_seed(5)
    a_nchw = torch.randint(-40, 40, (2, 640, h, w), generator=g, dtype=torch.int32)
    b_nchw = torch.randint(0, 64, (2, 640, h, w), generator=g, dtype=torch.int32)
    nhwc = lambda t: ops.IView(t.permute(0, 2, 3, 1).contiguous().cuda(), 0, 640)
    a, b = nhwc(a_nchw), nhwc(b_nchw)
    out_a, out_b = torch.empty_like(perm), torch.empty_like(perm)
    ops.rank_gather(perm, NS, a.window(320, 320), out_a, b.window(320, 320), out_b)          # the progressive halves
    pl = perm.long().cpu()
    assert torch.equal(out_a.cpu(), torch.gather(_segments(a_nchw[:, 320:]), 2, pl))
    assert torch.equal(out_b.cpu(), torch.gather(_segments(b_nchw[:, 320:]), 2, pl))
    only = torch.empty_like(perm)
    ops.rank_gather(perm, NS, a.window(320, 320), only)                                      # one view alone
    assert torch.equal(only, out_a)
    # count = n restores the view, every element in level 0
    sym = ops.new_iview(2, h, w, 320, "cuda")
    ids = torch.empty((2, h, w, 320), dtype=torch.uint8, device="cuda")
    full = torch.full((1, 2, NS), n, dtype=torch.int32, device="cuda")
    ops.rank_scatter(out_a, perm, full, 1, NS, sym, ids)
    assert torch.equal(sym.buf, a.buf[..., 320:]) and (ids == 0).all()
    # three levels: ids by the numpy rule, symbols 0 beyond the last count
    rng = np.random.default_rng(1)
    table = np.sort(rng.integers(0, n + 1, (3, 2, NS)), axis=0).astype(np.int32)
    table[:, 0, 0] = [0, 0, 0]
    table[:, 1, 1] = [5, 5, n]
    ops.rank_scatter(out_a, perm, torch.from_numpy(table).cuda(), 3, NS, sym, ids)
    got_ids = torch.gather(_segments(ids.permute(0, 3, 1, 2).contiguous()), 2, perm.long()).cpu().numpy()    # along the rank order
    got_sym = torch.gather(_segments(sym.buf.permute(0, 3, 1, 2).contiguous()), 2, perm.long()).cpu().numpy()
    for bb in range(2):
        for j in range(NS):
            assert np.array_equal(got_ids[bb, j], EC.level_ids(table[:, bb, j], n)), (bb, j)
            keep = np.arange(n) < table[2, bb, j]
            assert np.array_equal(got_sym[bb, j], np.where(keep, out_a[bb, j].cpu().numpy(), 0)), (bb, j)


# ------------------------------------------------------------------------------------------------ models
QS = [0, 0.05, 0.5, 2.5, 3.3, 7, 10]


def _coded(B, H, W, seed):
    """(x, containers) of one input, encoded once per session."""
    key = (B, H, W, seed)
    if key not in _CODED:
        x = _x(B, H, W, seed=seed)
        _CODED[key] = (x, EB.encode_batch(_net(), x))
    return _CODED[key]


def _same(a, b):
    return torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"])


def _ranked_reference(net, x):
    """(symbols, indexes) [B, NS, n] in rank order, from the model's module-level surface and the numpy contract."""
    with torch.no_grad():
        fw10 = net.forward_single_quality(x, 10)
        sym10 = net.compress(x, quality=10, real_compress=False)["strings"][0]
        idx = net.gaussian_conditional.build_indexes(fw10["std"]).int().cpu()
    sym = torch.cat(sym10[net.ns0:], 1).int().cpu()
    pl = torch.from_numpy(_contract_perm(fw10["std"].cpu())).long()
    return torch.gather(_segments(sym), 2, pl).numpy(), torch.gather(_segments(idx), 2, pl).numpy()


@pytest.mark.parametrize("shape", [(2, 64, 128, 2), (1, 128, 192, 1)])
def test_round_trip_and_qualities(shape):
    net = _net()
    x, cs = _coded(*shape)
    assert len(cs) == shape[0]
    for c in cs:
        assert set(c) == {"format", "shape", "z", "base", "embedded", "marks"} and c["format"] == "embedded-1"
        assert len(c["embedded"]) == NS and c["marks"]["q"] == P.Q_LIST
        assert np.asarray(c["marks"]["count"]).shape == np.asarray(c["marks"]["bytes"]).shape == (len(P.Q_LIST), NS)
    dec = EB.EmbeddedDecoder(net, cs)
    n = C * (shape[1] // 16) * (shape[2] // 16)
    assert (dec.available() == n).all()
    with torch.no_grad():
        fw = {q: net.forward_single_quality(x, q) for q in QS}
    assert _same(dec.decode(), fw[10])
    outs = dec.decode_qualities(QS)                              # 3.3, 7 and 10 are no marks
    for q, o in zip(QS, outs):
        assert _same(o, fw[q]), q
    back = dec.decode_qualities(QS[::-1])                        # any order
    assert all(_same(a, b) for a, b in zip(back, outs[::-1]))
    # cut at the mark of 2.5: the qualities up to it decode unchanged, 7 is refused
    cut = [EB.truncate(c, q=2.5) for c in cs]
    assert all(sum(EB.container_bytes(a)) < sum(EB.container_bytes(b)) for a, b in zip(cut, cs))
    dcut = EB.EmbeddedDecoder(net, cut)
    low = [q for q in QS if q <= 2.5]
    for q, o in zip(low, dcut.decode_qualities(low)):
        assert _same(o, fw[q]), q
    k25 = P.Q_LIST.index(2.5)                                    # whole words may complete a few elements beyond the mark
    assert (dcut.available() >= np.asarray([c["marks"]["count"][k25] for c in cut])).all() and (dcut.available() < n).any()
    with pytest.raises(ValueError, match=r"quality 7.0 needs \d+ elements of slice \d+ of image \d+, its container holds \d+"):
        dcut.decode_qualities([7])
    assert dcut.bits(2.5) == [8.0 * sum(EB.container_bytes(c)) for c in cut]
    assert dec.bits(2.5) == dcut.bits(2.5) and dec.bits(0)[0] < dec.bits(0.5)[0] < dec.bits(3.3)[0] < dec.bits(10)[0]
    assert dec.bits(10)[0] <= 8.0 * sum(EB.container_bytes(cs[0]))


def test_more_than_eight_qualities_split_into_groups():
    net = _net()
    x, cs = _coded(2, 64, 128, 2)
    qs = [0.1, 9, 0.2, 0.4, 0, 0.8, 1.5, 3, 5, 6, 2.5, 8]      # 11 levels > 0: two tails
    outs = EB.EmbeddedDecoder(net, cs).decode_qualities(qs)
    with torch.no_grad():
        for q, o in zip(qs, outs):
            assert _same(o, net.forward_single_quality(x, q)), q


def test_cut_at_any_byte_and_batch_invariance():
    """Every slice of image 0 cut at a length that is no multiple of 4, each its own, one to 0 bytes and one left whole;
    image 1 cut at a mark.  The quantised residual r_hat = symbol * present + mu is elementwise, so it equals the full
    decode's where rank < available and the all-cut decode's (mu) elsewhere.  y_hat adds the LRP stack of its own slice,
    five 3x3 convolutions over r_hat of that slice, so it is compared where a whole slice is present (the full decode's)
    or absent (the all-cut decode's), and through batch invariance everywhere."""
    net = _net()
    x, cs = _coded(2, 64, 128, 2)
    n = C * 4 * 8
    lens = [len(s) for s in cs[0]["embedded"]]
    cut = [max(9, ln * (j + 1) // 12) | 1 for j, ln in enumerate(lens)]           # odd lengths, a different share per slice
    cut[4], cut[8] = 0, lens[8] + 3                                               # one slice gone, one whole
    assert all(c % 4 for c in cut[:4] + cut[5:8] + cut[9:]) and len(set(cut)) == NS
    c0 = EB.truncate(cs[0], slice_bytes=cut)
    c1 = EB.truncate(cs[1], q=0.5)
    dec = EB.EmbeddedDecoder(net, [c0, c1])
    avail = dec.available()
    r_sym, r_idx = _ranked_reference(net, x)
    tg = bs.Tables.of(net.gaussian_conditional)
    outs = [np.zeros(n, dtype=np.int32) for _ in range(2 * NS)]
    want = bs.decode_prefix_streams([(c["embedded"][j], r_idx[b, j], outs[b * NS + j]) for b, c in enumerate((c0, c1))
                                     for j in range(NS)], tg)
    assert avail.tolist() == np.asarray(want).reshape(2, NS).tolist()
    assert avail[0, 4] == 0 and avail[0, 8] == n and (avail[0] < n).sum() == NS - 1
    assert (avail[1] >= np.asarray(cs[1]["marks"]["count"][P.Q_LIST.index(0.5)])).all()
    for b in range(2):
        for j in range(NS):
            assert np.array_equal(outs[b * NS + j][:avail[b, j]], r_sym[b, j][:avail[b, j]])
    got = dec.decode()
    rq = dec.dp.tails[1].rq.buf.permute(0, 3, 1, 2).clone()                       # r_hat of the level just decoded
    full_dec = EB.EmbeddedDecoder(net, cs)
    full = full_dec.decode()
    rq_full = full_dec.dp.tails[1].rq.buf.permute(0, 3, 1, 2).clone()
    none_dec = EB.EmbeddedDecoder(net, [EB.truncate(c, slice_bytes=[0] * NS) for c in cs])
    assert (none_dec.available() == 0).all()
    none = none_dec.decode()
    rq_none = none_dec.dp.tails[1].rq.buf.permute(0, 3, 1, 2).clone()
    with torch.no_grad():
        fw10 = net.forward_single_quality(x, 10)
        assert _same(full, fw10)
        perm = torch.from_numpy(_contract_perm(fw10["std"].cpu())).long().cuda()
    rank = torch.empty_like(perm)
    rank.scatter_(2, perm, torch.arange(n, device="cuda").expand_as(perm).contiguous())     # rank of every element
    present = rank < torch.from_numpy(avail).cuda()[..., None]
    assert torch.equal(_segments(rq), torch.where(present, _segments(rq_full), _segments(rq_none)))
    ys = lambda o: o["y_hat"].reshape(2, NS, C, 4, 8)
    assert torch.equal(ys(got)[0, 8], ys(full)[0, 8]) and torch.equal(ys(got)[0, 4], ys(none)[0, 4])
    # batch invariance: each image equals its single-image decode
    for b, c in enumerate((c0, c1)):
        one = EB.EmbeddedDecoder(net, [c]).decode()
        assert torch.equal(one["x_hat"][0], got["x_hat"][b]) and torch.equal(one["y_hat"][0], got["y_hat"][b]), b


def test_sizes_marks_and_base_bytes():
    net = _net()
    x, cs = _coded(2, 64, 128, 2)
    n = C * 4 * 8
    r_sym, r_idx = _ranked_reference(net, x)
    tg = bs.Tables.of(net.gaussian_conditional)
    layered, _ = P.encode_batch(net, x, P.Q_LIST)
    with torch.no_grad():
        masks = [net.forward_single_quality(x, q)["mask"] for q in P.Q_LIST]
    for b, c in enumerate(cs):
        assert c["z"] == layered[b]["z"] and c["base"] == layered[b]["base"]
        for j, s in enumerate(c["embedded"]):
            assert s == bs.encode(r_sym[b, j], r_idx[b, j], tg)                  # ONE stream, the elements in rank order
            lo, hi = bs.stream_bytes(bs.price(r_sym[b, j], r_idx[b, j], tg).sum(), n)
            assert lo <= len(s) <= hi, (b, j)
            counts = [row[j] for row in c["marks"]["count"]]
            assert [row[j] for row in c["marks"]["bytes"]] == bs.prefix_bytes(s, r_idx[b, j], counts, tg), (b, j)
        for k in range(len(P.Q_LIST)):
            assert c["marks"]["count"][k] == _segments(masks[k])[b].sum(-1).long().tolist(), k
    one = EB.encode_batch(net, x[1:2])                                           # batch invariance of the encoder
    assert one[0] == cs[1]


def test_one_graph_per_group_size():
    net = _net()
    assert net.use_graph
    x, cs = _coded(2, 64, 128, 2)
    dec = EB.EmbeddedDecoder(net, cs)
    a = dec.decode_qualities([0.5, 2.5])
    b = dec.decode_qualities([1, 7])                      # other cuts: the same graph, another count table
    c = dec.decode()
    d = EB.EmbeddedDecoder(net, [EB.truncate(c_, q=1) for c_ in cs])      # another decoder on the same plans
    e = d.decode_qualities([1])[0]
    a2 = dec.decode_qualities([0.5, 2.5])                 # the first one again after the plans served another
    assert dec.dp is d.dp and {1, 2} <= set(dec.dp.tails)       # the plans are the model's: other tests' group sizes stay
    assert all(len(t.runner.graphs) == 1 for t in dec.dp.tails.values())
    with torch.no_grad():
        for o, q in zip(a + b + [c, e] + a2, [0.5, 2.5, 1, 7, 10, 1, 0.5, 2.5]):
            assert _same(o, net.forward_single_quality(x, q)), q


def test_refusals(monkeypatch):
    x = _x(1, 64, 64)
    _, cs = _coded(2, 64, 128, 2)
    with pytest.raises(NotImplementedError, match="eager harness"):
        EB.encode_batch(_net("rem"), x)
    with pytest.raises(NotImplementedError, match="eager harness"):
        EB.EmbeddedDecoder(_net("rem"), cs)
    for over in (dict(all_scalable=False), dict(delta_encode=False)):
        with pytest.raises(NotImplementedError, match="all_scalable=True"):
            EB.encode_batch(_net(**over), x)
        with pytest.raises(NotImplementedError, match="all_scalable=True"):
            EB.EmbeddedDecoder(_net(**over), cs)
    net = _net()
    with pytest.raises(ValueError, match="non-decreasing"):
        EB.encode_batch(net, x, marks=[1, 0.5])
    with pytest.raises(ValueError, match="qualities"):
        EB.encode_batch(net, x, marks=[0.1] * 33)
    with pytest.raises(NotImplementedError, match="up to 262144"):
        EB.encode_batch(net, torch.zeros((1, 3, 1024, 2112), device="cuda"))
    layered, _ = P.encode_batch(net, x, [0.5, 1])
    with pytest.raises(ValueError, match="embedded container"):
        EB.EmbeddedDecoder(net, layered)
    with pytest.raises(ValueError, match="same shape"):
        EB.EmbeddedDecoder(net, cs[:1] + EB.encode_batch(net, x))
    with pytest.raises(ValueError, match="finite and >= 0"):
        EB.EmbeddedDecoder(net, cs).decode_qualities([-1])
    monkeypatch.setattr(sys.modules["vampic.models"], "MAX_PLAN_PIXELS", 64 * 128)      # one image per plan
    with pytest.raises(NotImplementedError, match="smaller batches"):
        EB.encode_batch(net, _x(2, 64, 128, seed=2))
    with pytest.raises(NotImplementedError, match="smaller batches"):
        EB.EmbeddedDecoder(net, cs)
    monkeypatch.undo()
    monkeypatch.setattr(net, "storage", "bf16")
    with pytest.raises(NotImplementedError, match="bf16 storage"):
        EB.encode_batch(net, x)
    with pytest.raises(NotImplementedError, match="bf16 storage"):
        EB.EmbeddedDecoder(net, cs)
    monkeypatch.setattr(net, "storage", "fp32")
    monkeypatch.setattr(ops, "f16x2_mode", lambda: True)
    with pytest.raises(NotImplementedError, match="f16x2"):
        EB.encode_batch(net, x)
    with pytest.raises(NotImplementedError, match="f16x2"):
        EB.EmbeddedDecoder(net, cs)


def test_embedded_rd():
    net = _net()
    imgs = [synth.synth_image(1, 50, 100, seed=s).cuda() for s in (11, 12)]
    qs = [0.05, 0.5, 3.3, 10]
    rows = EV.embedded_rd(net, imgs, qs)
    assert [r["q"] for r in rows] == [0.0] + qs
    xp, unpad = EV.pad_image(torch.cat(imgs, 0))
    dec = EB.EmbeddedDecoder(net, EB.encode_batch(net, xp))
    for r, o in zip(rows, dec.decode_qualities([0.0] + qs)):
        out = torch.nn.functional.pad(o["x_hat"], unpad)
        bits = dec.bits(r["q"])
        for i, x in enumerate(imgs):
            assert r["bpp_all"][i] == bits[i] / (50 * 100)
            # compute_psnr's float64 sum is accumulated with atomics (order unspecified): equal to the last few ulps
            assert abs(r["psnr_all"][i] - EV.compute_psnr(x, out[i:i + 1])) <= 1e-9
        assert r["enc_s"] > 0 and r["dec_s"] > 0
    assert all(b["bpp"] > a["bpp"] for a, b in zip(rows, rows[1:]))
